"""The committee table (mbls_committees_*): mbls_fast_aggregate_verify_batch_committee_msgtable_device -- a committee id and a bitfield per item, the key sum on the
direct or the complement route -- against the entry it has to equal, mbls_fast_aggregate_verify_batch_indexed_msgtable_device on the same items with the signers
spelled out through a ragged offset table, measured in the same process on the same items. Shapes: 2^16 items over 512 committees of 128 members at 100, 99, 90,
55, 50, 45 and 25 % participation; 2^16 items over one 512-member committee at 99 %; and the append of 2 048 committees of 128. Device-resident inputs, 512
messages in a resident table.
Same timing method for every variant: a host clock around a window of repetitions that ends in a device synchronise, every shape warmed up, the variants alternated
inside every round, medians over the rounds with [min, max] beside them. Every result is checked: every 16th item (i % 16 == 7) has one bit flipped against its
signers and must be rejected by every variant, every other item accepted.
The output also carries `bench_vs_parent`: the ms_per_step of bench.py runs of the parent commit and of this tree, read from the two files of bench.py result
lines beside the output (bench_committee_parent.jsonl, bench_committee_this_tree.jsonl: one `bench.py --gpus 1 --steps 20 --warmup 5` line per run, taken
alternately); the block is left out where those files are absent.
usage: python scripts/committee_throughput.py [OUT.json]   (default: profiles/committee_throughput.json; CTT_ROUNDS, default 10; CTT_ITEMS, default 65536)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "committee_throughput.json")
ROUNDS = int(os.environ.get("CTT_ROUNDS", "10"))
NI = int(os.environ.get("CTT_ITEMS", "65536"))
WINDOW_S = 0.2
N_MSGS = 512
ctx = N.default_context()
P = lambda t: t.data_ptr()
pool = bench.make_pool(bench.SEED)
POOL = len(pool)
limbs = np.array([[(sk >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for sk in pool], dtype=np.uint64)
d_pool_sk = torch.from_numpy(np.frombuffer(b"".join(s.to_bytes(32, "big") for s in pool), dtype=np.uint8).reshape(POOL, 32).copy()).to(dev)
d_pool_pk = torch.empty((POOL, 96), dtype=torch.uint8, device=dev)
ctx.check(lib.mbls_sk_to_pk_batch_device(ctx.handle, P(d_pool_sk), N.PK_UNCOMPRESSED, POOL, P(d_pool_pk), None))
table = N.KeyTable(ctx, capacity_hint=POOL)
d_errs = torch.zeros(POOL, dtype=torch.uint8, device=dev)
table.append_device(P(d_pool_pk), POOL, P(d_errs), pk_format=N.PK_UNCOMPRESSED, validate=False)
torch.cuda.synchronize(); assert int(d_errs.max().item()) == 0
rng0 = np.random.default_rng(5)
d_list = torch.from_numpy(rng0.integers(0, 256, size=(N_MSGS, 32), dtype=np.uint8)).to(dev)
mt = N.MsgTable(ctx, capacity_hint=N_MSGS)
assert mt.append_device(P(d_list), N_MSGS, msg_len=32) == 0
torch.cuda.synchronize()


def window(f, reps, d_res):
    d_res.fill_(7)
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def stat(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def measure(variants, d_res, expect, tag):
    reps, times = {}, {}
    for name, f in variants:
        window(f, 1, d_res)
        est = window(f, 1, d_res)
        assert bool((d_res == expect).all()), (tag, name)
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
        times[name] = []
    for _ in range(ROUNDS):
        for name, f in variants:
            times[name].append(1e3 * window(f, reps[name], d_res))
            assert bool((d_res == expect).all()), (tag, name)
    return {name: dict(stat(times[name]), reps_per_window=reps[name]) for name, _ in variants}


def committees_of(count, m, seed):
    """count committees of m distinct pool keys each (an odd stride from a random start)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, POOL, size=count, dtype=np.int64)
    s = rng.integers(0, POOL // 2, size=count, dtype=np.int64) * 2 + 1
    return (a[:, None] + np.arange(m, dtype=np.int64)[None, :] * s[:, None]) % POOL


def items_of(members, percent, seed):
    """per item a committee, the signers' mask (exactly round(m percent / 100) signers), the aggregate secret key of the signers, and the bitfield: the signers', with
    one bit flipped in every 16th item"""
    count, m = members.shape
    rng = np.random.default_rng(seed)
    cid = rng.integers(0, count, size=NI, dtype=np.int64)
    s = max(1, int(round(m * percent / 100.0)))
    order = np.argsort(rng.random((NI, m)), axis=1)
    signed = np.zeros((NI, m), dtype=bool)
    np.put_along_axis(signed, order[:, :s], True, axis=1)
    sk = np.zeros((NI, 32), dtype=np.uint8)
    for c0 in range(0, NI, 2048):
        agg = (limbs[members[cid[c0:c0 + 2048]]] * signed[c0:c0 + 2048, :, None]).sum(axis=1)
        for i in range(agg.shape[0]):
            v = sum(int(agg[i, j]) << (32 * j) for j in range(8)) % bench.R
            sk[c0 + i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    named = signed.copy()
    flip = np.arange(7, NI, 16)
    pos = rng.integers(0, m, size=flip.size)
    named[flip, pos] ^= True
    expect = np.ones(NI, dtype=np.uint8); expect[flip] = 0
    bits = np.packbits(named, axis=1, bitorder="little")            # SSZ bit order: member j is bit j & 7 of byte j >> 3
    stride = (bits.shape[1] + 3) // 4 * 4
    if stride != bits.shape[1]:
        bits = np.concatenate([bits, np.zeros((NI, stride - bits.shape[1]), dtype=np.uint8)], axis=1)
    lists = members[cid][named]                                      # row-major: every item's named members in member order
    off = np.concatenate([[0], np.cumsum(named.sum(axis=1))])
    return cid, sk, bits, stride, lists, off, expect, s


out = {"form": "device-resident inputs, %d 32-byte messages in a resident table; item i %% 16 == 7 has one bit flipped against its signers (rejected), the others are valid; "
               "items = %d" % (N_MSGS, NI),
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition; median [min, max] over the rounds",
       "baseline": "mbls_fast_aggregate_verify_batch_indexed_msgtable_device on the same items, signers spelled out through a ragged offset table",
       "round_items": int(ctx.limits().round_items), "shapes": {}, "append": {}}
ctx.reserve(N.plan_workspace_items(NI, 0, False, ctx.limits())); ctx.reserve_committee_items(NI, 512)
d_res = torch.full((NI,), 7, dtype=torch.uint8, device=dev)
rng = np.random.default_rng(9)
midx = rng.integers(0, N_MSGS, size=NI, dtype=np.int64)
d_midx = torch.from_numpy(midx.astype(np.int32)).to(dev)
d_signed_msgs = d_list[torch.from_numpy(midx).to(dev)].contiguous()
SHAPES = [(128, 512, p) for p in (100, 99, 90, 55, 50, 45, 25)] + [(512, 1, 99)]
tables = {}
for m, count, percent in SHAPES:
    if (m, count) not in tables:
        members = committees_of(count, m, 31 + m)
        ct = N.CommitteeTable(table, capacity_hint=count)
        assert ct.append(members.reshape(-1).tolist(), list(range(0, count * m + 1, m))) == 0
        tables[(m, count)] = (members, ct)
    members, ct = tables[(m, count)]
    cid, sk, bits, stride, lists, off, expect_h, s = items_of(members, percent, 100 * m + percent)
    d_sk = torch.from_numpy(sk).to(dev)
    d_sigs = torch.empty((NI, 96), dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_signed_msgs), 32, NI, P(d_sigs), None))
    d_cid = torch.from_numpy(cid.astype(np.int32)).to(dev); d_bits = torch.from_numpy(bits).to(dev)
    d_keys = torch.from_numpy(lists.astype(np.uint32).view(np.int32)).to(dev); d_off = torch.from_numpy(off.astype(np.uint32).view(np.int32)).to(dev)
    expect = torch.from_numpy(expect_h).to(dev)
    torch.cuda.synchronize()
    base = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_msgtable_device(ctx.handle, table.handle, P(d_sigs), mt.handle, P(d_midx), P(d_keys), P(d_off), NI, 0,
                                                                                          P(d_res), None, None, None))
    cmt = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_committee_msgtable_device(ctx.handle, ct.handle, P(d_sigs), mt.handle, P(d_midx), P(d_cid), P(d_bits), stride, NI,
                                                                                           P(d_res), None, None, None))
    route = "complement" if N.plan_committee_route(m, s) else "direct"
    row = {"items": NI, "members": m, "committees": count, "participation_percent": percent, "signers": s, "route": route, "rejected_items": int((expect_h == 0).sum()),
           "input_bytes_per_item": {"committee": 4 + stride, "indexed": 4 * s + 4}}
    variants = [("committee", cmt), ("indexed", base)]
    if route == "complement":                                       # the same entry held on the direct route: what k_cmt_expand costs on its own
        def direct():
            ctx.set_committee_route(N.CMT_ROUTE_DIRECT); cmt(); ctx.set_committee_route(N.CMT_ROUTE_AUTO)
        variants.append(("committee_forced_direct", direct))
    row.update(measure(variants, d_res, expect, (m, percent)))
    row["saved_vs_indexed_ms"] = round(row["indexed"]["ms_median"] - row["committee"]["ms_median"], 4)
    row["indexed_spread_ms"] = round(row["indexed"]["ms_max"] - row["indexed"]["ms_min"], 4)
    row["faster_beyond_indexed_spread"] = bool(row["saved_vs_indexed_ms"] > row["indexed_spread_ms"])
    row["slower_beyond_indexed_spread"] = bool(-row["saved_vs_indexed_ms"] > row["indexed_spread_ms"])
    out["shapes"]["%d_members/%d_percent" % (m, percent)] = row
    print("%4d members %3d %%  %-10s  committee %8.3f ms [%.3f, %.3f]   indexed %8.3f ms [%.3f, %.3f]   saved %7.3f ms (spread %.3f)" % (
        m, percent, route, row["committee"]["ms_median"], row["committee"]["ms_min"], row["committee"]["ms_max"], row["indexed"]["ms_median"], row["indexed"]["ms_min"],
        row["indexed"]["ms_max"], row["saved_vs_indexed_ms"], row["indexed_spread_ms"]), flush=True)
    with open(OUT, "w") as fh:                                      # (kept current shape by shape)
        json.dump(out, fh, indent=1); fh.write("\n")
for _, ct in tables.values():
    ct.close()

# ---- the append itself: 2 048 committees of 128 into an empty table of sufficient capacity (host memory in, records on the device; clear is outside the clock)
count, m = 2048, 128
members = committees_of(count, m, 77)
flat = (N.C.c_uint32 * (count * m))(*members.reshape(-1).tolist()); offs = (N.C.c_uint32 * (count + 1))(*range(0, count * m + 1, m))
ct = N.CommitteeTable(table, capacity_hint=count)
ts = []
first = N.C.c_uint64(0)
for r in range(ROUNDS + 2):
    ct.clear()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    ctx.check(lib.mbls_committees_append(ct.handle, flat, offs, count, N.C.byref(first)))
    torch.cuda.synchronize()
    if r >= 2:
        ts.append(1e3 * (time.perf_counter() - t0))
assert len(ct) == count and ct.get(count - 1)[1:] == (m, True)
ct.close()
out["append"]["%d_committees_of_%d" % (count, m)] = dict(stat(ts), committees=count, members=m)
print("append of %d committees of %d   %8.3f ms [%.3f, %.3f]" % (count, m, statistics.median(ts), min(ts), max(ts)), flush=True)
mt.close(); table.close()
# ---- bench.py against the parent commit: the result lines of the alternated runs, where they lie beside the output
lines = {}
for who in ("parent", "this_tree"):
    path = os.path.join(os.path.dirname(os.path.abspath(OUT)), "bench_committee_%s.jsonl" % who)
    if os.path.exists(path):
        with open(path) as fh:
            lines[who] = [round(json.loads(l)["ms_per_step"], 4) for l in fh if l.strip()]
if len(lines) == 2:
    out["bench_vs_parent"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5 of the parent commit and of this tree, alternated (full lines: bench_committee_parent.jsonl, "
                                      "bench_committee_this_tree.jsonl beside this file)",
                              "parent_ms_per_step": lines["parent"], "this_tree_ms_per_step": lines["this_tree"]}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
