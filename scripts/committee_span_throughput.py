"""fast_aggregate_verify over committee spans (mbls_fast_aggregate_verify_batch_committee_span_msgtable_device: up to 64 committee ids and ONE concatenated bitfield
per item; keys and messages resident) against the entry it has to equal, mbls_fast_aggregate_verify_batch_indexed_msgtable_device on the same items with the signers
spelled out through a ragged offset table, measured in the same process on the same items. Shapes: 4 096 items x 64 committees of 128 members at 100, 99, 90, 55
and 45 % participation (every segment has exactly round(128 p / 100) signers: 55 % goes complement, 45 % direct); 2^14 items x 4 committees of 128 at 99 %; and
2^16 items x a span of ONE 128-member committee at 99 %, there also against mbls_fast_aggregate_verify_batch_committee_msgtable_device -- the price of the general
path. Device-resident inputs.
Every 16th item (i % 16 == 7) has one bit flipped against its signers and must be rejected, every other item must be accepted: every result of every window is
checked. Same timing method for every variant: a host clock around a window of repetitions that ends in a device synchronise, every shape warmed up, the variants
alternated inside every round, medians over the rounds with [min, max] beside them.
The output also carries `bench_vs_parent`: the ms_per_step of bench.py runs of the parent commit and of this tree, read from the two files of bench.py result
lines beside the output (bench_committee_span_parent.jsonl, bench_committee_span_this_tree.jsonl: one `bench.py --gpus 1 --steps 20 --warmup 5` line per run, taken
alternately); the block is left out where those files are absent.
usage: python scripts/committee_span_throughput.py [OUT.json]   (default: profiles/committee_span_throughput.json; CST_ROUNDS, default 10)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "committee_span_throughput.json")
ROUNDS = int(os.environ.get("CST_ROUNDS", "10"))
WINDOW_S = 0.2
M_MEMBERS, COMMITTEES, ENTRIES = 128, 512, 512
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
# the committees: COMMITTEES x M_MEMBERS distinct pool keys each (an odd stride from a random start)
rng0 = np.random.default_rng(7549)
members = ((rng0.integers(0, POOL, size=COMMITTEES)[:, None] + np.arange(M_MEMBERS)[None, :] * (rng0.integers(0, POOL // 2, size=COMMITTEES) * 2 + 1)[:, None]) % POOL).astype(np.int32)
ct = N.CommitteeTable(table, capacity_hint=COMMITTEES)
assert ct.append(members.reshape(-1).tolist(), list(range(0, COMMITTEES * M_MEMBERS + 1, M_MEMBERS))) == 0
d_list = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(ENTRIES, 32), dtype=np.uint8)).to(dev)
mt = N.MsgTable(ctx, capacity_hint=ENTRIES)
assert mt.append_device(P(d_list), ENTRIES, msg_len=32) == 0


def window(f, reps, clear):
    clear()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def stat(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def measure(variants, clear, good, tag):
    reps, times = {}, {}
    for name, f in variants:
        window(f, 1, clear)
        est = window(f, 1, clear)
        assert good(), (tag, name)
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
        times[name] = []
    for _ in range(ROUNDS):
        for name, f in variants:
            times[name].append(1e3 * window(f, reps[name], clear))
            assert good(), (tag, name)
    return {name: dict(stat(times[name]), reps_per_window=reps[name]) for name, _ in variants}


def items_of(n, q, percent, seed):
    """n items of q committees each, exactly round(128 percent / 100) signers per segment; every 16th item with one bit flipped against its signers"""
    m = M_MEMBERS
    rng = np.random.default_rng(seed)
    cid = rng.integers(0, COMMITTEES, size=(n, q), dtype=np.int64)
    s = max(1, int(round(m * percent / 100.0)))
    order = np.argsort(rng.random((n, q, m)), axis=2)
    signed = np.zeros((n, q, m), dtype=bool)
    np.put_along_axis(signed, order[:, :, :s], True, axis=2)
    signed = signed.reshape(n, q * m)
    keys = members[cid].reshape(n, q * m)
    sk = np.zeros((n, 32), dtype=np.uint8)
    step = max(1, (1 << 18) // (q * m))
    for c0 in range(0, n, step):
        agg = (limbs[keys[c0:c0 + step]] * signed[c0:c0 + step, :, None]).sum(axis=1)
        for i in range(agg.shape[0]):
            v = sum(int(agg[i, j]) << (32 * j) for j in range(8)) % bench.R
            sk[c0 + i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    named = signed.copy()
    flip = np.arange(7, n, 16)
    named[flip, rng.integers(0, q * m, size=flip.size)] ^= True
    expect = np.ones(n, dtype=np.uint8); expect[flip] = 0
    bits_c = np.packbits(named, axis=1, bitorder="little")              # SSZ bit order: position p is bit p & 7 of byte p >> 3
    stride = (bits_c.shape[1] + 3) // 4 * 4
    bits = np.zeros((n, stride), dtype=np.uint8); bits[:, :bits_c.shape[1]] = bits_c
    off = np.concatenate([[0], np.cumsum(named.sum(axis=1))])
    return {"cid": cid, "sk": sk, "expect": expect, "signers_per_segment": s, "bits": bits, "stride": stride, "lists": keys[named], "off": off}


out = {"form": "device-resident inputs, keys and 32-byte messages resident; every 16th item has one bit flipped against its signers and must be rejected",
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition; median [min, max] over the rounds",
       "baseline": "mbls_fast_aggregate_verify_batch_indexed_msgtable_device on the same items, signers spelled out through a ragged offset table",
       "round_items": int(ctx.limits().round_items), "members_per_committee": M_MEMBERS, "committees_in_table": COMMITTEES, "table_entries": ENTRIES, "shapes": {}}
SHAPES = [("4096_items/64_committees/%d_percent" % p, 4096, 64, p) for p in (100, 99, 90, 55, 45)] + [("16384_items/4_committees/99_percent", 16384, 4, 99),
                                                                                                      ("65536_items/1_committee/99_percent", 65536, 1, 99)]
for name, n, q, percent in SHAPES:
    S = items_of(n, q, percent, 1000 * q + percent)
    rng = np.random.default_rng(9 + n)
    midx = rng.integers(0, ENTRIES, size=n, dtype=np.int64)
    d_midx = torch.from_numpy(midx.astype(np.int32)).to(dev)
    d_signed_msgs = d_list[torch.from_numpy(midx).to(dev)].contiguous()
    d_sk = torch.from_numpy(S["sk"]).to(dev)
    d_sigs = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_signed_msgs), 32, n, P(d_sigs), None))
    d_ids = torch.from_numpy(S["cid"].reshape(-1).astype(np.int32)).to(dev)
    d_soff = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * q).astype(np.int32)).to(dev)
    d_bits = torch.from_numpy(S["bits"]).to(dev); stride = S["stride"]
    d_keys = torch.from_numpy(S["lists"].astype(np.int32)).to(dev); d_off = torch.from_numpy(S["off"].astype(np.uint32).view(np.int32)).to(dev)
    d_res = torch.zeros(n, dtype=torch.uint8, device=dev)
    expect = torch.from_numpy(S["expect"]).to(dev)
    torch.cuda.synchronize()
    span = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_committee_span_msgtable_device(ctx.handle, ct.handle, P(d_sigs), mt.handle, P(d_midx), P(d_ids), n * q, P(d_soff),
                                                                                                  P(d_bits), stride, n, P(d_res), None, None, None))
    base = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_msgtable_device(ctx.handle, table.handle, P(d_sigs), mt.handle, P(d_midx), P(d_keys), P(d_off), n, 0,
                                                                                          P(d_res), None, None, None))
    good = lambda: bool((d_res == expect).all())
    clear = lambda: d_res.fill_(7)
    variants = [("span", span), ("indexed", base)]
    if q == 1:
        one = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_committee_msgtable_device(ctx.handle, ct.handle, P(d_sigs), mt.handle, P(d_midx), P(d_ids), P(d_bits), stride, n,
                                                                                               P(d_res), None, None, None))
        variants.append(("committee", one))
    r = measure(variants, clear, good, name)
    route = "complement" if N.plan_committee_route(M_MEMBERS, S["signers_per_segment"]) else "direct"
    row = dict(r, items=n, committees_per_item=q, participation_percent=percent, signers_per_segment=S["signers_per_segment"], route=route,
               flipped_items=int((S["expect"] == 0).sum()), bits_stride=stride,
               input_bytes_per_item={"span": 4 * q + 4 + stride, "indexed": round(4.0 * S["lists"].size / n + 4, 1)},
               span_scratch_bytes_per_item=4 * min(8 * stride, 64 * M_MEMBERS) + 164)
    row["saved_vs_indexed_ms"] = round(r["indexed"]["ms_median"] - r["span"]["ms_median"], 4)
    row["indexed_spread_ms"] = round(r["indexed"]["ms_max"] - r["indexed"]["ms_min"], 4)
    if q == 1:
        row["price_vs_committee_ms"] = round(r["span"]["ms_median"] - r["committee"]["ms_median"], 4)
    out["shapes"][name] = row
    print("%-40s %-10s  span %9.3f ms [%.3f, %.3f]   indexed %9.3f ms [%.3f, %.3f]%s" % (
        name, route, r["span"]["ms_median"], r["span"]["ms_min"], r["span"]["ms_max"], r["indexed"]["ms_median"], r["indexed"]["ms_min"], r["indexed"]["ms_max"],
        "   committee %9.3f ms [%.3f, %.3f]" % (r["committee"]["ms_median"], r["committee"]["ms_min"], r["committee"]["ms_max"]) if q == 1 else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:                                      # (kept current shape by shape)
        json.dump(out, fh, indent=1); fh.write("\n")
ct.close(); mt.close(); table.close()
# ---- bench.py against the parent commit: the result lines of the alternated runs, where they lie beside the output
lines = {}
for who in ("parent", "this_tree"):
    path = os.path.join(os.path.dirname(os.path.abspath(OUT)), "bench_committee_span_%s.jsonl" % who)
    if os.path.exists(path):
        with open(path) as fh:
            lines[who] = [round(json.loads(l)["ms_per_step"], 4) for l in fh if l.strip()]
if len(lines) == 2:
    out["bench_vs_parent"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5 of the parent commit and of this tree, alternated (full lines: bench_committee_span_parent.jsonl, "
                                      "bench_committee_span_this_tree.jsonl beside this file)",
                              "parent_ms_per_step": lines["parent"], "this_tree_ms_per_step": lines["this_tree"]}
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
