"""verify_multiple over committee spans (mbls_verify_multiple_committee_span_msgtable[_locate]_device: per set up to 64 committee ids and ONE concatenated bitfield,
or one key index; keys and messages resident) against the entry it has to equal, mbls_verify_multiple_sets_indexed_msgtable[_locate]_device on the same sets with
the signers spelled out through a ragged offset table, measured in the same process on the same sets. Every shape runs with the split factor of the key phase
(mbls_ctx_set_vm_span_split) forced to 1, 2, 4, 8 and 16 and on auto. Shapes:
  a block        8 span sets of 64 x 128 members, one set over a 512-member committee, 3 single-key sets, at 100, 99, 90, 55 and 45 % participation
  a sync range   64 such blocks in one call (768 sets), at 99 and 45 %
  4 096 span sets at 99 % (the throughput end) and at 45 %
  the block at 99 % with one flipped bit through the _locate entry
Every segment has exactly round(m p / 100) signers (55 % goes complement, 45 % direct). Device-resident inputs. Every result of every window is checked: the call's
byte and status word (1 and 0; with the flipped bit 0 and 0, the set bytes 0 at that set and 1 elsewhere). Same timing method for every variant: a host clock around
a window of repetitions that ends in a device synchronise, every variant warmed up, the variants alternated inside every round, medians over the rounds with
[min, max] beside them.
The output also carries `bench_vs_parent`: the ms_per_step of bench.py runs of the parent commit and of this tree, read from the two files of bench.py result lines
beside the output (bench_vm_committee_span_parent.jsonl, bench_vm_committee_span_this_tree.jsonl, taken alternately); left out where those files are absent.
usage: python scripts/vm_committee_span_throughput.py [OUT.json]   (default: profiles/vm_committee_span_throughput.json; VCST_ROUNDS, default 10)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_committee_span_throughput.json")
ROUNDS = int(os.environ.get("VCST_ROUNDS", "10"))
WINDOW_S = 0.2
M_MEMBERS, COMMITTEES, SYNC_MEMBERS, ENTRIES, Q = 128, 512, 512, 512, 64
WIDTH = Q * M_MEMBERS                                               # key slots per set: 8 192
STRIDE = WIDTH // 8                                                 # bytes per field: 1 024
SINGLE = N.VM_SET_SINGLE_KEY
SPLITS = (1, 2, 4, 8, 16)
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
# the committees: COMMITTEES x M_MEMBERS distinct pool keys each (an odd stride from a random start), and behind them the sync committee of SYNC_MEMBERS keys
rng0 = np.random.default_rng(7549)
members = ((rng0.integers(0, POOL, size=COMMITTEES)[:, None] + np.arange(M_MEMBERS)[None, :] * (rng0.integers(0, POOL // 2, size=COMMITTEES) * 2 + 1)[:, None]) % POOL).astype(np.int64)
sync = ((int(rng0.integers(0, POOL)) + np.arange(SYNC_MEMBERS) * 3) % POOL).astype(np.int64)
assert POOL >= 3 * SYNC_MEMBERS or len(set(sync.tolist())) == SYNC_MEMBERS
SYNC_ID = COMMITTEES
ct = N.CommitteeTable(table, capacity_hint=COMMITTEES + 1)
assert ct.append(members.reshape(-1).tolist() + sync.tolist(), list(range(0, COMMITTEES * M_MEMBERS + 1, M_MEMBERS)) + [COMMITTEES * M_MEMBERS + SYNC_MEMBERS]) == 0
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


def sets_of(kinds, percent, seed, flip_set=None):
    """kinds: one of "span", "sync", "single" per set -> the id arrays, the fields, the spelled-out lists and the aggregate secret key of every set. A span set has
    exactly round(128 percent / 100) signers in each of its 64 segments, the sync set round(512 percent / 100); flip_set: one bit of that set flipped against them."""
    n = len(kinds)
    rng = np.random.default_rng(seed)
    keys = np.zeros((n, WIDTH), dtype=np.int64)
    signed = np.zeros((n, WIDTH), dtype=bool)
    ids, off = [], [0]
    for i, kind in enumerate(kinds):
        if kind == "span":
            cid = rng.integers(0, COMMITTEES, size=Q)
            keys[i] = members[cid].reshape(-1)
            s = max(1, int(round(M_MEMBERS * percent / 100.0)))
            order = np.argsort(rng.random((Q, M_MEMBERS)), axis=1)
            seg = np.zeros((Q, M_MEMBERS), dtype=bool)
            np.put_along_axis(seg, order[:, :s], True, axis=1)
            signed[i] = seg.reshape(-1)
            ids += cid.tolist()
        elif kind == "sync":
            keys[i, :SYNC_MEMBERS] = sync
            s = max(1, int(round(SYNC_MEMBERS * percent / 100.0)))
            signed[i, rng.permutation(SYNC_MEMBERS)[:s]] = True
            ids.append(SYNC_ID)
        else:
            k = int(rng.integers(0, POOL))
            keys[i, 0] = k; signed[i, 0] = True
            ids.append(SINGLE | k)
        off.append(len(ids))
    sk = np.zeros((n, 32), dtype=np.uint8)
    step = max(1, (1 << 18) // WIDTH)
    for c0 in range(0, n, step):
        agg = (limbs[keys[c0:c0 + step]] * signed[c0:c0 + step, :, None]).sum(axis=1)
        for i in range(agg.shape[0]):
            v = sum(int(agg[i, j]) << (32 * j) for j in range(8)) % bench.R
            sk[c0 + i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    named = signed.copy()
    if flip_set is not None:
        named[flip_set, int(rng.integers(0, WIDTH))] ^= True
    bits = np.packbits(named, axis=1, bitorder="little")                # SSZ bit order: position p is bit p & 7 of byte p >> 3
    for i, kind in enumerate(kinds):
        if kind == "single":
            bits[i] = 0xA5                                              # not read
    loff = np.concatenate([[0], np.cumsum(named.sum(axis=1))])
    return {"ids": np.array(ids, dtype=np.uint32), "off": np.array(off, dtype=np.uint32), "sk": sk, "bits": bits, "lists": keys[named], "loff": loff}


BLOCK = ["span"] * 8 + ["sync"] + ["single"] * 3
out = {"form": "device-resident inputs, keys and 32-byte messages resident, one blinding scalar per set; every call's byte and status word checked in every window",
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition; median [min, max] over the rounds",
       "baseline": "mbls_verify_multiple_sets_indexed_msgtable[_locate]_device on the same sets, signers spelled out through a ragged offset table",
       "round_items": int(ctx.limits().round_items), "members_per_committee": M_MEMBERS, "sync_committee_members": SYNC_MEMBERS, "committees_in_table": COMMITTEES + 1,
       "table_entries": ENTRIES, "bits_stride": STRIDE, "region_words": WIDTH, "shapes": {}}
SHAPES = [("block/%d_percent" % p, BLOCK, p, False) for p in (100, 99, 90, 55, 45)]
SHAPES += [("sync_range_64_blocks/%d_percent" % p, BLOCK * 64, p, False) for p in (99, 45)]
SHAPES += [("4096_span_sets/%d_percent" % p, ["span"] * 4096, p, False) for p in (99, 45)] + [("block/99_percent/one_flipped_bit/locate", BLOCK, 99, True)]
for name, kinds, percent, locate in SHAPES:
    n = len(kinds)
    flip = 5 if locate else None
    S = sets_of(kinds, percent, 1000 * n + percent, flip)
    rng = np.random.default_rng(9 + n)
    midx = rng.integers(0, ENTRIES, size=n, dtype=np.int64)
    d_midx = torch.from_numpy(midx.astype(np.int32)).to(dev)
    d_signed_msgs = d_list[torch.from_numpy(midx).to(dev)].contiguous()
    d_sk = torch.from_numpy(S["sk"]).to(dev)
    d_sigs = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_signed_msgs), 32, n, P(d_sigs), None))
    d_rands = torch.from_numpy(rng.integers(1, 1 << 62, size=n, dtype=np.int64)).to(dev)
    d_ids = torch.from_numpy(S["ids"].view(np.int32)).to(dev); d_soff = torch.from_numpy(S["off"].view(np.int32)).to(dev)
    d_bits = torch.from_numpy(S["bits"]).to(dev)
    d_keys = torch.from_numpy(S["lists"].astype(np.int32)).to(dev); d_off = torch.from_numpy(S["loff"].astype(np.uint32).view(np.int32)).to(dev)
    d_res = torch.zeros(1, dtype=torch.uint8, device=dev); d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    d_sres = torch.zeros(n, dtype=torch.uint8, device=dev)
    want_sets = torch.ones(n, dtype=torch.uint8, device=dev)
    if locate:
        want_sets[flip] = 0
    torch.cuda.synchronize()
    n_ids = int(S["ids"].size)
    if locate:
        span = lambda: ctx.check(lib.mbls_verify_multiple_committee_span_msgtable_locate_device(ctx.handle, ct.handle, P(d_sigs), P(d_ids), n_ids, P(d_soff), P(d_bits), STRIDE,
                                                                                                  mt.handle, P(d_midx), P(d_rands), n, P(d_res), P(d_st), P(d_sres), None, None))
        base = lambda: ctx.check(lib.mbls_verify_multiple_sets_indexed_msgtable_locate_device(ctx.handle, table.handle, P(d_sigs), P(d_keys), P(d_off), 0, mt.handle, P(d_midx),
                                                                                              P(d_rands), n, P(d_res), P(d_st), P(d_sres), None, None))
        good = lambda: int(d_res.item()) == 0 and int(d_st.item()) == 0 and bool((d_sres == want_sets).all())
    else:
        span = lambda: ctx.check(lib.mbls_verify_multiple_committee_span_msgtable_device(ctx.handle, ct.handle, P(d_sigs), P(d_ids), n_ids, P(d_soff), P(d_bits), STRIDE, mt.handle,
                                                                                         P(d_midx), P(d_rands), n, P(d_res), P(d_st), None))
        base = lambda: ctx.check(lib.mbls_verify_multiple_sets_indexed_msgtable_device(ctx.handle, table.handle, P(d_sigs), P(d_keys), P(d_off), 0, mt.handle, P(d_midx), P(d_rands),
                                                                                       n, P(d_res), P(d_st), None))
        good = lambda: int(d_res.item()) == 1 and int(d_st.item()) == 0

    def clear():
        d_res.fill_(7); d_st.fill_(7); d_sres.fill_(7)

    def with_split(mode):
        def f():
            ctx.check(lib.mbls_ctx_set_vm_span_split(ctx.handle, mode))
            span()
        return f
    splits = [p for p in SPLITS if N.plan_verify_multiple_committee_span(n, ENTRIES, WIDTH, locate, p, ctx.limits())[0] == p]      # (a factor that 2 P n <= round halves is not a variant)
    variants = [("indexed", base)] + [("split_%d" % p, with_split(p)) for p in splits] + [("auto", with_split(0))]
    r = measure(variants, clear, good, name)
    ctx.check(lib.mbls_ctx_set_vm_span_split(ctx.handle, 0))
    auto_p, ws_items = N.plan_verify_multiple_committee_span(n, ENTRIES, WIDTH, locate, 0, ctx.limits())
    p1 = r["split_1"]
    row = dict(r, sets=n, kinds={k: kinds.count(k) for k in ("span", "sync", "single")}, participation_percent=percent, locate=locate,
               route="complement" if N.plan_committee_route(M_MEMBERS, max(1, int(round(M_MEMBERS * percent / 100.0)))) else "direct",
               auto_split=auto_p, auto_workspace_items=ws_items,
               input_bytes_per_set={"span": round((4.0 * n_ids + 4 * (n + 1)) / n + STRIDE, 1), "indexed": round(4.0 * S["lists"].size / n + 4, 1)})
    row["split_1_spread_ms"] = round(p1["ms_max"] - p1["ms_min"], 4)
    row["auto_minus_split_1_ms"] = round(r["auto"]["ms_median"] - p1["ms_median"], 4)
    row["auto_slower_than_split_1_beyond_its_spread"] = bool(row["auto_minus_split_1_ms"] > row["split_1_spread_ms"])
    row["auto_minus_indexed_ms"] = round(r["auto"]["ms_median"] - r["indexed"]["ms_median"], 4)
    row["best_split"] = min(splits, key=lambda p: r["split_%d" % p]["ms_median"])
    out["shapes"][name] = row
    print("%-42s %-10s indexed %8.3f [%.3f, %.3f]  %s  auto(P=%d) %8.3f [%.3f, %.3f]" % (
        name, row["route"], r["indexed"]["ms_median"], r["indexed"]["ms_min"], r["indexed"]["ms_max"],
        "  ".join("P%d %.3f [%.3f, %.3f]" % (p, r["split_%d" % p]["ms_median"], r["split_%d" % p]["ms_min"], r["split_%d" % p]["ms_max"]) for p in splits),
        auto_p, r["auto"]["ms_median"], r["auto"]["ms_min"], r["auto"]["ms_max"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:                                      # (kept current shape by shape)
        json.dump(out, fh, indent=1); fh.write("\n")
ct.close(); mt.close(); table.close()
# ---- bench.py against the parent commit: the result lines of the alternated runs, where they lie beside the output
lines = {}
for who in ("parent", "this_tree"):
    path = os.path.join(os.path.dirname(os.path.abspath(OUT)), "bench_vm_committee_span_%s.jsonl" % who)
    if os.path.exists(path):
        with open(path) as fh:
            lines[who] = [round(json.loads(l)["ms_per_step"], 4) for l in fh if l.strip()]
if len(lines) == 2:
    out["bench_vs_parent"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5 of the parent commit and of this tree, alternated (full lines: bench_vm_committee_span_parent.jsonl, "
                                      "bench_vm_committee_span_this_tree.jsonl beside this file)",
                              "parent_ms_per_step": lines["parent"], "this_tree_ms_per_step": lines["this_tree"]}
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
