"""Many verify_multiple batches per call over committee spans (mbls_verify_multiple_batches_committee_span_msgtable[_locate]_device: one verdict per BLOCK) against
the three things a caller can do without it, measured in the same process on the same sets:
  loop      one mbls_verify_multiple_committee_span_msgtable_locate_device call per block (for the 1 024-block shape 128 calls are measured and the total is
            computed: x 8; the profile says so)
  merged    ONE call of that entry over all sets: the floor -- it cannot say which block is bad
  indexed   mbls_verify_multiple_batches_locate_indexed_device on the spelled-out signers and message bytes
The new entry runs through _locate under the auto split and under P = 1 (mbls_ctx_set_vm_span_split). A block is the shape of
scripts/vm_committee_span_throughput.py: 8 span sets of 64 x 128 members, one set over a 512-member committee, 3 single-key sets. Shapes: 64 and 1 024 blocks per
call at 100, 99, 90 and 45 % participation, all valid; 64 blocks at 99 % with one bit flipped in one block. The 1 024-block call holds the 64 generated blocks 16
times over with scalars of its own per set (the host side of generating 12 288 distinct sets is minutes; no kernel knows two sets are equal, but equal ids and
fields may help the caches of the key phase: not measured, a caveat on the 1 024-block rows). Device-resident
inputs. Every result of every window is checked: every batch byte and status word, every set byte (all 1 / 0; with the flipped bit the block reads 0 with
MBLS_ST_PAIRING_FAILED, its set 0, everything else 1; the merged call reads 0). Same timing method for every variant: a host clock around a window of repetitions that
ends in a device synchronise, every variant warmed up, the variants alternated inside every round, medians over the rounds with [min, max] beside them.
The output also carries `bench_vs_parent` from bench_vm_batches_committee_span_{parent,this_tree}.jsonl beside it, where those files exist.
usage: python scripts/vm_batches_committee_span_throughput.py [OUT.json]   (default: profiles/vm_batches_committee_span_throughput.json; VBST_ROUNDS, default 10)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_batches_committee_span_throughput.json")
ROUNDS = int(os.environ.get("VBST_ROUNDS", "10"))
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
        assert good(name), (tag, name)
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
        times[name] = []
    for _ in range(ROUNDS):
        for name, f in variants:
            times[name].append(1e3 * window(f, reps[name], clear))
            assert good(name), (tag, name)
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
SPB = len(BLOCK)
GEN_BLOCKS, LOOP_MEASURED = 64, 128
PAIRING = 0x40
out = {"form": "device-resident inputs, keys and 32-byte messages resident, one blinding scalar per set; every batch byte, status word and set byte checked in every window",
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition (per whole range of blocks); median [min, max] over the rounds",
       "variants": {"auto": "the new _locate entry, split factor by rule on the call's sets", "split_1": "the new _locate entry, P = 1",
                    "loop": "one mbls_verify_multiple_committee_span_msgtable_locate_device call per block",
                    "merged": "ONE mbls_verify_multiple_committee_span_msgtable_locate_device call over all sets: cannot say which block is bad",
                    "indexed": "mbls_verify_multiple_batches_locate_indexed_device on the spelled-out signers and message bytes"},
       "loop_note": "1 024 blocks: %d calls are measured per repetition and the figure is multiplied by %d" % (LOOP_MEASURED, 1024 // LOOP_MEASURED),
       "tiling_note": "1 024 blocks: the 64 generated blocks 16 times over, scalars of their own per set; identical committee ids and fields across the tiles may help cache "
                      "behaviour in the key phase against 1 024 distinct blocks -- not measured, read the 1 024-block rows with that caveat",
       "round_items": int(ctx.limits().round_items), "members_per_committee": M_MEMBERS, "sync_committee_members": SYNC_MEMBERS, "committees_in_table": COMMITTEES + 1,
       "table_entries": ENTRIES, "bits_stride": STRIDE, "region_words": WIDTH, "sets_per_block": SPB, "shapes": {}}
SHAPES = [("%d_blocks/%d_percent" % (b, p), b, p, False) for b in (64, 1024) for p in (100, 99, 90, 45)] + [("64_blocks/99_percent/one_flipped_bit", 64, 99, True)]
gen = {}
for name, blocks, percent, flipped in SHAPES:
    n0 = GEN_BLOCKS * SPB
    flip = 5 * SPB + 5 if flipped else None                          # a span set of block 5
    key = (percent, flipped)
    if key not in gen:
        S = sets_of(BLOCK * GEN_BLOCKS, percent, 1000 * n0 + percent, flip)
        rng = np.random.default_rng(9 + n0)
        midx0 = rng.integers(0, ENTRIES, size=n0, dtype=np.int64)
        d_signed_msgs = d_list[torch.from_numpy(midx0).to(dev)].contiguous()
        d_sk = torch.from_numpy(S["sk"]).to(dev)
        d_sigs0 = torch.empty((n0, 96), dtype=torch.uint8, device=dev)
        ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_signed_msgs), 32, n0, P(d_sigs0), None))
        torch.cuda.synchronize()
        gen[key] = (S, midx0, d_sigs0, d_signed_msgs)
    S, midx0, d_sigs0, d_msgs0 = gen[key]
    tiles = blocks // GEN_BLOCKS
    n = blocks * SPB
    rng = np.random.default_rng(77 + n)
    ids = np.tile(S["ids"], tiles); n_ids = int(ids.size)
    off = np.concatenate([[0]] + [S["off"][1:].astype(np.int64) + t * int(S["ids"].size) for t in range(tiles)]).astype(np.uint32)
    loff = np.concatenate([[0]] + [S["loff"][1:].astype(np.int64) + t * int(S["lists"].size) for t in range(tiles)]).astype(np.uint32)
    d_sigs = d_sigs0.repeat(tiles, 1).contiguous(); d_msgs = d_msgs0.repeat(tiles, 1).contiguous()
    d_midx = torch.from_numpy(np.tile(midx0, tiles).astype(np.int32)).to(dev)
    d_rands = torch.from_numpy(rng.integers(1, 1 << 62, size=n, dtype=np.int64)).to(dev)
    d_ids = torch.from_numpy(ids.view(np.int32)).to(dev); d_soff = torch.from_numpy(off.view(np.int32)).to(dev)
    d_bits = torch.from_numpy(np.tile(S["bits"], (tiles, 1))).to(dev)
    d_keys = torch.from_numpy(np.tile(S["lists"].astype(np.int32), tiles)).to(dev); d_koff = torch.from_numpy(loff.view(np.int32)).to(dev)
    d_res = torch.zeros(blocks, dtype=torch.uint8, device=dev); d_st = torch.zeros(blocks, dtype=torch.int32, device=dev)
    d_sres = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_one = torch.zeros(1, dtype=torch.uint8, device=dev); d_one_st = torch.zeros(1, dtype=torch.int32, device=dev)
    want_sets = torch.ones(n, dtype=torch.uint8, device=dev); want_res = torch.ones(blocks, dtype=torch.uint8, device=dev)
    want_st = torch.zeros(blocks, dtype=torch.int32, device=dev)
    if flipped:
        want_sets[flip] = 0; want_res[flip // SPB] = 0; want_st[flip // SPB] = PAIRING
    # the per-block views of the loop: block b's ids start at off[b * SPB] (absolute offsets: the whole id array is handed over), its other arrays at set b * SPB
    calls = min(blocks, LOOP_MEASURED)
    torch.cuda.synchronize()

    def new():
        ctx.check(lib.mbls_verify_multiple_batches_committee_span_msgtable_locate_device(ctx.handle, ct.handle, P(d_sigs), P(d_ids), n_ids, P(d_soff), P(d_bits), STRIDE,
                                                                                         mt.handle, P(d_midx), P(d_rands), n, None, SPB, blocks, 0, P(d_res), P(d_st),
                                                                                         P(d_sres), None, None))

    def with_split(mode):
        def f():
            ctx.check(lib.mbls_ctx_set_vm_span_split(ctx.handle, mode))
            new()
            ctx.check(lib.mbls_ctx_set_vm_span_split(ctx.handle, 0))
        return f

    def loop():
        for b in range(calls):
            s0 = b * SPB
            ctx.check(lib.mbls_verify_multiple_committee_span_msgtable_locate_device(ctx.handle, ct.handle, P(d_sigs) + 96 * s0, P(d_ids), n_ids, P(d_soff) + 4 * s0,
                                                                                     P(d_bits) + STRIDE * s0, STRIDE, mt.handle, P(d_midx) + 4 * s0, P(d_rands) + 8 * s0, SPB,
                                                                                     P(d_res) + b, P(d_st) + 4 * b, P(d_sres) + s0, None, None))

    def merged():
        ctx.check(lib.mbls_verify_multiple_committee_span_msgtable_locate_device(ctx.handle, ct.handle, P(d_sigs), P(d_ids), n_ids, P(d_soff), P(d_bits), STRIDE, mt.handle,
                                                                                 P(d_midx), P(d_rands), n, P(d_one), P(d_one_st), P(d_sres), None, None))

    def indexed():
        ctx.check(lib.mbls_verify_multiple_batches_locate_indexed_device(ctx.handle, table.handle, P(d_sigs), P(d_keys), P(d_koff), 0, P(d_msgs), 32, None, P(d_rands), n,
                                                                         None, SPB, blocks, P(d_res), P(d_st), P(d_sres), None, None))

    def clear():
        d_res.fill_(7); d_st.fill_(7); d_sres.fill_(7); d_one.fill_(7); d_one_st.fill_(7)

    def good(which):
        if which == "merged":
            return int(d_one.item()) == (0 if flipped else 1) and int(d_one_st.item()) == 0 and bool((d_sres == want_sets).all())
        if which == "loop":      # (a one-batch call reports a failed pairing check through the bool only)
            return bool((d_res[:calls] == want_res[:calls]).all()) and bool((d_st[:calls] == 0).all()) and bool((d_sres[:calls * SPB] == want_sets[:calls * SPB]).all())
        return bool((d_res == want_res).all()) and bool((d_st == want_st).all()) and bool((d_sres == want_sets).all())
    variants = [("auto", with_split(0)), ("split_1", with_split(1)), ("loop", loop), ("merged", merged), ("indexed", indexed)]
    r = measure(variants, clear, good, name)
    scale = blocks // calls
    if scale > 1:
        r["loop"] = dict({k: round(v * scale, 4) for k, v in r["loop"].items() if k.startswith("ms_")}, reps_per_window=r["loop"]["reps_per_window"], calls_measured=calls,
                         multiplied_by=scale)
    plan, auto_p = N.plan_verify_multiple_batches_committee_span(n, blocks, SPB, ENTRIES, 0, 0, True, WIDTH, 0, ctx.limits())
    row = dict(r, blocks=blocks, sets=n, participation_percent=percent, one_flipped_bit=flipped, auto_split=auto_p, route=plan["route"], workspace_items=plan["workspace_items"],
               input_bytes_per_set={"span": round((4.0 * n_ids + 4 * (n + 1)) / n + STRIDE, 1), "indexed": round(4.0 * int(d_keys.numel()) / n + 4, 1)})
    for base in ("loop", "merged", "indexed", "split_1"):
        spread = round(r[base]["ms_max"] - r[base]["ms_min"], 4)
        diff = round(r["auto"]["ms_median"] - r[base]["ms_median"], 4)
        row["auto_vs_" + base] = {"auto_minus_it_ms": diff, "its_spread_ms": spread, "auto_slower_beyond_its_spread": bool(diff > spread),
                                  "ratio_it_over_auto": round(r[base]["ms_median"] / r["auto"]["ms_median"], 3)}
    out["shapes"][name] = row
    print("%-36s P=%-2d  %s" % (name, auto_p, "  ".join("%s %.3f [%.3f, %.3f]" % (k, r[k]["ms_median"], r[k]["ms_min"], r[k]["ms_max"]) for k, _ in variants)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:                                      # (kept current shape by shape)
        json.dump(out, fh, indent=1); fh.write("\n")
    del d_keys, d_bits, d_sigs, d_msgs
ct.close(); mt.close(); table.close()
# ---- bench.py against the parent commit: the result lines of the alternated runs, where they lie beside the output
lines = {}
for who in ("parent", "this_tree"):
    path = os.path.join(os.path.dirname(os.path.abspath(OUT)), "bench_vm_batches_committee_span_%s.jsonl" % who)
    if os.path.exists(path):
        with open(path) as fh:
            lines[who] = [round(json.loads(l)["ms_per_step"], 4) for l in fh if l.strip()]
if len(lines) == 2:
    out["bench_vs_parent"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5 of the parent commit and of this tree, alternated three times each, parent first (full lines: "
                                      "bench_vm_batches_committee_span_parent.jsonl, bench_vm_batches_committee_span_this_tree.jsonl beside this file)",
                              "parent_ms_per_step": lines["parent"], "this_tree_ms_per_step": lines["this_tree"]}
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
