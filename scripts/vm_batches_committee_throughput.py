"""Many verify_multiple batches per call over committee bitfields and the resident message table
(mbls_verify_multiple_batches_committee_msgtable_locate_device) against the two things a gossip caller with resident tables can do without it, measured in the same
process on the same sets:
  (a) `indexed`: mbls_verify_multiple_batches_locate_indexed_device on the spelled-out sets (signers through a ragged offset table, 32 message bytes per set);
  (b) `per_batch_loop`: one mbls_verify_multiple_committee_msgtable_locate_device call per batch (measured up to VBC_LOOP_MAX_BATCHES batches, default 128: the loop
      of 1 024 calls takes seconds per repetition; "not measured" beyond).
Shapes (batches x sets per batch): 16 x 10, 128 x 10, 1 024 x 10, 1 024 x 63, 64 x 1 000; every batch naming 1, 4 or sets-per-batch distinct table entries; 128-member
committees at 99 % participation in a gossip mix of two single-key sets per committee set; all valid, and 1 % of the batches (at least one) bad -- one participation
bit of one committee set flipped. Variants of the new entry: auto with max_groups = 0, auto with the exact count, grouped (mode 1) and per set (mode 2) forced,
both with the exact count. The _locate entries everywhere: that is what the caller retries with.
Same timing method for every variant: a host clock around a window of repetitions that ends in a device synchronise, every shape warmed up, the variants alternated
inside every round, medians over the rounds with [min, max] beside them. Every result of every window is checked. No target is set: every row is written down,
those where the new entry is slower than (a) included.
usage: python scripts/vm_batches_committee_throughput.py [OUT.json]  (default profiles/vm_batches_committee_throughput.json; VBC_ROUNDS, default 10; VBC_ONLY: a
substring of the shape names to run)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_batches_committee_throughput.json")
ROUNDS = int(os.environ.get("VBC_ROUNDS", "10"))
LOOP_MAX = int(os.environ.get("VBC_LOOP_MAX_BATCHES", "128"))
ONLY = os.environ.get("VBC_ONLY", "")
WINDOW_S = 0.1
SINGLE = N.VM_SET_SINGLE_KEY
M, COMMITTEES, PERCENT, T = 128, 512, 99, 1024
ctx = N.default_context()
P = lambda t: t.data_ptr()
pool = bench.make_pool(bench.SEED)
POOL = len(pool)
limbs = np.array([[(sk >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for sk in pool], dtype=np.uint64)
pool_sk = np.frombuffer(b"".join(x.to_bytes(32, "big") for x in pool), dtype=np.uint8).reshape(POOL, 32)
d_pool_sk = torch.from_numpy(pool_sk.copy()).to(dev)
d_pool_pk = torch.empty((POOL, 96), dtype=torch.uint8, device=dev)
ctx.check(lib.mbls_sk_to_pk_batch_device(ctx.handle, P(d_pool_sk), N.PK_UNCOMPRESSED, POOL, P(d_pool_pk), None))
table = N.KeyTable(ctx, capacity_hint=POOL)
d_errs = torch.zeros(POOL, dtype=torch.uint8, device=dev)
table.append_device(P(d_pool_pk), POOL, P(d_errs), pk_format=N.PK_UNCOMPRESSED, validate=False)
torch.cuda.synchronize(); assert int(d_errs.max().item()) == 0
rng0 = np.random.default_rng(31)
a0 = rng0.integers(0, POOL, size=COMMITTEES, dtype=np.int64); s0 = rng0.integers(0, POOL // 2, size=COMMITTEES, dtype=np.int64) * 2 + 1
members = (a0[:, None] + np.arange(M, dtype=np.int64)[None, :] * s0[:, None]) % POOL
ct = N.CommitteeTable(table, capacity_hint=COMMITTEES)
assert ct.append(members.reshape(-1).tolist(), list(range(0, COMMITTEES * M + 1, M))) == 0
d_list = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(T, 32), dtype=np.uint8)).to(dev)
mt = N.MsgTable(ctx, capacity_hint=T)
assert mt.append_device(P(d_list), T, msg_len=32) == 0
STRIDE = M // 8


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


def world(B, spb, entries, seed):
    """B x spb sets: committee sets with two single-key sets behind each; batch b names `entries` table entries -> the honest and the bent device inputs"""
    n = B * spb
    rng = np.random.default_rng(seed)
    is_cmt = (np.arange(n) % 3) == 0
    nc = int(is_cmt.sum())
    cid = rng.integers(0, COMMITTEES, size=nc, dtype=np.int64)
    s = max(1, int(round(M * PERCENT / 100.0)))
    order = np.argsort(rng.random((nc, M)), axis=1)
    signed = np.zeros((nc, M), dtype=bool)
    np.put_along_axis(signed, order[:, :s], True, axis=1)
    sk = np.zeros((n, 32), dtype=np.uint8); csk = np.zeros((nc, 32), dtype=np.uint8)
    for c0 in range(0, nc, 2048):
        agg = (limbs[members[cid[c0:c0 + 2048]]] * signed[c0:c0 + 2048, :, None]).sum(axis=1)
        for i in range(agg.shape[0]):
            v = sum(int(agg[i, j]) << (32 * j) for j in range(8)) % bench.R
            csk[c0 + i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    sk[is_cmt] = csk
    key = rng.integers(0, POOL, size=n, dtype=np.int64)
    sk[~is_cmt] = pool_sk[key[~is_cmt]]
    words = np.where(is_cmt, 0, SINGLE | key).astype(np.uint32); words[is_cmt] = cid.astype(np.uint32)
    b_of = np.arange(n) // spb
    midx = ((b_of * entries + (np.arange(n) % spb) % entries) % T).astype(np.int64)
    groups = int(sum(len(set(midx[b * spb:(b + 1) * spb].tolist())) for b in range(B)))
    # 1 % of the batches bad, at least one: the first committee set of the batch gets one bit flipped
    bad_batches = sorted({(7 + 100 * k) % B for k in range(max(1, B // 100))})
    cpos = np.flatnonzero(is_cmt)
    named = signed.copy()
    bad_sets = []
    for b in bad_batches:
        k = int(np.searchsorted(cpos, b * spb))
        assert cpos[k] < (b + 1) * spb
        named[k, int(rng.integers(0, M))] ^= True
        bad_sets.append(int(cpos[k]))
    w = {"n": n, "words": words, "sk": sk, "midx": midx, "groups": groups, "bad_batches": bad_batches, "bad_sets": bad_sets}
    for tag, sel in (("valid", signed), ("bad", named)):
        bits = np.zeros((n, STRIDE), dtype=np.uint8)
        bits[is_cmt] = np.packbits(sel, axis=1, bitorder="little")
        cnt = np.ones(n, dtype=np.int64); cnt[is_cmt] = sel.sum(axis=1)
        off = np.concatenate([[0], np.cumsum(cnt)])
        lists = np.zeros(int(off[-1]), dtype=np.int64)
        starts = off[:-1]
        lists[starts[~is_cmt]] = key[~is_cmt]
        flat = members[cid][sel]
        cstart = starts[is_cmt]; ccnt = cnt[is_cmt]
        lists[np.repeat(cstart, ccnt) + (np.arange(flat.size) - np.repeat(np.cumsum(ccnt) - ccnt, ccnt))] = flat
        w[tag] = (bits, lists, off)
    return w


out = {"form": "device-resident inputs; keys, committees and 32-byte messages resident; _locate entries on every side; `valid`: every batch answers 1; `bad`: 1 % of the "
               "batches (at least one) hold one committee set with one participation bit flipped",
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition; median [min, max] over the rounds",
       "baselines": {"indexed": "mbls_verify_multiple_batches_locate_indexed_device on the spelled-out sets",
                     "per_batch_loop": "one mbls_verify_multiple_committee_msgtable_locate_device call per batch (up to %d batches; not measured beyond)" % LOOP_MAX},
       "round_items": int(ctx.limits().round_items), "members": M, "participation_percent": PERCENT, "table_entries": T, "rows": {}}
SHAPES = [(16, 10), (128, 10), (1024, 10), (1024, 63), (64, 1000)]
ctx.reserve_committee_items(65536, M)
for B, spb in SHAPES:
    for entries in (1, 4, spb):
        name = "%dx%d/%d_entries_per_batch" % (B, spb, entries)
        if ONLY and ONLY not in name:
            continue
        W = world(B, spb, entries, 1000 * B + spb + entries)
        n = W["n"]
        d_midx = torch.from_numpy(W["midx"].astype(np.int32)).to(dev)
        d_msgs = d_list[torch.from_numpy(W["midx"]).to(dev)].contiguous()
        d_sk = torch.from_numpy(W["sk"]).to(dev)
        d_sigs = torch.empty((n, 96), dtype=torch.uint8, device=dev)
        ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_msgs), 32, n, P(d_sigs), None))
        d_words = torch.from_numpy(W["words"].view(np.int32)).to(dev)
        d_rands = torch.from_numpy(np.random.default_rng(B + spb).integers(1, 1 << 63, size=n, dtype=np.int64)).to(dev)
        d_res = torch.zeros(B, dtype=torch.uint8, device=dev); d_sres = torch.zeros(n, dtype=torch.uint8, device=dev)
        row = {"batches": B, "sets_per_batch": spb, "sets": n, "entries_per_batch": entries, "groups": W["groups"], "bad_batches": len(W["bad_batches"])}
        for mode, mg in ((0, 0), (0, W["groups"])):
            p = N.plan_verify_multiple_batches_committee(n, B, spb, T, mg, mode, True, limits=ctx.limits())
            row["plan_auto_max_groups_%s" % ("0" if not mg else "exact")] = {"route": {0: "per_set", 1: "grouped"}[p["route"]], "bound": p["bound"], "miller_items": p["miller_items"]}
        for form in ("valid", "bad"):
            bits, lists, off = W[form]
            d_bits = torch.from_numpy(bits).to(dev)
            d_keys = torch.from_numpy(lists.astype(np.uint32).view(np.int32)).to(dev); d_off = torch.from_numpy(off.astype(np.uint32).view(np.int32)).to(dev)
            want_b = torch.ones(B, dtype=torch.uint8, device=dev); want_s = torch.ones(n, dtype=torch.uint8, device=dev)
            if form == "bad":
                want_b[torch.tensor(W["bad_batches"], device=dev)] = 0; want_s[torch.tensor(W["bad_sets"], device=dev)] = 0
            torch.cuda.synchronize()

            def new(mode, mg):
                def f():
                    ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, mode))
                    ctx.check(lib.mbls_verify_multiple_batches_committee_msgtable_locate_device(ctx.handle, ct.handle, P(d_sigs), P(d_words), P(d_bits), STRIDE, mt.handle,
                                                                                                P(d_midx), P(d_rands), n, None, spb, B, mg, P(d_res), None, P(d_sres), None, None))
                    ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, 0))
                return f

            def indexed():
                ctx.check(lib.mbls_verify_multiple_batches_locate_indexed_device(ctx.handle, table.handle, P(d_sigs), P(d_keys), P(d_off), 0, P(d_msgs), 32, None, P(d_rands), n,
                                                                                 None, spb, B, P(d_res), None, P(d_sres), None, None))

            def loop():
                for b in range(B):
                    lo = b * spb
                    ctx.check(lib.mbls_verify_multiple_committee_msgtable_locate_device(ctx.handle, ct.handle, P(d_sigs) + 96 * lo, P(d_words) + 4 * lo, P(d_bits) + STRIDE * lo,
                                                                                        STRIDE, mt.handle, P(d_midx) + 4 * lo, P(d_rands) + 8 * lo, spb, P(d_res) + b, None,
                                                                                        P(d_sres) + lo, None, None))

            def clear():
                d_res.fill_(7); d_sres.fill_(7)
            good = lambda: bool((d_res == want_b).all()) and bool((d_sres == want_s).all())
            variants = [("auto_max_groups_0", new(0, 0)), ("auto_max_groups_exact", new(0, W["groups"])), ("grouped_forced", new(1, W["groups"])),
                        ("per_set_forced", new(2, W["groups"])), ("indexed", indexed)]
            if B <= LOOP_MAX:
                variants.append(("per_batch_loop", loop))
            r = measure(variants, clear, good, (name, form))
            if B > LOOP_MAX:
                r["per_batch_loop"] = "not measured"
            r["auto_exact_minus_indexed_ms"] = round(r["auto_max_groups_exact"]["ms_median"] - r["indexed"]["ms_median"], 4)
            r["auto_0_minus_indexed_ms"] = round(r["auto_max_groups_0"]["ms_median"] - r["indexed"]["ms_median"], 4)
            r["indexed_spread_ms"] = round(r["indexed"]["ms_max"] - r["indexed"]["ms_min"], 4)
            r["new_entry_slower_than_indexed"] = {k: bool(r[k]["ms_median"] > r["indexed"]["ms_median"]) for k in ("auto_max_groups_0", "auto_max_groups_exact")}
            row[form] = r
            print("%-34s %-5s  auto/0 %8.3f  auto/exact %8.3f  grouped %8.3f  per set %8.3f  indexed %8.3f [%.3f, %.3f]  loop %s" % (
                name, form, r["auto_max_groups_0"]["ms_median"], r["auto_max_groups_exact"]["ms_median"], r["grouped_forced"]["ms_median"], r["per_set_forced"]["ms_median"],
                r["indexed"]["ms_median"], r["indexed"]["ms_min"], r["indexed"]["ms_max"],
                ("%8.3f" % r["per_batch_loop"]["ms_median"]) if B <= LOOP_MAX else "not measured"), flush=True)
        out["rows"][name] = row
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:                                  # (kept current row by row)
            json.dump(out, fh, indent=1); fh.write("\n")
ct.close(); mt.close(); table.close()
# ---- bench.py against the parent commit: the result lines of the alternated runs, where they lie beside the output
lines = {}
for who in ("parent", "this_tree"):
    path = os.path.join(os.path.dirname(os.path.abspath(OUT)), "bench_vm_batches_committee_%s.jsonl" % who)
    if os.path.exists(path):
        with open(path) as fh:
            lines[who] = [round(json.loads(l)["ms_per_step"], 4) for l in fh if l.strip()]
if len(lines) == 2:
    out["bench_vs_parent"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5 of the parent commit and of this tree, alternated",
                              "parent_ms_per_step": lines["parent"], "this_tree_ms_per_step": lines["this_tree"]}
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
