"""The verify_multiple stream (mbls_stream_create_vm_committee, mbls_stream_submit_vm[_device]) on a gossip load: B callers' batches of 3, 10, 63 and 192 sets,
two single-key sets per committee set, 128-member committees at 99 % participation, every batch naming one table entry or 10 (at most its sets), every 100th
batch holding one bad set (one participation bit of a committee set flipped). Measured in the same process on the same sets:
  `stream_device`, `stream_host`: every batch submitted as a call of its own, from the first submit to the completion of the last (flush, wait for the last
      ticket, device synchronise); B is what fills SVT_FILL (default 3) rounds of SVT_ROUND_ITEMS (default 4 096) at n_sets + 1 per call;
  (a) `loop`: one mbls_verify_multiple_batches_committee_msgtable_locate_device call per batch (n_batches = 1) -- what a caller without the stream does; measured
      over the first min(B, SVT_LOOP_MAX_BATCHES = 128) batches (the whole loop takes seconds per repetition) and reported per batch, with the figure scaled to B
      marked as computed;
  (b) `one_call`: ONE such call over all B batches laid out back to back -- the floor the stream cannot beat: it needs every batch in one caller's hands.
The four are alternated inside every round; medians over SVT_ROUNDS (default 10) rounds with [min, max]; every result of every repetition is checked against what
the sets were built to give. No target is set: every row is written down, those where the stream loses to (a) included.
usage: python scripts/stream_vm_throughput.py [OUT.json]  (default profiles/stream_vm_throughput.json; SVT_ONLY: a substring of the row names to run)"""
import ctypes as C, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N
from milagro_bls_amd.stream import VerifyStream

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_vm_throughput.json")
ROUNDS = int(os.environ.get("SVT_ROUNDS", "10"))
ROUND_ITEMS = int(os.environ.get("SVT_ROUND_ITEMS", "4096"))
FILL = int(os.environ.get("SVT_FILL", "3"))
LOOP_MAX = int(os.environ.get("SVT_LOOP_MAX_BATCHES", "128"))
ONLY = os.environ.get("SVT_ONLY", "")
SINGLE = N.VM_SET_SINGLE_KEY
M, COMMITTEES, PERCENT, T = 128, 512, 99, 1024
STRIDE = M // 8
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


def stat(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def world(B, spb, entries, seed):
    """B batches of spb sets: within a batch set j is a committee set where j % 3 == 0 and a single-key set otherwise; batch b names `entries` table entries;
    every 100th batch (b % 100 == 7) has one bit of its first committee set flipped -> host arrays and what every batch and set must answer"""
    n = B * spb
    rng = np.random.default_rng(seed)
    is_cmt = ((np.arange(n) % spb) % 3) == 0
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
    midx = ((b_of * entries + (np.arange(n) % spb) % entries) % T).astype(np.uint32)
    bad_batches = [b for b in range(B) if b % 100 == 7]
    cpos = np.flatnonzero(is_cmt)
    named = signed.copy()
    bad_sets = []
    for b in bad_batches:
        k = int(np.searchsorted(cpos, b * spb))
        named[k, int(rng.integers(0, M))] ^= True
        bad_sets.append(int(cpos[k]))
    bits = np.zeros((n, STRIDE), dtype=np.uint8)
    bits[is_cmt] = np.packbits(named, axis=1, bitorder="little")
    want_b = np.ones(B, dtype=np.uint8); want_b[bad_batches] = 0
    want_s = np.ones(n, dtype=np.uint8); want_s[bad_sets] = 0
    return dict(n=n, sk=sk, words=words, midx=midx, bits=bits, want_b=want_b, want_s=want_s, bad_batches=len(bad_batches))


out = {"form": "keys, committees and 32-byte messages resident; every batch answers per batch and per set; every 100th batch (b % 100 == 7) holds one committee set "
               "with one participation bit flipped",
       "rounds": ROUNDS, "stream_round_items": ROUND_ITEMS, "rounds_filled": FILL, "context_round_items": int(ctx.limits().round_items),
       "timing": "host clock from the first submit (or call) to the completion of the last, ending in a device synchronise; ms per repetition of the whole sequence; "
                 "median [min, max] over the rounds, the variants alternated inside every round, every shape warmed up once",
       "baselines": {"loop": "(a) one mbls_verify_multiple_batches_committee_msgtable_locate_device call per batch, over the first min(B, %d) batches" % LOOP_MAX,
                     "one_call": "(b) one such call over all B batches back to back: the floor"},
       "members": M, "participation_percent": PERCENT, "table_entries": T, "rows": {}}
ctx.reserve_committee_items(65536, M)
for spb in (3, 10, 63, 192):
    for entries in (1, 10):
        name = "%d_sets/%d_entries_per_batch" % (spb, min(entries, spb))
        if ONLY and not any(p in "^" + name + "$" for p in ONLY.split(",")):     # (comma-separated alternatives; ^ and $ anchor a part at the ends of the name)
            continue
        B = int(math.ceil(FILL * ROUND_ITEMS / (spb + 1.0)))
        W = world(B, spb, min(entries, spb), 1000 * spb + entries)
        n = W["n"]
        d_midx = torch.from_numpy(W["midx"].view(np.int32)).to(dev)
        d_msgs = d_list[torch.from_numpy(W["midx"].astype(np.int64)).to(dev)].contiguous()
        d_sk = torch.from_numpy(W["sk"]).to(dev)
        d_sigs = torch.empty((n, 96), dtype=torch.uint8, device=dev)
        ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_msgs), 32, n, P(d_sigs), None))
        d_words = torch.from_numpy(W["words"].view(np.int32)).to(dev)
        rands = np.random.default_rng(spb + entries).integers(1, 1 << 63, size=n, dtype=np.int64).view(np.uint64)
        d_rands = torch.from_numpy(rands.view(np.int64)).to(dev)
        d_bits = torch.from_numpy(W["bits"]).to(dev)
        d_res = torch.zeros(B, dtype=torch.uint8, device=dev); d_sres = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        h_sigs = d_sigs.cpu().numpy().copy(); h_words, h_midx, h_bits = W["words"].copy(), W["midx"].copy(), W["bits"].copy()
        h_res = np.zeros(B, dtype=np.uint8); h_sres = np.zeros(n, dtype=np.uint8)
        d_want_b = torch.from_numpy(W["want_b"]).to(dev); d_want_s = torch.from_numpy(W["want_s"]).to(dev)
        vs = VerifyStream(ctx, vm=True, committees=ct, msg_table=mt, bits_stride=STRIDE, round_items=ROUND_ITEMS)
        t = C.c_uint64(0); tref = C.byref(t)
        dev_args = [(vs.handle, P(d_sigs) + 96 * b * spb, P(d_words) + 4 * b * spb, P(d_bits) + STRIDE * b * spb, STRIDE, P(d_midx) + 4 * b * spb, P(d_rands) + 8 * b * spb,
                     spb, P(d_res) + b, None, P(d_sres) + b * spb, None, None, tref) for b in range(B)]
        hp = lambda a: a.ctypes.data
        host_args = [(vs.handle, hp(h_sigs) + 96 * b * spb, hp(h_words) + 4 * b * spb, hp(h_bits) + STRIDE * b * spb, STRIDE, hp(h_midx) + 4 * b * spb, hp(rands) + 8 * b * spb,
                      spb, hp(h_res) + b, None, hp(h_sres) + b * spb, None, tref) for b in range(B)]
        direct = lib.mbls_verify_multiple_batches_committee_msgtable_locate_device
        BL = min(B, LOOP_MAX)

        def finish():
            vs.flush(); vs.check(lib.mbls_stream_wait(vs.handle, t.value)); torch.cuda.synchronize()

        def stream_device():
            f = lib.mbls_stream_submit_vm_device
            for a in dev_args:
                if f(*a):
                    raise RuntimeError(vs.last_error())
            finish()

        def stream_host():
            f = lib.mbls_stream_submit_vm
            for a in host_args:
                if f(*a):
                    raise RuntimeError(vs.last_error())
            finish()

        def loop():
            for b in range(BL):
                lo = b * spb
                ctx.check(direct(ctx.handle, ct.handle, P(d_sigs) + 96 * lo, P(d_words) + 4 * lo, P(d_bits) + STRIDE * lo, STRIDE, mt.handle, P(d_midx) + 4 * lo,
                                 P(d_rands) + 8 * lo, spb, None, spb, 1, 0, P(d_res) + b, None, P(d_sres) + lo, None, None))
            torch.cuda.synchronize()

        def one_call():
            ctx.check(direct(ctx.handle, ct.handle, P(d_sigs), P(d_words), P(d_bits), STRIDE, mt.handle, P(d_midx), P(d_rands), n, None, spb, B, 0, P(d_res), None,
                             P(d_sres), None, None))
            torch.cuda.synchronize()

        def clear():
            d_res.fill_(7); d_sres.fill_(7); h_res[:] = 7; h_sres[:] = 7; torch.cuda.synchronize()

        def good(which):
            if which == "stream_host":
                return bool((h_res == W["want_b"]).all()) and bool((h_sres == W["want_s"]).all())
            k = BL if which == "loop" else B
            return bool((d_res[:k] == d_want_b[:k]).all()) and bool((d_sres[:k * spb] == d_want_s[:k * spb]).all())
        variants = [("stream_device", stream_device), ("stream_host", stream_host), ("loop", loop), ("one_call", one_call)]
        times = {k: [] for k, _ in variants}
        for rnd in range(ROUNDS + 1):                               # round 0 warms every variant up and is not counted
            for k, f in variants:
                clear()
                t0 = time.perf_counter(); f(); dt = 1e3 * (time.perf_counter() - t0)
                assert good(k), (name, k, rnd)
                if rnd:
                    times[k].append(dt)
        st = vs.stats()
        vs.close()
        row = {"batches": B, "sets_per_batch": spb, "sets": n, "entries_per_batch": min(entries, spb), "bad_batches": W["bad_batches"], "loop_batches": BL}
        row.update({k: stat(v) for k, v in times.items()})
        per = row["loop"]["ms_median"] / BL
        row["loop_ms_per_batch"] = round(per, 4)
        row["loop_scaled_to_all_batches_ms"] = {"value": round(per * B, 2), "how": "computed: ms per batch x batches; measured only where loop_batches == batches"}
        row["stream_rounds_per_sequence"] = round(st["rounds"] / (2.0 * (ROUNDS + 1)), 2)
        row["stream_device_slower_than_loop"] = bool(row["stream_device"]["ms_median"] > per * B)
        row["stream_host_slower_than_loop"] = bool(row["stream_host"]["ms_median"] > per * B)
        out["rows"][name] = row
        print("%-30s B %5d  stream dev %9.3f [%.3f, %.3f]  host %9.3f [%.3f, %.3f]  one call %8.3f [%.3f, %.3f]  loop of %d %9.3f (%.3f / batch, x B = %.1f)  rounds/seq %.1f" % (
            name, B, row["stream_device"]["ms_median"], row["stream_device"]["ms_min"], row["stream_device"]["ms_max"], row["stream_host"]["ms_median"],
            row["stream_host"]["ms_min"], row["stream_host"]["ms_max"], row["one_call"]["ms_median"], row["one_call"]["ms_min"], row["one_call"]["ms_max"], BL,
            row["loop"]["ms_median"], per, per * B, row["stream_rounds_per_sequence"]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:                                  # (kept current row by row)
            json.dump(out, fh, indent=1); fh.write("\n")
ct.close(); mt.close(); table.close()
# ---- bench.py against the parent commit: the result lines of the alternated runs, where they lie beside the output
lines = {}
for who in ("parent", "this_tree"):
    path = os.path.join(os.path.dirname(os.path.abspath(OUT)), "bench_stream_vm_%s.jsonl" % who)
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
