"""The verification stream over the committee table and the message table (mbls_stream_create_committee): a sustained flow of calls of 1, 16, 64 and 4 096 items --
a committee id, a 17-byte Bitlist (128 members and the delimiter, so the gather re-strides byte by byte) and a message-table index per item -- packed into full
rounds, against (a) the loop of direct mbls_fast_aggregate_verify_batch_committee_msgtable_device calls of that size, (b) the existing index stream
(mbls_stream_submit_msgidx_device) on the same items with the signers spelled out, and (c) one direct committee call over the whole round, the floor. Shapes:
128-member committees at 99 % and at 45 % participation over 512 table entries, device-resident inputs.
Same timing method for every variant: a host clock from the first submit (or call) to the completion of the last, one round of items per window, the variants
alternated inside every round of the measurement, medians over the rounds with [min, max] beside them. The loop of direct calls runs LOOP_CALLS calls per window
(a lone call is a latency chain of milliseconds: a whole round of one-item calls would take minutes) and is scaled to the round. Every result is checked: every
16th item (i % 16 == 7) has one bit flipped against its signers and must be rejected by every variant, every other item accepted.
usage: python scripts/stream_committee_throughput.py [OUT.json]   (default: profiles/stream_committee_throughput.json; SCT_ROUNDS, default 10; SCT_ITEMS, default
the context's round; SCT_LOOP_CALLS, default 64)"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N
from milagro_bls_amd.stream import VerifyStream

lib = N.lib(); dev = torch.device("cuda:0"); C = N.C
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_committee_throughput.json")
ctx = N.default_context()
ROUNDS = int(os.environ.get("SCT_ROUNDS", "10"))
NI = int(os.environ.get("SCT_ITEMS", str(int(ctx.limits().round_items))))
LOOP_CALLS = int(os.environ.get("SCT_LOOP_CALLS", "64"))
N_MSGS, M, COUNT, BITS_LEN, STRIDE = 512, 128, 512, 17, 20
SIZES = (1, 16, 64, 4096)
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
rng = np.random.default_rng(31 + M)
members = (rng.integers(0, POOL, size=COUNT)[:, None] + np.arange(M)[None, :] * (rng.integers(0, POOL // 2, size=COUNT) * 2 + 1)[:, None]) % POOL
ct = N.CommitteeTable(table, capacity_hint=COUNT)
assert ct.append(members.reshape(-1).tolist(), list(range(0, COUNT * M + 1, M))) == 0
midx = np.random.default_rng(9).integers(0, N_MSGS, size=NI, dtype=np.int64)
d_midx = torch.from_numpy(midx.astype(np.int32)).to(dev)
d_signed_msgs = d_list[torch.from_numpy(midx).to(dev)].contiguous()


def items_of(percent, seed):
    """per item a committee, exactly round(M percent / 100) signers, their aggregate secret key, and the Bitlist of the NAMED members (one bit flipped in every 16th
    item) with its delimiter: BITS_LEN bytes"""
    r = np.random.default_rng(seed)
    cid = r.integers(0, COUNT, size=NI, dtype=np.int64)
    s = max(1, int(round(M * percent / 100.0)))
    order = np.argsort(r.random((NI, M)), axis=1)
    signed = np.zeros((NI, M), dtype=bool)
    np.put_along_axis(signed, order[:, :s], True, axis=1)
    sk = np.zeros((NI, 32), dtype=np.uint8)
    for c0 in range(0, NI, 2048):
        agg = (limbs[members[cid[c0:c0 + 2048]]] * signed[c0:c0 + 2048, :, None]).sum(axis=1)
        for i in range(agg.shape[0]):
            v = sum(int(agg[i, j]) << (32 * j) for j in range(8)) % bench.R
            sk[c0 + i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    named = signed.copy()
    flip = np.arange(7, NI, 16)
    named[flip, r.integers(0, M, size=flip.size)] ^= True
    expect = np.ones(NI, dtype=np.uint8); expect[flip] = 0
    field = np.concatenate([named, np.ones((NI, 1), dtype=bool)], axis=1)          # the delimiter: bit M
    bits = np.packbits(field, axis=1, bitorder="little")
    assert bits.shape[1] == BITS_LEN
    lists = members[cid][named]
    off = np.concatenate([[0], np.cumsum(named.sum(axis=1))]).astype(np.uint32)
    return cid, sk, bits, lists, off, expect, s


def stat(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


out = {"form": "device-resident inputs; %d committees of %d members over a key table of %d keys, %d 32-byte messages in a resident table; fields of %d bytes (the Bitlist "
               "with its delimiter) into a stride of %d; item i %% 16 == 7 has one bit flipped against its signers (rejected), the others are valid; a round = %d items"
               % (COUNT, M, POOL, N_MSGS, BITS_LEN, STRIDE, NI),
       "rounds": ROUNDS, "loop_calls": LOOP_CALLS,
       "timing": "host clock from the first submit (call) to the completion of the last; ms per round of items; median [min, max] over alternated rounds; the loop of direct "
                 "calls runs loop_calls calls per window and is scaled to the round",
       "round_items": int(ctx.limits().round_items), "shapes": {}}
ctx.reserve(N.plan_workspace_items(NI, 0, False, ctx.limits())); ctx.reserve_committee_items(NI, M)
opts = dict(round_items=NI, policy=N.STREAM_FULL_ROUNDS)
ONLY = os.environ.get("SCT_ONLY", "")      # comma-separated substrings of "^<percent>_percent/calls_of_<n>$": the rows to run (default all)
wanted = lambda percent, n: not ONLY or any(p in "^%d_percent/calls_of_%d$" % (percent, n) for p in ONLY.split(","))
for percent in (99, 45):
    if not any(wanted(percent, n) for n in SIZES):
        continue
    cid, sk, bits, lists, off, expect_h, s = items_of(percent, 100 * M + percent)
    d_sk = torch.from_numpy(sk).to(dev)
    d_sigs = torch.empty((NI, 96), dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_signed_msgs), 32, NI, P(d_sigs), None))
    d_cid = torch.from_numpy(cid.astype(np.int32)).to(dev)
    d_bits = torch.from_numpy(bits).to(dev)                                           # NI x 17 bytes back to back
    bits20 = np.zeros((NI, STRIDE), dtype=np.uint8); bits20[:, :BITS_LEN] = bits
    d_bits20 = torch.from_numpy(bits20).to(dev)
    d_keys = torch.from_numpy(lists.astype(np.uint32).view(np.int32)).to(dev)
    expect = torch.from_numpy(expect_h).to(dev)
    d_res = torch.full((NI,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    route = "complement" if N.plan_committee_route(M, s) else "direct"
    sig0, mi0, ci0, b0, b20, k0, r0, off0 = P(d_sigs), P(d_midx), P(d_cid), P(d_bits), P(d_bits20), P(d_keys), P(d_res), off.ctypes.data
    tk = C.c_uint64(0)

    def check(tag, upto=NI):
        assert bool((d_res[:upto] == expect[:upto]).all()), (percent, tag)

    def direct_calls(n, calls):
        """`calls` direct committee calls of n items each, back to back on one stream -> seconds"""
        d_res.fill_(7); torch.cuda.synchronize(); t = time.perf_counter()
        for j in range(calls):
            a = j * n
            ctx.check(lib.mbls_fast_aggregate_verify_batch_committee_msgtable_device(ctx.handle, ct.handle, sig0 + 96 * a, mt.handle, mi0 + 4 * a, ci0 + 4 * a, b20 + STRIDE * a,
                                                                                     STRIDE, n, r0 + a, None, None, None))
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def stream_cmt(vs, n):
        d_res.fill_(7); torch.cuda.synchronize(); t = time.perf_counter()
        h = vs.handle
        for a in range(0, NI, n):
            rc = lib.mbls_stream_submit_committee_device(h, sig0 + 96 * a, mi0 + 4 * a, ci0 + 4 * a, b0 + BITS_LEN * a, BITS_LEN, n, r0 + a, None, None, None, C.byref(tk))
            if rc:
                vs.check(rc)
        vs.flush(); vs.wait(tk.value)
        return time.perf_counter() - t

    def stream_idx(vs, n):
        d_res.fill_(7); torch.cuda.synchronize(); t = time.perf_counter()
        h = vs.handle
        for a in range(0, NI, n):
            rc = lib.mbls_stream_submit_msgidx_device(h, sig0 + 96 * a, mi0 + 4 * a, None, k0, off0 + 4 * a, n, 0, r0 + a, None, None, None, C.byref(tk))
            if rc:
                vs.check(rc)
        vs.flush(); vs.wait(tk.value)
        return time.perf_counter() - t

    rows = {}
    with VerifyStream(ctx, committees=ct, msg_table=mt, bits_stride=STRIDE, **opts) as vc, VerifyStream(ctx, table=table, msg_table=mt, **opts) as vi:
        for n in SIZES:
            if not wanted(percent, n):
                continue
            loop_calls =min(LOOP_CALLS, NI // n)
            variants = [("stream_committee", lambda: stream_cmt(vc, n), NI), ("stream_indexed", lambda: stream_idx(vi, n), NI),
                        ("direct_loop", lambda: direct_calls(n, loop_calls) * (NI / (n * loop_calls)), n * loop_calls), ("direct_full_round", lambda: direct_calls(NI, 1), NI)]
            times = {name: [] for name, _, _ in variants}
            for name, f, upto in variants:                                             # warm-up, checked
                f(); check((n, name), upto)
            for _ in range(ROUNDS):
                for name, f, upto in variants:
                    times[name].append(1e3 * f()); check((n, name), upto)
            row = {name: dict(stat(times[name]), items_per_s=round(NI / (statistics.median(times[name]) / 1e3))) for name, _, _ in variants}
            row["direct_loop"]["calls_per_window"] = loop_calls
            row["stream_committee_vs_indexed_ms"] = round(row["stream_indexed"]["ms_median"] - row["stream_committee"]["ms_median"], 4)
            row["stream_committee_over_floor_ms"] = round(row["stream_committee"]["ms_median"] - row["direct_full_round"]["ms_median"], 4)
            rows["calls_of_%d" % n] = row
            print("%2d %%  calls of %4d  stream committee %9.3f ms [%.3f, %.3f]  stream indexed %9.3f ms [%.3f, %.3f]  direct loop %11.3f ms  full round %8.3f ms [%.3f, %.3f]" % (
                percent, n, row["stream_committee"]["ms_median"], row["stream_committee"]["ms_min"], row["stream_committee"]["ms_max"], row["stream_indexed"]["ms_median"],
                row["stream_indexed"]["ms_min"], row["stream_indexed"]["ms_max"], row["direct_loop"]["ms_median"], row["direct_full_round"]["ms_median"],
                row["direct_full_round"]["ms_min"], row["direct_full_round"]["ms_max"]), flush=True)
        stats = vc.stats()
    out["shapes"]["%d_percent" % percent] = {"participation_percent": percent, "signers": s, "route": route, "rejected_items": int((expect_h == 0).sum()),
                                             "input_bytes_per_item": {"stream_committee": 96 + 4 + 4 + BITS_LEN, "stream_indexed": 96 + 4 + 4 * s},
                                             "gathered_bytes_per_item": stats["gathered_bytes"] / stats["items"], "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:                                                         # (kept current shape by shape)
        json.dump(out, fh, indent=1); fh.write("\n")
ct.close(); mt.close(); table.close()
# ---- the gather alone, where the probe's output lies beside this file (scripts/dbg/gather_cmt_probe.hip), and bench.py against the parent commit
d = os.path.dirname(os.path.abspath(OUT))
if os.path.exists(os.path.join(d, "stream_committee_gather.json")):
    with open(os.path.join(d, "stream_committee_gather.json")) as fh:
        out["gather"] = json.load(fh)
lines = {}
for who in ("parent", "this_tree"):
    path = os.path.join(d, "bench_stream_committee_%s.jsonl" % who)
    if os.path.exists(path):
        with open(path) as fh:
            lines[who] = [round(json.loads(l)["ms_per_step"], 4) for l in fh if l.strip()]
if len(lines) == 2:
    out["bench_vs_parent"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5 of the parent commit and of this tree, alternated (full lines: "
                                      "bench_stream_committee_parent.jsonl, bench_stream_committee_this_tree.jsonl beside this file)",
                              "parent_ms_per_step": lines["parent"], "this_tree_ms_per_step": lines["this_tree"]}
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1); fh.write("\n")
print("wrote", OUT)
