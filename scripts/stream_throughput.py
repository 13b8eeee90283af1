"""Sustained throughput of a flow of calls smaller than a round (a node's view), 128 keys per item, 32-byte messages, device-resident inputs:
(a) the direct device entry on one context, (b) the two-context recipe (calls alternate between two contexts and two streams), (c) the verification
stream with 96-byte keys under both launch policies, (d) the stream over key-table indices, (e) host submits over key-table indices. Every result is
checked against the expectation. Plus the latency of one lone 1 024-item call, submit to wait, against the direct entry.
usage: python scripts/stream_throughput.py [OUT.json]   (default: stream_throughput.json in the working directory)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N
from milagro_bls_amd.stream import VerifyStream

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else "stream_throughput.json"
MIN_S = float(os.environ.get("STREAM_MIN_SECONDS", "1.0"))
k, NB = 128, 1 << 16
ctx0, ctx1 = N.Context(0), N.Context(0)
s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
d_sigs, d_msgs, d_pks, expect, d_idx, table = bench.build_inputs(ctx0, dev, NB, k, N.PK_UNCOMPRESSED, rank=23, return_indices=True)
h_sigs, h_msgs, h_idx = d_sigs.cpu().numpy(), d_msgs.cpu().numpy(), d_idx.cpu().numpy().view(np.uint32)
for c in (ctx0, ctx1):
    c.reserve(NB)
sizes = [1024, 4096, 16384, 40960]
out = {"k": k, "msg_len": 32, "round_items": int(ctx0.limits().round_items), "min_seconds": MIN_S, "rows": {}}


def windows(n, calls):
    """call j covers items [a_j, a_j + n) of the 2^16-item inputs (contiguous, wrapping at a multiple of n)"""
    per = NB // n
    return [(j % per) * n for j in range(calls)]


def run_direct(n, calls, nctx):
    res = torch.zeros((calls, n), dtype=torch.uint8, device=dev)
    starts = windows(n, calls)
    torch.cuda.synchronize(); t = time.perf_counter()
    for j, a in enumerate(starts):
        c, s = (ctx0, s0) if nctx == 1 or j % 2 == 0 else (ctx1, s1)
        c.check(lib.mbls_fast_aggregate_verify_batch_device(c.handle, d_sigs[a].data_ptr(), d_msgs[a].data_ptr(), 32, None, d_pks[a].data_ptr(), N.PK_UNCOMPRESSED, None,
                                                            n, k, res[j].data_ptr(), None, None, s.cuda_stream))
    torch.cuda.synchronize(); dt = time.perf_counter() - t
    for j, a in enumerate(starts):
        assert torch.equal(res[j].cpu(), expect[a:a + n]), ("direct", n, j)
    return dt


def run_stream(n, calls, policy, indexed, host=False):
    res = torch.zeros((calls, n), dtype=torch.uint8, device=dev)
    starts = windows(n, calls)
    with VerifyStream(ctx0, pk_format=N.PK_UNCOMPRESSED, table=table if indexed else None, policy=policy) as vs:
        torch.cuda.synchronize(); t = time.perf_counter()
        if host:
            ts = [vs.submit(h_sigs[a:a + n], h_msgs[a:a + n], h_idx[a:a + n], n, k, msg_len=32) for a in starts]
            vs.flush()
            got = [x.result()[0] for x in ts]
        else:
            keys = d_idx if indexed else d_pks
            ts = [vs.submit_device(d_sigs[a], d_msgs[a], keys[a], n, k, res[j], msg_len=32) for j, a in enumerate(starts)]
            vs.flush()
            vs.wait(ts[-1])
        dt = time.perf_counter() - t
        st = vs.stats()
    for j, a in enumerate(starts):
        g = torch.frombuffer(bytearray(got[j]), dtype=torch.uint8) if host else res[j].cpu()
        assert torch.equal(g, expect[a:a + n]), ("stream", n, j, policy, indexed, host)
    return dt, st


def row(fn, n, *a):
    """calls enough for MIN_S seconds of work (one warm-up pass sizes it), median of 3"""
    fn(n, 4, *a)
    probe = fn(n, 16, *a); probe = probe[0] if isinstance(probe, tuple) else probe
    calls = max(16, int(MIN_S / (probe / 16)) + 1)
    ts, st = [], None
    for _ in range(3):
        r = fn(n, calls, *a)
        if isinstance(r, tuple):
            r, st = r
        ts.append(r)
    dt = float(np.median(ts))
    d = {"calls": calls, "seconds": round(dt, 3), "seconds_all": [round(t, 5) for t in ts],"items_per_s": round(calls * n / dt)}
    if st:
        d["stats"] = st
    return d


ONLY = os.environ.get("STREAM_ONLY", "")   # comma-separated substrings of "^<items per call>/<row name>$": the rows to run (default all)
ROWS = [("a_direct_1ctx", run_direct, (1,)), ("b_direct_2ctx", run_direct, (2,)), ("c_stream_u96_work_conserving", run_stream, (N.STREAM_WORK_CONSERVING, False)),
        ("c_stream_u96_full_rounds", run_stream, (N.STREAM_FULL_ROUNDS, False)), ("d_stream_indexed", run_stream, (N.STREAM_WORK_CONSERVING, True)),
        ("e_stream_host_indexed", run_stream, (N.STREAM_WORK_CONSERVING, True, True))]
for n in sizes:
    r = {}
    for name, fn, a in ROWS:
        if (name != "e_stream_host_indexed" or n >= 4096) and (not ONLY or any(p in "^%d/%s$" % (n, name) for p in ONLY.split(","))):
            r[name] = row(fn, n, *a)
    if not r:
        continue
    out["rows"][str(n)] = r
    print(n, json.dumps({kk: v["items_per_s"] for kk, v in r.items()}), flush=True)

# latency of one lone 1 024-item call, submit to wait (work-conserving: it starts at once), against the direct entry
n = 1024
res = torch.zeros(n, dtype=torch.uint8, device=dev)
lat = {"direct_ms": [], "stream_ms": []}
with VerifyStream(ctx0, pk_format=N.PK_UNCOMPRESSED) as vs:
    for rep in range(7):
        torch.cuda.synchronize(); t = time.perf_counter()
        ctx0.check(lib.mbls_fast_aggregate_verify_batch_device(ctx0.handle, d_sigs.data_ptr(), d_msgs.data_ptr(), 32, None, d_pks.data_ptr(), N.PK_UNCOMPRESSED, None,
                                                               n, k, res.data_ptr(), None, None, s0.cuda_stream))
        s0.synchronize(); lat["direct_ms"].append((time.perf_counter() - t) * 1e3)
        assert torch.equal(res.cpu(), expect[:n])
        res.zero_(); torch.cuda.synchronize(); t = time.perf_counter()
        vs.wait(vs.submit_device(d_sigs, d_msgs, d_pks, n, k, res, msg_len=32))
        lat["stream_ms"].append((time.perf_counter() - t) * 1e3)
        assert torch.equal(res.cpu(), expect[:n])
out["lone_1024"] = {kk: round(float(np.median(v[1:])), 3) for kk, v in lat.items()}
out["lone_1024"]["stream_minus_direct_ms"] = round(out["lone_1024"]["stream_ms"] - out["lone_1024"]["direct_ms"], 3)
print(json.dumps(out["lone_1024"]))
if os.path.dirname(OUT):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
