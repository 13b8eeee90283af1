"""One host call of mbls_fast_aggregate_verify_batch at 2^16 items x 128 keys, 96-byte keys in pageable host memory: the entry whose key upload runs behind the
signature and message phases (verify_host, csrc/mbls_kernels.hip) -- bench.py times the device entries and never sees it. The batch is bench.py's (every 16th item
corrupted); one warm-up call, then CALLS timed calls, a host clock around each (the call returns when the results are in host memory); every call's results are
checked against the expectation.
usage: python scripts/host_entry_time.py LABEL [OUT.json]   (default: profiles/host_entry_time.json; the label's entry of OUT is replaced, the others are kept;
HET_ITEMS, default 65536; HET_CALLS, default 5)"""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

LABEL = sys.argv[1]
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "host_entry_time.json")
NI = int(os.environ.get("HET_ITEMS", "65536")); K = 128
CALLS = int(os.environ.get("HET_CALLS", "5"))
lib = N.lib(); ctx = N.default_context(); dev = torch.device("cuda:0")
d_sigs, d_msgs, d_pks, expect = bench.build_inputs(ctx, dev, NI, K, N.PK_UNCOMPRESSED, 0)
sigs, msgs, pks = (np.ascontiguousarray(t.cpu().numpy()) for t in (d_sigs, d_msgs, d_pks))
del d_sigs, d_msgs, d_pks
torch.cuda.empty_cache()
want = expect.numpy().astype(np.uint8)
res = np.zeros(NI, dtype=np.uint8)
vp = lambda a: a.ctypes.data_as(C.c_void_p)


def call():
    res.fill(7)
    t = time.perf_counter()
    rc = lib.mbls_fast_aggregate_verify_batch(ctx.handle, vp(sigs), vp(msgs), 32, None, vp(pks), N.PK_UNCOMPRESSED, None, NI, K, vp(res), None)
    dt = time.perf_counter() - t
    ctx.check(rc)
    assert (res == want).all()
    return 1e3 * dt


call()
ms = [round(call(), 3) for _ in range(CALLS)]
row = {"entry": "mbls_fast_aggregate_verify_batch", "items": NI, "keys_per_item": K, "pk_format": "uncompressed", "key_bytes": int(pks.nbytes), "host_memory": "pageable",
       "warmup_calls": 1, "ms_per_call": ms, "ms_median": round(statistics.median(ms), 3), "ms_min": min(ms), "ms_max": max(ms),
       "round_items": int(ctx.limits().round_items), "library_source_hash": bench.library_source_hash()}
out = {}
if os.path.exists(OUT):
    with open(OUT) as fh:
        out = json.load(fh)
out[LABEL] = row
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(LABEL, json.dumps(row))
