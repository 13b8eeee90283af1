"""A short verification-stream run for a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/stream_kernel_trace.py): ROUNDS full
rounds, each packed from sixteen 4 096-item calls of 128 uncompressed keys, in full-rounds mode. Every result is checked."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from milagro_bls_amd import _native as N
from milagro_bls_amd.stream import VerifyStream

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
dev = torch.device("cuda:0")
ctx = N.default_context()
n, k = 4096, 128
d_sigs, d_msgs, d_pks, expect = bench.build_inputs(ctx, dev, 16 * n, k, N.PK_UNCOMPRESSED, rank=77)
res = torch.zeros((16 * ROUNDS, n), dtype=torch.uint8, device=dev)
with VerifyStream(ctx, pk_format=N.PK_UNCOMPRESSED, policy=N.STREAM_FULL_ROUNDS) as vs:
    ts = [vs.submit_device(d_sigs[(j % 16) * n], d_msgs[(j % 16) * n], d_pks[(j % 16) * n], n, k, res[j], msg_len=32) for j in range(16 * ROUNDS)]
    vs.wait(ts[-1])
    st = vs.stats()
for j in range(16 * ROUNDS):
    assert torch.equal(res[j].cpu(), expect[(j % 16) * n:(j % 16) * n + n])
print("stream kernel trace: %d rounds (%d full), %d calls, %.1f MB gathered per round" % (st["rounds"], st["full_rounds"], st["calls"], st["gathered_bytes"] / st["rounds"] / 1e6))
