"""Randomised GPU-vs-oracle stress over many seeds (dev tool; the cases of tests/stress_cases.py, which tests/test_gpu_stress_slices.py runs on a few
seeds): fast_aggregate_verify with batch sizes either side of every engine crossover -- each batch once with the default engines, once forced onto
the lane-pair kernels, once onto the two-pair loop of the headline and once onto the cooperative engine --, signing and sk -> pk; verify_multiple (one
call, cut into random shards, behind a two-context handle) and batched aggregate_verify with random members spoiled, against the oracle.
usage: stress_parity.py [n_seeds] [big: 1 = the shapes above 2 048 items on every fourth seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "pymodel"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, q)
import torch
import helpers
import stress_cases as sc
from milagro_bls_amd import _native as N
ctx = N.default_context()
nt = helpers.oracle_threads()
bad = 0; total = 0; t0 = time.time()
nseeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
big = int(sys.argv[2]) if len(sys.argv) > 2 else 1


def report(work, mismatches):
    global bad, total
    total += work; bad += len(mismatches)
    for m in mismatches:
        print("MISMATCH", m, flush=True)


for seed in range(100, 100 + nseeds):
    report(*sc.run_fav_engines(ctx, seed, nt, big=bool(big)))
    report(*sc.run_sign_keys(ctx, seed, nt))
# the n-pairing paths: verify_multiple (one call, cut into shards through the device entries, behind a two-context handle) and batched aggregate_verify
dev = torch.device("cuda:0")
m2 = N.MultiContext([0, 0])
for seed in range(100, 100 + max(1, nseeds // 4)):
    report(*sc.run_vm_shards(ctx, m2, dev, seed, nt))
m2.close()
print("items", total, "mismatching batches", bad, "%.1f s" % (time.time() - t0))
sys.exit(1 if bad else 0)
