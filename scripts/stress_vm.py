"""Randomised verify_multiple batches against the CPU oracle (the cases of tests/stress_cases.py, which tests/test_gpu_stress_slices.py runs on one
seed): random sizes 1 .. 48 sets (the lane-pair signature chain) and a few mid-size ones, random members replaced by a wrong / infinite / non-subgroup
signature, an infinite or wrong key, a zero scalar -- through the one-call entry with the caller's scalar source (result AND number of scalars asked
for, reference src/aggregates.rs:272-287), the entry that takes the scalars, and the device entry.
usage: stress_vm.py [n_batches] [seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, q)
import torch
import stress_cases as sc
from milagro_bls_amd import _native as N
ctx = N.default_context(); dev = torch.device("cuda:0")
count = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
t0 = time.time()
(batches, sets), mismatches = sc.run_vm(ctx, dev, count, seed)
for m in mismatches:
    print("MISMATCH", m, flush=True)
print("batches", batches, "sets", sets, "mismatching batches", len(mismatches), "%.1f s" % (time.time() - t0))
sys.exit(1 if mismatches else 0)
