"""Randomised sizes above a round through the device entries (two-track routes: the remainder beside the round, equal halves, rounds in front) against the
expectation by construction (bench.build_inputs: every 16th item corrupted over five rejection classes) -- every result, bitmap bit and status class --,
byte keys and table indices, with and without a bitmap and a status array (the cases of tests/stress_cases.py, which tests/test_gpu_stress_slices.py runs
on one seed, with an oracle sample of the round seams and the tail).
usage: stress_tracks.py [n_sizes] [seed] [oracle items per size, 0 = none]"""
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
oracle_count = int(sys.argv[3]) if len(sys.argv) > 3 else 0
inp = sc.TrackInputs(ctx, dev)
t0 = time.time()
(sizes, items), mismatches = sc.run_tracks(ctx, dev, inp, count, seed, oracle_count=oracle_count)
for m in mismatches:
    print("MISMATCH", m, flush=True)
print("sizes", sizes, "items", items, "mismatching batches", len(mismatches), "%.1f s" % (time.time() - t0))
sys.exit(1 if mismatches else 0)
