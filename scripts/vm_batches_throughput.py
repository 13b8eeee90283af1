"""Many small verify_multiple batches: ONE mbls_verify_multiple_batches_device call against (a) a loop of mbls_verify_multiple_aggregate_signatures_device over
the batches with one synchronisation at the end and (b) ONE mbls_verify_multiple_aggregate_signatures_device call over all sets as a single batch (the floor:
the same per-set work, one tail). Aggregate-key form, 32-byte messages, all sets valid, device-resident inputs; every result is checked.
Same process, same inputs, same timing method for the three variants: a host clock around work that ends in a device synchronise, every shape warmed up, the
variants alternated inside every round, medians over the rounds with the spread beside them. A window holds as many repetitions as make it about a quarter
of a second (one for the loops at the large shapes).
usage: python scripts/vm_batches_throughput.py [OUT.json]   (default: profiles/vm_batches_throughput.json; VMB_ROUNDS, default 10)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_batches_throughput.json")
ROUNDS = int(os.environ.get("VMB_ROUNDS", "10"))
WINDOW_S = 0.25
SHAPES = [(16, 10), (128, 10), (1024, 10), (1024, 63), (64, 1000)]
NMAX = max(B * s for B, s in SHAPES)
ctx = N.default_context()
d_sigs, d_msgs, d_apks, _ = bench.build_inputs(ctx, dev, NMAX, 1, N.PK_UNCOMPRESSED, rank=31, negatives=False)
rng = np.random.default_rng(31)
d_rands = torch.from_numpy(rng.integers(1, 1 << 62, size=NMAX, dtype=np.int64)).to(dev)
ctx.reserve(2 * NMAX + 4096)
P = lambda t: t.data_ptr()


def one_call(B, spb, res):
    ctx.check(lib.mbls_verify_multiple_batches_device(ctx.handle, P(d_sigs), P(d_apks), None, 0, None, 0, P(d_msgs), 32, None, P(d_rands), B * spb, None, spb, B,
                                                      P(res), None, None))


def loop(B, spb, res):
    for b in range(B):
        lo = b * spb
        ctx.check(lib.mbls_verify_multiple_aggregate_signatures_device(ctx.handle, P(d_sigs) + 96 * lo, P(d_apks) + 96 * lo, P(d_msgs) + 32 * lo, 32, None,
                                                                       P(d_rands) + 8 * lo, spb, P(res) + b, None, None))


def floor(B, spb, res):
    ctx.check(lib.mbls_verify_multiple_aggregate_signatures_device(ctx.handle, P(d_sigs), P(d_apks), P(d_msgs), 32, None, P(d_rands), B * spb, P(res), None, None))


VARIANTS = (("one_call", one_call, lambda B: B), ("loop", loop, lambda B: B), ("floor", floor, lambda B: 1))


def window(f, B, spb, res, reps):
    res.fill_(7)
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        f(B, spb, res)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


out = {"form": "aggregate keys, 32-byte messages, all sets valid, device-resident", "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition; median [min, max] over the rounds",
       "round_items": int(ctx.limits().round_items), "shapes": {}}
for B, spb in SHAPES:
    res = torch.full((max(B, 8),), 7, dtype=torch.uint8, device=dev)
    reps, times = {}, {}
    for name, f, nres in VARIANTS:                      # warm-up: every variant at this shape, results checked
        window(f, B, spb, res, 1)
        est = window(f, B, spb, res, 1)
        assert bool((res[:nres(B)] == 1).all()), (name, B, spb, res[:16].tolist())
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
        times[name] = []
    for _ in range(ROUNDS):
        for name, f, nres in VARIANTS:                  # alternated inside the round
            times[name].append(1e3 * window(f, B, spb, res, reps[name]))
            assert bool((res[:nres(B)] == 1).all()), (name, B, spb)
    row = {"batches": B, "sets_per_batch": spb, "sets": B * spb}
    for name, _, _ in VARIANTS:
        row[name] = {"ms_median": round(statistics.median(times[name]), 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4), "reps_per_window": reps[name]}
    row["loop_over_one_call"] = round(row["loop"]["ms_median"] / row["one_call"]["ms_median"], 2)
    row["one_call_over_floor"] = round(row["one_call"]["ms_median"] / row["floor"]["ms_median"], 2)
    out["shapes"]["%dx%d" % (B, spb)] = row
    print("%5d x %4d  one call %9.3f ms   loop %10.3f ms (x %.1f)   floor %8.3f ms (one call / floor %.2f)" % (
        B, spb, row["one_call"]["ms_median"], row["loop"]["ms_median"], row["loop_over_one_call"], row["floor"]["ms_median"], row["one_call_over_floor"]), flush=True)
sh = out["shapes"]
out["conditions"] = {
    "one_call_not_slower_than_loop_at_every_shape": all(r["one_call"]["ms_median"] <= r["loop"]["ms_median"] for r in sh.values()),
    "one_call_at_least_10x_faster_than_loop_at_1024x63": sh["1024x63"]["loop_over_one_call"] >= 10.0,
    "reported_not_gated": {"one_call_over_floor_1024x63": sh["1024x63"]["one_call_over_floor"], "one_call_over_floor_64x1000": sh["64x1000"]["one_call_over_floor"]},
}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out["conditions"]))
sys.exit(0 if out["conditions"]["one_call_not_slower_than_loop_at_every_shape"] and out["conditions"]["one_call_at_least_10x_faster_than_loop_at_1024x63"] else 1)
