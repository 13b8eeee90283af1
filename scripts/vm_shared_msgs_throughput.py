"""verify_multiple over a shared message list: mbls_verify_multiple_shared_msgs_device (the list hashed once; grouped route: one Miller loop per message) against
mbls_verify_multiple_aggregate_signatures_device on the same sets with every set's message spelled out -- the baseline: today's behaviour, measured in the same
run. Shapes: 2^16 sets over 1, 64, 512, 4 096, 2^15, 3 x 2^14 and 2^16 messages, 2^14 sets over 64 and 512, 1 024 sets over 8; at every shape the auto route and the two
forced routes (mode 1: always grouped, mode 2: never -- the list hashed once, every set gathers its point and walks its own Miller loop), so that the crossover
of the auto condition can be read off. One aggregate key per set, 32-byte messages, device-resident inputs.
Same process, same inputs, same timing method for all variants: a host clock around a window of repetitions that ends in a device synchronise, every shape
warmed up, the variants alternated inside every round, medians over the rounds with min and max beside them. Every result is checked: the batch is valid (result
byte 1 after every window), and once per shape a copy in which one set names another message must be rejected by every variant.
usage: python scripts/vm_shared_msgs_throughput.py [OUT.json]   (default: profiles/vm_shared_msgs_throughput.json; VSMT_ROUNDS, default 10)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_shared_msgs_throughput.json")
ROUNDS = int(os.environ.get("VSMT_ROUNDS", "10"))
WINDOW_S = 0.2
SHAPES = [(65536, 1), (65536, 64), (65536, 512), (65536, 4096), (65536, 32768), (65536, 49152), (65536, 65536), (16384, 64), (16384, 512), (1024, 8)]
ctx = N.default_context()
P = lambda t: t.data_ptr()
pool = bench.make_pool(bench.SEED)
POOL = len(pool)
d_pool_sk = torch.from_numpy(np.frombuffer(b"".join(s.to_bytes(32, "big") for s in pool), dtype=np.uint8).reshape(POOL, 32).copy()).to(dev)
d_pool_pk = torch.empty((POOL, 96), dtype=torch.uint8, device=dev)
ctx.check(lib.mbls_sk_to_pk_batch_device(ctx.handle, P(d_pool_sk), N.PK_UNCOMPRESSED, POOL, P(d_pool_pk), None))


def window(f, reps, d_res):
    d_res.fill_(7)
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


out = {"form": "device-resident inputs, one aggregate key per set, 32-byte messages, valid batches (result 1 checked after every window; a copy with one set renamed "
               "to another message is rejected by every variant)",
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per call; median [min, max] over the rounds",
       "variants": {"baseline": "mbls_verify_multiple_aggregate_signatures_device, messages spelled out per set", "auto": "mbls_verify_multiple_shared_msgs_device, mode 0",
                    "grouped": "mode 1: one Miller loop per message", "per_set": "mode 2: list hashed once, one Miller loop per set"},
       "round_items": int(ctx.limits().round_items), "shapes": {}}
L = ctx.limits()
ctx.reserve(max(N.plan_verify_multiple_shared_msgs_workspace_items(n, m, 1, L) for n, m in SHAPES)); ctx.reserve_msgs(max(m for _, m in SHAPES))
for n, n_msgs in SHAPES:
    rng = np.random.default_rng(5000 + n + n_msgs)
    who = torch.from_numpy(rng.integers(0, POOL, size=n, dtype=np.int64)).to(dev)
    d_apks = d_pool_pk[who].contiguous(); d_sk = d_pool_sk[who].contiguous()
    d_list = torch.from_numpy(rng.integers(0, 256, size=(n_msgs, 32), dtype=np.uint8)).to(dev)
    named = np.arange(n, dtype=np.int64) % n_msgs if n_msgs >= n else rng.integers(0, n_msgs, size=n, dtype=np.int64)
    d_spelled = d_list[torch.from_numpy(named).to(dev)].contiguous()
    d_sigs = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_spelled), 32, n, P(d_sigs), None))
    d_midx = torch.from_numpy(named.astype(np.int32)).to(dev)
    d_rands = torch.from_numpy(rng.integers(1, 1 << 63, size=n, dtype=np.int64)).to(dev)
    d_res = torch.full((8,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def shared(mode, midx=d_midx):
        def f():
            ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, mode))
            ctx.check(lib.mbls_verify_multiple_shared_msgs_device(ctx.handle, P(d_sigs), P(d_apks), P(d_list), 32, None, n_msgs, P(midx), P(d_rands), n, P(d_res), None, None))
        return f

    def baseline(spelled=d_spelled):
        return lambda: ctx.check(lib.mbls_verify_multiple_aggregate_signatures_device(ctx.handle, P(d_sigs), P(d_apks), P(spelled), 32, None, P(d_rands), n, P(d_res), None, None))
    variants = (("baseline", baseline()), ("auto", shared(0)), ("grouped", shared(1)), ("per_set", shared(2)))
    if n_msgs > 1:                                          # the negative check: set 5 names the next message
        bad = named.copy(); bad[5] = (bad[5] + 1) % n_msgs
        d_bad_idx = torch.from_numpy(bad.astype(np.int32)).to(dev); d_bad_sp = d_list[torch.from_numpy(bad).to(dev)].contiguous()
        for name, f in (("baseline", baseline(d_bad_sp)), ("auto", shared(0, d_bad_idx)), ("grouped", shared(1, d_bad_idx)), ("per_set", shared(2, d_bad_idx))):
            window(f, 1, d_res)
            assert int(d_res[0].item()) == 0, (n, n_msgs, name, "accepted a set that names another message")
    reps, times = {}, {}
    for name, f in variants:                                # warm-up: every variant at this shape, results checked
        window(f, 1, d_res)
        est = window(f, 1, d_res)
        assert int(d_res[0].item()) == 1, (n, n_msgs, name)
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
        times[name] = []
    for _ in range(ROUNDS):
        for name, f in variants:                            # alternated inside the round
            times[name].append(1e3 * window(f, reps[name], d_res))
            assert int(d_res[0].item()) == 1, (n, n_msgs, name)
    plan = N.plan_verify_multiple_shared_msgs(n, n_msgs, 0, L)
    row = {"sets": n, "n_msgs": n_msgs, "auto_route": "grouped" if plan["route"] == N.VM_ROUTE_GROUPED else "per_set"}
    for name, _ in variants:
        row[name] = {"ms_median": round(statistics.median(times[name]), 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
                     "reps_per_window": reps[name]}
    row["baseline_spread_ms"] = round(row["baseline"]["ms_max"] - row["baseline"]["ms_min"], 4)
    row["auto_saved_ms"] = round(row["baseline"]["ms_median"] - row["auto"]["ms_median"], 4)
    row["auto_over_baseline"] = round(row["auto"]["ms_median"] / row["baseline"]["ms_median"], 4)
    row["auto_within_baseline_spread"] = bool(row["auto"]["ms_median"] <= row["baseline"]["ms_median"] + row["baseline_spread_ms"])
    out["shapes"]["%d/%d" % (n, n_msgs)] = row
    print("%6d sets %6d msgs   baseline %8.3f [%.3f, %.3f]   auto(%s) %8.3f   grouped %8.3f   per set %8.3f   auto saves %7.3f ms (x %.3f)%s" % (
        n, n_msgs, row["baseline"]["ms_median"], row["baseline"]["ms_min"], row["baseline"]["ms_max"], row["auto_route"], row["auto"]["ms_median"],
        row["grouped"]["ms_median"], row["per_set"]["ms_median"], row["auto_saved_ms"], row["auto_over_baseline"],
        "" if row["auto_within_baseline_spread"] else "   AUTO SLOWER THAN THE BASELINE'S SPREAD ALLOWS"), flush=True)
ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, 0))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
