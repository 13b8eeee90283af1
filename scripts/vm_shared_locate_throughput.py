"""Which sets of a rejected call over a shared message list: ONE mbls_verify_multiple_shared_msgs_locate_device call against what a client does without it.
(a) all sets valid: the locate entry against mbls_verify_multiple_shared_msgs_device in the same run -- the price of the keeps (the blinded keys and signatures
    copied to the shadow items) and of phase two's launches, whose waves all return after one ballot.
(b) one bad set, and 1 % bad sets (wrong keys): the locate entry (one call, synchronise, read the bool and the per-set bytes) against the sequence a client runs
    today: mbls_verify_multiple_shared_msgs_device, synchronise, read the bool, and -- rejected -- mbls_verify_multiple_batches_locate_device with ONE batch over
    all n sets on the spelled-out messages (n hashes, n Miller loops), synchronise, read the per-set bytes. The spelled-out messages are device-resident before
    the clock starts: the host work of spelling them out is NOT charged to the sequence.
Shapes: 2^16 sets over 512 messages, 2^14 over 512, 1 024 over 8; auto routing (grouped at all three). One aggregate key per set, 32-byte messages,
device-resident inputs; every result is checked. Same process, same inputs, same timing method for all variants: a host clock around a window of repetitions,
each ending in a device synchronise and the read-back of its results, every shape warmed up, the variants alternated inside every round, medians over the
rounds with min and max beside them.
usage: python scripts/vm_shared_locate_throughput.py [OUT.json]   (default: profiles/vm_shared_locate_throughput.json; VSL_ROUNDS, default 10)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_shared_locate_throughput.json")
ROUNDS = int(os.environ.get("VSL_ROUNDS", "10"))
WINDOW_S = 0.2
SHAPES = [(65536, 512), (16384, 512), (1024, 8)]
ctx = N.default_context()
P = lambda t: t.data_ptr()
pool = bench.make_pool(bench.SEED)
POOL = len(pool)
d_pool_sk = torch.from_numpy(np.frombuffer(b"".join(s.to_bytes(32, "big") for s in pool), dtype=np.uint8).reshape(POOL, 32).copy()).to(dev)
d_pool_pk = torch.empty((POOL, 96), dtype=torch.uint8, device=dev)
ctx.check(lib.mbls_sk_to_pk_batch_device(ctx.handle, P(d_pool_sk), N.PK_UNCOMPRESSED, POOL, P(d_pool_pk), None))
L = ctx.limits()
ctx.reserve(max([N.plan_verify_multiple_shared_msgs_locate_workspace_items(n, m, 0, L) for n, m in SHAPES] + [N.plan_locate_workspace_items(n, 1, L) for n, _ in SHAPES]))
ctx.reserve_msgs(max(m for _, m in SHAPES))
ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, 0))


def window(f, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        got = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, got


def measure(variants, check):
    reps, times = {}, {name: [] for name, _ in variants}
    for name, f in variants:                                # warm-up: every variant at this shape, results checked
        window(f, 1)
        est, got = window(f, 1)
        check(name, got)
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
    for _ in range(ROUNDS):
        for name, f in variants:                            # alternated inside the round
            s, got = window(f, reps[name])
            times[name].append(1e3 * s)
            check(name, got)
    return {name: {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "reps_per_window": reps[name]}
            for name, t in times.items()}


out = {"form": "device-resident inputs (the spelled-out messages of the two-step sequence included), one aggregate key per set, 32-byte messages, auto routing",
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions, each ending in a device synchronise and the read-back of its results; ms per repetition; "
                 "median [min, max] over the rounds",
       "variants": {"shared": "mbls_verify_multiple_shared_msgs_device, the bool read back",
                    "locate": "mbls_verify_multiple_shared_msgs_locate_device, the bool and the per-set bytes read back",
                    "two_step": "shared, the bool read back, then (rejected) mbls_verify_multiple_batches_locate_device with one batch on the spelled-out messages, "
                                "the per-set bytes read back"},
       "round_items": int(L.round_items), "shapes": {}}
for n, n_msgs in SHAPES:
    rng = np.random.default_rng(7000 + n + n_msgs)
    h_who = rng.integers(0, POOL, size=n, dtype=np.int64)
    who = torch.from_numpy(h_who).to(dev)
    d_good_apks = d_pool_pk[who].contiguous(); d_sk = d_pool_sk[who].contiguous()
    d_list = torch.from_numpy(rng.integers(0, 256, size=(n_msgs, 32), dtype=np.uint8)).to(dev)
    named = rng.integers(0, n_msgs, size=n, dtype=np.int64)
    d_spelled = d_list[torch.from_numpy(named).to(dev)].contiguous()
    d_sigs = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_spelled), 32, n, P(d_sigs), None))
    d_midx = torch.from_numpy(named.astype(np.int32)).to(dev)
    d_rands = torch.from_numpy(rng.integers(1, 1 << 63, size=n, dtype=np.int64)).to(dev)
    d_res = torch.full((8,), 7, dtype=torch.uint8, device=dev); d_sres = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    plan = N.plan_verify_multiple_shared_msgs(n, n_msgs, 0, L)
    row = {"sets": n, "n_msgs": n_msgs, "route": "grouped" if plan["route"] == N.VM_ROUTE_GROUPED else "per_set",
           "workspace_items": {"shared": int(plan["workspace_items"]), "locate": N.plan_verify_multiple_shared_msgs_locate_workspace_items(n, n_msgs, 0, L)}}
    for label, n_bad in (("all_valid", 0), ("one_bad", 1), ("bad_1_percent", max(1, n // 100))):
        bad = np.sort(rng.choice(n, size=n_bad, replace=False)) if n_bad else np.zeros(0, dtype=np.int64)
        d_apks = d_good_apks.clone()
        if n_bad:                                           # a bad set carries the pool's next key
            d_apks[torch.from_numpy(bad).to(dev)] = d_pool_pk[torch.from_numpy((h_who[bad] + 1) % POOL).to(dev)]
        want_s = np.ones(n, dtype=np.uint8); want_s[bad] = 0
        want = 0 if n_bad else 1

        def shared():
            ctx.check(lib.mbls_verify_multiple_shared_msgs_device(ctx.handle, P(d_sigs), P(d_apks), P(d_list), 32, None, n_msgs, P(d_midx), P(d_rands), n, P(d_res), None, None))
            torch.cuda.synchronize()
            return int(d_res[0].item()), None

        def locate():
            ctx.check(lib.mbls_verify_multiple_shared_msgs_locate_device(ctx.handle, P(d_sigs), P(d_apks), P(d_list), 32, None, n_msgs, P(d_midx), P(d_rands), n, P(d_res),
                                                                         None, P(d_sres), None, None))
            torch.cuda.synchronize()
            return int(d_res[0].item()), d_sres.cpu().numpy()

        def two_step():
            ok, _ = shared()
            if ok:
                return ok, np.ones(n, dtype=np.uint8)
            ctx.check(lib.mbls_verify_multiple_batches_locate_device(ctx.handle, P(d_sigs), P(d_apks), None, 0, None, 0, P(d_spelled), 32, None, P(d_rands), n, None, n, 1,
                                                                     P(d_res), None, P(d_sres), None, None))
            torch.cuda.synchronize()
            return ok, d_sres.cpu().numpy()

        def check(name, got):
            ok, per_set = got
            assert ok == want, (n, n_msgs, label, name, ok)
            assert per_set is None or (per_set == want_s).all(), (n, n_msgs, label, name, np.flatnonzero(per_set != want_s)[:8].tolist())
        if n_bad:
            r = measure((("two_step", two_step), ("locate", locate)), check)
            r["bad_sets"] = int(n_bad)
            r["two_step_over_locate"] = round(r["two_step"]["ms_median"] / r["locate"]["ms_median"], 3)
            print("%6d sets %4d msgs  %-13s (%4d bad): two step %8.3f ms [%.3f, %.3f]   locate %8.3f ms [%.3f, %.3f]   two step / locate %.3f" % (
                n, n_msgs, label, n_bad, r["two_step"]["ms_median"], r["two_step"]["ms_min"], r["two_step"]["ms_max"], r["locate"]["ms_median"], r["locate"]["ms_min"],
                r["locate"]["ms_max"], r["two_step_over_locate"]), flush=True)
        else:
            r = measure((("shared", shared), ("locate", locate)), check)
            r["locate_minus_shared_ms"] = round(r["locate"]["ms_median"] - r["shared"]["ms_median"], 4)
            r["shared_spread_ms"] = round(r["shared"]["ms_max"] - r["shared"]["ms_min"], 4)
            print("%6d sets %4d msgs  all valid: shared %8.3f ms [%.3f, %.3f]   locate %8.3f ms [%.3f, %.3f]   difference %+.3f ms (the baseline's spread: %.3f)" % (
                n, n_msgs, r["shared"]["ms_median"], r["shared"]["ms_min"], r["shared"]["ms_max"], r["locate"]["ms_median"], r["locate"]["ms_min"], r["locate"]["ms_max"],
                r["locate_minus_shared_ms"], r["shared_spread_ms"]), flush=True)
        row[label] = r
    out["shapes"]["%d/%d" % (n, n_msgs)] = row
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
