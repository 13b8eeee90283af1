"""Batches whose items share messages: the *_shared_msgs device entries (the list hashed once, one index per item) against the entries that take one message per
item (the baseline: today's behaviour, measured in the same run on the same items with their messages spelled out). Shapes: 2^16 items x 128 keys through a
resident key table (mbls_fast_aggregate_verify_batch_indexed[_shared_msgs]_device) and 2^16 items x 1 key (mbls_verify_batch[_shared_msgs]_device), each over
lists of 1, 64, 512, 4096 and 2^16 messages (the last with identity indices: what the new entry costs when nothing is shared). Device-resident inputs.
Same process, same inputs, same timing method for both variants: a host clock around a window of repetitions that ends in a device synchronise, every shape warmed
up, the variants alternated inside every round, medians over the rounds with the spread beside them. Every result is checked: every 16th item (i % 16 == 7) names
another message than its signers saw (lists of more than one message) and must be rejected by both variants, every other item accepted.
usage: python scripts/shared_msgs_throughput.py [OUT.json]   (default: profiles/shared_msgs_throughput.json; SMT_ROUNDS, default 10; SMT_ITEMS, default 65536)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "shared_msgs_throughput.json")
ROUNDS = int(os.environ.get("SMT_ROUNDS", "10"))
NI = int(os.environ.get("SMT_ITEMS", "65536"))
WINDOW_S = 0.25
LISTS = [1, 64, 512, 4096, NI]
ctx = N.default_context()
P = lambda t: t.data_ptr()
pool = bench.make_pool(bench.SEED)
POOL = len(pool)
limbs = np.array([[(sk >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for sk in pool], dtype=np.uint64)
d_pool_sk = torch.from_numpy(np.frombuffer(b"".join(s.to_bytes(32, "big") for s in pool), dtype=np.uint8).reshape(POOL, 32).copy()).to(dev)


def keys_of(k, seed):
    """item i's k pool keys (distinct: odd stride) and its aggregate secret key"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, POOL, size=NI, dtype=np.int64)
    s = rng.integers(0, POOL // 2, size=NI, dtype=np.int64) * 2 + 1
    idx = (a[:, None] + np.arange(k, dtype=np.int64)[None, :] * s[:, None]) % POOL
    agg = np.zeros((NI, 8), dtype=np.uint64)
    for c0 in range(0, NI, 8192):
        agg[c0:c0 + 8192] = limbs[idx[c0:c0 + 8192]].sum(axis=1)
    sk = np.zeros((NI, 32), dtype=np.uint8)
    for i in range(NI):
        v = sum(int(agg[i, j]) << (32 * j) for j in range(8)) % bench.R
        sk[i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    return idx, torch.from_numpy(sk).to(dev)


def window(f, reps, d_res):
    d_res.fill_(7)
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


out = {"form": "device-resident inputs, 32-byte messages; item i %% 16 == 7 names another message than was signed (rejected), the others are valid; items = %d" % NI,
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition; median [min, max] over the rounds",
       "round_items": int(ctx.limits().round_items), "shapes": {}}
ctx.reserve(max(N.plan_shared_msgs_workspace_items(NI, m, 128, True, ctx.limits()) for m in LISTS)); ctx.reserve_msgs(NI)
for shape, k in (("indexed_128_keys", 128), ("verify_1_key", 1)):
    idx, d_sk = keys_of(k, 77 + k)
    table = None
    if k > 1:
        d_pool_pk = torch.empty((POOL, 96), dtype=torch.uint8, device=dev)
        ctx.check(lib.mbls_sk_to_pk_batch_device(ctx.handle, P(d_pool_sk), N.PK_UNCOMPRESSED, POOL, P(d_pool_pk), None))
        table = N.KeyTable(ctx, capacity_hint=POOL)
        d_errs = torch.zeros(POOL, dtype=torch.uint8, device=dev)
        table.append_device(P(d_pool_pk), POOL, P(d_errs), pk_format=N.PK_UNCOMPRESSED, validate=False)
        torch.cuda.synchronize(); assert int(d_errs.max().item()) == 0
        d_keys = torch.from_numpy(idx.astype(np.uint32).view(np.int32)).to(dev)
    else:
        d_pool_pk = torch.empty((POOL, 48), dtype=torch.uint8, device=dev)
        ctx.check(lib.mbls_sk_to_pk_batch_device(ctx.handle, P(d_pool_sk), N.PK_COMPRESSED, POOL, P(d_pool_pk), None))
        d_keys = d_pool_pk[torch.from_numpy(idx[:, 0]).to(dev)].contiguous()
    d_res = torch.full((NI,), 7, dtype=torch.uint8, device=dev)
    for n_msgs in LISTS:
        rng = np.random.default_rng(1000 + n_msgs)
        d_list = torch.from_numpy(rng.integers(0, 256, size=(n_msgs, 32), dtype=np.uint8)).to(dev)
        signed = np.arange(NI, dtype=np.int64) % n_msgs if n_msgs == NI else rng.integers(0, n_msgs, size=NI, dtype=np.int64)
        named = signed.copy()
        if n_msgs > 1:
            named[7::16] = (named[7::16] + 1) % n_msgs
        expect = torch.from_numpy((named == signed).astype(np.uint8)).to(dev)
        d_signed_msgs = d_list[torch.from_numpy(signed).to(dev)].contiguous()
        d_sigs = torch.empty((NI, 96), dtype=torch.uint8, device=dev)
        ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_signed_msgs), 32, NI, P(d_sigs), None))
        d_midx = torch.from_numpy(named.astype(np.int32)).to(dev)
        d_spelled = d_list[torch.from_numpy(named).to(dev)].contiguous()          # the baseline's input: every item's message spelled out
        torch.cuda.synchronize()
        if k > 1:
            new = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_shared_msgs_device(ctx.handle, table.handle, P(d_sigs), P(d_list), 32, None, n_msgs, P(d_midx),
                                                                                                    P(d_keys), None, NI, k, P(d_res), None, None, None))
            old = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_device(ctx.handle, table.handle, P(d_sigs), P(d_spelled), 32, None, P(d_keys), None, NI, k,
                                                                                        P(d_res), None, None, None))
        else:
            new = lambda: ctx.check(lib.mbls_verify_batch_shared_msgs_device(ctx.handle, P(d_sigs), P(d_list), 32, None, n_msgs, P(d_midx), P(d_keys), N.PK_COMPRESSED, NI,
                                                                             P(d_res), None, None, None))
            old = lambda: ctx.check(lib.mbls_verify_batch_device(ctx.handle, P(d_sigs), P(d_spelled), 32, None, P(d_keys), N.PK_COMPRESSED, NI, P(d_res), None, None, None))
        variants = (("shared_msgs", new), ("per_item", old))
        reps, times = {}, {}
        for name, f in variants:                            # warm-up: both variants at this shape, results checked
            window(f, 1, d_res)
            est = window(f, 1, d_res)
            assert bool((d_res == expect).all()), (shape, n_msgs, name)
            reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
            times[name] = []
        for _ in range(ROUNDS):
            for name, f in variants:                        # alternated inside the round
                times[name].append(1e3 * window(f, reps[name], d_res))
                assert bool((d_res == expect).all()), (shape, n_msgs, name)
        row = {"items": NI, "keys_per_item": k, "n_msgs": n_msgs, "rejected_items": int((named != signed).sum())}
        for name, _ in variants:
            row[name] = {"ms_median": round(statistics.median(times[name]), 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
                         "reps_per_window": reps[name]}
        row["saved_ms"] = round(row["per_item"]["ms_median"] - row["shared_msgs"]["ms_median"], 4)
        row["shared_over_per_item"] = round(row["shared_msgs"]["ms_median"] / row["per_item"]["ms_median"], 4)
        row["per_item_spread_ms"] = round(row["per_item"]["ms_max"] - row["per_item"]["ms_min"], 4)
        out["shapes"]["%s/%d" % (shape, n_msgs)] = row
        print("%-17s n_msgs %6d   shared %8.3f ms   per item %8.3f ms [%.3f, %.3f]   saved %7.3f ms (x %.3f)" % (
            shape, n_msgs, row["shared_msgs"]["ms_median"], row["per_item"]["ms_median"], row["per_item"]["ms_min"], row["per_item"]["ms_max"], row["saved_ms"],
            row["shared_over_per_item"]), flush=True)
    if table is not None:
        table.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
