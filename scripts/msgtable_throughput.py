"""The resident message table (mbls_msgtable_*): the `_msgtable_device` entries (the table built before timing, no call hashes anything) against the `_shared_msgs`
entries (the list hashed inside every call) and the entries that take one message per item -- the two baselines are entries this table does not touch, measured in
the same process on the same items. Shapes: 2^16 items x 128 keys through a resident key table over 1, 512, 4096 and 2^16 messages; 2^16 items x 1 key
(Signature::verify) over 512 messages; a verification stream of 4096-item and 16384-item calls over 512 messages, message-table stream against the stream that
takes the messages; and the append itself for 512 and 4096 messages. Device-resident inputs.
Same timing method for every variant: a host clock around a window of repetitions that ends in a device synchronise (streams: in the wait for the last call), every
shape warmed up, the variants alternated inside every round, medians over the rounds with [min, max] beside them. Every result is checked: every 16th item
(i % 16 == 7) names another message than its signers saw (lists of more than one message) and must be rejected by every variant, every other item accepted.
usage: python scripts/msgtable_throughput.py [OUT.json]   (default: profiles/msgtable_throughput.json; MTT_ROUNDS, default 10; MTT_ITEMS, default 65536)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N, batch
from milagro_bls_amd.stream import VerifyStream

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "msgtable_throughput.json")
ROUNDS = int(os.environ.get("MTT_ROUNDS", "10"))
NI = int(os.environ.get("MTT_ITEMS", "65536"))
WINDOW_S = 0.25
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


def stat(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def measure(variants, d_res, expect, tag):
    """variants: [(name, f)] -> {name: stats}; warm-up, results checked after every window, the variants alternated inside every round"""
    reps, times = {}, {}
    for name, f in variants:
        window(f, 1, d_res)
        est = window(f, 1, d_res)
        assert bool((d_res == expect).all()), (tag, name)
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
        times[name] = []
    for _ in range(ROUNDS):
        for name, f in variants:
            times[name].append(1e3 * window(f, reps[name], d_res))
            assert bool((d_res == expect).all()), (tag, name)
    return {name: dict(stat(times[name]), reps_per_window=reps[name]) for name, _ in variants}


def compare(row, new, base):
    """the difference to a baseline and whether it exceeds that baseline's own spread (max - min over the rounds)"""
    saved = round(row[base]["ms_median"] - row[new]["ms_median"], 4)
    spread = round(row[base]["ms_max"] - row[base]["ms_min"], 4)
    row["saved_vs_" + base + "_ms"] = saved
    row[base + "_spread_ms"] = spread
    row["beyond_" + base + "_spread"] = bool(abs(saved) > spread)


def inputs(n_msgs, d_sk, seed):
    rng = np.random.default_rng(seed)
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
    d_spelled = d_list[torch.from_numpy(named).to(dev)].contiguous()
    torch.cuda.synchronize()
    return d_list, d_sigs, d_midx, d_spelled, expect, int((named != signed).sum())


out = {"form": "device-resident inputs, 32-byte messages; item i %% 16 == 7 names another message than was signed (rejected), the others are valid; items = %d" % NI,
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition; median [min, max] over the rounds",
       "round_items": int(ctx.limits().round_items), "shapes": {}, "stream": {}, "append": {}}
LISTS = [1, 512, 4096, NI]
ctx.reserve(max(N.plan_shared_msgs_workspace_items(NI, m, 128, True, ctx.limits()) for m in LISTS)); ctx.reserve_msgs(NI)
d_res = torch.full((NI,), 7, dtype=torch.uint8, device=dev)
stream_inputs = None
for shape, k, lists in (("indexed_128_keys", 128, LISTS), ("verify_1_key", 1, [512])):
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
    for n_msgs in lists:
        d_list, d_sigs, d_midx, d_spelled, expect, rejected = inputs(n_msgs, d_sk, 1000 + n_msgs)
        mt = N.MsgTable(ctx, capacity_hint=n_msgs)                    # built before timing
        assert mt.append_device(P(d_list), n_msgs, msg_len=32) == 0
        torch.cuda.synchronize()
        if k > 1:
            res = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_msgtable_device(ctx.handle, table.handle, P(d_sigs), mt.handle, P(d_midx), P(d_keys), None, NI, k,
                                                                                                 P(d_res), None, None, None))
            shr = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_shared_msgs_device(ctx.handle, table.handle, P(d_sigs), P(d_list), 32, None, n_msgs, P(d_midx),
                                                                                                    P(d_keys), None, NI, k, P(d_res), None, None, None))
            old = lambda: ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_device(ctx.handle, table.handle, P(d_sigs), P(d_spelled), 32, None, P(d_keys), None, NI, k,
                                                                                        P(d_res), None, None, None))
        else:
            res = lambda: ctx.check(lib.mbls_verify_batch_msgtable_device(ctx.handle, P(d_sigs), mt.handle, P(d_midx), P(d_keys), N.PK_COMPRESSED, NI, P(d_res), None, None, None))
            shr = lambda: ctx.check(lib.mbls_verify_batch_shared_msgs_device(ctx.handle, P(d_sigs), P(d_list), 32, None, n_msgs, P(d_midx), P(d_keys), N.PK_COMPRESSED, NI,
                                                                             P(d_res), None, None, None))
            old = lambda: ctx.check(lib.mbls_verify_batch_device(ctx.handle, P(d_sigs), P(d_spelled), 32, None, P(d_keys), N.PK_COMPRESSED, NI, P(d_res), None, None, None))
        row = {"items": NI, "keys_per_item": k, "n_msgs": n_msgs, "rejected_items": rejected}
        row.update(measure((("msgtable", res), ("shared_msgs", shr), ("per_item", old)), d_res, expect, (shape, n_msgs)))
        compare(row, "msgtable", "shared_msgs"); compare(row, "msgtable", "per_item")
        out["shapes"]["%s/%d" % (shape, n_msgs)] = row
        print("%-17s n_msgs %6d   table %8.3f ms   shared list %8.3f ms [%.3f, %.3f]   per item %8.3f ms [%.3f, %.3f]   saved %7.3f / %7.3f ms" % (
            shape, n_msgs, row["msgtable"]["ms_median"], row["shared_msgs"]["ms_median"], row["shared_msgs"]["ms_min"], row["shared_msgs"]["ms_max"],
            row["per_item"]["ms_median"], row["per_item"]["ms_min"], row["per_item"]["ms_max"], row["saved_vs_shared_msgs_ms"], row["saved_vs_per_item_ms"]), flush=True)
        if k > 1 and n_msgs == 512:
            stream_inputs = (d_list, d_sigs, d_midx, d_spelled, expect, d_keys, table, mt)
        else:
            mt.close()

# ---- the stream: calls of `call` items, two rounds' worth per window, the message-table stream against the stream that takes the messages
d_list, d_sigs, d_midx, d_spelled, expect, d_keys, table, mt = stream_inputs
expect2 = torch.cat([expect, expect])
for call in (4096, 16384):
    per_round = NI // call
    outs = [torch.full((NI,), 7, dtype=torch.uint8, device=dev) for _ in range(2)]
    with VerifyStream(ctx, table=table, msg_table=mt, policy=N.STREAM_FULL_ROUNDS) as vnew, VerifyStream(ctx, table=table, policy=N.STREAM_FULL_ROUNDS) as vold:
        def run_new():
            t = 0
            for o in outs:
                for c in range(per_round):
                    a = c * call
                    t = vnew.submit_device(d_sigs[a:], d_midx[a:], d_keys[a:], call, 128, o[a:])
            vnew.flush(); vnew.wait(t)

        def run_old():
            t = 0
            for o in outs:
                for c in range(per_round):
                    a = c * call
                    t = vold.submit_device(d_sigs[a:], d_spelled[a:], d_keys[a:], call, 128, o[a:], msg_len=32)
            vold.flush(); vold.wait(t)

        times = {"msgtable_stream": [], "message_stream": []}
        variants = (("msgtable_stream", run_new), ("message_stream", run_old))
        for name, f in variants:                            # warm-up, results checked
            for o in outs:
                o.fill_(7)
            f(); torch.cuda.synchronize()
            assert bool((torch.cat(outs) == expect2).all()), (call, name)
        for _ in range(ROUNDS):
            for name, f in variants:
                for o in outs:
                    o.fill_(7)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / 2)           # ms per round of NI items
                assert bool((torch.cat(outs) == expect2).all()), (call, name)
    row = {"call_items": call, "calls_per_window": 2 * per_round, "items_per_window": 2 * NI, "keys_per_item": 128, "n_msgs": 512, "unit": "ms per %d items" % NI}
    for name, _ in variants:
        row[name] = stat(times[name])
        row[name]["items_per_s"] = round(NI / (row[name]["ms_median"] * 1e-3))
    compare(row, "msgtable_stream", "message_stream")
    out["stream"]["%d" % call] = row
    print("stream, calls of %5d items   table %8.3f ms / round   messages %8.3f ms / round [%.3f, %.3f]   saved %7.3f ms" % (
        call, row["msgtable_stream"]["ms_median"], row["message_stream"]["ms_median"], row["message_stream"]["ms_min"], row["message_stream"]["ms_max"],
        row["saved_vs_message_stream_ms"]), flush=True)
mt.close(); table.close()

# ---- the append itself: n messages into an empty table of sufficient capacity (clear between repetitions is outside the clock)
for n_msgs in (512, 4096):
    rng = np.random.default_rng(2000 + n_msgs)
    d_list = torch.from_numpy(rng.integers(0, 256, size=(n_msgs, 32), dtype=np.uint8)).to(dev)
    mt = N.MsgTable(ctx, capacity_hint=n_msgs)
    ts = []
    for r in range(ROUNDS + 2):
        mt.clear()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        mt.append_device(P(d_list), n_msgs, msg_len=32)
        torch.cuda.synchronize()
        if r >= 2:
            ts.append(1e3 * (time.perf_counter() - t0))
    pts, errs = mt.get(0, n_msgs)
    assert pts == batch.hash_to_g2_batch(d_list.cpu().numpy().tobytes(), n_msgs) and not any(errs)
    mt.close()
    out["append"]["%d" % n_msgs] = dict(stat(ts), n_msgs=n_msgs)
    print("append of %5d messages   %8.3f ms [%.3f, %.3f]" % (n_msgs, out["append"]["%d" % n_msgs]["ms_median"], min(ts), max(ts)), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
