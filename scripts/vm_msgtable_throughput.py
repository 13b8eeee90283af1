"""verify_multiple over the resident message table: mbls_verify_multiple_msgtable_device (nothing hashed; the entries a call names found on the device) against
mbls_verify_multiple_shared_msgs_device on the same sets and the same list, hashed in every call -- the baseline: today's behaviour, measured in the same run.
Shapes: 2^16 sets over 64, 512 and 4 096 table entries, 2^14 over 512, 1 024 over 8 (every entry named); 2^16 sets naming 512 entries of a 2^16-entry table
through the device entry (auto: per set, and mode 1 forced: 2^16 Miller items of which 512 are live) and through the host-counted route
(mbls_verify_multiple_msgtable_rng: host buffers, grouped with 512 Miller items) against the shared-message device entry over the list of the 512 named
messages; the _locate form at 2^16 / 512, valid and with 1 % bad sets, against mbls_verify_multiple_shared_msgs_locate_device. One aggregate key per set,
32-byte messages, device-resident inputs, the table built before timing.
Same process, same inputs, same timing method for all variants: a host clock around a window of repetitions that ends in a device synchronise, every shape
warmed up, the variants alternated inside every round, medians over the rounds with min and max beside them. Every result is checked after every window, and
once per shape a copy in which one set names another message must be rejected by every variant.
usage: python scripts/vm_msgtable_throughput.py [OUT.json]   (default: profiles/vm_msgtable_throughput.json; VMTT_ROUNDS, default 10)"""
import ctypes as C, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_msgtable_throughput.json")
ROUNDS = int(os.environ.get("VMTT_ROUNDS", "10"))
WINDOW_S = 0.2
# (sets, table entries, entries named, locate)
SHAPES = [(65536, 64, 64, False), (65536, 512, 512, False), (65536, 4096, 4096, False), (16384, 512, 512, False), (1024, 8, 8, False),
          (65536, 65536, 512, False), (65536, 512, 512, True)]
ctx = N.default_context()
P = lambda t: t.data_ptr()
pool = bench.make_pool(bench.SEED)
POOL = len(pool)
d_pool_sk = torch.from_numpy(np.frombuffer(b"".join(s.to_bytes(32, "big") for s in pool), dtype=np.uint8).reshape(POOL, 32).copy()).to(dev)
d_pool_pk = torch.empty((POOL, 96), dtype=torch.uint8, device=dev)
ctx.check(lib.mbls_sk_to_pk_batch_device(ctx.handle, P(d_pool_sk), N.PK_UNCOMPRESSED, POOL, P(d_pool_pk), None))


def window(f, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


out = {"form": "device-resident inputs, one aggregate key per set, 32-byte messages, the table built before timing; every result checked after every window; "
               "a copy with one set renamed to another message is rejected by every variant",
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per call; median [min, max] over the rounds",
       "variants": {"baseline": "mbls_verify_multiple_shared_msgs[_locate]_device, mode 0, over the list of the NAMED messages (hashed in every call)",
                    "table": "mbls_verify_multiple_msgtable[_locate]_device, mode 0", "table_grouped": "the same, mode 1", "table_per_set": "the same, mode 2",
                    "host_counted": "mbls_verify_multiple_msgtable_rng: host buffers in, staging and the synchronise included; the host counts the named entries",
                    "append": "mbls_msgtable_append_device of the named messages into a cleared table (what a call over a list pays for its hash)"},
       "round_items": int(ctx.limits().round_items), "shapes": {}}
L = ctx.limits()
ctx.reserve(max(N.plan_verify_multiple_shared_msgs_locate_workspace_items(n, D, 1, L) for n, _T, D, _l in SHAPES)); ctx.reserve_msgs(max(D for _n, _T, D, _l in SHAPES))
for n, T, D, locate in SHAPES:
    rng = np.random.default_rng(7000 + n + T + D + int(locate))
    who = torch.from_numpy(rng.integers(0, POOL, size=n, dtype=np.int64)).to(dev)
    d_apks = d_pool_pk[who].contiguous(); d_sk = d_pool_sk[who].contiguous()
    d_table_msgs = torch.from_numpy(rng.integers(0, 256, size=(T, 32), dtype=np.uint8)).to(dev)
    entries = np.sort(rng.choice(T, size=D, replace=False)) if D < T else np.arange(T)     # the entries the call names, in table order
    which = rng.integers(0, D, size=n, dtype=np.int64); which[:D] = np.arange(D)           # (every one of them is named)
    tab_idx = entries[which]
    d_list = d_table_msgs[torch.from_numpy(entries).to(dev)].contiguous()                  # the baseline's list: the named messages
    d_spelled = d_list[torch.from_numpy(which).to(dev)].contiguous()
    d_sigs = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_spelled), 32, n, P(d_sigs), None))
    d_lidx = torch.from_numpy(which.astype(np.int32)).to(dev); d_tidx = torch.from_numpy(tab_idx.astype(np.uint32).view(np.int32)).to(dev)
    d_rands = torch.from_numpy(rng.integers(1, 1 << 63, size=n, dtype=np.int64)).to(dev)
    d_res = torch.full((8,), 7, dtype=torch.uint8, device=dev)
    d_sres = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    mt = N.MsgTable(capacity_hint=T)
    assert mt.append_device(P(d_table_msgs), T, msg_len=32) == 0
    torch.cuda.synchronize()
    bad_sets = np.zeros(0, dtype=np.int64)
    if locate:                                              # 1 % of the sets name the next entry: rejected, and located
        bad_sets = np.sort(rng.choice(n, size=n // 100, replace=False))

    def indices(bad):
        """(list indices, table indices) with the sets of `bad` renamed to the next named entry"""
        w = which.copy(); w[bad] = (w[bad] + 1) % D
        return torch.from_numpy(w.astype(np.int32)).to(dev), torch.from_numpy(entries[w].astype(np.uint32).view(np.int32)).to(dev)

    def shared(lidx, loc):
        def f():
            ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, 0))
            if loc:
                ctx.check(lib.mbls_verify_multiple_shared_msgs_locate_device(ctx.handle, P(d_sigs), P(d_apks), P(d_list), 32, None, D, P(lidx), P(d_rands), n, P(d_res), None,
                                                                             P(d_sres), None, None))
            else:
                ctx.check(lib.mbls_verify_multiple_shared_msgs_device(ctx.handle, P(d_sigs), P(d_apks), P(d_list), 32, None, D, P(lidx), P(d_rands), n, P(d_res), None, None))
        return f

    def table(mode, tidx, loc):
        def f():
            ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, mode))
            if loc:
                ctx.check(lib.mbls_verify_multiple_msgtable_locate_device(ctx.handle, P(d_sigs), P(d_apks), mt.handle, P(tidx), P(d_rands), n, P(d_res), None, P(d_sres), None, None))
            else:
                ctx.check(lib.mbls_verify_multiple_msgtable_device(ctx.handle, P(d_sigs), P(d_apks), mt.handle, P(tidx), P(d_rands), n, P(d_res), None, None))
        return f

    def check(name, want, bad):
        assert int(d_res[0].item()) == want, (n, T, D, name, "result", int(d_res[0].item()))
        if locate:
            got = np.flatnonzero(d_sres.cpu().numpy() != 1)
            assert list(got) == list(bad), (n, T, D, name, "located", len(got), len(bad))

    def run_variants(variants, want, bad, tag):
        reps, times = {}, {}
        for name, f in variants:                            # warm-up: every variant at this shape, results checked
            d_res.fill_(7); d_sres.fill_(7)
            window(f, 1)
            est = window(f, 1)
            check(name, want, bad)
            reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
            times[name] = []
        for _ in range(ROUNDS):
            for name, f in variants:                        # alternated inside the round
                d_res.fill_(7); d_sres.fill_(7)
                times[name].append(1e3 * window(f, reps[name]))
                check(name, want, bad)
        row = {name: dict(stats(times[name]), reps_per_window=reps[name]) for name, _ in variants}
        b, t = row["baseline"], row["table"]
        row["baseline_spread_ms"] = round(b["ms_max"] - b["ms_min"], 4)
        row["table_saved_ms"] = round(b["ms_median"] - t["ms_median"], 4)
        row["table_over_baseline"] = round(t["ms_median"] / b["ms_median"], 4)
        row["table_faster_by_more_than_baseline_spread"] = bool(row["table_saved_ms"] > row["baseline_spread_ms"])
        print("%s   baseline %8.3f [%.3f, %.3f]   %s   table saves %7.3f ms (x %.3f)%s" % (
            tag, b["ms_median"], b["ms_min"], b["ms_max"], "   ".join("%s %8.3f" % (k, row[k]["ms_median"]) for k, _ in variants[1:]), row["table_saved_ms"],
            row["table_over_baseline"], "" if row["table_faster_by_more_than_baseline_spread"] else "   NOT FASTER BY MORE THAN THE BASELINE'S SPREAD"), flush=True)
        return row

    # the negative check: set 5 names the next named entry -- rejected by every variant (and located by the locate forms)
    d_bl, d_bt = indices(np.array([5]))
    for name, f in (("baseline", shared(d_bl, locate)), ("table", table(0, d_bt, locate)), ("table_grouped", table(1, d_bt, locate)), ("table_per_set", table(2, d_bt, locate))):
        d_res.fill_(7); d_sres.fill_(7)
        window(f, 1)
        check(name, 0, [5])
    variants = [("baseline", shared(d_lidx, locate)), ("table", table(0, d_tidx, locate)), ("table_grouped", table(1, d_tidx, locate)), ("table_per_set", table(2, d_tidx, locate))]
    h_sigs = h_apks = h_idx = None
    if D < T:                                               # the host-counted route: host buffers in, the scalars handed over by the callback
        h_sigs, h_apks = N.cbuf(d_sigs.cpu().numpy().tobytes()), N.cbuf(d_apks.cpu().numpy().tobytes())
        h_idx = (C.c_uint32 * n)(*[int(x) for x in tab_idx])
        h_rands = (C.c_uint64 * n)(*[int(x) for x in d_rands.cpu().numpy()])
        h_res = N.outbuf(1)
        cb = N.SCALAR_SOURCE(lambda _u, o, count: C.memmove(o, h_rands, 8 * count) and None)

        def host():
            ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, 0))
            ctx.check(lib.mbls_verify_multiple_msgtable_rng(ctx.handle, h_sigs, h_apks, mt.handle, h_idx, n, h_res, cb, None))
            d_res[0] = int(h_res[0])
        variants.append(("host_counted", host))
    pd, ph = N.plan_verify_multiple_msgtable(n, T, 0, 0, L), N.plan_verify_multiple_msgtable(n, T, D, 0, L)
    route = lambda p: "grouped" if p["route"] == N.VM_ROUTE_GROUPED else "per_set"
    key = "%d/%d/%d%s" % (n, T, D, "/locate" if locate else "")
    row = {"sets": n, "table_entries": T, "named": D, "locate": locate, "device_auto_route": route(pd), "device_miller_items": int(pd["miller_items"]),
           "host_route": route(ph), "host_miller_items": int(ph["miller_items"])}
    row.update(run_variants(variants, 1, [], "%-22s valid " % key))
    if locate:
        d_bl, d_bt = indices(bad_sets)
        bad_variants = [("baseline", shared(d_bl, True)), ("table", table(0, d_bt, True)), ("table_grouped", table(1, d_bt, True)), ("table_per_set", table(2, d_bt, True))]
        row["one_percent_bad"] = run_variants(bad_variants, 0, bad_sets, "%-22s 1%% bad" % key)
    # what the list costs a call: an append of the named messages into a cleared table of their size
    mt2 = N.MsgTable(capacity_hint=D)
    ts = []
    for _ in range(ROUNDS + 1):
        mt2.clear(); torch.cuda.synchronize(); t0 = time.perf_counter()
        mt2.append_device(P(d_list), D, msg_len=32)
        torch.cuda.synchronize(); ts.append(1e3 * (time.perf_counter() - t0))
    row["append"] = stats(ts[1:])
    mt2.close(); mt.close()
    out["shapes"][key] = row
ctx.check(lib.mbls_ctx_set_vm_grouping(ctx.handle, 0))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
