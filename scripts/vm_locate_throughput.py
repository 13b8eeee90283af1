"""Which sets of a rejected batch: ONE mbls_verify_multiple_batches_locate_device call against what a client does without it.
(a) all sets valid: the locate entry against mbls_verify_multiple_batches_device -- the price of keeping the leaves (two copy kernels) and of phase two's launches
    whose waves all return.
(b) 1 %, 10 % and 100 % of the batches carry one wrong-key set: the locate entry (one call, synchronise, read the per-set bytes) against the two-call sequence:
    mbls_verify_multiple_batches_device, synchronise, read the per-batch bytes, gather the rejected batches' sets on the host, mbls_verify_multiple_batches (host
    entry, synchronous) with sets_per_batch = 1 over them.
Aggregate-key form, 32-byte messages, device-resident inputs (the client keeps host copies for the second call); every result is checked. Same process, same
inputs, same timing method for all variants: a host clock around work that ends in a device synchronise, every shape warmed up, the variants alternated inside
every round, medians over the rounds with the spread beside them.
usage: python scripts/vm_locate_throughput.py [OUT.json]   (default: profiles/vm_locate_throughput.json; VML_ROUNDS, default 10)"""
import ctypes as C, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_locate_throughput.json")
ROUNDS = int(os.environ.get("VML_ROUNDS", "10"))
WINDOW_S = 0.25
SHAPES = [(128, 10), (1024, 10), (1024, 63)]
FRACTIONS = (0.01, 0.10, 1.00)
NMAX = max(B * s for B, s in SHAPES)
ctx = N.default_context()
d_sigs, d_msgs, d_good_apks, _ = bench.build_inputs(ctx, dev, NMAX, 1, N.PK_UNCOMPRESSED, rank=32, negatives=False)
rng = np.random.default_rng(32)
h_rands = rng.integers(1, 1 << 62, size=NMAX, dtype=np.int64)
d_rands = torch.from_numpy(h_rands).to(dev)
h_sigs = d_sigs.view(NMAX, 96).cpu().numpy(); h_msgs = d_msgs.view(NMAX, 32).cpu().numpy(); h_good_apks = d_good_apks.view(NMAX, 96).cpu().numpy()
L = ctx.limits()
ctx.reserve(max([N.plan_locate_workspace_items(B * s, B, L) for B, s in SHAPES] + [3 * NMAX]) + 64)       # (the second call at 100 %: as many batches as sets)
P = lambda t: t.data_ptr()


class Case:
    """a shape with `frac` of its batches carrying one set whose key is its neighbour's"""

    def __init__(self, B, spb, frac):
        n = B * spb
        self.B, self.spb, self.n = B, spb, n
        bad_b = sorted(rng.choice(B, size=max(1, int(round(frac * B))), replace=False).tolist()) if frac else []
        self.h_apks = h_good_apks[:n].copy()
        self.bad_sets = []
        for b in bad_b:
            i = b * spb + int(rng.integers(spb))
            j = i + 1 if i + 1 < (b + 1) * spb else i - 1
            self.h_apks[i] = h_good_apks[j]
            self.bad_sets.append(i)
        self.d_apks = torch.from_numpy(self.h_apks).to(dev)
        self.want_b = np.ones(B, dtype=np.uint8); self.want_b[bad_b] = 0
        self.want_s = np.ones(n, dtype=np.uint8); self.want_s[self.bad_sets] = 0
        self.res = torch.full((B,), 7, dtype=torch.uint8, device=dev)
        self.sres = torch.full((n,), 7, dtype=torch.uint8, device=dev)


def batches(c):
    ctx.check(lib.mbls_verify_multiple_batches_device(ctx.handle, P(d_sigs), P(c.d_apks), None, 0, None, 0, P(d_msgs), 32, None, P(d_rands), c.n, None, c.spb, c.B,
                                                      P(c.res), None, None))
    torch.cuda.synchronize()
    return c.res.cpu().numpy(), None


def locate(c):
    ctx.check(lib.mbls_verify_multiple_batches_locate_device(ctx.handle, P(d_sigs), P(c.d_apks), None, 0, None, 0, P(d_msgs), 32, None, P(d_rands), c.n, None, c.spb,
                                                             c.B, P(c.res), None, P(c.sres), None, None))
    torch.cuda.synchronize()
    return c.res.cpu().numpy(), c.sres.cpu().numpy()


def two_calls(c):
    rb, _ = batches(c)
    sets = (np.flatnonzero(rb == 0)[:, None] * c.spb + np.arange(c.spb)[None, :]).reshape(-1)
    rs = np.ones(c.n, dtype=np.uint8)
    if len(sets):
        s, a, m, r = (np.ascontiguousarray(x[sets]) for x in (h_sigs, c.h_apks, h_msgs, h_rands))
        out = np.zeros(len(sets), dtype=np.uint8)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        ctx.check(lib.mbls_verify_multiple_batches(ctx.handle, vp(s), vp(a), vp(m), 32, None, vp(r), len(sets), None, 1, len(sets), vp(out), None))
        rs[sets] = out
    torch.cuda.synchronize()
    return rb, rs


def window(f, c, reps):
    c.res.fill_(7); c.sres.fill_(7)
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        got = f(c)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, got


def check(c, got, name):
    rb, rs = got
    assert (rb == c.want_b).all(), (name, c.B, c.spb)
    assert rs is None or (rs == c.want_s).all(), (name, c.B, c.spb, np.flatnonzero(rs != c.want_s)[:8].tolist())


def measure(c, variants):
    reps, times = {}, {name: [] for name, _ in variants}
    for name, f in variants:                              # warm-up: every variant at this shape, results checked
        window(f, c, 1)
        est, got = window(f, c, 1)
        check(c, got, name)
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
    for _ in range(ROUNDS):
        for name, f in variants:                          # alternated inside the round
            ms, got = window(f, c, reps[name])
            times[name].append(1e3 * ms)
            check(c, got, name)
    return {name: {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "reps_per_window": reps[name]}
            for name, t in times.items()}


out = {"form": "aggregate keys, 32-byte messages, device-resident inputs, host copies for the second call", "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions, each ending in a device synchronise and the read-back of its results; ms per repetition; "
                 "median [min, max] over the rounds",
       "round_items": int(L.round_items), "shapes": {}}
for B, spb in SHAPES:
    row = {"batches": B, "sets_per_batch": spb, "sets": B * spb}
    a = measure(Case(B, spb, 0.0), (("batches", batches), ("locate", locate)))
    a["locate_minus_batches_ms"] = round(a["locate"]["ms_median"] - a["batches"]["ms_median"], 4)
    a["batches_spread_ms"] = round(a["batches"]["ms_max"] - a["batches"]["ms_min"], 4)
    row["all_valid"] = a
    print("%5d x %3d  all valid: batches %8.3f ms [%.3f, %.3f]   locate %8.3f ms [%.3f, %.3f]   difference %+.3f ms" % (
        B, spb, a["batches"]["ms_median"], a["batches"]["ms_min"], a["batches"]["ms_max"], a["locate"]["ms_median"], a["locate"]["ms_min"], a["locate"]["ms_max"],
        a["locate_minus_batches_ms"]), flush=True)
    for frac in FRACTIONS:
        c = Case(B, spb, frac)
        r = measure(c, (("two_calls", two_calls), ("locate", locate)))
        r["bad_batches"] = int((c.want_b == 0).sum())
        r["two_calls_over_locate"] = round(r["two_calls"]["ms_median"] / r["locate"]["ms_median"], 2)
        row["bad_%d_percent" % round(100 * frac)] = r
        print("%5d x %3d  %3d %% bad (%d batches): two calls %8.3f ms [%.3f, %.3f]   locate %8.3f ms [%.3f, %.3f]   two calls / locate %.2f" % (
            B, spb, round(100 * frac), r["bad_batches"], r["two_calls"]["ms_median"], r["two_calls"]["ms_min"], r["two_calls"]["ms_max"], r["locate"]["ms_median"],
            r["locate"]["ms_min"], r["locate"]["ms_max"], r["two_calls_over_locate"]), flush=True)
    out["shapes"]["%dx%d" % (B, spb)] = row
out["locate_faster_than_two_calls"] = {k: {f: v[f]["two_calls_over_locate"] > 1.0 for f in v if f.startswith("bad_")} for k, v in out["shapes"].items()}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out["locate_faster_than_two_calls"]))
