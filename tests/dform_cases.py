"""Cases for the generated digit-form bodies at the inputs their own generator admits, shared by tests/test_dform_cases_cpu.py (tools/asm_sim.py) and
tests/test_gpu_dform.py (the raw-register probe kernel, mbls_dform_probe): per probe of tools/gen_tower_d.py probe_ops() a list of lanes, each the raw 32-bit
register contents the probe loads. Every limit comes from the generator's predicates (AllocD.call_limits_ok / call_bounds, the bounds recorded in
gen_tower_d.QSITES while the routines are generated, estimate_error), none is a number written down here.

simulate(case) runs the very instruction list the kernel contains -- loads and stores included -- on the interpreter; check(case, words) judges a lane's stored
registers by big-integer arithmetic alone, so it can be applied to the interpreter's registers and to the GPU's independently."""
import contextlib
import functools
import io
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fpd_asm as d          # noqa: E402
import gen_tower_d as t          # noqa: E402
from asm_sim import Machine, M32, s32, digits_signed, from_digits_signed, from_limbs, limbs   # noqa: E402

P = d.P
RI = pow(1 << 392, -1, P)
PTOP = t.PTOP
W364 = 1 << 364
OPS = t.probe_ops()                                   # [(name, input registers, output registers, body)]
OP = {o[0]: i for i, o in enumerate(OPS)}
LINES = {o[0]: t.probe_lines(o[1], o[2], o[3]) for o in OPS}
LEAF_KIND = {r["name"][5:-7]: k for k, r in t.ROUTINES.items()}          # probe name -> the allocator's name of the routine
IN_BASE, OUT_BASE = 0x10000, 0x80000


class Case:
    __slots__ = ("op", "cls", "words", "info")

    def __init__(self, op, cls, words, info=None):
        self.op, self.cls, self.words, self.info = op, cls, [w & M32 for w in words], info

    def __repr__(self):
        return "<%s/%s>" % (self.op, self.cls)


def simulate(case, lines=None):
    """the probe's instruction list on one interpreted lane: the registers it stores (the interpreter's overflow assertions are live)"""
    name, ins, outs, _ = OPS[OP[case.op]]
    m = Machine()
    m.s[66], m.s[67], m.s[68], m.s[69], m.s[70] = IN_BASE, 0, OUT_BASE, 0, 4
    m.v[252] = 0
    for w, x in enumerate(case.words):
        m.mem[IN_BASE + 4 * w] = x
    m.run(LINES[name] if lines is None else lines)
    return [m.mem[OUT_BASE + 4 * w] for w in range(len(outs))]


def exact_bound(dg):
    """the Bound that contains exactly this digit vector"""
    sd = [s32(v) for v in dg]
    x = from_digits_signed(dg)
    return t.Bound(min(sd[:13]), max(sd[:13]), sd[13], sd[13], x, x)


def admitted(kind, bounds):
    """what the allocator requires before it emits the routine: the column limits, and a result whose top digit fits a register"""
    if not t.AllocD.call_limits_ok(None, kind, bounds):
        return False
    try:
        return all(b.fits() for b in t.AllocD.call_bounds(None, kind, bounds))
    except AssertionError:
        return False


# ---------------------------------------------------------------------------------------------- the leaves
def normalised(x):
    dg = [(x >> (28 * i)) & 0xFFFFFFF for i in range(13)]
    return dg + [((x - sum(v << (28 * i) for i, v in enumerate(dg))) >> 364) & M32]


# sign / shape of digit j of operand o at magnitude M
PATTERNS = {
    "all_pos": lambda o, j: 1, "all_neg": lambda o, j: -1,
    "opposed_ab": lambda o, j: 1 if o < 2 else -1,            # the operands of a product against each other: every column at its negative end
    "opposed_01": lambda o, j: 1 if o % 2 == 0 else -1,       # a0 - a1 and b1 - b0 (the third product of the Karatsuba form) at both ends
    "alternating": lambda o, j: 1 if j % 2 == 0 else -1, "alternating_neg_first": lambda o, j: -1 if j % 2 == 0 else 1,
    "alternating_shifted": lambda o, j: 1 if (j + o) % 2 == 0 else -1,
    "middle": lambda o, j: 1 if 4 <= j <= 9 else 0, "middle_opposed": lambda o, j: (1 if o < 2 else -1) if 4 <= j <= 9 else 0,
    "low13": lambda o, j: 1 if j < 13 else 0, "low13_opposed": lambda o, j: (1 if o < 2 else -1) if j < 13 else 0,      # every column loaded, the value small
}


def pattern_digits(pat, M):
    return [[(PATTERNS[pat](o, j) * M) & M32 for j in range(14)] for o in range(4)]


def limit_magnitude(kind, pat):
    """the largest M at which the generator still admits the pattern (bisection over its own predicates)"""
    slots = t.ROUTINES[kind]["ins"]
    ok = lambda M: admitted(kind, [exact_bound(pattern_digits(pat, M)[s]) for s in slots])
    lo, hi = 1, (1 << 31) - 1
    assert ok(lo)
    if ok(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def leaf_cases(name, n_random=60, n_redundant=30):
    kind = LEAF_KIND[name]
    slots = t.ROUTINES[kind]["ins"]
    rng = random.Random("leaf " + name)
    groups = {}

    def add(cls, blocks):
        words = []
        for b in range(4):
            words += blocks[b]
        groups.setdefault(cls, []).append(Case(name, cls, words, dict(kind=kind)))
    edge = [0, 1, P - 1, P - 2]
    for i in range(8):
        add("canonical_edge", [normalised(edge[(i + b * (1 + i // 4)) % 4]) for b in range(4)])
    for _ in range(6):
        add("zero", [normalised(0)] * 4)
    for _ in range(n_random):
        add("canonical_random", [normalised(rng.randrange(P)) for b in range(4)])
    uniform = lambda M: [t.Bound(-M, M, -M, M, -(M << 366), M << 366)] * len(slots)
    for i in range(n_redundant):
        dmax = [1 << 28, 1 << 29, 1 << 30][i % 3]
        while not t.AllocD.call_limits_ok(None, kind, uniform(dmax)):            # stay inside the routine's own digit limit
            dmax >>= 1
        while True:
            blocks = [digits_signed(rng.randrange(-3 * P, 4 * P), dmax, rng) for b in range(4)]
            if admitted(kind, [exact_bound(blocks[s]) for s in slots]):
                break
        add("redundant", blocks)
    # columns that end NEGATIVE with a zero quotient digit: the carry out of them is -1, which only an arithmetic shift delivers
    neg, one = [(-(1 << 28)) & M32] * 14, [1] + [0] * 13
    add("negative_carry", [neg, neg, one, one])
    add("negative_carry", [neg, one, one, neg])
    chain = [(-(1 << 28)) & M32] + [(1 - (1 << 28)) & M32] * 13          # ... in EVERY column: each is -2^28 once the carry -1 has arrived
    add("negative_carry", [chain, chain, one, one])
    for pat in PATTERNS:
        M = limit_magnitude(kind, pat)
        add("limit", pattern_digits(pat, M))
        add("limit", pattern_digits(pat, M - 1))
    return interleave(groups)


def interleave(groups):
    """different classes in neighbouring lanes (an edge case next to a random one next to a zero), and a lane count that is no multiple of 64"""
    order = sorted(groups)
    zero = groups["zero"][0]
    out, i = [], 0
    while any(groups[g] for g in order):
        g = order[i % len(order)]; i += 1
        if groups[g]:
            out.append(groups[g].pop())
    while len(out) % 64 == 0 or len(out) < 65:        # more than one wave, the last one partly filled
        out.append(zero)
    return out


def check_leaf(case, words):
    kind = case.info["kind"]
    R = t.ROUTINES[kind]
    blk = [case.words[14 * b:14 * b + 14] for b in range(4)]
    val = [from_digits_signed(b) for b in blk]
    for s in R["ins"]:
        if s not in R["clob"]:
            assert words[14 * s:14 * s + 14] == blk[s], (case, "operand block %d not preserved" % s)
    a0, a1, b0, b1 = val
    if kind == "mul":
        want = [a0 * b0 - a1 * b1, a0 * b1 + a1 * b0]
    elif kind == "sqr":
        want = [a0 * a0 - a1 * a1, 2 * a0 * a1]
    elif kind == "mulfp":
        want = [a0 * b0, a1 * b0]
    elif kind == "mulpair":
        want = [a0 * b0, a1 * b1]
    elif kind == "mul1":
        want = [a0 * b0]
    elif kind == "sqrpair":
        want = [a0 * a0, a1 * a1]
    elif kind == "fp4sqr0":
        want = [a0 * a0 - a1 * a1 + b0 * b0 - b1 * b1 - 2 * b0 * b1, 2 * a0 * a1 + b0 * b0 - b1 * b1 + 2 * b0 * b1]
    else:
        assert kind == "redc7"
        want = None
    bounds = t.AllocD.call_bounds(None, kind, [exact_bound(blk[s]) for s in R["ins"]])
    for i in range(len(R["outs"])):
        dg = words[56 + 14 * i:70 + 14 * i]
        r = from_digits_signed(dg)
        if want is None:
            assert (r - a0 * pow(1 << 196, -1, P)) % P == 0, (case, "value")
        else:
            assert (r - want[i] * RI) % P == 0, (case, "value of result %d" % i)
        assert all(0 <= s32(v) < (1 << 28) for v in dg[:13]), (case, "digits not normalised")
        assert bounds[i].vlo <= r <= bounds[i].vhi and bounds[i].tlo <= s32(dg[13]) <= bounds[i].thi, (case, "outside the allocator's bound", r / P)


# ---------------------------------------------------------------------------------------------- the passes
SITE_LIST = []                                        # gen_tower_d.QSITES as one whole generation leaves it (set by recorded_sites)
PASSES_EMITTED = [None]                               # how many seq_reduce / seq_pack_pass sequences the routines contain (set by recorded_sites)


@functools.lru_cache(None)
def recorded_sites():
    """(site, pass) -> the widest input the generator records there while it generates every routine: (|v| bound, digit magnitude bound)"""
    del t.QSITES[:]
    calls = [0]
    real = t.seq_reduce, t.seq_pack_pass

    def counting(f):
        def g(reg):
            calls[0] += 1
            return f(reg)
        return g
    t.seq_reduce, t.seq_pack_pass = counting(real[0]), counting(real[1])
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            t.generate_text()
        emitted = calls[0]
        t.probe_ops()                                  # the probes' own bodies are no sites
        PASSES_EMITTED[0] = emitted - (calls[0] - emitted)
    finally:
        t.seq_reduce, t.seq_pack_pass = real
    SITE_LIST[:] = list(t.QSITES)                      # a snapshot: generator functions that other tests call later append to the live list
    sites = {}
    for site, kind, B, res in SITE_LIST:
        v, dm = sites.get((site, kind), (0, 0))
        sites[(site, kind)] = (max(v, B.vabs()), max(dm, abs(B.dlo), abs(B.dhi)))
    return sites


def pass_limits(kind):
    """the widest value and the widest lower digits any site of the pass records"""
    s = [v for (site, k), v in recorded_sites().items() if k == kind]
    return max(v for v, _ in s), max(dm for _, dm in s)


def qbound_for(dg, pack):
    """the result bound the allocator would assign to an input bound that contains just this digit vector"""
    B = exact_bound(dg)
    return t.packed_bound(B) if pack else t.reduced_bound(B)


def qpass_cases(name, per_binade=24, n_random=120):
    pack = name == "pack32"
    kind = "pack" if pack else "reduce"
    rng = random.Random("pass " + name)
    vmax, dmax = pass_limits(kind)
    kmax = vmax // P
    groups = {}

    def add(cls, x, redundant, beyond=False):
        if abs(x) > vmax and not beyond:
            return
        dg = digits_signed(x, dmax, rng) if redundant else normalised(x)
        if abs(s32(dg[13])) >= (1 << 31) - 1:
            return
        groups.setdefault(cls, []).append(Case(name, cls, dg, dict(x=x, pack=pack)))
    kcap = ((1 << 31) - 16) * W364 // P - 1          # beyond what the sites record, up to the largest top digit a register holds: REDUCED_ANY's claim
    b = 0
    while (1 << b) <= kcap:                          # (k + 1/2) p +- delta: where the rounded quotient flips, in every binade of k
        inside = (1 << b) <= max(kmax, 1)
        for i in range(per_binade if inside else per_binade // 3):
            k = min(rng.randrange(1 << b, 2 << b), (max(kmax - 1, 0) if inside else kcap)) if i else (1 << b)
            slack = int(t.estimate_error((k + 1) * P, -dmax, dmax, pack, tmag=(1 << 31) - 1) * P) + 1
            delta = [1, rng.randrange(1, slack), slack >> 8, slack >> 2, slack >> 1, slack][i % 6]
            x = k * P + P // 2 + rng.choice([-1, 1]) * delta
            add("edge" if inside else "edge_beyond", x if i % 2 else -x, redundant=bool(i & 2), beyond=not inside)
        b += 1
    for k in (0, 0, 1):
        add("edge", rng.choice([-1, 1]) * (k * P + P // 2 + rng.randrange(-2, 3)), redundant=False)
    tops = [(1 << 24) + e for e in (-1, 0, 1)]      # top digits where the conversion to f32 starts to round
    for k in range(1, 31):
        tops += [(1 << 24) + (1 << k) + e for e in (-1, 1)]
    tops += [vmax // W364 - 1, (1 << 31) - 2]       # the largest a site records, and the largest a register holds (estimate_error covers it)
    for top in tops:
        for sign in (1, -1):
            add("f32_edge", sign * (top * W364 + rng.randrange(W364)), redundant=False, beyond=True)
    for x in (0, 1, -1, P, -P, P - 1, P // 2, -(P // 2)):
        add("small", x, redundant=False)
    for i in range(n_random):
        add("random", rng.randrange(-vmax, vmax + 1) >> rng.randrange(0, 12), redundant=bool(i % 2))
    for _ in range(8):
        add("zero", 0, redundant=False)
    return interleave(groups)


def check_qpass(case, words):
    x, pack = case.info["x"], case.info["pack"]
    B = qbound_for(case.words, pack)
    if pack:                                           # 12 packed words of the representative in (0.5 p, 1.5 p)
        r = from_limbs(words[:12])
        assert (r - x) % P == 0, (case, "value")
        assert B.vlo <= r <= B.vhi, (case, "outside the bound the allocator assigns", (r - P) / P)
        assert words[12:14] == [(r >> 336) & 0xFFFFFFF, r >> 364], (case, "leftover digits")
    else:
        dg = words[:14]
        r = from_digits_signed(dg)
        assert (r - x) % P == 0, (case, "value")
        assert all(0 <= s32(v) < (1 << 28) for v in dg[:13]), (case, "digits not normalised")
        assert B.vlo <= r <= B.vhi, (case, "outside the bound the allocator assigns", r / P)
    q = (x - r) // P
    assert (x - r) % P == 0 and s32(words[14]) == -q, (case, "quotient register")


def norm_cases():
    rng = random.Random("norm")
    groups = {"zero": [Case("norm", "zero", [0] * 14, dict(x=0))] * 6}
    for i in range(60):
        x = rng.randrange(-200 * P, 200 * P)
        dg = digits_signed(x, [1 << 28, 1 << 30, (1 << 31) - 1][i % 3], rng)
        groups.setdefault("redundant", []).append(Case("norm", "redundant", dg, dict(x=x)))
    uniform = lambda M: t.Bound(-M, M, -M, M, 0, 0)
    lo, hi = 1, (1 << 31) - 1                        # the largest uniform digit magnitude the generator sends into a carry pass (gen_tower_d.norm_ok)
    assert t.norm_ok(uniform(lo)) and not t.norm_ok(uniform(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if t.norm_ok(uniform(mid)) else (lo, mid)
    lim = lo
    for dg in ([lim] * 14, [-lim] * 14, [lim, -lim] * 7, [-lim, lim] * 7, [lim] * 13 + [0], [-lim] * 13 + [0], [lim - 1] * 14, [1 - lim] * 14):
        groups.setdefault("limit", []).append(Case("norm", "limit", dg, dict(x=from_digits_signed([v & M32 for v in dg]))))
    for x in (0, 1, -1, P - 1):
        groups.setdefault("small", []).append(Case("norm", "small", normalised(x), dict(x=x)))
    return interleave(groups)


def check_norm(case, words):
    assert from_digits_signed(words) == case.info["x"], (case, "value")
    assert all(0 <= s32(v) < (1 << 28) for v in words[:13]), (case, "digits not normalised")


def canon_cases():
    rng = random.Random("canon")
    groups = {"zero": [Case("canon32", "zero", [0] * 14, dict(x=0))] * 6}
    lim = t.REDUCED_ANY.vhi
    for x in (0, 1, -1, P - 1, -(P - 1), P // 2, -(P // 2), lim, -lim, P - 2, 2 - P):
        groups.setdefault("edge", []).append(Case("canon32", "edge", normalised(x), dict(x=x)))
    for i in range(60):
        x = rng.randrange(-P + 1, P)
        groups.setdefault("random", []).append(Case("canon32", "random", normalised(x), dict(x=x)))
    return interleave(groups)


def check_canon(case, words):
    x = case.info["x"]
    assert from_limbs(words[:12]) == x % P, (case, "value")
    assert words[14] == (1 if x < 0 else 0), (case, "sign register")


def conv_cases():
    rng = random.Random("conv")
    groups = {"zero": [Case("conv_reduce", "zero", [0] * 12, dict(w=0))] * 6}
    for w in (0, 1, P - 1, P - 2, P, (1 << 384) - 1, (1 << 384) - 2, 1 << 383, M32, ((1 << 384) - 1) ^ M32):
        groups.setdefault("edge", []).append(Case("conv_reduce", "edge", limbs(w), dict(w=w)))
    for i in range(80):
        w = rng.randrange(P) if i % 2 else rng.getrandbits(384)
        groups.setdefault("below_p" if i % 2 else "any_words", []).append(Case("conv_reduce", "random", limbs(w), dict(w=w)))
    return interleave(groups)


def check_conv(case, words):
    w = case.info["w"]
    dg = words[:14]
    r = from_digits_signed(dg)
    B = t.reduced_bound(t.G_IN)                        # what the generator assigns to the conversion followed by a reduction
    assert (r - (w << 8)) % P == 0, (case, "value")
    assert all(0 <= s32(v) < (1 << 28) for v in dg[:13]), (case, "digits not normalised")
    assert B.vlo <= r <= B.vhi, (case, "outside the bound the allocator assigns", r / P)
    assert s32(words[14]) == -(((w << 8) - r) // P), (case, "quotient register")


@functools.lru_cache(None)
def cases(name):
    if name in LEAF_KIND:
        return leaf_cases(name)
    if name in ("reduce", "pack32"):
        return qpass_cases(name)
    return {"norm": norm_cases, "canon32": canon_cases, "conv_reduce": conv_cases}[name]()


def check(case, words):
    if case.op in LEAF_KIND:
        return check_leaf(case, words)
    return {"reduce": check_qpass, "pack32": check_qpass, "norm": check_norm, "canon32": check_canon, "conv_reduce": check_conv}[case.op](case, words)


@functools.lru_cache(None)
def simulated(name):
    """the interpreter's registers for every case of a probe: computed once per session, shared by the CPU and the GPU tests"""
    return [simulate(c) for c in cases(name)]
