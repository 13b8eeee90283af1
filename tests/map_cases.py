"""Field elements for the part of hash_to_curve_g2 that follows hash_to_field, at the inputs no hashed message reaches -- shared by tests/test_map_cases_cpu.py
(tools/coop_sim.py, tools/asm_sim.py, the host emulator) and tests/test_gpu_map.py (mbls_map_to_g2_probe). A case is a named pair (u0, u1) of Fp2 elements, the
predicates it must satisfy and the point the Python model (oracle/pymodel) gives for it:
    H = clear_cofactor_g2(g2_add(iso3_g2(sswu_g2(u0)), iso3_g2(sswu_g2(u1)))), compressed.
Every predicate is evaluated with the model when the list is built (cases() raises if one fails), so a case cannot silently stop reaching its branch; which
branches a set of cases provably enters is therefore a property of this list, not of anything observed on a GPU.

Branches covered: the exceptional denominator of the simplified SWU map (tv2 = Z^2 u^4 + Z u^2 = 0, i.e. u = 0), the three classes of sgn0(u) = s0 | (z0 & s1)
and the class with both terms clear, both square classes of gx1, q0 = q1 (the doubling fix-up of the addition), q0 = -q1 (the cofactor clearing on infinity).
OUT OF SCOPE: the degenerate branches of the complex-method square root inside the map (t = 0, G.c1 = 0). Reaching them needs a u that solves a system of high
degree; no such u is known, so no case here enters them."""
import functools
import random

from pymodel import bls12_381 as M

P = M.P
SEED = 0x6d6170                 # every random element below comes from this one seed
INF = bytes([0xC0]) + bytes(95)
A, B, Z = M.SSWU_A, M.SSWU_B, M.SSWU_Z


# ---------------------------------------------------------------------------------------------- the model's own quantities
def tv2(u):
    """the denominator term of the simplified SWU map: Z^2 u^4 + Z u^2"""
    zu2 = M.f2_mul(Z, M.f2_sqr(u))
    return M.f2_add(M.f2_sqr(zu2), zu2)


def x1(u):
    d = tv2(u)
    if M.f2_is_zero(d):
        return M.f2_mul(B, M.f2_inv(M.f2_mul(Z, A)))
    return M.f2_mul(M.f2_mul(M.f2_neg(B), M.f2_inv(A)), M.f2_add(M.F2_ONE, M.f2_inv(d)))


def gx1_is_square(u):
    x = x1(u)
    return M.f2_is_square(M.f2_add(M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.f2_mul(A, x)), B))


def q(u):
    """map_to_curve: the point of E the 3-isogeny makes of the SWU point"""
    return M.iso3_g2(M.sswu_g2(u))


def sgn0_class(u):
    """which term of sgn0(u) = s0 | (z0 & s1) decides: 's0' (odd real part), 'z0_s1' / 'z0_ns1' (zero real part, odd / even imaginary part),
    'nz_even' (non-zero even real part: the imaginary part must NOT matter)"""
    if u[0] % 2:
        return "s0"
    if u[0] % P == 0:
        return "z0_s1" if u[1] % 2 else "z0_ns1"
    return "nz_even"


def neg(u):
    return M.f2_neg(u)


def model_h(u0, u1):
    return M.clear_cofactor_g2(M.g2_add(q(u0), q(u1)))


# name -> predicate on (u0, u1); `e` below is 0 for u0, 1 for u1
PRED = {
    "q_equal": lambda u0, u1: q(u0) is not None and M.g2_eq(q(u0), q(u1)),
    "q_opposite": lambda u0, u1: q(u0) is not None and M.g2_eq(q(u0), M.g2_neg(q(u1))),
    "q_general": lambda u0, u1: not M.f2_eq(q(u0)[0], q(u1)[0]),
    "inputs_differ": lambda u0, u1: not M.f2_eq(u0, u1) and not M.f2_eq(u0, neg(u1)),
    "same_tv2": lambda u0, u1: M.f2_eq(tv2(u0), tv2(u1)),
    "h_infinity": lambda u0, u1: model_h(u0, u1) is None,
}
for _e in (0, 1):
    PRED["tv2_zero_%d" % _e] = lambda u0, u1, e=_e: M.f2_is_zero(tv2((u0, u1)[e]))
    PRED["tv2_nonzero_%d" % _e] = lambda u0, u1, e=_e: not M.f2_is_zero(tv2((u0, u1)[e]))
    PRED["sq_%d" % _e] = lambda u0, u1, e=_e: gx1_is_square((u0, u1)[e])
    PRED["nsq_%d" % _e] = lambda u0, u1, e=_e: not gx1_is_square((u0, u1)[e])
    for _c in ("s0", "z0_s1", "z0_ns1", "nz_even"):
        PRED["sgn0_%d:%s" % (_e, _c)] = lambda u0, u1, e=_e, c=_c: sgn0_class((u0, u1)[e]) == c

SGN0_VALUES = [(0, 1), (0, 2), (0, P - 1), (0, P - 2), (1, 0), (2, 0), (P - 1, 0), (P - 1, P - 1), (P - 1, P - 2)]
DEGENERATE = ("zero_both", "zero_first", "zero_second", "same", "neg", "twin_same", "twin_neg")
MAX_CASES = 48


class Case:
    __slots__ = ("name", "u0", "u1", "preds", "point", "expected")

    def __init__(self, name, u0, u1, preds):
        self.name, self.u0, self.u1, self.preds = name, u0, u1, tuple(preds)
        for p in self.preds:
            assert PRED[p](u0, u1), "case %s no longer satisfies %s" % (name, p)
        self.point = model_h(u0, u1)
        self.expected = M.g2_compress(self.point)

    @property
    def packed(self):
        """the 192 bytes mbls_map_to_g2_probe takes: u0.c0, u0.c1, u1.c0, u1.c1, 48 bytes big-endian each"""
        return b"".join(c.to_bytes(48, "big") for c in (self.u0[0], self.u0[1], self.u1[0], self.u1[1]))

    def __repr__(self):
        return "<map case %s>" % self.name


def sgn0_name(u):
    return "_".join("p-%d" % (P - c) if c > P // 2 else "%d" % c for c in u)


def find_twins(rng, draws=64):
    """(u0, u1, -u1) with Z u1^2 = -1 - Z u0^2 and gx1(u0) a square: tv1' = -1 - tv1 gives tv2' = tv2, hence the same x1, hence -- gx1 being a square -- the same
    x and y = +-sqrt(gx1) with the sign sgn0(u) asks for: q(u1) = +-q(u0) although u1 != +-u0. Each condition holds for about half of all u0."""
    zi = M.f2_inv(Z)
    for _ in range(draws):
        u0 = (rng.randrange(P), rng.randrange(P))
        if not gx1_is_square(u0):
            continue
        u1 = M.f2_sqrt(M.f2_mul(M.f2_sub(M.f2_neg(M.F2_ONE), M.f2_mul(Z, M.f2_sqr(u0))), zi))
        if u1 is None or M.f2_is_zero(u1):
            continue
        return u0, u1, neg(u1)
    raise AssertionError("no twin pair within %d draws" % draws)


@functools.lru_cache(maxsize=None)
def cases():
    """the list, in a fixed order; built (and every predicate asserted) once per process"""
    rng = random.Random(SEED)
    rnd = lambda: (rng.randrange(P), rng.randrange(P))      # noqa: E731
    zero = (0, 0)
    out = []
    v = rnd()
    out.append(Case("zero_both", zero, zero, ("tv2_zero_0", "tv2_zero_1", "q_equal")))
    out.append(Case("zero_first", zero, v, ("tv2_zero_0", "tv2_nonzero_1", "q_general")))
    out.append(Case("zero_second", v, zero, ("tv2_nonzero_0", "tv2_zero_1", "q_general")))
    out.append(Case("same", v, v, ("q_equal", "tv2_nonzero_0")))
    out.append(Case("neg", v, neg(v), ("q_opposite", "tv2_nonzero_0", "h_infinity")))
    t0, ta, tb = find_twins(rng)
    same, opp = (ta, tb) if M.f2_sgn0(ta) == M.f2_sgn0(t0) else (tb, ta)
    out.append(Case("twin_same", t0, same, ("inputs_differ", "same_tv2", "q_equal", "sq_0", "sq_1")))
    out.append(Case("twin_neg", t0, opp, ("inputs_differ", "same_tv2", "q_opposite", "sq_0", "sq_1", "h_infinity")))
    for u in SGN0_VALUES:
        w = rnd()
        out.append(Case("sgn0_%s_first" % sgn0_name(u), u, w, ("sgn0_0:%s" % sgn0_class(u), "tv2_nonzero_0", "q_general")))
        out.append(Case("sgn0_%s_second" % sgn0_name(u), w, u, ("sgn0_1:%s" % sgn0_class(u), "tv2_nonzero_1", "q_general")))
    for want, tag in ((True, "sq"), (False, "nsq")):
        for k in range(2):
            pair = []
            while len(pair) < 2:
                u = rnd()
                if gx1_is_square(u) == want:
                    pair.append(u)
            out.append(Case("%s_%d" % (tag, k), pair[0], pair[1], ("%s_0" % tag, "%s_1" % tag, "q_general")))
    for k in range(8):
        out.append(Case("plain_%d" % k, rnd(), rnd(), ("q_general", "tv2_nonzero_0", "tv2_nonzero_1")))
    assert len(out) <= MAX_CASES and len({c.name for c in out}) == len(out)
    # the list as a whole: every sgn0 class in both positions, both square classes, every degenerate branch
    have = {p for c in out for p in c.preds}
    for e in (0, 1):
        assert {"sgn0_%d:%s" % (e, c) for c in ("s0", "z0_s1", "z0_ns1", "nz_even")} <= have
        assert {"tv2_zero_%d" % e, "sq_%d" % e, "nsq_%d" % e} <= have
    assert {"q_equal", "q_opposite", "h_infinity"} <= have
    return tuple(out)


def by_name():
    return {c.name: c for c in cases()}


def plain():
    return [c for c in cases() if c.name.startswith("plain_")]


def sgn0_representatives():
    """one case of each sgn0 class (the first in list order)"""
    seen, out = set(), []
    for c in cases():
        for p in c.preds:
            if p.startswith("sgn0_") and p.split(":")[1] not in seen:
                seen.add(p.split(":")[1]); out.append(c)
    return out


def check_isogeny_has_no_rational_pole():
    """The 3-isogeny's denominators are (x + k)^2 and (x + k)^3 (the kernels keep Z = x + k as the Jacobian Z), and the only pole x = -k has g(-k) a NON-square
    of Fp2: no point of E'(Fp2) has that x, so no rational point maps to infinity, Z = x + k is never 0 and the kernels need no branch for it."""
    c0, c1, c2 = M.ISO3_XDEN
    assert c2 == M.F2_ONE and M.f2_is_zero(M.f2_sub(M.f2_sqr(c1), M.f2_muls(c0, 4)))          # discriminant 0: a double root
    k = M.f2_mul(c1, (M.fp_inv(2), 0))
    lin = [k, M.F2_ONE]
    sq = M._poly_mul(lin, lin)
    assert [M.f2(*c) for c in sq] == [M.f2(*c) for c in M.ISO3_XDEN]
    assert [M.f2(*c) for c in M._poly_mul(sq, lin)] == [M.f2(*c) for c in M.ISO3_YDEN]
    x = neg(k)
    g = M.f2_add(M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.f2_mul(A, x)), B)
    assert not M.f2_is_zero(g) and not M.f2_is_square(g)
    return k
