"""Operands for the two halves of the pairing -- the Miller loop and the final exponentiation -- at the inputs no verification reaches, shared by
tests/test_pairing_cases_cpu.py (the host emulator's compiled bodies, tools/coop_sim.py) and tests/test_gpu_pairing.py (mbls_miller_probe, mbls_final_exp_probe).
Two lists of named cases; every predicate a case names is evaluated with the Python model (oracle/pymodel) when the list is built (fe_cases() / miller_cases()
raise if one fails), so which branches a list provably enters is a property of the list, not of anything observed on a GPU.

FINAL EXPONENTIATION. A case is an element f of Fp12 (the model's order: coefficients of w^0..w^5) and the value the routines must give for it:
M.f12_pow(M.final_exp(f), 3) -- they compute the CUBE of f^((p^12-1)/r), their hard part is 3 (p^4-p^2+1)/r (mbls_pairing.h). Branches covered: a compressed state
that is all zero (every element the easy part sends to 1: 1, -1, elements of Fp, Fp2, Fp4, Fp6, w Fp6, a single non-zero coefficient; the "zero denominator ->
decompress to 1" path of prog_fexp_pinv / decompress12), the general decompression (z2 != 0) for everything else, a result that is exactly 1 behind a general chain
(r-th powers, a genuine valid Miller product), elements already cyclotomic / unitary, coefficients at p - 1, and 0 (not invertible: only `is_one == 0` is asked).
OUT OF SCOPE: a record of the compressed chain with z2 = 0 and z3 != 0. A full-routine input for it would be an element of the cyclotomic subgroup on a variety of
codimension 2; no construction is known, so no case here enters that branch. Its body stays covered by test_compressed_squaring_decompression_formulas on the
interpreter.

MILLER LOOP. A case is (apk: G1 Jacobian, sig: G2 affine with y = 0 for infinity, H: G2 Jacobian), as the workspace holds them. The GPU's projective formulas and
the model's affine lines differ by factors in Fp2, Fp4 and Fp6, which the easy part f -> f^((p^6-1)(p^2+1)) kills: the comparison is easy(f_gpu) == easy(f_model),
exactly, with f_model = M.miller_loop on the affine points (where the model's value lies in Fp4 -- x_P = 0, an infinite member -- the GPU's must lie there too). Three expectations per case: `two` = f(sig, -G1) f(H, apk), `one` = f(H, apk), `s` = f(H, -G1) (the
form that reads H as the signature sum S). Branches covered: every projective representative (Z = 1, Z = p - 1, small, random, Z in Fp2 with a zero real part),
keys outside G1 among them x_P = 0 (every c2 coefficient vanishes: the lines and f(H, apk) lie in Fp4), an infinite member in either slot of either pair, equal and opposite G2 arguments in the
two pairs, the same G1 argument in both pairs. Every G2 argument is checked to keep the loop's incomplete formulas regular (never T = +-Q, never T = O); points
for which they are not lie outside G2, the verdict kernel rejects them and their Miller value is not defined. No twist point has x = 0 (4 (1 + i) is not a
square: check_no_twist_point_with_x_zero), so there is no such case."""
import functools
import random

from pymodel import bls12_381 as M

import edge_points as E

P, R = M.P, M.R
SEED = 0x70616972                # every random element below comes from this one seed
MAX_CASES = 48
ZERO12 = [M.F2_ZERO] * 6
NEG_G1 = M.g1_neg(M.G1)


# ---------------------------------------------------------------------------------------------- layouts
def tower_of(model12):
    """model [a0, b0, a1, b1, a2, b2] (w^0..w^5) -> the kernels' order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) = (w^0, w^2, w^4, w^1, w^3, w^5)"""
    return [model12[2 * j + h] for h in range(2) for j in range(3)]


def model_of(tower):
    return [tower[0], tower[3], tower[1], tower[4], tower[2], tower[5]]


def pack12(model12):
    """the 576 bytes both probes use for an element of Fp12: 12 canonical 48-byte big-endian coefficients in the kernels' order"""
    return b"".join(c.to_bytes(48, "big") for co in tower_of(model12) for c in co)


def unpack12(b576):
    v = [int.from_bytes(b576[48 * i:48 * i + 48], "big") for i in range(12)]
    return model_of([(v[2 * e], v[2 * e + 1]) for e in range(6)])


# ---------------------------------------------------------------------------------------------- the model's own quantities
def easy(f):
    """f^((p^6 - 1)(p^2 + 1))"""
    t = M.f12_mul(M.f12_conj(f), M.f12_inv(f))
    return M.f12_mul(M.f12_frob(M.f12_frob(t)), t)


def in_fp4(f):
    """a + b w^3"""
    return all(M.f2_is_zero(f[k]) for k in (1, 2, 4, 5))


def is_zero12(f):
    return all(M.f2_is_zero(c) for c in f)


def frob_n(f, n):
    for _ in range(n):
        f = M.f12_frob(f)
    return f


@functools.lru_cache(maxsize=None)
def _fe(key):
    f = [tuple(c) for c in key]
    return M.final_exp(f)


def fe(f):
    """the model's final exponentiation, once per element and process (0.3 s each)"""
    return _fe(tuple(tuple(c) for c in f))


def is_cyclotomic(f):
    """f^(p^4 - p^2 + 1) = 1"""
    return M.f12_eq(M.f12_mul(frob_n(f, 4), f), frob_n(f, 2))


FE_PRED = {
    "fe_is_one": lambda f: M.f12_is_one(fe(f)),
    "fe_not_one": lambda f: not M.f12_is_one(fe(f)),
    "easy_is_one": lambda f: M.f12_is_one(easy(f)),
    "easy_not_one": lambda f: not M.f12_is_one(easy(f)),
    "cyclotomic": is_cyclotomic,
    "not_cyclotomic": lambda f: not is_cyclotomic(f),
    "unitary": lambda f: M.f12_is_one(M.f12_mul(f, M.f12_conj(f))),
    "zero": is_zero12,
    "one_coefficient": lambda f: sum(1 for c in f if not M.f2_is_zero(c)) == 1,
    "in_fp6": lambda f: all(M.f2_is_zero(f[k]) for k in (1, 3, 5)),
    "in_w_fp6": lambda f: all(M.f2_is_zero(f[k]) for k in (0, 2, 4)),
    "in_fp4": in_fp4,
    "all_coefficients_p_minus_1": lambda f: all(c == (P - 1, P - 1) for c in f),
}


class FeCase:
    __slots__ = ("name", "f", "preds", "expected", "is_one")

    def __init__(self, name, f, preds):
        self.name, self.f, self.preds = name, [(c[0] % P, c[1] % P) for c in f], tuple(preds)
        for p in self.preds:
            assert FE_PRED[p](self.f), "case %s no longer satisfies %s" % (name, p)
        if is_zero12(self.f):
            self.expected, self.is_one = None, False          # not invertible: no value is defined, only "not one"
        else:
            self.expected = M.f12_pow(fe(self.f), 3)
            self.is_one = M.f12_is_one(self.expected)
            assert self.is_one == M.f12_is_one(fe(self.f))    # gcd(3, r) = 1
            if "easy_is_one" in self.preds:
                assert self.is_one

    @property
    def packed(self):
        """the 576 bytes mbls_final_exp_probe takes"""
        return pack12(self.f)

    @property
    def expected_packed(self):
        return None if self.expected is None else pack12(self.expected)

    def __repr__(self):
        return "<final-exponentiation case %s>" % self.name


def check_rth_powers_are_the_kernel():
    """r divides p^12 - 1 exactly once: the r-th powers are exactly the elements the final exponentiation sends to 1"""
    n = P ** 12 - 1
    assert n % R == 0 and n % (R * R) != 0


def coeff_name(c):
    return "p-1" if c == P - 1 else "half" if c == (P - 1) // 2 else "%d" % c


@functools.lru_cache(maxsize=None)
def valid_and_spoiled():
    """(sk, pk, H, sig, H') of one honest item and the point of another message"""
    rng = random.Random(SEED + 1)
    sk = rng.randrange(1, R)
    h = M.hash_to_curve_g2(b"pairing cases: the valid item")
    return sk, M.sk_to_pk(sk), h, M.g2_mul(h, sk), M.hash_to_curve_g2(b"pairing cases: the spoiled item")


@functools.lru_cache(maxsize=None)
def fe_cases():
    """the list, in a fixed order; built (and every predicate asserted) once per process"""
    check_rth_powers_are_the_kernel()
    rng = random.Random(SEED)
    rf = lambda: rng.randrange(P)                                   # noqa: E731
    rnd12 = lambda: [(rf(), rf()) for _ in range(6)]                # noqa: E731
    out = []
    for k in range(4):
        out.append(FeCase("general_%d" % k, rnd12(), ("easy_not_one", "fe_not_one", "not_cyclotomic")))
    sk, pk, h, sig, h2 = valid_and_spoiled()
    out.append(FeCase("miller_valid", M.miller_loop([(sig, NEG_G1), (h, pk)]), ("fe_is_one", "easy_not_one")))
    out.append(FeCase("miller_spoiled", M.miller_loop([(sig, NEG_G1), (h2, pk)]), ("fe_not_one", "easy_not_one")))
    # what the easy part sends to 1
    out.append(FeCase("one", M.F12_ONE, ("easy_is_one",)))
    out.append(FeCase("minus_one", [(P - 1, 0)] + [M.F2_ZERO] * 5, ("easy_is_one",)))
    out.append(FeCase("in_fp", [(rf(), 0)] + [M.F2_ZERO] * 5, ("easy_is_one", "one_coefficient")))
    out.append(FeCase("in_fp2", [(rf(), rf())] + [M.F2_ZERO] * 5, ("easy_is_one", "one_coefficient")))
    out.append(FeCase("in_fp6", [(rf(), rf()) if k % 2 == 0 else M.F2_ZERO for k in range(6)], ("easy_is_one", "in_fp6")))
    out.append(FeCase("in_fp4", [(rf(), rf()) if k in (0, 3) else M.F2_ZERO for k in range(6)], ("easy_is_one", "in_fp4")))
    out.append(FeCase("in_w_fp6", [(rf(), rf()) if k % 2 == 1 else M.F2_ZERO for k in range(6)], ("easy_is_one", "in_w_fp6")))
    # r-th powers: exactly the kernel
    zeta = fe(M.miller_loop([(M.G2, M.G1)]))                        # e(G1, G2): a primitive r-th root of unity
    u = rnd12()
    sparse = [(rf(), 0), M.F2_ZERO, M.F2_ZERO, (0, rf()), M.F2_ZERO, (1, 0)]
    ur = M.f12_pow(u, R)
    out.append(FeCase("rth_power", ur, ("fe_is_one", "easy_not_one")))
    out.append(FeCase("rth_power_of_sparse", M.f12_pow(sparse, R), ("fe_is_one", "easy_not_one")))
    out.append(FeCase("rth_power_times_zeta", M.f12_mul(ur, zeta), ("fe_not_one", "easy_not_one")))
    out.append(FeCase("zeta", zeta, ("fe_not_one", "cyclotomic", "unitary")))
    v = rnd12()
    out.append(FeCase("cyclotomic", easy(v), ("cyclotomic", "unitary", "fe_not_one")))
    out.append(FeCase("unitary", M.f12_mul(M.f12_conj(v), M.f12_inv(v)), ("unitary", "not_cyclotomic", "fe_not_one")))
    # the limits of the import and of the first products: the shape of a line
    for k in range(6):
        for c in (1, P - 1, (P - 1) // 2):
            if k == 0 and c in (1, P - 1):
                continue                                            # (one / minus_one above)
            f = [M.F2_ZERO] * 6
            f[k] = (c, 0)
            out.append(FeCase("w%d_times_%s" % (k, coeff_name(c)), f, ("easy_is_one", "one_coefficient")))
    out.append(FeCase("all_p_minus_1", [(P - 1, P - 1)] * 6, ("all_coefficients_p_minus_1", "easy_not_one", "fe_not_one")))
    out.append(FeCase("all_ones", [(1, 1)] * 6, ("easy_not_one", "fe_not_one")))
    out.append(FeCase("zero", ZERO12, ("zero",)))
    assert len(out) <= MAX_CASES and len({c.name for c in out}) == len(out)
    have = {p for c in out for p in c.preds}
    assert {"fe_is_one", "fe_not_one", "easy_is_one", "cyclotomic", "unitary", "zero", "in_fp6", "in_fp4", "in_w_fp6", "all_coefficients_p_minus_1"} <= have
    return tuple(out)


def fe_by_name():
    return {c.name: c for c in fe_cases()}


def fe_general():
    return [c for c in fe_cases() if c.name.startswith("general_")]


# ---------------------------------------------------------------------------------------------- Miller cases
def g1_affine(j):
    X, Y, Z = j
    if Z % P == 0:
        return None
    zi = M.fp_inv(Z)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def g2_affine(j):
    X, Y, Z = j
    if M.f2_is_zero(Z):
        return None
    zi = M.f2_inv(Z); zi2 = M.f2_sqr(zi)
    return (M.f2_mul(X, zi2), M.f2_mul(Y, M.f2_mul(zi2, zi)))


def g1_scaled(pt, lam):
    return (pt[0] * lam * lam % P, pt[1] * lam * lam * lam % P, lam % P)


def g2_scaled(pt, mu):
    m2 = M.f2_sqr(mu)
    return (M.f2_mul(pt[0], m2), M.f2_mul(pt[1], M.f2_mul(m2, mu)), (mu[0] % P, mu[1] % P))


def sig_affine(sig):
    """the workspace's form (x, y) with y = 0 for infinity -> the model's point"""
    return None if M.f2_is_zero(sig[1]) else sig


def loop_is_regular(q):
    """the loop over |x| from T = Q never doubles T = O and never adds T = +-Q or T = O: what the incomplete formulas of mbls_pairing.h need"""
    if q is None:
        return True
    t = q
    for bit in bin(M.X_ABS)[3:]:
        if t is None or M.f2_is_zero(t[1]):
            return False
        t = M.g2_add(t, t)
        if bit == "1":
            if t is None or M.f2_eq(t[0], q[0]):
                return False
            t = M.g2_add(t, q)
    return t is not None


def check_no_twist_point_with_x_zero():
    """y^2 = 4 (1 + i) has no solution in Fp2: no point of the twist has x = 0"""
    assert not M.f2_is_square(M.B2)


MI_PRED = {
    "apk_on_curve": lambda c: M.g1_on_curve(g1_affine(c.apk)),
    "apk_in_g1": lambda c: M.subgroup_check_g1(g1_affine(c.apk)),
    "apk_outside_g1": lambda c: M.g1_on_curve(g1_affine(c.apk)) and not M.subgroup_check_g1(g1_affine(c.apk)),
    "apk_x_zero": lambda c: g1_affine(c.apk)[0] == 0,
    "one_pair_value_in_fp4": lambda c: in_fp4(c.model["one"]) and not M.f12_is_one(c.model["one"]),
    "apk_is_neg_g1": lambda c: g1_affine(c.apk) == NEG_G1,
    "apk_z_one": lambda c: c.apk[2] == 1,
    "apk_z_not_one": lambda c: c.apk[2] not in (0, 1),
    "h_z_one": lambda c: c.h[2] == (1, 0),
    "h_z_not_one": lambda c: c.h[2] != (1, 0) and not M.f2_is_zero(c.h[2]),
    "h_z_imaginary": lambda c: c.h[2][0] == 0 and c.h[2][1] != 0,
    "apk_infinite": lambda c: c.apk[2] == 0 and c.apk[0] != 0 and c.apk[1] != 0,
    "h_infinite": lambda c: M.f2_is_zero(c.h[2]) and not M.f2_is_zero(c.h[0]) and not M.f2_is_zero(c.h[1]),
    "sig_infinite": lambda c: M.f2_is_zero(c.sig[1]),
    "sig_finite": lambda c: not M.f2_is_zero(c.sig[1]),
    "h_in_g2": lambda c: M.subgroup_check_g2(g2_affine(c.h)),
    "sig_in_g2": lambda c: M.subgroup_check_g2(sig_affine(c.sig)),
    "sig_equals_h": lambda c: M.g2_eq(sig_affine(c.sig), g2_affine(c.h)),
    "sig_opposite_h": lambda c: M.g2_eq(sig_affine(c.sig), M.g2_neg(g2_affine(c.h))),
    "loops_regular": lambda c: loop_is_regular(g2_affine(c.h)) and loop_is_regular(sig_affine(c.sig)),
    "valid_item": lambda c: M.f12_is_one(fe(c.model["two"])),
    "spoiled_item": lambda c: not M.f12_is_one(fe(c.model["two"])),
}
KINDS = ("two", "one", "s")


class MillerCase:
    __slots__ = ("name", "apk", "sig", "h", "preds", "same_as", "model", "expected")

    def __init__(self, name, apk, sig, h, preds, same_as=None):
        self.name, self.apk, self.sig, self.h, self.preds, self.same_as = name, apk, sig, h, tuple(preds) + ("loops_regular",), same_as
        pk, hq, sg = g1_affine(apk), g2_affine(h), sig_affine(sig)
        self.model = {"two": M.miller_loop([(sg, NEG_G1), (hq, pk)]), "one": M.miller_loop([(hq, pk)]), "s": M.miller_loop([(hq, NEG_G1)])}
        for p in self.preds:
            assert MI_PRED[p](self), "case %s no longer satisfies %s" % (name, p)
        if same_as is not None:                                      # another representative of the same points: the same affine points, hence the same value
            assert pk == g1_affine(same_as.apk) and M.g2_eq(hq, g2_affine(same_as.h)) and sig == same_as.sig, name
            assert all(M.f12_eq(self.model[k], same_as.model[k]) for k in KINDS)
        self.expected = {k: easy(self.model[k]) for k in KINDS}

    @property
    def packed(self):
        """the 624 bytes mbls_miller_probe takes: apk X, Y, Z; sig x.c0, x.c1, y.c0, y.c1; H X.c0, X.c1, Y.c0, Y.c1, Z.c0, Z.c1 -- 48 bytes big-endian each"""
        vals = list(self.apk) + [c for co in self.sig for c in co] + [c for co in self.h for c in co]
        return b"".join(v.to_bytes(48, "big") for v in vals)

    def contributes_one(self, kind):
        return M.f12_is_one(self.model[kind])

    def __repr__(self):
        return "<Miller case %s>" % self.name


def miller_value_matches(case, kind, b576, conjugated=False):
    """easy(f_gpu) == easy(f_model) for the 576 bytes a form exported; conjugated: the form leaves conj(f) (the loop's value before the sign of x is applied)"""
    e = _easy_of_bytes(bytes(b576))
    if e is None:
        return False
    if in_fp4(case.model[kind]) and not in_fp4(unpack12(b576)):      # x_P = 0, or an infinite member: the easy part alone would let any element of Fp6 pass
        return False
    return M.f12_eq(M.f12_conj(e) if conjugated else e, case.expected[kind])         # easy(conj f) = conj(easy f)


@functools.lru_cache(maxsize=4096)
def _easy_of_bytes(b576):
    """easy() of an exported value, once per distinct value (layouts repeat the list's cases); None for 0"""
    f = unpack12(b576)
    return None if is_zero12(f) else easy(f)


@functools.lru_cache(maxsize=None)
def miller_cases():
    check_no_twist_point_with_x_zero()
    rng = random.Random(SEED + 2)
    rf = lambda: rng.randrange(1, P)                                # noqa: E731
    g1r = lambda: M.g1_mul(M.G1, rng.randrange(1, R))               # noqa: E731
    g2r = lambda: M.g2_mul(M.G2, rng.randrange(1, R))               # noqa: E731
    aff = lambda s: (s[0], s[1])                                    # noqa: E731
    plain = ("apk_in_g1", "h_in_g2", "sig_in_g2", "sig_finite")
    out = []
    base = []
    for k in range(3):
        pk, hq, sg = g1r(), g2r(), g2r()
        base.append((pk, hq, sg))
        out.append(MillerCase("general_%d" % k, g1_scaled(pk, 1), aff(sg), g2_scaled(hq, (1, 0)), plain + ("apk_z_one", "h_z_one")))
    pk, hq, sg = base[0]
    g0 = out[0]
    for tag, lam in (("2", 2), ("p-1", P - 1), ("half", (P - 1) // 2), ("random", rf())):
        out.append(MillerCase("p_scaled_%s" % tag, g1_scaled(pk, lam), aff(sg), g2_scaled(hq, (1, 0)), plain + ("apk_z_not_one", "h_z_one"), same_as=g0))
    for tag, mu in (("i", (0, 1)), ("p-1", (P - 1, 0)), ("1+i", (1, 1)), ("random", (rf(), rf()))):
        out.append(MillerCase("q_scaled_%s" % tag, g1_scaled(pk, 1), aff(sg), g2_scaled(hq, mu), plain + ("apk_z_one", "h_z_not_one") + (("h_z_imaginary",) if tag == "i" else ()),
                              same_as=g0))
    out.append(MillerCase("both_scaled", g1_scaled(pk, rf()), aff(sg), g2_scaled(hq, (rf(), rf())), plain + ("apk_z_not_one", "h_z_not_one"), same_as=g0))
    # keys outside G1: the unchecked keys the reference multiplies in like any other
    for ell, t, _ in E.g1_torsion_points(rng, orders=E.TORSION_ORDERS[1:]):         # (the rational 3-torsion is (0, +-2): the two x0 points)
        name = "torsion_%d" % ell if t[0] else "torsion_3_x0_y%s" % ("2" if t[1] == 2 else "m2")
        out.append(MillerCase(name, g1_scaled(t, rf()), aff(sg), g2_scaled(hq, (rf(), rf())),
                              ("apk_outside_g1", "h_in_g2", "sig_in_g2") + (("apk_x_zero", "one_pair_value_in_fp4") if t[0] == 0 else ())))
    # infinite members: each contributes exactly 1
    junk1 = lambda: (rf(), rf(), 0)                                 # noqa: E731
    junk2 = lambda: ((rf(), rf()), (rf(), rf()), (0, 0))            # noqa: E731
    nosig = ((0, 0), (0, 0))
    hj, pj = g2_scaled(hq, (rf(), rf())), g1_scaled(pk, rf())
    out.append(MillerCase("apk_infinite", junk1(), aff(sg), hj, ("apk_infinite", "sig_finite")))
    out.append(MillerCase("h_infinite", pj, aff(sg), junk2(), ("h_infinite", "sig_finite")))
    out.append(MillerCase("sig_infinite", pj, nosig, hj, ("sig_infinite", "apk_in_g1", "h_in_g2")))
    out.append(MillerCase("apk_and_h_infinite", junk1(), aff(sg), junk2(), ("apk_infinite", "h_infinite", "sig_finite")))
    out.append(MillerCase("sig_and_apk_infinite", junk1(), nosig, hj, ("sig_infinite", "apk_infinite")))
    out.append(MillerCase("sig_and_h_infinite", pj, nosig, junk2(), ("sig_infinite", "h_infinite")))
    out.append(MillerCase("all_infinite", junk1(), nosig, junk2(), ("sig_infinite", "apk_infinite", "h_infinite")))
    # the two pairs of the two-pair form on related arguments: the loop must not care
    out.append(MillerCase("sig_equals_h", pj, aff(hq), hj, ("sig_equals_h", "apk_in_g1")))
    out.append(MillerCase("sig_opposite_h", pj, aff(M.g2_neg(hq)), hj, ("sig_opposite_h", "apk_in_g1")))
    out.append(MillerCase("apk_is_neg_g1", g1_scaled(NEG_G1, rf()), aff(sg), hj, ("apk_is_neg_g1", "sig_in_g2", "h_in_g2")))
    # one honest item and the same with another message's point
    sk, vpk, vh, vsig, vh2 = valid_and_spoiled()
    out.append(MillerCase("valid_item", g1_scaled(vpk, rf()), aff(vsig), g2_scaled(vh, (rf(), rf())), plain + ("valid_item",)))
    out.append(MillerCase("spoiled_item", g1_scaled(vpk, rf()), aff(vsig), g2_scaled(vh2, (rf(), rf())), plain + ("spoiled_item",)))
    assert len(out) <= MAX_CASES and len({c.name for c in out}) == len(out)
    have = {p for c in out for p in c.preds}
    assert {"apk_x_zero", "apk_outside_g1", "apk_infinite", "h_infinite", "sig_infinite", "sig_equals_h", "sig_opposite_h", "apk_is_neg_g1", "h_z_imaginary",
            "valid_item", "spoiled_item"} <= have
    by = {c.name: c for c in out}
    # an infinite member makes its pair's value exactly 1
    for name, kinds in (("apk_infinite", ("one",)), ("h_infinite", ("one", "s")), ("apk_and_h_infinite", ("one", "s")), ("all_infinite", KINDS), ("sig_and_h_infinite", KINDS),
                        ("sig_and_apk_infinite", ("two", "one"))):
        assert all(by[name].contributes_one(k) for k in kinds), name
    assert M.f12_eq(by["sig_infinite"].model["two"], by["sig_infinite"].model["one"]) and not by["sig_infinite"].contributes_one("two")
    return tuple(out)


def miller_by_name():
    return {c.name: c for c in miller_cases()}


def miller_general():
    return [c for c in miller_cases() if c.name.startswith("general_")]
