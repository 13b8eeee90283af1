"""CPU-only: the case list of tests/map_cases.py (field elements for the message phase after hash_to_field at the inputs no hashed message reaches) checked
against itself, and every model of the GPU forms run on it: the wave programs hashg2 / hashg2x4 in tools/coop_sim.py, the generated map_to_curve body and
the one-lane and two-lane routines in tools/asm_sim.py, the compiled lane body in the host emulator. tests/test_gpu_map.py repeats the list on the GPU."""
import ctypes as C
import os
import sys

import pytest

import helpers
import map_cases as mc

sys.path.insert(0, os.path.join(helpers.ROOT, "tools"))
from pymodel import bls12_381 as M  # noqa: E402

P = helpers.P
R384 = 1 << 384


def affine(X, Y, Z):
    if M.f2_is_zero(Z):
        return None
    zi = M.f2_inv(Z); zi2 = M.f2_sqr(zi)
    return (M.f2_mul(X, zi2), M.f2_mul(Y, M.f2_mul(zi2, zi)))


# ---------------------------------------------------------------------------------------------- the list itself
def test_case_list_self_checks():
    """cases() asserts every case's predicates with the model while it builds the list; here the properties of the list as a whole"""
    cs = mc.cases()
    assert len(cs) <= mc.MAX_CASES
    by = mc.by_name()
    assert set(mc.DEGENERATE) <= set(by) and len(mc.plain()) == 8
    for c in cs:
        assert len(c.packed) == 192 and len(c.expected) == 96
        assert c.point is None or M.subgroup_check_g2(c.point), c.name
        assert (c.point is None) == ("h_infinity" in c.preds) == (c.expected == mc.INF), c.name
    plain = {c.expected for c in mc.plain()}
    assert len(plain) == 8
    for c in cs:
        if not c.name.startswith("plain_"):
            assert c.expected not in plain, c.name
    # the twins reach q1 = +-q0 without equal inputs; same / neg reach it with them
    for name in ("twin_same", "twin_neg"):
        c = by[name]
        assert c.u1 not in (c.u0, mc.neg(c.u0)) and M.f2_eq(mc.x1(c.u0), mc.x1(c.u1))
    assert by["twin_same"].expected == M.g2_compress(M.clear_cofactor_g2(M.g2_add(mc.q(by["twin_same"].u0), mc.q(by["twin_same"].u0))))
    # zero_first and zero_second are the same sum in the other order
    assert by["zero_first"].expected == by["zero_second"].expected and by["zero_first"].u0 == by["zero_second"].u1 == (0, 0)
    assert {mc.sgn0_class(u) for u in mc.SGN0_VALUES} == {"s0", "z0_s1", "z0_ns1", "nz_even"}
    assert len(mc.sgn0_representatives()) == 4


def test_twin_search_is_bounded_and_loud():
    import random
    with pytest.raises(AssertionError, match="no twin pair"):
        mc.find_twins(random.Random(1), draws=0)


def test_isogeny_has_no_rational_pole():
    """x = -k, the double root of the isogeny's denominator, is the x of no point of E'(Fp2): the kernels' Jacobian Z = x + k is never 0"""
    k = mc.check_isogeny_has_no_rational_pole()
    for c in mc.cases()[:8]:
        for u in (c.u0, c.u1):
            assert not M.f2_is_zero(M.f2_add(M.sswu_g2(u)[0], k))


# ---------------------------------------------------------------------------------------------- the host emulator (the compiled lane body)
def test_host_emulator_on_the_whole_list(emul):
    cs = mc.cases()
    out = helpers.ob(96 * len(cs))
    emul.emul_map_to_g2(helpers.cb(b"".join(c.packed for c in cs)), C.c_uint64(len(cs)), out)
    bad = [c.name for i, c in enumerate(cs) if bytes(out)[96 * i:96 * i + 96] != c.expected]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- the wave programs
@pytest.fixture(scope="module")
def coop():
    import coop_sim as CS
    import gen_coop as G
    comp = {name: G.compile_program(G.PROGRAMS[name]()) for name in ("hashg2", "hashg2x4")}
    return G, CS, comp


def wave_cases():
    by = mc.by_name()
    return [by[n] for n in mc.DEGENERATE] + mc.sgn0_representatives()


@pytest.mark.parametrize("prog", ["hashg2", "hashg2x4"])
def test_wave_programs_on_the_degenerate_cases(coop, prog):
    G, CS, comp = coop
    ri = pow(R384, -1, P)
    for c in wave_cases():
        ws = {G.WS_U0: c.u0[0] * R384 % P, G.WS_U0 + 1: c.u0[1] * R384 % P, G.WS_U1: c.u1[0] * R384 % P, G.WS_U1 + 1: c.u1[1] * R384 % P}
        sim = CS.Sim(comp[prog], ws)
        sim.run()
        X, Y, Z = [(sim.ws[G.WS_H + 2 * e] * ri % P, sim.ws[G.WS_H + 2 * e + 1] * ri % P) for e in range(3)]
        assert M.g2_compress(affine(X, Y, Z)) == c.expected, (prog, c.name)


# ---------------------------------------------------------------------------------------------- the generated routines in asm_sim
@pytest.fixture(scope="module")
def T():
    import test_asm_sim_d_cpu as T
    return T


def sswu_inputs():
    """every sgn0_* and zero_* field element, once: (name, u)"""
    out, seen = [], set()
    for c in mc.cases():
        if c.name.startswith("sgn0_") and c.name.endswith("_first"):
            u = c.u0
        elif c.name == "zero_both":
            u = c.u0
        else:
            continue
        if u not in seen:
            seen.add(u); out.append((c.name, u))
    return out


@pytest.mark.parametrize("rec", [0, 1])
def test_generated_map_to_curve_body_on_sgn0_and_zero_inputs(T, rec):
    """the generated simplified-SWU + isogeny body, run-time records 0 and 1 (u0's and u1's slots), on u = 0 and on every sgn0 value of the list:
    the Jacobian point it stores against the model's iso3_g2(sswu_g2(u))"""
    import gen_fp_asm as gf
    t = T.t
    rout = dict(T.ROUT); rout.update(gf.pow_subroutines()); rout["mbls_fp_pow_pm3d4_asm_fn"] = gf.pow_body(gf.EXP_PM3D4)
    body, _ = t.build_g2("sswu")
    S = t.G2_SLOTS
    inputs = sswu_inputs()
    assert len(inputs) == 1 + len(mc.SGN0_VALUES)
    for name, u in inputs:
        m = T.Machine(rout); m.v[252] = T.LADDR
        m.s[68] = T.GBASE & 0xFFFFFFFF; m.s[69] = T.GBASE >> 32; m.s[70] = T.STRIDE * 4
        m.run(t.shell_constants())
        m.s[71] = rec * (T.STRIDE * 4 * 12 * 6)
        for i in range(2):
            T.ws_put(m, S["U"] + 6 * rec + i, u[i] * R384 % P)
        m.run(body)
        got = [T.ws_get(m, S["Q0"] + 6 * rec + i) * T.RI392 % P for i in range(6)]
        assert affine((got[0], got[1]), (got[2], got[3]), (got[4], got[5])) == mc.q(u), (name, rec)


def test_one_lane_routine_takes_the_fixup_on_equal_points(T):
    """q0 = q1: the first addition of the routine runs its doubling fix-up (every body against the model as it runs, H against the list)"""
    c = mc.by_name()["same"]
    want, log = T.hash_routine_one_lane([c.u0, c.u1])
    assert log[log.index("h_start") + 1:log.index("h_start") + 3] == ["add", "fix"]
    assert want is not None and M.g2_compress(want) == c.expected


def test_one_lane_routine_clears_the_cofactor_of_infinity(T):
    """q0 = -q1: the sum is infinity and stays infinity through both ladders, the three subtractions and the export (hash_routine_one_lane compares the
    accumulator and the stored H with the model's point: None)"""
    c = mc.by_name()["neg"]
    want, log = T.hash_routine_one_lane([c.u0, c.u1])
    assert want is None and c.expected == mc.INF
    assert "fix" not in log[:log.index("h_base1")]


def test_two_lane_routine_takes_the_fixup_on_equal_points(T):
    c = mc.by_name()["same"]
    want, log = T.hash_routine_two_lanes([c.u0, c.u1])
    assert log[log.index("h_q0") + 1:log.index("h_q0") + 3] == ["add", "fix"]
    assert want is not None and M.g2_compress(want) == c.expected
