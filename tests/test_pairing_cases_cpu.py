"""CPU-only: the two case lists of tests/pairing_cases.py (operands of the Miller loop and of the final exponentiation at the inputs no verification reaches)
checked against themselves, the compiled bodies (lane_miller / miller_loop / final_exp of mbls_pairing.h in the host emulator) run on the WHOLE of both lists
with the comparison functions tests/test_gpu_pairing.py uses, and the wave programs vmfinal / miller1 / smiller run in tools/coop_sim.py on the classes
tests/test_coop_cpu.py does not already run. This is what proves the expected values and the comparison code before a GPU is involved."""
import ctypes as C
import os
import sys

import pytest

import helpers
import pairing_cases as pc

sys.path.insert(0, os.path.join(helpers.ROOT, "tools"))
from pymodel import bls12_381 as M  # noqa: E402

P = helpers.P
R384 = 1 << 384


# ---------------------------------------------------------------------------------------------- the lists themselves
def test_final_exponentiation_list_census():
    """fe_cases() asserts every case's predicates with the model while it builds the list; here the properties of the list as a whole"""
    cs = pc.fe_cases()
    by = pc.fe_by_name()
    assert len(cs) <= pc.MAX_CASES and len(by) == len(cs)
    assert len(pc.fe_general()) == 4
    for name in ("miller_valid", "miller_spoiled", "one", "minus_one", "in_fp", "in_fp2", "in_fp6", "in_fp4", "in_w_fp6", "rth_power", "rth_power_of_sparse",
                 "rth_power_times_zeta", "zeta", "cyclotomic", "unitary", "all_p_minus_1", "all_ones", "zero"):
        assert name in by, name
    lines = [c for c in cs if c.name.startswith("w") and "_times_" in c.name]
    assert len(lines) == 16 and {c.name.split("_")[0] for c in lines} == {"w%d" % k for k in range(6)}         # 6 x 3 less one / minus_one (listed by name)
    for c in cs:
        assert len(c.packed) == 576
        assert (c.expected is None) == (c.name == "zero")
        if "easy_is_one" in c.preds:
            assert c.is_one and c.expected == M.F12_ONE, c.name
        if "fe_is_one" in c.preds:
            assert c.is_one and "easy_is_one" not in c.preds, c.name             # 1 behind a general chain
        if "fe_not_one" in c.preds:
            assert not c.is_one, c.name
    assert sum(1 for c in cs if c.is_one) >= 20 and sum(1 for c in cs if not c.is_one) >= 10
    # the cube is what is expected, and it is not the plain value where that is not 1
    g = by["general_0"]
    assert not M.f12_eq(g.expected, pc.fe(g.f)) and M.f12_eq(g.expected, M.f12_mul(M.f12_sqr(pc.fe(g.f)), pc.fe(g.f)))
    # the byte layout: the kernels' order, c0.c1 (the coefficient of w^2) second
    f = [(10 * k + 1, 10 * k + 2) for k in range(6)]
    b = pc.pack12(f)
    assert int.from_bytes(b[96:144], "big") == 21 and int.from_bytes(b[3 * 96 + 48:4 * 96], "big") == 12 and pc.unpack12(b) == f


def test_miller_list_census():
    cs = pc.miller_cases()
    by = pc.miller_by_name()
    assert len(cs) <= pc.MAX_CASES and len(by) == len(cs)
    assert len(pc.miller_general()) == 3
    for name in ["p_scaled_%s" % t for t in ("2", "p-1", "half", "random")] + ["q_scaled_%s" % t for t in ("i", "p-1", "1+i", "random")] + [
            "both_scaled", "torsion_3_x0_y2", "torsion_3_x0_ym2", "torsion_11", "apk_infinite", "h_infinite", "sig_infinite", "apk_and_h_infinite",
            "sig_and_apk_infinite", "sig_and_h_infinite", "all_infinite", "sig_equals_h", "sig_opposite_h", "apk_is_neg_g1", "valid_item", "spoiled_item"]:
        assert name in by, name
    assert sum(1 for c in cs if "apk_outside_g1" in c.preds) == 6
    for c in cs:
        assert len(c.packed) == 624 and "loops_regular" in c.preds
        if c.same_as is not None:
            assert c.same_as.name == "general_0" and c.expected == c.same_as.expected
    # the expectations tell the cases apart: no two unrelated cases share a two-pair value, and a conjugated value does not pass. (The keys (0, +-2): with
    # x_P = 0 every line is c0 + c3 w^3, an element of Fp4, so f(H, apk) is one and the easy part sends it to 1 -- asserted when the list is built; the
    # two-pair value is then f(sig, -G1)'s for both, and what the case checks is that a zero px does not disturb the other pair or the accumulator.)
    for name in ("torsion_3_x0_y2", "torsion_3_x0_ym2"):
        assert "one_pair_value_in_fp4" in by[name].preds and M.f12_is_one(by[name].expected["one"]) and not by[name].contributes_one("one")
    seen = {}
    for c in cs:
        if c.same_as is None and "apk_x_zero" not in c.preds and not any(p.endswith("_infinite") for p in c.preds):
            key = pc.pack12(c.expected["two"])
            assert key not in seen, (c.name, seen.get(key))
            seen[key] = c.name
    g = by["general_0"]
    assert pc.miller_value_matches(g, "two", pc.pack12(g.model["two"]))
    assert not pc.miller_value_matches(g, "two", pc.pack12(g.model["two"]), conjugated=True)
    assert not pc.miller_value_matches(g, "two", pc.pack12(g.model["one"])) and not pc.miller_value_matches(g, "two", bytes(576))
    # a factor from a proper subfield does not matter, any other factor does
    sub = [(3, 4), pc.M.F2_ZERO, (5, 6), pc.M.F2_ZERO, (7, 8), pc.M.F2_ZERO]
    assert pc.miller_value_matches(g, "two", pc.pack12(M.f12_mul(g.model["two"], sub)))
    assert not pc.miller_value_matches(g, "two", pc.pack12(M.f12_mul(g.model["two"], [(3, 4), (1, 0)] + [pc.M.F2_ZERO] * 4)))
    # the valid item's product is in the kernel of the final exponentiation, the spoiled item's is not
    assert M.f12_is_one(pc.fe(by["valid_item"].model["two"])) and not M.f12_is_one(pc.fe(by["spoiled_item"].model["two"]))


def test_list_facts():
    pc.check_rth_powers_are_the_kernel()
    pc.check_no_twist_point_with_x_zero()
    # a point outside G2 can break the loop's formulas: the walker sees it (a point of order 2 does not exist on the twist; one of small order is met by a prefix)
    assert pc.loop_is_regular(M.G2) and pc.loop_is_regular(None)


# ---------------------------------------------------------------------------------------------- the compiled bodies (host emulator)
def emul_miller(emul, cases, one_pair):
    out = helpers.ob(576 * len(cases))
    emul.emul_miller(helpers.cb(b"".join(c.packed for c in cases)), C.c_uint64(len(cases)), out, C.c_int(one_pair))
    b = bytes(out)
    return [b[576 * i:576 * i + 576] for i in range(len(cases))]


def emul_final_exp(emul, cases):
    out, bits = helpers.ob(576 * len(cases)), helpers.ob(len(cases))
    emul.emul_final_exp(helpers.cb(b"".join(c.packed for c in cases)), C.c_uint64(len(cases)), out, bits)
    b = bytes(out)
    return [b[576 * i:576 * i + 576] for i in range(len(cases))], [bool(x) for x in bytes(bits)[:len(cases)]]


def fe_failures(cases, values, bits):
    """names of the cases whose value (where one is defined) or whose bit differs from the model's -- the comparison tests/test_gpu_pairing.py makes"""
    bad = []
    for c, v, b in zip(cases, values, bits):
        if b != c.is_one or (c.expected is not None and v is not None and v != c.expected_packed):
            bad.append(c.name)
    return bad


def miller_failures(cases, kind, values, conjugated=False):
    return [c.name for c, v in zip(cases, values) if not pc.miller_value_matches(c, kind, v, conjugated)]


def test_compiled_final_exponentiation_on_the_whole_list(emul):
    cs = pc.fe_cases()
    values, bits = emul_final_exp(emul, cs)
    assert fe_failures(cs, values, bits) == []


@pytest.mark.parametrize("one_pair,kind", [(0, "two"), (1, "one")], ids=["two_pair", "one_pair"])
def test_compiled_miller_loop_on_the_whole_list(emul, one_pair, kind):
    cs = pc.miller_cases()
    values = emul_miller(emul, cs, one_pair)
    assert miller_failures(cs, kind, values) == []
    # the convention matters: read as conjugates, only the values that are their own conjugates' equals (those the easy part sends to 1) still pass
    wrong = miller_failures(cs, kind, values, conjugated=True)
    assert set(wrong) == {c.name for c in cs if not M.f12_is_one(c.expected[kind])}


def test_compiled_bodies_compose(emul):
    """the two-pair value of the valid / the spoiled item, fed to the compiled final exponentiation: one / not one"""
    by = pc.miller_by_name()
    items = [by["valid_item"], by["spoiled_item"]]
    values = emul_miller(emul, items, 0)
    out, bits = helpers.ob(576 * 2), helpers.ob(2)
    emul.emul_final_exp(helpers.cb(b"".join(values)), C.c_uint64(2), out, bits)
    assert [bool(x) for x in bytes(bits)[:2]] == [True, False]


# ---------------------------------------------------------------------------------------------- the wave programs
@pytest.fixture(scope="module")
def coop():
    import coop_sim as CS
    import gen_coop as G
    return G, CS, {name: G.compile_program(G.PROGRAMS[name]()) for name in ("vmfinal", "miller1", "smiller")}


def mont(x):
    return x * R384 % P


@pytest.mark.parametrize("name", ["in_fp6", "rth_power", "rth_power_times_zeta", "zero"])
def test_vmfinal_verdict(coop, name):
    """slot F = f, 1 in slots 97..108 (what mbls_final_exp_probe sets up in its verdict mode): an element the easy part sends to 1, an r-th power (1 behind
    a general chain), the same times a primitive r-th root of unity, and 0 -- tests/test_coop_cpu.py runs a valid and a spoiled Miller product and F = 1"""
    G, CS, comp = coop
    c = pc.fe_by_name()[name]
    ws = {G.WS_F + i: mont(v) for i, v in enumerate(x for co in pc.tower_of(c.f) for x in co)}
    ws.update({G.WS_G + i: mont(1) if i == 0 else 0 for i in range(12)})
    assert CS.Sim(comp["vmfinal"], ws).run() is c.is_one


@pytest.mark.parametrize("prog,name", [("miller1", "torsion_3_x0_y2"), ("smiller", "q_scaled_i")])
def test_wave_miller_values(coop, prog, name):
    """miller1 on the key (0, 2) (x_P = 0: every c2 coefficient vanishes), smiller on a point whose Z has a zero real part: the stored value against the
    model's through the comparison the GPU file uses -- smiller's is the loop's value before the conjugation"""
    G, CS, comp = coop
    c = pc.miller_by_name()[name]
    ws = {G.WS_APK + i: mont(v) for i, v in enumerate(c.apk)}
    ws.update({(G.WS_S if prog == "smiller" else G.WS_H) + i: mont(v) for i, v in enumerate(x for co in c.h for x in co)})
    sim = CS.Sim(comp[prog], ws)
    sim.run()
    ri = pow(R384, -1, P)
    base = G.WS_G if prog == "smiller" else G.WS_F
    got = b"".join((sim.ws[base + i] * ri % P).to_bytes(48, "big") for i in range(12))
    kind, conj = ("s", True) if prog == "smiller" else ("one", False)
    assert pc.miller_value_matches(c, kind, got, conjugated=conj)
    if prog == "smiller":
        assert not pc.miller_value_matches(c, kind, got, conjugated=not conj)
    else:                         # x_P = 0: the value lies in Fp4 (the comparison asks for that too) and is not 1
        f = pc.unpack12(got)
        assert pc.in_fp4(f) and not M.f12_is_one(f) and M.f12_is_one(c.expected["one"])
