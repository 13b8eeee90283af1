"""The two instruction cuts of the headline path, on the CPU (tools/asm_sim.py interprets what the generators emit):
the key sum of 96-byte keys on the isomorphic curve E_l: y^2 = x^3 + 4 l^6, l = 2^-196 (tools/gen_tower_d.py, mode "rawiso", with its leaf
mbls_fp_redc7_d_asm_fn), and the fused Fp4 squaring of the compressed cyclotomic squaring (mbls_fp4_sqr0_d_asm_fn inside `csqr`).
The helpers (big-integer models, the simulated workspace, affine chord-and-tangent arithmetic) are those of tests/test_asm_sim_d_cpu.py."""
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_fpd_asm as d          # noqa: E402
import gen_tower_d as t          # noqa: E402
import instr_census              # noqa: E402
import test_asm_sim_d_cpu as base   # noqa: E402
from asm_sim import Machine, s32, digits_signed, from_digits_signed   # noqa: E402

P = d.P
R392, R384 = 1 << 392, 1 << 384
RI392 = pow(R392, -1, P)
LAM = pow(1 << 196, -1, P)                      # l = 2^-196: (x, y) on E  <->  (l^2 x, l^3 y) on E_l
ROUT = {k: f() for k, f in d.ROUTINE_BODIES.items()}
normalised_digits, jac_affine, g1_add_affine, g1_mul_affine, G1_GEN = base.normalised_digits, base.jac_affine, base.g1_add_affine, base.g1_mul_affine, base.G1_GEN


def digits_at(value_digits):
    return [v & 0xFFFFFFFF for v in value_digits]


# ---------------------------------------------------------------------------------------------- the key sum on E_l
def test_redc7_leaf_against_big_integers():
    """a * 2^-196 mod p on random digits, on redundant signed digits, and on digits at the 32-bit limit the allocator admits (both signs):
    the 64-bit overflow assertion of the simulator stays silent, the result is normalised and lies in [a / 2^196, a / 2^196 + p]"""
    rng = random.Random(21)
    body = d.fp_redc7_d_body()
    assert sum(l.startswith("v_mad_i64_i32") for l in body) == 112 and len(body) == 160
    cases = [normalised_digits(x) for x in (0, 1, P - 1, P - 2)] + [normalised_digits(rng.randrange(P)) for _ in range(20)]
    cases += [digits_signed(rng.randrange(-3 * P, 4 * P), 1 << 29, rng) for _ in range(10)]
    lim = (1 << 31) - 1
    cases += [digits_at([lim] * 14), digits_at([-lim] * 14), digits_at([lim, -lim] * 7), digits_at([-lim, lim] * 7)]
    for dg in cases:
        a = from_digits_signed(dg)
        m = Machine(); m.run(d.load_constants())
        m.v[0:14] = dg
        m.run(body)
        r = from_digits_signed(m.v[70:84])
        assert (r - a * LAM) % P == 0
        assert (a >> 196) <= r <= (a >> 196) + P + 1
        assert all(0 <= s32(v) < (1 << 28) for v in m.v[70:83])
        assert m.v[0:14] == dg                                             # the operand survives


def lam_map(pt):
    return None if pt is None else (pt[0] * LAM * LAM % P, pt[1] * pow(LAM, 3, P) % P)


def test_g1_sum_step_on_the_isomorphic_curve():
    """one key into the running sum (mode "rawiso") against affine chord-and-tangent arithmetic on E mapped through l: general position, sum at
    infinity, key flagged infinite, key = -sum (result infinity), key = sum (the masks select the doubling body, which is then run),
    off-curve key, and a key with x = p - 1, y = p - 1 (in range; off the curve)"""
    step, _ = t.build_g1("rawiso")
    dbl, _ = t.build_g1("dbl")
    rng = random.Random(78)
    for case in ("general", "acc_inf", "key_inf", "inverse", "double", "offcurve", "pm1"):
        accp = g1_mul_affine(G1_GEN, rng.randrange(1, 1 << 64))
        key = g1_mul_affine(G1_GEN, rng.randrange(1, 1 << 64))
        if case == "inverse": key = (accp[0], P - accp[1])
        if case == "double": key = accp
        if case == "offcurve": key = (key[0], (key[1] + 1) % P)
        if case == "pm1": key = (P - 1, P - 1)
        z = rng.randrange(1, P)
        acc_l = lam_map(accp)                                               # the running sum lives on E_l
        acc = (acc_l[0] * z * z % P, acc_l[1] * z * z * z % P, z) if case != "acc_inf" else (rng.randrange(P), rng.randrange(P), 0)
        m = Machine(ROUT); m.run(t.shell_constants())
        m.s[("pair", 48)] = 1 if case == "key_inf" else 0
        for i in range(3):
            m.a[14 * i:14 * i + 14] = normalised_digits(acc[i] * R392 % P)
        m.v[112:126] = normalised_digits(key[0]); m.v[126:140] = normalised_digits(key[1])      # plain integers below p
        m.run(step)
        got = [from_digits_signed(m.a[14 * i:14 * i + 14]) for i in range(3)]
        for i in range(3):
            assert t.STATE_IN.vlo <= got[i] <= t.STATE_IN.vhi and all(0 <= s32(w) < (1 << 28) for w in m.a[14 * i:14 * i + 13])
        assert [from_digits_signed(m.a[14 * (5 + i):14 * (5 + i) + 14]) * RI392 % P for i in range(3)] == list(acc)     # the old sum, for the doubling
        got = [g * RI392 % P for g in got]
        h0, r0, i1, i2f = m.s[("pair", 52)], m.s[("pair", 54)], m.s[("pair", 84)], m.s[("pair", 86)]
        assert i2f == (1 if case in ("key_inf", "offcurve", "pm1") else 0), case
        assert i1 == (1 if case == "acc_inf" else 0)
        if case in ("inverse", "double"):
            assert h0 == 1 and r0 == (1 if case == "double" else 0)
        need_dbl = h0 and r0 and not i1 and not i2f
        assert bool(need_dbl) == (case == "double")
        if need_dbl:
            m.run(dbl)
            got = [from_digits_signed(m.a[14 * i:14 * i + 14]) * RI392 % P for i in range(3)]
        want = accp if case != "acc_inf" else None
        if case not in ("key_inf", "offcurve", "pm1"):
            want = g1_add_affine(want, key)
        assert jac_affine(*got) == lam_map(want), case                      # the sum on E_l ...
        X, Y, Z = got
        assert jac_affine(X, Y, Z * LAM % P) == want, case                  # ... is (X, Y, l Z) on E


def test_g1_sum_routine_shell_on_the_isomorphic_curve():
    """prologue, per-key fetch / decode / step / status, epilogue of the "rawiso" routine for one lane with the five-key list of the
    existing shell test (a repeated key, an infinite key, an undecodable key): slots 0..2 hold the sum ON E, the status is 3"""
    full, pieces, _ = t.g1_aggregate_d_routine("rawiso")
    assert not any("scratch" in l or "buffer_" in l for l in full)
    pts = [g1_mul_affine(G1_GEN, s) for s in (5, 7, 11)]
    keys = [pts[0], pts[1], "inf", pts[1], "bad", pts[2]]
    KEYS = 0x7E0000100000
    m = base.miller_machine(0)
    m.v[252] = base.LADDR
    words = lambda b: [int.from_bytes(b[4 * j:4 * j + 4], "little") for j in range(len(b) // 4)]
    for n_, kx in enumerate(keys + [pts[0]]):                      # one more record: the fetch runs a key ahead
        blob = bytes([0x40]) + bytes(95) if kx == "inf" else bytes([0x20]) + bytes(95) if kx == "bad" else kx[0].to_bytes(48, "big") + kx[1].to_bytes(48, "big")
        for j, w in enumerate(words(blob)):
            m.mem[KEYS + 96 * n_ + 4 * j] = w
    m.v[248], m.v[249] = KEYS & 0xFFFFFFFF, KEYS >> 32
    m.v[250] = len(keys)
    m.run(pieces["pro"])
    want = None
    for n_, kx in enumerate(keys):
        m.s[39] = n_
        m.run(pieces["decode"]); m.run(pieces["nxt"]); m.run(pieces["step"]); m.run(pieces["post"])
        h0, r0, i1, i2 = m.s[("pair", 52)], m.s[("pair", 54)], m.s[("pair", 84)], m.s[("pair", 86)]
        if h0 and r0 and not i1 and not i2:
            m.run(pieces["dbl"])
        if kx not in ("inf", "bad"):
            want = g1_add_affine(want, kx)
    m.run(pieces["epi"][1:-1])
    ri = pow(R384, -1, P)
    X, Y, Z = [base.ws_get(m, sl) * ri % P for sl in range(3)]
    assert all(base.ws_get(m, sl) < P for sl in range(3))
    assert jac_affine(X, Y, Z) == want
    assert m.v[251] == 3                                            # an infinite and an undecodable key were seen, the sum is finite


# ---------------------------------------------------------------------------------------------- the fused Fp4 squaring
def fp4_sqr0_model(a0, a1, b0, b1):
    """(a + b s)^2 = (a^2 + xi b^2) + 2 a b s with xi = 1 + i: the first half, on integers"""
    return a0 * a0 - a1 * a1 + (b0 * b0 - b1 * b1) - 2 * b0 * b1, 2 * a0 * a1 + (b0 * b0 - b1 * b1) + 2 * b0 * b1


def limit_of(bound_of):
    """the largest digit magnitude D for which the allocator's own test admits four operands bounded by bound_of(D)"""
    ok = lambda D: t.AllocD.call_limits_ok(None, "fp4sqr0", [bound_of(D)] * 4)
    lo, hi = 1, 1 << 31
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def test_fp4_sqr0_leaf_against_big_integers():
    """the fused scan on random redundant digits and on digits AT the input limits the allocator assumes (call_limits_ok), non-negative and
    of both signs: no 64-bit column overflows (the simulator asserts), results right mod p, normalised, inside call_bounds, operands intact"""
    rng = random.Random(31)
    body = d.fp4_sqr0_d_body()
    assert sum(l.startswith("v_mad_i64_i32") for l in body) == 4 * 196 + 2 * 196
    d_signed = limit_of(lambda D: t.Bound(-D, D, -D, D, -(D << 365), D << 365))
    d_plain = limit_of(lambda D: t.Bound(0, D, 0, D, 0, D << 365))
    assert d_plain >= (1 << 28) - 1                       # normalised operands never need narrowing
    print("fp4sqr0 input limits: signed digits", d_signed, "non-negative digits", d_plain)
    cases = []
    for trial in range(24):
        dm = [1 << 27, 1 << 27, 1 << 26][trial % 3]
        vals = [rng.randrange(-2 * P, 3 * P) for _ in range(4)] if trial else [0, 1, P - 1, -P]
        cases.append([digits_signed(x, dm, rng) for x in vals])
    for signs in range(16):                                # every sign pattern of the four operands at the signed limit
        cases.append([digits_at([d_signed if (signs >> i) & 1 else -d_signed] * 14) for i in range(4)])
    for pat in range(16):                                  # all-zero / all-maximal non-negative digits
        cases.append([digits_at([d_plain if (pat >> i) & 1 else 0] * 14) for i in range(4)])
    cases.append([digits_at([d_signed, -d_signed] * 7), digits_at([-d_signed, d_signed] * 7), digits_at([d_signed, -d_signed] * 7), digits_at([d_signed] * 14)])
    for ops in cases:
        vals = [from_digits_signed(x) for x in ops]
        m = Machine(); m.run(d.load_constants())
        for i, x in enumerate(ops):
            m.v[14 * i:14 * i + 14] = x
        m.run(body)
        c0, c1 = from_digits_signed(m.v[70:84]), from_digits_signed(m.v[84:98])
        w0, w1 = fp4_sqr0_model(*vals)
        assert (c0 - w0 * RI392) % P == 0 and (c1 - w1 * RI392) % P == 0
        assert all(0 <= s32(v) < (1 << 28) for v in m.v[70:83] + m.v[84:97])
        a0, a1, b0, b1 = [abs(v) for v in vals]
        for c, first in ((c0, (a0 + a1) * (a0 + a1)), (c1, 2 * a0 * a1)):
            X = (first + (b0 + b1) * (b0 + b1) + 2 * b0 * b1) // R392 + 2
            assert -X <= c <= P + X                                                 # what product_bound promises the callers
        assert [m.v[14 * i:14 * i + 14] for i in range(4)] == ops


def csqr_state_digits(x, rng):
    """a loop-carried value as the body may meet it: canonical on the first round, the representative nearest to zero afterwards"""
    rep = x * R392 % P
    return normalised_digits(rep - P if rep > P // 2 and rng.getrandbits(1) else rep)


def test_fused_compressed_squaring_body():
    """the built `csqr` body (both Fp4 squarings fused) against the UNFUSED recorded program run on field values: random states, the
    all-zero state (the element 1), z2 = 0, z4 = z5 = 0 -- five squarings in a row each; after every squaring the values agree mod p, lie
    inside REDUCED and their digits are normalised"""
    p = t.fuse_fp4_squarings(t.prog_fexp_csqr())
    assert p.fused_fp4 == 2 and [o[0] for o in p.ops].count("fp4sqr0") == 2 and not any(o[0] == "sqr" for o in p.ops)
    assert [o[0] for o in t.prog_fexp_csqr().ops].count("sqr") == 6                       # the recorded program is what it was
    empty = t.Prog(); assert t.fuse_fp4_squarings(empty).ops == []
    body, _ = t.build_fexp("csqr")
    assert not any(l.startswith("CALL") or "scratch" in l or "buffer_" in l for l in body)
    rng = random.Random(32)
    homes = t.CSTATE_HOME
    for kind in ("random", "random", "one", "z2=0", "z4=z5=0"):
        z = [rng.randrange(P) for _ in range(8)]
        if kind == "one": z = [0] * 8
        if kind == "z2=0": z[0] = z[1] = 0
        if kind == "z4=z5=0": z[4:8] = [0] * 4
        m = base.miller_machine(0); m.run(t.shell_constants())
        for i, (bank, blk) in enumerate(homes):
            getattr(m, bank)[14 * blk:14 * blk + 14] = csqr_state_digits(z[i], rng)
        state = {homes[i]: z[i] for i in range(8)}
        for rnd_ in range(5):
            m.run(body)
            mp = base.run_model(t.prog_fexp_csqr, state, {})
            state = dict(mp.out_home)
            assert set(state) == set(homes)
            for (bank, blk) in homes:
                dg = getattr(m, bank)[14 * blk:14 * blk + 14]
                got = from_digits_signed(dg)
                assert (got - state[(bank, blk)] * R392) % P == 0, (kind, rnd_, bank, blk)
                assert t.REDUCED.vlo <= got <= t.REDUCED.vhi and all(0 <= s32(w) < (1 << 28) for w in dg[:13]), (kind, rnd_, bank, blk)
        if kind == "one":
            assert all(v == 0 for v in state.values())


# ---------------------------------------------------------------------------------------------- counts
@pytest.fixture(scope="module")
def census():
    return instr_census.compute()


def test_instruction_counts(census):
    """what the cuts are for: the squaring body's multiply-accumulates and instructions, the key sum's instructions per item"""
    cs = census["routines"]["final_exp_d_csqr"]
    total = cs["valu"] + cs["salu"] + cs["lds"]
    print("csqr: multiply-accumulates", cs["mad_u64_u32"], "instructions", total, "(before the fusion: 4928 and 7064)")
    assert cs["mad_u64_u32"] <= 4536 and total < 7064
    agg = census["per_item"]["k_aggregate"]["valu"]
    print("k_aggregate valu per item:", agg, "(the form it replaced:", census["per_item"]["k_aggregate_raw_form"]["valu"], ")")
    assert census["per_item"]["k_aggregate_raw_form"]["valu"] == 1077738
    assert agg <= 1020000


def test_committed_census_is_fresh(census):
    with open(instr_census.CENSUS_PATH) as f:
        assert json.load(f) == json.loads(json.dumps(census)), "profiles/instr_census.json is stale: run tools/instr_census.py"
