"""g1_tree_routine (tools/gen_tower_d.py) on the CPU: one level of the per-message sums of the blinded keys of the shared-message verify_multiple
(k_g1_seg_tree_d) -- the lane's own Jacobian point in slots 0..2 plus the one of the item s71 bytes further on -- interpreted by tools/asm_sim.py and compared
with oracle/pymodel's g1_add. The keys are whatever the callers passed (the verifiers run no KeyValidate), so the operands are points of E(Fp), not of G1: general
pairs, each of the exceptional cases (equal, opposite, either operand at infinity, both), and the torsion points of tests/edge_points.py on both sides.
The helpers (simulated workspace, Jacobian -> affine) are those of tests/test_asm_sim_d_cpu.py."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_tower_d as t          # noqa: E402
import test_asm_sim_d_cpu as base   # noqa: E402
import edge_points as E          # noqa: E402

P = base.P
R384 = 1 << 384
RI = pow(R384, -1, P)
PARTNER = 4 * 41                  # the partner item's byte offset (s71)
_R = {}


def routine():
    if not _R:
        _R["full"], _R["pieces"], _R["st"] = t.g1_tree_routine()
    return _R["full"], _R["pieces"]


def jac(rng, pt):
    """a random Jacobian form of the affine model point (None: infinity = Z = 0 with arbitrary X, Y)"""
    if pt is None:
        return [rng.randrange(P), rng.randrange(P), 0]
    z = rng.randrange(1, P)
    return [pt[0] * z * z % P, pt[1] * z * z * z % P, z]


def tree_add(rng, a, b):
    """the routine in its control order on acc = a (the lane's item), addend = b (the partner's) -> (affine sum or None, fix-up taken)"""
    _full, pieces = routine()
    m = base.miller_machine(0)
    for off, pt in ((0, jac(rng, a)), (PARTNER, jac(rng, b))):
        for i, c in enumerate(pt):
            for j, w in enumerate(base.limbs(c * R384 % P)):
                m.mem[base.ws_addr(i, j) + off] = w
    m.s[71] = PARTNER
    m.run(pieces["pro"]); m.run(pieces["tstart"]); m.run(pieces["add"])
    pr = lambda nm: m.s[("pair", int(nm[2:nm.index(":")]))]
    fix = bool(pr(t.M_H0) and pr(t.M_R0) and not pr(t.M_INF1) and not pr(t.M_INF2))
    if fix:
        m.run(pieces["fix"])
    m.run(pieces["epi"][:-1])
    w = [base.ws_get(m, i) for i in range(3)]
    assert all(x < P for x in w)                                       # canonical words: what the next level and the Miller kernels read
    X, Y, Z = [x * RI % P for x in w]
    return base.jac_affine(X, Y, Z), fix


def test_no_lane_private_memory():
    full, pieces = routine()
    assert not any("scratch" in l or "buffer_" in l or l.startswith("ds_") for l in full)
    assert all(v["lds"] == 0 for v in _R["st"].values())


def test_general_pairs_and_the_four_exceptional_cases():
    M = base._g2m()
    rng = random.Random(61)
    A = E.curve_point(rng); B = E.curve_point(rng)
    G = M.g1_mul(M.G1, rng.randrange(1, M.R)); H = M.g1_mul(M.G1, rng.randrange(1, M.R))
    cases = {"general": (A, B), "general in G1": (G, H), "mixed": (G, B), "equal": (A, A), "equal in G1": (G, G), "opposite": (A, M.g1_neg(A)),
             "acc_inf": (None, B), "addend_inf": (A, None), "both_inf": (None, None)}
    for case, (a, b) in cases.items():
        got, fix = tree_add(rng, a, b)
        assert got == M.g1_add(a, b), case
        assert fix == case.startswith("equal"), case


def test_torsion_points_on_both_sides():
    """points of order 3, 11 and the two 3-torsion points with x = 0 ((0, 2) and (0, p - 2): a zero coordinate in every product with X) as accumulator and as
    addend: against a G1 point, against themselves (the fix-up), against their negation (the two x = 0 points are each other's), against infinity"""
    M = base._g2m()
    rng = random.Random(62)
    tors = E.g1_torsion_points(rng, orders=(3, 11))
    x0 = [T for _ell, T, g in tors if g is None]
    assert sorted(x0) == [(0, 2), (0, P - 2)]
    G = M.g1_mul(M.G1, rng.randrange(1, M.R))
    fixes = 0
    for _ell, T, _g in tors:
        for a, b in ((T, G), (G, T), (T, T), (T, M.g1_neg(T)), (M.g1_neg(T), T), (T, None), (None, T), (M.g1_add(G, T), T), (T, M.g1_add(G, T)),
                     (M.g1_add(G, T), M.g1_add(G, T))):
            got, fix = tree_add(rng, a, b)
            assert got == M.g1_add(a, b), (T, a, b)
            assert fix == (a == b), (T, a, b)
            fixes += fix
    # 2 T = -T for the order-3 points: T + T and T + (-T) both ran, on the accumulator and on the addend side, for each x = 0 point
    assert fixes == 2 * len(tors)
    a, b = x0
    for p, q in ((a, b), (b, a)):
        assert tree_add(rng, p, q) == (None, False)
