"""The case generators of tests/edge_points.py, without a GPU: the oracle agrees with the Python model on every class of key outside G1 and on a verify_multiple
batch of coinciding sets (the GPU tests compare with the oracle: this pins the oracle on that class), and the inputs the GPU tests use really drive the
exceptional cases they are meant for -- counted by replaying the window and tree schedules on integers (conditions, not measurements)."""
import random
from collections import Counter

import bls12_381 as M

import edge_points as E
import helpers
import orc


def _model_sig(c):
    return None if c["sig_inf"] else E.g2_point(orc.g2_compress(orc.sign(c["msg"], c["sk"])))


def test_oracle_and_model_agree_on_keys_outside_g1():
    """one instance of every class for T of order 3, order 11 and (0, 2): fast_aggregate_verify on the key list; for one-key items also verify, the
    pre-aggregated form and aggregate_verify -- oracle == model == the expectation by construction"""
    rnd = random.Random(31337)
    torsion = [t for t in E.g1_torsion_points(rnd, orders=(3, 11)) if t[1] != (0, M.P - 2)]
    classes = E.outside_key_classes(rnd, torsion)
    assert {c["name"] for c in classes} >= {"pk+T", "pk,T", "T", "ell*T", "T,pk,T,T,T", "T,pk,-T", "-T,T", "2T+pk", "curve point", "inf sig,T", "inf sig,pk+T"}
    for c in classes:
        sig96, msg, keys = E.class_wire(c, 1)
        e, sig192 = orc.g2_from_compressed(sig96)
        assert e == 0
        for fmt in (0, 1):                                             # both encodings decode to the same point: (0, +-2) and every point compress normally
            for k, pt in zip(E.class_wire(c, fmt)[2], c["keys"]):
                e, dec = (orc.g1_from_compressed if fmt == 0 else orc.g1_from_uncompressed)(k)
                assert e == 0 and dec == M.g1_serialize_uncompressed(pt)
                assert (M.g1_decompress(k) if fmt == 0 else M.g1_deserialize_uncompressed(k)) == (0, pt)
        what = (c["name"], c["ell"])
        want = orc.fast_aggregate_verify(sig192, msg, keys)
        assert want == c["expect"], what
        sig = _model_sig(c)
        assert M.fast_aggregate_verify(sig, msg, c["keys"]) == want, what
        if len(keys) == 1:
            v = orc.verify(sig192, msg, keys[0])
            assert v == want and orc.fast_aggregate_verify_pre_aggregated(sig192, msg, keys[0]) == want, what
            assert orc.aggregate_verify(sig192, [msg], keys) == want, what
            if c["name"] in ("pk+T", "inf sig,T"):                     # (the model's verify / aggregate_verify are the same two-pairing product)
                assert M.verify(sig, msg, c["keys"][0]) == want and M.aggregate_verify(sig, [msg], c["keys"]) == want, what


def test_oracle_and_model_agree_on_a_coincidence_batch():
    """verify_multiple over a dozen sets of the coincidence pool (plain, negation, shifted key, pure torsion; one scalar per base), and the same with one set
    spoiled: oracle == model"""
    pool = E.vm_pool()
    assert {e["kind"] for e in pool.entries} == {"plain", "neg", "shift", "torsion"}
    rnd = random.Random(5)
    picks = pool.entries + [rnd.choice(pool.entries) for _ in range(12 - len(pool.entries))]
    rnd.shuffle(picks)
    batch = ([e["sig"] for e in picks], [e["apk"] for e in picks], [e["msg"] for e in picks], [e["r"] for e in picks])
    i = next(i for i, e in enumerate(picks) if e["kind"] == "shift")
    for b, want in ((batch, True), (E.spoil(batch, i), False)):
        assert E.oracle_verify_multiple(b) is want
        sets = [(E.g2_point(s), E.g1_point(a), m) for s, a, m in zip(*b[:3])]
        assert M.verify_multiple(sets, b[3]) is want


def test_chunked_oracle_equals_the_whole_batch():
    """the chunk algebra of oracle_verify_multiple on a batch small enough to evaluate whole"""
    pool = E.vm_pool()
    b, at = E.vm_seeded_batch(pool, 150)
    for bb in (b, E.spoil(b, at)):
        whole = E.oracle_verify_multiple(bb, chunk=1000)
        assert E.oracle_verify_multiple(bb, nthreads=helpers.oracle_threads(), chunk=32) == whole
    assert E.oracle_verify_multiple(b, chunk=1000) is True and whole is False


def test_edge_scalars_and_signed_digits():
    rs = E.edge_scalars()
    assert set(E.BLIND_EDGE_SCALARS) <= set(rs) and {3, 2, 4, 48, 11, 10, 12, 176} <= set(rs) and len(set(rs)) == len(rs)
    assert E.signed_digits(0x7777777777777778) == (1, [-8] * 16)                           # every digit -8, the carry digit 1
    assert E.signed_digits(0x7777777777777777) == (0, [7] * 16)
    assert E.signed_digits(0x8888888888888888) == (1, [-7] * 15 + [-8])
    carry, ds = E.signed_digits((1 << 64) - 1)
    assert carry == 1 and ds == [0] * 15 + [-1]
    assert all(-8 <= d <= 7 for r in rs for d in E.signed_digits(r)[1])


def test_window_census_conditions_of_the_gpu_inputs():
    """G1 blinding over the keys and scalars of the structured verify_multiple batches: every case class (general, equal operands, opposite operands,
    accumulator at infinity, addend at infinity / zero digit) is met at least 8 times in the table build AND in the window loop; a key of order 3 alone
    drives the doubling fix-up in both"""
    seen = {}
    for name, (sigs, apks, msgs, rands), _ in E.vm_structured_batches():
        if name.startswith(("edge scalars", "apk = pk + T")):
            for a, r in zip(apks, rands):
                seen.setdefault((a, r), 0)
                seen[(a, r)] += 1
    total = {"table": Counter(), "window": Counter()}
    order3 = {"table": Counter(), "window": Counter()}
    t3 = {M.g1_serialize_uncompressed((0, 2)), M.g1_serialize_uncompressed((0, M.P - 2))}
    for (a, r), cnt in seen.items():
        pt = None if a == E.G1_INF_U else E.g1_point(a)
        census, _ = E.window_case_census(pt, r)
        for part in total:
            for case, c in census[part].items():
                total[part][case] += c * cnt
                if a in t3:
                    order3[part][case] += c * cnt
    for part in ("table", "window"):
        assert all(total[part][case] >= 8 for case in E.CASES), (part, dict(total[part]))
        assert all(order3[part][case] >= 8 for case in ("equal", "opposite", "acc_inf")), (part, dict(order3[part]))


def test_tree_census_conditions_of_the_gpu_inputs():
    """the sum tree over the blinded signatures of the seeded coincidence batches (one call, one device: set i = item i): equal and opposite partners at
    least 8 times each on each of the first three levels of at least one batch, at least once on a level above MBLS_COOP_TREE_PAIRS pairs (k_g2_tree_d,
    one lane per sum) and once on a level below (program g2add, one wave per sum); the three sizes sit where their docstring says; a structured batch has
    the total sum at infinity and the oracle's verdict True"""
    from milagro_bls_amd import _native as N
    L = N.default_limits()
    pairs = E.coop_tree_pairs()
    small, mid, big = E.vm_batch_sizes(L.coop_max_items, pairs)
    pool = E.vm_pool()
    levels = {n: E.tree_case_census(E.blinded_signatures(*[E.vm_seeded_batch(pool, n)[0][i] for i in (0, 3)]))[0] for n in (small, mid, big)}
    assert any(all(c[case] >= 8 for _, c in lv[:3] for case in ("equal", "opposite")) for lv in levels.values())
    every = [pc for lv in levels.values() for pc in lv]
    for case in ("equal", "opposite"):
        assert any(p > pairs and c[case] >= 8 for p, c in every) and any(p <= pairs and c[case] >= 8 for p, c in every), case
    assert levels[big][0][0] > pairs and all(p <= pairs for lv in (levels[small], levels[mid]) for p, _ in lv)
    assert all(c[case] >= 8 for case in E.CASES for _, c in levels[big][:1])               # k_g2_tree_d: lanes of every case side by side in one launch
    inf_true = 0
    for name, b, spoil_at in E.vm_structured_batches():
        lv, tot = E.tree_case_census(E.blinded_signatures(b[0], b[3]))
        if tot is None and any(s != helpers.G2_INF for s in b[0]):
            assert E.oracle_verify_multiple(b) is True and E.oracle_verify_multiple(E.spoil(b, spoil_at)) is False, name
            inf_true += 1
        if name.startswith("identical"):
            assert lv[0][1]["equal"] == lv[0][0]
    assert inf_true >= 1


def test_class_balance_of_the_gpu_items():
    """of the fast_aggregate_verify items of the GPU test that carry a key outside G1, the oracle accepts at least a quarter and rejects at least a quarter"""
    items = [c for c in E.fav_items(E.FAV_SEED) if c["ell"]]
    verdicts = []
    for c in items:
        sig96, msg, keys = E.class_wire(c, 1)
        assert any(not orc.g1_key_validate(k) for k in keys), c["name"]
        verdicts.append(orc.fast_aggregate_verify(orc.g2_from_compressed(sig96)[1], msg, keys))
        assert verdicts[-1] == c["expect"], (c["name"], c["ell"])
    assert len(items) >= 60 and 4 * verdicts.count(True) >= len(items) and 4 * verdicts.count(False) >= len(items)
