"""Legal but adversarial inputs through every verify path of the C ABI (tests/edge_points.py makes them; tests/test_edge_points_cpu.py pins the oracle on
them against the Python model and counts which exceptional cases they drive): public keys OUTSIDE G1 -- the verifiers do not run KeyValidate, like the
reference's (src/signature.rs:27-40, src/aggregates.rs:130-170, 177-215, 261-316), and the 96-byte key format is the unchecked one --, some of which must
be ACCEPTED (a key pk + T with T of an order dividing the cofactor verifies what pk verifies); verify_multiple batches whose blinded points coincide (equal
or opposite partners in the sum tree, tables of an order-3 key built through the doubling fix-up, only SOME lanes of a wave in it); and blinding scalars
with extreme signed digits. Every expectation is the oracle's verdict on the same bytes and the same scalars (for large batches: the oracle's verdicts on
the chunks, whose products multiply)."""
import ctypes as C
import functools
import random

import pytest

import edge_points as E
import helpers
import orc

pytestmark = pytest.mark.gpu

ST_APK_INF = 0x08
SUM_INF = ("ell*T", "-T,T")


@pytest.fixture(scope="module")
def mb():
    from milagro_bls_amd import batch, _native
    _native.default_context()
    return batch


@pytest.fixture(scope="module")
def N():
    from milagro_bls_amd import _native
    _native.default_context()
    return _native


# ------------------------------------------------------------------------------------------------ 1. keys outside G1, item by item
@functools.lru_cache(maxsize=None)
def _fav(fmt):
    """the seeded items in key format fmt: (items, sigs, msgs, keys per item, key offsets, the oracle's verdicts)"""
    items = E.fav_items(E.FAV_SEED)
    wire = [E.class_wire(c, fmt) for c in items]
    wire96 = wire if fmt == 1 else [E.class_wire(c, 1) for c in items]
    want = [orc.fast_aggregate_verify(orc.g2_from_compressed(s)[1], m, ks) for s, m, ks in wire96]
    assert want == [c["expect"] for c in items]
    off = [0]
    for _, _, ks in wire:
        off.append(off[-1] + len(ks))
    return items, [w[0] for w in wire], [w[1] for w in wire], [w[2] for w in wire], off, want


def _check_status(items, got, st):
    for c, g, s in zip(items, got, st):
        if g:
            assert s == 0, (c["name"], c["ell"], hex(s))                    # an accepted item, inside G1 or not, carries no rejection bit
        else:
            assert s != 0, (c["name"], c["ell"])
        if c["name"] in SUM_INF:
            assert s & ST_APK_INF, (c["name"], c["ell"], hex(s))


@pytest.mark.usefixtures("engine")
@pytest.mark.parametrize("fmt", [0, 1])
def test_fast_aggregate_verify_with_keys_outside_g1_vs_oracle(mb, fmt):
    """~200 ragged items in seeded order: every class of key outside G1 for every prime order dividing the cofactor and the x = 0 points, on arbitrary lanes
    of a wave next to honest valid and rejected items"""
    items, sigs, msgs, keys, off, want = _fav(fmt)
    n = len(items)
    assert n >= 190 and sum(1 for c, w in zip(items, want) if c["ell"] and w) >= 40
    got, st = mb.fast_aggregate_verify_batch(b"".join(sigs), b"".join(msgs), b"".join(b"".join(k) for k in keys), n, pk_format=fmt, pk_offsets=off)
    assert got == want, [(i, items[i]["name"], items[i]["ell"], got[i]) for i in range(n) if got[i] != want[i]][:8]
    _check_status(items, got, st)


@functools.lru_cache(maxsize=None)
def _fixed_k(fmt, k=5):
    """items of exactly k keys (the uniform layout's key-sum kernels): torsion keys among honest ones, whose secret keys sign -> (kinds, sigs, msgs, pks, want)"""
    import bls12_381 as M
    rnd = random.Random(640 + k)
    nt = helpers.oracle_threads()
    kinds, sks, keys = [], [], []
    for _ell, T, _g in E.g1_torsion_points(rnd) + E.g1_torsion_points(rnd, orders=(3,), x0=False):
        nT, T3 = M.g1_neg(T), E.g1_torsion_points(rnd, orders=(3,), x0=False)[0][1]
        for kind in ("T,pk,T,T,T", "pk,T,pk,-T,pk", "T3,T3,T3,pk,pk", "T3,T3,T3,T,-T", "pk+T,pk,pk,pk,2T+pk", "curve,pk,pk,pk,pk", "honest", "honest wrong"):
            sk = [rnd.randrange(1, helpers.R) for _ in range(k)]
            pk = [E.g1_point(orc.sk_to_pk(x)) for x in sk]
            ks, signed = {
                "T,pk,T,T,T": ([T, pk[1], T, T, T], [1]), "pk,T,pk,-T,pk": ([pk[0], T, pk[2], nT, pk[4]], [0, 2, 4]),
                "T3,T3,T3,pk,pk": ([T3, T3, T3, pk[3], pk[4]], [3, 4]), "T3,T3,T3,T,-T": ([T3, T3, T3, T, nT], []),
                "pk+T,pk,pk,pk,2T+pk": ([M.g1_add(pk[0], T)] + pk[1:4] + [M.g1_add(M.g1_mul(T, 2), pk[4])], range(k)),
                "curve,pk,pk,pk,pk": ([E.curve_point(rnd)] + pk[1:], range(1, k)), "honest": (pk, range(k)), "honest wrong": (pk, range(1, k))}[kind]
            kinds.append(kind); keys.append(ks); sks.append(sum(sk[j] for j in signed) % helpers.R or 1)
    order = list(range(len(kinds)))
    rnd.shuffle(order)
    kinds, keys, sks = [kinds[i] for i in order], [keys[i] for i in order], [sks[i] for i in order]
    n = len(kinds)
    msgs = rnd.randbytes(32 * n)
    sigs = orc.batch_sign(b"".join(x.to_bytes(32, "big") for x in sks), msgs, n, nthreads=nt)
    pks = b"".join(E.g1_bytes(q, fmt) for ks in keys for q in ks)
    want = orc.batch_fast_aggregate_verify(sigs, msgs, pks, n, k, fmt, nthreads=nt)
    assert want == [kind not in ("T3,T3,T3,T,-T", "curve,pk,pk,pk,pk", "honest wrong") for kind in kinds]
    return kinds, sigs, msgs, pks, want


@pytest.mark.usefixtures("engine")
@pytest.mark.parametrize("fmt", [0, 1])
def test_uniform_key_count_with_torsion_keys_vs_oracle(mb, fmt):
    """the uniform layout (k = 5 keys per item, no offsets): torsion keys before, between and after honest ones, three equal keys of order 3 in a row (the
    running sum meets its own negative, then infinity), a sum at infinity, shifted keys, a random curve point, in seeded order"""
    kinds, sigs, msgs, pks, want = _fixed_k(fmt)
    n = len(kinds)
    got, st = mb.fast_aggregate_verify_batch(sigs, msgs, pks, n, 5, pk_format=fmt)
    assert got == want, [(i, kinds[i]) for i in range(n) if got[i] != want[i]]
    assert all((s == 0) == g for s, g in zip(st, got)) and all(st[i] & ST_APK_INF for i in range(n) if kinds[i] == "T3,T3,T3,T,-T")


@pytest.mark.usefixtures("engine")
@pytest.mark.parametrize("fmt", [0, 1])
def test_verify_batch_and_pre_aggregated_with_a_key_outside_g1_vs_oracle(mb, N, fmt):
    """Signature::verify on the one-key items (pk + T, 2 T + pk, T alone, a curve point, the infinite signature under T: accepted) and the same items through
    the fixed-k fast_aggregate_verify entry with k = 1; fast_aggregate_verify_pre_aggregated one call per item (96-byte keys)"""
    items, sigs, msgs, keys, off, want = _fav(fmt)
    sel = [i for i, c in enumerate(items) if len(c["keys"]) == 1]
    assert len(sel) >= 60
    S, Mg, K = b"".join(sigs[i] for i in sel), b"".join(msgs[i] for i in sel), b"".join(keys[i][0] for i in sel)
    w = [want[i] for i in sel]
    k96 = [_fav(1)[3][i][0] for i in sel]
    assert w == [orc.verify(orc.g2_from_compressed(sigs[i])[1], msgs[i], k) for i, k in zip(sel, k96)]
    got, st = mb.verify_batch(S, Mg, K, len(sel), pk_format=fmt)
    assert got == w, [(items[sel[j]]["name"], items[sel[j]]["ell"]) for j in range(len(sel)) if got[j] != w[j]]
    _check_status([items[i] for i in sel], got, st)
    got1, st1 = mb.fast_aggregate_verify_batch(S, Mg, K, len(sel), 1, pk_format=fmt)
    assert got1 == w
    _check_status([items[i] for i in sel], got1, st1)
    if fmt == 1:
        ctx = N.default_context()
        for i, k in zip(sel, k96):
            e, sig192 = orc.g2_from_compressed(sigs[i])
            assert want[i] == orc.fast_aggregate_verify_pre_aggregated(sig192, msgs[i], k)
            got_p = bool(N.lib().mbls_fast_aggregate_verify_pre_aggregated(ctx.handle, N.cbuf(sigs[i]), N.cbuf(msgs[i]), 32, N.cbuf(k)))
            assert got_p == want[i], (items[i]["name"], items[i]["ell"])


@pytest.mark.usefixtures("engine")
def test_aggregate_verify_batch_with_torsion_keys_on_some_pairs_vs_oracle(mb):
    """ragged items of 1 .. 6 (message, key) pairs; on some pairs the key is shifted by a torsion point (the item still verifies), is a pure torsion point (the
    pair contributes 1: the item verifies without that signer's share), or is a random curve point (the item fails)"""
    rnd = random.Random(808)
    torsion = E.g1_torsion_points(rnd)
    import bls12_381 as M
    n = 60
    S, allm, allp, off, want_by_construction, items = [], b"", b"", [0], [], []
    for i in range(n):
        k = rnd.randrange(1, 7)
        sks = [rnd.randrange(1, helpers.R) for _ in range(k)]
        ms = [rnd.randbytes(32) for _ in range(k)]
        keys = [E.g1_point(orc.sk_to_pk(s)) for s in sks]
        signed = list(range(k))
        ok = True
        kind = ("honest", "shift", "pure", "curve", "shift+pure")[i % 5]
        T = torsion[(i // 5) % len(torsion)][1]
        j = rnd.randrange(k)
        if kind in ("shift", "shift+pure"):
            keys[j] = M.g1_add(keys[j], T)
        if kind in ("pure", "shift+pure"):
            j2 = (j + 1) % k
            if j2 != j or kind == "pure":
                keys[j2] = M.g1_neg(T); signed.remove(j2)
        if kind == "curve":
            keys[j] = E.curve_point(rnd); ok = False
        agg = None
        for q in signed:
            sg = orc.sign(ms[q], sks[q])
            agg = sg if agg is None else orc.g2_add(agg, sg)
        sig = orc.g2_compress(agg) if agg is not None else helpers.G2_INF
        pk = [E.g1_bytes(q, 1) for q in keys]
        items.append((sig, ms, pk)); want_by_construction.append(ok)
        S.append(sig); allm += b"".join(ms); allp += b"".join(pk); off.append(off[-1] + k)
    want = [orc.aggregate_verify(orc.g2_from_compressed(sig)[1], ms, pk) for sig, ms, pk in items]
    assert want == want_by_construction and want.count(True) >= 40
    got, st = mb.aggregate_verify_batch(b"".join(S), allm, allp, n, pair_offsets=off)
    assert got == want, [i for i in range(n) if got[i] != want[i]]
    assert all((s == 0) == g for s, g in zip(st, got))


@pytest.mark.usefixtures("engine")
def test_key_table_takes_unchecked_keys_and_refuses_what_key_validate_refuses(mb, N):
    """the indexed entry over a table appended with validate=False: the same verdicts as the oracle on the same items; validate=True refuses exactly the keys
    the oracle's KeyValidate refuses (and an item cannot name them)"""
    items, sigs, msgs, keys, off, want = _fav(1)
    n = len(items)
    uniq = list(dict.fromkeys(k for ks in keys for k in ks))
    tab = N.KeyTable()
    try:
        first, errs = tab.append(b"".join(uniq), len(uniq), pk_format=1, validate=False)
        assert errs == [0] * len(uniq)
        at = {k: first + j for j, k in enumerate(uniq)}
        idx = [at[k] for ks in keys for k in ks]
        got, st = mb.fast_aggregate_verify_batch_indexed(tab, b"".join(sigs), b"".join(msgs), idx, n, offsets=off)
        assert got == want, [(i, items[i]["name"], items[i]["ell"]) for i in range(n) if got[i] != want[i]][:8]
        _check_status(items, got, st)
    finally:
        tab.close()
    for fmt in (0, 1):
        blobs = uniq if fmt == 1 else [orc.g1_compress(k) for k in uniq]
        tab = N.KeyTable()
        try:
            _, errs = tab.append(b"".join(blobs), len(uniq), pk_format=fmt, validate=True)
        finally:
            tab.close()
        valid = [orc.g1_key_validate(k) for k in uniq]
        assert [e == 0 for e in errs] == valid and valid.count(False) >= 32 and valid.count(True) >= 100


# ------------------------------------------------------------------------------------------------ 2. eight-lane partial key sums
@pytest.mark.parametrize("k", [32, 128])
def test_eight_lane_partial_key_sums_with_torsion_keys_vs_oracle(mb, N, k):
    """small batches cut an item's key sum into eight partial sums of k / 8 consecutive keys on lanes of their own (k_apk_combine adds them): items whose
    part 0 is pure torsion, whose part 3 sums to infinity (T, -T pairs), whose parts 1 and 2 are EQUAL (the combine doubles), whose parts 5 and 6 are
    opposite, and whose every part is pure torsion with total infinity -- byte keys and table indices against the oracle"""
    import bls12_381 as M
    N.default_context().reset_tuning()
    rnd = random.Random(1200 + k)
    per = k // 8
    torsion = E.g1_torsion_points(rnd, orders=(3, 11, 10177))
    n = 70
    pool = [rnd.randrange(1, helpers.R) for _ in range(k + 8)]
    pkb = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for s in pool), len(pool), 1, nthreads=helpers.oracle_threads())
    pk = [pkb[96 * j:96 * j + 96] for j in range(len(pool))]
    tb = lambda pt: E.g1_bytes(pt, 1)
    keys, sks, expect, kinds = [], [], [], []
    for i in range(n):
        idx = rnd.sample(range(len(pool)), k)
        ks = [pk[j] for j in idx]
        honest = [True] * k
        T = torsion[i % len(torsion)][1]
        kind = ("plain", "part0 torsion", "part3 infinity", "parts 1 = 2", "parts 5 = -6", "all torsion", "wrong")[i % 7 if i >= 7 else i]

        def put(j, key):
            ks[j] = key; honest[j] = False
        if kind == "part0 torsion":
            for j in range(per):
                put(j, tb(M.g1_mul(T, 1 + j % 2)))
        elif kind == "part3 infinity":
            for j in range(3 * per, 4 * per, 2):
                put(j, tb(T)); put(j + 1, tb(M.g1_neg(T)))
        elif kind == "parts 1 = 2":
            for j in range(per):
                ks[2 * per + j] = ks[per + j]; idx[2 * per + j] = idx[per + j]
        elif kind == "parts 5 = -6":
            for j in range(per):
                put(5 * per + j, orc.g1_mul(ks[6 * per + j], helpers.R - 1)); honest[6 * per + j] = False
        elif kind == "all torsion":
            for j in range(0, k, 2):
                put(j, tb(T)); put(j + 1, tb(M.g1_neg(T)))
        sk = sum(pool[idx[j]] for j in range(k) if honest[j]) % helpers.R
        if kind == "wrong":
            sk = sk % (helpers.R - 1) + 1
        keys.append(ks); sks.append(sk or 1); kinds.append(kind)
        expect.append(kind not in ("all torsion", "wrong"))
    msgs = [rnd.randbytes(32) for _ in range(n)]
    sg = orc.batch_sign(b"".join(s.to_bytes(32, "big") for s in sks), b"".join(msgs), n, nthreads=helpers.oracle_threads())
    pks = b"".join(b"".join(ks) for ks in keys)
    want = orc.batch_fast_aggregate_verify(sg, b"".join(msgs), pks, n, k, 1, nthreads=helpers.oracle_threads())
    assert want == expect, [(i, kinds[i]) for i in range(n) if want[i] != expect[i]]
    got, st = mb.fast_aggregate_verify_batch(sg, b"".join(msgs), pks, n, k, pk_format=1)
    assert got == want, [(i, kinds[i]) for i in range(n) if got[i] != want[i]]
    assert all((s == 0) == g for s, g in zip(st, got)) and all(st[i] & ST_APK_INF for i in range(n) if kinds[i] == "all torsion")
    uniq = list(dict.fromkeys(key for ks in keys for key in ks))
    tab = N.KeyTable()
    try:
        first, errs = tab.append(b"".join(uniq), len(uniq), pk_format=1, validate=False)
        assert errs == [0] * len(uniq)
        at = {key: first + j for j, key in enumerate(uniq)}
        got_i, st_i = mb.fast_aggregate_verify_batch_indexed(tab, sg, b"".join(msgs), [at[key] for ks in keys for key in ks], n, k)
    finally:
        tab.close()
    assert got_i == want, [(i, kinds[i]) for i in range(n) if got_i[i] != want[i]]
    assert all((s == 0) == g for s, g in zip(st_i, got_i))


# ------------------------------------------------------------------------------------------------ 3. verify_multiple: coincidences and edge scalars
def _vm_all_entries(N, mb, m2, batch, cuts_seed):
    """the batch through the one-call entry, the entry with the caller's scalar source (-> also the scalars it asked for), the device entry, shard records cut
    at seeded points and the two-context handle -> {entry: bool}, scalars asked for"""
    import torch
    lib = N.lib()
    ctx = N.default_context()
    dev = torch.device("cuda:0")
    sigs, apks, msgs, rands = batch
    n = len(sigs)
    Sb, Ab, Mb = b"".join(sigs), b"".join(apks), b"".join(msgs)
    S, A, Mg = N.cbuf(Sb), N.cbuf(Ab), N.cbuf(Mb)
    rr = (C.c_uint64 * n)(*rands)
    out = {"one call": bool(lib.mbls_verify_multiple_aggregate_signatures(ctx.handle, S, A, Mg, 32, None, rr, n))}
    asked = []

    def draw(_u, o, cnt):
        C.memmove(o, rr, 8 * cnt); asked.append(int(cnt))
    cb = N.SCALAR_SOURCE(draw)
    out["rng"] = bool(lib.mbls_verify_multiple_aggregate_signatures_rng(ctx.handle, S, A, Mg, 32, None, n, cb, None))
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    i64 = lambda rs: torch.tensor([r - (1 << 64) if r >> 63 else r for r in rs], dtype=torch.int64, device=dev)
    d_s, d_a, d_m, d_r = t(Sb), t(Ab), t(Mb), i64(rands)
    d_res = torch.full((8,), 7, dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_verify_multiple_aggregate_signatures_device(ctx.handle, d_s.data_ptr(), d_a.data_ptr(), d_m.data_ptr(), 32, None, d_r.data_ptr(), n,
                                                                   d_res.data_ptr(), None, None))
    torch.cuda.synchronize()
    assert int(d_res[0].item()) in (0, 1)
    out["device"] = bool(d_res[0].item())
    rnd = random.Random(cuts_seed)
    cuts = sorted([0, n] + [rnd.randrange(n + 1) for _ in range(rnd.randrange(1, 4))])
    recs = torch.zeros((len(cuts) - 1) * N.VM_PARTIAL_BYTES, dtype=torch.uint8, device=dev)
    for g in range(len(cuts) - 1):
        lo, hi = cuts[g], cuts[g + 1]
        mb.verify_multiple_partial_device(d_s.data_ptr() + 96 * lo, d_m.data_ptr() + 32 * lo, d_r.data_ptr() + 8 * lo, hi - lo,
                                          recs.data_ptr() + g * N.VM_PARTIAL_BYTES, d_apks=d_a.data_ptr() + 96 * lo)
    out["shards %s" % cuts] = mb.verify_multiple_finish_device(recs.data_ptr(), len(cuts) - 1)
    out["two contexts"] = mb.multi_verify_multiple_aggregate_signatures(m2, Sb, Ab, Mb, rands, n)
    return out, asked


@pytest.fixture
def m2(N, request):
    """two contexts on device 0, made after the `engine` fixture has set the environment they read their routing from"""
    if "engine" in request.fixturenames:
        request.getfixturevalue("engine")
    m = N.MultiContext([0, 0])
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _structured():
    """[(name, batch, the oracle's verdict)]: every structured batch and its spoiled twin"""
    out = []
    for name, b, spoil_at in E.vm_structured_batches():
        out.append((name, b, E.oracle_verify_multiple(b, chunk=1000)))
        out.append((name + ", set %d spoiled" % spoil_at, E.spoil(b, spoil_at), E.oracle_verify_multiple(E.spoil(b, spoil_at), chunk=1000)))
        assert out[-2][2] is True and out[-1][2] is False, name
    return out


@pytest.mark.usefixtures("engine")
def test_verify_multiple_structured_coincidences_and_edge_scalars_vs_oracle(N, mb, m2):
    """identical sets with one scalar (n = 2 .. 65: every addition of the sum tree has equal operands), set / negation alternating (opposite partners; a
    total of infinity with verdict True), every edge scalar (digits -8, 0, 7, the carry digit) on an honest set and on pure-torsion sets in the lanes next to
    it (keys of order 3 -- also (0, +-2) -- and 11: their G1 tables and windows run through equal / opposite operands and infinity while the neighbours
    take the general case), apk = pk + T with scalars that are and are not multiples of the order; each once more with one set spoiled -- five entries
    against the oracle with the same scalars"""
    for j, (name, b, want) in enumerate(_structured()):
        got, asked = _vm_all_entries(N, mb, m2, b, 300 + j)
        assert all(v == want for v in got.values()), (name, want, got)
        assert asked == [len(b[0])], (name, asked)


@functools.lru_cache(maxsize=None)
def _seeded(which):
    """(batch, the oracle's verdict, spoiled batch, the oracle's verdict) of the seeded coincidence batch number `which` (0: lane-pair signature chain,
    1: above it, trees on the wave engine, 2: first tree level one lane per sum)"""
    from milagro_bls_amd import _native as N
    n = E.vm_batch_sizes(N.default_limits().coop_max_items, E.coop_tree_pairs())[which]
    b, at = E.vm_seeded_batch(E.vm_pool(), n)
    nt = helpers.oracle_threads()
    bad = E.spoil(b, at)
    return b, E.oracle_verify_multiple(b, nt), bad, E.oracle_verify_multiple(bad, nt)


@pytest.mark.usefixtures("engine")
@pytest.mark.parametrize("which", [0, 1, 2])
def test_verify_multiple_seeded_coincidence_batches_vs_oracle(N, mb, m2, which):
    """thousands of sets drawn from two base sets, their negations, their torsion-shifted forms (one scalar per base) and pure-torsion sets: the sum tree
    meets equal partners (the doubling fix-up on SOME lanes of a wave), opposite partners and infinities on every early level -- on the lane-pair
    signature chain (k_blind_sig2_d), above it, and where the first level runs one lane per sum (k_g2_tree_d); tests/test_edge_points_cpu.py counts the
    cases. The oracle evaluates the batch in chunks with the same scalars."""
    L = N.default_limits()
    b, want, bad, want_bad = _seeded(which)
    n = len(b[0])
    assert (2 * n <= L.coop_max_items) == (which == 0) and (n - (n + 1) // 2 > E.coop_tree_pairs()) == (which == 2)
    assert want is True and want_bad is False
    for batch, w, seed in ((b, want, 50 + which), (bad, want_bad, 60 + which)):
        got, asked = _vm_all_entries(N, mb, m2, batch, seed)
        assert all(v == w for v in got.values()), (n, w, got)
        assert asked == [n]


# ------------------------------------------------------------------------------------------------ 4. aggregation entries with members outside the subgroups
@pytest.mark.parametrize("fmt", [0, 1])
def test_aggregate_public_keys_batch_with_torsion_members_vs_oracle(mb, fmt):
    """AggregatePublicKey::aggregate (src/aggregates.rs:29-39) over ell copies of T (infinity), ell + 1 copies (T), T and -T around honest keys, torsion
    points of different orders mixed with honest members"""
    import bls12_381 as M
    rnd = random.Random(1400)
    torsion = E.g1_torsion_points(rnd)
    honest = [E.g1_point(orc.sk_to_pk(rnd.randrange(1, helpers.R))) for _ in range(6)]
    sets = []
    for ell, T, _g in torsion:
        if ell <= 11:
            sets += [[T] * ell, [T] * (ell + 1), [T] * ell + [honest[0]], [honest[1]] + [T] * (ell - 1) + [honest[2], T]]
        sets += [[T, M.g1_neg(T)], [T, honest[0], M.g1_neg(T)], [honest[3], T, T], [T, torsion[0][1], honest[4], torsion[1][1]], [M.g1_mul(T, 2), T, honest[5]]]
    rnd.shuffle(sets)
    n = len(sets)
    off = [0]
    for s in sets:
        off.append(off[-1] + len(s))
    flat = b"".join(E.g1_bytes(q, fmt) for s in sets for q in s)
    out, st = mb.aggregate_public_keys_batch(flat, n, pk_format=fmt, pk_offsets=off)
    inf = 0
    for i, s in enumerate(sets):
        e, want = orc.aggregate_pks([E.g1_bytes(q, 1) for q in s])
        assert e == 0 and out[96 * i:96 * i + 96] == want, (i, len(s))
        assert want == M.g1_serialize_uncompressed(M.aggregate_pks(s))
        inf += want == E.G1_INF_U
    assert inf >= len(torsion) + 4


def test_aggregate_signatures_batch_with_members_outside_g2_vs_oracle(mb, vectors):
    """AggregateSignature::aggregate (src/aggregates.rs:100-106) does not test its members' subgroup: curve points of order 13, 23 and 2713 (made by the model
    from the golden file's curve points outside G2) -- ell copies (infinity), ell + 1 copies (the point), a point and its negative around honest signatures --
    and the golden points themselves, against the oracle's g2_add"""
    import bls12_381 as M
    rnd = random.Random(1500)
    probes = [bytes.fromhex(p["compressed"]) for p in vectors["model"]["g2_subgroup_probes"][:3]]
    honest = [orc.g2_compress(orc.sign(rnd.randbytes(32), rnd.randrange(1, helpers.R))) for _ in range(4)]
    sets = [[probes[0], honest[0], probes[1]], [probes[2], probes[2]], probes + honest]
    for ell, T in E.g2_torsion_points([E.g2_point(p) for p in probes]):
        c, neg = M.g2_compress(T), M.g2_compress(M.g2_neg(T))
        if ell <= 23:
            sets += [[c] * ell, [c] * (ell + 1), [honest[0]] + [c] * ell, [c] * (ell - 1) + [honest[1], c, honest[2]]]
        sets += [[c, neg], [c, honest[3], neg], [c, c, honest[0]], [honest[1], c]]
    n = len(sets)
    off = [0]
    for s in sets:
        off.append(off[-1] + len(s))
    out, errs = mb.aggregate_signatures_batch(b"".join(x for s in sets for x in s), n, offsets=off)
    assert errs == [0] * n
    inf = 0
    for i, s in enumerate(sets):
        acc = orc.g2_from_compressed(s[0])[1]
        for x in s[1:]:
            acc = orc.g2_add(acc, orc.g2_from_compressed(x)[1])
        assert out[96 * i:96 * i + 96] == orc.g2_compress(acc), (i, len(s))
        inf += out[96 * i:96 * i + 96] == helpers.G2_INF
    assert inf >= 5
