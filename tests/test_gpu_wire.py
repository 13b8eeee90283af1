"""Every case of tests/wire_cases.py through every route that reaches a decoder on the device (wire_cases.ROUTES). Where the decoded value comes back it is the
model's class and the model's bytes; where only the accept bit and the status word come back, the bit is the oracle's on the same bytes (cached per item: a
verdict does not depend on the route) and the status bits are the model's class. Every alias of a valid point stands beside its canonical twin: the twin is
accepted with status 0, the alias is rejected with the encoding bit -- a decoder that reduces instead of refusing flips that. verify_multiple answers once per
call, so its kernels see every case as a batch of one set (the device entry and the entry that draws its own scalars, on either side of the wave limit); the
one-call entries run on the aliases and their twins among honest sets. wire_cases.ROUTES names, per decode site, the tests here that reach it."""
import ctypes as C

import pytest

import bls12_381 as M

import orc
import wire_cases as W

pytestmark = pytest.mark.gpu

BAD_SIG, NOT_IN_G2, BAD_PK, APK_INF, PK_INF = 0x01, 0x02, 0x04, 0x08, 0x20
CS = W.cases()
_VERDICTS = {}


def dec_key(fmt, b):
    return orc.g1_from_compressed(b) if fmt == 0 else orc.g1_from_uncompressed(b)


def oracle_verdict(mode, it, extra=None):
    """the oracle's answer on the item's bytes: verify (one key), fav, aggregate_verify (extra = the messages), vm (extra = the scalar)"""
    key = (mode, it.sig, it.msg, tuple(it.keys), it.fmt, extra)
    if key not in _VERDICTS:
        es, sig = orc.g2_from_compressed(it.sig)
        ks = [dec_key(it.fmt, k) for k in it.keys]
        if es or any(e for e, _ in ks):
            v = False
        elif mode == "verify":
            v = orc.verify(sig, it.msg, ks[0][1])
        elif mode == "fav":
            v = orc.fast_aggregate_verify(sig, it.msg, [k for _, k in ks])
        elif mode == "aggregate_verify":
            v = orc.aggregate_verify(sig, list(extra), [k for _, k in ks])
        else:
            v = orc.verify_multiple([(sig, ks[0][1], it.msg)], [extra])
        _VERDICTS[key] = bool(v)
    return _VERDICTS[key]


_IN_G2 = {}


def in_g2(c):
    if c.data not in _IN_G2:
        _IN_G2[c.data] = c.ok and orc.g2_subgroup_check(W.uncompressed(W.G2C, c.point))
    return _IN_G2[c.data]


def check_status(items, res, st, mode, key_inf_bit, extras=None):
    """verdicts against the oracle, status bits against the model's class of the case, aliases against their twins"""
    for i, it in enumerate(items):
        c = it.case
        want = oracle_verdict(mode, it, None if extras is None else extras[i])
        assert res[i] == want, (c, it.twin, hex(st[i]))
        canonical_twin = it.twin is not None
        if c.fmt == W.G2C:
            ok, finite_outside = (True, False) if canonical_twin else (c.ok, c.cls == W.OK_FINITE and not in_g2(c))
            assert bool(st[i] & BAD_SIG) == (not ok) and bool(st[i] & NOT_IN_G2) == finite_outside and not st[i] & (BAD_PK | PK_INF), (c, hex(st[i]))
        else:
            ok, inf = (True, False) if canonical_twin else (c.ok, c.cls == W.OK_INF)
            assert bool(st[i] & BAD_PK) == (not ok) and not st[i] & (BAD_SIG | NOT_IN_G2), (c, hex(st[i]))
            if key_inf_bit:
                assert bool(st[i] & PK_INF) == (inf or not ok), (c, hex(st[i]))
        if canonical_twin:                                  # the honest item: accepted with a clean word; its alias: refused for its encoding
            assert res[i] and st[i] == 0, (c, hex(st[i]))
            assert not res[it.twin] and st[it.twin] & (BAD_SIG if c.fmt == W.G2C else BAD_PK), (c, hex(st[it.twin]))
    assert sum(it.twin is not None for it in items) >= 2


# ------------------------------------------------------------------------------------------------ routes that hand the decoded value back
@pytest.mark.parametrize("fmt", [W.G1C, W.G1U])
def test_pk_decode_batch(fmt):
    from milagro_bls_amd import batch
    cs = CS[fmt]
    blob = b"".join(c.data for c in cs)
    for validate in (False, True):
        out, errs = batch.pk_decode_batch(blob, len(cs), 0 if fmt == W.G1C else 1, validate=validate)
        for i, c in enumerate(cs):
            good = c.ok
            if validate:                                    # the verdict of the oracle's from_bytes (96-byte keys: its decoder, then its KeyValidate)
                e, pk = orc.pk_from_bytes(c.data) if fmt == W.G1C else orc.g1_from_uncompressed(c.data)
                good = e == 0 and orc.g1_key_validate(pk)
            want = (0, W.uncompressed(fmt, c.point)) if good else (c.err or W.ERR_INVALID_POINT, bytes(96))
            assert (errs[i], out[96 * i:96 * i + 96]) == want, (c, validate)


def test_pk_compress_batch_and_single_key_entries():
    from milagro_bls_amd import api, batch
    cs = CS[W.G1U]
    out, errs = batch.pk_compress_batch(b"".join(c.data for c in cs), len(cs))
    for i, c in enumerate(cs):
        assert (errs[i], out[48 * i:48 * i + 48]) == (c.err, M.g1_compress(c.point) if c.ok else bytes(48)), c
    g = api.PublicKey(M.g1_serialize_uncompressed(W.honest()[0][2]))
    for c in cs:                                            # k_g1_key_validate, k_g1_add: one item per call
        assert api.PublicKey(c.data).key_validate() == (c.cls == W.OK_FINITE and orc.g1_key_validate(W.uncompressed(W.G1U, c.point))), c
        a = api.AggregatePublicKey(c.data)
        if c.ok:
            a.add(g)
            assert a.point == M.g1_serialize_uncompressed(M.g1_add(c.point, W.honest()[0][2])), c
        else:
            with pytest.raises(api.AmclError) as e:
                a.add(g)
            assert e.value.code == c.err, c


@pytest.mark.parametrize("fmt", [W.G1C, W.G1U])
def test_keytable_append_and_export(fmt):
    from milagro_bls_amd import _native as N
    cs = CS[fmt]
    blob = b"".join(c.data for c in cs)
    for validate in (False, True):
        t = N.KeyTable()
        try:
            first, errs = t.append(blob, len(cs), 0 if fmt == W.G1C else 1, validate=validate)
            out, gerrs = t.get(first, len(cs))
            for i, c in enumerate(cs):
                good = c.ok and (not validate or (c.cls == W.OK_FINITE and orc.g1_key_validate(W.uncompressed(fmt, c.point))))
                assert errs[i] == (0 if good else c.err or W.ERR_INVALID_POINT), (c, validate)
                assert (gerrs[i], out[96 * i:96 * i + 96]) == ((0, W.uncompressed(fmt, c.point)) if good else (W.ERR_INVALID_POINT, bytes(96))), (c, validate)
        finally:
            t.close()


def _aggregate_rows(fmt, k):
    h = [s[2] for s in W.honest()]
    rows = []
    for i, c in enumerate(CS[fmt]):
        keys = [h[(i + t) % len(h)] for t in range(k - 1)]
        keys.insert(i % k, c)
        rows.append(keys)
    return rows


def _aggregate_expect(row):
    st, acc = 0, None
    for x in row:
        if isinstance(x, W.Case):
            st |= 0 if x.ok else BAD_PK | PK_INF
            st |= PK_INF if x.cls == W.OK_INF else 0
            acc = M.g1_add(acc, x.point if x.ok else None)
        else:
            acc = M.g1_add(acc, x)
    return st | (APK_INF if acc is None else 0), acc


@pytest.mark.parametrize("fmt", [W.G1C, W.G1U])
@pytest.mark.parametrize("shape", ["k=1", "k=3", "ragged"])
def test_aggregate_public_keys_batch(fmt, shape):
    """fmt 0: the compiled k_aggregate; fmt 1 (the staging buffer is aligned): the generated key sum with g1_decode_raw, k_aggregate_raw_d"""
    from milagro_bls_amd import batch
    rows = _aggregate_rows(fmt, 1 if shape == "k=1" else 3)
    if shape == "ragged":                                   # one to three keys, the case always among them
        cut = lambda i, r: (lambda L: r[min(i % 3, 3 - L):min(i % 3, 3 - L) + L])(1 + (i // 3) % 3)        # (the case sits at i % 3)
        rows = [cut(i, r) for i, r in enumerate(rows)]
        assert all(any(isinstance(x, W.Case) for x in r) for r in rows) and {len(r) for r in rows} == {1, 2, 3}
    blob = b"".join(x.data if isinstance(x, W.Case) else W.canonical(fmt, x) for r in rows for x in r)
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + len(r))
    kf = 0 if fmt == W.G1C else 1
    out, st = batch.aggregate_public_keys_batch(blob, len(rows), pk_format=kf, pk_offsets=offs) if shape == "ragged" else \
        batch.aggregate_public_keys_batch(blob, len(rows), k=len(rows[0]), pk_format=kf)
    for i, r in enumerate(rows):
        want_st, acc = _aggregate_expect(r)
        assert (st[i], out[96 * i:96 * i + 96]) == (want_st, M.g1_serialize_uncompressed(acc)), (CS[fmt][i], shape)


def test_sig_check_batch():
    from milagro_bls_amd import batch
    cs = CS[W.G2C]
    errs, g2 = batch.sig_check_batch(b"".join(c.data for c in cs), len(cs))
    for i, c in enumerate(cs):
        assert (errs[i], g2[i]) == (c.err, in_g2(c)), c


def test_aggregate_signatures_decode_then_encode():
    """k = 1: the canonical bytes of the model's point; k = 2 with an honest signature: the sum, which pins the root the decoder chose (y.c1 = 0 included) even
    against a sign rule that is wrong in decoder and encoder alike. k_g2_decode_affine; one item per call through k_g2_add"""
    from milagro_bls_amd import api, batch
    cs = CS[W.G2C]
    g = W.honest()[0][3]
    out, errs = batch.aggregate_signatures_batch(b"".join(c.data for c in cs), len(cs), k=1)
    for i, c in enumerate(cs):
        assert (errs[i], out[96 * i:96 * i + 96]) == (c.err, M.g2_compress(c.point) if c.ok else bytes(96)), c
    out, errs = batch.aggregate_signatures_batch(b"".join(c.data + M.g2_compress(g) for c in cs), len(cs), k=2)
    for i, c in enumerate(cs):
        assert (errs[i], out[96 * i:96 * i + 96]) == (c.err, M.g2_compress(M.g2_add(c.point, g)) if c.ok else bytes(96)), c
    for c in cs:
        a = api.AggregateSignature(c.data)
        if c.ok:
            a.add(api.Signature(M.g2_compress(g)))
            assert a.point == M.g2_compress(M.g2_add(c.point, g)), c
        else:
            with pytest.raises(api.AmclError) as e:
                a.add(api.Signature(M.g2_compress(g)))
            assert e.value.code == c.err, c


# ------------------------------------------------------------------------------------------------ routes that hand back the verdict and the status word
def _wire(items):
    return b"".join(it.sig for it in items), b"".join(it.msg for it in items), b"".join(b"".join(it.keys) for it in items)


@pytest.mark.parametrize("what", [W.G1C, W.G1U, W.G2C])
def test_verify_batch(engine, what):
    """k_sig (lanes) / k_sig2 (waves) on the signature; the key through k_aggregate (48 bytes) or the generated key sum (96 bytes)"""
    from milagro_bls_amd import batch
    items = W.sig_items() if what == W.G2C else W.key_items(what)
    sigs, msgs, pks = _wire(items)
    res, st = batch.verify_batch(sigs, msgs, pks, len(items), pk_format=items[0].fmt)
    check_status(items, res, st, "verify", key_inf_bit=True)


def _cancelling(count):
    """`count` >= 2 honest points whose sum is infinity: pairs (Q, -Q) and, for an odd count, one triple (A, B, -(A + B))"""
    h = [s[2] for s in W.honest()]
    out = [h[0], h[1], M.g1_neg(M.g1_add(h[0], h[1]))] if count % 2 else []
    for j in range((count - len(out)) // 2):
        out += [h[j % len(h)], M.g1_neg(h[j % len(h)])]
    assert len(out) == count and M.aggregate_pks(out) is None
    return out


@pytest.mark.parametrize("what,k", [(W.G1C, 3), (W.G1C, 32), (W.G1U, 3), (W.G1U, 32), (W.G2C, 3), (W.G2C, 32)])
def test_fast_aggregate_verify_batch(engine, what, k):
    """48-byte keys, uniform k > 1: k_pk_decompress + k_aggregate_decoded; 96-byte keys: k_aggregate_raw_d, and with k = 32 on the wave engine its eight-lane
    split (k >= 32, a multiple of 8, 96-byte keys in an aligned buffer, a pass on waves: pass_key_split in mbls_kernels.hip -- the plan is asserted).
    Signature cases: 48-byte keys for k = 3, 96-byte keys for k = 32"""
    from milagro_bls_amd import _native as N, batch
    if what == W.G2C:                                       # the signer's key and k - 1 keys that cancel
        items = W.sig_items(k=1, fmt=0 if k == 3 else 1)
        rest = [W.canonical(W.G1C if k == 3 else W.G1U, q) for q in _cancelling(k - 1)]
        for it in items:
            it.keys += rest
    else:
        items = W.key_items(what, k)
    if engine == "waves" and k == 32 and items[0].fmt == 1:
        _mode, passes = N.plan_batch(len(items), N.default_context().limits())
        assert all(p["pairing"] in (N.PAIRING_WAVE, N.PAIRING_WAVE_X2) for p in passes), passes
    sigs, msgs, pks = _wire(items)
    res, st = batch.fast_aggregate_verify_batch(sigs, msgs, pks, len(items), k=k, pk_format=items[0].fmt)
    check_status(items, res, st, "fav", key_inf_bit=True)


def test_fast_aggregate_verify_device_on_a_shifted_key_buffer():
    """96-byte keys at an address that is 1 mod 4: the compiled byte loads of g1_load_words96 and g1_decode_uncompressed_w (k_aggregate)"""
    import torch
    from milagro_bls_amd import _native as N
    items = W.key_items(W.G1U, 3)
    n = len(items)
    sigs, msgs, pks = _wire(items)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    d_s, d_m = dev(sigs), dev(msgs)
    d_p = torch.zeros(len(pks) + 32, dtype=torch.uint8, device="cuda")
    shift = 1 + (-d_p.data_ptr()) % 4                       # data_ptr() + shift = 1 mod 4
    d_p[shift:shift + len(pks)] = dev(pks)
    assert (d_p.data_ptr() + shift) % 4 == 1 and shift + len(pks) <= d_p.numel()
    d_r = torch.full((n,), 7, dtype=torch.uint8, device="cuda"); d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx = N.default_context()
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_device(ctx.handle, d_s.data_ptr(), d_m.data_ptr(), 32, None, d_p.data_ptr() + shift, 1, None, n, 3,
                                                              d_r.data_ptr(), None, d_st.data_ptr(), None))
    torch.cuda.synchronize()
    check_status(items, [bool(x) for x in d_r.cpu().tolist()], [x & 0xFFFFFFFF for x in d_st.cpu().tolist()], "fav", key_inf_bit=True)


@pytest.mark.parametrize("what", [W.G1U, W.G2C])
def test_aggregate_verify_batch(what):
    """three (message, key) pairs per item: the item's own message and key, then a second message under Q and under -Q, which cancel -- so the item's signature
    verifies exactly when it verifies its own pair. The keys go through the compiled k_blind_g1, the signatures through k_sig"""
    from milagro_bls_amd import batch
    q = W.honest()[3][2]
    items = W.sig_items(fmt=1) if what == W.G2C else W.key_items(W.G1U)
    msgs3 = []
    for it in items:
        m2 = bytes([it.msg[0] ^ 0xFF]) + it.msg[1:]
        it.keys += [W.canonical(W.G1U, q), W.canonical(W.G1U, M.g1_neg(q))]
        msgs3.append((it.msg, m2, m2))
    n = len(items)
    res, st = batch.aggregate_verify_batch(b"".join(it.sig for it in items), b"".join(b"".join(m) for m in msgs3), b"".join(b"".join(it.keys) for it in items), n, k=3)
    check_status(items, res, st, "aggregate_verify", key_inf_bit=False, extras=msgs3)


@pytest.mark.parametrize("side", ["lane pairs", "lanes"])
@pytest.mark.parametrize("what", [W.G1U, W.G2C])
def test_verify_multiple_batches_of_one_set(what, side):
    """one set per batch, so every case has a verdict and a status word of its own: the 96-byte key through k_blind_g1_d, the signature through
    k_blind_sig2_d (2 n within the wave limit) or k_blind_sig_d (the limit set to 0)"""
    import torch
    from milagro_bls_amd import _native as N, batch
    items = W.sig_items(fmt=1) if what == W.G2C else W.key_items(W.G1U)
    n = len(items)
    rands = [0x4000000000000001 + 2 * i for i in range(n)]
    ctx = N.default_context()
    assert 2 * n <= ctx.limits().coop_max_items
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    sigs, msgs, pks = _wire(items)
    d_s, d_m, d_p = dev(sigs), dev(msgs), dev(pks)
    d_r = torch.tensor(rands, dtype=torch.int64, device="cuda")
    d_res = torch.full((n,), 7, dtype=torch.uint8, device="cuda"); d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    try:
        if side == "lanes":
            ctx.set_coop_max_items(0)
        batch.verify_multiple_batches_device(d_s.data_ptr(), d_m.data_ptr(), d_r.data_ptr(), n, n, d_res.data_ptr(), d_status=d_st.data_ptr(), d_apks=d_p.data_ptr(),
                                             sets_per_batch=1, ctx=ctx)
        torch.cuda.synchronize()
    finally:
        ctx.reset_tuning()
    check_status(items, [bool(x) for x in d_res.cpu().tolist()], [x & 0xFFFFFFFF for x in d_st.cpu().tolist()], "vm", key_inf_bit=False, extras=rands)


@pytest.mark.parametrize("side", ["lane pairs", "lanes"])
@pytest.mark.parametrize("what", [W.G1U, W.G2C])
def test_verify_multiple_rng_entry_one_set_per_batch(what, side):
    """the entries that draw their own scalars decode and test the signatures first -- vm_rng_phase1: k_sig2 while 2 n is within the wave limit, k_sig above it (the
    limit set to 0) --, ask for the scalars of the sets whose signature passed, and run the blinded chains on the rest. mbls_verify_multiple_batches_locate_rng
    with one set per batch gives every case a verdict and a status word of its own"""
    from milagro_bls_amd import _native as N
    items = W.sig_items(fmt=1) if what == W.G2C else W.key_items(W.G1U)
    n = len(items)
    reached = []
    for it in items:                                        # the sets the reference's loop draws a scalar for: signature decodable and in G2 (infinity is)
        cls, pt = W.classify(W.G2C, it.sig)
        reached.append(cls == W.OK_INF or (cls == W.OK_FINITE and orc.g2_subgroup_check(W.uncompressed(W.G2C, pt))))
    scalar = lambda j: 0x4000000000000001 + 2 * j
    counts = []

    def source(_user, out, count):
        for j in range(count):
            out[j] = scalar(j)
        counts.append(int(count))
    cb = N.SCALAR_SOURCE(source)
    sigs, msgs, pks = _wire(items)
    res, sres, sst = N.outbuf(n), N.outbuf(n), (C.c_uint32 * n)()
    ctx = N.default_context()
    assert 2 * n <= ctx.limits().coop_max_items
    try:
        if side == "lanes":
            ctx.set_coop_max_items(0)
        ctx.check(N.lib().mbls_verify_multiple_batches_locate_rng(ctx.handle, N.cbuf(sigs), N.cbuf(pks), N.cbuf(msgs), 32, None, n, None, 1, n, res, sres, sst, cb, None))
    finally:
        ctx.reset_tuning()
    assert counts == [sum(reached)]
    rands, j = [], 0
    for r in reached:
        rands.append(scalar(j) if r else 1)
        j += r
    got = [bool(x) for x in bytes(res)[:n]]
    assert got == [bool(x) for x in bytes(sres)[:n]]        # one set per batch: the set's answer is the batch's
    check_status(items, got, list(sst)[:n], "vm", key_inf_bit=False, extras=rands)


def test_verify_multiple_entries_refuse_the_aliases():
    """the plain device entry and the entry that draws its own scalars (k_sig / k_sig2, then the blinded chains): honest sets are accepted with a clean word; the same
    sets with ONE key or signature replaced by an alias of itself are rejected with the encoding bit"""
    import random
    import torch
    from milagro_bls_amd import _native as N, api
    ctx = N.default_context()
    hs = W.honest()
    base = [(M.g2_compress(s[3]), M.g1_serialize_uncompressed(s[2]), s[1]) for s in hs]
    swaps = [(None, None, 0)]
    for c in CS[W.G1U]:
        if c.family == "alias":
            i = next(i for i, s in enumerate(hs) if s[2] == c.info["of"])
            swaps.append((i, (base[i][0], c.data, base[i][2]), BAD_PK))
    for c in CS[W.G2C]:
        if c.family == "alias":
            e, apk = orc.g1_from_uncompressed(orc.sk_to_pk(c.info["sk"]))
            swaps.append((0, (c.data, apk, c.info["msg"]), BAD_SIG))
            swaps.append((0, (c.canon, apk, c.info["msg"]), 0))
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    for at, repl, bit in swaps:
        sets = list(base)
        if repl:
            sets[at] = repl
        n = len(sets)
        d = [dev(b"".join(s[j] for s in sets)) for j in range(3)]
        d_r = torch.tensor([3 + 2 * i for i in range(n)], dtype=torch.int64, device="cuda")
        d_res = torch.full((8,), 7, dtype=torch.uint8, device="cuda"); d_st = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        ctx.check(N.lib().mbls_verify_multiple_aggregate_signatures_device(ctx.handle, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 32, None, d_r.data_ptr(), n,
                                                                           d_res.data_ptr(), d_st.data_ptr(), None))
        torch.cuda.synchronize()
        assert (int(d_res[0]), int(d_st[0]) & 0xFFFFFFFF) == ((1, 0) if not bit else (0, bit)), (at, bit)
        ok = api.AggregateSignature.verify_multiple_aggregate_signatures(random.Random(5), [(api.Signature(s[0]), api.PublicKey(s[1]), s[2]) for s in sets])
        assert ok == (not bit), (at, bit)
    assert len(swaps) >= 20
