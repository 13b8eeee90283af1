"""GPU parity tests proper: the HIP path, called through the C ABI of libmbls_hip.so, against the oracle on the same
seeded inputs, against the committed golden vectors, and -- at sizes the oracle cannot cover in seconds -- through
size-independent properties. Bit-exact: accept bits, status classes, serialized bytes, error codes."""
import ctypes as C
import random

import pytest

import helpers
import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mb():
    import milagro_bls_amd
    from milagro_bls_amd import batch, _native
    _native.default_context()          # raises if the HIP library or the GPU is missing: no fallback
    return batch


def test_native_library_is_loaded(mb):
    from milagro_bls_amd import _native
    assert _native.lib() is not None
    with open("/proc/self/maps") as f:
        assert "libmbls_hip.so" in f.read()


def test_fp_mul_sqr_parity(mb):
    rnd = random.Random(1)
    n = 4096
    A = [rnd.randrange(helpers.P) for _ in range(n)]; B = [rnd.randrange(helpers.P) for _ in range(n)]
    A[:4] = [0, 1, helpers.P - 1, helpers.P - 1]; B[:4] = [5, helpers.P - 1, helpers.P - 1, 2]
    a = b"".join(x.to_bytes(48, "big") for x in A); b = b"".join(x.to_bytes(48, "big") for x in B)
    o = mb.fp_mul_batch(a, b, n)
    assert all(int.from_bytes(o[48 * i:48 * i + 48], "big") == A[i] * B[i] % helpers.P for i in range(n))
    o = mb.fp_mul_batch(a, b, n, square=True)
    assert all(int.from_bytes(o[48 * i:48 * i + 48], "big") == A[i] * A[i] % helpers.P for i in range(n))
    # spot-check the oracle's own multiplier on the same inputs
    assert orc.fp_mul(a[:48 * 5][-48:], b[:48 * 5][-48:]) == o[:0] + mb.fp_mul_batch(a[48 * 4:48 * 5], b[48 * 4:48 * 5], 1)


def test_fp_mul_bulk_and_structured_operands(mb):
    """2^18 random pairs plus structured limb patterns (carry-chain corner cases of the hand-written multiplier)."""
    rnd = random.Random(123)
    P = helpers.P
    special = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2**380, 2**380 - 1, 2**352 - 1, 2**32 - 1, 2**32, 2**64 - 1, 2**96,
               int("ffffffff" * 11, 16), int("00000000ffffffff" * 5, 16), int("ffffffff00000000" * 5, 16) % P, int("80000000" * 11, 16),
               0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffff00000000 % P]
    pairs = [(a, b) for a in special for b in special]
    n = 1 << 18
    while len(pairs) < n:
        pairs.append((rnd.randrange(P), rnd.randrange(P)))
    a = b"".join(x.to_bytes(48, "big") for x, _ in pairs); b = b"".join(y.to_bytes(48, "big") for _, y in pairs)
    o = mb.fp_mul_batch(a, b, n)
    bad = [i for i in range(n) if int.from_bytes(o[48 * i:48 * i + 48], "big") != pairs[i][0] * pairs[i][1] % P]
    assert not bad, bad[:5]


def test_field_routines_structured_operands(mb):
    """The hand-written Fp2 product / square, paired product and the two exponentiation routines (28-bit digit core) on
    structured and random operands, against big-integer arithmetic."""
    rnd = random.Random(77)
    P = helpers.P
    special = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 2**380, 2**364, 2**364 - 1, 2**28 - 1, 2**28, 2**56 - 1, int("0fffffff" * 11, 16),
               int("ffffffff" * 11, 16), int("f0000000" * 11, 16) % P, 2**383 % P]
    vals = [(a, b) for a in special for b in special]
    while len(vals) < 2048:
        vals.append((rnd.randrange(P), rnd.randrange(P)))
    n = len(vals)
    a = b"".join(x.to_bytes(48, "big") for x, _ in vals); b = b"".join(y.to_bytes(48, "big") for _, y in vals)
    get = lambda o, i: int.from_bytes(o[48 * i:48 * i + 48], "big")
    o = mb.fp_mul_batch(a, b, n, op=2)
    for i in range(0, n, 2):
        (a0, b0), (a1, b1) = vals[i], vals[i + 1]
        assert (get(o, i), get(o, i + 1)) == ((a0 * b0 - a1 * b1) % P, (a0 * b1 + a1 * b0) % P), i
    o = mb.fp_mul_batch(a, b, n, op=3)
    for i in range(0, n, 2):
        a0, a1 = vals[i][0], vals[i + 1][0]
        assert (get(o, i), get(o, i + 1)) == ((a0 * a0 - a1 * a1) % P, 2 * a0 * a1 % P), i
    o = mb.fp_mul_batch(a, b, n, op=6)
    assert all(get(o, i) == vals[i][0] * vals[i][1] % P for i in range(n))
    m = 256                                   # the exponentiations are ~480 multiplications each
    o = mb.fp_mul_batch(a[:48 * m], b[:48 * m], m, op=4)
    assert all(get(o, i) == pow(vals[i][0], P - 2, P) for i in range(m))
    o = mb.fp_mul_batch(b[:48 * m], a[:48 * m], m, op=5)
    assert all(get(o, i) == pow(vals[i][1], (P - 3) // 4, P) for i in range(m))


@pytest.mark.usefixtures("engine")
def test_hash_to_g2_golden_and_oracle(mb, vectors):
    for v in vectors["model"]["hash_to_g2"]:
        m = helpers.expand_msg(v["msg"])
        assert mb.hash_to_g2_batch(m, 1, msg_len=len(m)).hex() == v["compressed"], v["msg"][:16]
    rnd = random.Random(2)
    msgs = rnd.randbytes(32 * 256)
    assert mb.hash_to_g2_batch(msgs, 256) == orc.batch_hash_to_g2(msgs, 256)


def test_sign_and_keys_external_vectors(mb, vectors):
    e = vectors["external"]["eth2_sign"]
    assert mb.sign_batch(bytes.fromhex(e["sk"]), bytes.fromhex(e["msg"]), 1).hex() == e["sig"]
    sks = b"".join(bytes.fromhex(kp["sk"]) for kp in vectors["external"]["eth2_sk_to_pk"])
    got = mb.sk_to_pk_batch(sks, 3)
    assert [got[48 * i:48 * i + 48].hex() for i in range(3)] == [kp["pk"] for kp in vectors["external"]["eth2_sk_to_pk"]]
    rnd = random.Random(3)
    n = 64
    sk = b"".join(rnd.randrange(1, helpers.R).to_bytes(32, "big") for _ in range(n)); msgs = rnd.randbytes(32 * n)
    assert mb.sign_batch(sk, msgs, n) == orc.batch_sign(sk, msgs, n, nthreads=8)
    assert mb.sk_to_pk_batch(sk, n, out_format=1) == orc.batch_sk_to_pk(sk, n, 1, nthreads=8)
    # scalars at the edges of the base-|x| split of the signing path and of the 64 x 16 generator table: small, sparse, powers of the
    # curve parameter, r - 1, and 32-byte values that are not below r (no SecretKey holds one; the product is [sk mod r] all the same)
    y = 0xd201000000010000
    edge = [1, 2, 15, 16, y - 1, y, y + 1, y * y, y ** 3, y ** 3 - 1, (y - 1) * (1 + y + y * y + y ** 3), helpers.R - 1, helpers.R - 2,
            0, helpers.R, helpers.R + 1, 2 ** 255 - 1, 2 ** 255, 2 ** 256 - 1, 0x1111111111111111111111111111111111111111111111111111111111111111,
            0xf0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0, 1 << 252, (1 << 128) - 1]
    n = len(edge)
    sk = b"".join(v.to_bytes(32, "big") for v in edge); msgs = rnd.randbytes(32 * n)
    assert mb.sign_batch(sk, msgs, n) == orc.batch_sign(sk, msgs, n, nthreads=8)
    assert mb.sk_to_pk_batch(sk, n, out_format=0) == orc.batch_sk_to_pk(sk, n, 0, nthreads=8)
    n = 3000                                                               # more than one wave per SIMD row, one lane per item in the message phase
    sk = b"".join(rnd.randrange(1, helpers.R).to_bytes(32, "big") for _ in range(n)); msgs = rnd.randbytes(32 * n)
    got = mb.sign_batch(sk, msgs, n)
    pick = rnd.sample(range(n), 48)
    assert b"".join(got[96 * i:96 * i + 96] for i in pick) == orc.batch_sign(b"".join(sk[32 * i:32 * i + 32] for i in pick), b"".join(msgs[32 * i:32 * i + 32] for i in pick), 48, nthreads=8)
    assert mb.sk_to_pk_batch(sk, n) == orc.batch_sk_to_pk(sk, n, 0, nthreads=8)


def test_secret_key_paths_constant_time_and_variable_time_forms(mb, vectors):
    """signing and sk -> pk look their tables up by scan + selection by default (include/mbls.h "SECRET KEYS ON THE DEVICE"; reference src/signature.rs:17-21,
    src/keys.rs:124-137: amcl selects in constant time); mbls_ctx_set_secret_ops(1) restores the key-dependent addresses. Same bytes either way, equal to the
    oracle's and to the Eth2 vectors -- edge scalars (zero / extreme window digits, the base-|x| split) included, across chunk boundaries of the staged selection."""
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    rnd = random.Random(17)
    y = 0xd201000000010000
    edge = [1, 2, 15, 16, y - 1, y, y + 1, y * y, y ** 3 - 1, helpers.R - 1, 0, helpers.R, 2 ** 256 - 1, 0x8888888888888888888888888888888888888888888888888888888888888888,
            0x0807060504030201080706050403020108070605040302010807060504030201, 0xf0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0]
    n = len(edge) + 200
    sk = b"".join(v.to_bytes(32, "big") for v in edge) + b"".join(rnd.randrange(1, helpers.R).to_bytes(32, "big") for _ in range(200))
    msgs = rnd.randbytes(32 * n)
    out = {}
    try:
        for vt in (False, True):
            ctx.set_secret_ops(vt)
            e = vectors["external"]["eth2_sign"]
            assert mb.sign_batch(bytes.fromhex(e["sk"]), bytes.fromhex(e["msg"]), 1).hex() == e["sig"]
            out[vt] = (mb.sign_batch(sk, msgs, n), mb.sk_to_pk_batch(sk, n, out_format=0), mb.sk_to_pk_batch(sk, n, out_format=1))
    finally:
        ctx.set_secret_ops(False)
    assert out[False] == out[True]
    assert out[False][0] == orc.batch_sign(sk, msgs, n, nthreads=8)
    assert out[False][1] == orc.batch_sk_to_pk(sk, n, 0, nthreads=8) and out[False][2] == orc.batch_sk_to_pk(sk, n, 1, nthreads=8)
    # more keys than one staged chunk of the constant-time sk -> pk (32 768 keys): the chunk boundary
    m = 33000
    skb = b"".join(((7919 * i + 1) % helpers.R).to_bytes(32, "big") for i in range(m))
    got = mb.sk_to_pk_batch(skb, m, out_format=0)
    pick = [0, 1, 32767, 32768, 32769, m - 1]
    assert b"".join(got[48 * i:48 * i + 48] for i in pick) == orc.batch_sk_to_pk(b"".join(skb[32 * i:32 * i + 32] for i in pick), len(pick), 0, nthreads=4)


def test_codec_parity(mb, vectors):
    ref = vectors["reference"]
    g1 = [bytes.fromhex(h) for h in ref["g1_compressed_round_trip"]["hex"]]
    out, errs = mb.pk_decode_batch(b"".join(g1), 3, validate=True)
    assert errs == [0, 0, 0] and [out[96 * i:96 * i + 96] for i in range(3)] == [orc.g1_from_compressed(b)[1] for b in g1]
    back, errs = mb.pk_compress_batch(out, 3)
    assert errs == [0, 0, 0] and back == b"".join(g1)                      # reference src/amcl_utils.rs:81-99
    g2 = [bytes.fromhex(h) for h in ref["g2_compressed_round_trip"]["hex"]]
    errs, in_g2 = mb.sig_check_batch(b"".join(g2), 3)
    assert errs == [0, 0, 0] and in_g2 == [True, True, True]
    probes = vectors["model"]["g2_subgroup_probes"]
    errs, in_g2 = mb.sig_check_batch(b"".join(bytes.fromhex(p["compressed"]) for p in probes), len(probes))
    assert errs == [0] * len(probes) and in_g2 == [p["in_g2"] for p in probes]
    p1 = vectors["model"]["g1_subgroup_probes"]
    out, errs = mb.pk_decode_batch(b"".join(bytes.fromhex(p["compressed"]) for p in p1), len(p1), validate=True)
    assert [e == 0 for e in errs] == [p["key_validate"] for p in p1]
    out, errs = mb.pk_decode_batch(b"".join(bytes.fromhex(p["compressed"]) for p in p1), len(p1), validate=False)
    assert errs == [0] * len(p1) and out == b"".join(bytes.fromhex(p["uncompressed"]) for p in p1)
    bad = [bytes.fromhex(h) for h in vectors["model"]["g1_bad_compressed"]]
    assert mb.pk_decode_batch(b"".join(bad), len(bad), validate=False)[1] == [3] * len(bad)
    # random garbage: identical error classes as the oracle (differential decode test, cf. reference fuzz/ targets)
    rnd = random.Random(4)
    blobs = [bytes([rnd.choice([0x80, 0xA0, 0xC0, 0x00, 0xE0, 0x9f]) | rnd.getrandbits(5)]) + rnd.randbytes(47) for _ in range(256)]
    out, errs = mb.pk_decode_batch(b"".join(blobs), 256, validate=False)
    for i, bl in enumerate(blobs):
        e, pt = orc.g1_from_compressed(bl)
        assert errs[i] == e and (e != 0 or out[96 * i:96 * i + 96] == pt)
    blobs2 = [bytes([rnd.choice([0x80, 0xA0, 0xC0, 0x00, 0xE0]) | rnd.getrandbits(5)]) + rnd.randbytes(95) for _ in range(128)]
    errs, in_g2 = mb.sig_check_batch(b"".join(blobs2), 128)
    for i, bl in enumerate(blobs2):
        e, pt = orc.g2_from_compressed(bl)
        assert errs[i] == e and (e != 0 or in_g2[i] == orc.g2_subgroup_check(pt))


def test_key_validate_outside_the_subgroup_vs_oracle(mb):
    """KeyValidate (reference src/keys.rs:176-185: subgroup_check_g1 = [r]P == O) on curve points outside G1: points of every prime order
    dividing the cofactor, G1 points shifted by them, random curve points -- the kernel decides by phi(P) == [-x^2]P, the oracle by [r]P."""
    import bls12_381 as M
    import edge_points as E
    rnd = random.Random(77)
    curve_point = lambda: E.curve_point(rnd)
    h = E.G1_COFACTOR                                                # (x - 1)^2 / 3, x = -X_ABS
    pts = []
    for ell, t, g in E.g1_torsion_points(rnd, per_order=2):          # two points of each prime order dividing h, then (0, 2) and (0, p - 2)
        pts += [t] if g is None else [t, M.g1_add(g, t), M.g1_add(M.g1_mul(t, 2), g)]
    pts += [curve_point() for _ in range(96)]
    pts += [M.g1_mul(M.G1, rnd.randrange(1, M.R)) for _ in range(24)]
    pts += [M.g1_mul(curve_point(), h) for _ in range(8)]            # cofactor-cleared: in G1
    blobs = [M.g1_compress(pt) for pt in pts]
    want = [orc.g1_key_validate(orc.g1_from_compressed(b)[1]) for b in blobs]
    assert sum(want) >= 32 and want.count(False) >= 96
    out, errs = mb.pk_decode_batch(b"".join(blobs), len(blobs), validate=True)
    assert [e == 0 for e in errs] == want
    from milagro_bls_amd import api
    for i in (0, 1, 2, 30, 31, len(pts) - 1, len(pts) - 9):          # PublicKey::key_validate, one key per call
        assert api.PublicKey(M.g1_serialize_uncompressed(pts[i])).key_validate() == want[i]


def test_signature_subgroup_verdict_out_of_the_miller_loop_vs_oracle(mb):
    """subgroup_check_g2 of the signature (reference src/signature.rs:29-31) on the one-lane-per-item path is decided from the Miller loop's
    own running point ([|x|] sig when the loop ends, lane_sig_verdict): curve points of every small prime order dividing the G2 cofactor
    (order 13 sends the loop's incomplete addition through T = -sig at the prefix 13 of |x|, and on through infinity), G2 points shifted
    by them, random curve points, and points of G2 that are no valid signature -- status bit 0x02 exactly where the oracle's [r]P says
    so, on both engines."""
    import bls12_381 as M
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    rnd = random.Random(91)
    h2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5

    def curve_point():
        while True:
            x = (rnd.randrange(M.P), rnd.randrange(M.P)); y = M.f2_sqrt(M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.B2))
            if y is not None:
                return (x, y if rnd.getrandbits(1) else M.f2_neg(y))
    assert M.g2_mul(curve_point(), h2 * M.R) is None
    g2pt = lambda: M.g2_mul(M.G2, rnd.randrange(1, M.R))
    pts = []
    for ell in (13, 23, 2713, 11953, 262069):
        for _ in range(2):
            t = None
            while t is None:
                t = M.g2_mul(curve_point(), h2 * M.R // (ell * ell if h2 % (ell * ell) == 0 else ell))
            assert M.g2_mul(t, ell) is None
            pts += [t, M.g2_add(g2pt(), t), M.g2_add(M.g2_mul(t, 5), g2pt()), M.g2_neg(t)]
    pts += [curve_point() for _ in range(40)]
    pts += [g2pt() for _ in range(16)] + [M.g2_mul(curve_point(), h2) for _ in range(6)]
    sigs = [M.g2_compress(pt) for pt in pts]
    n = len(sigs)
    want_in = [orc.g2_subgroup_check(orc.g2_from_compressed(b)[1]) for b in sigs]
    assert want_in.count(True) == 22 and want_in.count(False) == n - 22
    msgs = rnd.randbytes(32 * n)
    pk = orc.sk_to_pk(12345)
    want = orc.batch_verify(b"".join(sigs), msgs, orc.g1_compress(pk) * n, n, nthreads=8)
    assert not any(want)
    try:
        for lim, split in ((0, 0), (0, 1 << 20), (1 << 20, 0)):       # two-pair loop / the two pairs on two lanes / one wave per item
            ctx.set_coop_max_items(lim); ctx.set_lane_shaping(split, (1 << 64) - 1)
            got, st = mb.verify_batch(b"".join(sigs), msgs, pk * n, n, pk_format=1)
            assert got == want, (lim, split)
            assert [(x & 0x02) == 0 for x in st] == want_in, (lim, split)
    finally:
        ctx.reset_tuning()
    # a real signature next to them still verifies on the one-lane path, and the same signature shifted by a point of order 13 does not
    sk = 777; msg = b"m" * 32
    good = orc.g2_compress(orc.sign(msg, sk))
    shifted = M.g2_compress(M.g2_add(M.g2_decompress(good)[1], pts[0]))
    for split in (0, 1 << 20):
        try:
            ctx.set_coop_max_items(0); ctx.set_lane_shaping(split, (1 << 64) - 1)
            got, st = mb.verify_batch(good + shifted, msg * 2, orc.sk_to_pk(sk) * 2, 2, pk_format=1)
        finally:
            ctx.reset_tuning()
        assert got == [True, False] and st[0] == 0 and st[1] & 0x02


@pytest.mark.usefixtures("engine")
@pytest.mark.parametrize("fmt", [0, 1])
def test_fast_aggregate_verify_batch_vs_oracle(mb, fmt):
    b = helpers.make_batch(96, 8, fmt=fmt, seed=40 + fmt)
    got, st = mb.fast_aggregate_verify_batch(b.sigs, b.msgs, b.pks, b.n, b.k, pk_format=fmt)
    want = orc.batch_fast_aggregate_verify(b.sigs, b.msgs, b.pks, b.n, b.k, fmt, nthreads=8)
    assert got == want == b.expect
    flag = {"sig_not_in_g2": 0x02, "apk_infinity": 0x08, "bad_sig_bytes": 0x01, "bad_pk_bytes": 0x04, "flip_msg": 0x40, "wrong_key": 0x40}
    for kind, s in zip(b.kinds, st):
        if kind in flag:
            assert s & flag[kind], (kind, s)


@pytest.mark.usefixtures("engine")
def test_fast_aggregate_verify_128_keys_vs_oracle(mb):
    b = helpers.make_batch(192, 128, fmt=1, seed=50, pool_n=256)
    got, _ = mb.fast_aggregate_verify_batch(b.sigs, b.msgs, b.pks, b.n, b.k, pk_format=1)
    assert got == orc.batch_fast_aggregate_verify(b.sigs, b.msgs, b.pks, b.n, b.k, 1, nthreads=8) == b.expect
    b = helpers.make_batch(96, 128, fmt=0, seed=51, pool_n=256)
    got, _ = mb.fast_aggregate_verify_batch(b.sigs, b.msgs, b.pks, b.n, b.k, pk_format=0)
    assert got == orc.batch_fast_aggregate_verify(b.sigs, b.msgs, b.pks, b.n, b.k, 0, nthreads=8) == b.expect


@pytest.mark.usefixtures("engine")
def test_golden_batch_and_edge_cases(mb, vectors):
    fb = vectors["model"]["fast_aggregate_verify_batch"]
    items = fb["items"]
    sigs = b"".join(bytes.fromhex(i["sig"]) for i in items); msgs = b"".join(bytes.fromhex(i["msg"]) for i in items)
    for fmt, key in ((0, "pks_compressed"), (1, "pks_uncompressed")):
        pks = b"".join(bytes.fromhex(h) for i in items for h in i[key])
        assert mb.fast_aggregate_verify_batch(sigs, msgs, pks, len(items), fb["k"], pk_format=fmt)[0] == [i["result"] for i in items]
    # ragged key sets incl. an empty one (reference src/aggregates.rs:179-181, :384-389)
    b = helpers.make_batch(6, 3, fmt=0, seed=21, negatives=False)
    counts = [3, 3, 0, 3, 2, 3]
    pks = b"".join(b.pks[48 * 3 * i:48 * 3 * i + 48 * c] for i, c in enumerate(counts))
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    got, st = mb.fast_aggregate_verify_batch(b.sigs, b.msgs, pks, 6, pk_offsets=offs)
    assert got == [True, True, False, True, False, True] and st[2] & 0x10
    # empty batch
    assert mb.fast_aggregate_verify_batch(b"", b"", b"", 0, 3) == ([], [])
    # n not a multiple of the wave size, k = 1
    b = helpers.make_batch(67, 1, fmt=0, seed=22)
    assert mb.fast_aggregate_verify_batch(b.sigs, b.msgs, b.pks, b.n, b.k)[0] == b.expect


@pytest.mark.usefixtures("engine")
def test_verify_batch_vs_oracle(mb):
    b = helpers.make_batch(128, 1, fmt=0, seed=60)
    got, _ = mb.verify_batch(b.sigs, b.msgs, b.pks, b.n)
    assert got == orc.batch_verify(b.sigs, b.msgs, b.pks, b.n, nthreads=8)


def test_aggregate_public_keys_vs_oracle(mb):
    b = helpers.make_batch(32, 16, fmt=0, seed=70, negatives=False)
    apks, st = mb.aggregate_public_keys_batch(b.pks, b.n, b.k, pk_format=0)
    for i in range(b.n):
        keys = [orc.g1_from_compressed(b.pks[48 * (16 * i + j):48 * (16 * i + j + 1)])[1] for j in range(16)]
        assert apks[96 * i:96 * i + 96] == orc.aggregate_pks(keys)[1]


@pytest.mark.usefixtures("engine")
def test_differential_bit_flips_vs_oracle(mb):
    """Differential test in the spirit of the reference's fuzz targets (fuzz/fuzz_targets/*.rs): valid items with random
    single-bit flips anywhere in the signature, one key or the message; the accept bit must equal the oracle's for every item
    (most flips give undecodable or off-curve encodings, some give valid points outside the subgroup, a few stay valid)."""
    rnd = random.Random(2024)
    n, k = 384, 4
    for fmt in (0, 1):
        b = helpers.make_batch(n, k, fmt=fmt, seed=90 + fmt, negatives=False)
        sigs, msgs, pks = bytearray(b.sigs), bytearray(b.msgs), bytearray(b.pks)
        pkb = 48 if fmt == 0 else 96
        for i in range(n):
            what = rnd.randrange(4)
            if what == 0:
                sigs[96 * i + rnd.randrange(96)] ^= 1 << rnd.randrange(8)
            elif what == 1:
                pks[pkb * (k * i + rnd.randrange(k)) + rnd.randrange(pkb)] ^= 1 << rnd.randrange(8)
            elif what == 2:
                msgs[32 * i + rnd.randrange(32)] ^= 1 << rnd.randrange(8)
            # what == 3: left valid
        got, st = mb.fast_aggregate_verify_batch(bytes(sigs), bytes(msgs), bytes(pks), n, k, pk_format=fmt)
        want = orc.batch_fast_aggregate_verify(bytes(sigs), bytes(msgs), bytes(pks), n, k, fmt, nthreads=8)
        assert got == want
        assert 0 < sum(got) < n


def test_aggregation_with_repeated_inverse_and_infinite_keys(mb):
    # complete-addition semantics of AggregatePublicKey::aggregate (reference src/aggregates.rs:34-37, :74-75): the running sum meets
    # doubling (same key twice), inverse pairs (sum passes through infinity) and explicit infinity keys
    g = orc.sk_to_pk(1); g2 = orc.sk_to_pk(2); mg = orc.sk_to_pk(helpers.R - 1); inf = bytes([0x40]) + bytes(95); q = orc.sk_to_pk(0xABCDEF)
    sets = [[g, g, mg, g2, g2, g2], [g, mg, q, q, inf, q], [inf, inf, g, mg, inf, inf], [q, q, q, q, q, q], [mg, g, mg, g, g2, inf], [g2, g, g, inf, mg, mg]]
    for fmt in (1, 0):
        enc = (lambda p: p) if fmt == 1 else orc.g1_compress
        flat = b"".join(enc(p) for s_ in sets for p in s_)
        apks, st = mb.aggregate_public_keys_batch(flat, len(sets), 6, pk_format=fmt)
        for i, s_ in enumerate(sets):
            assert apks[96 * i:96 * i + 96] == orc.aggregate_pks(s_)[1], (fmt, i)
        assert st[2] & 0x08 and not st[0] & 0x08        # set 2 sums to infinity


def test_device_entry_point_bitmap_and_large_batch_properties(mb):
    """Config-2-sized property test (2^16 x Signature::verify): sign on the device, corrupt a known subset, check the
    accept bitmap by construction, and pin a seeded sample of 1 000+ items over the whole batch against the oracle."""
    import torch
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    dev = torch.device("cuda:0")
    n = 1 << 16
    g = torch.Generator(device="cpu"); g.manual_seed(0x6d626c73)
    sks = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g); sks[:, 0] &= 0x3F; sks[:, 31] |= 1   # nonzero, < r
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    d_sk, d_msg = sks.to(dev), msgs.to(dev)
    d_sig = torch.empty((n, 96), dtype=torch.uint8, device=dev); d_pk = torch.empty((n, 48), dtype=torch.uint8, device=dev)
    ctx.check(N.lib().mbls_sign_batch_device(ctx.handle, d_sk.data_ptr(), d_msg.data_ptr(), 32, n, d_sig.data_ptr(), None))
    ctx.check(N.lib().mbls_sk_to_pk_batch_device(ctx.handle, d_sk.data_ptr(), 0, n, d_pk.data_ptr(), None))
    bad = torch.arange(7, n, 16, device=dev)
    d_msg[bad, 0] ^= 1
    d_res = torch.full((n,), 7, dtype=torch.uint8, device=dev); d_bm = torch.full((n // 64,), -1, dtype=torch.int64, device=dev)
    ctx.check(N.lib().mbls_verify_batch_device(ctx.handle, d_sig.data_ptr(), d_msg.data_ptr(), 32, None, d_pk.data_ptr(), 0, n,
                                               d_res.data_ptr(), d_bm.data_ptr(), None, None))
    torch.cuda.synchronize()
    res = d_res.cpu()
    expect = torch.ones(n, dtype=torch.uint8); expect[7::16] = 0
    assert torch.equal(res, expect)
    assert (helpers.bitmap_bits(d_bm, n) == expect.numpy()).all()          # all 1 024 bitmap words
    # the oracle on the first wave and a seeded sample over the whole batch (round seam, tail, corrupted items)
    sel = sorted(set(helpers.sample_indices(n, seed=0x6d62)) | set(range(64)))
    helpers.oracle_check_verify(d_sig, d_msg, d_pk, sel, expect, res)
