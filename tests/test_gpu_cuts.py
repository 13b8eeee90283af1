"""GPU parity of the two instruction cuts of the headline path -- the key sum of 96-byte keys on the isomorphic curve (k_aggregate_raw_d) and
the fused Fp4 squaring inside the compressed cyclotomic squaring (k_final) -- at small n on the engine the headline number is measured on.
130 items (two full waves and a partial one), once with ragged key counts 1..3 from an offset table and once with 128 keys each, hold the
cases the key sum selects by mask: a repeated key (the doubling), a key equal to minus the running sum in the middle and as the LAST key
(MBLS_ST_APK_INFINITY), an infinite key, an undecodable key, an off-curve key, an order-3 torsion key, and an (infinite signature, torsion
key) item whose Miller value 1 goes through the squarings and the decompression. Results against the oracle; results, status words and bitmap
of the generated routine against the compiled lane body (which a key buffer that is not 4-byte aligned selects: an independent
implementation of the same sum)."""
import random

import pytest

import edge_points as E
import helpers
import orc

pytestmark = pytest.mark.gpu

N_ITEMS = 130
G1_INF_U = bytes([0x40]) + bytes(95)
UNDEC = bytes([0x20]) + bytes(95)                        # sign flag on an uncompressed key
OFFCURVE = bytes(48) + bytes([1]) + bytes(47)            # (0, 2^376): in range, not on the curve
BAD = (UNDEC, OFFCURVE)
ST_BAD_PK, ST_APK_INF, ST_NO_KEYS, ST_PK_INF, ST_PAIRING = 0x04, 0x08, 0x10, 0x20, 0x40


def neg_key(b96):
    y = int.from_bytes(b96[48:], "big")
    return b96[:48] + ((helpers.P - y) % helpers.P).to_bytes(48, "big")


class Sets:
    """items as (key bytes list, secret-key sum of the honest part, infinite signature?, spoil the message?) -> wire buffers + the oracle's verdicts"""

    def __init__(self, items, seed):
        rnd = random.Random(seed)
        self.n = len(items)
        self.keys = [it[0] for it in items]
        self.msgs = [rnd.randbytes(32) for _ in items]
        sks = b"".join(((it[1] % helpers.R) or 1).to_bytes(32, "big") for it in items)
        sg = orc.batch_sign(sks, b"".join(self.msgs), self.n, nthreads=8)
        self.sigs = [helpers.G2_INF if it[2] else sg[96 * i:96 * i + 96] for i, it in enumerate(items)]
        for i, it in enumerate(items):
            if it[3]:
                self.msgs[i] = bytes([self.msgs[i][0] ^ 1]) + self.msgs[i][1:]
        self.offsets = [0]
        for ks in self.keys:
            self.offsets.append(self.offsets[-1] + len(ks))
        self.flat = b"".join(b"".join(ks) for ks in self.keys)
        self.want = [orc.fast_aggregate_verify(orc.g2_from_compressed(s)[1], m, ks) for s, m, ks in zip(self.sigs, self.msgs, self.keys)]
        self.apk = []                                       # AggregatePublicKey::aggregate per set; an undecodable key is skipped and reported
        for ks in self.keys:
            good = [k for k in ks if k not in BAD]
            self.apk.append(orc.aggregate_pks(good)[1] if good else G1_INF_U)


@pytest.fixture(scope="module")
def material():
    rnd = random.Random(20261)
    sks = [rnd.randrange(1, helpers.R) for _ in range(160)]
    pkb = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for s in sks), len(sks), 1, nthreads=8)
    pk = [pkb[96 * j:96 * j + 96] for j in range(len(sks))]
    T = E.g1_bytes(E.g1_torsion_points(rnd, orders=(3,), x0=False)[0][1], 1)          # order 3: T + T = -T, 3 T = infinity
    T0 = E.g1_bytes((0, 2), 1)                                                           # the 3-torsion point with x = 0

    # ---- ragged sets of 1..3 keys
    k = lambda j: pk[j]
    special = [
        ([k(0), k(0)], 2 * sks[0], False, False),                   # repeated key: the doubling
        ([k(1), neg_key(k(1))], 1, False, False),                   # the LAST key is minus the running sum: the sum is infinity
        ([k(2), neg_key(k(2)), k(3)], sks[3], False, False),        # through infinity in the middle
        ([k(4), G1_INF_U], sks[4], False, False),                   # infinite key
        ([G1_INF_U], 1, False, False),
        ([G1_INF_U, k(5), k(6)], sks[5] + sks[6], False, False),
        ([UNDEC, k(7)], sks[7], False, False),                      # undecodable key
        ([k(8), OFFCURVE, k(9)], sks[8] + sks[9], False, False),    # off-curve key
        ([T], 1, True, False),                                      # (infinite signature, torsion key): both pairings are 1
        ([T0], 1, True, False),
        ([T, k(10)], sks[10], False, False),                        # the torsion part pairs to 1
        ([T, T, T], 1, False, False),                               # doubling, then T + T = -T meets T: infinity
        ([T, T], 1, True, False),                                   # 2 T = -T: still torsion
        ([k(11), k(11), k(11)], 3 * sks[11], False, False),
        ([k(12), k(13)], sks[12], False, False),                    # wrong signature
        ([k(14)], sks[14], True, False),                            # infinite signature, honest key
    ]
    items = []
    for i in range(N_ITEMS - len(special)):
        idx = [rnd.randrange(16, 160) for _ in range(1 + i % 3)]
        items.append(([k(j) for j in idx], sum(sks[j] for j in idx), False, i % 7 == 6))
    rnd.shuffle(items)
    for j, sp in enumerate(special):                                # spread over the three waves, the partial one included
        items.insert((j * 9 + 3) % len(items), sp)
    items[-1], items[5] = items[5], items[-1]
    ragged = Sets(items, 1)
    assert ragged.n == N_ITEMS and {len(x) for x in ragged.keys} == {1, 2, 3}

    # ---- sets of 128 keys
    K = 128
    items = []
    for i in range(N_ITEMS):
        idx = [rnd.randrange(0, 160) for _ in range(K)]
        ks, sk = [k(j) for j in idx], sum(sks[j] for j in idx)
        inf_sig = False
        if i == 5:                                                  # repeated key
            ks[17] = ks[16]; sk += sks[idx[16]] - sks[idx[17]]
        elif i == 70:                                               # key 40 is minus the sum of keys 0..39: through infinity in the middle
            ks[40] = neg_key(orc.aggregate_pks(ks[:40])[1]); sk -= sks[idx[40]] + sum(sks[j] for j in idx[:40])
        elif i == 129:                                              # the last key is minus the sum of the others
            ks[127] = neg_key(orc.aggregate_pks(ks[:127])[1]); sk = 1
        elif i == 64:                                               # infinite keys, first and in the middle
            ks[0] = ks[77] = G1_INF_U; sk -= sks[idx[0]] + sks[idx[77]]
        elif i == 3:
            ks[100] = UNDEC; sk -= sks[idx[100]]
        elif i == 100:
            ks[5] = OFFCURVE; sk -= sks[idx[5]]
        elif i == 128:                                              # a torsion key among honest ones
            ks[127] = T; sk -= sks[idx[127]]
        elif i == 66:                                               # 128 T = 2 T = -T: torsion, with the infinite signature
            ks = [T] * K; sk = 1; inf_sig = True
        elif i == 67:                                               # the same sum with an honest signature: rejected
            ks = [T] * K; sk = 1
        elif i == 2:                                                # 126 T = infinity
            ks = [T] * 126 + [G1_INF_U] * 2; sk = 1
        items.append((ks, sk, inf_sig, i % 9 == 8))
    wide = Sets(items, 2)
    return ragged, wide


def run_device(N, s, k, offsets, shift):
    """mbls_fast_aggregate_verify_batch_device on keys placed `shift` bytes into a device buffer -> (results, bitmap bits, status)"""
    import torch
    ctx = N.default_context(); dev = torch.device("cuda:0")
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_s, d_m = t(b"".join(s.sigs)), t(b"".join(s.msgs))
    buf = torch.zeros(len(s.flat) + 8, dtype=torch.uint8, device=dev)
    buf[shift:shift + len(s.flat)] = t(s.flat)
    d_off = torch.tensor(offsets, dtype=torch.int32, device=dev) if offsets is not None else None
    n = s.n
    d_res = torch.full((n,), 7, dtype=torch.uint8, device=dev); d_bm = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_device(ctx.handle, d_s.data_ptr(), d_m.data_ptr(), 32, None, buf.data_ptr() + shift, N.PK_UNCOMPRESSED,
                                                              d_off.data_ptr() if d_off is not None else None, n, k, d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
    torch.cuda.synchronize()
    return [bool(x) for x in d_res.cpu().tolist()], [bool(x) for x in helpers.bitmap_bits(d_bm, n)], [x & 0xFFFFFFFF for x in d_st.cpu().tolist()]


def check_sets(N, s, k, offsets):
    res, bits, st = run_device(N, s, k, offsets, 0)                  # the generated routine
    res_c, bits_c, st_c = run_device(N, s, k, offsets, 1)            # the compiled lane body
    assert res == s.want, [i for i in range(s.n) if res[i] != s.want[i]]
    assert bits == res and res_c == res and bits_c == res
    assert st == st_c, [(i, hex(st[i]), hex(st_c[i])) for i in range(s.n) if st[i] != st_c[i]]
    for i, ks in enumerate(s.keys):
        assert bool(st[i] & ST_BAD_PK) == any(x in BAD for x in ks), (i, hex(st[i]))
        assert bool(st[i] & ST_PK_INF) == any(x in BAD or x == G1_INF_U for x in ks), (i, hex(st[i]))
        assert bool(st[i] & ST_APK_INF) == (s.apk[i] == G1_INF_U), (i, hex(st[i]))
        assert not st[i] & ST_NO_KEYS
        if res[i]:
            assert st[i] & (ST_BAD_PK | ST_APK_INF | ST_PAIRING | 0x03) == 0, (i, hex(st[i]))
    return res, st


@pytest.fixture(scope="module")
def N():
    from milagro_bls_amd import _native
    _native.default_context()
    return _native


@pytest.mark.parametrize("engine", ["lanes2pair"], indirect=True)
def test_ragged_sets_of_one_to_three_keys(N, engine, material):
    ragged, _ = material
    res, st = check_sets(N, ragged, 0, ragged.offsets)
    assert sum(res) > N_ITEMS // 2 and not all(res)
    last_is_minus_sum = [i for i, ks in enumerate(ragged.keys) if len(ks) == 2 and ks[1] == neg_key(ks[0])]
    assert last_is_minus_sum and all(st[i] & ST_APK_INF and not res[i] for i in last_is_minus_sum)
    torsion_inf_sig = [i for i, (ks, sg) in enumerate(zip(ragged.keys, ragged.sigs)) if sg == helpers.G2_INF and ragged.want[i]]
    assert len(torsion_inf_sig) == 3 and all(res[i] for i in torsion_inf_sig)      # a Miller value of 1 is accepted


@pytest.mark.parametrize("engine", ["lanes2pair"], indirect=True)
def test_sets_of_128_keys(N, engine, material):
    _, wide = material
    res, st = check_sets(N, wide, 128, None)
    assert res[5] and res[70] and res[64] and res[128] and res[66] and not res[67]
    assert not res[129] and st[129] & ST_APK_INF and not res[2] and st[2] & ST_APK_INF
    assert not res[3] and not res[100]


@pytest.mark.parametrize("engine", ["lanes2pair"], indirect=True)
def test_aggregate_public_keys_bytes(engine, material):
    """mbls_aggregate_public_keys_batch over the same sets against the oracle, byte for byte"""
    from milagro_bls_amd import batch as mb
    for s, k, off in ((material[0], None, material[0].offsets), (material[1], 128, None)):
        apks, st = mb.aggregate_public_keys_batch(s.flat, s.n, k, pk_format=1, pk_offsets=off)
        for i in range(s.n):
            assert apks[96 * i:96 * i + 96] == s.apk[i], i
            assert bool(st[i] & ST_BAD_PK) == any(x in BAD for x in s.keys[i]), (i, hex(st[i]))


def test_eight_lane_key_split_over_the_new_routine():
    """24 items of 128 keys on the library's defaults: the wave engine cuts each key sum into eight partial sums on lanes of their own
    (k_aggregate_raw_d over 16 keys each) and k_apk_combine adds them"""
    from milagro_bls_amd import batch as mb
    b = helpers.make_batch(24, 128, fmt=1, seed=77, pool_n=160)
    got, _ = mb.fast_aggregate_verify_batch(b.sigs, b.msgs, b.pks, b.n, b.k, pk_format=1)
    want = orc.batch_fast_aggregate_verify(b.sigs, b.msgs, b.pks, b.n, b.k, 1, nthreads=8)
    assert got == want == b.expect
