"""GPU tests of mbls_verify_multiple_batches_locate* (include/mbls.h, "WHICH SETS OF A REJECTED BATCH"): the per-batch outputs against
mbls_verify_multiple_batches_device, the per-set outputs of rejected batches against that entry over one-set batches with the same scalars and against the
oracle, every route, the placement of a bad set inside the trees, the sets a passing batch hides, device-side table faults, the reference's RNG order and the
argument handling. The mix is built as tests/test_gpu_vm_batches.py builds its own."""
import ctypes as C
import random

import numpy as np
import pytest

import helpers
import orc

pytestmark = pytest.mark.gpu

G1_INF_U = bytes([0x40]) + bytes(95)
ST_BAD_PK = 0x04
ST_PAIRING_FAILED = 0x40
REJECT_BATCH = 0x01 | 0x02 | 0x04 | 0x100 | 0x80          # mbls_coop.h COOP_REJECT_BATCH

SIZES_32 = [0, 1, 2, 3, 10, 64, 5, 1, 2, 3, 10, 64, 7, 0, 9, 1, 2, 3, 10, 33, 17, 0, 12, 6]
SIZES_RAGGED = [64, 3, 0, 10, 2, 1, 13, 64, 1, 2, 3, 10, 0, 8, 21, 4, 3, 10, 2, 1, 11, 19, 5, 0]
DEFECTS = ("wrong_key", "swapped_sig", "inf_sig", "inf_key", "both_inf", "not_in_g2", "undecodable", "zero_scalar")


@pytest.fixture(scope="module")
def N():
    from milagro_bls_amd import _native
    _native.default_context()
    return _native


def _dev(b, dtype=np.uint8):
    import torch
    a = np.frombuffer(bytes(b), dtype=dtype).copy() if not isinstance(b, np.ndarray) else b
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


class Mix:
    """host-side sets: sigs (96 B), apks (96 B), wire (two 96 B keys per set), msgs, rands; off = the batch table"""

    def __init__(self, sigs, apks, wire, msgs, rands, off):
        self.sigs, self.apks, self.wire, self.msgs, self.rands, self.off = list(sigs), list(apks), [list(w) for w in wire], list(msgs), list(rands), list(off)
        self.n, self.B = len(self.sigs), len(off) - 1
        self.moff = _offsets([len(x) for x in self.msgs])
        self.ragged = any(len(x) != 32 for x in self.msgs)                      # (fixed 32-byte messages go without an offset table)

    def pick(self, sets):
        """the one-set batches over `sets`, same scalars"""
        return Mix([self.sigs[i] for i in sets], [self.apks[i] for i in sets], [self.wire[i] for i in sets], [self.msgs[i] for i in sets],
                   [self.rands[i] for i in sets], list(range(len(sets) + 1)))


def _build_mix(seed, sizes, ragged, probe):
    """every set has two keys: sig = [sk1 + sk2] H(msg), apk = pk1 + pk2 = the wire keys (pk1, pk2). A third of the non-empty batches carry one defect each."""
    rnd = random.Random(seed)
    off = _offsets(sizes)
    n = off[-1]
    sks = [(rnd.randrange(1, helpers.R), rnd.randrange(1, helpers.R)) for _ in range(n)]
    flat = b"".join(s.to_bytes(32, "big") for pair in sks for s in pair)
    pk96 = orc.batch_sk_to_pk(flat, 2 * n, 1, nthreads=8)
    wire = [[pk96[192 * i:192 * i + 96], pk96[192 * i + 96:192 * i + 192]] for i in range(n)]
    apks = [orc.g1_add(w[0], w[1]) for w in wire]
    msgs = [rnd.randbytes(rnd.choice([0, 1, 31, 32, 33, 55, 56, 64, 65, 100, 200]) if ragged else 32) for _ in range(n)]
    sigs = [orc.g2_compress(orc.sign(mm, (a + b) % helpers.R)) for mm, (a, b) in zip(msgs, sks)]
    rands = [rnd.randrange(1, 1 << 63) for _ in range(n)]
    spare_wire = [orc.sk_to_pk(111), orc.sk_to_pk(222)]
    spare_apk, spare_sig = orc.g1_add(*spare_wire), orc.g2_compress(orc.sign(b"spare", 999))
    nonempty = [b for b, s in enumerate(sizes) if s]
    bad = sorted(rnd.sample(nonempty, (len(sizes) + 2) // 3))
    defect = {}
    for t, b in enumerate(bad):
        d = DEFECTS[t % len(DEFECTS)]
        lo, hi = off[b], off[b + 1]
        i = rnd.randrange(lo, hi)
        other = (i + 1 - lo) % (hi - lo) + lo if hi - lo > 1 else None
        if d == "wrong_key":
            apks[i], wire[i] = (apks[other], list(wire[other])) if other is not None else (spare_apk, list(spare_wire))
        elif d == "swapped_sig":
            sigs[i] = sigs[other] if other is not None else spare_sig
        elif d == "inf_sig":
            sigs[i] = helpers.G2_INF
        elif d == "inf_key":
            apks[i] = G1_INF_U; wire[i] = [wire[i][0], orc.g1_mul(wire[i][0], helpers.R - 1)]
        elif d == "both_inf":
            sigs[i] = helpers.G2_INF; apks[i] = G1_INF_U; wire[i] = [wire[i][0], orc.g1_mul(wire[i][0], helpers.R - 1)]
        elif d == "not_in_g2":
            sigs[i] = probe
        elif d == "undecodable":
            sigs[i] = bytes([sigs[i][0] & 0x7F]) + sigs[i][1:]
        elif d == "zero_scalar":
            rands[i] = 0
        defect[b] = (d, i)
    m = Mix(sigs, apks, wire, msgs, rands, off)
    m.sizes, m.defect = sizes, defect
    assert m.ragged == ragged
    return m


@pytest.fixture(scope="module")
def mixes(vectors):
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    return [_build_mix(2026, SIZES_32, False, probe), _build_mix(2027, SIZES_RAGGED, True, probe)]


class DevMix:
    """a Mix resident on the device in every key form"""

    def __init__(self, N, m, table=False):
        self.sigs = _dev(b"".join(m.sigs)); self.apks = _dev(b"".join(m.apks)); self.wire = _dev(b"".join(k for w in m.wire for k in w))
        self.msgs = _dev(b"".join(m.msgs)); self.rands = _dev(np.array(m.rands, dtype=np.uint64))
        self.moff = _dev(np.array(m.moff, dtype=np.uint64)) if m.ragged else None
        self.msg_len = 0 if m.ragged else 32
        self.boff = _dev(np.array(m.off, dtype=np.uint32))
        self.tab = self.idx = None
        if table:
            self.tab = N.KeyTable()
            first, errs = self.tab.append(b"".join(k for w in m.wire for k in w), 2 * m.n, pk_format=N.PK_UNCOMPRESSED, validate=False)
            assert not any(errs)
            self.idx = _dev(np.arange(first, first + 2 * m.n, dtype=np.uint32))


FORMS = ("apk", "wire", "indexed")


def _call(N, m, d, form, locate, boff=None, n_batches=None, spb=0):
    """the batches entry (locate = False) or the locate entry over the whole of m -> (results, status[, set results, set status]) as lists"""
    import torch
    B = m.B if n_batches is None else n_batches
    res = torch.full((max(1, B),), 7, dtype=torch.uint8, device="cuda:0"); st = torch.full((max(1, B),), -1, dtype=torch.int32, device="cuda:0")
    sres = torch.full((max(1, m.n),), 7, dtype=torch.uint8, device="cuda:0"); sst = torch.full((max(1, m.n),), -1, dtype=torch.int32, device="cuda:0")
    ctx = N.default_context()
    boff = None if spb else (d.boff.data_ptr() if boff is None else boff.data_ptr())
    tail = (res.data_ptr(), st.data_ptr()) + ((sres.data_ptr(), sst.data_ptr()) if locate else ()) + (None,)
    common = (d.msgs.data_ptr(), d.msg_len, None if d.moff is None else d.moff.data_ptr(), d.rands.data_ptr(), m.n, boff, spb, B)
    L = N.lib()
    if form == "indexed":
        f = L.mbls_verify_multiple_batches_locate_indexed_device if locate else L.mbls_verify_multiple_batches_indexed_device
        rc = f(ctx.handle, d.tab.handle, d.sigs.data_ptr(), d.idx.data_ptr(), None, 2, *common, *tail)
    else:
        f = L.mbls_verify_multiple_batches_locate_device if locate else L.mbls_verify_multiple_batches_device
        wire = form == "wire"
        rc = f(ctx.handle, d.sigs.data_ptr(), None if wire else d.apks.data_ptr(), d.wire.data_ptr() if wire else None, N.PK_UNCOMPRESSED, None, 2, *common, *tail)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    out = ([int(x) for x in res.cpu().numpy()[:B]], [int(x) & 0xFFFFFFFF for x in st.cpu().numpy()[:B]])
    if locate:
        out += ([int(x) for x in sres.cpu().numpy()[:m.n]], [int(x) & 0xFFFFFFFF for x in sst.cpu().numpy()[:m.n]])
    return out


def _one_set_batches(N, m, sets, form):
    """mbls_verify_multiple_batches[_indexed]_device with sets_per_batch = 1 over exactly `sets`, same scalars -> (results, status) per set"""
    if not sets:
        return [], []
    s = m.pick(sets)
    return _call(N, s, DevMix(N, s, table=form == "indexed"), form, False, spb=1)


def _check_against_existing(N, m, form, d=None):
    """contract items 1 - 4 for one mix and key form; returns the locate call's outputs and the examined sets"""
    d = d or DevMix(N, m, table=form == "indexed")
    res0, st0 = _call(N, m, d, form, False)
    res, st, sres, sst = _call(N, m, d, form, True)
    assert (res, st) == (res0, st0), form                                          # item 1
    rejected = [i for b in range(m.B) if not res[b] for i in range(m.off[b], m.off[b + 1])]
    for b in range(m.B):
        if res[b]:
            for i in range(m.off[b], m.off[b + 1]):
                assert sres[i] == 1 and not sst[i] & (ST_PAIRING_FAILED | REJECT_BATCH), (form, b, i, hex(sst[i]))      # item 2
    r1, s1 = _one_set_batches(N, m, rejected, form)
    assert [sres[i] for i in rejected] == r1, (form, [(i, sres[i], r) for i, r in zip(rejected, r1) if sres[i] != r])     # item 3
    assert [sst[i] for i in rejected] == s1, (form, [(i, hex(sst[i]), hex(s)) for i, s in zip(rejected, s1) if sst[i] != s])   # item 4
    for i in rejected:
        assert bool(sst[i] & ST_PAIRING_FAILED) == (not sst[i] & REJECT_BATCH and not sres[i]), (form, i, hex(sst[i]))
    examined = [i for i in rejected if not sst[i] & REJECT_BATCH]
    return (res, st, sres, sst), examined


# ------------------------------------------------------------------------------------------------ test 1: the mix against the existing entry
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", [0, 1], ids=["msg32", "ragged"])
def test_mix_against_the_batches_entry(N, mixes, which, form):
    """per batch byte-equal to mbls_verify_multiple_batches_device; per set of a rejected batch byte-equal (result and status word) to that entry over the
    one-set batches; every set of an accepted batch 1. Every defect is present; the bad set of a rejected batch is the one that reads 0."""
    m = mixes[which]
    assert {d for d, _ in m.defect.values()} == set(DEFECTS)
    (res, st, sres, sst), examined = _check_against_existing(N, m, form)
    assert res.count(0) >= 6 and res.count(1) >= 12 and len(examined) >= 20
    for b, (kind, i) in m.defect.items():
        lo, hi = m.off[b], m.off[b + 1]
        if kind == "both_inf":
            assert res[b] == 1 and sres[lo:hi] == [1] * (hi - lo)
            continue
        assert res[b] == 0 and sres[i] == 0, (b, kind)
        others = [j for j in range(lo, hi) if j != i]
        assert all(sres[j] == 1 for j in others), (b, kind, [j for j in others if sres[j] != 1])        # (a set whose key or signature was COPIED stays good)
        if kind in ("wrong_key", "swapped_sig", "inf_sig", "inf_key"):
            assert sst[i] & ST_PAIRING_FAILED and not sst[i] & REJECT_BATCH
        else:
            assert not sst[i] & ST_PAIRING_FAILED and sst[i] & REJECT_BATCH


# ------------------------------------------------------------------------------------------------ test 2: the oracle
def test_examined_sets_against_the_oracle(N, mixes):
    m = mixes[1]
    (_res, _st, sres, _sst), examined = _check_against_existing(N, m, "apk")
    assert len(examined) >= 20 and any(sres[i] == 0 for i in examined) and any(sres[i] == 1 for i in examined)
    for i in examined:
        err, sig = orc.g2_from_compressed(m.sigs[i])
        assert not err
        assert bool(sres[i]) == orc.verify_multiple([(sig, m.apks[i], m.msgs[i])], [m.rands[i]]), i


# ------------------------------------------------------------------------------------------------ test 3: every route
@pytest.mark.parametrize("route", ["default", "lanes", "one_lane", "rounds"])
def test_every_route_same_answers(N, mixes, route):
    """the wave engine in phase one (default), lane forms, one lane per item without lane pairs, and calls cut into rounds of 128 plus a rest (phase two as
    well): the same expectation, and the same bytes as the default route"""
    m = mixes[0]
    ctx = N.default_context()
    L = N.lib()
    d = DevMix(N, m)
    want = _call(N, m, d, "apk", True)
    try:
        if route == "lanes":
            assert L.mbls_ctx_set_coop_max_items(ctx.handle, 0) == 0
        elif route == "one_lane":
            assert L.mbls_ctx_set_coop_max_items(ctx.handle, 0) == 0 and L.mbls_ctx_set_lane_shaping(ctx.handle, 0, 0) == 0
        elif route == "rounds":
            assert L.mbls_ctx_set_coop_max_items(ctx.handle, 0) == 0 and L.mbls_ctx_set_round_items(ctx.handle, 128) == 0
        got, _ = _check_against_existing(N, m, "apk", d)
        assert got[0] == want[0] and got[2] == want[2] and got[3] == want[3]
    finally:
        assert L.mbls_ctx_reset_tuning(ctx.handle) == 0


# ------------------------------------------------------------------------------------------------ test 4: placement
def _plain(rnd, n):
    sks = [rnd.randrange(1, helpers.R) for _ in range(n)]
    pk96 = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for s in sks), n, 1, nthreads=8)
    pks = [pk96[96 * i:96 * i + 96] for i in range(n)]
    msgs = [rnd.randbytes(32) for _ in range(n)]
    sigs = [orc.g2_compress(orc.sign(mm, s)) for mm, s in zip(msgs, sks)]
    rands = [rnd.randrange(1, 1 << 63) for _ in range(n)]
    return sigs, pks, msgs, rands


def _plain_mix(sigs, pks, msgs, rands, off):
    return Mix(sigs, pks, [[p, G1_INF_U] for p in pks], msgs, rands, off)


def test_placement_of_the_bad_set(N):
    """one wrong signature (in G2) at the head of its range, at a left partner of level 0, at the last set of an odd-sized batch; a batch where every set is
    bad; a batch with two bad sets -- in a 5-set and an 8-set batch, all in one call with good batches in between. Exactly the bad sets read 0."""
    rnd = random.Random(404)
    cases = [(5, [0]), (5, [2]), (5, [4]), (5, [0, 1, 2, 3, 4]), (5, [1, 3]), (8, [0]), (8, [2]), (8, [6]), (7, [6]), (8, list(range(8))), (8, [3, 4])]
    sizes = []
    for size, _ in cases:
        sizes += [size, 3]                            # a good batch behind every case
    off = _offsets(sizes)
    sigs, pks, msgs, rands = _plain(rnd, off[-1])
    good = list(sigs)
    bad_sets = set()
    for c, (size, bad) in enumerate(cases):
        lo = off[2 * c]
        for j in bad:
            sigs[lo + j] = good[lo + (j + 1) % size] if len(bad) < size else good[off[2 * c + 1] + j % 3]       # another set's signature
            bad_sets.add(lo + j)
    m = _plain_mix(sigs, pks, msgs, rands, off)
    (res, _st, sres, sst), examined = _check_against_existing(N, m, "apk")
    assert res == [0, 1] * len(cases)
    assert [i for i in range(m.n) if sres[i] == 0] == sorted(bad_sets)
    assert all(sst[i] == ST_PAIRING_FAILED for i in bad_sets) and all(sst[i] == 0 for i in range(m.n) if i not in bad_sets)
    assert len(examined) == sum(size for size, _ in cases)


# ------------------------------------------------------------------------------------------------ test 5: not examined
def test_a_passing_batch_is_not_examined(N):
    """sig1 + D and sig2 - [r1 r2^-1 mod r] D: the errors cancel in the batch check under the GIVEN scalars (an attacker who knew them; the blinding makes that a
    2^-63 event), and neither set verifies alone. The batch passes and both sets read 1 -- contract item 2: a passing batch is not examined. The same two sets
    in a batch that a third bad set rejects both read 0."""
    rnd = random.Random(55)
    sigs, pks, msgs, rands = _plain(rnd, 5)
    from pymodel import bls12_381 as M
    D = M.g2_decompress(sigs[4])[1]                   # any point of G2
    c = rands[0] * pow(rands[1], -1, helpers.R) % helpers.R
    s = list(sigs)
    s[0] = M.g2_compress(M.g2_add(M.g2_decompress(sigs[0])[1], D))
    s[1] = M.g2_compress(M.g2_add(M.g2_decompress(sigs[1])[1], M.g2_neg(M.g2_mul(D, c))))
    m = _plain_mix(s[:2], pks[:2], msgs[:2], rands[:2], [0, 2])
    res, st, sres, sst = _call(N, m, DevMix(N, m), "apk", True)
    assert (res, st, sres, sst) == ([1], [0], [1, 1], [0, 0])
    r1, _ = _one_set_batches(N, m, [0, 1], "apk")
    assert r1 == [0, 0]                               # neither verifies alone
    s[2] = sigs[3]                                    # a third set with another set's signature
    m = _plain_mix(s[:3], pks[:3], msgs[:3], rands[:3], [0, 3])
    (res, _st, sres, sst), _ = _check_against_existing(N, m, "apk")
    assert res == [0] and sres == [0, 0, 0] and sst == [ST_PAIRING_FAILED] * 3


# ------------------------------------------------------------------------------------------------ test 6: device-side table faults
def test_device_side_table_faults(N):
    """a range running backwards, a range beyond n_sets, two ranges sharing a set, an uncovered set: the affected sets read 0 with MBLS_ST_BAD_PK_ENCODING; the
    sets of sound batches read what they read under a sound table"""
    rnd = random.Random(66)
    n = 12
    sigs, pks, msgs, rands = _plain(rnd, n)
    sigs[7] = sigs[8]                                 # set 7 is bad by itself: its sound batch is rejected and located
    m = _plain_mix(sigs, pks, msgs, rands, [0, n])
    d = DevMix(N, m)
    sound = [0, 2, 4, 6, 9, 12]
    _res, _st, want_sres, want_sst = _call(N, m, d, "apk", True, boff=_dev(np.array(sound, dtype=np.uint32)), n_batches=5)
    assert want_sres == [1] * 7 + [0, 1] + [1] * 3 and want_sst[7] == ST_PAIRING_FAILED
    # ranges of each table, and the sets that a sound batch owns alone
    tables = {
        "backwards": ([0, 2, 1, 6, 9, 12], list(range(6, 12))),                          # [0,2) [2,1)! [1,6): [0,2) and [1,6) share set 1 -> both lose; [6,9) [9,12) sound
        "beyond": ([0, 2, 4, 6, 9, 40], list(range(0, 9))),                              # [9,40)! its sets 9..11 have no owner
        "shared": ([0, 2, 4, 6, 6, 9, 7, 12], [0, 1, 2, 3, 4, 5]),                        # [6,9) and [7,12) share 7, 8; [9,7)! runs backwards
        "uncovered": ([0, 2, 4, 6, 9, 11], list(range(0, 11))),                          # set 11 is in no range
    }
    for name, (tab, owned) in tables.items():
        B = len(tab) - 1
        boff = _dev(np.array(tab, dtype=np.uint32))
        res0, st0 = _call(N, m, d, "apk", False, boff=boff, n_batches=B)
        res, st, sres, sst = _call(N, m, d, "apk", True, boff=boff, n_batches=B)
        assert (res, st) == (res0, st0), name
        for i in range(n):
            if i in owned:
                assert (sres[i], sst[i]) == (want_sres[i], want_sst[i]), (name, i, sres[i], hex(sst[i]))
            else:
                assert sres[i] == 0 and sst[i] & ST_BAD_PK, (name, i, sres[i], hex(sst[i]))


# ------------------------------------------------------------------------------------------------ test 7: the _rng form
def test_rng_form_draws_as_the_batches_entry(N, vectors):
    """one batch has a signature outside G2 in the middle: the source is asked for the same scalars as by mbls_verify_multiple_batches_rng (counts and values;
    the Python mirrors leave random.Random in the same state); the sets at or behind the bad signature read 0; the sets in front are examined, and the one with
    a wrong key among them reads 0 with MBLS_ST_PAIRING_FAILED"""
    from milagro_bls_amd import AggregateSignature, AggregatePublicKey
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    rnd = random.Random(77)
    sizes = [3, 6, 2]
    off = _offsets(sizes)
    n = off[-1]
    sigs, pks, msgs, rands = _plain(rnd, n)
    sigs[off[1] + 3] = probe                          # batch 1: sets 3, 4, 5 have no scalar
    pks[off[1] + 1] = pks[0]                          # batch 1, set 1: wrong key, in front of the bad signature
    ctx = N.default_context()

    def run(locate):
        asked, handed = [], []

        def draw(_user, out, count):
            for i in range(count):
                out[i] = rands[i]; handed.append(rands[i])
            asked.append(int(count))
        cb = N.SCALAR_SOURCE(draw)
        res = N.outbuf(3); sres = N.outbuf(n); sst = (C.c_uint32 * n)()
        boff = (C.c_uint32 * len(off))(*off)
        args = (ctx.handle, N.cbuf(b"".join(sigs)), N.cbuf(b"".join(pks)), N.cbuf(b"".join(msgs)), 32, None, n, boff, 0, 3, res)
        if locate:
            rc = N.lib().mbls_verify_multiple_batches_locate_rng(*args, sres, sst, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_batches_rng(*args, cb, None)
        assert rc == 0, ctx.last_error()
        return list(bytes(res)[:3]), asked, handed, list(bytes(sres)[:n]), list(sst)
    res0, asked0, handed0, _, _ = run(False)
    res, asked, handed, sres, sst = run(True)
    assert (res, asked, handed) == (res0, asked0, handed0) and res == [1, 0, 1] and asked == [3 + 3 + 2]
    lo = off[1]
    assert sres[:lo] == [1] * 3 and sres[off[2]:] == [1] * 2
    assert sres[lo:lo + 6] == [1, 0, 1, 0, 0, 0]
    assert sst[lo + 1] == ST_PAIRING_FAILED and sst[lo] == 0 and sst[lo + 2] == 0
    assert sst[lo + 3] & 0x02 and not sst[lo + 3] & ST_PAIRING_FAILED and sst[lo + 4] == 0 and sst[lo + 5] == 0
    # the Python mirror: same per-batch bools and generator state as the batches method
    batches = [[(AggregateSignature(sigs[i]), AggregatePublicKey(pks[i]), msgs[i]) for i in range(off[b], off[b + 1])] for b in range(3)]
    g1, g2 = random.Random(4242), random.Random(4242)
    per_batch, per_set = AggregateSignature.verify_multiple_aggregate_signatures_batches_locate(g1, batches)
    assert per_batch == AggregateSignature.verify_multiple_aggregate_signatures_batches(g2, batches) == [True, False, True]
    assert g1.getstate() == g2.getstate()
    assert per_set == [[True] * 3, [True, False, True, False, False, False], [True] * 2]
    assert AggregateSignature.verify_multiple_aggregate_signatures_batches_locate(random.Random(1), []) == ([], [])
    assert AggregateSignature.verify_multiple_aggregate_signatures_batches_locate(random.Random(1), [[], []]) == ([True, True], [[], []])


# ------------------------------------------------------------------------------------------------ test 8: arguments
def test_argument_handling_and_workspace_reuse(N):
    import torch
    from milagro_bls_amd import batch
    rnd = random.Random(88)
    sigs, pks, msgs, rands = _plain(rnd, 6)
    sigs[4] = sigs[5]
    ctx = N.default_context()
    S, A, M = N.cbuf(b"".join(sigs)), N.cbuf(b"".join(pks)), N.cbuf(b"".join(msgs))
    rr = (C.c_uint64 * 6)(*rands)
    f = N.lib().mbls_verify_multiple_batches_locate
    res = N.outbuf(8); st = (C.c_uint32 * 8)(); sres = N.outbuf(8); sst = (C.c_uint32 * 8)()
    off = lambda *v: (C.c_uint32 * len(v))(*v)
    marker = bytes([9] * 8)
    C.memmove(res, marker, 8); C.memmove(sres, marker, 8)
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 2, 6), 0, 2, res, st, None, sst) == N.ERR_ARGUMENT          # no set results
    assert f(ctx.handle, S, A, M, 32, None, None, 6, off(0, 2, 6), 0, 2, res, st, sres, sst) == N.ERR_ARGUMENT       # no scalars
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 2, 6), 0, 2, None, st, sres, sst) == N.ERR_ARGUMENT        # no results
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 4, 2, 6), 0, 3, res, st, sres, sst) == N.ERR_ARGUMENT      # runs backwards
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(1, 2, 6), 0, 2, res, st, sres, sst) == N.ERR_ARGUMENT         # does not start at 0
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 2, 5), 0, 2, res, st, sres, sst) == N.ERR_ARGUMENT         # does not end at n_sets
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, None, 4, 2, res, st, sres, sst) == N.ERR_ARGUMENT                  # 2 x 4 != 6
    assert bytes(res)[:8] == marker and bytes(sres)[:8] == marker                                                      # nothing written
    assert f(ctx.handle, S, A, M, 32, None, rr, 0, None, 0, 0, res, st, sres, sst) == 0 and bytes(res)[:8] == marker and bytes(sres)[:8] == marker
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 2, 6), 0, 2, res, st, sres, None) == 0                       # the status words are optional
    assert bytes(res)[:2] == b"\x01\x00" and bytes(sres)[:6] == b"\x01\x01\x01\x01\x00\x01"
    # the device form: NULL d_set_results is refused on the host and nothing is written; n_batches = 0 is accepted
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")
    d_s, d_a, d_m = t(b"".join(sigs)), t(b"".join(pks)), t(b"".join(msgs))
    d_r = _dev(np.array(rands, dtype=np.uint64)); d_o = _dev(np.array([0, 2, 6], dtype=np.uint32))
    d_res = torch.full((8,), 7, dtype=torch.uint8, device="cuda:0"); d_sres = torch.full((8,), 7, dtype=torch.uint8, device="cuda:0")
    fd = N.lib().mbls_verify_multiple_batches_locate_device
    head = (ctx.handle, d_s.data_ptr(), d_a.data_ptr(), None, 0, None, 0, d_m.data_ptr(), 32, None)
    assert fd(*head, d_r.data_ptr(), 6, d_o.data_ptr(), 0, 2, d_res.data_ptr(), None, None, None, None) == N.ERR_ARGUMENT
    assert fd(*head, None, 6, d_o.data_ptr(), 0, 2, d_res.data_ptr(), None, d_sres.data_ptr(), None, None) == N.ERR_ARGUMENT
    assert fd(*head, d_r.data_ptr(), 6, None, 4, 2, d_res.data_ptr(), None, d_sres.data_ptr(), None, None) == N.ERR_ARGUMENT
    assert fd(*head, d_r.data_ptr(), 0, None, 0, 0, d_res.data_ptr(), None, d_sres.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in d_res.cpu().numpy()] == [7] * 8 and [int(x) for x in d_sres.cpu().numpy()] == [7] * 8
    assert fd(*head, d_r.data_ptr(), 6, d_o.data_ptr(), 0, 2, d_res.data_ptr(), None, d_sres.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in d_res.cpu().numpy()[:2]] == [1, 0] and [int(x) for x in d_sres.cpu().numpy()[:6]] == [1, 1, 1, 1, 0, 1]
    # repeated on one context and interleaved with mbls_verify_multiple_batches: the workspace is reused (its reserved size is the plan's and does not grow)
    # and the results do not change
    want = batch.verify_multiple_batches_locate(b"".join(sigs), b"".join(pks), b"".join(msgs), rands, 6, 2, batch_offsets=[0, 2, 6])
    assert want == ([True, False], [0, ST_PAIRING_FAILED], [True, True, True, True, False, True], [0, 0, 0, 0, ST_PAIRING_FAILED, 0])
    assert N.plan_locate_workspace_items(6, 2) == 3 * 6
    for _ in range(3):
        assert batch.verify_multiple_batches(b"".join(sigs), b"".join(pks), b"".join(msgs), rands, 6, 2, batch_offsets=[0, 2, 6]) == (want[0], want[1])
        assert batch.verify_multiple_batches_locate(b"".join(sigs), b"".join(pks), b"".join(msgs), rands, 6, 2, batch_offsets=[0, 2, 6]) == want
