"""GPU tests of mbls_verify_multiple*_shared_msgs_locate* (include/mbls.h, "WHICH SETS OF A REJECTED SHARED-MESSAGE CALL"): the call's outputs against
mbls_verify_multiple_shared_msgs_device, the per-set outputs against mbls_verify_multiple_batches_locate_device with one batch on the spelled-out messages and
against the oracle, under every grouping mode and both key forms; the placement of a bad set on the grouped route, every launch route, the sets a passing call
hides, message faults of device-side lists, the reference's RNG order and the argument handling. The mix is built as tests/test_gpu_vm_locate.py builds its own,
over a shared list."""
import ctypes as C
import random

import numpy as np
import pytest

import helpers
import orc

pytestmark = pytest.mark.gpu

G1_INF_U = bytes([0x40]) + bytes(95)
ST_SIG_NOT_IN_G2, ST_PAIRING_FAILED, ST_BAD_MSG_RANGE = 0x02, 0x40, 0x100
REJECT_BATCH = 0x01 | 0x02 | 0x04 | 0x100 | 0x80          # mbls_coop.h COOP_REJECT_BATCH
DEFECTS = ("wrong_key", "swapped_sig", "inf_sig", "inf_key", "both_inf", "not_in_g2", "undecodable", "zero_scalar")
RAGGED_LENS = [0, 1, 31, 32, 33, 55, 56, 64, 65, 100, 200]
MODES = (0, 1, 2)


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


def _offsets(items):
    off = [0]
    for x in items:
        off.append(off[-1] + len(x))
    return off


class Case:
    """n sets over a list: sigs / apks / wire (two 96 B keys per set) / rands per set, `listed` messages and idx per set"""

    def __init__(self, sigs, apks, wire, rands, listed, idx):
        self.sigs, self.apks, self.wire, self.rands, self.listed, self.idx = list(sigs), list(apks), [list(w) for w in wire], list(rands), list(listed), list(idx)
        self.n = len(self.sigs)

    def spelled(self):
        return [self.listed[j] for j in self.idx]


class DevCase:
    def __init__(self, N, c, table=False):
        self.n, self.n_msgs = c.n, len(c.listed)
        self.sigs = _dev(b"".join(c.sigs)); self.apks = _dev(b"".join(c.apks)); self.rands = _dev(np.array(c.rands, dtype=np.uint64))
        self.list = _dev(b"".join(c.listed)); self.list_off = _dev(np.array(_offsets(c.listed), dtype=np.uint64))
        self.idx = _dev(np.array(c.idx, dtype=np.uint32))
        sp = c.spelled()
        self.msgs = _dev(b"".join(sp)); self.moff = _dev(np.array(_offsets(sp), dtype=np.uint64))
        self.tab = self.key_idx = None
        if table:
            self.tab = N.KeyTable()
            first, errs = self.tab.append(b"".join(k for w in c.wire for k in w), 2 * c.n, pk_format=N.PK_UNCOMPRESSED, validate=False)
            assert not any(errs)
            self.key_idx = _dev(np.arange(first, first + 2 * c.n, dtype=np.uint32))


def _bufs(n):
    import torch
    return (torch.full((8,), 7, dtype=torch.uint8, device="cuda:0"), torch.full((2,), -1, dtype=torch.int32, device="cuda:0"),
            torch.full((max(1, n),), 7, dtype=torch.uint8, device="cuda:0"), torch.full((max(1, n),), -1, dtype=torch.int32, device="cuda:0"))


def call_shared(N, d, mode, locate, indexed=False, n_msgs=None, idx=None, list_off=None):
    """the shared-message entry (locate = False) or its locate form under grouping `mode` -> (result, status[, set results, set status])"""
    import torch
    from milagro_bls_amd import batch
    ctx = N.default_context()
    res, st, sres, sst = _bufs(d.n)
    n_msgs = d.n_msgs if n_msgs is None else n_msgs
    idx = d.idx if idx is None else idx
    list_off = d.list_off if list_off is None else list_off
    L = N.lib()
    tail = (res.data_ptr(), st.data_ptr()) + ((sres.data_ptr(), sst.data_ptr()) if locate else ()) + (None,)
    common = (d.list.data_ptr(), 0, list_off.data_ptr(), n_msgs, idx.data_ptr(), d.rands.data_ptr(), d.n)
    batch.set_vm_grouping(mode, ctx)
    try:
        if indexed:
            f = L.mbls_verify_multiple_sets_indexed_shared_msgs_locate_device if locate else L.mbls_verify_multiple_sets_indexed_shared_msgs_device
            rc = f(ctx.handle, d.tab.handle, d.sigs.data_ptr(), d.key_idx.data_ptr(), None, 2, *common, *tail)
        else:
            f = L.mbls_verify_multiple_shared_msgs_locate_device if locate else L.mbls_verify_multiple_shared_msgs_device
            rc = f(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), *common, *tail)
        assert rc == 0, ctx.last_error()
        torch.cuda.synchronize()
    finally:
        batch.set_vm_grouping(0, ctx)
    out = (int(res[0].item()), int(st[0].item()) & 0xFFFFFFFF)
    if locate:
        assert [int(x) for x in res.cpu().numpy()[1:]] == [7] * 7
        out += ([int(x) for x in sres.cpu().numpy()[:d.n]], [int(x) & 0xFFFFFFFF for x in sst.cpu().numpy()[:d.n]])
    return out


def one_batch_locate(N, d, indexed=False):
    """mbls_verify_multiple_batches_locate[_indexed]_device with ONE batch over the spelled-out messages -> (set results, set status)"""
    import torch
    ctx = N.default_context()
    res, st, sres, sst = _bufs(d.n)
    L = N.lib()
    common = (d.msgs.data_ptr(), 0, d.moff.data_ptr(), d.rands.data_ptr(), d.n, None, d.n, 1, res.data_ptr(), st.data_ptr(), sres.data_ptr(), sst.data_ptr(), None)
    if indexed:
        rc = L.mbls_verify_multiple_batches_locate_indexed_device(ctx.handle, d.tab.handle, d.sigs.data_ptr(), d.key_idx.data_ptr(), None, 2, *common)
    else:
        rc = L.mbls_verify_multiple_batches_locate_device(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), None, N.PK_UNCOMPRESSED, None, 0, *common)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    return int(res[0].item()), [int(x) for x in sres.cpu().numpy()[:d.n]], [int(x) & 0xFFFFFFFF for x in sst.cpu().numpy()[:d.n]]


def build_mix(seed, n, listed, probe):
    """every set has two keys: sig = [sk1 + sk2] H(msg), apk = pk1 + pk2 = the wire keys (pk1, pk2); every defect of DEFECTS on one set each"""
    rnd = random.Random(seed)
    M = len(listed)
    sks = [(rnd.randrange(1, helpers.R), rnd.randrange(1, helpers.R)) for _ in range(n)]
    pk96 = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for pair in sks for s in pair), 2 * n, 1, nthreads=8)
    wire = [[pk96[192 * i:192 * i + 96], pk96[192 * i + 96:192 * i + 192]] for i in range(n)]
    apks = [orc.g1_add(w[0], w[1]) for w in wire]
    idx = list(range(M)) + [rnd.randrange(M) for _ in range(n - M)]
    rnd.shuffle(idx)
    sigs = [orc.g2_compress(orc.sign(listed[j], (a + b) % helpers.R)) for j, (a, b) in zip(idx, sks)]
    rands = [rnd.randrange(1, 1 << 63) for _ in range(n)]
    c = Case(sigs, apks, wire, rands, listed, idx)
    c.defect = {}
    for kind, i in zip(DEFECTS, rnd.sample(range(n), len(DEFECTS))):
        other = next(j for j in range(n) if j != i and j not in c.defect)
        if kind == "wrong_key":
            c.apks[i], c.wire[i] = apks[other], list(wire[other])
        elif kind == "swapped_sig":
            c.sigs[i] = sigs[other]
        elif kind == "inf_sig":
            c.sigs[i] = helpers.G2_INF
        elif kind == "inf_key":
            c.apks[i] = G1_INF_U; c.wire[i] = [wire[i][0], orc.g1_mul(wire[i][0], helpers.R - 1)]
        elif kind == "both_inf":
            c.sigs[i] = helpers.G2_INF; c.apks[i] = G1_INF_U; c.wire[i] = [wire[i][0], orc.g1_mul(wire[i][0], helpers.R - 1)]
        elif kind == "not_in_g2":
            c.sigs[i] = probe
        elif kind == "undecodable":
            c.sigs[i] = bytes([sigs[i][0] & 0x7F]) + sigs[i][1:]
        elif kind == "zero_scalar":
            c.rands[i] = 0
        c.defect[i] = kind
    return c


@pytest.fixture(scope="module")
def mixes(vectors):
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    r = random.Random(7)
    return [build_mix(2030, 200, [r.randbytes(32) for _ in range(5)], probe), build_mix(2031, 64, [r.randbytes(l) for l in RAGGED_LENS], probe)]


def check_call(N, c, d, mode, indexed=False, **kw):
    """contract items 1 - 4 for one case, mode and key form against the existing entries; returns the locate call's outputs"""
    r0, s0 = call_shared(N, d, mode, False, indexed, **kw)
    res, st, sres, sst = call_shared(N, d, mode, True, indexed, **kw)
    assert (res, st) == (r0, s0), (mode, indexed, res, hex(st), r0, hex(s0))                     # item 1
    if res:
        assert sres == [1] * c.n and not any(w & (ST_PAIRING_FAILED | REJECT_BATCH) for w in sst), (mode, indexed)      # item 2
    for i in range(c.n):
        assert bool(sst[i] & ST_PAIRING_FAILED) == (not res and not sst[i] & REJECT_BATCH and not sres[i]), (mode, indexed, i, hex(sst[i]))
    return res, st, sres, sst


# ------------------------------------------------------------------------------------------------ test 1: the mix against the existing entries
@pytest.mark.parametrize("indexed", [False, True], ids=["apk", "indexed"])
@pytest.mark.parametrize("which", [0, 1], ids=["200over5", "64ragged"])
def test_mix_against_the_existing_entries(N, mixes, which, indexed):
    """the call's result and status equal mbls_verify_multiple_shared_msgs_device under modes 0, 1 and 2; the per-set results and status words equal
    mbls_verify_multiple_batches_locate_device with one batch on the spelled-out messages; modes 1 and 2 are byte-equal; every defect reads what it must"""
    c = mixes[which]
    assert sorted(c.defect.values()) == sorted(DEFECTS)
    d = DevCase(N, c, table=indexed)
    ref_res, ref_sres, ref_sst = one_batch_locate(N, d, indexed)
    assert ref_res == 0
    got = {}
    for mode in MODES:
        res, st, sres, sst = got[mode] = check_call(N, c, d, mode, indexed)
        assert res == 0
        assert sres == ref_sres, (mode, [(i, sres[i], ref_sres[i]) for i in range(c.n) if sres[i] != ref_sres[i]])          # item 3
        assert sst == ref_sst, (mode, [(i, hex(sst[i]), hex(ref_sst[i])) for i in range(c.n) if sst[i] != ref_sst[i]])       # item 4
    assert got[1] == got[2] == got[0]
    _res, _st, sres, sst = got[1]
    for i in range(c.n):
        kind = c.defect.get(i)
        if kind is None or kind == "both_inf":
            assert sres[i] == 1 and not sst[i] & (ST_PAIRING_FAILED | REJECT_BATCH), (i, kind, hex(sst[i]))
        elif kind in ("wrong_key", "swapped_sig", "inf_sig", "inf_key"):
            assert sres[i] == 0 and sst[i] & ST_PAIRING_FAILED and not sst[i] & REJECT_BATCH, (i, kind, hex(sst[i]))
        else:
            assert sres[i] == 0 and not sst[i] & ST_PAIRING_FAILED and sst[i] & REJECT_BATCH, (i, kind, hex(sst[i]))
    plan = N.plan_verify_multiple_shared_msgs(c.n, len(c.listed), 0)
    assert plan["route"] == N.VM_ROUTE_GROUPED                                                    # (mode 0 took the grouped route, mode 2 the other)


# ------------------------------------------------------------------------------------------------ test 2: the oracle
@pytest.mark.parametrize("which", [0, 1], ids=["200over5", "64ragged"])
def test_examined_sets_against_the_oracle(N, mixes, which):
    c = mixes[which]
    d = DevCase(N, c)
    res, _st, sres, sst = call_shared(N, d, 1, True)
    assert res == 0
    examined = [i for i in range(c.n) if not sst[i] & REJECT_BATCH]
    assert len(examined) == c.n - 3 and any(sres[i] == 0 for i in examined) and any(sres[i] == 1 for i in examined)
    sp = c.spelled()
    for i in examined:
        err, sig = orc.g2_from_compressed(c.sigs[i])
        assert not err
        assert bool(sres[i]) == orc.verify_multiple([(sig, c.apks[i], sp[i])], [c.rands[i]]), i


# ------------------------------------------------------------------------------------------------ tests 3 - 8 work on plain sets: one key each
_POOL = {}


def plain_case(n, listed, idx, seed):
    """n valid one-key sets over `listed` (wire = (pk, infinity)); the keys and signatures are made once per (seed, message, slot)"""
    rnd = random.Random(seed)
    sks = [rnd.randrange(1, helpers.R) for _ in range(n)]
    key = (seed, n)
    if key not in _POOL:
        pk96 = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for s in sks), n, 1, nthreads=8)
        _POOL[key] = [pk96[96 * i:96 * i + 96] for i in range(n)]
    pks = _POOL[key]
    sigs = []
    for i in range(n):
        k = (seed, i, listed[idx[i]])
        if k not in _POOL:
            _POOL[k] = orc.g2_compress(orc.sign(listed[idx[i]], sks[i]))
        sigs.append(_POOL[k])
    rands = [rnd.randrange(1, 1 << 63) for _ in range(n)]
    return Case(sigs, pks, [[p, G1_INF_U] for p in pks], rands, listed, idx)


def spare_key():
    if "spare" not in _POOL:
        _POOL["spare"] = orc.sk_to_pk(0x5eed)
    return _POOL["spare"]


# ------------------------------------------------------------------------------------------------ test 3: placement on the grouped route
PLACEMENT = [
    # (n, M, idx, the bad positions tried one by one)
    (5, 3, [0, 1, 0, 2, 1], [0, 1, 2, 3, 4]),                 # groups of 2, 2 and 1; index 0, M - 1 = 2, M = 3, n - 1 = 4
    (2, 1, [0, 0], [0, 1]),                                   # one group of two: the left and the right partner of the only level
    (3, 7, [6, 0, 3], [0, 1, 2]),                             # more messages than sets under mode 1: pbase = M, three groups of one
    # groups of 3, 4, 5 and 21 interleaved: message 0 = sets {0, 5, 32}, message 1 = {1, 2, 6, 7}, message 2 = {3, 4, 8, 9, 10}, message 3 = the rest
    (33, 4, [0, 1, 1, 2, 2, 0, 1, 1, 2, 2, 2] + [3] * 21 + [0], [0, 3, 4, 32, 5, 1, 7, 2, 6, 8, 10, 11, 31, 20]),
]


@pytest.mark.parametrize("shape", range(len(PLACEMENT)), ids=["n%d_M%d" % (p[0], p[1]) for p in PLACEMENT])
def test_placement_of_the_bad_set_on_the_grouped_route(N, shape):
    """one set with a wrong key at set index 0, M - 1, M and n - 1 -- the heads overwrite the key slots of items [0, M) --, at the first and the last set of a
    group, in a group of one and in groups of 2, 3, 4 and 5 (a left and a right partner at the first tree levels): every other set reads 1, the bad one 0 with
    MBLS_ST_PAIRING_FAILED"""
    n, M, idx, tries = PLACEMENT[shape]
    assert len(idx) == n
    rnd = random.Random(500 + shape)
    listed = [rnd.randbytes(32) for _ in range(M)]
    good = plain_case(n, listed, idx, 510 + shape)
    assert N.plan_verify_multiple_shared_msgs(n, M, 1)["route"] == N.VM_ROUTE_GROUPED
    for p in tries:
        c = Case(good.sigs, good.apks, good.wire, good.rands, listed, idx)
        c.apks[p] = spare_key(); c.wire[p] = [spare_key(), G1_INF_U]
        res, _st, sres, sst = check_call(N, c, DevCase(N, c), 1)
        assert res == 0
        assert sres == [0 if i == p else 1 for i in range(n)], (n, M, p, sres)
        assert sst == [ST_PAIRING_FAILED if i == p else 0 for i in range(n)], (n, M, p, [hex(w) for w in sst])


# ------------------------------------------------------------------------------------------------ test 4: every route
@pytest.fixture(scope="module")
def case130():
    rnd = random.Random(44)
    listed = [rnd.randbytes(32) for _ in range(5)]
    idx = list(range(5)) + [rnd.randrange(5) for _ in range(125)]
    c = plain_case(130, listed, idx, 440)
    c.bad = [0, 4, 63, 64, 127, 128, 129]                     # on both sides of the round boundary of the 2 n-item Miller launch, and in its rest of 4
    for p in c.bad:
        c.apks[p] = spare_key(); c.wire[p] = [spare_key(), G1_INF_U]
    c.sigs[77] = helpers.G2_INF                               # the call is rejected by its pairing check alone: every set is a candidate
    return c


@pytest.mark.parametrize("route", ["default", "lanes", "one_lane", "rounds"])
def test_every_route_same_answers(N, case130, route):
    """the wave engine in phase one (default), lane forms, one lane per item without lane pairs, and rounds of 128 with n = 130 -- the 2 n-item Miller launch and
    the product then cross a round boundary with a rest of 4: the same expectation in modes 1 and 2, and the same bytes as the default route"""
    c = case130
    ctx = N.default_context()
    L = N.lib()
    d = DevCase(N, c)
    want = {mode: call_shared(N, d, mode, True) for mode in (1, 2)}
    bad = sorted(c.bad + [77])
    for mode in (1, 2):
        res, _st, sres, sst = want[mode]
        assert res == 0 and [i for i in range(c.n) if not sres[i]] == bad and sst == [ST_PAIRING_FAILED if i in bad else 0 for i in range(c.n)]
    try:
        if route == "lanes":
            assert L.mbls_ctx_set_coop_max_items(ctx.handle, 0) == 0
        elif route == "one_lane":
            assert L.mbls_ctx_set_coop_max_items(ctx.handle, 0) == 0 and L.mbls_ctx_set_lane_shaping(ctx.handle, 0, 0) == 0
        elif route == "rounds":
            assert L.mbls_ctx_set_coop_max_items(ctx.handle, 0) == 0 and L.mbls_ctx_set_lane_shaping(ctx.handle, 0, 0) == 0
            assert L.mbls_ctx_set_round_items(ctx.handle, 128) == 0
        for mode in (1, 2):
            assert check_call(N, c, d, mode) == want[mode], (route, mode)
    finally:
        assert L.mbls_ctx_reset_tuning(ctx.handle) == 0


# ------------------------------------------------------------------------------------------------ test 5: not examined
def test_a_passing_call_is_not_examined(N):
    """sig0 + D and sig1 - [r0 r1^-1 mod r] D: the errors cancel in the batch check under the GIVEN scalars (an attacker who knew them; the blinding makes that a
    2^-63 event), and neither set verifies alone. The call passes and both sets read 1 -- contract item 2. The same two sets in a call that a third bad set
    rejects both read 0. On both routes."""
    from pymodel import bls12_381 as M
    rnd = random.Random(55)
    listed = [rnd.randbytes(32), rnd.randbytes(32)]
    g = plain_case(4, listed, [0, 1, 1, 0], 550)
    D = M.g2_decompress(g.sigs[3])[1]                 # any point of G2
    k = g.rands[0] * pow(g.rands[1], -1, helpers.R) % helpers.R
    s = list(g.sigs)
    s[0] = M.g2_compress(M.g2_add(M.g2_decompress(g.sigs[0])[1], D))
    s[1] = M.g2_compress(M.g2_add(M.g2_decompress(g.sigs[1])[1], M.g2_neg(M.g2_mul(D, k))))
    two = Case(s[:2], g.apks[:2], g.wire[:2], g.rands[:2], listed, [0, 1])
    s[2] = g.sigs[3]                                  # a third set with another set's signature
    three = Case(s[:3], g.apks[:3], g.wire[:3], g.rands[:3], listed, [0, 1, 1])
    for mode in (1, 2):
        assert check_call(N, two, DevCase(N, two), mode) == (1, 0, [1, 1], [0, 0]), mode
        assert one_batch_locate(N, DevCase(N, three))[1] == [0, 0, 0]                               # none of the three verifies alone
        assert check_call(N, three, DevCase(N, three), mode) == (0, 0, [0, 0, 0], [ST_PAIRING_FAILED] * 3), mode


# ------------------------------------------------------------------------------------------------ test 6: message faults
def test_message_faults_of_device_side_lists(N):
    """an index >= n_msgs, n_msgs = 0, and an offset table with a backward range one set names and another nobody names: the affected sets read 0 with
    MBLS_ST_BAD_MSG_RANGE in their OWN word and no pairing failure; the sets of sound messages keep their answers (one of them has a wrong key). The call's
    bool and word stay those of the entry without _locate. In every mode."""
    rnd = random.Random(66)
    buf = rnd.randbytes(48)
    # five messages cut out of one 48-byte buffer by absolute offsets
    fault_off = [0, 32, 0, 40, 8, 48]                 # message 1 = [32, 0) and message 3 = [40, 8) run backwards; 0 = [0, 32), 2 = [0, 40), 4 = [8, 48)
    listed_fault = [buf[0:32], b"", buf[0:40], b"", buf[8:48]]
    idx = [0, 2, 4, 1, 2, 0, 4, 2]                    # set 3 names the broken message 1; nobody names message 3
    c = plain_case(8, listed_fault, idx, 660)
    c.apks[5] = spare_key(); c.wire[5] = [spare_key(), G1_INF_U]
    d = DevCase(N, c)
    d.list = _dev(buf)
    off = _dev(np.array(fault_off, dtype=np.uint64))
    for mode in MODES:
        res, st, sres, sst = check_call(N, c, d, mode, list_off=off)
        assert res == 0 and st & ST_BAD_MSG_RANGE
        assert sres == [1, 1, 1, 0, 1, 0, 1, 1], (mode, sres)
        assert sst == [0, 0, 0, ST_BAD_MSG_RANGE, 0, ST_PAIRING_FAILED, 0, 0], (mode, [hex(w) for w in sst])
    # the broken message named by nobody: the call is rejected by set 5 alone, and every other set reads 1
    idx2 = [0, 2, 4, 4, 2, 0, 4, 2]
    c2 = plain_case(8, listed_fault, idx2, 661)
    c2.apks[5] = spare_key(); c2.wire[5] = [spare_key(), G1_INF_U]
    d2 = DevCase(N, c2); d2.list = _dev(buf)
    for mode in MODES:
        assert check_call(N, c2, d2, mode, list_off=off) == (0, 0, [1, 1, 1, 1, 1, 0, 1, 1], [0, 0, 0, 0, 0, ST_PAIRING_FAILED, 0, 0]), mode
    # indices that name no message: n_msgs itself, far outside, 2^32 - 1 -- and the same list cut down to its first two messages
    listed = [rnd.randbytes(32) for _ in range(3)]
    c3 = plain_case(6, listed, [0, 1, 2, 1, 0, 2], 662)
    d3 = DevCase(N, c3)
    for bad_idx, n_msgs in (([0, 3, 2, 1000, 0, 0xFFFFFFFF], 3), ([0, 1, 2, 1, 0, 2], 2)):
        out_of_list = [j >= n_msgs for j in bad_idx]
        for mode in MODES:
            res, st, sres, sst = check_call(N, c3, d3, mode, n_msgs=n_msgs, idx=_dev(np.array(bad_idx, dtype=np.uint32)))
            assert res == 0 and st & ST_BAD_MSG_RANGE
            assert sres == [0 if o else 1 for o in out_of_list], (mode, bad_idx, sres)
            assert sst == [ST_BAD_MSG_RANGE if o else 0 for o in out_of_list], (mode, bad_idx, [hex(w) for w in sst])
    # the empty list: every set carries the bit, nothing is examined
    for mode in MODES:
        assert check_call(N, c3, d3, mode, n_msgs=0) == (0, ST_BAD_MSG_RANGE, [0] * 6, [ST_BAD_MSG_RANGE] * 6), mode


# ------------------------------------------------------------------------------------------------ test 7: the _rng form
def test_rng_form_draws_as_the_shared_entry(N, vectors):
    """a signature outside G2 in the middle: the source is asked for the same scalars as by mbls_verify_multiple_shared_msgs_rng (counts and values; the Python
    mirrors leave random.Random in the same state); the sets at or behind the bad signature read 0; the sets in front are examined, and the one with a wrong
    key among them reads 0 with MBLS_ST_PAIRING_FAILED. On both routes."""
    from milagro_bls_amd import AggregateSignature, AggregatePublicKey, batch
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    rnd = random.Random(77)
    listed = [rnd.randbytes(l) for l in (32, 0, 57)]
    idx = [0, 1, 2, 2, 1, 0, 0, 2]
    n = len(idx)
    good = plain_case(n, listed, idx, 770)
    c = Case(good.sigs, good.apks, good.wire, good.rands, listed, idx)
    c.sigs[5] = probe                                 # sets 5, 6, 7 have no scalar
    c.apks[2] = spare_key()                           # wrong key, in front of the bad signature
    ctx = N.default_context()
    moff = (C.c_uint64 * (len(listed) + 1))(*_offsets(listed))
    midx = (C.c_uint32 * n)(*idx)

    def run(case, locate):
        asked, handed = [], []

        def draw(_user, out, count):
            for i in range(count):
                out[i] = case.rands[i]; handed.append(case.rands[i])
            asked.append(int(count))
        cb = N.SCALAR_SOURCE(draw)
        res = N.outbuf(1); sres = N.outbuf(n); sst = (C.c_uint32 * n)()
        args = (ctx.handle, N.cbuf(b"".join(case.sigs)), N.cbuf(b"".join(case.apks)), N.cbuf(b"".join(listed)), 0, moff, len(listed), midx, n, res)
        if locate:
            rc = N.lib().mbls_verify_multiple_shared_msgs_locate_rng(*args, sres, sst, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_shared_msgs_rng(*args, cb, None)
        assert rc == 0, ctx.last_error()
        return bytes(res)[0], asked, handed, list(bytes(sres)[:n]), list(sst)
    for mode in (1, 2):
        batch.set_vm_grouping(mode, ctx)
        try:
            r0, asked0, handed0, _, _ = run(c, False)
            r, asked, handed, sres, sst = run(c, True)
            assert (r, asked, handed) == (r0, asked0, handed0) and r == 0 and asked == [5]
            assert sres == [1, 1, 0, 1, 1, 0, 0, 0], (mode, sres)
            assert sst[:5] == [0, 0, ST_PAIRING_FAILED, 0, 0] and sst[5] & ST_SIG_NOT_IN_G2 and not sst[5] & ST_PAIRING_FAILED and sst[6:] == [0, 0], (mode, sst)
            r0, asked0, handed0, _, _ = run(good, False)
            assert run(good, True) == (r0, asked0, handed0, [1] * n, [0] * n) and r0 == 1 and asked0 == [n]
            # the Python mirror: same bool and generator state as the shared-message method
            sets = [(AggregateSignature(c.sigs[i]), AggregatePublicKey(c.apks[i]), listed[idx[i]]) for i in range(n)]
            g1, g2 = random.Random(4242), random.Random(4242)
            ok, per_set = AggregateSignature.verify_multiple_aggregate_signatures_shared_msgs_locate(g1, sets)
            assert ok == AggregateSignature.verify_multiple_aggregate_signatures_shared_msgs(g2, sets) is False
            assert g1.getstate() == g2.getstate()
            assert per_set == [True, True, False, True, True, False, False, False]
        finally:
            batch.set_vm_grouping(0, ctx)
    assert AggregateSignature.verify_multiple_aggregate_signatures_shared_msgs_locate(random.Random(1), []) == (True, [])


# ------------------------------------------------------------------------------------------------ test 8: arguments and reuse
def test_argument_handling_and_workspace_reuse(N):
    import torch
    from milagro_bls_amd import batch
    rnd = random.Random(88)
    listed = [rnd.randbytes(32) for _ in range(3)]
    idx = [0, 1, 2, 1, 0, 1]
    c = plain_case(6, listed, idx, 880)
    c.sigs[4] = c.sigs[5]
    ctx = N.default_context()
    S, A, Mb = N.cbuf(b"".join(c.sigs)), N.cbuf(b"".join(c.apks)), N.cbuf(b"".join(listed))
    rr = (C.c_uint64 * 6)(*c.rands)
    mi = lambda *v: (C.c_uint32 * len(v))(*v)
    f = N.lib().mbls_verify_multiple_shared_msgs_locate
    res = N.outbuf(8); st = C.c_uint32(0xAAAA); sres = N.outbuf(8); sst = (C.c_uint32 * 8)()
    marker = bytes([9] * 8)
    C.memmove(res, marker, 8); C.memmove(sres, marker, 8)
    stp = C.byref(st)
    assert f(ctx.handle, S, A, Mb, 32, None, 3, mi(*idx), rr, 6, res, stp, None, sst) == N.ERR_ARGUMENT                 # no set results
    assert f(ctx.handle, S, A, Mb, 32, None, 3, mi(*idx), None, 6, res, stp, sres, sst) == N.ERR_ARGUMENT               # no scalars
    assert f(ctx.handle, S, A, Mb, 32, None, 3, mi(*idx), rr, 6, None, stp, sres, sst) == N.ERR_ARGUMENT                # no result
    assert f(ctx.handle, S, A, Mb, 32, None, 3, mi(0, 1, 3, 1, 0, 1), rr, 6, res, stp, sres, sst) == N.ERR_ARGUMENT     # the host entries refuse an index outside the list
    assert f(ctx.handle, S, A, Mb, 0, (C.c_uint64 * 4)(0, 64, 32, 96), 3, mi(*idx), rr, 6, res, stp, sres, sst) == N.ERR_ARGUMENT      # ... and a backward range
    assert f(ctx.handle, S, A, Mb, 32, None, 3, None, rr, 6, res, stp, sres, sst) == N.ERR_ARGUMENT                     # no indices
    assert bytes(res)[:8] == marker and bytes(sres)[:8] == marker and st.value == 0xAAAA                                # nothing written
    assert f(ctx.handle, S, A, Mb, 32, None, 3, mi(*idx), rr, 0, res, stp, sres, sst) == 0                              # n = 0: true, no set to answer for
    assert bytes(res)[:8] == b"\x01" + marker[1:] and st.value == 0 and bytes(sres)[:8] == marker
    assert f(ctx.handle, S, A, Mb, 32, None, 3, mi(*idx), rr, 6, res, None, sres, None) == 0                            # both status outputs are optional
    assert bytes(res)[:1] == b"\x00" and bytes(sres)[:6] == b"\x01\x01\x01\x01\x00\x01"
    # the device form: NULL d_set_results is refused on the host and nothing is written; n = 0 is accepted
    d = DevCase(N, c)
    d_res, d_st, d_sres, d_sst = _bufs(8)
    fd = N.lib().mbls_verify_multiple_shared_msgs_locate_device
    head = (ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), d.list.data_ptr(), 32, None, 3, d.idx.data_ptr())
    assert fd(*head, d.rands.data_ptr(), 6, d_res.data_ptr(), d_st.data_ptr(), None, d_sst.data_ptr(), None) == N.ERR_ARGUMENT
    assert fd(*head, None, 6, d_res.data_ptr(), d_st.data_ptr(), d_sres.data_ptr(), d_sst.data_ptr(), None) == N.ERR_ARGUMENT
    assert fd(*head, d.rands.data_ptr(), 6, None, d_st.data_ptr(), d_sres.data_ptr(), d_sst.data_ptr(), None) == N.ERR_ARGUMENT
    tab = N.KeyTable()
    fi = N.lib().mbls_verify_multiple_sets_indexed_shared_msgs_locate_device
    assert fi(ctx.handle, tab.handle, d.sigs.data_ptr(), d.idx.data_ptr(), None, 1, d.list.data_ptr(), 32, None, 3, d.idx.data_ptr(), d.rands.data_ptr(), 6,
              d_res.data_ptr(), d_st.data_ptr(), None, None, None) == N.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert [int(x) for x in d_res.cpu().numpy()] == [7] * 8 and [int(x) for x in d_sres.cpu().numpy()] == [7] * 8 and int(d_st[0].item()) == -1
    assert fd(*head, d.rands.data_ptr(), 0, d_res.data_ptr(), d_st.data_ptr(), d_sres.data_ptr(), d_sst.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in d_res.cpu().numpy()] == [1] + [7] * 7 and int(d_st[0].item()) == 0 and [int(x) for x in d_sres.cpu().numpy()] == [7] * 8
    assert fd(*head, d.rands.data_ptr(), 6, d_res.data_ptr(), None, d_sres.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert int(d_res[0].item()) == 0 and [int(x) for x in d_sres.cpu().numpy()[:6]] == [1, 1, 1, 1, 0, 1]
    # two calls of different n and M back to back on one context, a non-locate shared call in between whose bytes do not change, in every mode; the reserved
    # workspace is the plan's
    want6 = (False, 0, [True, True, True, True, False, True], [0, 0, 0, 0, ST_PAIRING_FAILED, 0])
    big_listed = [rnd.randbytes(32) for _ in range(4)]
    big = plain_case(33, big_listed, [i % 4 for i in range(33)], 881)
    big.apks[32] = spare_key()
    want33 = (False, 0, [True] * 32 + [False], [0] * 32 + [ST_PAIRING_FAILED])
    args6 = (b"".join(c.sigs), b"".join(c.apks), b"".join(listed), 3, idx, c.rands, 6)
    args33 = (b"".join(big.sigs), b"".join(big.apks), b"".join(big_listed), 4, big.idx, big.rands, 33)
    assert N.plan_verify_multiple_shared_msgs_locate_workspace_items(6, 3, 1) == N.plan_verify_multiple_shared_msgs_workspace_items(6, 3, 1) + 12
    assert N.plan_verify_multiple_shared_msgs_locate_workspace_items(6, 3, 2) == N.plan_verify_multiple_shared_msgs_workspace_items(6, 3, 2) + 6
    for mode in MODES:
        batch.set_vm_grouping(mode, ctx)
        try:
            plain = batch.verify_multiple_shared_msgs(*args33)
            assert plain == (False, 0)
            for _ in range(2):
                assert batch.verify_multiple_shared_msgs_locate(*args6) == want6, mode
                assert batch.verify_multiple_shared_msgs(*args33) == plain, mode
                assert batch.verify_multiple_shared_msgs_locate(*args33) == want33, mode
                assert batch.verify_multiple_shared_msgs(*args6) == (False, 0), mode
        finally:
            batch.set_vm_grouping(0, ctx)
