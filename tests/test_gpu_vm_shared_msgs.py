"""GPU tests of mbls_verify_multiple*_shared_msgs (include/mbls.h, "verify_multiple OVER A SHARED MESSAGE LIST"): the sets' messages named by index in a list
that is hashed once, and -- grouped route -- one Miller loop per message over the per-message sums of the blinded keys. Every case is judged against the
ungrouped device entry (mbls_verify_multiple_aggregate_signatures_device) on the same sets with each set's message spelled out: equal result byte, equal
status word in the bits that reject a batch; where sizes allow, against the oracle with the same scalars too. Modes 1 (always grouped) and 2 (never) in every
case, mode 0 on each side of the auto condition."""
import ctypes as C
import random

import numpy as np
import pytest

import bls12_381 as M
import edge_points as E
import helpers
import orc

pytestmark = pytest.mark.gpu

G1_INF_U = bytes([0x40]) + bytes(95)
REJECT_BATCH = 0x01 | 0x02 | 0x04 | 0x100 | 0x80          # the bits that reject a verify_multiple batch (mbls_coop.h COOP_REJECT_BATCH)
ST_BAD_MSG_RANGE, ST_BAD_SCALAR, ST_SIG_NOT_IN_G2, ST_BAD_SIG_ENCODING = 0x100, 0x80, 0x02, 0x01
DEFECTS = ("wrong_key", "swapped_sig", "inf_sig", "inf_key", "both_inf", "not_in_g2", "undecodable", "zero_scalar")
N_SETS = 150


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
    """n sets over a list: sigs / apks / wire (two keys per set) / rands per set, `listed` messages and idx per set"""

    def spelled(self):
        return [self.listed[j] for j in self.idx]


class DevCase:
    def __init__(self, c, N=None, table=None):
        self.n, self.n_msgs = len(c.sigs), len(c.listed)
        self.sigs = _dev(b"".join(c.sigs)); self.apks = _dev(b"".join(c.apks)); self.rands = _dev(np.array(c.rands, dtype=np.uint64))
        self.list = _dev(b"".join(c.listed)); self.list_off = _dev(np.array(_offsets(c.listed), dtype=np.uint64))
        self.idx = _dev(np.array(c.idx, dtype=np.uint32))
        sp = c.spelled()
        self.msgs = _dev(b"".join(sp)); self.moff = _dev(np.array(_offsets(sp), dtype=np.uint64))
        self.key_idx = None
        if table is not None:
            first, errs = table.append(b"".join(k for w in c.wire for k in w), 2 * self.n, pk_format=N.PK_UNCOMPRESSED, validate=False)
            self.key_idx = _dev(np.arange(first, first + 2 * self.n, dtype=np.uint32))
            self.table = table


def _out():
    import torch
    return torch.full((8,), 7, dtype=torch.uint8, device="cuda:0"), torch.full((2,), -1, dtype=torch.int32, device="cuda:0")


def _read(res, st):
    import torch
    torch.cuda.synchronize()
    return int(res[0].item()), int(st[0].item()) & 0xFFFFFFFF


def run_ungrouped(N, d):
    """the existing entry on the spelled-out messages (offset table: messages of any length)"""
    ctx = N.default_context()
    res, st = _out()
    rc = N.lib().mbls_verify_multiple_aggregate_signatures_device(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), d.msgs.data_ptr(), 0, d.moff.data_ptr(),
                                                                  d.rands.data_ptr(), d.n, res.data_ptr(), st.data_ptr(), None)
    assert rc == 0, ctx.last_error()
    return _read(res, st)


def run_shared(N, d, mode, indexed=False, n_msgs=None, idx=None, list_off=None):
    from milagro_bls_amd import batch
    ctx = N.default_context()
    batch.set_vm_grouping(mode, ctx)
    res, st = _out()
    n_msgs = d.n_msgs if n_msgs is None else n_msgs
    idx = d.idx if idx is None else idx
    list_off = d.list_off if list_off is None else list_off
    if indexed:
        batch.verify_multiple_sets_indexed_shared_msgs_device(d.table, d.sigs.data_ptr(), d.key_idx.data_ptr(), d.list.data_ptr(), n_msgs, idx.data_ptr(), d.rands.data_ptr(),
                                                              d.n, res.data_ptr(), st.data_ptr(), k=2, msg_len=0, d_msg_offsets=list_off.data_ptr(), ctx=ctx)
    else:
        batch.verify_multiple_shared_msgs_device(d.sigs.data_ptr(), d.apks.data_ptr(), d.list.data_ptr(), n_msgs, idx.data_ptr(), d.rands.data_ptr(), d.n, res.data_ptr(),
                                                 st.data_ptr(), msg_len=0, d_msg_offsets=list_off.data_ptr(), ctx=ctx)
    out = _read(res, st)
    batch.set_vm_grouping(0, ctx)
    return out


# ------------------------------------------------------------------------------------------------ the oracle-judged mix
# (messages in the list, ragged lengths, unused entries at the end); variant t carries defect t % 8 and is also run valid
VARIANTS = [(1, False, 0), (2, False, 0), (7, False, 0), (N_SETS, False, 0), (N_SETS, False, 3), (1, True, 0), (2, True, 0), (7, True, 0), (N_SETS, True, 0), (N_SETS, True, 3)]
_MIX = {}


def _keys(seed):
    """the sets' keys and secrets, once per module: two keys per set (apk = pk1 + pk2 = table entries 2 i, 2 i + 1)"""
    if "keys" not in _MIX:
        rnd = random.Random(seed)
        sks = [(rnd.randrange(1, helpers.R), rnd.randrange(1, helpers.R)) for _ in range(N_SETS)]
        pk96 = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for pair in sks for s in pair), 2 * N_SETS, 1, nthreads=8)
        wire = [[pk96[192 * i:192 * i + 96], pk96[192 * i + 96:192 * i + 192]] for i in range(N_SETS)]
        _MIX["keys"] = (sks, wire, [orc.g1_add(w[0], w[1]) for w in wire])
    return _MIX["keys"]


def _oracle(c):
    if any(r == 0 for r in c.rands):
        return False                          # the reference never draws a zero (src/aggregates.rs:280-287); the ABI rejects it
    dec = [orc.g2_from_compressed(s) for s in c.sigs]
    if any(e for e, _ in dec):
        return False
    return orc.verify_multiple([(d[1], a, mm) for d, a, mm in zip(dec, c.apks, c.spelled())], c.rands)


def build_variant(t, probe):
    """-> (valid case, defective case, defect name), each with the oracle's answer in .want"""
    if t in _MIX:
        return _MIX[t]
    used, ragged, unused = VARIANTS[t]
    rnd = random.Random(3100 + t)
    sks, wire, apks = _keys(3000)
    n = N_SETS
    lens = [0, 1, 31, 32, 33, 55, 56, 64, 65, 100, 200]
    listed = [rnd.randbytes(lens[j % len(lens)] if ragged else 32) for j in range(used + unused)]
    idx = list(range(used)) + [rnd.randrange(used) for _ in range(n - used)]        # every one of the first `used` entries is named; `unused` more are not
    rnd.shuffle(idx)
    c = Case()
    c.listed, c.idx = listed, idx
    c.sigs = [orc.g2_compress(orc.sign(listed[j], (a + b) % helpers.R)) for j, (a, b) in zip(idx, sks)]
    c.apks, c.wire, c.rands = list(apks), [list(w) for w in wire], [rnd.randrange(1, 1 << 63) for _ in range(n)]
    c.want = _oracle(c)
    b = Case()
    b.listed, b.idx, b.sigs, b.apks, b.wire, b.rands = listed, idx, list(c.sigs), list(c.apks), [list(w) for w in c.wire], list(c.rands)
    kind = DEFECTS[t % len(DEFECTS)]
    i = rnd.randrange(n); other = (i + 1) % n
    if kind == "wrong_key":
        b.apks[i], b.wire[i] = b.apks[other], list(b.wire[other])
    elif kind == "swapped_sig":
        b.sigs[i] = b.sigs[other]
    elif kind == "inf_sig":
        b.sigs[i] = helpers.G2_INF
    elif kind == "inf_key":
        b.apks[i] = G1_INF_U; b.wire[i] = [b.wire[i][0], orc.g1_mul(b.wire[i][0], helpers.R - 1)]
    elif kind == "both_inf":
        b.sigs[i] = helpers.G2_INF; b.apks[i] = G1_INF_U; b.wire[i] = [b.wire[i][0], orc.g1_mul(b.wire[i][0], helpers.R - 1)]
    elif kind == "not_in_g2":
        b.sigs[i] = probe
    elif kind == "undecodable":
        b.sigs[i] = bytes([b.sigs[i][0] & 0x7F]) + b.sigs[i][1:]
    elif kind == "zero_scalar":
        b.rands[i] = 0
    b.want = _oracle(b)
    _MIX[t] = (c, b, kind)
    return _MIX[t]


@pytest.mark.usefixtures("engine")
@pytest.mark.parametrize("t", range(len(VARIANTS)), ids=["%dmsgs%s%s" % (u, "-ragged" if r else "", "+%d" % x if x else "") for u, r, x in VARIANTS])
def test_mix_vs_oracle_and_ungrouped_entry(N, vectors, t):
    """150 sets over 1, 2, 7, n and n + 3 (three unused) listed messages, 32-byte and ragged (the empty message included), valid and with one defect: both key
    forms in modes 1 and 2 give the oracle's bool, the ungrouped entry's result byte and its status word in the rejecting bits; mode 0 takes the route its
    condition names and gives the same"""
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    good, bad, kind = build_variant(t, probe)
    assert good.want is True and bad.want == (kind == "both_inf"), (kind, good.want, bad.want)
    for c in (good, bad):
        d = DevCase(c, N, N.KeyTable())
        r0, s0 = run_ungrouped(N, d)
        assert r0 == int(c.want), (kind, r0)
        for mode in (1, 2, 0):
            for indexed in ((False, True) if mode else (False,)):
                r, s = run_shared(N, d, mode, indexed)
                assert r == r0, (kind, mode, indexed, r, hex(s), hex(s0))
                assert s & REJECT_BATCH == s0 & REJECT_BATCH, (kind, mode, indexed, hex(s), hex(s0))
    plan = N.plan_verify_multiple_shared_msgs(N_SETS, len(good.listed), 0)
    assert plan["route"] == (N.VM_ROUTE_GROUPED if 2 * len(good.listed) <= N_SETS else N.VM_ROUTE_PER_SET)
    if c is bad and kind in ("not_in_g2", "undecodable", "zero_scalar"):
        assert s0 & {"not_in_g2": ST_SIG_NOT_IN_G2, "undecodable": ST_BAD_SIG_ENCODING, "zero_scalar": ST_BAD_SCALAR}[kind]


def test_host_entry_and_two_equal_list_entries(N, vectors):
    """the host entry returns the device entry's bool and status; a list that holds the same bytes twice is two groups and changes nothing"""
    from milagro_bls_amd import batch
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    good, bad, kind = build_variant(2, probe)
    for c in (good, bad):
        for mode in (1, 2):
            batch.set_vm_grouping(mode)
            r, s = batch.verify_multiple_shared_msgs(b"".join(c.sigs), b"".join(c.apks), b"".join(c.listed), len(c.listed), c.idx, c.rands, len(c.sigs), msg_len=32)
            assert r == c.want and bool(s & REJECT_BATCH) == (kind in ("not_in_g2", "undecodable", "zero_scalar") and c is bad)
            # entry 0 repeated at the end of the list, half of its sets renamed to the copy
            twice = c.listed + [c.listed[0]]
            seen, idx2 = 0, []
            for j in c.idx:
                if j == 0:
                    seen += 1
                idx2.append(len(c.listed) if (j == 0 and seen % 2) else j)
            assert len(c.listed) in idx2 and 0 in idx2
            r2, s2 = batch.verify_multiple_shared_msgs(b"".join(c.sigs), b"".join(c.apks), b"".join(twice), len(twice), idx2, c.rands, len(c.sigs), msg_len=32)
            assert (r2, s2) == (r, s)
    batch.set_vm_grouping(0)
    assert batch.verify_multiple_shared_msgs(b"", b"", b"", 0, [], [], 0) == (True, 0)


# ------------------------------------------------------------------------------------------------ coincident points inside a group
def _coincidence_case(n):
    """n sets drawn from tests/edge_points.py's pool -- one scalar per pool entry, every base set also as its negation and torsion-shifted, and per torsion point
    (orders 3 and 11, the two x = 0 points included) the pure-torsion set --, a fifth of them pure-torsion sets, over the pool's handful of messages"""
    key = ("coinc", n)
    if key in _MIX:
        return _MIX[key]
    pool = E.vm_pool()
    sigs, apks, msgs, rands = E.vm_coincidence_batch(random.Random(9100 + n), n, pool, torsion_share=0.2)
    c = Case()
    c.listed = list(dict.fromkeys(msgs))
    c.idx = [c.listed.index(m) for m in msgs]
    c.sigs, c.apks, c.rands, c.wire = sigs, apks, rands, None
    _MIX[key] = c
    return c


def g1_tree_case_census(c):
    """the cases the per-message key sums meet for the in-group order 'sets in the caller's order' (the GPU's order inside a group is free: this is a property of
    the INPUT -- which operands a group offers --, not of the run): per group, vmb_takes_partner's levels over the blinded keys [r_i] apk_i -> Counter over E.CASES"""
    from collections import Counter
    memo, census = {}, Counter()
    for g in range(len(c.listed)):
        pts = []
        for i, j in enumerate(c.idx):
            if j == g:
                k = (c.apks[i], c.rands[i])
                if k not in memo:
                    memo[k] = M.g1_mul(E.g1_point(c.apks[i]), c.rands[i])
                pts.append(memo[k])
        half = 1
        while half < len(pts):
            for p in range(0, len(pts) - half, 2 * half):
                a, b = pts[p], pts[p + half]
                census[E._classify(M.g1_add, a, b)] += 1
                pts[p] = M.g1_add(a, b)
            half *= 2
    return census


@pytest.mark.usefixtures("engine")
def test_coincident_points_inside_a_group(N):
    """a few hundred sets over the pool's handful of messages: equal, opposite and infinite partners meet in the levels of k_g1_seg_tree_d (asserted by the CPU
    census of the input); same result byte and rejecting bits as the ungrouped entry, for the batch as drawn (true) and with one set's message spoiled (false)"""
    n = 300
    c = _coincidence_case(n)
    assert len(c.listed) <= 8
    census = g1_tree_case_census(c)
    assert all(census[k] > 0 for k in E.CASES), census
    if "want" not in c.__dict__:
        c.want = E.oracle_verify_multiple((c.sigs, c.apks, c.spelled(), c.rands), nthreads=8)
    assert c.want is True
    d = DevCase(c)
    r0, s0 = run_ungrouped(N, d)
    assert r0 == 1
    for mode in (1, 2):
        r, s = run_shared(N, d, mode)
        assert (r, s & REJECT_BATCH) == (r0, s0 & REJECT_BATCH), (mode, r, hex(s))
    # one honest set renamed to another message of the list: false on both routes
    i = next(i for i in range(n // 3, n) if c.sigs[i] != helpers.G2_INF)
    b = Case()
    b.listed, b.sigs, b.apks, b.rands, b.wire = c.listed, c.sigs, c.apks, c.rands, None
    b.idx = list(c.idx); b.idx[i] = (c.idx[i] + 1) % len(c.listed)
    d = DevCase(b)
    r0, s0 = run_ungrouped(N, d)
    assert r0 == 0
    for mode in (1, 2):
        r, s = run_shared(N, d, mode)
        assert (r, s & REJECT_BATCH) == (r0, s0 & REJECT_BATCH), (mode, r, hex(s))


# ------------------------------------------------------------------------------------------------ bad indices and ranges
def test_bad_indices_and_ranges(N, vectors):
    """device entries: an index >= n_msgs and n_msgs = 0 reject with MBLS_ST_BAD_MSG_RANGE, a listed range that runs backwards rejects exactly when a set names
    it; host entries refuse both with MBLS_ERR_ARGUMENT and leave the outputs untouched"""
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    good, _bad, _kind = build_variant(2, probe)                  # 7 messages of 32 bytes
    d = DevCase(good)
    n, Mn = d.n, d.n_msgs
    for mode in (1, 2):
        assert run_shared(N, d, mode)[0] == 1
        idx = list(good.idx); idx[17] = Mn
        r, s = run_shared(N, d, mode, idx=_dev(np.array(idx, dtype=np.uint32)))
        assert r == 0 and s & ST_BAD_MSG_RANGE, (mode, r, hex(s))
        idx[17] = 0xFFFFFFFF
        r, s = run_shared(N, d, mode, idx=_dev(np.array(idx, dtype=np.uint32)))
        assert r == 0 and s & ST_BAD_MSG_RANGE, (mode, r, hex(s))
        r, s = run_shared(N, d, mode, n_msgs=0)
        assert r == 0 and s & ST_BAD_MSG_RANGE, (mode, r, hex(s))
        # an eighth entry whose range runs backwards (and one whose length would be 2^32): unnamed -> harmless; named by one set -> rejects
        off = _offsets(good.listed)
        back = _dev(np.array(off + [off[-1] - 5], dtype=np.uint64)); huge = _dev(np.array(off + [off[-1] + (1 << 32)], dtype=np.uint64))
        for lo in (back, huge):
            r, s = run_shared(N, d, mode, n_msgs=Mn + 1, list_off=lo)
            assert r == 1 and not s & REJECT_BATCH, (mode, r, hex(s))
            idx = list(good.idx); idx[40] = Mn
            r, s = run_shared(N, d, mode, n_msgs=Mn + 1, list_off=lo, idx=_dev(np.array(idx, dtype=np.uint32)))
            assert r == 0 and s & ST_BAD_MSG_RANGE, (mode, r, hex(s))
    # host entries
    ctx = N.default_context()
    S, A, L = N.cbuf(b"".join(good.sigs)), N.cbuf(b"".join(good.apks)), N.cbuf(b"".join(good.listed))
    rr = (C.c_uint64 * n)(*good.rands)
    ix = lambda v: (C.c_uint32 * n)(*v)
    res = N.outbuf(1); res[0] = 9
    st = C.c_uint32(0xABCD)
    f = N.lib().mbls_verify_multiple_shared_msgs
    bad_idx = list(good.idx); bad_idx[3] = Mn
    off = _offsets(good.listed); off[3] = off[4] + 1
    assert f(ctx.handle, S, A, L, 32, None, Mn, ix(bad_idx), rr, n, res, C.byref(st)) == N.ERR_ARGUMENT
    assert f(ctx.handle, S, A, L, 32, None, 0, ix(good.idx), rr, n, res, C.byref(st)) == N.ERR_ARGUMENT
    assert f(ctx.handle, S, A, L, 0, (C.c_uint64 * len(off))(*off), Mn, ix(good.idx), rr, n, res, C.byref(st)) == N.ERR_ARGUMENT
    assert f(ctx.handle, S, A, L, 32, None, Mn, ix(good.idx), None, n, res, C.byref(st)) == N.ERR_ARGUMENT       # no scalars
    cb = N.SCALAR_SOURCE(lambda _u, out, count: [out.__setitem__(i, good.rands[i]) for i in range(count)] and None)
    g = N.lib().mbls_verify_multiple_shared_msgs_rng
    assert g(ctx.handle, S, A, L, 32, None, Mn, ix(bad_idx), n, res, cb, None) == N.ERR_ARGUMENT
    assert g(ctx.handle, S, A, L, 32, None, Mn, ix(good.idx), n, res, N.SCALAR_SOURCE(0), None) == N.ERR_ARGUMENT
    assert res[0] == 9 and st.value == 0xABCD
    assert f(ctx.handle, S, A, L, 32, None, Mn, ix(good.idx), rr, n, res, C.byref(st)) == 0 and res[0] == 1 and st.value == 0
    # device entries without scalars are refused; n = 0 gives result 1 and status 0
    import torch
    r_, s_ = _out()
    fd = N.lib().mbls_verify_multiple_shared_msgs_device
    assert fd(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), d.list.data_ptr(), 32, None, Mn, d.idx.data_ptr(), None, n, r_.data_ptr(), s_.data_ptr(), None) == N.ERR_ARGUMENT
    assert fd(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), d.list.data_ptr(), 32, None, Mn, d.idx.data_ptr(), d.rands.data_ptr(), 0, r_.data_ptr(), s_.data_ptr(), None) == 0
    assert _read(r_, s_) == (1, 0)
    assert N.lib().mbls_ctx_set_vm_grouping(ctx.handle, 3) == N.ERR_ARGUMENT


# ------------------------------------------------------------------------------------------------ the reference's RNG order
@pytest.mark.parametrize("mode", [1, 2])
def test_rng_order_matches_verify_multiple(N, vectors, mode):
    """the _rng entry and the Python mirror against AggregateSignature.verify_multiple_aggregate_signatures: same bool, the generator left in the same state (as
    many bytes drawn), with a signature outside G2 first, in the middle, last, and nowhere"""
    from milagro_bls_amd import batch
    from milagro_bls_amd.api import AggregateSignature, AggregatePublicKey
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    good, _bad, _kind = build_variant(2, probe)
    n = 40
    sigs, apks, idx = good.sigs[:n], good.apks[:n], good.idx[:n]
    batch.set_vm_grouping(mode)
    try:
        for where in (None, 0, n // 2, n - 1):
            s = list(sigs)
            if where is not None:
                s[where] = probe
            sets = [(AggregateSignature(s[i]), AggregatePublicKey(apks[i]), good.listed[idx[i]]) for i in range(n)]
            r1, r2 = random.Random(777), random.Random(777)
            want = AggregateSignature.verify_multiple_aggregate_signatures(r1, sets)
            got = AggregateSignature.verify_multiple_aggregate_signatures_shared_msgs(r2, sets)
            assert got == want == (where is None), where
            assert r1.getstate() == r2.getstate(), where
            asked = []

            def draw(count):
                asked.append(count)
                return good.rands[:count]
            got = batch.verify_multiple_shared_msgs_rng(b"".join(s), b"".join(apks), b"".join(good.listed), len(good.listed), idx, n, draw, msg_len=32)
            assert got == (where is None) and asked == ([n if where is None else where] if where != 0 else []), (where, asked)
        assert AggregateSignature.verify_multiple_aggregate_signatures_shared_msgs(random.Random(1), []) is True
    finally:
        batch.set_vm_grouping(0)


# ------------------------------------------------------------------------------------------------ routing at scale, no oracle
SCALE = [("just above a round, 3 messages", 70, 3), ("two rounds + 1, 3 messages", 129, 3), ("above a round, n / 2 messages", 70, 35), ("one group holds every set", 70, 1)]


@pytest.mark.usefixtures("engine")
@pytest.mark.parametrize("name,n,n_msgs", SCALE, ids=[s[0] for s in SCALE])
def test_routing_at_scale_with_a_small_round(N, vectors, name, n, n_msgs):
    """the round shrunk to 64 items (the smallest mbls_ctx_set_round_items accepts): the per-set chains and, with 35 messages, the Miller phase cross a round;
    valid and with one swapped signature, modes 1 and 2 against the ungrouped entry under the same round"""
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    good, _bad, _kind = build_variant(3, probe)                  # 150 sets, each with a message of its own
    ctx = N.default_context()
    assert N.lib().mbls_ctx_set_round_items(ctx.handle, 32) == N.ERR_ARGUMENT
    ctx.set_round_items(64)
    try:
        rnd = random.Random(n * 1000 + n_msgs)
        sks, _wire, _apks = _keys(3000)
        c = Case()
        c.listed = [rnd.randbytes(32) for _ in range(n_msgs)]
        c.idx = list(range(n_msgs)) + [rnd.randrange(n_msgs) for _ in range(n - n_msgs)]
        c.sigs = [orc.g2_compress(orc.sign(c.listed[j], (a + b) % helpers.R)) for j, (a, b) in zip(c.idx, sks[:n])]
        c.apks, c.rands, c.wire = good.apks[:n], [rnd.randrange(1, 1 << 64) for _ in range(n)], None
        for spoil in (False, True):
            if spoil:
                c.sigs[n - 2] = c.sigs[n - 1]                 # another set's signature (another key): false whatever the messages are
            d = DevCase(c)
            r0, s0 = run_ungrouped(N, d)
            assert r0 == (0 if spoil else 1), (name, spoil)
            for mode in (1, 2):
                r, s = run_shared(N, d, mode)
                assert (r, s & REJECT_BATCH) == (r0, s0 & REJECT_BATCH), (name, spoil, mode, r, hex(s))
    finally:
        ctx.reset_tuning()


def test_determinism(N, vectors):
    """the order inside a group follows the atomics and is free; result and status are not: five runs of one call agree"""
    c = _coincidence_case(300)
    d = DevCase(c)
    outs = {run_shared(N, d, 1) for _ in range(5)}
    assert len(outs) == 1 and next(iter(outs))[0] == 1, outs
