"""GPU checks of the verification stream over a committee table and a message table (include/mbls.h, mbls_stream_create_committee /
mbls_stream_submit_committee[_device]; milagro_bls_amd/stream.py, VerifyStream(committees=, msg_table=, bits_stride=)): every call's results, status words and
bitmap equal a direct call of mbls_fast_aggregate_verify_batch_committee_msgtable_device on the same signatures, indices and ids with every field zero-extended
to the stream's stride by numpy -- byte for byte, however the stream packed and split the call, whatever bits_len and alignment the call's fields had. One world of
about 150 keys, seven committees (1, 7, 64, 65, 127, 128 and 130 members: a field ends on a dword, just past one, or mid-dword), 32 table entries and a pool of
signed items is built once per module."""
import random
import threading

import numpy as np
import pytest

import bls12_381 as M
from milagro_bls_amd import _native as N
from milagro_bls_amd.stream import VerifyStream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
NK = 150
SIZES = (1, 7, 64, 65, 127, 128, 130)
STRIDE = 20                                                      # 160 bits cover the largest committee
N_MSGS, N_ENTRIES = 4, 32                                        # table entry j holds message j % 4
GUARD, GUARD_BYTE = 0x5A5A5A5A5A5A5A5A, 0xC3
NO_KEYS, BAD_PK, PAIRING, BAD_MSG = 0x10, 0x04, 0x40, 0x100


class World:
    pass


@pytest.fixture(scope="module")
def world():
    from milagro_bls_amd import batch
    ctx = N.default_context()
    rnd = random.Random(950)
    w = World(); w.ctx = ctx
    sks = [rnd.randrange(1, M.R) for _ in range(NK)]
    pk96 = batch.sk_to_pk_batch(b"".join(s.to_bytes(32, "big") for s in sks), NK, out_format=N.PK_UNCOMPRESSED)
    w.kt = N.KeyTable(ctx, capacity_hint=256)
    first, errs = w.kt.append(pk96, NK, pk_format=N.PK_UNCOMPRESSED, validate=False)
    assert first == 0 and not any(errs)
    w.msgs = [rnd.randbytes(32) for _ in range(N_MSGS)]
    w.mt = N.MsgTable(ctx, capacity_hint=64)
    assert w.mt.append(b"".join(w.msgs[j % N_MSGS] for j in range(N_ENTRIES)), N_ENTRIES, msg_len=32) == 0
    w.members = [[(5 * c + 3 * j) % NK for j in range(m)] for c, m in enumerate(SIZES)]
    w.ct = N.CommitteeTable(w.kt, capacity_hint=4)
    off = [0]
    for mem in w.members:
        off.append(off[-1] + len(mem))
    assert w.ct.append([x for mem in w.members for x in mem], off) == 0 and w.ct.max_members == 130
    # the pool: per committee an almost full field (complement route), one near 30 % (direct), the full, the empty and a one-member field
    pool = []
    for c, m in enumerate(SIZES):
        near99 = sorted(set(range(m)) - {rnd.randrange(m)}) if m > 1 else [0]
        near30 = sorted(rnd.sample(range(m), max(1, (3 * m) // 10)))
        for tag, sel in (("near99", near99), ("near30", near30), ("all", list(range(m))), ("empty", []), ("last", [m - 1])):
            for e in (c, c + 9):
                pool.append(dict(cid=c, sel=sel, entry=e, tag=tag))
    one = batch.sign_batch(b"".join(sks[i].to_bytes(32, "big") for _ in range(N_MSGS) for i in range(NK)), b"".join(w.msgs[j] for j in range(N_MSGS) for _ in range(NK)),
                           N_MSGS * NK, msg_len=32)
    sig_of = lambda key, msg: one[96 * (msg * NK + key):96 * (msg * NK + key) + 96]
    parts, off = [], [0]
    for it in pool:
        signers = [w.members[it["cid"]][j] for j in it["sel"]] or [0]
        parts += [sig_of(k, it["entry"] % N_MSGS) for k in signers]
        off.append(len(parts))
    agg, errs = batch.aggregate_signatures_batch(b"".join(parts), len(pool), offsets=off)
    assert not any(errs)
    w.pool = pool
    w.sig = np.frombuffer(agg, dtype=np.uint8).reshape(len(pool), 96).copy()
    w.midx = np.array([it["entry"] for it in pool], dtype=np.uint32)
    w.cid = np.array([it["cid"] for it in pool], dtype=np.uint32)
    w.bits = np.zeros((len(pool), STRIDE), dtype=np.uint8)
    for i, it in enumerate(pool):
        for j in it["sel"]:
            w.bits[i, j >> 3] |= 1 << (j & 7)
    w.small = [i for i, it in enumerate(pool) if SIZES[it["cid"]] <= 24]
    yield w
    ctx.set_committee_route(0)
    w.ct.close(); w.mt.close(); w.kt.close()


class Arrays:
    """the four arrays of a call, the fields at the full stride"""

    def __init__(self, w, picks):
        picks = np.asarray(picks)
        self.n = len(picks)
        self.sig, self.midx, self.cid, self.bits = w.sig[picks].copy(), w.midx[picks].copy(), w.cid[picks].copy(), w.bits[picks].copy()


def picks_of(w, n, start=0, step=9, among=None):
    among = list(range(len(w.pool))) if among is None else among
    return [among[(start + step * i) % len(among)] for i in range(n)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def direct(w, a, bits_len):
    """the direct device entry on the call's arrays with every field cut to bits_len bytes and zero-extended to the stride -> (results, status, bitmap) on the host"""
    b = a.bits.copy(); b[:, bits_len:] = 0
    d_s, d_mi, d_ci, d_b = dev(a.sig), dev(a.midx), dev(a.cid), dev(b)
    res = torch.zeros(a.n, dtype=torch.uint8, device=DEV); st = torch.zeros(a.n, dtype=torch.int32, device=DEV)
    bm = torch.zeros((a.n + 63) // 64, dtype=torch.int64, device=DEV)
    w.ctx.check(N.lib().mbls_fast_aggregate_verify_batch_committee_msgtable_device(w.ctx.handle, w.ct.handle, d_s.data_ptr(), w.mt.handle, d_mi.data_ptr(), d_ci.data_ptr(),
                                                                                   d_b.data_ptr(), STRIDE, a.n, res.data_ptr(), bm.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()
    return res.cpu(), st.cpu(), bm.cpu()


class Call:
    """one device call's output buffers: results between guard bytes, status words and bitmap between guard words"""

    def __init__(self, n):
        self.n = n
        self.res_all = torch.full((n + 32,), GUARD_BYTE, dtype=torch.uint8, device=DEV); self.res = self.res_all[16:16 + n]
        self.st_all = torch.full((n + 8,), 0x6B6B6B6B, dtype=torch.int32, device=DEV); self.st = self.st_all[4:4 + n]
        self.bm_all = torch.full(((n + 63) // 64 + 2,), GUARD, dtype=torch.int64, device=DEV); self.bm = self.bm_all[1:-1]

    def check(self, want):
        res, st, bm = want
        r, s, b = self.res_all.cpu(), self.st_all.cpu(), self.bm_all.cpu()
        assert torch.equal(r[16:16 + self.n], res) and torch.equal(s[4:4 + self.n], st) and torch.equal(b[1:-1], bm)
        assert bool((r[:16] == GUARD_BYTE).all()) and bool((r[16 + self.n:] == GUARD_BYTE).all()), "result bytes outside the call were touched"
        assert bool((s[:4] == 0x6B6B6B6B).all()) and bool((s[4 + self.n:] == 0x6B6B6B6B).all()), "status words outside the call were touched"
        assert int(b[0]) == GUARD and int(b[-1]) == GUARD, "bitmap words outside the call were touched"


def submit(vs, a, bits_len, host, skew=1):
    """the call with its fields cut to bits_len bytes back to back; a device call's fields start `skew` bytes into an allocation -> wait-and-check function"""
    fields = np.ascontiguousarray(a.bits[:, :bits_len])
    if host:
        h = vs.submit_committee(a.sig, a.midx, a.cid, fields, bits_len, a.n)
        return lambda want: _check_host(h, want)
    d_s, d_mi, d_ci = dev(a.sig), dev(a.midx), dev(a.cid)
    d_b = torch.zeros(a.n * bits_len + skew + 3, dtype=torch.uint8, device=DEV)
    d_b[skew:skew + a.n * bits_len] = dev(fields)
    assert (d_b.data_ptr() + skew) % 4 == skew % 4
    torch.cuda.synchronize()
    c = Call(a.n)
    t = vs.submit_committee_device(d_s, d_mi, d_ci, d_b.data_ptr() + skew, bits_len, a.n, c.res, bitmap=c.bm, status=c.st)
    keep = (d_s, d_mi, d_ci, d_b)
    return lambda want: (vs.wait(t), torch.cuda.synchronize(), c.check(want), keep)


def _check_host(h, want):
    res, st = h.result()
    assert res == bytes(want[0].tolist()) and [x & 0xffffffff for x in st] == [x & 0xffffffff for x in want[1].tolist()]


def make_stream(w, **kw):
    kw.setdefault("round_items", 256)
    return VerifyStream(w.ctx, committees=w.ct, msg_table=w.mt, bits_stride=STRIDE, **kw)


@pytest.fixture(autouse=True)
def _route_back():
    yield
    N.default_context().set_committee_route(0)


@pytest.mark.usefixtures("engine")
def test_calls_of_1_100_300_and_55_items_with_mixed_field_lengths(world):
    w = world
    sizes, lens = (1, 100, 300, 55), (17, 16, 3, 20)
    calls = [Arrays(w, picks_of(w, n, start=11 * j, step=9 if j != 2 else 3)) for j, n in enumerate(sizes)]
    big = calls[1]
    tags = [w.pool[p]["tag"] for p in picks_of(w, 100, start=11, step=9)]
    first = lambda tag: next(i for i, t in enumerate(tags) if t == tag and i not in (5, 6) and 0 < big.cid[i] < 6)   # (a committee of more than one member that 128 bits hold)
    i99, i30, iempty, flip = first("near99"), first("near30"), first("empty"), first("all")
    big.bits[flip, 0] ^= 1                                      # one flipped bit: rejected
    big.cid[5] = len(w.ct)                                      # an id equal to the count
    big.midx[6] = len(w.mt)                                     # a message index equal to the size
    wants = [direct(w, a, L) for a, L in zip(calls, lens)]
    res, st, _ = wants[1]
    assert not res[flip] and int(st[flip]) == PAIRING
    assert not res[5] and int(st[5]) & BAD_PK and not res[6] and int(st[6]) & BAD_MSG
    assert not res[iempty] and int(st[iempty]) & NO_KEYS
    for i in (i99, i30):
        assert res[i] and int(st[i]) == 0, (i, tags[i])
    assert int(res.sum()) >= 40
    # bits_len = 3: a field shorter than its committee selects nobody beyond bit 23 -- a signature by the whole selection no longer verifies
    short = [i for i in range(300) if SIZES[calls[2].cid[i]] > 24 and calls[2].bits[i, 3:].any()]
    assert short and not any(bool(wants[2][0][i]) for i in short) and int(wants[2][0].sum()) > 0
    with make_stream(w, policy=N.STREAM_FULL_ROUNDS) as vs:
        checks = [submit(vs, a, L, host=(j % 2 == 1)) for j, (a, L) in enumerate(zip(calls, lens))]
        vs.flush()
        for chk, want in zip(checks, wants):
            chk(want)
        stats = vs.stats()
        shapes = [dict(n=n, k=0, msg_len=4) for n in sizes]; shapes[-1]["flush_after"] = 1
        pieces = N.stream_cut(shapes, 256, 128 * 256, 4 * 256)
        assert stats["calls"] == 4 and stats["items"] == sum(sizes) and stats["pieces"] == len(pieces) == 5 and stats["split_calls"] == 1
        assert stats["rounds"] == len({pc["round"] for pc in pieces}) == 2 and stats["full_rounds"] == 1
        assert stats["gathered_bytes"] == sum(n * (96 + 4 + 4 + L) for n, L in zip(sizes, lens))


@pytest.mark.usefixtures("engine")
def test_the_three_route_modes(world):
    w = world
    a = Arrays(w, picks_of(w, 64, start=2, step=3))
    outs = []
    with make_stream(w) as vs:
        for mode in (0, 1, 2):
            w.ctx.set_committee_route(mode)
            want = direct(w, a, 17)
            submit(vs, a, 17, host=False)(want)
            submit(vs, a, 17, host=True)(want)
            outs.append(want)
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(o, outs[0]))
    assert 20 <= int(outs[0][0].sum()) < 64


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.usefixtures("engine")
def test_no_stale_bits(world, host):
    """depth = 1: two slots, so the third round stages into the first round's slot. All-ones fields of the whole stride, then the true fields at 3 bytes, then at 16:
    each round equals its direct call. Then the same over committees larger than the short field, where a byte left over from the all-ones round would select
    members the zero-extended field does not."""
    w = world
    small = Arrays(w, picks_of(w, 64, among=w.small, step=1))
    ones = Arrays(w, picks_of(w, 64, among=w.small, step=1)); ones.bits[:] = 0xFF
    wide = Arrays(w, picks_of(w, 64, start=20, step=3))
    wide_ones = Arrays(w, picks_of(w, 64, start=20, step=3)); wide_ones.bits[:] = 0xFF
    assert int(direct(w, small, 3)[0].sum()) >= 30
    with make_stream(w, depth=1, policy=N.STREAM_FULL_ROUNDS) as vs:
        for a, L in ((ones, 20), (small, 3), (small, 16), (wide_ones, 20), (wide_ones, 20), (wide, 3), (wide, 16)):
            chk = submit(vs, a, L, host=host)
            vs.flush()
            chk(direct(w, a, L))
        assert vs.stats()["rounds"] == 7


@pytest.mark.usefixtures("engine")
def test_a_gather_tile_boundary_inside_one_piece(world):
    w = world
    a = Arrays(w, picks_of(w, 300, start=1, step=11))
    want = direct(w, a, 17)
    with make_stream(w, round_items=512, policy=N.STREAM_FULL_ROUNDS) as vs:
        chk = submit(vs, a, 17, host=False)
        vs.flush()
        chk(want)
        assert vs.stats()["pieces"] == 1 and vs.stats()["rounds"] == 1
    assert int(want[0][250:].sum()) >= 10                        # (accepted items on both sides of item 256)


@pytest.mark.usefixtures("engine")
def test_the_dword_fast_path_and_the_same_call_two_bytes_off(world):
    w = world
    a = Arrays(w, picks_of(w, 70, start=4, step=13))
    want = direct(w, a, 16)
    with make_stream(w) as vs:
        submit(vs, a, 16, host=False, skew=0)(want)              # a 4-byte aligned base, bits_len a multiple of 4
        submit(vs, a, 16, host=False, skew=2)(want)
        submit(vs, a, 16, host=False, skew=4)(want)
    assert int(want[0].sum()) >= 20


def test_interlocks_with_the_committee_table(world):
    w = world
    ct = N.CommitteeTable(w.kt, capacity_hint=4)
    seven = [i for i, it in enumerate(w.pool) if it["cid"] == 1]
    a = Arrays(w, picks_of(w, 12, among=seven, step=1)); a.cid[:] = 0
    try:
        assert ct.append(w.members[1], [0, 7]) == 0
        vs = VerifyStream(w.ctx, committees=ct, msg_table=w.mt, bits_stride=STRIDE, round_items=256, policy=N.STREAM_FULL_ROUNDS)
        try:
            h = vs.submit_committee(a.sig, a.midx, a.cid, a.bits[:, :1].copy(), 1, a.n)
            assert vs.query(h.ticket) == N.PENDING
            for table in (ct, w.mt):                             # clear is refused while the call is pending ...
                with pytest.raises(N.MblsError) as e:
                    table.clear()
                assert e.value.code == N.ERR_ARGUMENT and "not completed" in str(e.value)
            res, st = h.result()
            assert len(ct) == 1 and sum(res) >= 6
            ct.clear()                                           # ... and accepted after the wait
            assert len(ct) == 0
            # an id the table does not hold yet, then the append, then the flush: the round reads the table at the count it has at launch
            h2 = vs.submit_committee(a.sig, a.midx, a.cid, a.bits[:, :1].copy(), 1, a.n)
            assert vs.query(h2.ticket) == N.PENDING and len(ct) == 0
            assert ct.append(w.members[1], [0, 7]) == 0
            vs.flush()
            assert h2.result() == (res, st)
            # a committee the stream's stride cannot hold
            with pytest.raises(N.MblsError) as e:
                ct.append(list(range(100)) + list(range(61)), [0, 161])
            assert e.value.code == N.ERR_ARGUMENT and "stride" in str(e.value) and len(ct) == 1
            assert ct.append(list(range(100)) + list(range(60)), [0, 160]) == 1
        finally:
            vs.close()
        assert ct.append(list(range(100)) + list(range(61)), [0, 161]) == 2 and ct.max_members == 161
        h = N.vp()                                               # and now the stride no longer covers the table
        assert N.lib().mbls_stream_create_committee(w.ctx.handle, ct.handle, w.mt.handle, STRIDE, None, N.C.byref(h)) == N.ERR_ARGUMENT and not h.value
    finally:
        ct.close()


def test_refusals(world):
    w = world
    lib = N.lib(); C = N.C
    a = Arrays(w, picks_of(w, 8))
    d_s, d_mi, d_ci, d_b = dev(a.sig), dev(a.midx), dev(a.cid), dev(a.bits)
    res = torch.zeros(8, dtype=torch.uint8, device=DEV)
    h_res = N.outbuf(8); h_st = (C.c_uint32 * 8)()
    t = C.c_uint64(0)
    p = lambda x: x.data_ptr()
    hp = lambda x: x.ctypes.data
    msgs = np.zeros(8 * 32, dtype=np.uint8)
    with make_stream(w) as cs, VerifyStream(w.ctx, table=w.kt, msg_table=w.mt, round_items=256) as ms:
        # the old entries on a committee stream
        assert lib.mbls_stream_submit_device(cs.handle, p(d_s), p(d_b), 32, None, None, p(d_ci), None, 8, 1, p(res), None, None, None, C.byref(t)) == N.ERR_ARGUMENT
        assert "mbls_stream_submit_committee" in cs.last_error()
        assert lib.mbls_stream_submit(cs.handle, hp(a.sig), hp(msgs), 32, None, None, hp(a.cid), None, 8, 1, h_res, h_st, C.byref(t)) == N.ERR_ARGUMENT
        assert lib.mbls_stream_submit_msgidx_device(cs.handle, p(d_s), p(d_mi), None, p(d_ci), None, 8, 1, p(res), None, None, None, C.byref(t)) == N.ERR_ARGUMENT
        assert lib.mbls_stream_submit_msgidx(cs.handle, hp(a.sig), hp(a.midx), None, hp(a.cid), None, 8, 1, h_res, h_st, C.byref(t)) == N.ERR_ARGUMENT
        assert "mbls_stream_submit_committee" in cs.last_error()
        # the new ones on a message-table stream
        assert lib.mbls_stream_submit_committee_device(ms.handle, p(d_s), p(d_mi), p(d_ci), p(d_b), STRIDE, 8, p(res), None, None, None, C.byref(t)) == N.ERR_ARGUMENT
        assert "mbls_stream_submit_msgidx" in ms.last_error()
        assert lib.mbls_stream_submit_committee(ms.handle, hp(a.sig), hp(a.midx), hp(a.cid), hp(a.bits), STRIDE, 8, h_res, h_st, C.byref(t)) == N.ERR_ARGUMENT
        # bits_len 0 and 21
        for L in (0, STRIDE + 1):
            assert lib.mbls_stream_submit_committee_device(cs.handle, p(d_s), p(d_mi), p(d_ci), p(d_b), L, 8, p(res), None, None, None, C.byref(t)) == N.ERR_ARGUMENT
            assert "bits_len" in cs.last_error()
            assert lib.mbls_stream_submit_committee(cs.handle, hp(a.sig), hp(a.midx), hp(a.cid), hp(a.bits), L, 8, h_res, h_st, C.byref(t)) == N.ERR_ARGUMENT
        assert t.value == 0 and cs.stats()["calls"] == 0 and ms.stats()["calls"] == 0 and cs.last_error() and ms.last_error()
    h = N.vp()
    mk = lambda ctx, ct, mt, stride: lib.mbls_stream_create_committee(ctx.handle, None if ct is None else ct.handle, None if mt is None else mt.handle, stride, None, C.byref(h))
    assert mk(w.ctx, w.ct, w.mt, 18) == N.ERR_ARGUMENT and "multiple of 4" in w.ctx.last_error()
    assert mk(w.ctx, w.ct, w.mt, 16) == N.ERR_ARGUMENT and "largest committee" in w.ctx.last_error()       # 128 bits, 130 members
    assert mk(w.ctx, None, w.mt, STRIDE) == N.ERR_ARGUMENT and mk(w.ctx, w.ct, None, STRIDE) == N.ERR_ARGUMENT
    other = N.Context(0)
    try:
        assert mk(other, w.ct, w.mt, STRIDE) == N.ERR_ARGUMENT   # tables of another context
        okt = N.KeyTable(other, capacity_hint=4); omt = N.MsgTable(other, capacity_hint=4)
        oct_ = N.CommitteeTable(okt, capacity_hint=4)
        try:
            assert mk(w.ctx, w.ct, omt, STRIDE) == N.ERR_ARGUMENT and mk(w.ctx, oct_, w.mt, STRIDE) == N.ERR_ARGUMENT
        finally:
            oct_.close(); omt.close(); okt.close()
    finally:
        other.close()
    assert not h.value
    with make_stream(w) as vs:
        submit(vs, a, STRIDE, host=True)(direct(w, a, STRIDE))


def test_four_threads_share_one_stream(world):
    w = world
    spans = [(0, 40, 17), (40, 70, 16), (110, 7, 3), (117, 90, 20)]
    calls = [Arrays(w, picks_of(w, n, start=s0, step=1)) for s0, n, _ in spans]
    wants = [direct(w, a, L) for a, (_, _, L) in zip(calls, spans)]
    errors = []
    with make_stream(w) as vs:
        def work(j):
            try:
                for _ in range(3):
                    submit(vs, calls[j], spans[j][2], host=(j % 2 == 0))(wants[j])
            except BaseException as e:      # noqa: BLE001 -- reported by the main thread
                errors.append((j, repr(e)))
        threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert vs.stats()["calls"] == 12
