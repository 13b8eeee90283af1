"""GPU checks of the verification stream over a resident message table (include/mbls.h, mbls_stream_create_msgtable / mbls_stream_submit_msgidx[_device];
milagro_bls_amd/stream.py, VerifyStream(msg_table=)): every call's results, status words and bitmap equal a direct call of the `_msgtable_device` entry on the same
inputs, byte for byte, however the stream packed and split it -- and that direct call equals the per-item entry on the messages spelled out."""
import threading
import time

import numpy as np
import pytest

import bench
from milagro_bls_amd import _native as N
from milagro_bls_amd.stream import VerifyStream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BASE = 512
K = 3
GUARD = 0x5A5A5A5A5A5A5A5A
BAD = 0x100
SIZES = (1, 100, 300, 55)


class Source:
    pass


@pytest.fixture(scope="module")
def sources():
    """three key sources over ONE message table: bench.build_inputs' items (five rejection classes at i % 16 == 7), item i's message at entry perm[i] of the table;
    item 3 names item 4's entry (pairing fails), items 9 and 200 name nothing (`size` and 0xFFFFFFFF)"""
    ctx = N.default_context()
    dev = torch.device(DEV)
    out = {}
    mt = N.MsgTable(ctx, capacity_hint=3 * BASE)
    for j, name in enumerate(("bytes96", "bytes48", "table")):
        fmt = N.PK_COMPRESSED if name == "bytes48" else N.PK_UNCOMPRESSED
        s = Source(); s.name = name; s.fmt = fmt
        r = bench.build_inputs(ctx, dev, BASE, K, fmt, rank=60 + j, return_indices=(name == "table"))
        s.d_sigs, s.d_msgs, s.d_pks = r[0], r[1], r[2]
        s.table, s.d_kidx = (r[5], r[4].to(torch.int32).contiguous()) if name == "table" else (None, None)
        perm = np.random.default_rng(70 + j).permutation(BASE)
        listed = torch.empty_like(s.d_msgs)
        listed[torch.from_numpy(perm).to(dev)] = s.d_msgs
        torch.cuda.synchronize()
        first = mt.append_device(listed.data_ptr(), BASE, msg_len=32)
        torch.cuda.synchronize()
        idx = (perm + first).astype(np.int64)
        idx[3] = idx[4]
        s.idx = idx; s.keep = listed
        out[name] = s
    size = len(mt)
    assert size == 3 * BASE
    for s in out.values():
        s.idx[9] = size; s.idx[200] = 0xFFFFFFFF
        s.h_idx = s.idx.astype(np.uint32)
        s.d_midx = torch.from_numpy(s.h_idx.view(np.int32).copy()).to(dev)
    torch.cuda.synchronize()
    yield ctx, mt, out
    for s in out.values():
        if s.table is not None:
            s.table.close()
    mt.close()


def direct(ctx, mt, s, a, n):
    """the `_msgtable_device` entry of the source on items [a, a + n)"""
    lib = N.lib()
    res = torch.zeros(n, dtype=torch.uint8, device=DEV); st = torch.zeros(n, dtype=torch.int32, device=DEV)
    bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device=DEV)
    p = lambda t: t.data_ptr()
    if s.table is not None:
        rc = lib.mbls_fast_aggregate_verify_batch_indexed_msgtable_device(ctx.handle, s.table.handle, p(s.d_sigs[a:]), mt.handle, p(s.d_midx[a:]), p(s.d_kidx[a:]), None,
                                                                          n, K, p(res), p(bm), p(st), None)
    else:
        rc = lib.mbls_fast_aggregate_verify_batch_msgtable_device(ctx.handle, p(s.d_sigs[a:]), mt.handle, p(s.d_midx[a:]), p(s.d_pks[a:]), s.fmt, None, n, K,
                                                                  p(res), p(bm), p(st), None)
    ctx.check(rc)
    torch.cuda.synchronize()
    return res.cpu(), st.cpu(), bm.cpu()


class Call:
    """one device call's output buffers, the bitmap between two guard words"""

    def __init__(self, n):
        self.n = n
        self.res = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
        self.st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        self.bm_all = torch.full(((n + 63) // 64 + 2,), GUARD, dtype=torch.int64, device=DEV)
        self.bm = self.bm_all[1:-1]

    def check(self, want):
        res, st, bm = want
        assert torch.equal(self.res.cpu(), res) and torch.equal(self.st.cpu(), st)
        allw = self.bm_all.cpu()
        assert int(allw[0]) == GUARD and int(allw[-1]) == GUARD, "bitmap words outside the call were touched"
        assert torch.equal(allw[1:-1], bm)


def make_stream(ctx, mt, s, **kw):
    kw.setdefault("round_items", 256)
    return VerifyStream(ctx, pk_format=s.fmt, table=s.table, msg_table=mt, **kw)


def submit(vs, s, a, n, host):
    """-> (wait-and-check function)"""
    keys = s.d_kidx if s.table is not None else s.d_pks
    if host:
        h = vs.submit(s.d_sigs[a:a + n].cpu().numpy(), s.h_idx[a:a + n], keys[a:a + n].cpu().numpy().view(np.uint32 if s.table is not None else np.uint8), n, K)
        return lambda want: _check_host(h, want)
    c = Call(n)
    t = vs.submit_device(s.d_sigs[a:], s.d_midx[a:], keys[a:], n, K, c.res, bitmap=c.bm, status=c.st)
    return lambda want: (vs.wait(t), c.check(want))


def _check_host(h, want):
    res, st = h.result()
    assert res == bytes(want[0].tolist()) and [x & 0xffffffff for x in st] == [x & 0xffffffff for x in want[1].tolist()]


@pytest.mark.usefixtures("engine")
def test_calls_of_1_100_300_and_55_items_in_the_three_key_sources(sources):
    ctx, mt, src = sources
    for name, s in src.items():
        wants = []; a = 0
        for n in SIZES:
            wants.append((a, n, direct(ctx, mt, s, a, n))); a += n
        # the direct call itself: items that name nothing carry the bit and are rejected, item 3 (another item's entry) fails its pairing check, the rest is
        # what the per-item entry gives on the spelled-out messages
        whole = direct(ctx, mt, s, 0, BASE)
        assert not whole[0][9] and int(whole[1][9]) & BAD and not whole[0][200] and int(whole[1][200]) & BAD
        assert not whole[0][3] and int(whole[1][3]) == 0x40
        lib = N.lib(); p = lambda t: t.data_ptr()
        res = torch.zeros(BASE, dtype=torch.uint8, device=DEV); st = torch.zeros(BASE, dtype=torch.int32, device=DEV)
        if s.table is not None:
            ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_device(ctx.handle, s.table.handle, p(s.d_sigs), p(s.d_msgs), 32, None, p(s.d_kidx), None, BASE, K,
                                                                          p(res), None, p(st), None))
        else:
            ctx.check(lib.mbls_fast_aggregate_verify_batch_device(ctx.handle, p(s.d_sigs), p(s.d_msgs), 32, None, p(s.d_pks), s.fmt, None, BASE, K, p(res), None, p(st), None))
        torch.cuda.synchronize()
        same = [i for i in range(BASE) if i not in (3, 9, 200)]
        assert torch.equal(whole[0][same], res.cpu()[same]) and torch.equal(whole[1][same], st.cpu()[same])
        with make_stream(ctx, mt, s, policy=N.STREAM_FULL_ROUNDS) as vs:
            checks = [submit(vs, s, a, n, host=(j % 2 == 1)) for j, (a, n, _) in enumerate(wants)]
            vs.flush()
            for chk, (_, _, want) in zip(checks, wants):
                chk(want)
            stats = vs.stats()
            shapes = [dict(n=n, k=K, msg_len=4) for n in SIZES]; shapes[-1]["flush_after"] = 1
            pieces = N.stream_cut(shapes, 256, 128 * 256, 4 * 256)
            assert stats["calls"] == 4 and stats["items"] == sum(SIZES) and stats["pieces"] == len(pieces) and stats["split_calls"] == 1
            assert stats["rounds"] == len({pc["round"] for pc in pieces}) == 2


def test_a_lone_call_completes_without_a_flush_and_late_entries_are_seen(sources):
    """work-conserving (the default): a lone call launches at once. FULL_ROUNDS: a call submitted with indices the table does not hold yet, an append, then the
    flush -- the round reads the table at the size it has at launch, so the indices are valid."""
    ctx, mt, src = sources
    s = src["bytes96"]
    want = direct(ctx, mt, s, 0, 40)
    with make_stream(ctx, mt, s) as vs:
        c = Call(40)
        t = vs.submit_device(s.d_sigs, s.d_midx, s.d_pks, 40, K, c.res, bitmap=c.bm, status=c.st)
        deadline = time.monotonic() + 60            # no flush and no wait (a wait would launch the round itself): the query turns by itself
        while vs.query(t) == N.PENDING and time.monotonic() < deadline:
            time.sleep(0.001)
        assert vs.query(t) == N.OK and vs.stats()["rounds"] == 1
        c.check(want)
    n = 20
    late = N.MsgTable(ctx, capacity_hint=64)
    try:
        with VerifyStream(ctx, pk_format=s.fmt, msg_table=late, round_items=256, policy=N.STREAM_FULL_ROUNDS) as vs:
            d_midx = torch.arange(n, dtype=torch.int32, device=DEV)
            c = Call(n)
            t = vs.submit_device(s.d_sigs[16:], d_midx, s.d_pks[16:], n, K, c.res, bitmap=c.bm, status=c.st)
            assert vs.query(t) == N.PENDING and len(late) == 0
            assert late.append_device(s.d_msgs[16:].data_ptr(), n, msg_len=32) == 0
            vs.flush(); vs.wait(t)
            lib = N.lib(); p = lambda x: x.data_ptr()
            res = torch.zeros(n, dtype=torch.uint8, device=DEV); st = torch.zeros(n, dtype=torch.int32, device=DEV); bm = torch.zeros(1, dtype=torch.int64, device=DEV)
            ctx.check(lib.mbls_fast_aggregate_verify_batch_device(ctx.handle, p(s.d_sigs[16:]), p(s.d_msgs[16:]), 32, None, p(s.d_pks[16:]), s.fmt, None, n, K,
                                                                  p(res), p(bm), p(st), None))
            torch.cuda.synchronize()
            c.check((res.cpu(), st.cpu(), bm.cpu()))
            assert int(res.sum()) == n - 1              # item 23 of the source (i % 16 == 7) is a rejection class
    finally:
        late.close()


def test_the_old_and_the_new_submit_entries_do_not_mix(sources):
    ctx, mt, src = sources
    s = src["bytes96"]
    lib = N.lib(); p = lambda x: x.data_ptr()
    res = torch.zeros(8, dtype=torch.uint8, device=DEV)
    h_res = N.outbuf(8); h_st = (N.C.c_uint32 * 8)()
    t = N.C.c_uint64(0)
    sig = s.d_sigs[:8].cpu().numpy(); pk = s.d_pks[:8].cpu().numpy(); msg = s.d_msgs[:8].cpu().numpy()
    with make_stream(ctx, mt, s) as new, VerifyStream(ctx, pk_format=s.fmt, round_items=256) as old:
        assert lib.mbls_stream_submit_device(new.handle, p(s.d_sigs), p(s.d_msgs), 32, None, p(s.d_pks), None, None, 8, K, p(res), None, None, None, N.C.byref(t)) == N.ERR_ARGUMENT
        assert "message indices" in new.last_error()
        assert lib.mbls_stream_submit(new.handle, sig.ctypes.data, msg.ctypes.data, 32, None, pk.ctypes.data, None, None, 8, K, h_res, h_st, N.C.byref(t)) == N.ERR_ARGUMENT
        assert lib.mbls_stream_submit_msgidx_device(old.handle, p(s.d_sigs), p(s.d_midx), p(s.d_pks), None, None, 8, K, p(res), None, None, None, N.C.byref(t)) == N.ERR_ARGUMENT
        assert "not message-table indices" in old.last_error()
        assert lib.mbls_stream_submit_msgidx(old.handle, sig.ctypes.data, s.h_idx.ctypes.data, pk.ctypes.data, None, None, 8, K, h_res, h_st, N.C.byref(t)) == N.ERR_ARGUMENT
        assert t.value == 0 and new.stats()["calls"] == 0 and old.stats()["calls"] == 0
    other = N.Context(0)
    try:
        h = N.vp()
        assert lib.mbls_stream_create_msgtable(other.handle, 0, s.fmt, None, mt.handle, None, N.C.byref(h)) == N.ERR_ARGUMENT      # a table of another context
        assert lib.mbls_stream_create_msgtable(ctx.handle, 0, s.fmt, None, None, None, N.C.byref(h)) == N.ERR_ARGUMENT
    finally:
        other.close()


def test_four_threads_share_one_stream(sources):
    ctx, mt, src = sources
    s = src["bytes48"]
    spans = [(0, 90), (90, 130), (220, 7), (227, 200)]
    wants = [direct(ctx, mt, s, a, n) for a, n in spans]
    errors = []
    with make_stream(ctx, mt, s) as vs:
        def work(j):
            try:
                a, n = spans[j]
                for _ in range(3):
                    submit(vs, s, a, n, host=(j % 2 == 0))(wants[j])
            except BaseException as e:      # noqa: BLE001 -- reported by the main thread
                errors.append((j, repr(e)))
        threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert vs.stats()["calls"] == 12
