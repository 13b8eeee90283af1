"""GPU checks of the verification stream (include/mbls.h, "verification stream"; milagro_bls_amd/stream.py): every call's results, status words and
bitmap equal a direct call of the device entry on the same inputs, byte for byte, however the stream packed and split it."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import bench
from milagro_bls_amd import _native as N
from milagro_bls_amd.stream import VerifyStream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BASE = 9000
GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def sets():
    """(fmt, k) -> device inputs of BASE items: bench.build_inputs' five rejection classes at i % 16 == 7, plus an undecodable signature
    (i % 32 == 11) and an undecodable key (i % 32 == 27)"""
    ctx = N.default_context()
    out = {}
    for fmt in (N.PK_UNCOMPRESSED, N.PK_COMPRESSED):
        for k in (1, 3, 128):
            d_sigs, d_msgs, d_pks, expect = bench.build_inputs(ctx, torch.device(DEV), BASE, k, fmt, rank=5 + k + 7 * fmt)
            bs = torch.arange(11, BASE, 32, device=DEV)
            d_sigs[bs, 0] &= 0x7F                                               # compression flag cleared
            bp = torch.arange(27, BASE, 32, device=DEV)
            bad = torch.full((d_pks.shape[-1],), 0xFF, dtype=torch.uint8, device=DEV); bad[0] = 0x80 if fmt == N.PK_COMPRESSED else 0x00
            d_pks[bp, 0] = bad                                                  # x >= p
            torch.cuda.synchronize()
            out[(fmt, k)] = (d_sigs, d_msgs, d_pks)
    return out


def direct(ctx, d_sigs, d_msgs, msg_len, moff, d_pks, fmt, poff, n, k, mode=0, table=None, d_idx=None):
    lib = N.lib()
    res = torch.zeros(n, dtype=torch.uint8, device=DEV); st = torch.zeros(n, dtype=torch.int32, device=DEV)
    bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device=DEV)
    dm = torch.tensor(np.array(moff, dtype=np.uint64).view(np.int64), device=DEV) if moff is not None else None
    dp = torch.tensor(np.array(poff, dtype=np.uint32).view(np.int32), device=DEV) if poff is not None else None
    p = lambda t: t.data_ptr() if t is not None else None
    if mode == N.STREAM_VERIFY:
        rc = lib.mbls_verify_batch_device(ctx.handle, p(d_sigs), p(d_msgs), msg_len, p(dm), p(d_pks), fmt, n, p(res), p(bm), p(st), None)
    elif table is not None:
        rc = lib.mbls_fast_aggregate_verify_batch_indexed_device(ctx.handle, table.handle, p(d_sigs), p(d_msgs), msg_len, p(dm), p(d_idx), p(dp), n, k, p(res), p(bm), p(st), None)
    else:
        rc = lib.mbls_fast_aggregate_verify_batch_device(ctx.handle, p(d_sigs), p(d_msgs), msg_len, p(dm), p(d_pks), fmt, p(dp), n, k, p(res), p(bm), p(st), None)
    ctx.check(rc)
    torch.cuda.synchronize()
    return res.cpu(), st.cpu(), bm.cpu()


class Call:
    """one call's output buffers, the bitmap between two guard words"""

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


@pytest.mark.usefixtures("engine")
def test_mixed_traffic_matches_direct_calls(sets):
    ctx = N.default_context()
    rnd = random.Random(2024)
    R = 4096
    streams = {fmt: VerifyStream(ctx, pk_format=fmt, round_items=R, policy=N.STREAM_FULL_ROUNDS) for fmt in (N.PK_UNCOMPRESSED, N.PK_COMPRESSED)}
    shapes = {fmt: [] for fmt in streams}
    calls = []
    keep = []
    for j in range(40):
        fmt = rnd.choice(list(streams))
        n = rnd.choice([1, 63, 64, 65, 1000, 4096, 9000])
        a = rnd.randrange(0, BASE - n + 1)
        kind = rnd.choice(["k1", "k3", "k128", "ragged_keys"])
        k = {"k1": 1, "k3": 3, "k128": 128, "ragged_keys": 128}[kind]
        d_sigs, d_msgs, d_pks = sets[(fmt, k)]
        sig = d_sigs[a:a + n]
        poff = None
        if kind == "ragged_keys":          # absolute offsets into the whole key buffer, items of 128 keys and a few shorter ones
            cnt = [128 if rnd.random() < 0.9 else rnd.randrange(0, 128) for _ in range(n)]
            poff = [128 * a] + (128 * a + np.cumsum(cnt)).tolist()
            pks, kk = d_pks, 0
        else:
            pks, kk = d_pks[a:a + n], k
        if rnd.random() < 0.4:              # ragged messages: some items lose their last byte (they reject)
            m = d_msgs[a:a + n].cpu().numpy()
            lens = [32 if rnd.random() < 0.85 else 31 for _ in range(n)]
            buf = b"".join(m[i].tobytes()[:lens[i]] for i in range(n))
            msgs = torch.frombuffer(bytearray(buf + b"\0"), dtype=torch.uint8).to(DEV)
            moff = [0] + list(np.cumsum(lens).tolist()); msg_len = 0
        else:
            msgs, moff, msg_len = d_msgs[a:a + n], None, 32
        c = Call(n)
        want = direct(ctx, sig, msgs, msg_len, moff, pks, fmt, poff, n, kk)
        t = streams[fmt].submit_device(sig, msgs, pks, n, kk, c.res, msg_len=msg_len, msg_offsets=moff, pk_offsets=poff, bitmap=c.bm, status=c.st)
        shapes[fmt].append(dict(n=n, k=kk, msg_len=msg_len, pk_offsets=poff, msg_offsets=moff))
        calls.append((streams[fmt], t, c, want, fmt, kind, a, n, moff, poff))
        keep.append((sig, msgs, pks))
    for vs in streams.values():
        vs.flush()
    for vs, t, c, want, *_ in calls:
        vs.wait(t)
        c.check(want)
    for fmt, vs in streams.items():
        if not shapes[fmt]:
            continue
        sh = [dict(s) for s in shapes[fmt]]; sh[-1]["flush_after"] = 1
        pieces = N.stream_cut(sh, R, 128 * R, 64 * R)
        st = vs.stats()
        rounds = {}
        for p in pieces:
            rounds[p["round"]] = rounds.get(p["round"], 0) + p["items"]
        per_call = {}
        for p in pieces:
            per_call[p["call"]] = per_call.get(p["call"], 0) + 1
        assert st["pieces"] == len(pieces) and st["rounds"] == len(rounds) and st["calls"] == len(sh)
        assert st["split_calls"] == sum(1 for v in per_call.values() if v > 1)
        assert st["full_rounds"] == sum(1 for v in rounds.values() if v == R)
    for vs in streams.values():
        vs.close()
    # a seeded subsample against the oracle: calls of k = 1 / 3 keys with uniform layouts, every rejection class included
    import orc
    rs = random.Random(9)
    pick = []
    for vs, t, c, want, fmt, kind, a, n, moff, poff in calls:
        if kind in ("k1", "k3") and moff is None:
            res = c.res.cpu()
            for i in range(n):
                if (a + i) % 16 == 7 or (a + i) % 32 in (11, 27) or rs.random() < 0.05:
                    pick.append((fmt, int(kind[1]), a + i, int(res[i])))
    rs.shuffle(pick)
    pick = pick[:600]
    assert len(pick) >= 256
    for fmt in (N.PK_UNCOMPRESSED, N.PK_COMPRESSED):
        for k in (1, 3):
            sel = [p for p in pick if p[0] == fmt and p[1] == k]
            if not sel:
                continue
            d_sigs, d_msgs, d_pks = sets[(fmt, k)]
            ix = torch.tensor([p[2] for p in sel], device=DEV)
            got = orc.batch_fast_aggregate_verify(d_sigs[ix].cpu().numpy().tobytes(), d_msgs[ix].cpu().numpy().tobytes(), d_pks[ix].cpu().numpy().tobytes(),
                                                  len(sel), k, fmt, nthreads=8)
            assert [bool(p[3]) for p in sel] == [bool(g) for g in got]


def test_keytable_stream_with_an_out_of_range_index():
    ctx = N.default_context()
    d_sigs, d_msgs, d_pks, expect, d_idx, table = bench.build_inputs(ctx, torch.device(DEV), 3000, 16, N.PK_UNCOMPRESSED, rank=31, return_indices=True)
    d_idx = d_idx.clone(); d_idx[5, 3] = len(table) + 1000                       # outside the table: MBLS_ST_BAD_PK_ENCODING as in the direct entry
    with VerifyStream(ctx, table=table, round_items=1024, policy=N.STREAM_FULL_ROUNDS) as vs:
        cs = []
        for a, n in ((0, 700), (700, 1500), (2200, 800)):
            c = Call(n)
            want = direct(ctx, d_sigs[a:], d_msgs[a:], 32, None, None, 0, None, n, 16, table=table, d_idx=d_idx[a:])
            t = vs.submit_device(d_sigs[a:], d_msgs[a:], d_idx[a:], n, 16, c.res, msg_len=32, bitmap=c.bm, status=c.st)
            cs.append((t, c, want))
        for t, c, want in cs:
            vs.wait(t)
            c.check(want)
        assert int(cs[0][2][1][5]) & 0x04 and torch.equal(cs[0][1].res.cpu()[:], cs[0][2][0])
        exp = expect.clone(); exp[5] = 0
        assert torch.equal(torch.cat([c.res.cpu() for _, c, _ in cs]), exp)


def test_verify_mode_with_an_infinity_key(sets):
    ctx = N.default_context()
    d_sigs, d_msgs, d_pks = sets[(N.PK_UNCOMPRESSED, 1)]
    n = 300
    pks = d_pks[:n].clone(); pks[10, 0] = 0; pks[10, 0, 0] = 0x40                     # uncompressed infinity
    sigs = d_sigs[:n].clone(); sigs[20] = 0; sigs[20, 0] = 0xC0; pks[20, 0] = 0; pks[20, 0, 0] = 0x40   # infinity / infinity: accepted
    with VerifyStream(ctx, mode=N.STREAM_VERIFY, pk_format=N.PK_UNCOMPRESSED, round_items=256) as vs:
        c = Call(n)
        want = direct(ctx, sigs, d_msgs[:n], 32, None, pks, N.PK_UNCOMPRESSED, None, n, 1, mode=N.STREAM_VERIFY)
        vs.wait(vs.submit_device(sigs, d_msgs[:n], pks, n, 1, c.res, msg_len=32, bitmap=c.bm, status=c.st))
        c.check(want)
        assert int(want[0][10]) == 0 and int(want[0][20]) == 1


def test_full_round_coalescing_at_the_real_round():
    ctx = N.default_context()
    n = 4096
    d_sigs, d_msgs, d_pks, expect = bench.build_inputs(ctx, torch.device(DEV), n, 128, N.PK_UNCOMPRESSED, rank=41)
    with VerifyStream(ctx, pk_format=N.PK_UNCOMPRESSED, policy=N.STREAM_FULL_ROUNDS) as vs:
        assert ctx.limits().round_items == 16 * n
        cs, ts = [], []
        for j in range(16):
            c = Call(n)
            ts.append(vs.submit_device(d_sigs, d_msgs, d_pks, n, 128, c.res, msg_len=32, bitmap=c.bm, status=c.st))
            cs.append(c)
            if j == 14:
                assert all(vs.query(t) == N.PENDING for t in ts)
        for t in ts:
            vs.wait(t)
        st = vs.stats()
        assert st["rounds"] == 1 and st["full_rounds"] == 1 and st["pieces"] == 16
        for c in cs:
            assert torch.equal(c.res.cpu(), expect)


def test_host_submit(sets):
    ctx = N.default_context()
    d_sigs, d_msgs, d_pks = sets[(N.PK_COMPRESSED, 3)]
    with VerifyStream(ctx, pk_format=N.PK_COMPRESSED, round_items=512) as vs:
        hs = []
        for a, n in ((0, 100), (100, 700), (800, 5)):
            sig, msg, pk = (x[a:a + n].cpu().numpy().tobytes() for x in (d_sigs, d_msgs, d_pks))
            hs.append((vs.submit(sig, msg, pk, n, 3, msg_len=32), direct(ctx, d_sigs[a:a + n], d_msgs[a:a + n], 32, None, d_pks[a:a + n], N.PK_COMPRESSED, None, n, 3)))
        for h, want in hs:
            res, st = h.result()
            assert res == bytes(want[0].numpy()) and st == [int(v) & 0xFFFFFFFF for v in want[1].tolist()]
    # nothing written past n
    lib = N.lib()
    with VerifyStream(ctx, pk_format=N.PK_COMPRESSED, round_items=512) as vs:
        n = 10
        res = (C.c_uint8 * (n + 8))(*([0xAB] * (n + 8))); st = (C.c_uint32 * (n + 8))(*([7] * (n + 8)))
        sig, msg, pk = (N.cbuf(x[:n].cpu().numpy().tobytes()) for x in (d_sigs, d_msgs, d_pks))
        t = C.c_uint64(0)
        vs.check(lib.mbls_stream_submit(vs.handle, sig, msg, 32, None, pk, None, None, n, 3, res, st, C.byref(t)))
        vs.wait(t.value)
        assert list(res)[n:] == [0xAB] * 8 and list(st)[n:] == [7] * 8 and all(v in (0, 1) for v in list(res)[:n])


def test_eight_threads_share_one_stream(sets):
    ctx = N.default_context()
    d_sigs, d_msgs, d_pks = sets[(N.PK_UNCOMPRESSED, 3)]
    want = direct(ctx, d_sigs, d_msgs, 32, None, d_pks, N.PK_UNCOMPRESSED, None, BASE, 3)
    errs = []
    with VerifyStream(ctx, pk_format=N.PK_UNCOMPRESSED, round_items=4096) as vs:
        def worker(w):
            try:
                rnd = random.Random(w)
                for _ in range(4):
                    n = rnd.choice([1, 100, 1000]); a = rnd.randrange(0, BASE - n)
                    c = Call(n)
                    vs.wait(vs.submit_device(d_sigs[a:a + n], d_msgs[a:a + n], d_pks[a:a + n], n, 3, c.res, msg_len=32, status=c.st))
                    assert torch.equal(c.res.cpu(), want[0][a:a + n]) and torch.equal(c.st.cpu(), want[1][a:a + n])
            except Exception as e:          # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=worker, args=(w,)) for w in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert not errs, errs


def test_flush_and_destroy(sets):
    ctx = N.default_context()
    d_sigs, d_msgs, d_pks = sets[(N.PK_UNCOMPRESSED, 1)]
    want = direct(ctx, d_sigs[:50], d_msgs[:50], 32, None, d_pks[:50], N.PK_UNCOMPRESSED, None, 50, 1)
    vs = VerifyStream(ctx, pk_format=N.PK_UNCOMPRESSED, round_items=4096, policy=N.STREAM_FULL_ROUNDS)
    c = Call(50)
    t = vs.submit_device(d_sigs, d_msgs, d_pks, 50, 1, c.res, msg_len=32, status=c.st)
    assert vs.query(t) == N.PENDING
    vs.flush()
    vs.wait(t)
    assert vs.query(t) == N.OK and torch.equal(c.res.cpu(), want[0])
    c2 = Call(50)
    vs.submit_device(d_sigs, d_msgs, d_pks, 50, 1, c2.res, msg_len=32, status=c2.st)
    vs.close()                                   # destroy completes the pending call
    assert torch.equal(c2.res.cpu(), want[0]) and torch.equal(c2.st.cpu(), want[1])


def test_argument_refusals(sets):
    ctx = N.default_context()
    lib = N.lib()
    d_sigs, d_msgs, d_pks = sets[(N.PK_UNCOMPRESSED, 1)]
    other = N.Context(0)
    t_other = N.KeyTable(other, 16)
    h = N.vp()
    assert lib.mbls_stream_create(ctx.handle, 0, 1, t_other.handle, None, C.byref(h)) == N.ERR_ARGUMENT          # a key table of another context
    t_mine = N.KeyTable(ctx, 16)
    assert lib.mbls_stream_create(ctx.handle, N.STREAM_VERIFY, 1, t_mine.handle, None, C.byref(h)) == N.ERR_ARGUMENT   # verify mode has no indexed entry
    with VerifyStream(ctx, pk_format=N.PK_UNCOMPRESSED, round_items=256) as vs:
        res = torch.zeros(4, dtype=torch.uint8, device=DEV)
        t = C.c_uint64(0)
        idx = torch.zeros(4, dtype=torch.int32, device=DEV)
        rc = lib.mbls_stream_submit_device(vs.handle, d_sigs.data_ptr(), d_msgs.data_ptr(), 32, None, None, idx.data_ptr(), None, 4, 1, res.data_ptr(), None, None, None, C.byref(t))
        assert rc == N.ERR_ARGUMENT                                                # indices on a byte-key stream
        back = (C.c_uint32 * 5)(0, 2, 1, 3, 4)
        rc = lib.mbls_stream_submit_device(vs.handle, d_sigs.data_ptr(), d_msgs.data_ptr(), 32, None, d_pks.data_ptr(), None, back, 4, 0, res.data_ptr(), None, None, None, C.byref(t))
        assert rc == N.ERR_ARGUMENT and "backwards" in vs.last_error()            # a backward offset table: no ticket
        assert vs.query(1) == N.ERR_ARGUMENT and lib.mbls_stream_wait(vs.handle, 1) == N.ERR_ARGUMENT   # an unknown (future) ticket
        big = (C.c_uint32 * 3)(0, 1, 1 + 128 * 256 + 1)
        rc = lib.mbls_stream_submit_device(vs.handle, d_sigs.data_ptr(), d_msgs.data_ptr(), 32, None, d_pks.data_ptr(), None, big, 2, 0, res.data_ptr(), None, None, None, C.byref(t))
        assert rc == N.ERR_ARGUMENT and "round_keys" in vs.last_error()          # an item larger than an empty round
    t_mine.close(); t_other.close(); other.close()
