"""GPU checks of the verify_multiple stream over a committee table and a message table (include/mbls.h, mbls_stream_create_vm_committee /
mbls_stream_submit_vm[_device] / mbls_stream_cut_vm; milagro_bls_amd/stream.py, VerifyStream(vm=True, committees=, msg_table=, bits_stride=)). A call is one
batch; every output of a call -- its byte, its status word, its sets' bytes and words -- is compared BYTE FOR BYTE with
mbls_verify_multiple_batches_committee_msgtable_locate_device on that call alone as one batch (n_batches = 1, sets_per_batch = n_sets), the same signatures, set
words, indices and scalars, every field cut to the call's bits_len and zero-extended to the stride by numpy. Outputs lie between guard bytes and guard words, for
device and host submits alike. The world is that of tests/test_gpu_stream_committee.py -- 150 keys, committees of 1, 7, 64, 65, 127, 128 and 130 members, 32
table entries, stride 20 -- plus signatures under single keys; it is built once per module."""
import ctypes
import random
import threading

import numpy as np
import pytest

import bls12_381 as M
import helpers
from milagro_bls_amd import _native as N
from milagro_bls_amd.stream import VerifyStream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
NK = 150
SIZES = (1, 7, 64, 65, 127, 128, 130)
STRIDE = 20                                                      # 160 bits cover the largest committee
N_MSGS, N_ENTRIES = 4, 32                                        # table entry j holds message j % 4
GUARD_BYTE, GUARD_WORD = 0xC3, 0x6B6B6B6B
NOT_IN_G2, BAD_PK, PAIRING, BAD_SCALAR, BAD_MSG = 0x02, 0x04, 0x40, 0x80, 0x100
SINGLE = N.VM_SET_SINGLE_KEY


class World:
    pass


def set_grouping(ctx, mode):
    ctx.check(N.lib().mbls_ctx_set_vm_grouping(ctx.handle, mode))


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
    # the pool, every set of it valid: per committee an almost full field (complement route), one near 30 % (direct), the full and a one-member field; then
    # signatures under single keys
    pool = []
    for c, m in enumerate(SIZES):
        near99 = sorted(set(range(m)) - {rnd.randrange(m)}) if m > 1 else [0]
        near30 = sorted(rnd.sample(range(m), max(1, (3 * m) // 10)))
        for tag, sel in (("near99", near99), ("near30", near30), ("all", list(range(m))), ("last", [m - 1])):
            for e in (c, c + 9):
                pool.append(dict(cid=c, sel=sel, entry=e, tag=tag, size=m))
    for j in range(40):
        pool.append(dict(key=(7 * j + 1) % NK, entry=(3 * j) % N_ENTRIES, tag="single", size=0))
    one = batch.sign_batch(b"".join(sks[i].to_bytes(32, "big") for _ in range(N_MSGS) for i in range(NK)), b"".join(w.msgs[j] for j in range(N_MSGS) for _ in range(NK)),
                           N_MSGS * NK, msg_len=32)
    sig_of = lambda key, msg: one[96 * (msg * NK + key):96 * (msg * NK + key) + 96]
    parts, off = [], [0]
    for it in pool:
        signers = [it["key"]] if it["tag"] == "single" else [w.members[it["cid"]][j] for j in it["sel"]]
        parts += [sig_of(k, it["entry"] % N_MSGS) for k in signers]
        off.append(len(parts))
    agg, errs = batch.aggregate_signatures_batch(b"".join(parts), len(pool), offsets=off)
    assert not any(errs)
    w.pool = pool
    w.sig = np.frombuffer(agg, dtype=np.uint8).reshape(len(pool), 96).copy()
    w.midx = np.array([it["entry"] for it in pool], dtype=np.uint32)
    w.word = np.array([SINGLE | it["key"] if it["tag"] == "single" else it["cid"] for it in pool], dtype=np.uint32)
    w.bits = np.zeros((len(pool), STRIDE), dtype=np.uint8)
    for i, it in enumerate(pool):
        for j in it.get("sel", ()):
            w.bits[i, j >> 3] |= 1 << (j & 7)
    w.singles = [i for i, it in enumerate(pool) if it["tag"] == "single"]
    w.not_in_g2 = np.frombuffer(bytes.fromhex(helpers.load_vectors()["model"]["g2_subgroup_probes"][0]["compressed"]), dtype=np.uint8)
    yield w
    ctx.set_committee_route(0); set_grouping(ctx, 0)
    w.ct.close(); w.mt.close(); w.kt.close()


@pytest.fixture(autouse=True)
def _modes_back():
    yield
    N.default_context().set_committee_route(0); set_grouping(N.default_context(), 0)


class Batch:
    """one call: n sets whose fields fit bits_len bytes -- two single-key sets per committee set where a committee fits, single-key sets only otherwise --, the
    fields at the full stride, nonzero scalars"""

    def __init__(self, w, n, bits_len, seed):
        rnd = random.Random(1000 * seed + n)
        fits = [i for i, it in enumerate(w.pool) if it["tag"] != "single" and it["size"] <= 8 * bits_len]
        picks = [rnd.choice(fits) if fits and j % 3 == 0 else rnd.choice(w.singles) for j in range(n)]
        self.n, self.bits_len, self.picks = n, bits_len, picks
        self.sig, self.word, self.midx, self.bits = w.sig[picks].copy(), w.word[picks].copy(), w.midx[picks].copy(), w.bits[picks].copy()
        self.rands = np.array([rnd.randrange(1, 1 << 64) for _ in range(n)], dtype=np.uint64)
        self.committee_sets = [j for j, p in enumerate(picks) if w.pool[p]["tag"] != "single"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def direct(w, b):
    """the call alone as ONE batch of the direct entry, every field cut to bits_len bytes and zero-extended to the stride -> (byte, word, set bytes, set words)"""
    f = b.bits.copy(); f[:, b.bits_len:] = 0
    d_s, d_w, d_f, d_mi, d_r = dev(b.sig), dev(b.word), dev(f), dev(b.midx), dev(b.rands)
    res = torch.full((1,), 7, dtype=torch.uint8, device=DEV); st = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    sres = torch.full((b.n,), 7, dtype=torch.uint8, device=DEV); sst = torch.full((b.n,), 7, dtype=torch.int32, device=DEV)
    w.ctx.check(N.lib().mbls_verify_multiple_batches_committee_msgtable_locate_device(
        w.ctx.handle, w.ct.handle, d_s.data_ptr(), d_w.data_ptr(), d_f.data_ptr(), STRIDE, w.mt.handle, d_mi.data_ptr(), d_r.data_ptr(), b.n, None, b.n, 1, 0,
        res.data_ptr(), st.data_ptr(), sres.data_ptr(), sst.data_ptr(), None))
    torch.cuda.synchronize()
    return res.cpu().numpy(), st.cpu().numpy().view(np.uint32), sres.cpu().numpy(), sst.cpu().numpy().view(np.uint32)


class Out:
    """a call's four outputs between guards, on the device (torch) or on the host (numpy): 16 guard bytes / 4 guard words on either side"""

    def __init__(self, n, host):
        self.n, self.host = n, host
        mk8 = (lambda k: np.full(k, GUARD_BYTE, dtype=np.uint8)) if host else (lambda k: torch.full((k,), GUARD_BYTE, dtype=torch.uint8, device=DEV))
        mk32 = (lambda k: np.full(k, GUARD_WORD, dtype=np.uint32)) if host else (lambda k: torch.full((k,), GUARD_WORD, dtype=torch.int32, device=DEV))
        self.res, self.st, self.sres, self.sst = mk8(1 + 32), mk32(1 + 8), mk8(n + 32), mk32(n + 8)

    def ptrs(self):
        a = (lambda x, o, sz: x.ctypes.data + o * sz) if self.host else (lambda x, o, sz: x.data_ptr() + o * sz)
        return a(self.res, 16, 1), a(self.st, 4, 4), a(self.sres, 16, 1), a(self.sst, 4, 4)

    def read(self):
        h = (lambda x: x) if self.host else (lambda x: x.cpu().numpy())
        return h(self.res), h(self.st).view(np.uint32), h(self.sres), h(self.sst).view(np.uint32)

    def check(self, want, what=""):
        res, st, sres, sst = self.read()
        n = self.n
        got = (res[16:17], st[4:5], sres[16:16 + n], sst[4:4 + n])
        for name, g, x in zip(("batch byte", "batch word", "set bytes", "set words"), got, want):
            assert np.array_equal(g, x), (what, name, g.tolist(), x.tolist())
        for name, a, k, guard in (("batch byte", res, 1, GUARD_BYTE), ("set bytes", sres, n, GUARD_BYTE)):
            assert (a[:16] == guard).all() and (a[16 + k:] == guard).all(), (what, name, "bytes outside the call were touched")
        for name, a, k, guard in (("batch word", st, 1, GUARD_WORD), ("set words", sst, n, GUARD_WORD)):
            assert (a[:4] == guard).all() and (a[4 + k:] == guard).all(), (what, name, "words outside the call were touched")


def submit(vs, b, host, skew=1, sets_out=True):
    """the call with its fields cut to bits_len bytes back to back; a device call's fields start `skew` bytes into an allocation -> (ticket, check function)"""
    fields = np.ascontiguousarray(b.bits[:, :b.bits_len])
    o = Out(b.n, host)
    p_res, p_st, p_sres, p_sst = o.ptrs()
    if not sets_out:
        p_sres = p_sst = None
    t = ctypes.c_uint64(0)
    if host:
        keep = (np.ascontiguousarray(b.sig), b.word.copy(), fields, b.midx.copy(), b.rands.copy())
        hp = lambda x: x.ctypes.data
        rc = N.lib().mbls_stream_submit_vm(vs.handle, hp(keep[0]), hp(keep[1]), hp(fields) if b.bits_len else None, b.bits_len, hp(keep[3]), hp(keep[4]), b.n,
                                           p_res, p_st, p_sres, p_sst, ctypes.byref(t))
    else:
        d_f = torch.zeros(b.n * b.bits_len + skew + 3, dtype=torch.uint8, device=DEV)
        if b.bits_len:
            d_f[skew:skew + b.n * b.bits_len] = dev(fields)
        keep = (dev(b.sig), dev(b.word), d_f, dev(b.midx), dev(b.rands))
        torch.cuda.synchronize()
        rc = N.lib().mbls_stream_submit_vm_device(vs.handle, keep[0].data_ptr(), keep[1].data_ptr(), d_f.data_ptr() + skew if b.bits_len else None, b.bits_len,
                                                  keep[3].data_ptr(), keep[4].data_ptr(), b.n, p_res, p_st, p_sres, p_sst, None, ctypes.byref(t))
    vs.check(rc)

    def chk(want, what=""):
        vs.wait(t.value)
        torch.cuda.synchronize()
        if not sets_out:
            want = (want[0], want[1], np.full(b.n, GUARD_BYTE, dtype=np.uint8), np.full(b.n, GUARD_WORD, dtype=np.uint32))
        o.check(want, what)
        return keep
    return t.value, chk


def make_stream(w, **kw):
    kw.setdefault("round_items", 256)
    return VerifyStream(w.ctx, vm=True, committees=w.ct, msg_table=w.mt, bits_stride=STRIDE, **kw)


def test_mixed_calls_in_one_round_under_all_grouping_and_route_modes(world):
    """calls of 1, 2, 3, 10 and 63 sets that mix committee and single-key sets, device and host submits interleaved in one round, bits_len 0, 1, 17 and 20, the
    device fields at an odd address -- under all 3 x 3 modes of mbls_ctx_set_vm_grouping and mbls_ctx_set_committee_route"""
    w = world
    sizes, lens = (1, 2, 3, 10, 63), (0, 1, 17, 20, 17)
    calls = [Batch(w, n, L, seed=j) for j, (n, L) in enumerate(zip(sizes, lens))]
    assert not calls[0].committee_sets and all(c.committee_sets for c in calls[2:])
    with make_stream(w, policy=N.STREAM_FULL_ROUNDS) as vs:
        rounds = 0
        for grouping in (0, 1, 2):
            for route in (0, 1, 2):
                set_grouping(w.ctx, grouping); w.ctx.set_committee_route(route)
                wants = [direct(w, c) for c in calls]
                assert all(int(x[0][0]) == 1 and int(x[1][0]) == 0 for x in wants), (grouping, route)
                checks = [submit(vs, c, host=(j + grouping + route) % 2 == 1)[1] for j, c in enumerate(calls)]
                vs.flush()
                for j, (chk, want) in enumerate(zip(checks, wants)):
                    chk(want, (grouping, route, j))
                rounds += 1
                assert vs.stats()["rounds"] == rounds                # device and host calls shared the round
        st = vs.stats()
        assert st["calls"] == st["pieces"] == 9 * 5 and st["split_calls"] == 0 and st["items"] == 9 * sum(sizes)
        assert st["gathered_bytes"] == 9 * sum(n * (96 + 4 + 4 + 8 + L) for n, L in zip(sizes, lens))


@pytest.mark.parametrize("n,host", [(257, False), (513, False), (257, True)])
def test_calls_that_cross_gather_tile_boundaries(world, n, host):
    """257 and 513 sets: one set past one and two tiles of 256, in a round that holds exactly the call"""
    w = world
    b = Batch(w, n, 17, seed=n)
    want = direct(w, b)
    assert int(want[0][0]) == 1 and want[2].all()
    with make_stream(w, round_items=n + 1, policy=N.STREAM_FULL_ROUNDS) as vs:
        chk = submit(vs, b, host=host)[1]
        chk(want)
        st = vs.stats()
        assert st["rounds"] == 1 and st["full_rounds"] == 1 and st["pieces"] == 1
        # a flipped bit in the last set, behind the last tile boundary
        b.bits[b.committee_sets[-1], 0] ^= 1
        bad = direct(w, b)
        assert int(bad[0][0]) == 0 and not bad[2][b.committee_sets[-1]] and int(bad[2].sum()) == n - 1
        submit(vs, b, host=host)[1](bad)


def test_a_bad_call_rejects_itself_alone(world):
    """one round: valid calls with, between them, one call each with a flipped participation bit, a signature outside G2, a message index beyond the table, a
    committee id beyond the count and a zero scalar. The neighbours equal their direct calls and are accepted; the bad call's set bytes and words name the bad set."""
    w = world
    good = [Batch(w, 6, 17, seed=20 + j) for j in range(6)]
    bad = [Batch(w, 7, 17, seed=40 + j) for j in range(5)]
    at = [b.committee_sets[1] for b in bad]
    whole = next(i for i, it in enumerate(w.pool) if it.get("cid") == 2 and it["tag"] == "all")        # all 64 members: without member 0 the pairing fails
    bad[0].sig[at[0]], bad[0].word[at[0]], bad[0].midx[at[0]], bad[0].bits[at[0]] = w.sig[whole], w.word[whole], w.midx[whole], w.bits[whole]
    bad[0].bits[at[0], 0] ^= 1
    bad[1].sig[at[1]] = w.not_in_g2
    bad[2].midx[at[2]] = len(w.mt)
    bad[3].word[at[3]] = len(w.ct)
    bad[4].rands[at[4]] = 0
    order = [good[0]]
    for j in range(5):
        order += [bad[j], good[j + 1]]
    wants = [direct(w, b) for b in order]
    with make_stream(w, policy=N.STREAM_FULL_ROUNDS) as vs:
        checks = [submit(vs, b, host=(j % 3 == 1))[1] for j, b in enumerate(order)]
        vs.flush()
        for j, (chk, want) in enumerate(zip(checks, wants)):
            chk(want, j)
        assert vs.stats()["rounds"] == 1
    for j, want in enumerate(wants):
        if j % 2 == 0:
            assert int(want[0][0]) == 1 and int(want[1][0]) == 0 and want[2].all() and not want[3].any(), j
    flip, g2, midx, cid, zero = (wants[1 + 2 * j] for j in range(5))
    for j, x in enumerate((flip, g2, midx, cid, zero)):
        assert int(x[0][0]) == 0, j
    for x, i, bit in ((g2, at[1], NOT_IN_G2), (midx, at[2], BAD_MSG), (cid, at[3], BAD_PK)):
        assert int(x[3][i]) & bit and not x[2][i] and int(x[2].sum()) == 6 and int(x[1][0]) & bit
    assert not flip[2][at[0]] and int(flip[2].sum()) == 6 and int(flip[3][at[0]]) == PAIRING
    assert int(zero[1][0]) & BAD_SCALAR and int(zero[3][at[4]]) & BAD_SCALAR


def test_cutting_equals_mbls_stream_cut_vm(world):
    w = world
    sizes = (3, 10, 1, 14, 1, 13, 15, 2, 2)
    calls = [Batch(w, n, 20 if j % 2 else 1, seed=60 + j) for j, n in enumerate(sizes)]
    wants = [direct(w, c) for c in calls]
    pieces = N.stream_cut_vm(list(sizes), 16, [0] * (len(sizes) - 1) + [1])
    assert [p["items"] for p in pieces] == list(sizes) and all(p["first"] == 0 for p in pieces)
    lib = N.lib()
    with make_stream(w, round_items=16, policy=N.STREAM_FULL_ROUNDS) as vs:
        checks = [submit(vs, c, host=(j % 2 == 0))[1] for j, c in enumerate(calls)]
        # a call of round_items sets is refused with no ticket; one of round_items - 1 was accepted above
        big = Batch(w, 16, 0, seed=99); t = ctypes.c_uint64(0); o = Out(16, True); hp = lambda x: x.ctypes.data
        assert lib.mbls_stream_submit_vm(vs.handle, hp(big.sig), hp(big.word), None, 0, hp(big.midx), hp(big.rands), 16, *o.ptrs(), ctypes.byref(t)) == N.ERR_ARGUMENT
        assert t.value == 0 and "16" in vs.last_error() and "round_items" in vs.last_error()
        vs.flush()
        for j, (chk, want) in enumerate(zip(checks, wants)):
            chk(want, j)
        st = vs.stats()
        assert st["rounds"] == len({p["round"] for p in pieces}) == 6
        assert st["calls"] == st["pieces"] == len(pieces) and st["split_calls"] == 0
        o.check((np.full(1, GUARD_BYTE, np.uint8), np.full(1, GUARD_WORD, np.uint32), np.full(16, GUARD_BYTE, np.uint8), np.full(16, GUARD_WORD, np.uint32)))


@pytest.mark.parametrize("host", [False, True])
def test_a_slot_shows_no_round_the_fields_or_scalars_of_the_round_before(world, host):
    """depth = 1: two slots, so the third round stages into the first round's slot. A round of all-ones fields over the whole stride and 40 sets, then rounds of
    fewer sets with true fields at 17, 1 and 0 bytes: each equals its direct call, where a byte left over from the all-ones round would select members the
    zero-extended field does not, and a scalar left over would blind with the wrong value."""
    w = world
    ones = Batch(w, 40, 20, seed=70); ones.bits[:] = 0xFF
    seq = [ones, ones, Batch(w, 12, 17, seed=71), Batch(w, 9, 1, seed=72), Batch(w, 5, 0, seed=73), ones, Batch(w, 30, 20, seed=74)]
    assert int(direct(w, ones)[0][0]) == 0
    with make_stream(w, depth=1, round_items=64, policy=N.STREAM_FULL_ROUNDS) as vs:
        for j, b in enumerate(seq):
            chk = submit(vs, b, host=host)[1]
            vs.flush()
            want = direct(w, b)
            assert b is ones or int(want[0][0]) == 1
            chk(want, j)
        assert vs.stats()["rounds"] == len(seq)


def test_four_threads_share_one_stream(world):
    w = world
    shapes = [(3, 17), (10, 20), (5, 0), (24, 1)]
    calls = [Batch(w, n, L, seed=80 + j) for j, (n, L) in enumerate(shapes)]
    wants = [direct(w, c) for c in calls]
    errors = []
    with make_stream(w, round_items=64) as vs:
        def work(j):
            try:
                for r in range(4):
                    submit(vs, calls[j], host=(j + r) % 2 == 0, sets_out=(r != 3))[1](wants[j], (j, r))
            except BaseException as e:      # noqa: BLE001 -- reported by the main thread
                errors.append((j, repr(e)))
        threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        st = vs.stats()
        assert st["calls"] == st["pieces"] == 16 and st["split_calls"] == 0


def test_refusals_and_interlocks(world):
    w = world
    lib = N.lib(); C = ctypes
    b = Batch(w, 8, 20, seed=90)
    want = direct(w, b)
    d_s, d_w, d_f, d_mi, d_r = dev(b.sig), dev(b.word), dev(b.bits), dev(b.midx), dev(b.rands)
    res = torch.zeros(8, dtype=torch.uint8, device=DEV)
    h_res = N.outbuf(8); h_st = (C.c_uint32 * 8)()
    t = C.c_uint64(0)
    p = lambda x: x.data_ptr()
    hp = lambda x: x.ctypes.data
    with make_stream(w) as vs, VerifyStream(w.ctx, committees=w.ct, msg_table=w.mt, bits_stride=STRIDE, round_items=256) as cs, \
            VerifyStream(w.ctx, table=w.kt, msg_table=w.mt, round_items=256) as ms, VerifyStream(w.ctx, round_items=256) as ps:
        # the other submit entries on a verify_multiple stream
        assert lib.mbls_stream_submit_device(vs.handle, p(d_s), p(d_f), 32, None, None, p(d_w), None, 8, 1, p(res), None, None, None, C.byref(t)) == N.ERR_ARGUMENT
        assert "mbls_stream_submit_vm" in vs.last_error()
        assert lib.mbls_stream_submit(vs.handle, hp(b.sig), hp(b.bits), 32, None, None, hp(b.word), None, 8, 1, h_res, h_st, C.byref(t)) == N.ERR_ARGUMENT
        assert lib.mbls_stream_submit_msgidx_device(vs.handle, p(d_s), p(d_mi), None, p(d_w), None, 8, 1, p(res), None, None, None, C.byref(t)) == N.ERR_ARGUMENT
        assert lib.mbls_stream_submit_msgidx(vs.handle, hp(b.sig), hp(b.midx), None, hp(b.word), None, 8, 1, h_res, h_st, C.byref(t)) == N.ERR_ARGUMENT
        assert "mbls_stream_submit_vm" in vs.last_error()
        assert lib.mbls_stream_submit_committee_device(vs.handle, p(d_s), p(d_mi), p(d_w), p(d_f), STRIDE, 8, p(res), None, None, None, C.byref(t)) == N.ERR_ARGUMENT
        assert "mbls_stream_submit_vm" in vs.last_error()
        assert lib.mbls_stream_submit_committee(vs.handle, hp(b.sig), hp(b.midx), hp(b.word), hp(b.bits), STRIDE, 8, h_res, h_st, C.byref(t)) == N.ERR_ARGUMENT
        assert "mbls_stream_submit_vm" in vs.last_error()
        # these submit entries on the other streams: the message names the right entry
        for other, name in ((cs, "mbls_stream_submit_committee"), (ms, "mbls_stream_submit_msgidx"), (ps, "mbls_stream_submit[_device]")):
            assert lib.mbls_stream_submit_vm_device(other.handle, p(d_s), p(d_w), p(d_f), STRIDE, p(d_mi), p(d_r), 8, p(res), None, None, None, None, C.byref(t)) == N.ERR_ARGUMENT
            assert name in other.last_error()
            assert lib.mbls_stream_submit_vm(other.handle, hp(b.sig), hp(b.word), hp(b.bits), STRIDE, hp(b.midx), hp(b.rands), 8, h_res, h_st, None, None, C.byref(t)) == N.ERR_ARGUMENT
            assert name in other.last_error() and other.stats()["calls"] == 0
        # no sets, no scalars, no result byte, a field longer than the stride, fields missing where bits_len says there are some
        dv = lambda n=8, rands=p(d_r), r=p(res), L=STRIDE, f=p(d_f): lib.mbls_stream_submit_vm_device(vs.handle, p(d_s), p(d_w), f, L, p(d_mi), rands, n, r, None, None, None, None, C.byref(t))
        hv = lambda n=8, rands=hp(b.rands), r=h_res, L=STRIDE, f=hp(b.bits): lib.mbls_stream_submit_vm(vs.handle, hp(b.sig), hp(b.word), f, L, hp(b.midx), rands, n, r, h_st, None, None, C.byref(t))
        for call in (dv, hv):
            assert call(n=0) == N.ERR_ARGUMENT and "at least one set" in vs.last_error()
            assert call(rands=None) == N.ERR_ARGUMENT and "rands" in vs.last_error()
            assert call(r=None) == N.ERR_ARGUMENT
            assert call(L=STRIDE + 1) == N.ERR_ARGUMENT and "bits_len" in vs.last_error()
            assert call(f=None) == N.ERR_ARGUMENT and "bits_len" in vs.last_error()
            assert call(n=256) == N.ERR_ARGUMENT and "256" in vs.last_error() and "round_items" in vs.last_error()
        assert t.value == 0 and vs.stats()["calls"] == 0
        submit(vs, b, host=False)[1](want)
    h = N.vp()
    mk = lambda ctx, ct, mt, stride, opts=None: lib.mbls_stream_create_vm_committee(ctx.handle, None if ct is None else ct.handle, None if mt is None else mt.handle, stride,
                                                                                    opts, C.byref(h))
    assert mk(w.ctx, w.ct, w.mt, 18) == N.ERR_ARGUMENT and "multiple of 4" in w.ctx.last_error()
    assert mk(w.ctx, w.ct, w.mt, 16) == N.ERR_ARGUMENT and "largest committee" in w.ctx.last_error()       # 128 bits, 130 members
    assert mk(w.ctx, None, w.mt, STRIDE) == N.ERR_ARGUMENT and mk(w.ctx, w.ct, None, STRIDE) == N.ERR_ARGUMENT
    one = N.StreamOpts(1, 0, 0, 0, 0)
    assert mk(w.ctx, w.ct, w.mt, STRIDE, C.byref(one)) == N.ERR_ARGUMENT                                   # no call fits a round of one item
    other = N.Context(0)
    try:
        assert mk(other, w.ct, w.mt, STRIDE) == N.ERR_ARGUMENT   # tables of another context
    finally:
        other.close()
    assert not h.value
    # the committee stream's interlocks with its tables
    ct = N.CommitteeTable(w.kt, capacity_hint=4)
    try:
        assert ct.append(w.members[1], [0, 7]) == 0
        seven = [i for i, it in enumerate(w.pool) if it.get("cid") == 1]
        c = Batch(w, 4, 1, seed=91)
        for j in range(4):
            i = seven[j % len(seven)]
            c.sig[j], c.word[j], c.midx[j], c.bits[j] = w.sig[i], 0, w.midx[i], w.bits[i]
        vs = VerifyStream(w.ctx, vm=True, committees=ct, msg_table=w.mt, bits_stride=STRIDE, round_items=64, policy=N.STREAM_FULL_ROUNDS)
        try:
            tk, chk = submit(vs, c, host=True)
            assert vs.query(tk) == N.PENDING
            for table in (ct, w.mt):                             # clear is refused while the call is pending ...
                with pytest.raises(N.MblsError) as e:
                    table.clear()
                assert e.value.code == N.ERR_ARGUMENT and "not completed" in str(e.value)
            vs.wait(tk)
            ct.clear()                                           # ... and accepted after the wait
            assert ct.append(w.members[1], [0, 7]) == 0
            with pytest.raises(N.MblsError) as e:                # a committee the stream's stride cannot hold
                ct.append(list(range(100)) + list(range(61)), [0, 161])
            assert e.value.code == N.ERR_ARGUMENT and "stride" in str(e.value) and len(ct) == 1
        finally:
            vs.close()
        assert ct.append(list(range(100)) + list(range(61)), [0, 161]) == 1
    finally:
        ct.close()


def test_python_mirror_submit_vm(world):
    """submit_vm takes the set tuples of verify_multiple_aggregate_signatures_committee, draws one scalar per set at submit in set order by the reference's rule,
    and answers (bool, list[bool]): the direct call with those scalars"""
    from milagro_bls_amd.api import Signature, SingleKey
    from milagro_bls_amd.stream import _reference_scalar
    w = world
    b = Batch(w, 9, 17, seed=95)

    def tuples(b):
        out = []
        for j, pi in enumerate(b.picks):
            it = w.pool[pi]
            if it["tag"] == "single":
                out.append((Signature(bytes(b.sig[j])), SingleKey(it["key"]), None, int(b.midx[j])))
            else:
                out.append((Signature(bytes(b.sig[j])), int(b.word[j]), bytes(b.bits[j, :(it["size"] + 7) // 8]), int(b.midx[j])))
        return out
    model = random.Random(4)
    b.rands = np.array([_reference_scalar(model) for _ in range(b.n)], dtype=np.uint64)
    replay = random.Random(4)
    assert b.rands.tolist() == [abs(int.from_bytes(bytes(replay.getrandbits(8) for _ in range(8)), "big", signed=True)) for _ in range(b.n)]
    want = direct(w, b)
    rng = random.Random(4)
    with make_stream(w) as vs:
        tk = vs.submit_vm(tuples(b), rng)
        assert tk.result() == (True, [True] * b.n) and int(want[0][0]) == 1
        assert rng.getstate() == model.getstate()               # one scalar per set, nothing else drawn
        # a signature outside G2 still consumes a scalar for every set
        b.sig[3] = w.not_in_g2
        model = random.Random(5); b.rands = np.array([_reference_scalar(model) for _ in range(b.n)], dtype=np.uint64)
        want = direct(w, b)
        rng = random.Random(5)
        tk = vs.submit_vm(tuples(b), rng)
        ok, per_set = tk.result()
        assert not ok and per_set == [bool(x) for x in want[2]] and not per_set[3] and sum(per_set) == b.n - 1
        assert tk.status() == (int(want[1][0]), want[3].tolist())
        assert rng.getstate() == model.getstate()
        with pytest.raises(ValueError):
            vs.submit_vm([], rng)
