"""GPU tests of the resident message table (include/mbls.h, "resident message table"): mbls_msgtable_* and the verification entries
mbls_fast_aggregate_verify_batch[_indexed]_msgtable[_device] / mbls_verify_batch_msgtable[_device]. Table contents are checked against mbls_hash_to_g2_batch byte for
byte; every verification is checked against the per-item entry on the same items with their messages spelled out (results, status words and bitmap bits identical)
and against the oracle. Inputs: tests/shared_msgs_cases.py; the per-item calls and the cached cases are those of tests/test_gpu_shared_msgs.py. Every test runs on
the three engines."""
import random

import pytest

import shared_msgs_cases as smc
from test_gpu_shared_msgs import case, cuts_case, dev_call, make_crossed, oracle_check_32, _msgs

pytestmark = pytest.mark.gpu

BAD = smc.ST_BAD_MSG_RANGE
RAGGED = [0, 1, 55, 56, 64, 200]


@pytest.fixture(scope="module")
def mb():
    from milagro_bls_amd import batch, _native
    _native.default_context()
    return batch


def new_table(msgs=None, capacity_hint=0):
    """a table on the default context, optionally holding `msgs` (any lengths) through the host append"""
    from milagro_bls_amd import _native as N
    mt = N.MsgTable(N.default_context(), capacity_hint=capacity_hint)
    if msgs:
        append(mt, msgs)
    return mt


def append(mt, msgs):
    off = [sum(len(m) for m in msgs[:j]) for j in range(len(msgs) + 1)]
    return mt.append(b"".join(msgs), len(msgs), msg_len=0, msg_offsets=off)


_POINTS = {}


def points(msgs):
    """mbls_hash_to_g2_batch of each message (one call per length), cached: the reference the table's contents are compared with"""
    from milagro_bls_amd import batch
    todo = [m for m in dict.fromkeys(msgs) if m not in _POINTS]
    by_len = {}
    for m in todo:
        by_len.setdefault(len(m), []).append(m)
    for L, ms in by_len.items():
        out = batch.hash_to_g2_batch(b"".join(ms), len(ms), msg_len=L)
        for j, m in enumerate(ms):
            _POINTS[m] = bytes(out[96 * j:96 * j + 96])
    return b"".join(_POINTS[m] for m in msgs)


def tab_call(cs, mt, *, verify=False, table=None, key_idx=None, idx=None, stream=None, sync=True):
    """the `_msgtable_device` entry with a bitmap and the caller's status array -> (results, status, bitmap bits)"""
    import torch
    from milagro_bls_amd import _native as N
    ctx = N.default_context(); dev = torch.device("cuda:0"); L = N.lib(); n = cs.n
    t = lambda b, dt=torch.uint8: torch.frombuffer(bytearray(b if b else b"\0"), dtype=dt).to(dev)
    d_s = t(cs.sigs)
    d_res = torch.full((n,), 9, dtype=torch.uint8, device=dev); d_bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), 0x7fffffff, dtype=torch.int32, device=dev)
    midx = cs.idx if idx is None else idx
    d_mi = torch.tensor([x if x < 2 ** 31 else x - 2 ** 32 for x in midx], dtype=torch.int32, device=dev)
    hs = stream.cuda_stream if stream is not None else None
    if stream is not None:
        torch.cuda.synchronize()                       # the inputs above are there; the call below is ordered by the library alone
    out = (d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), hs)
    if table is not None:
        d_k = torch.tensor(key_idx, dtype=torch.int32, device=dev)
        ctx.check(L.mbls_fast_aggregate_verify_batch_indexed_msgtable_device(ctx.handle, table.handle, d_s.data_ptr(), mt.handle, d_mi.data_ptr(), d_k.data_ptr(), None,
                                                                             n, cs.k, *out))
    elif verify:
        d_p = t(cs.pks)
        ctx.check(L.mbls_verify_batch_msgtable_device(ctx.handle, d_s.data_ptr(), mt.handle, d_mi.data_ptr(), d_p.data_ptr(), cs.fmt, n, *out))
    else:
        d_p = t(cs.pks)
        ctx.check(L.mbls_fast_aggregate_verify_batch_msgtable_device(ctx.handle, d_s.data_ptr(), mt.handle, d_mi.data_ptr(), d_p.data_ptr(), cs.fmt, None, n, cs.k, *out))
    if not sync:
        return d_res, d_st, d_bm, (d_s, d_mi)
    torch.cuda.synchronize()
    return read_out(n, d_res, d_st, d_bm)


def read_out(n, d_res, d_st, d_bm):
    got = [bool(x) for x in d_res.cpu().tolist()]
    bits = [(int(w) >> b) & 1 for w in d_bm.cpu().tolist() for b in range(64)][:n]
    return got, [x & 0xffffffff for x in d_st.cpu().tolist()], bits


def check_table(cs, mt, **kw):
    """table entry == per-item entry on the spelled-out messages (results, status, bitmap), == the oracle; the rejection kinds carry their bits"""
    new = tab_call(cs, mt, **kw)
    old = dev_call(cs, False, **kw)
    assert new == old, [(i, new[0][i], old[0][i], hex(new[1][i]), hex(old[1][i])) for i in range(cs.n) if (new[0][i], new[1][i]) != (old[0][i], old[1][i])][:8]
    got, st, bits = new
    assert got == cs.want
    assert bits == [int(x) for x in got]
    for i, kind in enumerate(cs.kinds):
        if kind == "valid":
            assert st[i] == 0, (i, hex(st[i]))
        elif kind in smc.FLAG:
            assert st[i] & smc.FLAG[kind], (i, kind, hex(st[i]))
    return new


def ragged_msgs():
    rnd = random.Random(14)
    return [rnd.randbytes(L) for L in RAGGED]


def test_table_contents_through_two_growths_and_a_verification_between(engine):
    """ragged messages of 0, 1, 55, 56, 64 and 200 bytes into a table of capacity_hint = 2, a verification, then 70 more: after each append every entry equals
    mbls_hash_to_g2_batch of its message, byte for byte; then items that name old and new entries"""
    from milagro_bls_amd import _native as N
    first_msgs = ragged_msgs()
    more = _msgs(70, 31)
    mt = N.MsgTable(N.default_context(), capacity_hint=2)
    try:
        assert len(mt) == 0 and append(mt, []) == 0
        assert append(mt, first_msgs) == 0 and len(mt) == 6
        pts, errs = mt.get(0, 6)
        assert pts == points(first_msgs) and errs == [0] * 6
        cs = case("ragged", lambda: (smc.build(26, 2, ragged_msgs(), [i % 6 for i in range(26)], seed=504), False))
        first = check_table(cs, mt)
        assert mt.append(b"".join(more), 70, msg_len=32) == 6 and len(mt) == 76
        pts, errs = mt.get(0, 76)
        assert pts == points(first_msgs + more) and errs == [0] * 76
        assert mt.get(75, 1) == (points(more[-1:]), [0]) and mt.get(76, 0) == (b"", [])
        assert check_table(cs, mt) == first
        both = case("old_and_new", lambda: (smc.build(20, 2, ragged_msgs() + _msgs(70, 31), [(i * 17 + 3) % 76 for i in range(20)], seed=530), False))
        assert {j < 6 for j in both.idx} == {True, False}
        check_table(both, mt)
    finally:
        mt.close()


def test_device_append_with_a_backwards_range_flags_that_entry_alone(engine):
    """the list's bytes are pad | message 2 | message 0 and the table 64, 96, 32, 64: entries 0 and 2 get their messages, entry 1 the range [96, 32). get reports it,
    its neighbours hold the right points, and exactly the items that name it are rejected with MBLS_ST_BAD_MSG_RANGE"""
    import torch
    from milagro_bls_amd import _native as N
    cs = case("crossed", make_crossed)
    base = dev_call(cs, False)
    dev = torch.device("cuda:0")
    d_m = torch.frombuffer(bytearray(bytes(32) + cs.msgs[2] + cs.msgs[0]), dtype=torch.uint8).to(dev)
    d_mo = torch.tensor([64, 96, 32, 64], dtype=torch.int64, device=dev)
    mt = N.MsgTable(N.default_context(), capacity_hint=8)
    try:
        assert mt.append_device(d_m.data_ptr(), 3, msg_len=0, d_msg_offsets=d_mo.data_ptr()) == 0
        pts, errs = mt.get(0, 3)
        assert errs == [0, N.ERR_ARGUMENT, 0]
        assert pts[:96] == points([cs.msgs[0]]) and pts[192:] == points([cs.msgs[2]])
        got, st, bits = tab_call(cs, mt)
        naming = {i for i in range(cs.n) if cs.idx[i] == 1}
        assert naming and len(naming) < cs.n
        for i in range(cs.n):
            if i in naming:
                # (checked against the empty message's point: where the item's own checks get that far, the pairing check fails as well)
                assert not got[i] and st[i] & BAD and not bits[i], (i, hex(st[i]))
                assert st[i] & ~(BAD | smc.ST_PAIRING_FAILED) == base[1][i] & ~smc.ST_PAIRING_FAILED, (i, hex(st[i]), hex(base[1][i]))
            else:
                assert (got[i], st[i], bits[i]) == (base[0][i], base[1][i], base[2][i]), i
    finally:
        mt.close()


def test_crossed_indices_device_and_host_and_indices_that_name_nothing(engine, mb):
    """n = 130, k = 2, three entries: item 0 names entry 2, item 2 names entry 0, item 5 is signed over another entry's message. Then indices `size` and 0xFFFFFFFF:
    only those items are rejected and only that bit is added; an empty table rejects every item."""
    cs = case("crossed", make_crossed)
    mt = new_table(cs.msgs)
    empty = new_table()
    try:
        got, st, bits = check_table(cs, mt)
        oracle_check_32(cs, got)
        assert cs.kinds[5] == "wrong_index" and not got[5] and st[5] == smc.ST_PAIRING_FAILED
        assert (cs.idx[0], cs.idx[2]) == (2, 0) and got[0] and got[2]
        assert mb.fast_aggregate_verify_batch_msgtable(mt, cs.sigs, cs.idx, cs.pks, cs.n, cs.k, pk_format=1) == (got, st)
        idx = list(cs.idx); idx[1] = len(mt); idx[66] = 0xFFFFFFFF
        g2, s2, b2 = tab_call(cs, mt, idx=idx)
        for i in range(cs.n):
            if i in (1, 66):
                assert not g2[i] and s2[i] & BAD and not b2[i], (i, hex(s2[i]))
                assert s2[i] & ~(BAD | smc.ST_PAIRING_FAILED) == st[i] & ~smc.ST_PAIRING_FAILED, (i, hex(s2[i]), hex(st[i]))
            else:
                assert (g2[i], s2[i], b2[i]) == (got[i], st[i], bits[i]), i
        # such an item is checked against the empty message's point: exactly what a per-item call with a backwards range gives it
        g0, s0, b0 = tab_call(cs, empty)
        assert len(empty) == 0 and not any(g0) and not any(b0) and all(s & BAD for s in s0)
        assert (g0[1], s0[1]) == (g2[1], s2[1]) and (g0[66], s0[66]) == (g2[66], s2[66])
    finally:
        mt.close(); empty.close()


def test_one_item(engine, mb):
    cs = case("one", lambda: (smc.build(1, 2, _msgs(1, 12), [0], seed=502), False))
    mt = new_table(cs.msgs)
    try:
        got, st, _ = check_table(cs, mt)
        assert got == [True] and st == [0]
        assert mb.fast_aggregate_verify_batch_msgtable(mt, cs.sigs, [0], cs.pks, 1, 2, pk_format=1) == (got, st)
    finally:
        mt.close()


def test_key_table_form_verify_form_and_48_byte_keys(engine, mb):
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    cs = case("table", lambda: (smc.build(70, 4, _msgs(5, 15), [(3 * i) % 5 for i in range(70)], seed=506), False))
    tab = N.KeyTable(ctx, capacity_hint=cs.n * cs.k)
    mt = new_table(cs.msgs)
    try:
        first, _ = tab.append(cs.pks, cs.n * cs.k, pk_format=1, validate=False)
        assert first == 0
        kidx = list(range(cs.n * cs.k))
        got, st, _ = check_table(cs, mt, table=tab, key_idx=kidx)
        oracle_check_32(cs, got)
        assert mb.fast_aggregate_verify_batch_indexed_msgtable(tab, mt, cs.sigs, cs.idx, kidx, cs.n, cs.k) == (got, st)
    finally:
        tab.close(); mt.close()
    cv = case("verify", lambda: (smc.build(67, 1, _msgs(4, 16), [(i * i) % 4 for i in range(67)], seed=507, fmt=0), True))
    mt = new_table(cv.msgs)
    try:
        got, st, _ = check_table(cv, mt, verify=True)
        oracle_check_32(cv, got, verify=True)
        assert mb.verify_batch_msgtable(mt, cv.sigs, cv.idx, cv.pks, cv.n) == (got, st)
    finally:
        mt.close()
    c48 = case("keys48", lambda: (smc.build(66, 3, _msgs(3, 19), [(2 * i + 1) % 3 for i in range(66)], seed=531, fmt=0), False))
    mt = new_table(c48.msgs)
    try:
        got, st, _ = check_table(c48, mt)
        assert mb.fast_aggregate_verify_batch_msgtable(mt, c48.sigs, c48.idx, c48.pks, c48.n, c48.k, pk_format=0) == (got, st)
    finally:
        mt.close()


def test_host_forms_refuse_a_bad_index_and_leave_the_outputs_alone(engine):
    import ctypes as C
    from milagro_bls_amd import _native as N
    ctx = N.default_context(); L = N.lib()
    cs = case("crossed", make_crossed)
    n = cs.n
    mt = new_table(cs.msgs)
    other = N.Context(0)
    try:
        def call(idx, c=ctx):
            res = (C.c_uint8 * n)(*([9] * n)); st = (C.c_uint32 * n)(*([0x7fffffff] * n))
            rc = L.mbls_fast_aggregate_verify_batch_msgtable(c.handle, N.cbuf(cs.sigs), mt.handle, (C.c_uint32 * n)(*idx), N.cbuf(cs.pks), 1, None, n, cs.k, res, st)
            return rc, list(res), list(st)

        for bad in (len(mt), 0xFFFFFFFF):
            idx = list(cs.idx); idx[1] = bad
            assert call(idx) == (N.ERR_ARGUMENT, [9] * n, [0x7fffffff] * n)
        assert call(cs.idx, other) == (N.ERR_ARGUMENT, [9] * n, [0x7fffffff] * n)       # a table of another context
        assert "another context" in other.last_error()
        rc, res, st = call(cs.idx)
        assert rc == N.OK and [bool(x) for x in res] == cs.want
        # the host append refuses a table that runs backwards, and nothing is appended
        moff = (C.c_uint64 * 4)(0, 32, 24, 96); first = C.c_uint64(77)
        assert L.mbls_msgtable_append(mt.handle, N.cbuf(cs.list_bytes), 0, moff, 3, C.byref(first)) == N.ERR_ARGUMENT
        assert len(mt) == 3 and first.value == 77
    finally:
        mt.close(); other.close()


@pytest.mark.parametrize("n,tracks", [(300, None), (300, 0), (276, 64), (165, None), (165, 0), (144, 64)])
def test_the_cuts_on_small_rounds(engine, mb, n, tracks):
    """rounds of 128 items: 300 items = two rounds + 44 (rounds, then the rest); with mbls_ctx_set_tracks(1, side_max) the two-halves mode (300 items) and the
    round-beside-rest mode (276 items, side_max = 64) where the engine's limits allow two tracks: every pass gathers from the table. Rounds of 64 items (165 = two
    rounds + 37 and 144 = two rounds + 16 items, a table of five messages): the same three modes through the device entry AND the host entry, and the first 32
    items against the oracle."""
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    small = n < 200
    cs = cuts_case(n)
    mt = new_table(cs.msgs)
    try:
        ctx.set_round_items(64 if small else 128)
        if tracks is not None:
            ctx.set_tracks(1, tracks)
        mode, passes, _ = N.plan_batch_shared_msgs(n, 0, ctx.limits())
        assert len(passes) >= 2 and all(p["message"] == N.MESSAGE_GATHER for p in passes)
        if tracks is None:
            assert mode == N.BATCH_ROUNDS_THEN_REST
        elif engine != "waves":
            assert mode == (N.BATCH_TWO_HALVES if tracks == 0 else N.BATCH_ROUND_BESIDE_REST)
        got, st, _ = check_table(cs, mt)
        if small:
            oracle_check_32(cs, got)
            assert mb.fast_aggregate_verify_batch_msgtable(mt, cs.sigs, cs.idx, cs.pks, cs.n, cs.k, pk_format=1) == (got, st)
    finally:
        ctx.reset_tuning(); mt.close()


def test_an_append_in_two_pieces(engine):
    """rounds of 64 items: 70 messages are hashed in two pieces (64 + 6) behind two entries the table holds already; items name entries of both pieces"""
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    cs = case("wide", lambda: (smc.build(3, 2, _msgs(70, 13), [69, 0, 64], seed=503, negatives=False), False))
    lead = _msgs(2, 32)
    mt = new_table(lead, capacity_hint=2)
    try:
        ctx.set_round_items(64)
        _, _, lst = N.plan_batch_shared_msgs(1, 70, ctx.limits())
        assert (lst["list_pieces"], lst["list_piece_items"]) == (2, 64)
        assert mt.append(cs.list_bytes, 70, msg_len=32) == 2
        ctx.reset_tuning()
        pts, errs = mt.get(0, 72)
        assert pts == points(lead + cs.msgs) and errs == [0] * 72
        got, st, bits = tab_call(cs, mt, idx=[j + 2 for j in cs.idx])
        assert (got, st, bits) == dev_call(cs, False) and got == [True] * 3
    finally:
        ctx.reset_tuning(); mt.close()


def test_append_on_one_stream_and_verify_on_another_without_a_host_synchronisation(engine):
    """the append is enqueued on stream A and the verification on stream B right behind it: B waits for A on the device. Then a second append on A and a second
    verification on B whose items are signed over, and name, the entries of BOTH appends: B has to wait for the second append as well."""
    import torch
    from milagro_bls_amd import _native as N
    cs = case("crossed", make_crossed)
    dev = torch.device("cuda:0")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    d_list = torch.frombuffer(bytearray(cs.list_bytes), dtype=torch.uint8).to(dev)
    late = _msgs(2, 33)
    d_late = torch.frombuffer(bytearray(b"".join(late)), dtype=torch.uint8).to(dev)
    want = dev_call(cs, False)
    both = case("cross_late", lambda: (smc.build(40, 2, _msgs(3, 11) + _msgs(2, 33), [(3 * i + 4) % 5 for i in range(40)], seed=532), False))
    assert both.msgs == cs.msgs + late and {3, 4} <= set(both.idx) and {0, 1, 2} <= set(both.idx)
    assert any(both.expect[i] and both.idx[i] >= 3 for i in range(both.n))          # accepted only if the late entry is there when the gather runs
    want_both = dev_call(both, False)
    mt = N.MsgTable(N.default_context(), capacity_hint=16)
    try:
        torch.cuda.synchronize()
        assert mt.append_device(d_list.data_ptr(), 3, msg_len=32, stream=sa.cuda_stream) == 0
        d_res, d_st, d_bm, keep = tab_call(cs, mt, stream=sb, sync=False)
        assert mt.append_device(d_late.data_ptr(), 2, msg_len=32, stream=sa.cuda_stream) == 3
        d_res2, d_st2, d_bm2, keep2 = tab_call(both, mt, stream=sb, sync=False)
        torch.cuda.synchronize()
        assert read_out(cs.n, d_res, d_st, d_bm) == want
        assert read_out(both.n, d_res2, d_st2, d_bm2) == want_both and want_both[0] == both.want
        pts, errs = mt.get(0, 5)
        assert pts == points(cs.msgs + late) and errs == [0] * 5
    finally:
        mt.close()


def test_clear_then_append_again_and_clear_under_a_stream(engine):
    """after clear index 0 names the next message appended; clear is refused while a stream bound to the table has an unflushed call and succeeds after wait"""
    import torch
    from milagro_bls_amd import _native as N
    from milagro_bls_amd.stream import VerifyStream
    ctx = N.default_context()
    cs = case("crossed", make_crossed)
    dev = torch.device("cuda:0")
    mt = new_table(_msgs(3, 34), capacity_hint=8)
    try:
        g0, s0, _ = tab_call(cs, mt)                      # other messages under the same indices: every pairing check fails
        assert not any(g0) and all(s & smc.ST_PAIRING_FAILED for i, s in enumerate(s0) if cs.kinds[i] == "valid")
        mt.clear()
        assert len(mt) == 0
        assert append(mt, cs.msgs) == 0
        want = check_table(cs, mt)
        with VerifyStream(ctx, pk_format=N.PK_UNCOMPRESSED, msg_table=mt, round_items=256, policy=N.STREAM_FULL_ROUNDS) as vs:
            t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
            d_s, d_p = t(cs.sigs), t(cs.pks)
            d_mi = torch.tensor(cs.idx, dtype=torch.int32, device=dev)
            d_res = torch.full((cs.n,), 9, dtype=torch.uint8, device=dev)
            tk = vs.submit_device(d_s, d_mi, d_p, cs.n, cs.k, d_res)
            with pytest.raises(N.MblsError) as e:
                mt.clear()
            assert e.value.code == N.ERR_ARGUMENT and "not completed" in ctx.last_error()
            assert len(mt) == 3
            vs.wait(tk)
            assert [bool(x) for x in d_res.cpu().tolist()] == want[0]
            mt.clear()
            assert len(mt) == 0
    finally:
        mt.close()
