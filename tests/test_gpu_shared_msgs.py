"""GPU tests of the shared-message entries (include/mbls.h, "shared message lists"): mbls_fast_aggregate_verify_batch[_indexed]_shared_msgs[_device] and
mbls_verify_batch_shared_msgs[_device]. Every case is checked twice: against the entry without `_shared_msgs` on the same items with their messages spelled out
(results, status words and bitmap bits identical) and against the oracle (results). Inputs: tests/shared_msgs_cases.py. Every test runs on the three engines."""
import random

import pytest

import helpers
import shared_msgs_cases as smc

pytestmark = pytest.mark.gpu

BAD = smc.ST_BAD_MSG_RANGE


@pytest.fixture(scope="module")
def mb():
    from milagro_bls_amd import batch, _native
    _native.default_context()
    return batch


def _msgs(count, seed, length=32):
    rnd = random.Random(seed)
    return [rnd.randbytes(length) for _ in range(count)]


_CACHE = {}


def case(name, make):
    """inputs and the oracle's verdicts are computed once and shared by the engines"""
    if name not in _CACHE:
        cs, verify = make()
        cs.want = smc.oracle(cs, verify=verify)
        assert cs.want == cs.expect, [i for i in range(cs.n) if cs.want[i] != cs.expect[i]][:8]
        _CACHE[name] = cs
    return _CACHE[name]


def oracle_check_32(cs, got, verify=False):
    """the suite's own oracle check (helpers.oracle_check_fav / oracle_check_verify) on the spelled-out 32-byte messages"""
    import torch
    sz = 48 if cs.fmt == 0 else 96
    t = lambda b, *shape: torch.frombuffer(bytearray(b), dtype=torch.uint8).reshape(*shape)
    idx = list(range(cs.n))
    exp, g = torch.tensor([int(x) for x in cs.expect]), torch.tensor([int(x) for x in got])
    if verify:
        helpers.oracle_check_verify(t(cs.sigs, cs.n, 96), t(cs.spelled_bytes, cs.n, 32), t(cs.pks, cs.n, sz), idx, exp, g)
    else:
        helpers.oracle_check_fav(t(cs.sigs, cs.n, 96), t(cs.spelled_bytes, cs.n, 32), t(cs.pks, cs.n, cs.k, sz), idx, cs.k, cs.fmt, exp, g)


def dev_call(cs, shared, *, verify=False, table=None, key_idx=None, idx=None, n_msgs=None, list_offsets=None, list_bytes=None, force_offsets=False):
    """the device entry (shared list or per-item messages) with a bitmap and the caller's status array -> (results, status, bitmap bits)"""
    import torch
    from milagro_bls_amd import _native as N
    ctx = N.default_context(); dev = torch.device("cuda:0"); L = N.lib(); n = cs.n
    t = lambda b, dt=torch.uint8: torch.frombuffer(bytearray(b if b else b"\0"), dtype=dt).to(dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    d_s = t(cs.sigs)
    d_res = torch.full((n,), 9, dtype=torch.uint8, device=dev); d_bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), 0x7fffffff, dtype=torch.int32, device=dev)
    out = (d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None)
    ragged = force_offsets or not cs.uniform or list_offsets is not None
    if shared:
        d_m = t(cs.list_bytes if list_bytes is None else list_bytes)
        d_mo = i64(list_offsets if list_offsets is not None else cs.list_offsets) if ragged else None
        midx = cs.idx if idx is None else idx
        d_mi = torch.tensor([x if x < 2 ** 31 else x - 2 ** 32 for x in midx], dtype=torch.int32, device=dev)
        nm = cs.n_msgs if n_msgs is None else n_msgs
        margs = (d_m.data_ptr(), cs.msg_len, d_mo.data_ptr() if ragged else None, nm, d_mi.data_ptr())
    else:
        d_m = t(cs.spelled_bytes)
        d_mo = i64(cs.spelled_offsets) if ragged else None
        margs = (d_m.data_ptr(), cs.msg_len, d_mo.data_ptr() if ragged else None)
    if table is not None:
        d_k = torch.tensor(key_idx, dtype=torch.int32, device=dev)
        f = L.mbls_fast_aggregate_verify_batch_indexed_shared_msgs_device if shared else L.mbls_fast_aggregate_verify_batch_indexed_device
        ctx.check(f(ctx.handle, table.handle, d_s.data_ptr(), *margs, d_k.data_ptr(), None, n, cs.k, *out))
    elif verify:
        d_p = t(cs.pks)
        f = L.mbls_verify_batch_shared_msgs_device if shared else L.mbls_verify_batch_device
        ctx.check(f(ctx.handle, d_s.data_ptr(), *margs, d_p.data_ptr(), cs.fmt, n, *out))
    else:
        d_p = t(cs.pks)
        f = L.mbls_fast_aggregate_verify_batch_shared_msgs_device if shared else L.mbls_fast_aggregate_verify_batch_device
        ctx.check(f(ctx.handle, d_s.data_ptr(), *margs, d_p.data_ptr(), cs.fmt, None, n, cs.k, *out))
    torch.cuda.synchronize()
    got = [bool(x) for x in d_res.cpu().tolist()]
    bits = [(int(w) >> b) & 1 for w in d_bm.cpu().tolist() for b in range(64)][:n]
    return got, [x & 0xffffffff for x in d_st.cpu().tolist()], bits


def check_both(cs, **kw):
    """shared list == per-item entry (results, status, bitmap), == the oracle; the rejection kinds carry their bits"""
    new = dev_call(cs, True, **kw)
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


def make_crossed():
    n = 130
    msgs = _msgs(3, 11)
    idx = [2, 1, 0] + [(7 * i + 1) % 3 for i in range(3, n)]      # item 0 names message 2, item 2 names message 0
    return smc.build(n, 2, msgs, idx, seed=501, signed_as={5: (idx[5] + 1) % 3}), False


def test_two_waves_and_a_partial_one_crossed_indices(engine, mb):
    """n = 130, k = 2, three messages: item 0 names message 2 while item 2 names message 0 (no in-place copy could serve both), and item 5's signature is over
    another message than its index names: result 0 with MBLS_ST_PAIRING_FAILED. Device and host entries."""
    cs = case("crossed", make_crossed)
    got, st, _ = check_both(cs)
    oracle_check_32(cs, got)
    assert cs.kinds[5] == "wrong_index" and not got[5] and st[5] == smc.ST_PAIRING_FAILED
    assert (cs.idx[0], cs.idx[2]) == (2, 0) and got[0] and got[2]
    hgot, hst = mb.fast_aggregate_verify_batch_shared_msgs(cs.sigs, cs.list_bytes, 3, cs.idx, cs.pks, cs.n, cs.k, pk_format=1)
    assert (hgot, hst) == (got, st)


def test_one_item_one_message(engine, mb):
    cs = case("one", lambda: (smc.build(1, 2, _msgs(1, 12), [0], seed=502), False))
    got, st, _ = check_both(cs)
    assert got == [True] and st == [0]
    assert mb.fast_aggregate_verify_batch_shared_msgs(cs.sigs, cs.list_bytes, 1, [0], cs.pks, 1, 2, pk_format=1) == (got, st)


def test_more_messages_than_items_and_the_list_in_pieces(engine):
    """n = 3 over a list of 70 messages (67 of them unused): the workspace is sized by the list, not by the items; with rounds of 64 items the list is hashed in two
    pieces (64 + 6 messages) and the items name messages of both."""
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    cs = case("wide", lambda: (smc.build(3, 2, _msgs(70, 13), [69, 0, 64], seed=503, negatives=False), False))
    first = check_both(cs)
    assert first[0] == [True] * 3
    try:
        ctx.set_round_items(64)
        _, _, lst = N.plan_batch_shared_msgs(3, 70, ctx.limits())
        assert (lst["list_pieces"], lst["list_piece_items"]) == (2, 64)
        assert check_both(cs) == first
    finally:
        ctx.reset_tuning()


def test_ragged_list_at_the_sha256_padding_edges_and_empty_messages(engine, mb):
    """messages of 0, 1, 55, 56, 64 and 200 bytes through msg_offsets; a list of zero-length messages through msg_len = 0"""
    lens = [0, 1, 55, 56, 64, 200]
    rnd = random.Random(14)
    cs = case("ragged", lambda: (smc.build(26, 2, [rnd.randbytes(L) for L in lens], [i % 6 for i in range(26)], seed=504), False))
    got, st, _ = check_both(cs)
    assert mb.fast_aggregate_verify_batch_shared_msgs(cs.sigs, cs.list_bytes, 6, cs.idx, cs.pks, cs.n, cs.k, pk_format=1, msg_offsets=cs.list_offsets) == (got, st)
    ce = case("empty", lambda: (smc.build(9, 2, [b"", b""], [i % 2 for i in range(9)], seed=505), False))
    assert ce.uniform and ce.msg_len == 0
    check_both(ce)


def test_key_table_form_and_verify_form(engine, mb):
    """keys by table index and messages by list index; Signature::verify (one 48-byte key, no infinity test) over a list"""
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    cs = case("table", lambda: (smc.build(70, 4, _msgs(5, 15), [(3 * i) % 5 for i in range(70)], seed=506), False))
    tab = N.KeyTable(ctx, capacity_hint=cs.n * cs.k)
    try:
        first, _ = tab.append(cs.pks, cs.n * cs.k, pk_format=1, validate=False)
        assert first == 0
        kidx = list(range(cs.n * cs.k))
        got, st, _ = check_both(cs, table=tab, key_idx=kidx)
        oracle_check_32(cs, got)
        assert mb.fast_aggregate_verify_batch_indexed_shared_msgs(tab, cs.sigs, cs.list_bytes, 5, cs.idx, kidx, cs.n, cs.k) == (got, st)
    finally:
        tab.close()
    cv = case("verify", lambda: (smc.build(67, 1, _msgs(4, 16), [(i * i) % 4 for i in range(67)], seed=507, fmt=0), True))
    got, st, _ = check_both(cv, verify=True)
    oracle_check_32(cv, got, verify=True)
    assert mb.verify_batch_shared_msgs(cv.sigs, cv.list_bytes, 4, cv.idx, cv.pks, cv.n) == (got, st)


def test_device_entry_rejects_an_index_that_names_no_message(engine):
    """msg_idx = n_msgs and 0xFFFFFFFF: result 0 and MBLS_ST_BAD_MSG_RANGE for those items, their neighbours untouched; the same with an empty list"""
    cs = case("crossed", make_crossed)
    base = dev_call(cs, True)
    idx = list(cs.idx); idx[1] = cs.n_msgs; idx[66] = 0xFFFFFFFF
    got, st, bits = dev_call(cs, True, idx=idx)
    for i in range(cs.n):
        if i in (1, 66):
            assert not got[i] and st[i] & BAD and not bits[i], (i, hex(st[i]))
        else:
            assert (got[i], st[i], bits[i]) == (base[0][i], base[1][i], base[2][i]), i
    got, st, bits = dev_call(cs, True, n_msgs=0)
    assert not any(got) and not any(bits) and all(s & BAD for s in st)


def test_device_entry_rejects_the_items_of_a_message_with_a_bad_range(engine):
    """one listed message's range runs backwards: every item that names it is rejected with MBLS_ST_BAD_MSG_RANGE, no other item is touched. The list's bytes are
    laid out as pad | message 2 | message 0, so that the table 64, 96, 32, 64 gives messages 0 and 2 their bytes and message 1 the range [96, 32)."""
    cs = case("crossed", make_crossed)
    base = dev_call(cs, True)
    assert base == dev_call(cs, True, force_offsets=True)
    got, st, bits = dev_call(cs, True, list_bytes=bytes(32) + cs.msgs[2] + cs.msgs[0], list_offsets=[64, 96, 32, 64])
    naming = {i for i in range(cs.n) if cs.idx[i] == 1}
    assert naming and len(naming) < cs.n
    for i in range(cs.n):
        if i in naming:
            assert not got[i] and st[i] & BAD and not bits[i], (i, hex(st[i]))
        else:
            assert (got[i], st[i], bits[i]) == (base[0][i], base[1][i], base[2][i]), i


def test_host_entries_refuse_bad_tables_and_leave_the_outputs_alone(engine):
    import ctypes as C
    from milagro_bls_amd import _native as N
    ctx = N.default_context(); L = N.lib()
    cs = case("crossed", make_crossed)
    n = cs.n

    def call(idx, moff):
        res = (C.c_uint8 * n)(*([9] * n)); st = (C.c_uint32 * n)(*([0x7fffffff] * n))
        mo = None if moff is None else (C.c_uint64 * len(moff))(*moff)
        rc = L.mbls_fast_aggregate_verify_batch_shared_msgs(ctx.handle, N.cbuf(cs.sigs), N.cbuf(cs.list_bytes), 32, mo, cs.n_msgs, (C.c_uint32 * n)(*idx),
                                                            N.cbuf(cs.pks), 1, None, n, cs.k, res, st)
        return rc, list(res), list(st)

    for bad in (cs.n_msgs, 0xFFFFFFFF):
        idx = list(cs.idx); idx[1] = bad
        assert call(idx, None) == (N.ERR_ARGUMENT, [9] * n, [0x7fffffff] * n)
    assert call(cs.idx, [0, 32, 24, 96]) == (N.ERR_ARGUMENT, [9] * n, [0x7fffffff] * n)
    rc, res, st = call(cs.idx, None)
    assert rc == N.OK and [bool(x) for x in res] == cs.want


def cuts_case(n):
    """the items of test_the_cuts_on_small_rounds (here and in tests/test_gpu_msgtable.py): below 200 items a list of 5 messages for rounds of 64 items, else 4 for 128"""
    if n < 200:
        return case("cuts%d" % n, lambda: (smc.build(n, 2, _msgs(5, 17), [(3 * i + i // 64) % 5 for i in range(n)], seed=508 + n), False))
    return case("cuts%d" % n, lambda: (smc.build(n, 2, _msgs(4, 17), [(5 * i + i // 64) % 4 for i in range(n)], seed=508 + n), False))


@pytest.mark.parametrize("n,tracks", [(300, None), (300, 0), (276, 64), (165, None), (165, 0), (144, 64)])
def test_the_cuts_on_small_rounds(engine, mb, n, tracks):
    """rounds of 128 items: 300 items = two rounds + 44 (rounds, then the rest); with mbls_ctx_set_tracks(1, side_max) the two-halves mode (300 items) and the
    round-beside-rest mode (276 items, side_max = 64) where the engine's limits allow two tracks -- the list of four messages is hashed once, before the first pass.
    Rounds of 64 items (165 = two rounds + 37 and 144 = two rounds + 16 items, five messages): the same three modes through the device entries AND the host entries,
    with the list and with the messages spelled out (the host entry that takes per-item messages queues its rounds in two parts around the key upload and the rest
    as one pass behind them, whatever the tracks), and the first 32 items against the oracle."""
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    small = n < 200
    cs = cuts_case(n)
    try:
        ctx.set_round_items(64 if small else 128)
        if tracks is not None:
            ctx.set_tracks(1, tracks)
        mode, passes, lst = N.plan_batch_shared_msgs(n, cs.n_msgs, ctx.limits())
        assert len(passes) >= 2 and all(p["message"] == N.MESSAGE_GATHER for p in passes) and lst["list_pieces"] == 1
        if tracks is None:
            assert mode == N.BATCH_ROUNDS_THEN_REST
        elif engine != "waves":
            assert mode == (N.BATCH_TWO_HALVES if tracks == 0 else N.BATCH_ROUND_BESIDE_REST)
        got, st, _ = check_both(cs)
        if small:
            oracle_check_32(cs, got)
            assert mb.fast_aggregate_verify_batch_shared_msgs(cs.sigs, cs.list_bytes, cs.n_msgs, cs.idx, cs.pks, cs.n, cs.k, pk_format=1) == (got, st)
            assert mb.fast_aggregate_verify_batch(cs.sigs, cs.spelled_bytes, cs.pks, cs.n, cs.k, pk_format=1) == (got, st)
    finally:
        ctx.reset_tuning()


def test_two_calls_back_to_back_with_a_shorter_second_list(engine):
    """the second call's list is shorter and different: no point of the first call's table survives into it"""
    a = case("crossed", make_crossed)
    b = case("second", lambda: (smc.build(40, 2, _msgs(2, 18), [i % 2 for i in range(40)], seed=520), False))
    first = dev_call(a, True)
    second = dev_call(b, True)
    assert first[0] == a.want
    assert second == dev_call(b, False) and second[0] == b.want
