"""GPU tests of mbls_verify_multiple*_msgtable* (include/mbls.h, "verify_multiple OVER THE RESIDENT MESSAGE TABLE"): the sets' messages named by index into a
resident message table, nothing hashed, the entries a call names found on the device. Every verdict is judged against the existing entry
mbls_verify_multiple_aggregate_signatures_device on the same sets with each set's message spelled out and the same scalars -- equal result byte, equal status
word in the bits that reject a batch -- and, up to 40 sets, against the oracle. Modes 1 and 2 in every case, mode 0 on each side of the auto condition; the
key-table-indexed form on the same cases as its apk twin. The per-set answers: tests/test_gpu_vm_msgtable_locate.py."""
import ctypes as C
import random

import numpy as np
import pytest

import helpers
import orc
import test_gpu_vm_shared_locate as SL
import test_gpu_vm_shared_msgs as SM
import vm_msgtable_cases as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from milagro_bls_amd import _native
    _native.default_context()
    return _native


@pytest.fixture(scope="module")
def probe(vectors):
    return bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])


# ------------------------------------------------------------------------------------------------ the shapes, valid and with every defect
@pytest.mark.parametrize("name", V.SHAPES)
def test_valid_shapes_and_routes(N, name):
    """every entry named (T = D = 12); 9 entries of a 2 500-entry table (entry 0, entry 2 499 and two neighbours among them); one entry named by all sets; one
    set per entry: the judge's verdict under every mode and both key forms, and the routes the plan function names"""
    c, d, mt = V.built(N, name)
    assert V.check_verdict(N, c, d, mt, want=True)[1] & V.REJECT_BATCH == 0
    T, D = len(c.listed), len(set(c.idx))
    dev, host = N.plan_verify_multiple_msgtable(c.n, T, 0, 0), N.plan_verify_multiple_msgtable(c.n, T, D, 0)
    assert dev["route"] == (N.VM_ROUTE_GROUPED if 2 * min(c.n, T) <= c.n else N.VM_ROUTE_PER_SET)
    assert host["route"] == (N.VM_ROUTE_GROUPED if 2 * D <= c.n else N.VM_ROUTE_PER_SET)
    if name == "sparse_9_of_2500":
        assert dev["route"] == N.VM_ROUTE_PER_SET and dev["miller_items"] == 150
        assert host["route"] == N.VM_ROUTE_GROUPED and host["miller_items"] == 9
        assert {0, 2499, 1200, 1201} <= set(c.idx) and D == 9
        forced = N.plan_verify_multiple_msgtable(c.n, T, 0, 1)
        assert forced["route"] == N.VM_ROUTE_GROUPED and forced["miller_items"] == 150


@pytest.mark.parametrize("kind", V.DEFECTS + ("three",))
@pytest.mark.parametrize("name", ["every_entry_of_12", "sparse_9_of_2500"])
def test_defects(N, probe, name, kind):
    """each defect of the shared-message tests alone on one set, and three together: the judge's verdict and rejecting bits, every mode, both key forms"""
    c, _d, mt = V.built(N, name)
    rnd = random.Random(V.hash_name(name + kind))
    if kind == "three":
        b = c
        for k, i in zip(("wrong_key", "not_in_g2", "zero_scalar"), rnd.sample(range(c.n), 3)):
            b = V.with_defect(b, k, i, probe)
    else:
        b = V.with_defect(c, kind, rnd.randrange(c.n), probe)
    r0, s0 = V.check_verdict(N, b, SL.DevCase(N, b, table=True), mt, want=(kind == "both_inf"))
    if kind in ("not_in_g2", "undecodable", "zero_scalar", "three"):
        assert s0 & V.REJECT_BATCH


def test_forty_sets_against_the_oracle(N, probe):
    """40 sets over 6 of 12 entries: the oracle with the same scalars, valid and with a wrong key"""
    listed = V.messages(11, 12)
    rnd = random.Random(40)
    idx = [0, 11, 5, 6, 2, 9] + [rnd.choice([0, 11, 5, 6, 2, 9]) for _ in range(34)]
    c = V.base_case(listed, idx, 41)
    mt = V.make_table(N, listed)
    try:
        for case in (c, V.with_defect(c, "wrong_key", 17, probe)):
            dec = [orc.g2_from_compressed(s)[1] for s in case.sigs]
            want = orc.verify_multiple([(s, a, m) for s, a, m in zip(dec, case.apks, case.spelled())], case.rands)
            assert want == (case is c)
            V.check_verdict(N, case, SL.DevCase(N, case, table=True), mt, want=want)
    finally:
        mt.close()


def test_coincident_points_inside_a_group(N):
    """the pool of tests/edge_points.py over its handful of messages, now entries of a table: a pair (sig, pk, m) / (-sig, -pk, m) under one scalar in one group,
    keys shifted by torsion points, pure-torsion sets -- the judge's verdict as drawn and with one set renamed to another entry"""
    c = SM._coincidence_case(300)
    mt = V.make_table(N, c.listed)
    try:
        d = SM.DevCase(c)
        d.tab = None
        assert V.check_verdict(N, c, d, mt, modes=(1, 2), indexed=(False,))[0] == 1
        i = next(i for i in range(100, 300) if c.sigs[i] != helpers.G2_INF)
        b = SM.Case()
        b.listed, b.sigs, b.apks, b.rands, b.wire = c.listed, c.sigs, c.apks, c.rands, None
        b.idx = list(c.idx); b.idx[i] = (c.idx[i] + 1) % len(c.listed)
        d = SM.DevCase(b)
        assert V.check_verdict(N, b, d, mt, modes=(1, 2), indexed=(False,))[0] == 0
    finally:
        mt.close()


# ------------------------------------------------------------------------------------------------ index faults
def test_index_faults(N):
    """a set naming T or 2^32 - 1 rejects the call with MBLS_ST_BAD_MSG_RANGE; an empty table rejects every call that names anything; n = 0 accepts"""
    c, d, mt = V.built(N, "every_entry_of_12")
    T = len(c.listed)
    empty = N.MsgTable(capacity_hint=4)
    try:
        for mode in (1, 2, 0):
            for ix in (False, True):
                for bad in (T, V.NO_ENTRY):
                    idx = list(c.idx); idx[17] = bad
                    r, s = V.call_table(N, d, mt, mode, False, ix, idx=V.dev_idx(idx))
                    assert r == 0 and s & V.ST_BAD_MSG_RANGE, (mode, ix, bad, r, hex(s))
                r, s = V.call_table(N, d, empty, mode, False, ix)
                assert r == 0 and s & V.ST_BAD_MSG_RANGE, (mode, ix, r, hex(s))
        # n = 0: accepted, status 0, over the full and over the empty table
        ctx = N.default_context()
        for t in (mt, empty):
            res, st, _a, _b = out = V.bufs(1)
            assert N.lib().mbls_verify_multiple_msgtable_device(ctx.handle, None, None, t.handle, None, None, 0, res.data_ptr(), st.data_ptr(), None) == 0
            assert V.read(1, out, False) == (1, 0)
        # refused: no scalars, no table, a table of another context
        res, st, _a, _b = out = V.bufs(1)
        f = N.lib().mbls_verify_multiple_msgtable_device
        assert f(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), mt.handle, d.idx.data_ptr(), None, d.n, res.data_ptr(), st.data_ptr(), None) == N.ERR_ARGUMENT
        assert f(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), None, d.idx.data_ptr(), d.rands.data_ptr(), d.n, res.data_ptr(), st.data_ptr(), None) == N.ERR_ARGUMENT
        other = N.Context(0)
        foreign = N.MsgTable(ctx=other, capacity_hint=4)
        try:
            assert f(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), foreign.handle, d.idx.data_ptr(), d.rands.data_ptr(), d.n, res.data_ptr(), st.data_ptr(),
                     None) == N.ERR_ARGUMENT
        finally:
            foreign.close()
        assert V.read(1, out, False) == (7, 0xFFFFFFFF)
    finally:
        empty.close()


def test_flagged_entry(N):
    """an entry appended through append_device with a backwards offset pair: present but unnamed it changes nothing, named by one set it rejects the call"""
    c, d, _mt = V.built(N, "every_entry_of_12")
    T = len(c.listed)
    mt = V.make_table(N, c.listed)
    try:
        raw = SL._dev(bytes(64)); off = SL._dev(np.array([40, 8], dtype=np.uint64))
        assert mt.append_device(raw.data_ptr(), 1, msg_len=0, d_msg_offsets=off.data_ptr()) == T
        assert mt.get(T, 1)[1] == [N.ERR_ARGUMENT]
        V.check_verdict(N, c, d, mt, want=True)
        idx = list(c.idx); idx[33] = T
        for mode in (1, 2, 0):
            for ix in (False, True):
                r, s = V.call_table(N, d, mt, mode, False, ix, idx=V.dev_idx(idx))
                assert r == 0 and s & V.ST_BAD_MSG_RANGE, (mode, ix, r, hex(s))
    finally:
        mt.close()


# ------------------------------------------------------------------------------------------------ table life
def test_table_life(N):
    """a table created with capacity_hint = 1 and grown by appends (relayout) before the call; two calls back to back over one table; clear, other messages
    re-appended, the call again"""
    c, d, _mt = V.built(N, "every_entry_of_12")
    mt = V.make_table(N, c.listed, capacity_hint=1, pieces=4)
    try:
        V.check_verdict(N, c, d, mt, want=True)
        from milagro_bls_amd import batch
        for mode in (1, 2):
            batch.set_vm_grouping(mode)
            a = V.enqueue_table(N, d, mt, False)
            b = V.enqueue_table(N, d, mt, False, indexed=True)
            assert V.read(d.n, a, False)[0] == 1 and V.read(d.n, b, False)[0] == 1
        batch.set_vm_grouping(0)
        mt.clear()
        assert len(mt) == 0
        listed2, idx2 = V.shape("one_entry_for_all")
        c2 = V.base_case(listed2, idx2, 77)
        assert mt.append(b"".join(listed2), len(listed2), msg_len=0, msg_offsets=SL._offsets(listed2)) == 0
        V.check_verdict(N, c2, SL.DevCase(N, c2, table=True), mt, want=True)
        # the first case names entries that now hold other messages (or none): rejected
        for mode in (1, 2):
            assert V.call_table(N, d, mt, mode, False)[0] == 0
    finally:
        N.lib().mbls_ctx_set_vm_grouping(N.default_context().handle, 0)
        mt.close()


def test_append_on_another_stream_right_before_the_call(N):
    """the table's event is awaited on the caller's stream: an append enqueued on stream A, the call on stream B, no host synchronisation in between"""
    import torch
    from milagro_bls_amd import batch
    c, d, _mt = V.built(N, "every_entry_of_12")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    d_list = SL._dev(b"".join(c.listed)); d_off = SL._dev(np.array(SL._offsets(c.listed), dtype=np.uint64))
    torch.cuda.synchronize()
    for mode in (1, 2):
        mt = N.MsgTable(capacity_hint=64)
        try:
            batch.set_vm_grouping(mode)
            assert mt.append_device(d_list.data_ptr(), len(c.listed), msg_len=0, d_msg_offsets=d_off.data_ptr(), stream=sa.cuda_stream) == 0
            out = V.enqueue_table(N, d, mt, False, stream=sb.cuda_stream)
            assert V.read(d.n, out, False) == (1, 0), mode
        finally:
            batch.set_vm_grouping(0)
            mt.close()


# ------------------------------------------------------------------------------------------------ Miller forms at small size, the early exit
def _tuned(N, coop_max=None, round_items=None):
    ctx = N.default_context()
    if round_items is not None:
        assert N.lib().mbls_ctx_set_round_items(ctx.handle, round_items) == 0
    if coop_max is not None:
        assert N.lib().mbls_ctx_set_coop_max_items(ctx.handle, coop_max) == 0


FORMS = [("20_of_20", 0, None, "PAIRING_LANES2", 0), ("20_of_40", 0, 64, "PAIRING_LANE", 0), ("70_of_70", 0, 64, "PAIRING_LANES2", 1), ("5_of_600", None, None, "PAIRING_WAVE", 0),
         ("5_of_600", 0, 64, "PAIRING_LANES2", 2)]


@pytest.mark.parametrize("name,coop_max,round_items,form,rounds", FORMS, ids=["lane_pairs", "lanes", "cut_at_a_round", "waves_5_of_150_live", "lanes_5_of_150_live"])
def test_miller_forms(N, probe, name, coop_max, round_items, form, rounds):
    """mode 1 on the device entries: 20 named entries on lane pairs; 20 named among 40 Miller items on one lane each; 70 Miller items cut at a round of 64;
    and T = 600 > D = 5 -- 150 Miller items of which 5 are live, the other waves return before any arithmetic -- on the wave form and on lanes (two rounds of 64
    and a rest on lane pairs, all of the second round and the rest idle). Valid and with a wrong key,
    against the judge under the same tuning; the Miller form is the plan function's under the same limits"""
    listed, idx = V.shape(name)
    c = V.base_case(listed, idx, V.hash_name(name))
    mt = V.make_table(N, listed)
    ctx = N.default_context()
    try:
        _tuned(N, coop_max, round_items)
        L = N.Limits()
        assert N.lib().mbls_ctx_get_limits(ctx.handle, C.byref(L)) == 0
        p = N.plan_verify_multiple_msgtable(c.n, len(listed), 0, 1, limits=L)
        assert p["route"] == N.VM_ROUTE_GROUPED and p["miller_items"] == min(c.n, len(listed))
        assert (p["miller"], p["miller_rounds"]) == (getattr(N, form), rounds), p
        for case in (c, V.with_defect(c, "wrong_key", 5, probe)):
            V.check_verdict(N, case, SL.DevCase(N, case, table=True), mt, modes=(1, 2), want=case is c)
    finally:
        ctx.reset_tuning()
        mt.close()


# ------------------------------------------------------------------------------------------------ the reference's RNG order, the Python API
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_rng_entries_and_api(N, probe, mode):
    """the _rng entry and the API methods against AggregateSignature.verify_multiple_aggregate_signatures on the spelled-out sets: same bool, the generator left
    in the same state -- valid, and with the third signature outside G2, where the draws stop; the host entry takes the grouped route for 9 entries of 2 500
    (the plan function with the count) and refuses an index that names no entry"""
    from milagro_bls_amd import batch
    from milagro_bls_amd.api import AggregateSignature, AggregatePublicKey
    c, _d, mt = V.built(N, "sparse_9_of_2500")
    n = 40
    sigs, apks, idx, rands = c.sigs[:n], c.apks[:n], c.idx[:n], c.rands[:n]
    D = len(set(idx))
    assert N.plan_verify_multiple_msgtable(n, len(c.listed), D, 0)["route"] == N.VM_ROUTE_GROUPED
    assert N.plan_verify_multiple_msgtable(n, len(c.listed), 0, 0)["route"] == N.VM_ROUTE_PER_SET
    batch.set_vm_grouping(mode)
    try:
        for where in (None, 2):
            s = list(sigs)
            if where is not None:
                s[where] = probe
            spelled = [(AggregateSignature(s[i]), AggregatePublicKey(apks[i]), c.listed[idx[i]]) for i in range(n)]
            named = [(AggregateSignature(s[i]), AggregatePublicKey(apks[i]), idx[i]) for i in range(n)]
            r1, r2, r3 = random.Random(777), random.Random(777), random.Random(777)
            want = AggregateSignature.verify_multiple_aggregate_signatures(r1, spelled)
            got = AggregateSignature.verify_multiple_aggregate_signatures_msgtable(r2, named, mt)
            got_l, sets_l = AggregateSignature.verify_multiple_aggregate_signatures_msgtable_locate(r3, named, mt)
            assert got == got_l == want == (where is None), (mode, where)
            assert r1.getstate() == r2.getstate() == r3.getstate(), (mode, where)
            assert sets_l == ([True] * n if where is None else [True] * where + [False] * (n - where)), (mode, where, sets_l)
            asked = []

            def draw(count):
                asked.append(count)
                return rands[:count]
            assert batch.verify_multiple_msgtable_rng(mt, b"".join(s), b"".join(apks), idx, n, draw) == (where is None)
            assert asked == [n if where is None else where], (mode, where, asked)
        bad = list(idx); bad[7] = len(c.listed)
        with pytest.raises(N.MblsError):
            batch.verify_multiple_msgtable_rng(mt, b"".join(sigs), b"".join(apks), bad, n, lambda count: rands[:count])
        assert AggregateSignature.verify_multiple_aggregate_signatures_msgtable(random.Random(1), [], mt) is True
    finally:
        batch.set_vm_grouping(0)
