"""GPU tests of mbls_verify_multiple*_msgtable_locate* (include/mbls.h, "verify_multiple OVER THE RESIDENT MESSAGE TABLE, LOCATED PER SET"): the call's bool
and word byte for byte the non-locate entry's under the same grouping mode; every set of an accepted call 1; every set of a rejected call what the one-set
call with its scalar returns, judged against mbls_verify_multiple_batches_locate[_indexed]_device with one batch on the spelled-out messages; a message fault
in the word of exactly the sets that name it. The shapes are those of tests/test_gpu_vm_msgtable.py (tests/vm_msgtable_cases.py)."""
import ctypes as C
import random

import numpy as np
import pytest

import test_gpu_vm_shared_locate as SL
import vm_msgtable_cases as V

pytestmark = pytest.mark.gpu
MODES = (1, 2, 0)


@pytest.fixture(scope="module")
def N():
    from milagro_bls_amd import _native
    _native.default_context()
    return _native


@pytest.fixture(scope="module")
def probe(vectors):
    return bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])


def all_defects(c, probe, seed):
    """every defect of DEFECTS on one set each -> (case, {set: kind})"""
    rnd = random.Random(seed)
    where = dict(zip(rnd.sample(range(c.n), len(V.DEFECTS)), V.DEFECTS))
    b = c
    for i, kind in where.items():
        b = V.with_defect(b, kind, i, probe)
    return b, where


@pytest.mark.parametrize("name", V.SHAPES)
def test_accepted_calls_read_one_for_every_set(N, name):
    c, d, mt = V.built(N, name)
    res, sres, sst = V.check_located(N, c, d, mt)
    assert res == 1 and sres == [1] * c.n


@pytest.mark.parametrize("name", V.SHAPES)
def test_every_defect_is_located(N, probe, name):
    """all eight defects in one call, each on a set of its own: the per-set answers and words of the one-batch baseline, in every mode and both key forms; the
    sets read what their defect makes them read"""
    c, _d, mt = V.built(N, name)
    b, where = all_defects(c, probe, V.hash_name(name))
    res, sres, sst = V.check_located(N, b, SL.DevCase(N, b, table=True), mt)
    assert res == 0
    for i in range(b.n):
        kind = where.get(i)
        # (a swapped signature or a wrong key may by chance land on a set with the same message and key: not with these seeds)
        if kind is None or kind == "both_inf":
            assert sres[i] == 1 and not sst[i] & (V.ST_PAIRING_FAILED | V.REJECT_BATCH), (i, kind, hex(sst[i]))
        elif kind in ("wrong_key", "swapped_sig", "inf_sig", "inf_key"):
            assert sres[i] == 0 and sst[i] & V.ST_PAIRING_FAILED and not sst[i] & V.REJECT_BATCH, (i, kind, hex(sst[i]))
        else:
            assert sres[i] == 0 and not sst[i] & V.ST_PAIRING_FAILED and sst[i] & V.REJECT_BATCH, (i, kind, hex(sst[i]))


@pytest.mark.parametrize("kind", V.DEFECTS)
def test_each_defect_alone(N, probe, kind):
    c, _d, mt = V.built(N, "every_entry_of_12")
    i = random.Random(V.hash_name(kind)).randrange(c.n)
    b = V.with_defect(c, kind, i, probe)
    res, sres, sst = V.check_located(N, b, SL.DevCase(N, b, table=True), mt)
    assert res == (1 if kind == "both_inf" else 0)
    assert sres == [1 if (j != i or kind == "both_inf") else 0 for j in range(b.n)]


def test_index_faults_land_on_the_sets_that_name_them(N):
    """a set naming T, and one naming 2^32 - 1: the call is rejected, the bit is in those sets' words alone, every other set is examined and reads 1; an empty
    table: every set 0 with the bit; a flagged entry: the sets that name it, and nobody else"""
    c, d, _mt = V.built(N, "every_entry_of_12")
    T = len(c.listed)
    mt = V.make_table(N, c.listed)
    empty = N.MsgTable(capacity_hint=4)
    try:
        raw = SL._dev(bytes(64)); off = SL._dev(np.array([40, 8], dtype=np.uint64))
        assert mt.append_device(raw.data_ptr(), 1, msg_len=0, d_msg_offsets=off.data_ptr()) == T        # entry T: flagged
        for bads in ({17: T + 1}, {3: V.NO_ENTRY, 149: T + 1}, {33: T, 90: T}):
            idx = list(c.idx)
            for i, v in bads.items():
                idx[i] = v
            for mode in MODES:
                for ix in (False, True):
                    r0, s0 = V.call_table(N, d, mt, mode, False, ix, idx=V.dev_idx(idx))
                    res, st, sres, sst = V.call_table(N, d, mt, mode, True, ix, idx=V.dev_idx(idx))
                    assert (res, st) == (r0, s0) and res == 0 and st & V.ST_BAD_MSG_RANGE, (bads, mode, ix, res, hex(st))
                    assert sres == [0 if i in bads else 1 for i in range(c.n)], (bads, mode, ix)
                    assert sst == [V.ST_BAD_MSG_RANGE if i in bads else 0 for i in range(c.n)], (bads, mode, ix, [hex(w) for w in sst if w])
        # the flagged entry present but unnamed changes nothing
        res, sres, _sst = V.check_located(N, c, d, mt)
        assert res == 1 and sres == [1] * c.n
        for mode in MODES:
            for ix in (False, True):
                res, st, sres, sst = V.call_table(N, d, empty, mode, True, ix)
                assert res == 0 and st & V.ST_BAD_MSG_RANGE and sres == [0] * c.n and all(w & V.ST_BAD_MSG_RANGE for w in sst), (mode, ix)
    finally:
        mt.close(); empty.close()


def test_table_life(N, probe):
    """a table grown from capacity_hint = 1; two locate calls back to back; clear, other messages, the call again"""
    c, _d, _mt = V.built(N, "every_entry_of_12")
    b = V.with_defect(c, "wrong_key", 21, probe)
    d = SL.DevCase(N, b, table=True)
    mt = V.make_table(N, c.listed, capacity_hint=1, pieces=4)
    from milagro_bls_amd import batch
    try:
        ref = V.check_located(N, b, d, mt)
        assert ref[0] == 0 and ref[1] == [0 if i == 21 else 1 for i in range(b.n)]
        for mode in (1, 2):
            batch.set_vm_grouping(mode)
            o1 = V.enqueue_table(N, d, mt, True)
            o2 = V.enqueue_table(N, d, mt, True, indexed=True)
            for o in (o1, o2):
                res, _st, sres, sst = V.read(d.n, o, True)
                assert (res, sres, sst) == ref, mode
        batch.set_vm_grouping(0)
        mt.clear()
        listed2, idx2 = V.shape("one_entry_for_all")
        c2 = V.with_defect(V.base_case(listed2, idx2, 77), "swapped_sig", 8, probe)
        assert mt.append(b"".join(listed2), len(listed2), msg_len=0, msg_offsets=SL._offsets(listed2)) == 0
        ref2 = V.check_located(N, c2, SL.DevCase(N, c2, table=True), mt)
        assert ref2[0] == 0 and ref2[1] == [0 if i == 8 else 1 for i in range(c2.n)]
    finally:
        batch.set_vm_grouping(0)
        mt.close()


def test_append_on_another_stream_right_before_the_call(N, probe):
    import torch
    from milagro_bls_amd import batch
    c, _d, _mt = V.built(N, "every_entry_of_12")
    b = V.with_defect(c, "inf_sig", 140, probe)
    d = SL.DevCase(N, b)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    d_list = SL._dev(b"".join(c.listed)); d_off = SL._dev(np.array(SL._offsets(c.listed), dtype=np.uint64))
    torch.cuda.synchronize()
    for mode in (1, 2):
        mt = N.MsgTable(capacity_hint=64)
        try:
            batch.set_vm_grouping(mode)
            assert mt.append_device(d_list.data_ptr(), len(c.listed), msg_len=0, d_msg_offsets=d_off.data_ptr(), stream=sa.cuda_stream) == 0
            res, _st, sres, sst = V.read(d.n, V.enqueue_table(N, d, mt, True, stream=sb.cuda_stream), True)
            assert res == 0 and sres == [0 if i == 140 else 1 for i in range(b.n)] and sst[140] == V.ST_PAIRING_FAILED, mode
        finally:
            batch.set_vm_grouping(0)
            mt.close()


FORMS = [("20_of_20", 0, None), ("20_of_40", 0, 64), ("70_of_70", 0, 64), ("5_of_600", None, None), ("5_of_600", 0, 64)]


@pytest.mark.parametrize("name,coop_max,round_items", FORMS, ids=["lane_pairs", "lanes", "cut_at_a_round", "waves_5_of_150_live", "lanes_5_of_150_live"])
def test_miller_forms(N, probe, name, coop_max, round_items):
    """the Miller forms of tests/test_gpu_vm_msgtable.py::test_miller_forms with three bad sets: the baseline's answers under the same tuning"""
    listed, idx = V.shape(name)
    c = V.base_case(listed, idx, V.hash_name(name))
    b = V.with_defect(V.with_defect(V.with_defect(c, "wrong_key", 0, probe), "inf_sig", 64, probe), "not_in_g2", c.n - 1, probe)
    mt = V.make_table(N, listed)
    ctx = N.default_context()
    try:
        if round_items is not None:
            assert N.lib().mbls_ctx_set_round_items(ctx.handle, round_items) == 0
        if coop_max is not None:
            assert N.lib().mbls_ctx_set_coop_max_items(ctx.handle, coop_max) == 0
        res, sres, sst = V.check_located(N, b, SL.DevCase(N, b, table=True), mt, modes=(1, 2))
        assert res == 0 and [i for i in range(b.n) if not sres[i]] == [0, 64, b.n - 1]
    finally:
        ctx.reset_tuning()
        mt.close()


@pytest.mark.parametrize("mode", MODES)
def test_rng_entry(N, probe, mode):
    """mbls_verify_multiple_msgtable_locate_rng: the draws of the non-locate entry; a set at or behind the first signature outside G2 reads 0 with the word the
    signature phase found, the sets in front of it are examined; required and refused arguments"""
    from milagro_bls_amd import batch
    c, _d, mt = V.built(N, "sparse_9_of_2500")
    n = 40
    b = V.with_defect(c, "wrong_key", 1, probe)
    sigs, apks, idx, rands = b.sigs[:n], b.apks[:n], b.idx[:n], b.rands[:n]
    batch.set_vm_grouping(mode)
    try:
        for where in (None, 2):
            s = list(sigs)
            if where is not None:
                s[where] = probe
            asked = []

            def draw(count):
                asked.append(count)
                return rands[:count]
            res, sres, sst = batch.verify_multiple_msgtable_locate_rng(mt, b"".join(s), b"".join(apks), idx, n, draw)
            assert asked == [n if where is None else where] and res is False
            reached = n if where is None else where
            assert sres == [i != 1 and i < reached for i in range(n)], (mode, where, sres)
            assert sst[1] == V.ST_PAIRING_FAILED and (where is None or sst[where] & 0x02)
        ctx = N.default_context()
        f = N.lib().mbls_verify_multiple_msgtable_locate_rng
        cb = N.SCALAR_SOURCE(lambda _u, out, count: None)
        res1 = N.outbuf(1); res1[0] = 9
        S, A = N.cbuf(b"".join(sigs)), N.cbuf(b"".join(apks))
        ix = (C.c_uint32 * n)(*idx)
        assert f(ctx.handle, S, A, mt.handle, ix, n, res1, None, None, cb, None) == N.ERR_ARGUMENT          # set_results is required
        bad = (C.c_uint32 * n)(*([len(c.listed)] + idx[1:]))
        sres1 = N.outbuf(n)
        assert f(ctx.handle, S, A, mt.handle, bad, n, res1, sres1, None, cb, None) == N.ERR_ARGUMENT       # an index that names no entry
        assert res1[0] == 9
    finally:
        batch.set_vm_grouping(0)
