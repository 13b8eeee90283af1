"""The resident message table without a GPU (include/mbls.h, "resident message table"): the table's index arithmetic (milagro_bls_amd/csrc/mbls_mtb.h) with the lane
bodies lane_h_export / lane_h_gather on the host (tests/msgtab_emul/mbls_msgtab_harness.cpp), and the cut of a message-table stream's calls, whose "message bytes"
are 4 bytes of index per item."""
import ctypes as C
import os
import subprocess

import pytest

import helpers

BAD = 0x100          # MBLS_ST_BAD_MSG_RANGE
EMPTY_SEED = 0xE0E0


@pytest.fixture(scope="module")
def mt():
    d = os.path.join(helpers.ROOT, "tests", "msgtab_emul")
    so = os.path.join(d, "libmbls_msgtab_harness.so")
    csrc = os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc")
    src = [os.path.join(d, "mbls_msgtab_harness.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src[0]])
    lib = C.CDLL(so)
    lib.mt_new.restype = C.c_void_p; lib.mt_new.argtypes = [C.c_uint64, C.c_uint32]
    lib.mt_free.argtypes = [C.c_void_p]
    for f in (lib.mt_size, lib.mt_capacity, lib.mt_growths):
        f.restype = C.c_uint64; f.argtypes = [C.c_void_p]
    lib.mt_append.restype = C.c_uint64; lib.mt_append.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.mt_read_entry.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.mt_gather.restype = C.c_uint32; lib.mt_gather.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.mt_pattern.restype = C.c_uint32; lib.mt_pattern.argtypes = [C.c_uint32, C.c_int]
    lib.mt_entry_of.restype = C.c_uint64; lib.mt_entry_of.argtypes = [C.c_uint32, C.c_uint64]
    return lib


def want72(lib, seed):
    return [lib.mt_pattern(seed, w) for w in range(72)]


def read(lib, t, e):
    out = (C.c_uint32 * 72)(); flag = C.c_uint32(0xDEAD)
    lib.mt_read_entry(t, e, out, C.byref(flag))
    return list(out), flag.value


def gather(lib, t, idx, item=0, items=1):
    out = (C.c_uint32 * 72)()
    st = lib.mt_gather(t, idx, item, items, out)
    return list(out), st


def test_appends_of_1_3_and_70_into_a_table_of_capacity_2(mt):
    """two growths (2 -> 4 -> 74) and a first index that is no multiple of 64; after each append every earlier entry's 72 dwords and flag are what they were, the
    private entry included; the gather returns the entry an index names, from any workspace item"""
    t = mt.mt_new(2, EMPTY_SEED)
    try:
        seeds, flags, firsts, caps = [], [], [], []
        for step, n in enumerate((1, 3, 70)):
            new = [1000 * (step + 1) + i for i in range(n)]
            # message 1 of the second append and message 69 of the third had a bad range; other status bits of the list's own hash never become flags
            st = [(BAD | 0x40) if (step, i) in ((1, 1), (2, 69)) else (0x40 if i % 5 == 0 else 0) for i in range(n)]
            first = mt.mt_append(t, n, (C.c_uint32 * n)(*new), (C.c_uint32 * n)(*st))
            firsts.append(first); caps.append(mt.mt_capacity(t))
            assert first == len(seeds)
            seeds += new; flags += [s & BAD for s in st]
            assert mt.mt_size(t) == len(seeds)
            assert read(mt, t, 0) == (want72(mt, EMPTY_SEED), 0)
            for j, (sd, fl) in enumerate(zip(seeds, flags)):
                assert read(mt, t, j + 1) == (want72(mt, sd), fl), (step, j)
        assert firsts == [0, 1, 4] and firsts[2] % 64 != 0
        assert caps == [2, 4, 74] and mt.mt_growths(t) == 2
        size = mt.mt_size(t)
        assert size == 74
        for j in (0, 1, 2, 4, 63, 64, size - 1):
            for item, items in ((0, 1), (66, 130)):
                assert gather(mt, t, j, item, items) == (want72(mt, seeds[j]), flags[j]), j
        assert flags[2] == BAD and flags[size - 1] == BAD
    finally:
        mt.mt_free(t)


def test_indices_at_and_above_the_size_get_the_empty_message_and_the_bad_range_bit(mt):
    t = mt.mt_new(2, EMPTY_SEED)
    try:
        empty = (want72(mt, EMPTY_SEED), BAD)
        for idx in (0, 1, 0xFFFFFFFF):               # an empty table: every index names nothing
            assert gather(mt, t, idx) == empty
            assert mt.mt_entry_of(idx, 0) == 0
        seeds = list(range(500, 574))
        for a, b in ((0, 1), (1, 4), (4, 74)):
            mt.mt_append(t, b - a, (C.c_uint32 * (b - a))(*seeds[a:b]), (C.c_uint32 * (b - a))())
        size = mt.mt_size(t)
        assert gather(mt, t, size - 1) == (want72(mt, seeds[-1]), 0)
        assert gather(mt, t, size) == empty
        assert gather(mt, t, 0xFFFFFFFF) == empty
        assert [mt.mt_entry_of(i, size) for i in (0, size - 1, size, 0xFFFFFFFF)] == [1, size, 0, 0]
    finally:
        mt.mt_free(t)


def test_stream_cut_of_message_index_calls():
    """a message-table stream stages 4 bytes per item: calls of 40, 40 and 10 items with msg_len = 4 into rounds of 64 items -- the second call is split 24 + 16.
    The same cut when the message bytes are what fills the round (round_msg_bytes = 4 x 64 in rounds of 128 items)."""
    from milagro_bls_amd import _native as N
    calls = [dict(n=40, k=2, msg_len=4), dict(n=40, k=2, msg_len=4), dict(n=10, k=2, msg_len=4, flush_after=1)]
    want = [dict(call=0, first=0, items=40, round=0, round_first=0),
            dict(call=1, first=0, items=24, round=0, round_first=40),
            dict(call=1, first=24, items=16, round=1, round_first=0),
            dict(call=2, first=0, items=10, round=1, round_first=16)]
    assert N.stream_cut(calls, 64, 128 * 64, 4 * 64) == want
    assert N.stream_cut(calls, 128, 128 * 128, 4 * 64) == want


def test_header_names_the_new_entries_and_the_routing():
    txt = open(os.path.join(helpers.ROOT, "include", "mbls.h")).read()
    for sym in ("mbls_msgtable_create", "mbls_msgtable_append_device", "mbls_msgtable_get", "mbls_msgtable_clear", "mbls_verify_batch_msgtable_device",
                "mbls_fast_aggregate_verify_batch_indexed_msgtable", "mbls_stream_create_msgtable", "mbls_stream_submit_msgidx_device", "mbls_stream_submit_msgidx"):
        assert sym + "(" in txt, sym
    assert "Not covered: the verification stream" not in txt
    assert "mbls_plan_batch_shared_msgs(limits, n, 0).batch" in txt
