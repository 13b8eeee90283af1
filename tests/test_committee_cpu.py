"""The committee table without a GPU (include/mbls.h, "committee table"): the route and the expansion of a bitfield into an index list
(milagro_bls_amd/csrc/mbls_cmt.h, the functions k_cmt_expand runs) and the committee kind of the batch description (mbls_batch.h) on the host
(tests/cmt_emul/mbls_cmt_harness.cpp) against a Python model; mbls_plan_committee_route through ctypes; the harness as a program of its own under the address and
undefined-behaviour sanitizers; and what the entries refuse, or fail loudly at, on a machine without a GPU."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import pytest

import helpers

CXX = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
DIR = os.path.join(helpers.ROOT, "tests", "cmt_emul")
SRC = os.path.join(DIR, "mbls_cmt_harness.cpp")
CSRC = os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc")
EDGE_M = list(range(1, 131)) + [2047, 2048]


# ---- the model: ten lines
def model_route(m, s, eligible, mode):
    """True: complement. mode 0 auto, 1 always direct, 2 complement whenever eligible"""
    if not eligible or mode == 1:
        return False
    return mode == 2 or (m - s) + 1 < s


def model_list(bits, m, eligible, mode):
    """(listed positions, complement) of a committee of m under the bitfield `bits` (bytes, SSZ order)"""
    sel = [j for j in range(m) if (bits[j >> 3] >> (j & 7)) & 1]
    comp = model_route(m, len(sel), eligible, mode)
    return ([j for j in range(m) if j not in set(sel)] if comp else sel), comp


class Flat(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("sigs", "results", "bitmap", "status", "n", "cmt_idx", "bits", "bits_stride", "msg_idx", "crecs", "members", "cmax", "ccount",
                                          "committee", "indexed", "key_idx", "key_off")]


@pytest.fixture(scope="module")
def ch():
    so = os.path.join(DIR, "libmbls_cmt_harness.so")
    deps = [SRC, os.path.join(CSRC, "mbls_cmt.h"), os.path.join(CSRC, "mbls_batch.h"), os.path.join(helpers.ROOT, "include", "mbls.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.ch_route.restype = C.c_int; lib.ch_route.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    lib.ch_count.restype = C.c_uint32; lib.ch_count.argtypes = [C.c_void_p, C.c_uint32]
    lib.ch_expand.restype = C.c_uint32; lib.ch_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    lib.ch_slice.restype = None; lib.ch_slice.argtypes = [C.POINTER(Flat), C.c_uint64, C.c_uint64, C.POINTER(Flat)]
    return lib


def crossover(m):
    """the largest s that stays direct in the automatic mode: (m - s) + 1 < s  <=>  s > (m + 1) / 2"""
    return (m + 1) // 2


def test_route_at_every_m_and_s(ch):
    """every (m, s) with m <= 130, and at m = 2047, 2048 the edges: s = 0, 1, m - 1, m and both sides of the crossover; three modes, eligible and not"""
    for m in EDGE_M:
        ss = range(m + 1) if m <= 130 else sorted({0, 1, m - 1, m, crossover(m), crossover(m) + 1, crossover(m) - 1})
        for s in ss:
            for mode in (0, 1, 2):
                for el in (0, 1):
                    assert bool(ch.ch_route(m, s, el, mode)) == model_route(m, s, el, mode), (m, s, el, mode)
    for m in EDGE_M:                                              # the crossover is where the count of additions says: direct s, complement (m - s) + 1
        s = crossover(m)
        assert not ch.ch_route(m, s, 1, 0) and (s + 1 > m or ch.ch_route(m, s + 1, 1, 0))
        assert (m - s) + 1 >= s and (s + 1 > m or (m - (s + 1)) + 1 < s + 1)


def test_plan_committee_route_through_ctypes_equals_the_model():
    from milagro_bls_amd import _native as N
    L = N.lib()
    for m in EDGE_M:
        ss = range(m + 1) if m <= 130 else (0, 1, crossover(m), crossover(m) + 1, m - 1, m)
        for s in ss:
            for mode in (0, 1, 2):
                for el in (0, 1):
                    assert L.mbls_plan_committee_route(m, s, el, mode) == int(model_route(m, s, el, mode)), (m, s, el, mode)
    assert N.plan_committee_route(128, 127) and not N.plan_committee_route(128, 127, eligible=False) and not N.plan_committee_route(128, 127, mode=N.CMT_ROUTE_DIRECT)
    assert N.plan_committee_route(128, 1, mode=N.CMT_ROUTE_COMPLEMENT)
    for bad in ((0, 0, 1, 0), (2049, 1, 1, 0), (4, 5, 1, 0), (4, 1, 1, 3), (4, 1, 1, -1)):
        assert L.mbls_plan_committee_route(*bad) == N.ERR_ARGUMENT, bad
    assert N.COMMITTEE_MAX_MEMBERS == 2048


def expand(ch, bits, m, eligible, mode, members=None):
    nw = (m + 31) // 32
    raw = bytes(bits[:4 * nw]).ljust(4 * nw, b"\0")
    words = (C.c_uint32 * nw).from_buffer_copy(raw)               # little-endian words: bit j & 31 of word j >> 5 is bit j & 7 of byte j >> 3
    out = (C.c_uint32 * m)(*([0xDEADBEEF] * m)); comp = C.c_int(-1)
    mem = None if members is None else (C.c_uint32 * m)(*members)
    cnt = ch.ch_expand(words, mem, m, eligible, mode, out, C.byref(comp))
    assert list(out)[cnt:] == [0xDEADBEEF] * (m - cnt)            # nothing written past the count
    return list(out)[:cnt], bool(comp.value)


@pytest.mark.parametrize("m", [1, 31, 32, 33, 63, 64, 65, 2048])
def test_listed_positions(ch, m):
    """random bitfields of every density, the all-ones field with stray bits above m, the empty field: the list is the model's, in member order"""
    rnd = random.Random(m)
    nbytes = 4 * ((m + 31) // 32)
    fields = [bytes(nbytes), b"\xff" * nbytes]
    for density in (0.02, 0.25, 0.45, 0.5, 0.55, 0.9, 0.99):
        fields.append(bytes(sum((rnd.random() < density) << b for b in range(8)) for _ in range(nbytes)))
    one_missing = bytearray(b"\xff" * nbytes); one_missing[(m - 1) >> 3] &= ~(1 << ((m - 1) & 7)) & 0xFF
    fields.append(bytes(one_missing))
    for bits in fields:
        words = (C.c_uint32 * (nbytes // 4)).from_buffer_copy(bits)
        assert ch.ch_count(words, m) == sum((bits[j >> 3] >> (j & 7)) & 1 for j in range(m))
        for mode in (0, 1, 2):
            for el in (0, 1):
                assert expand(ch, bits, m, el, mode) == model_list(bits, m, el, mode), (m, mode, el)
    members = [rnd.randrange(2 ** 32) for _ in range(m)]
    got, comp = expand(ch, fields[-1], m, 1, 0, members)
    want, wcomp = model_list(fields[-1], m, 1, 0)
    assert comp == wcomp and got == [members[j] for j in want]


def test_slice_of_a_committee_batch(ch):
    """lo = 0, 64 and n - 1: the ids advance by 4 bytes per item, the bits by the stride, the table's pointers stay; the other per-item pointers as everywhere"""
    n, stride = 300, 20
    f = Flat(sigs=1 << 20, results=2 << 20, bitmap=3 << 20, status=4 << 20, n=n, cmt_idx=5 << 20, bits=6 << 20, bits_stride=stride, msg_idx=7 << 20, crecs=8 << 20,
             members=9 << 20, cmax=129, ccount=18)
    for lo, hi in ((0, n), (64, n), (n - 1, n), (64, 128), (0, 64)):
        o = Flat()
        ch.ch_slice(C.byref(f), lo, hi, C.byref(o))
        assert o.n == hi - lo and o.committee == 1 and o.indexed == 1
        assert (o.cmt_idx, o.bits, o.msg_idx) == (f.cmt_idx + 4 * lo, f.bits + stride * lo, f.msg_idx + 4 * lo)
        assert (o.sigs, o.results, o.status, o.bitmap) == (f.sigs + 96 * lo, f.results + lo, f.status + 4 * lo, f.bitmap + 8 * (lo // 64))
        assert (o.crecs, o.members, o.cmax, o.ccount, o.bits_stride) == (f.crecs, f.members, 129, 18, stride)
        assert (o.key_idx, o.key_off) == (0, 0)
    f.cmt_idx = 0; f.bits = 0                                      # null stays null
    o = Flat(); ch.ch_slice(C.byref(f), 64, n, C.byref(o))
    assert (o.cmt_idx, o.bits) == (0, 0)


def test_harness_as_its_own_program_under_asan_and_ubsan():
    """the same functions over heap buffers of exactly the promised sizes: a read past the bitfield or a write past the list aborts the program"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "cmt_harness")
        subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMBLS_CMT_HARNESS_MAIN", "-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-300:], r.stderr[-2000:])


def test_entries_refuse_null_handles_and_fail_loudly_without_a_gpu():
    from milagro_bls_amd import _native as N
    L = N.lib()
    out = C.c_void_p()
    assert L.mbls_committees_create(None, None, 0, C.byref(out)) == N.ERR_ARGUMENT and not out.value
    assert L.mbls_committees_count(None) == 0 and L.mbls_committees_clear(None) == N.ERR_ARGUMENT
    L.mbls_committees_destroy(None)
    first = C.c_uint64(7)
    assert L.mbls_committees_append(None, None, None, 1, C.byref(first)) == N.ERR_ARGUMENT and first.value == 7
    assert L.mbls_committees_get(None, 0, None, None, None) == N.ERR_ARGUMENT
    assert L.mbls_ctx_set_committee_route(None, 0) == N.ERR_ARGUMENT and L.mbls_ctx_reserve_committee_items(None, 1, 1) == N.ERR_ARGUMENT
    res = (C.c_uint8 * 4)(9, 9, 9, 9)
    assert L.mbls_fast_aggregate_verify_batch_committee(None, None, None, None, 32, None, None, None, 4, 1, res, None) == N.ERR_ARGUMENT
    assert L.mbls_fast_aggregate_verify_batch_committee_device(None, None, None, None, 32, None, None, None, 4, 1, res, None, None, None) == N.ERR_ARGUMENT
    assert L.mbls_fast_aggregate_verify_batch_committee_msgtable(None, None, None, None, None, None, None, 4, 1, res, None) == N.ERR_ARGUMENT
    assert L.mbls_fast_aggregate_verify_batch_committee_msgtable_device(None, None, None, None, None, None, None, 4, 1, res, None, None, None) == N.ERR_ARGUMENT
    assert list(res) == [9, 9, 9, 9]
    assert L.mbls_committees_max_members(None) == 0
    with pytest.raises(ValueError):                               # an offset table has one entry more than there are committees: never none
        N.CommitteeTable.append(object.__new__(N.CommitteeTable), [], [])
    import torch
    if not torch.cuda.is_available():                             # no CPU fallback: without a context there is no table, and the mirror says so
        with pytest.raises(N.MblsError):
            N.Context(0)
        with pytest.raises(N.MblsError):
            N.CommitteeTable(N.KeyTable())
