"""Committee spans without a GPU (include/mbls.h, "committee spans"): the expansion of a committee list and one concatenated bitfield into the direct list, the
missing list and the item's record (milagro_bls_amd/csrc/mbls_cms.h, the functions k_cms_expand runs) and the span kind of the batch description (mbls_batch.h) on
the host (tests/cms_emul/mbls_cms_harness.cpp) against a Python model; mbls_plan_committee_span through ctypes; the harness as a program of its own under the
address and undefined-behaviour sanitizers; what the entries refuse; and that a machine without a GPU gives no context to call them with."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import pytest

import helpers

CXX = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
DIR = os.path.join(helpers.ROOT, "tests", "cms_emul")
SRC = os.path.join(DIR, "mbls_cms_harness.cpp")
CSRC = os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc")
EDGE = [1, 31, 32, 33, 63, 64, 65, 2048]
POISON = 0xDEADBEEF


# ---- the model: ten lines
def model_span(bits, sizes, eligible, mode):
    """(direct list, missing list, complement mask, nobody) of the segments `sizes` under the field `bits` (bytes, SSZ order): bit positions, in order"""
    direct, missing, mask, o, total = [], [], 0, 0, 0
    for t, m in enumerate(sizes):
        sel = [j for j in range(m) if (bits[(o + j) >> 3] >> ((o + j) & 7)) & 1]
        comp = bool(eligible[t]) and mode != 1 and (mode == 2 or (m - len(sel)) + 1 < len(sel))
        if comp:
            mask |= 1 << t
            missing += [o + j for j in sorted(set(range(m)) - set(sel))]
        else:
            direct += [o + j for j in sel]
        o += m; total += len(sel)
    return direct, missing, mask, total == 0


class Flat(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("sigs", "results", "bitmap", "status", "n", "cmt_idx", "bits", "bits_stride", "msg_idx", "crecs", "members", "cmax", "ccount",
                                          "committee", "indexed", "key_idx", "key_off", "span", "cmt_ids", "n_cmt_ids", "span_off")]


@pytest.fixture(scope="module")
def sh():
    so = os.path.join(DIR, "libmbls_cms_harness.so")
    deps = [SRC, os.path.join(CSRC, "mbls_cms.h"), os.path.join(CSRC, "mbls_cmt.h"), os.path.join(CSRC, "mbls_batch.h"), os.path.join(helpers.ROOT, "include", "mbls.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.sh_seg_offset.restype = C.c_uint32; lib.sh_seg_offset.argtypes = [C.c_void_p, C.c_uint32]
    lib.sh_count.restype = C.c_uint32; lib.sh_count.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.sh_selected.restype = C.c_int; lib.sh_selected.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.sh_stride.restype = C.c_uint64; lib.sh_stride.argtypes = [C.c_uint32, C.c_uint32]
    lib.sh_range_ok.restype = C.c_int; lib.sh_range_ok.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.sh_expand.restype = None
    lib.sh_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.sh_slice.restype = None; lib.sh_slice.argtypes = [C.POINTER(Flat), C.c_uint64, C.c_uint64, C.POINTER(Flat)]
    return lib


def expand(sh, bits, sizes, eligible, mode, extra=0, members=None):
    """the region (M + extra words, poisoned) and the record -> (direct list, missing list in its (segment, member) order, mask, nobody)"""
    q, M = len(sizes), sum(sizes)
    nw = (M + 31) // 32
    words = (C.c_uint32 * max(1, nw)).from_buffer_copy(bytes(bits[:4 * nw]).ljust(4 * max(1, nw), b"\0"))
    stride = max(1, M) + extra
    region = (C.c_uint32 * stride)(*([POISON] * stride))
    rec = (C.c_uint32 * 5)(*([POISON] * 5))
    firsts = [sum(sizes[:t]) for t in range(q)]
    sh.sh_expand(words, None if members is None else (C.c_uint32 * max(1, M))(*members), (C.c_uint32 * max(1, q))(*sizes), (C.c_uint32 * max(1, q))(*firsts),
                 (C.c_uint8 * max(1, q))(*eligible), q, mode, region, stride, rec)
    nd, nm = rec[0], rec[1]
    out = list(region)
    assert nd + nm <= M and out[nd:stride - nm] == [POISON] * (stride - nm - nd)       # nothing written past the counts, from either end
    assert rec[4] in (0, 1)
    return out[:nd], out[stride - nm:][::-1], rec[2] | (rec[3] << 32), bool(rec[4])


def fields_for(M, rnd):
    """densities from 0 to 1; every field carries stray bits at and above M (the last word's upper part, where there is one)"""
    nbytes = 4 * ((M + 31) // 32)
    out = [bytes(nbytes), b"\xff" * nbytes]
    for density in (0.02, 0.25, 0.45, 0.5, 0.55, 0.9, 0.99):
        f = bytearray(sum((rnd.random() < density) << b for b in range(8)) for _ in range(nbytes))
        for p in range(M, 8 * nbytes):
            f[p >> 3] |= 1 << (p & 7)
        out.append(bytes(f))
    if M:
        one = bytearray(b"\xff" * nbytes); one[(M - 1) >> 3] &= ~(1 << ((M - 1) & 7)) & 0xFF
        out.append(bytes(one))
    return out


def span_cases():
    rnd = random.Random(7549)
    cases = [[m] for m in EDGE]
    cases += [[a, b] for a in (1, 31, 33, 63, 65) for b in (1, 32, 64, 65)]                       # boundaries at bits 1, 31, 33, 63, 65
    cases += [[1, 30, 2], [31, 2, 30], [63, 2, 64], [65, 64, 1], [33, 32, 2048], [2048, 1, 31]]    # ... and beyond a word, with three segments
    cases += [[rnd.choice(EDGE[:7]) for _ in range(64)], [1] * 64, [65] * 64]
    return cases


@pytest.mark.parametrize("sizes", span_cases(), ids=lambda s: "x".join(map(str, s[:4])) + ("_q%d" % len(s)))
def test_lists_counts_and_mask_equal_the_model(sh, sizes):
    rnd = random.Random(sum(sizes) * 131 + len(sizes))
    q, M = len(sizes), sum(sizes)
    arr = (C.c_uint32 * q)(*sizes)
    assert [sh.sh_seg_offset(arr, t) for t in range(q)] == [sum(sizes[:t]) for t in range(q)]
    eligibles = [[1] * q, [0] * q, [rnd.randrange(4) != 0 for _ in range(q)], [t & 1 for t in range(q)]]
    for bits in fields_for(M, rnd):
        words = (C.c_uint32 * (len(bits) // 4)).from_buffer_copy(bits)
        o = 0
        for m in sizes[:8]:
            assert sh.sh_count(words, o, m) == sum((bits[(o + j) >> 3] >> ((o + j) & 7)) & 1 for j in range(m))
            assert sh.sh_selected(words, o, m - 1) == (bits[(o + m - 1) >> 3] >> ((o + m - 1) & 7)) & 1
            o += m
        for mode in (0, 1, 2):
            for el in eligibles:
                assert expand(sh, bits, sizes, el, mode) == model_span(bits, sizes, el, mode), (sizes, mode, el)
    # key indices instead of positions, and a region wider than M: the missing list hangs from the region's END
    members = [rnd.randrange(2 ** 32) for _ in range(M)]
    bits = fields_for(M, rnd)[-1]
    d, ms, mask, nobody = expand(sh, bits, sizes, [1] * q, 0, extra=37, members=members)
    wd, wm, wmask, wnobody = model_span(bits, sizes, [1] * q, 0)
    assert (d, ms, mask, nobody) == ([members[p] for p in wd], [members[p] for p in wm], wmask, wnobody)


def test_empty_span_and_stride(sh):
    assert expand(sh, b"", [], [], 0) == ([], [], 0, True)
    assert sh.sh_stride(0, 128) == 1 and sh.sh_stride(4, 0) == 1 and sh.sh_stride(4, 128) == 32 and sh.sh_stride(4096, 128) == 8192 and sh.sh_stride(1024, 2048) == 8192
    q = C.c_uint32(99)
    assert sh.sh_range_ok(5, 69, 69, C.byref(q)) == 1 and q.value == 64
    assert sh.sh_range_ok(5, 5, 5, C.byref(q)) == 1 and q.value == 0
    for lo, hi, n in ((5, 70, 100), (6, 5, 100), (5, 9, 8)):          # 65 ids, backwards, past the id array
        assert sh.sh_range_ok(lo, hi, n, C.byref(q)) == 0


def test_plan_committee_span_through_ctypes_equals_the_model():
    from milagro_bls_amd import _native as N
    L = N.lib()
    for sizes in span_cases():
        rnd = random.Random(len(sizes) + 17 * sum(sizes))
        q, M = len(sizes), sum(sizes)
        for bits in fields_for(M, rnd)[::3]:
            for mode in (0, 1, 2):
                for el in ([1] * q, [rnd.randrange(3) != 0 for _ in range(q)]):
                    d, ms, mask, _ = model_span(bits, sizes, el, mode)
                    assert N.plan_committee_span(sizes, el, bits, mode) == (mask, len(d), len(ms)), (sizes, mode, el)
    assert N.plan_committee_span([], [], b"") == (0, 0, 0)
    assert N.plan_committee_span([128, 128], [1, 1], b"\xff" * 32) == (3, 0, 0)
    assert N.plan_committee_span([128, 128], [1, 0], b"\xff" * 32) == (1, 128, 0)
    assert N.SPAN_MAX_COMMITTEES == 64
    mask, nd, nm = C.c_uint64(5), C.c_uint32(5), C.c_uint32(5)
    outs = (C.byref(mask), C.byref(nd), C.byref(nm))
    one = lambda sizes, el, bits, nbytes, mode: L.mbls_plan_committee_span((C.c_uint32 * len(sizes))(*sizes), (C.c_uint8 * len(el))(*el), len(sizes), bits, nbytes, mode, *outs)
    f = (C.c_uint8 * 8192)()
    assert one([1] * 64, [1] * 64, f, 8, 0) == N.OK
    assert one([1] * 65, [1] * 65, f, 16, 0) == N.ERR_ARGUMENT                  # q > 64
    assert one([4, 0], [1, 1], f, 8, 0) == N.ERR_ARGUMENT                       # a size of 0
    assert one([4, 2049], [1, 1], f, 8192, 0) == N.ERR_ARGUMENT                 # a size above 2048
    assert one([2048], [1], f, 256, 0) == N.OK
    assert one([33, 32], [1, 1], f, 8, 0) == N.ERR_ARGUMENT                     # M = 65 > 8 * 8
    assert one([32, 32], [1, 1], f, 8, 0) == N.OK                               # M exactly 8 * bits_bytes
    assert one([4], [1], f, 8, 3) == N.ERR_ARGUMENT and one([4], [1], f, 8, -1) == N.ERR_ARGUMENT
    assert L.mbls_plan_committee_span((C.c_uint32 * 1)(4), (C.c_uint8 * 1)(1), 1, f, 8, 0, None, C.byref(nd), C.byref(nm)) == N.ERR_ARGUMENT


def test_slice_of_a_span_batch(sh):
    """lo = 0, 64 and n - 1: the offsets advance by 4 bytes per item, the bits by the stride; the id base, n_cmt_ids and the table's pointers stay"""
    n, stride = 300, 20
    f = Flat(sigs=1 << 20, results=2 << 20, bitmap=3 << 20, status=4 << 20, n=n, cmt_ids=5 << 20, n_cmt_ids=900, span_off=10 << 20, bits=6 << 20, bits_stride=stride,
             msg_idx=7 << 20, crecs=8 << 20, members=9 << 20, cmax=129, ccount=18)
    for lo, hi in ((0, n), (64, n), (n - 1, n), (64, 128), (0, 64)):
        o = Flat()
        sh.sh_slice(C.byref(f), lo, hi, C.byref(o))
        assert o.n == hi - lo and o.committee == 1 and o.indexed == 1 and o.span == 1
        assert (o.span_off, o.bits, o.msg_idx) == (f.span_off + 4 * lo, f.bits + stride * lo, f.msg_idx + 4 * lo)
        assert (o.sigs, o.results, o.status, o.bitmap) == (f.sigs + 96 * lo, f.results + lo, f.status + 4 * lo, f.bitmap + 8 * (lo // 64))
        assert (o.cmt_ids, o.n_cmt_ids, o.crecs, o.members, o.cmax, o.ccount, o.bits_stride) == (f.cmt_ids, 900, f.crecs, f.members, 129, 18, stride)
        assert (o.cmt_idx, o.key_idx, o.key_off) == (0, 0, 0)
    f.span_off = 0; f.bits = 0; f.cmt_ids = 0                          # null stays null
    o = Flat(); sh.sh_slice(C.byref(f), 64, n, C.byref(o))
    assert (o.span_off, o.bits, o.cmt_ids) == (0, 0, 0)


def test_harness_as_its_own_program_under_asan_and_ubsan():
    """the same functions over heap buffers of exactly the promised sizes: a read past the field or the member array, or a write past the region, aborts the program"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "cms_harness")
        subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMBLS_CMS_HARNESS_MAIN", "-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-300:], r.stderr[-2000:])


def test_entries_refuse_null_handles_and_no_context_exists_without_a_gpu():
    from milagro_bls_amd import _native as N
    from milagro_bls_amd import batch as B
    L = N.lib()
    assert L.mbls_ctx_reserve_committee_span_items(None, 1, 1) == N.ERR_ARGUMENT
    res = (C.c_uint8 * 4)(9, 9, 9, 9)
    st = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert L.mbls_fast_aggregate_verify_batch_committee_span(None, None, None, None, 32, None, None, 0, None, None, 4, 1, res, st) == N.ERR_ARGUMENT
    assert L.mbls_fast_aggregate_verify_batch_committee_span_device(None, None, None, None, 32, None, None, 0, None, None, 4, 1, res, None, st, None) == N.ERR_ARGUMENT
    assert L.mbls_fast_aggregate_verify_batch_committee_span_msgtable(None, None, None, None, None, None, 0, None, None, 4, 1, res, st) == N.ERR_ARGUMENT
    assert L.mbls_fast_aggregate_verify_batch_committee_span_msgtable_device(None, None, None, None, None, None, 0, None, None, 4, 1, res, None, st, None) == N.ERR_ARGUMENT
    assert list(res) == [9, 9, 9, 9] and list(st) == [7, 7, 7, 7]
    with pytest.raises(ValueError):                               # one field per id list; a field longer than the stride
        B._span([[0]], [], 4)
    with pytest.raises(ValueError):
        B._span([[0]], [b"\0" * 5], 4)
    ids, n_ids, off, bits = B._span([[3, 4], [], [5]], [b"\x01", b"", b"\xff\xff"], 4)
    assert (list(ids), n_ids, list(off), bytes(bits)) == ([3, 4, 5], 3, [0, 2, 2, 3], b"\x01\0\0\0" + b"\0\0\0\0" + b"\xff\xff\0\0")
    import torch
    if not torch.cuda.is_available():                             # no CPU fallback: without a context there is nothing to reserve or verify over
        with pytest.raises(N.MblsError):
            N.Context(0)
