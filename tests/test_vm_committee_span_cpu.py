"""verify_multiple over committee spans without a GPU (include/mbls.h, mbls_verify_multiple_committee_span_msgtable*): the descriptor predicates, the expansion of a
set, the chunk ranges and the split rule of milagro_bls_amd/csrc/mbls_vcs.h on the host (tests/vcs_emul/mbls_vcs_harness.cpp) against a Python model;
mbls_plan_verify_multiple_span through ctypes; the harness as a program of its own under the address and undefined-behaviour sanitizers; and what the
entries refuse without a context."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import pytest

import helpers

CXX = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
DIR = os.path.join(helpers.ROOT, "tests", "vcs_emul")
SRC = os.path.join(DIR, "mbls_vcs_harness.cpp")
CSRC = os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc")
SINGLE = 0x80000000
POISON = 0xDEADBEEF
REC = 40                                    # MBLS_CMT_REC_DWORDS: [0] first member, [1] size, [2] eligible
SIZES = [1, 31, 32, 33, 63, 64, 65, 129]
ELIGIBLE = [1, 1, 1, 0, 1, 1, 1, 1]
SPLITS = (1, 2, 4, 8, 16)


@pytest.fixture(scope="module")
def vh():
    so = os.path.join(DIR, "libmbls_vcs_harness.so")
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mbls_vcs.h", "mbls_vmc.h", "mbls_cms.h", "mbls_cmt.h")] + [os.path.join(helpers.ROOT, "include", "mbls.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    u32, u64, i, vp = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
    for name, res, args in (("vh_is_single", i, [u32, u32]), ("vh_id_ok", i, [u32, u64]), ("vh_single_names_nothing", i, [u32, u64]), ("vh_key_status", u32, [u32]),
                            ("vh_expand", i, [u32, u32, vp, u64, vp, u64, vp, vp, u32, i, vp, u64, vp]), ("vh_chunk_lo", u32, [u32, u32, u32]),
                            ("vh_lane_set", u64, [u64, u32]), ("vh_lane_list", u32, [u64, u32]), ("vh_lane_chunk", u32, [u64, u32]), ("vh_lane_of", u64, [u64, u32, u32, u32]),
                            ("vh_extra_items", u64, [u64, u32]), ("vh_split_mode_ok", i, [i]), ("vh_split", u32, [u64, u64, u64, i]), ("vh_split_max_sets", u32, []),
                            ("vh_min_chunk", u32, [])):
        getattr(lib, name).restype = res; getattr(lib, name).argtypes = args
    return lib


def table():
    """committee records and a member array of exactly the committees' total"""
    crecs, first = [], 0
    for m, e in zip(SIZES, ELIGIBLE):
        crecs += [first, m, e] + [0] * (REC - 3)
        first += m
    return crecs, [700 + 5 * j for j in range(first)]


def model_expand(ids, n_ids, lo, hi, field, bits_stride, mode):
    """-> ("single", key) | ("reject",) | ("span", direct list, missing list in (segment, member) order, mask, nobody): key-table indices"""
    if hi < lo or hi > n_ids or hi - lo > 64:
        return ("reject",)
    own = ids[lo:hi]
    if len(own) == 1 and own[0] & SINGLE:
        return ("single", own[0] & 0x7FFFFFFF)
    if any(x & SINGLE or x >= len(SIZES) for x in own):
        return ("reject",)
    if sum(SIZES[x] for x in own) > 8 * bits_stride:
        return ("reject",)
    _c, members = table()
    firsts = [sum(SIZES[:x]) for x in own]
    direct, missing, mask, o, total = [], [], 0, 0, 0
    for t, x in enumerate(own):
        m = SIZES[x]
        sel = [j for j in range(m) if (field[(o + j) >> 3] >> ((o + j) & 7)) & 1]
        comp = bool(ELIGIBLE[x]) and mode != 1 and (mode == 2 or (m - len(sel)) + 1 < len(sel))
        if comp:
            mask |= 1 << t
            missing += [members[firsts[t] + j] for j in range(m) if j not in sel]
        else:
            direct += [members[firsts[t] + j] for j in sel]
        o += m; total += len(sel)
    return ("span", direct, missing, mask, total == 0)


def run_expand(vh, ids, n_ids, lo, hi, field, bits_stride, mode):
    crecs, members = table()
    stride = max(1, min(8 * bits_stride, 64 * max(SIZES)))
    region = (C.c_uint32 * stride)(*([POISON] * stride)); rec = (C.c_uint32 * 5)(*([POISON] * 5))
    kind = vh.vh_expand(lo, hi, (C.c_uint32 * max(1, len(ids)))(*ids), n_ids, (C.c_uint32 * len(crecs))(*crecs), len(SIZES), (C.c_uint32 * len(members))(*members),
                        (C.c_uint32 * max(1, bits_stride // 4)).from_buffer_copy(bytes(field).ljust(max(4, bits_stride), b"\0")), bits_stride, mode, region, stride, rec)
    out = list(region)
    if kind == 0:
        assert list(rec) == [1, 0, 0, 0, 0] and out[1:] == [POISON] * (stride - 1)
        return ("single", out[0])
    if kind == 2:
        assert list(rec) == [1, 0, 0, 0, 0] and out[0] == 0xFFFFFFFF and out[1:] == [POISON] * (stride - 1)
        return ("reject",)
    nd, nm = rec[0], rec[1]
    assert kind == 1 and out[nd:stride - nm] == [POISON] * (stride - nm - nd)
    return ("span", out[:nd], out[stride - nm:][::-1], rec[2] | (rec[3] << 32), bool(rec[4]))


def test_descriptor_predicates(vh):
    for q in (0, 1, 2, 64):
        for word in (0, 5, 0x7FFFFFFF, SINGLE, SINGLE | 5, 0xFFFFFFFF):
            assert vh.vh_is_single(q, word) == int(q == 1 and bool(word & SINGLE)), (q, hex(word))      # bit 31 as the SOLE id, never among several
    for word, count, want in ((0, 1, 1), (7, 8, 1), (8, 8, 0), (SINGLE | 1, 8, 0), (SINGLE, 1 << 33, 0), (0x7FFFFFFF, 1 << 31, 1), (0xFFFFFFFF, 1 << 33, 0)):
        assert vh.vh_id_ok(word, count) == want, (hex(word), count)
    for word, tsize, want in ((SINGLE | 5, 6, 0), (SINGLE | 6, 6, 1), (SINGLE, 0, 1), (0xFFFFFFFF, 1 << 31, 0), (0xFFFFFFFF, (1 << 31) - 1, 1)):
        assert vh.vh_single_names_nothing(word, tsize) == want, (hex(word), tsize)
    assert vh.vh_key_status(0xFFFFFFFF) == 0xFFFFFFFF & ~0x18 and vh.vh_key_status(0x24) == 0x24      # NO_KEYS and APK_INFINITY are cut, nothing else


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_expansion_of_single_key_well_formed_and_every_malformed_kind(vh, mode):
    rnd = random.Random(75490 + mode)
    stride = 48                                                   # 384 bits
    field = lambda density: bytes(sum((rnd.random() < density) << b for b in range(8)) for _ in range(stride))
    cases = []
    for ids in ([0], [7], [1, 2], [3, 5], [7, 7], [4, 3, 6], [0] * 64, [0, 1, 0, 1] * 16, []):
        for d in (0.0, 0.3, 0.6, 0.97, 1.0):
            cases.append((ids, len(ids), 0, len(ids), field(d)))
    cases += [([SINGLE | 9], 1, 0, 1, field(0.5)), ([0xFFFFFFFF], 1, 0, 1, field(0.5)), ([3, SINGLE | 9, 2], 3, 1, 2, field(0.5))]      # single-key, also inside a longer id array
    cases += [([SINGLE | 9, 2], 2, 0, 2, field(0.5)), ([2, SINGLE | 9], 2, 0, 2, field(0.5))]                                          # bit 31 among several: malformed
    cases += [([1, 8], 2, 0, 2, field(0.5)), ([8], 1, 0, 1, field(0.5))]                                                                # an id at the count
    cases += [([0] * 65, 65, 0, 65, field(0.5))]                                                                                        # q > 64
    cases += [([1, 2, 3], 3, 2, 1, field(0.5)), ([1, 2, 3], 2, 1, 3, field(0.5))]                                                       # backwards; past n_cmt_ids
    # M > 8 * bits_stride = 384 (sizes 129, 65, 64, 63 under ids 7, 6, 5, 4): 387, 386, 385 -- and 384 exactly, which passes
    cases += [([7, 7, 7], 3, 0, 3, field(0.5)), ([7, 7, 6, 4], 4, 0, 4, field(0.9)), ([7, 7, 5, 4], 4, 0, 4, field(0.9)), ([7, 7, 4, 4], 4, 0, 4, field(0.9))]
    seen = set()
    for ids, n_ids, lo, hi, f in cases:
        want = model_expand(ids, n_ids, lo, hi, f, stride, mode)
        assert run_expand(vh, ids, n_ids, lo, hi, f, stride, mode) == want, (ids[:6], lo, hi)
        seen.add(want[0])
    assert seen == {"single", "reject", "span"}
    assert run_expand(vh, [7, 7, 4, 4], 4, 0, 4, b"\xff" * stride, stride, mode)[0] == "span"


def test_chunk_ranges_tile_the_list(vh):
    for P in SPLITS:
        for L in sorted({0, 1, P - 1, P, P + 1, 323}):
            edges = [vh.vh_chunk_lo(L, P, p) for p in range(P + 1)]
            assert edges == [p * L // P for p in range(P + 1)], (L, P)
            assert edges[0] == 0 and edges[-1] == L and all(a <= b for a, b in zip(edges, edges[1:]))      # no gap, no overlap
            assert max(b - a for a, b in zip(edges, edges[1:])) - min(b - a for a, b in zip(edges, edges[1:])) <= 1
        for g in range(5 * 2 * P):
            i, which, p = vh.vh_lane_set(g, P), vh.vh_lane_list(g, P), vh.vh_lane_chunk(g, P)
            assert (i, which, p) == (g // (2 * P), (g % (2 * P)) // P, g % P) and vh.vh_lane_of(i, which, p, P) == g
        assert vh.vh_extra_items(12, P) == (0 if P == 1 else 2 * P * 12)
    assert vh.vh_chunk_lo(0xFFFFFFFF, 16, 16) == 0xFFFFFFFF and vh.vh_chunk_lo(0xFFFFFFFF, 16, 15) == 15 * 0xFFFFFFFF // 16      # no 32-bit overflow


def model_split(n, stride, R, mode, max_sets, min_chunk):
    if mode not in (0, 1, 2, 4, 8, 16) or n == 0:
        return 1
    if mode == 0 and (2 * n >= R or n > max_sets):
        return 1
    P = mode or 16
    while P > 1 and (2 * P * n > R or (mode == 0 and (4 * P * n > R or stride < P * min_chunk))):
        P //= 2
    return P


def test_split_rule_at_its_boundaries(vh):
    S, K = vh.vh_split_max_sets(), vh.vh_min_chunk()
    assert [vh.vh_split_mode_ok(m) for m in (-1, 0, 1, 2, 3, 4, 5, 8, 16, 17, 32)] == [0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 0]
    for R in (65536, 16384, 1024, 128):
        ns = sorted({1, 2, 12, S - 1, S, S + 1, R // 64 - 1, R // 64, R // 64 + 1, R // 32 - 1, R // 32, R // 32 + 1, R // 8 - 1, R // 8, R // 8 + 1, R // 4 - 1, R // 4, R // 4 + 1, R // 2 - 1, R // 2, R // 2 + 1, R, 3 * R} - {0, -1})
        for n in ns:
            for stride in (1, K, 2 * K - 1, 2 * K, 16 * K - 1, 16 * K, 352, 8192):
                for mode in (0,) + SPLITS:
                    P = vh.vh_split(n, stride, R, mode)
                    assert P == model_split(n, stride, R, mode, S, K), (n, stride, R, mode)
                    assert P == 1 or 2 * P * n <= R                 # every chunk has its lane inside ONE round
                    assert mode or P == 1 or (4 * P * n <= R and n <= S and stride >= P * K)
                    if mode == 0 and 2 * n >= R:
                        assert P == 1                               # where verify_multiple_impl stops forking its chains
    assert vh.vh_split(12, 8192, 65536, 0) == 16 and vh.vh_split(12, 8192, 65536, 3) == 1 and vh.vh_split(0, 8192, 65536, 16) == 1


def test_plan_through_ctypes_equals_the_model(vh):
    from milagro_bls_amd import _native as N
    L = N.lib()
    S, K = vh.vh_split_max_sets(), vh.vh_min_chunk()
    for R in (65536, 4096):
        lim = N.default_limits(R)
        for n in (1, 12, 65, 768, S, S + 1, R // 4, R // 2, R):
            for T in (1, 12, 700):
                for stride in (1, 352, 8192):
                    for mode in (0,) + SPLITS:
                        for locate in (False, True):
                            P, items = N.plan_verify_multiple_committee_span(n, T, stride, locate, mode, lim)
                            base = (N.plan_verify_multiple_msgtable_locate_workspace_items if locate else N.plan_verify_multiple_msgtable_workspace_items)(n, T, limits=lim)
                            assert P == model_split(n, stride, R, mode, S, K) and items == base + (2 * P * n if P > 1 else 0), (n, T, stride, mode, locate)
    split, items = C.c_uint32(7), C.c_uint64(7)
    lim = N.default_limits(65536)
    f = L.mbls_plan_verify_multiple_span
    assert f(None, 12, 12, 8192, 0, 0, C.byref(split), C.byref(items)) == N.ERR_ARGUMENT
    assert f(C.byref(lim), 0, 12, 8192, 0, 0, C.byref(split), C.byref(items)) == N.ERR_ARGUMENT
    assert f(C.byref(lim), 12, 12, 8192, 0, 3, C.byref(split), C.byref(items)) == N.ERR_ARGUMENT
    assert f(C.byref(lim), 12, 12, 8192, 0, 0, None, C.byref(items)) == N.ERR_ARGUMENT and f(C.byref(lim), 12, 12, 8192, 0, 0, C.byref(split), None) == N.ERR_ARGUMENT
    assert (split.value, items.value) == (7, 7)
    assert N.VM_SPAN_SPLITS == (0, 1, 2, 4, 8, 16)


def test_harness_as_its_own_program_under_asan_and_ubsan():
    """the same functions over heap buffers of exactly the promised sizes: a read past the ids, the field or the member array, or a write past the region or the
    record, aborts the program"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "vcs_harness")
        subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMBLS_VCS_HARNESS_MAIN", "-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-300:], r.stderr[-2000:])


def test_entries_refuse_null_handles_and_no_context_exists_without_a_gpu():
    from milagro_bls_amd import _native as N
    L = N.lib()
    res = (C.c_uint8 * 4)(9, 9, 9, 9)
    st = (C.c_uint32 * 4)(7, 7, 7, 7)
    cb = N.SCALAR_SOURCE(lambda _u, _o, _c: None)
    assert L.mbls_verify_multiple_committee_span_msgtable_device(None, None, None, None, 0, None, None, 4, None, None, None, 1, res, st, None) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_committee_span_msgtable_locate_device(None, None, None, None, 0, None, None, 4, None, None, None, 1, res, st, res, st, None) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_committee_span_msgtable_rng(None, None, None, None, 0, None, None, 4, None, None, 1, res, cb, None) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_committee_span_msgtable_locate_rng(None, None, None, None, 0, None, None, 4, None, None, 1, res, res, st, cb, None) == N.ERR_ARGUMENT
    assert L.mbls_ctx_set_vm_span_split(None, 0) == N.ERR_ARGUMENT
    assert list(res) == [9, 9, 9, 9] and list(st) == [7, 7, 7, 7]
    import torch
    if not torch.cuda.is_available():                             # no CPU fallback: without a context there is nothing to verify over
        with pytest.raises(N.MblsError):
            N.Context(0)
