"""The draw order of the verify_multiple*_rng entries without a GPU (milagro_bls_amd/csrc/mbls_vmr.h through tests/vmr_emul/mbls_vmr_harness.cpp): which sets get
a scalar from the caller's generator, in which order, and what locate mode answers for the sets that never got one. The model is the reference's loop
(src/aggregates.rs:272-287) written out below: B consecutive calls sharing one generator, each drawing for set i only after set i's signature passed and stopping
at the first that does not. The harness also runs as a program of its own under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import pytest

import helpers

CXX = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
DIR = os.path.join(helpers.ROOT, "tests", "vmr_emul")
SRC = os.path.join(DIR, "mbls_vmr_harness.cpp")
BAD_ENC, NOT_G2 = 0x01, 0x02
BAD = (BAD_ENC, NOT_G2, BAD_ENC | NOT_G2, NOT_G2 | 0x104)
OTHER = (0x04, 0x80, 0x100, 0xFFFFFFFC)          # bits beside the two rejecting ones
POISON_RES, POISON_ST = 7, 0xDEADBEEF


# ---- the model
def reference_calls(st, ranges, generator):
    """B calls of the reference, one after the other on one generator -> (per-batch number of draws, the scalar every set was given or None)"""
    given, reach = [None] * len(st), []
    for lo, hi in ranges:
        drew = 0
        for i in range(lo, hi):
            if st[i] & (BAD_ENC | NOT_G2):
                break                                  # :273-275: the call returns false, the generator stays where it is
            given[i] = next(generator); drew += 1      # :280-287
        reach.append(drew)
    return reach, given


@pytest.fixture(scope="module")
def vr():
    so = os.path.join(DIR, "libmbls_vmr_harness.so")
    deps = [SRC, os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc", "mbls_vmr.h"), os.path.join(helpers.ROOT, "include", "mbls.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.vr_reach.restype = C.c_uint64; lib.vr_reach.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    lib.vr_range.restype = None; lib.vr_range.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.vr_plan.restype = C.c_uint64; lib.vr_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    lib.vr_spread.restype = None; lib.vr_spread.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    lib.vr_close.restype = None; lib.vr_close.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def fill(kind, sizes, rnd):
    """status words for batches of the given sizes"""
    st = []
    for m in sizes:
        for j in range(m):
            other = rnd.choice(OTHER) if rnd.random() < 0.5 else 0
            st.append({"good": 0, "bad": rnd.choice(BAD), "first": rnd.choice(BAD) if j == 0 else other, "last": rnd.choice(BAD) if j == m - 1 else other,
                       "other": rnd.choice(OTHER), "seeded": (rnd.choice(BAD) | other) if rnd.random() < 0.2 else other}[kind])
    return st


def cases():
    rnd = random.Random(20251)
    out = []
    for kind in ("good", "bad", "first", "last", "other", "seeded"):
        for B in (1, 2, 3, 5, 8):
            for spb in (0, 1, 2, 5):                                       # uniform counts; 0: n = 0 with B > 0
                out.append((kind, [spb] * B, False)); out.append((kind, [spb] * B, True))
            for shape in ("seeded", "front", "middle", "end", "alternate"):   # tables, with empty batches
                sizes = [rnd.randint(1, 6) for _ in range(B)]
                if shape == "front": sizes[0] = 0
                if shape == "middle": sizes[B // 2] = 0
                if shape == "end": sizes[-1] = 0
                if shape == "alternate": sizes[::2] = [0] * len(sizes[::2])
                out.append((kind, sizes, True))
    return [(kind, sizes, table, fill(kind, sizes, rnd)) for kind, sizes, table in out]


CASES = cases()


def arrays(sizes, table, st):
    n, B = len(st), len(sizes)
    boff = (C.c_uint32 * (B + 1))(*[sum(sizes[:b]) for b in range(B + 1)]) if table else None
    spb = 0xDEAD if table else sizes[0]
    ranges = [(sum(sizes[:b]), sum(sizes[:b + 1])) for b in range(B)]
    return n, B, boff, spb, ranges, (C.c_uint32 * max(1, n))(*st)


def test_the_cases_cover_what_they_should():
    kinds = {k for k, _, _, _ in CASES}
    assert kinds == {"good", "bad", "first", "last", "other", "seeded"}
    assert any(len(s) == 1 for _, s, _, _ in CASES) and any(sum(s) == 0 and len(s) > 1 for _, s, _, _ in CASES)
    assert any(t and s[0] == 0 and sum(s) for _, s, t, _ in CASES) and any(t and s[-1] == 0 and sum(s) for _, s, t, _ in CASES)
    assert any(t and len(s) > 2 and s[len(s) // 2] == 0 and s[0] and s[-1] for _, s, t, _ in CASES)
    assert all(not (w & (BAD_ENC | NOT_G2)) for k, _, _, st in CASES if k == "other" for w in st) and any(w for k, _, _, st in CASES if k == "other" for w in st)


def test_ranges_and_reach(vr):
    for kind, sizes, table, st in CASES:
        n, B, boff, spb, ranges, cst = arrays(sizes, table, st)
        reach, _ = reference_calls(st, ranges, iter(range(1000, 10 ** 6)))
        for b, (lo, hi) in enumerate(ranges):
            glo, ghi = C.c_uint64(99), C.c_uint64(99)
            vr.vr_range(boff, spb, b, C.byref(glo), C.byref(ghi))
            assert (glo.value, ghi.value) == (lo, hi), (kind, sizes, table, b)
            assert vr.vr_reach(cst, lo, hi) == reach[b], (kind, sizes, table, b)
    # 64-bit positions: a range that starts above 2^32 is walked from there (the words are addressed from a base moved back by as much)
    words = (C.c_uint32 * 4)(0x104, 0, NOT_G2, 0)
    base = C.addressof(words) - 4 * (1 << 33)
    assert vr.vr_reach(base, 1 << 33, (1 << 33) + 4) == 2 and vr.vr_reach(base, (1 << 33) + 3, (1 << 33) + 4) == 1


def test_total_reach_and_every_scalar(vr):
    for kind, sizes, table, st in CASES:
        n, B, boff, spb, ranges, cst = arrays(sizes, table, st)
        want_reach, given = reference_calls(st, ranges, iter(range(1000, 10 ** 6)))
        reach = (C.c_uint64 * B)(*([POISON_ST] * B))
        total = vr.vr_plan(cst, boff, spb, B, reach)
        assert total == sum(want_reach) == sum(g is not None for g in given), (kind, sizes, table)
        assert list(reach) == want_reach, (kind, sizes, table)
        drawn = (C.c_uint64 * max(1, total))(*range(1000, 1000 + total))          # what `draw` hands back: the generator's next `total` values, in order
        rands = (C.c_uint64 * max(1, n))(*([POISON_ST] * max(1, n)))
        vr.vr_spread(drawn, reach, boff, spb, B, rands)
        assert list(rands)[:n] == [1 if g is None else g for g in given], (kind, sizes, table)
        if n == 0:
            assert rands[0] == POISON_ST


def test_close_writes_the_sets_behind_the_reaches_and_no_other(vr):
    for kind, sizes, table, st in CASES:
        n, B, boff, spb, ranges, cst = arrays(sizes, table, st)
        want_reach, given = reference_calls(st, ranges, iter(range(1000, 10 ** 6)))
        reach = (C.c_uint64 * B)(*want_reach)
        sres = (C.c_uint8 * max(1, n))(*([POISON_RES] * max(1, n))); sst = (C.c_uint32 * max(1, n))(*([POISON_ST] * max(1, n)))
        vr.vr_close(cst, reach, boff, spb, B, sres, sst)
        assert list(sres)[:n] == [0 if g is None else POISON_RES for g in given], (kind, sizes, table)
        assert list(sst)[:n] == [st[i] if g is None else POISON_ST for i, g in enumerate(given)], (kind, sizes, table)
        if n == 0:
            assert (sres[0], sst[0]) == (POISON_RES, POISON_ST)
        sres2 = (C.c_uint8 * max(1, n))(*([POISON_RES] * max(1, n)))
        vr.vr_close(cst, reach, boff, spb, B, sres2, None)                         # the words are optional
        assert list(sres2) == list(sres)


def test_every_rng_entry_goes_through_the_header():
    """the rule exists once: no _rng implementation spells the rejecting pair of bits or a batch's range itself"""
    with open(os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc", "mbls_kernels.hip")) as f:
        src = f.read()
    assert "MBLS_ST_BAD_SIG_ENCODING | MBLS_ST_SIG_NOT_IN_G2" not in src
    assert "boff ? boff[b]" not in src
    assert src.count("vmr_reach(") == 3 and src.count("vmr_plan(") == 1 and src.count("vmr_spread(") == 1 and src.count("vmr_close(") == 2


def test_harness_as_its_own_program_under_asan_and_ubsan():
    """the same kinds of cases over heap buffers of exactly n words, n scalars, B reaches and B + 1 offsets: a read or a write past any of them aborts the program"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "vmr_harness")
        subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMBLS_VMR_HARNESS_MAIN", "-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-300:], r.stderr[-2000:])
