"""CPU checks of mbls_verify_multiple_committee_msgtable* (include/mbls.h, "verify_multiple OVER COMMITTEE BITFIELDS AND THE RESIDENT MESSAGE TABLE"): the set
descriptor and the whole-set expansion, milagro_bls_amd/csrc/mbls_vmc.h, built with the host compiler under AddressSanitizer and UBSan
(tests/vmc_emul/mbls_vmc_harness.cpp, a stand-alone program) and compared with a Python restatement; the planning functions the entries share with the _msgtable
entries; the new symbols and kernels as the library carries them; and what the entries refuse without a GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import helpers

ROOT = helpers.ROOT
SINGLE = 0x80000000
NO_COMMITTEE = 0xFFFFFFFF
SIZES = (1, 31, 32, 33, 63, 64, 65, 128, 129, 2048)
TSIZE = 136
NEW_ENTRIES = ("mbls_verify_multiple_committee_msgtable_device", "mbls_verify_multiple_committee_msgtable_locate_device",
               "mbls_verify_multiple_committee_msgtable_rng", "mbls_verify_multiple_committee_msgtable_locate_rng")
NEW_KERNELS = ("k_vmc_expand", "k_aggregate_vmc_d")


# ---- the restatement
def model_set(word, committees, bits, mode):
    """(single, key_index, count, route word, list) of one set; committees: [(m, eligible)], committee c's member j is 1000 c + 7 j"""
    if word & SINGLE:
        return 1, word & 0x7FFFFFFF, 1, 0, [word & 0x7FFFFFFF]
    if word >= len(committees):
        return 0, word, 1, 0, [NO_COMMITTEE]
    m, eligible = committees[word]
    sel = [j for j in range(m) if (bits[j >> 3] >> (j & 7)) & 1]
    comp = bool(eligible) and mode != 1 and (mode == 2 or (m - len(sel)) + 1 < len(sel))
    listed = [j for j in range(m) if (j in set(sel)) != comp]
    return 0, word, len(listed), (1 if comp else 0) | (2 if not sel else 0), [1000 * word + 7 * j for j in listed]


def model_refused(word, ccount, tsize):
    return (word & 0x7FFFFFFF) >= tsize if word & SINGLE else word >= ccount


def patterns(m, rnd):
    """nobody, first, last, everybody, all-but-one, half, half + 1 -- each also with every bit from m to the end of the last word set (a Bitlist's delimiter among
    them) -- and the delimiter bit alone above each"""
    nbytes = 4 * ((m + 31) // 32)
    half = sorted(rnd.sample(range(m), m // 2))
    rest = [j for j in range(m) if j not in half]
    sels = [[], [0], [m - 1], list(range(m)), list(range(1, m)), list(range(m - 1)), half, sorted(half + rest[:1])]
    out = []
    for sel in sels:
        for stray in ((), range(m, 8 * nbytes), [m] if m < 8 * nbytes else ()):
            b = bytearray(nbytes)
            for j in list(sel) + list(stray):
                b[j >> 3] |= 1 << (j & 7)
            out.append(bytes(b))
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vmc") / "vmc_harness")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "vmc_emul", "mbls_vmc_harness.cpp")])

    def run(committees, tsize, sets):
        """sets: (word, mode, bits or None) -> per set (single, key_index, refused, count, route, list)"""
        text = "%d %d\n" % (len(committees), tsize) + "".join("%d %d\n" % c for c in committees) + "%d\n" % len(sets)
        text += "".join("%d %d %s\n" % (w, mode, bits.hex() if bits is not None else "-") for w, mode, bits in sets)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
        res = []
        for line in out.stdout.splitlines():
            v = [int(x) for x in line.split()]
            res.append((v[0], v[1], v[2], v[3], v[4], v[5:]))
        assert len(res) == len(sets)
        return res
    return run


def test_committee_sets_of_every_size_pattern_route_and_eligibility(harness):
    """the expansion of a committee set is the committee entries': the listed members in member order, the count, the route word; bits above the size ignored"""
    rnd = random.Random(77)
    committees = [(m, el) for m in SIZES for el in (1, 0)]
    sets = [(c, mode, bits) for c, (m, _el) in enumerate(committees) for bits in patterns(m, rnd) for mode in (0, 1, 2)]
    got = harness(committees, TSIZE, sets)
    for (w, mode, bits), (single, key, refused, cnt, route, lst) in zip(sets, got):
        assert (single, key, cnt, route, lst) == model_set(w, committees, bits, mode), (w, committees[w], mode, bits.hex())
        assert refused == 0
        assert cnt == len(lst) <= committees[w][0]
        if not committees[w][1]:
            assert not route & 1                                 # an ineligible committee always goes direct


def test_words_that_name_no_committee_and_single_key_sets(harness):
    """an id at the count and 0x7FFFFFFF list the one index 0xFFFFFFFF; 0x80000000 is key 0, 0xFFFFFFFF key 0x7FFFFFFF (outside every table: it still rejects);
    single-key sets of every index list that index, count 1, direct, route word 0 -- under every mode, and WITHOUT a bitfield: the harness hands them a null pointer"""
    committees = [(m, 1) for m in SIZES]
    words = [len(committees), len(committees) + 1, 0x7FFFFFFF, SINGLE, SINGLE | 1, SINGLE | (TSIZE - 1), SINGLE | TSIZE, SINGLE | 0x7FFFFFFE, 0xFFFFFFFF]
    sets = [(w, mode, None) for w in words for mode in (0, 1, 2)]
    got = harness(committees, TSIZE, sets)
    for (w, mode, _b), (single, key, refused, cnt, route, lst) in zip(sets, got):
        assert (single, key, cnt, route, lst) == model_set(w, committees, None, mode), hex(w)
        assert refused == int(model_refused(w, len(committees), TSIZE)), hex(w)
        assert cnt == 1 and route == 0
    by = {w: got[3 * i] for i, w in enumerate(words)}
    assert by[len(committees)][5] == [NO_COMMITTEE] and by[0x7FFFFFFF][5] == [NO_COMMITTEE] and by[0x7FFFFFFF][0] == 0
    assert by[SINGLE][:2] == (1, 0) and by[SINGLE][5] == [0] and by[SINGLE][2] == 0
    assert by[0xFFFFFFFF][:3] == (1, 0x7FFFFFFF, 1) and by[0xFFFFFFFF][5] == [0x7FFFFFFF]
    assert by[SINGLE | (TSIZE - 1)][2] == 0 and by[SINGLE | TSIZE][2] == 1
    # an empty committee table: every committee id names nothing, single-key sets are what they were
    got = harness([], TSIZE, [(0, 0, None), (SINGLE | 5, 0, None)])
    assert got[0][3:] == (1, 0, [NO_COMMITTEE]) and got[0][2] == 1 and got[1][3:] == (1, 0, [5]) and got[1][2] == 0


def test_the_committee_source_plans_with_the_msgtable_functions():
    """routing and workspace of the committee entries are mbls_plan_verify_multiple_msgtable, _workspace_items and _locate_workspace_items, unchanged: the header
    says so in the entries' section, no planning symbol of their own exists, the key source reserves nothing in the workspace beside what those functions state
    (its scratch is the committee entries': reserve_committee), and the Python mirror hands out the same three functions"""
    from milagro_bls_amd import batch, _native as N
    with open(os.path.join(ROOT, "include", "mbls.h")) as f:
        header = f.read()
    section = header[header.index("verify_multiple OVER COMMITTEE BITFIELDS"):header.index("#define MBLS_VM_SET_SINGLE_KEY")]
    for name in ("mbls_plan_verify_multiple_msgtable", "_workspace_items", "_locate_workspace_items", "UNCHANGED"):
        assert name in section, name
    assert not re.search(r"mbls_plan_verify_multiple_committee", header)
    assert not hasattr(N.lib(), "mbls_plan_verify_multiple_committee_msgtable")
    with open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_kernels.hip")) as f:
        src = f.read()
    impl = src[src.index("static int verify_multiple_impl("):src.index("// verify_multiple over sets named by indices into a resident key table")]
    assert impl.count("mbls_ctx_reserve(") == 1 and impl.count("vm_shared_plan_and_reserve(") == 1          # the one reservation of the workspace, source or no source
    assert "reserve_committee(c, n, ks.cmax)" in impl
    # the same values, whatever the sets' kinds: the functions do not know the key source
    L = N.default_limits()
    for n, T, named, mode in ((1, 1, 0, 0), (65, 3, 0, 0), (200, 8, 3, 1), (65536, 512, 0, 0), (65536, 512, 512, 2), (1024, 8, 8, 0)):
        a = batch.plan_verify_multiple_msgtable_workspace_items(n, T, named, mode, limits=L)
        assert a == N.plan_verify_multiple_msgtable_workspace_items(n, T, named, mode, limits=L) and a >= n
        b = batch.plan_verify_multiple_msgtable_locate_workspace_items(n, T, named, mode, limits=L)
        assert b > a
        assert batch.plan_verify_multiple_msgtable(n, T, named, mode, limits=L)["workspace_items"] == a


def test_new_symbols_and_kernels_are_in_the_library():
    from milagro_bls_amd import batch, _native as N
    import milagro_bls_amd as pkg
    lib = N.lib()
    for name in NEW_ENTRIES:
        assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, "milagro_bls_amd", "libmbls_hip.so"), "rb") as f:
        blob = f.read()
    for k in NEW_KERNELS + ("k_cmt_expand", "k_aggregate_cmt_d"):
        assert k.encode() in blob, k
    assert N.VM_SET_SINGLE_KEY == batch.VM_SET_SINGLE_KEY == SINGLE
    with open(os.path.join(ROOT, "include", "mbls.h")) as f:
        assert "#define MBLS_VM_SET_SINGLE_KEY 0x80000000u" in f.read()
    assert pkg.SingleKey(5).index == 5
    for bad in (-1, SINGLE):
        with pytest.raises(ValueError):
            pkg.SingleKey(bad)
    for f in ("verify_multiple_aggregate_signatures_committee", "verify_multiple_aggregate_signatures_committee_locate"):
        assert callable(getattr(pkg.AggregateSignature, f))
    # an empty iterator is true and touches nothing, as in the reference
    assert pkg.AggregateSignature.verify_multiple_aggregate_signatures_committee(None, [], None, None) is True
    assert pkg.AggregateSignature.verify_multiple_aggregate_signatures_committee_locate(None, [], None, None) == (True, [])


def test_entries_refuse_null_handles_without_a_gpu():
    """no context, no committee table or no message table: MBLS_ERR_ARGUMENT, the outputs untouched, the scalar source never asked"""
    from milagro_bls_amd import _native as N
    L = N.lib()
    asked = []
    cb = N.SCALAR_SOURCE(lambda _u, _out, count: asked.append(count))
    res = (C.c_uint8 * 4)(9, 9, 9, 9); sres = (C.c_uint8 * 4)(7, 7, 7, 7); sst = (C.c_uint32 * 4)(5, 5, 5, 5)
    one = (C.c_uint32 * 1)(0)
    assert L.mbls_verify_multiple_committee_msgtable_device(None, None, None, None, None, 4, None, None, None, 1, res, None, None) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_committee_msgtable_locate_device(None, None, None, None, None, 4, None, None, None, 1, res, None, sres, sst, None) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_committee_msgtable_rng(None, None, None, one, None, 4, None, one, 1, res, cb, None) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_committee_msgtable_locate_rng(None, None, None, one, None, 4, None, one, 1, res, sres, sst, cb, None) == N.ERR_ARGUMENT
    assert list(res) == [9] * 4 and list(sres) == [7] * 4 and list(sst) == [5] * 4 and asked == []
    import torch
    if not torch.cuda.is_available():                             # no CPU fallback: without a context there are no tables to verify over
        with pytest.raises(N.MblsError):
            N.Context(0)
