"""CPU checks of mbls_verify_multiple*_msgtable* (include/mbls.h, "verify_multiple OVER THE RESIDENT MESSAGE TABLE"): the step from the sets' table indices to
the Miller items, milagro_bls_amd/csrc/mbls_vmt.h, built with the host compiler under AddressSanitizer and UBSan (tests/vmt_emul/mbls_vmt_harness.cpp, a
stand-alone program) and compared with a Python model; and the new symbols and kernels as the library carries them."""
import os
import random
import subprocess

import pytest

import helpers

ROOT = helpers.ROOT
NO = 0xFFFFFFFF
NEW_ENTRIES = ("mbls_verify_multiple_msgtable_device", "mbls_verify_multiple_sets_indexed_msgtable_device", "mbls_verify_multiple_msgtable_rng",
               "mbls_verify_multiple_msgtable_locate_device", "mbls_verify_multiple_sets_indexed_msgtable_locate_device", "mbls_verify_multiple_msgtable_locate_rng",
               "mbls_plan_verify_multiple_msgtable", "mbls_plan_verify_multiple_msgtable_workspace_items", "mbls_plan_verify_multiple_msgtable_locate_workspace_items")
NEW_KERNELS = ("k_vmt_flag", "k_vmt_named", "k_vmt_heads", "k_vmt_miller", "k_vmt_miller2")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vmt") / "vmt_harness")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "vmt_emul", "mbls_vmt_harness.cpp")])

    def run(cases):
        """cases: (n, T, miller_items, idx) -> per case (D, overflow, idle_from, named, [(live, idx, pos, map)] per Miller item)"""
        text = "".join("%d %d %d %s\n" % (n, T, items, " ".join(map(str, idx))) for n, T, items, idx in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-4000:]
        res = []
        for line in out.stdout.splitlines():
            head, named, items = line.split("|")
            D, overflow, idle = (int(x) for x in head.split())
            w = [int(x) for x in items.split()]
            res.append((D, overflow, idle, [int(x) for x in named.split()], [tuple(w[4 * i:4 * i + 4]) for i in range(len(w) // 4)]))
        assert len(res) == len(cases)
        return res
    return run


def cases():
    """(n, T, miller_items, idx): T = 1; T = 1025 and 2500 (scan chunks of more than one entry per lane, an uneven last chunk); only entry 0 and only entry T - 1
    named; every entry named; no valid index at all; indices equal to T and to 2^32 - 1; sized as the device entries (min(n, T)) and as the host entries (D)"""
    rnd = random.Random(20271)
    out = []
    for T in (1, 2, 12, 600, 1024, 1025, 2500):
        shapes = {
            "first": [0] * 7,
            "last": [T - 1] * 5,
            "ends": [0, T - 1, 0, T - 1, T - 1],
            "every": rnd.sample(range(T), T) + [rnd.randrange(T) for _ in range(T // 3)],
            "none": [T, NO, T + 1, NO],
            "mixed": [rnd.choice([0, T - 1, T, NO, rnd.randrange(T), T // 2]) for _ in range(150)],
            "sparse": [rnd.choice([0, T - 1, T // 2, min(T - 1, T // 2 + 1)]) for _ in range(150)],
            "one": [rnd.randrange(T)],
        }
        for idx in shapes.values():
            n = len(idx)
            D = len({j for j in idx if j < T})
            out.append((n, T, max(min(n, T), 1), idx))       # the device entries' bound
            out.append((n, T, max(D, 1), idx))               # the host entries' exact count
    out.append((3, 0, 1, [0, 1, NO]))                        # an empty table: every index names nothing
    return out


def test_named_entries_and_heads_match_the_model(harness):
    """named = the sorted distinct valid indices, D their number; Miller item r < D gets entry named[r] and the first position of that entry's range (the number
    of sets naming a smaller entry), where the scatter's map names the same entry; items at or above D are idle (the private entry, position 0); D never
    exceeds the Miller items either bound gives; and the harness -- built with -fsanitize=address,undefined as a stand-alone program -- runs clean"""
    cs = cases()
    for (n, T, items, idx), (D, overflow, idle, named, heads) in zip(cs, harness(cs)):
        valid = [j for j in idx if j < T]
        want = sorted(set(valid))
        assert named == want and D == len(want), (n, T)
        assert overflow == 0 and idle == min(D, items), (n, T, items, D)
        assert len(heads) == items
        for r, (live, e, pos, owner) in enumerate(heads):
            if r < D:
                assert (live, e, pos, owner) == (1, want[r], sum(1 for j in valid if j < want[r]), want[r]), (n, T, r)
            else:
                assert (live, e, pos, owner) == (0, NO, 0, NO), (n, T, r)


def test_a_bound_below_the_named_entries_is_reported(harness):
    """fail closed: were a call sized with fewer Miller items than it names entries, the device would see it (vmt_overflow) and reject"""
    (D, overflow, idle, named, heads), = harness([(6, 10, 2, [1, 3, 5, 7, 3, 1])])
    assert D == 4 and overflow == 1 and named == [1, 3, 5, 7] and len(heads) == 2 and idle == 2


def test_new_symbols_and_kernels_are_in_the_library():
    from milagro_bls_amd import _native as N
    lib = N.lib()
    for name in NEW_ENTRIES:
        assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, "milagro_bls_amd", "libmbls_hip.so"), "rb") as f:
        blob = f.read()
    for k in NEW_KERNELS:
        assert k.encode() in blob, k
