"""CPU checks of mbls_verify_multiple_batches_committee_msgtable* (include/mbls.h, "MANY verify_multiple BATCHES PER CALL OVER COMMITTEE BITFIELDS AND THE
RESIDENT MESSAGE TABLE"): the grouping arithmetic of milagro_bls_amd/csrc/mbls_vbg.h, built with the host compiler under AddressSanitizer and UBSan
(tests/vbg_emul/mbls_vbg_harness.cpp, a stand-alone program) and held word for word to the Python model of tests/vbg_cases.py; the plan function at every
boundary of the routing rule; and the new symbols and kernels as the library carries them."""
import os
import subprocess

import pytest

import helpers
import vbg_cases as V

ROOT = helpers.ROOT
NEW_ENTRIES = ("mbls_verify_multiple_batches_committee_msgtable_device", "mbls_verify_multiple_batches_committee_msgtable_locate_device",
               "mbls_verify_multiple_batches_committee_msgtable_rng", "mbls_verify_multiple_batches_committee_msgtable_locate_rng",
               "mbls_plan_verify_multiple_batches_committee", "mbls_vbg_group_probe")
NEW_KERNELS = ("k_vbg_group", "k_vbg_scatter", "k_vbg_key_tree", "k_vbg_heads", "k_vbg_gather", "k_vbg_mark")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vbg") / "vbg_harness")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "vbg_emul", "mbls_vbg_harness.cpp")])

    def run(cases):
        text = ""
        for idx, T, B, spb, off, mg in cases:
            text += "%d %d %d %d %d %s %s\n" % (len(idx), T, B, -1 if off is not None else spb, mg, " ".join(map(str, idx)), " ".join(map(str, off or [])))
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-4000:]
        res = [[[int(x) for x in part.split()] for part in line.split("|")] for line in out.stdout.splitlines()]
        assert len(res) == len(cases)
        return res
    return run


def test_grouping_equals_the_model(harness):
    """every array of the wave -- positions, set words, ranges, batch-local group records, counts, offsets -- equals the model's word for word: batch sizes 0, 1,
    2, 63, 64, 65, 129, the cap and the cap + 1; one entry, distinct entries, indices at and above T, T = 0; tables that run backwards, overlap or leave sets
    uncovered; and the wave agrees with the sequential statement vbg_group_batch and writes nothing outside its batch's range"""
    cs = V.cases()
    for (idx, T, B, spb, off, mg), got in zip(cs, harness(cs)):
        want = V.model(idx, T, B, spb, off)
        names = ("pos", "status", "pos_lo", "pos_hi", "head", "entry", "count", "off")
        for name, words in zip(names, got[:8]):
            assert words == want[name], (name, len(idx), T, B, spb, off)
        assert got[10] == [0], "wave and sequential statement differ, or a write left the batch's range"


def test_overflow_rule(harness):
    """a batch whose groups reach beyond the bound is flagged, the batches in front of it are not, and exactly the groups of batches that do not overflow are
    live Miller items -- under no promise, the exact count, half of it and 1"""
    cs = [c for c in V.cases() if c[5]] + [c for c in V.cases() if not c[5]][:12]
    seen_overflow = seen_clean = False
    for (idx, T, B, spb, off, mg), got in zip(cs, harness(cs)):
        goff = V.model(idx, T, B, spb, off)["off"]
        bnd = V.bound(len(idx), B, T, spb, mg)
        assert got[8][0] == bnd
        flags = [1 if goff[b + 1] > bnd else 0 for b in range(B)]
        assert got[8][1:] == flags
        assert got[9] == V.live(goff, B, bnd)
        assert flags == sorted(flags), "an overflowing batch in front of one that fits"
        seen_overflow |= any(flags)
        seen_clean |= mg != 0 and not any(flags)
    assert seen_overflow and seen_clean


def test_plan_at_the_routing_boundaries():
    """auto groups exactly when 2 x bound <= n_sets, with bound the smallest of n_sets, n_batches x T, n_batches x sets_per_batch and max_groups; modes 1 and 2
    force the route; Miller items, levels and workspace follow the route"""
    from milagro_bls_amd import _native as N
    P = N.plan_verify_multiple_batches_committee
    for n, B, spb in ((64, 1, 64), (64, 1, 0), (200, 20, 10), (200, 7, 0), (1, 1, 1), (65, 65, 1), (2048, 2, 1024), (2050, 2, 1025)):
        for T in (1, 2, n // (2 * B), n // (2 * B) + 1, n, 5 * n):
            for mg in (0, 1, n // 2, n // 2 + 1, n):
                if T == 0:
                    continue
                bnd = V.bound(n, B, T, spb, mg)
                for locate in (False, True):
                    p = P(n, B, spb, T, mg, 0, locate)
                    grouped = 2 * bnd <= n
                    assert p["bound"] == bnd
                    assert p["route"] == (N.VM_ROUTE_GROUPED if grouped else N.VM_ROUTE_PER_SET), (n, B, spb, T, mg)
                    assert p["miller_items"] == (B + bnd if grouped else n + B)
                    longest = spb or n
                    lv = lambda m: max(0, (m - 1).bit_length())
                    if grouped:
                        assert p["tree_levels"] == lv(min(longest, N.VBG_MAX_SETS)) and p["product_levels"] == lv(min(longest, bnd))
                        assert p["workspace_items"] == max(n, B + bnd) + n + 2 * B + (2 * n if locate else 0)
                    else:
                        assert p["tree_levels"] == p["product_levels"] == lv(longest)
                        assert p["workspace_items"] == n + 2 * B + (n if locate else 0)
                    assert P(n, B, spb, T, mg, 1, locate)["route"] == N.VM_ROUTE_GROUPED and P(n, B, spb, T, mg, 2, locate)["route"] == N.VM_ROUTE_PER_SET
    # the Miller form follows bound + n_batches on the grouped route
    L = N.default_limits()
    n, B = 60000, 1000
    assert P(n, B, 60, 2, 0, 0, False, L)["miller_items"] == 3 * B
    for bad in ((0, 1, 0, 1, 0, 0), (1, 0, 0, 1, 0, 0), (10, 2, 4, 1, 0, 0), (10, 2, 5, 1, 0, 3)):
        with pytest.raises(N.MblsError):
            P(*bad)


def test_symbols_and_kernels():
    """the library exports the new entries, and the grouped route's kernels are in a code object of their own"""
    lib = os.path.join(ROOT, "milagro_bls_amd", "libmbls_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in NEW_ENTRIES:
        assert " T %s\n" % name in syms, name
    for k in NEW_KERNELS:
        assert k in syms, k
    src = open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_kernels.hip")).read()
    for k in NEW_KERNELS:
        assert "__global__" not in "".join(l for l in src.splitlines() if k + "(" in l), k
