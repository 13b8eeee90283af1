"""CPU checks of mbls_verify_multiple_batches_committee_span_msgtable* (include/mbls.h, "MANY verify_multiple BATCHES PER CALL OVER COMMITTEE SPANS AND THE
RESIDENT MESSAGE TABLE"): mbls_plan_verify_multiple_batches_committee_span at the boundaries of the split rule and on both routes -- the plan is
mbls_plan_verify_multiple_batches_committee's with the partial sums' items added, the split factor mbls_plan_verify_multiple_span's --; the workspace layout of
milagro_bls_amd/csrc/mbls_vbg.h with the partial sums behind it, swept by a stand-alone host program under AddressSanitizer and UBSan
(tests/vbs_emul/mbls_vbs_harness.cpp) and held to the library's plan figure; and the new symbols as the library carries them."""
import os
import subprocess

import pytest

import helpers

ROOT = helpers.ROOT
SPLIT_MODES = (0, 1, 2, 4, 8, 16)
NEW_ENTRIES = ("mbls_verify_multiple_batches_committee_span_msgtable_device", "mbls_verify_multiple_batches_committee_span_msgtable_locate_device",
               "mbls_verify_multiple_batches_committee_span_msgtable_rng", "mbls_verify_multiple_batches_committee_span_msgtable_locate_rng",
               "mbls_plan_verify_multiple_batches_committee_span")
STRIDE_WORDS = 352                          # the span tests' regions: min(8 * 44, 64 * the largest committee)


def boundaries():
    from milagro_bls_amd import _native as N
    R = N.default_limits().round_items
    return (1, 2, 4096, 4097, R // 2 - 1, R // 2)


def layouts(n):
    """(n_batches, sets_per_batch) of a call of n sets: one batch, batches of one, a ragged table of about a dozen sets per batch"""
    return ((1, n), (n, 1), (max(1, n // 12), 0))


def test_plan_is_the_batches_plan_plus_the_partial_sums_at_every_boundary():
    from milagro_bls_amd import _native as N
    seen_split = seen_none = False
    for n in boundaries():
        for B, spb in layouts(n):
            for T in (1, 3, n + 1):
                for mode in (1, 2):                                # both routes
                    for locate in (False, True):
                        base = N.plan_verify_multiple_batches_committee(n, B, spb, T, 0, mode, locate)
                        assert base["route"] == (N.VM_ROUTE_GROUPED if mode == 1 else N.VM_ROUTE_PER_SET)
                        for sm in SPLIT_MODES:
                            plan, P = N.plan_verify_multiple_batches_committee_span(n, B, spb, T, 0, mode, locate, STRIDE_WORDS, sm)
                            P1, _items = N.plan_verify_multiple_committee_span(n, T, STRIDE_WORDS, locate=locate, split_mode=sm)
                            assert P == P1, (n, sm)
                            extra = 2 * P * n if P > 1 else 0
                            assert plan["workspace_items"] == base["workspace_items"] + extra, (n, B, spb, T, mode, locate, sm)
                            assert {k: v for k, v in plan.items() if k != "workspace_items"} == {k: v for k, v in base.items() if k != "workspace_items"}
                            seen_split |= P > 1; seen_none |= P == 1
    assert seen_split and seen_none


def test_the_split_factor_follows_the_one_call_rule_on_the_calls_sets():
    """auto: no split above 4 096 sets or once 2 n reaches a round; a factor asked for is halved until 2 P n fits a round; a narrow region takes a smaller factor"""
    from milagro_bls_amd import _native as N
    R = N.default_limits().round_items
    P = lambda n, sm, stride=STRIDE_WORDS: N.plan_verify_multiple_batches_committee_span(n, max(1, n // 12), 0, 3, 0, 0, True, stride, sm)[1]
    assert P(4096, 0) > 1 and P(4097, 0) == 1 and P(R // 2, 0) == 1 and P(R // 2 - 1, 0) == 1
    assert P(12, 0) == 16 and P(12, 0, 64) == 8 and P(12, 0, 15) == 1 and P(12, 1) == 1
    assert P(R // 2, 16) == 1 and P(R // 2 - 1, 16) == 1 and P(R // 4, 16) == 2 and P(R // 32, 16) == 16
    for n in boundaries():
        for sm in SPLIT_MODES:
            assert 2 * P(n, sm) * n <= R or P(n, sm) == 1


def test_plan_argument_errors():
    from milagro_bls_amd import _native as N
    P = N.plan_verify_multiple_batches_committee_span
    assert P(10, 2, 5, 1, 0, 0, False, STRIDE_WORDS, 0)[1] >= 1
    for bad in ((0, 1, 0, 1, 0, 0), (1, 0, 0, 1, 0, 0), (10, 2, 4, 1, 0, 0), (10, 2, 5, 1, 0, 3)):       # mbls_plan_verify_multiple_batches_committee's
        with pytest.raises(N.MblsError):
            P(*bad, False, STRIDE_WORDS, 0)
    for sm in (3, 5, 32, -1):
        with pytest.raises(N.MblsError):
            P(10, 2, 5, 1, 0, 0, False, STRIDE_WORDS, sm)
    import ctypes as C
    L = N.default_limits(); vp = N.VmBatchesCommitteePlan(); sp = C.c_uint32(0)
    f = N.lib().mbls_plan_verify_multiple_batches_committee_span
    assert f(None, 10, 2, 5, 1, 0, 0, 0, 1, 0, C.byref(vp), C.byref(sp)) == N.ERR_ARGUMENT
    assert f(C.byref(L), 10, 2, 5, 1, 0, 0, 0, 1, 0, None, C.byref(sp)) == N.ERR_ARGUMENT
    assert f(C.byref(L), 10, 2, 5, 1, 0, 0, 0, 1, 0, C.byref(vp), None) == N.ERR_ARGUMENT
    assert f(C.byref(L), 10, 2, 5, 1, 0, 0, 0, 0, 0, C.byref(vp), C.byref(sp)) == N.OK and sp.value >= 1      # stride_words 0 reads as 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vbs") / "vbs_harness")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "vbs_emul", "mbls_vbs_harness.cpp")])
    return exe


def test_layout_sweep_under_the_sanitizers(harness):
    """the harness's own sweep of (n, B, bound, P, locate, route): the partial items and their status words overlap no region of the batches layout, and nothing is
    painted outside the plan's items (the end of the range is held to the library's figure by the next test)"""
    out = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[1]) >= 4000


def test_layout_ends_at_the_librarys_plan(harness):
    """the same painting at the points of the plan test, with the bound, the route and P the LIBRARY's plan function answers: the end of the partial sums' range is
    the library's workspace_items, and nothing overlaps"""
    from milagro_bls_amd import _native as N
    R = N.default_limits().round_items
    points, want = [], []
    for n in (1, 2, 3, 63, 64, 65, 200, 4096, 4097, R // 2 - 1):
        for B, spb in layouts(n):
            for mode in (1, 2):
                for locate in (False, True):
                    for sm in SPLIT_MODES:
                        plan, P = N.plan_verify_multiple_batches_committee_span(n, B, spb, 3, 0, mode, locate, STRIDE_WORDS, sm)
                        points.append("%d %d %d %d %d %d" % (n, B, plan["bound"], P, locate, mode == 1))
                        want.append((plan["workspace_items"], P, n))
    out = subprocess.run([harness, "stdin"], input="\n".join(points) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [[int(x) for x in l.split()] for l in out.stdout.splitlines()]
    assert len(rows) == len(points)
    for (first, end, plan, over_items, over_words, holes), (items, P, n), pt in zip(rows, want, points):
        assert end == plan == items, pt
        assert end - first == (2 * P * n if P > 1 else 0), pt
        assert over_items == 0 and over_words == 0 and holes == 0, pt


def test_symbols():
    """the library exports the new entries"""
    lib = os.path.join(ROOT, "milagro_bls_amd", "libmbls_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in NEW_ENTRIES:
        assert " T %s\n" % name in syms, name
