"""CPU checks of mbls_verify_multiple*_shared_msgs_locate* (include/mbls.h, "WHICH SETS OF A REJECTED SHARED-MESSAGE CALL"): the marking rule and the workspace
figure of milagro_bls_amd/csrc/mbls_vsl.h, built with the host compiler (tests/vsl_emul/mbls_vsl_harness.cpp, a stand-alone program, under AddressSanitizer and
UBSan: the rule indexes a table); the per-set check the grouped route has to recompute, on the Python model; and the new symbols and kernels as the cross-compiled
library carries them."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

import helpers

ROOT = helpers.ROOT
NEW_ENTRIES = ("mbls_verify_multiple_shared_msgs_locate_device", "mbls_verify_multiple_sets_indexed_shared_msgs_locate_device",
               "mbls_verify_multiple_shared_msgs_locate", "mbls_verify_multiple_shared_msgs_locate_rng")
PLAN = "mbls_plan_verify_multiple_shared_msgs_locate_workspace_items"
NEW_KERNELS = ("k_vsl_keep_key", "k_vsl_mark", "k_vsl_miller", "k_vsl_miller2")
# include/mbls.h MBLS_ST_* (tests/test_vm_locate_cpu.py checks the values against the header)
ST = {"BAD_SIG_ENCODING": 0x01, "SIG_NOT_IN_G2": 0x02, "BAD_PK_ENCODING": 0x04, "APK_INFINITY": 0x08, "NO_KEYS": 0x10, "PK_INFINITY": 0x20, "BAD_SCALAR": 0x80,
      "BAD_MSG_RANGE": 0x100}
REJECTING = ("BAD_SIG_ENCODING", "SIG_NOT_IN_G2", "BAD_PK_ENCODING", "BAD_MSG_RANGE", "BAD_SCALAR")
FALSE, TRUE, CANDIDATE = 0, 1, 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vsl") / "vsl_harness")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "vsl_emul", "mbls_vsl_harness.cpp")])

    def run(mode, rows):
        out = subprocess.run([exe, mode], input="".join(" ".join(map(str, r)) + "\n" for r in rows), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-4000:]
        got = [tuple(map(int, l.split())) for l in out.stdout.splitlines()]
        assert len(got) == len(rows)
        return got
    return run


def _want(ok, st, idx, M, mask):
    """the contract, spelled out: the word of the one-set call with the message spelled out, then accepted -> 1, a rejecting bit -> 0, else a candidate"""
    fault = idx >= M or bool((mask >> idx) & 1)
    word = st | (ST["BAD_MSG_RANGE"] if fault else 0)
    if ok:
        return TRUE, word
    if word & sum(ST[b] for b in REJECTING):
        return FALSE, word
    return CANDIDATE, word


def test_marking_rule_over_all_combinations(harness):
    """(call verdict) x (every subset of the status bits a set can carry) x (index in range naming a sound message, naming a flagged message, at n_msgs, far out
    of range, 2^32 - 1) x (lists of 0, 1 and 3 messages with every pattern of flagged messages): the verdict and the word against the contract. Entry 0 of the
    flags table -- the empty message's -- carries a bit in the harness, and no verdict may depend on it."""
    names = list(ST)
    rows, want = [], []
    for ok in (0, 1):
        for r in range(len(names) + 1):
            for sub in itertools.combinations(names, r):
                st = sum(ST[n] for n in sub)
                for M, masks in ((0, (0,)), (1, (0, 1)), (3, range(8))):
                    for mask in masks:
                        for idx in sorted({0, 1, 2, M, M + 1, 1000, 0xFFFFFFFF}):
                            rows.append((ok, st, idx, M, mask)); want.append(_want(ok, st, idx, M, mask))
    assert len(rows) == 2 * 2 ** len(names) * (5 + 2 * 5 + 8 * 7)
    assert harness("m", rows) == want
    # the rule in words
    assert harness("m", [(0, 0, 1, 3, 0b010)]) == [(FALSE, ST["BAD_MSG_RANGE"])]           # names the flagged message: the bit goes to the set's OWN word
    assert harness("m", [(0, 0, 0, 3, 0b010), (0, 0, 2, 3, 0b010)]) == [(CANDIDATE, 0)] * 2   # its neighbours do not
    assert harness("m", [(0, 0, 3, 3, 0), (0, 0, 0, 0, 0)]) == [(FALSE, ST["BAD_MSG_RANGE"])] * 2      # index >= n_msgs; the empty list
    assert harness("m", [(1, 0, 0, 3, 0)]) == [(TRUE, 0)]                                   # an accepted call is not examined
    for n in names:
        (v, st), = harness("m", [(0, ST[n], 0, 1, 0)])
        assert v == (FALSE if n in REJECTING else CANDIDATE) and st == ST[n], n
    # the Miller launch over the shadows: item t of A(0..n), B(0..n) answers for set t mod n
    for n in (1, 2, 5, 130):
        assert harness("s", [(t, n) for t in range(2 * n)]) == [(t % n,) for t in range(2 * n)]


def test_workspace_function_against_the_layout(harness):
    """mbls_plan_verify_multiple_shared_msgs_locate_workspace_items = phase one's workspace + one shadow item per set on the per-set route, two on the grouped
    one; the shadows start behind the sets [0, n), the Miller items [0, max(M, 1)), the positions [pbase, pbase + n) and the items of the list's own hash; the
    candidate flags fit the context's status words. At the boundaries of the routing and of the launch forms."""
    from milagro_bls_amd import _native as N
    L = N.default_limits()
    R = L.round_items
    half = R // 2
    cases = [(1, 0), (1, 1), (1, 5), (2, 1), (5, 3), (3, 7), (33, 4), (130, 5)]
    cases += [(n, M) for n in (half - 1, half, half + 1, R - 1, R, R + 1) for M in (0, 1, 512, n // 2, (n + 1) // 2, n, n + 1)]
    cases += [(10, 5), (11, 6), (9, 5), (1024, 512), (1025, 513)]                         # 2 M = n, 2 M = n + 1 under auto
    for n, M in cases:
        for mode in (0, 1, 2):
            vp = N.plan_verify_multiple_shared_msgs(n, M, mode, L)
            grouped = vp["route"] == N.VM_ROUTE_GROUPED
            assert grouped == (mode == 1 or (mode == 0 and 2 * M <= n)), (n, M, mode)
            (first, items, flags, per_set), = harness("w", [(n, M, int(grouped), vp["list_workspace_items"])])
            assert per_set == (2 if grouped else 1)
            assert first == vp["workspace_items"] == N.plan_verify_multiple_shared_msgs_workspace_items(n, M, mode, L)
            assert N.plan_verify_multiple_shared_msgs_locate_workspace_items(n, M, mode, L) == items == first + per_set * n, (n, M, mode)
            # nothing phase one touches reaches the first shadow
            assert first >= n and first >= vp["list_workspace_items"]
            if grouped:
                pbase = max(n, max(M, 1))
                assert vp["miller_items"] == max(M, 1) <= pbase and first >= pbase + n
            else:
                assert vp["miller_items"] == n
            assert flags == n and flags + n <= items                                    # one status word per workspace item: the flags [n, 2 n) fit
    # auto routing at the threshold: 2 M = n groups, 2 M = n + 1 does not
    assert N.plan_verify_multiple_shared_msgs_locate_workspace_items(10, 5, 0, L) == N.plan_verify_multiple_shared_msgs_workspace_items(10, 5, 0, L) + 20
    assert N.plan_verify_multiple_shared_msgs_locate_workspace_items(9, 5, 0, L) == N.plan_verify_multiple_shared_msgs_workspace_items(9, 5, 0, L) + 9
    # arguments the plan refuses
    f = N.plan_verify_multiple_shared_msgs_locate_workspace_items
    assert f(0, 5) == 0 and f(5, 5, 3) == 0 and f(5, 5, -1) == 0
    assert N.lib().mbls_plan_verify_multiple_shared_msgs_locate_workspace_items(None, 5, 5, 0) == 0
    assert f(5, 3) == f(5, 3, 0, L)


# ------------------------------------------------------------------------------------------------ the per-set check, on the model
def test_per_set_check_locates_the_tampered_set_on_the_model():
    """six sets over two messages, one of them tampered (another set's signature): the grouped check -- one pairing per message on the summed blinded keys --
    rejects, and FE(ML([r] apk, H(m)) . ML(-G1, [r] sig)) = 1 holds for exactly the five good sets. One good set's key is shifted by a point of order 3
    (tests/edge_points.py): pk + T verifies what pk verifies, alone as in the group. This is the check phase two of the grouped route runs per candidate; the
    group sums say nothing about a single set."""
    import bls12_381 as B
    import edge_points as E
    rnd = random.Random(89)
    m = [b"root-a" * 5, b"root-b" * 5]
    Hm = [B.hash_to_curve_g2(x) for x in m]
    T3 = E.g1_torsion_points(rnd, orders=(3,), x0=True)[0][1]
    sk = [rnd.randrange(1, B.R) for _ in range(6)]
    pk = [B.g1_mul(B.G1, s) for s in sk]
    idx = [0, 1, 1, 0, 1, 0]
    sig = [B.g2_mul(Hm[j], s) for s, j in zip(sk, idx)]
    pk[1] = B.g1_add(pk[1], T3)
    rands = [rnd.randrange(1, 1 << 63) for _ in range(6)]
    neg_g1 = B.g1_neg(B.G1)

    def grouped(sigs):
        S, keys = None, {}
        for s, a, j, r in zip(sigs, pk, idx, rands):
            S = B.g2_add(S, B.g2_mul(s, r))
            keys[j] = B.g1_add(keys.get(j), B.g1_mul(a, r))
        return B.pairing_product_is_one([(Hm[j], keys[j]) for j in sorted(keys)] + [(S, neg_g1)])

    def alone(s, a, j, r):
        return B.pairing_product_is_one([(Hm[j], B.g1_mul(a, r)), (B.g2_mul(s, r), neg_g1)])
    assert grouped(sig) is True
    bad = list(sig)
    bad[4] = sig[2]                                   # a sound signature of the same message under another key
    assert grouped(bad) is False
    got = [alone(s, a, j, r) for s, a, j, r in zip(bad, pk, idx, rands)]
    assert got == [True, True, True, True, False, True]
    assert got == [B.verify_multiple([(s, a, m[j])], [r]) for s, a, j, r in zip(bad, pk, idx, rands)]


# ------------------------------------------------------------------------------------------------ the ABI and the kernels, as built
@pytest.fixture(scope="module")
def lib_path():
    from milagro_bls_amd import build
    return build.build()


def test_new_entries_are_declared_exported_and_mirrored(lib_path):
    import test_build_cpu as T
    from milagro_bls_amd import _native
    declared = T.declared_symbols()
    l = ctypes.CDLL(lib_path)
    protos = T._c_prototypes()
    rust = T._rust_decls(os.path.join(ROOT, "rust", "src", "lib.rs"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_ENTRIES + (PLAN,):
        assert name in declared, name
        assert hasattr(l, name), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == len(protos[name]), name
        assert name in integ, name
    for name in NEW_ENTRIES:
        assert name in rust and all(len(v) == len(protos[name]) for v in rust[name]), name
    # the locate entries take the shared-message entries' parameters, then the two per-set outputs in front of the stream / the scalar source
    for a, b in (("mbls_verify_multiple_shared_msgs_device", "mbls_verify_multiple_shared_msgs_locate_device"),
                 ("mbls_verify_multiple_sets_indexed_shared_msgs_device", "mbls_verify_multiple_sets_indexed_shared_msgs_locate_device")):
        assert protos[b] == protos[a][:-1] + [("mut", "u8", 1), ("mut", "u32", 1)] + protos[a][-1:]
    assert protos["mbls_verify_multiple_shared_msgs_locate"] == protos["mbls_verify_multiple_shared_msgs"] + [("mut", "u8", 1), ("mut", "u32", 1)]
    assert protos["mbls_verify_multiple_shared_msgs_locate_rng"] == protos["mbls_verify_multiple_shared_msgs_rng"][:-2] + [("mut", "u8", 1), ("mut", "u32", 1)] + \
        protos["mbls_verify_multiple_shared_msgs_rng"][-2:]
    assert protos[PLAN] == protos["mbls_plan_verify_multiple_shared_msgs_workspace_items"]
    from milagro_bls_amd import api, batch
    assert hasattr(api.AggregateSignature, "verify_multiple_aggregate_signatures_shared_msgs_locate")
    assert all(hasattr(batch, f) for f in ("verify_multiple_shared_msgs_locate", "verify_multiple_shared_msgs_locate_rng", "verify_multiple_shared_msgs_locate_device",
                                           "verify_multiple_sets_indexed_shared_msgs_locate_device"))
    hpp = open(os.path.join(ROOT, "include", "milagro_bls.hpp")).read()
    assert "verify_multiple_aggregate_signatures_shared_msgs_locate" in hpp and "mbls_verify_multiple_shared_msgs_locate_rng" in hpp
    rs = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    assert "pub fn verify_multiple_aggregate_signatures_shared_msgs_locate" in rs
    hdr = open(os.path.join(ROOT, "include", "mbls.h")).read()
    assert "locate forms of the shared-message entries" not in hdr


def test_new_kernels_have_no_private_memory_and_no_spills(lib_path):
    import test_build_cpu as T
    meta = T.kernel_metadata(lib_path)
    for k in NEW_KERNELS:
        prefix = "_Z%d%s" % (len(k), k)
        recs = [v for name, v in meta.items() if name.startswith(prefix)]
        assert len(recs) == 1, (k, [n for n in meta if k in n])
        assert int(recs[0]["private_segment_fixed_size"]) == 0 and int(recs[0]["vgpr_spill_count"]) == 0, (k, recs[0])
    # the Miller kernels are one-wave-per-SIMD kernels like k_miller_single, and their LDS fits four waves per CU
    for k in ("k_vsl_miller", "k_vsl_miller2"):
        v = next(v for name, v in meta.items() if name.startswith("_Z%d%s" % (len(k), k)))
        assert int(v["vgpr_count"]) > 256 and int(v["group_segment_fixed_size"]) * 4 <= 160 * 1024, k


def test_locate_mode_adds_to_the_sequence_and_changes_none_of_it():
    """verify_multiple_impl enqueues the keeps, the mark and phase two only in locate mode: every launch of a k_vsl_* / k_vml_* kernel there stands behind
    `if (loc` or inside the locate block behind the tail; without locate the call reserves the workspace it reserved before"""
    src = open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_kernels.hip")).read()
    body = src.split("static int verify_multiple_impl(", 1)[1].split("\nextern \"C\"", 1)[0]
    for line in body.splitlines():
        if "hipLaunchKernelGGL(k_vsl_keep" in line or "hipLaunchKernelGGL(k_vml_keep" in line:
            assert line.strip().startswith("if (loc)"), line
    head, tail = body.split("if (loc && grouped) {", 1)
    assert "k_vsl_mark" not in head and "vsl_examine" not in head and "k_vml_mark" not in head
    assert "k_vsl_mark" in tail and "k_vml_mark" in tail and tail.count("vsl_examine(") == 2
    assert "loc && !grouped ? shf : 0" in body                                            # the Miller values are kept on the per-set route only, in locate mode only
    assert "d.locate ? vsl_workspace_items(" in src and ": sh.vp.workspace_items)" in src
