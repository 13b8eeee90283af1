"""CPU checks of mbls_verify_multiple_batches_locate* (include/mbls.h, "WHICH SETS OF A REJECTED BATCH"): the marking rule and the workspace figure of
milagro_bls_amd/csrc/mbls_vml.h, built with the host compiler (tests/vml_emul/mbls_vml_harness.cpp), and the new symbols and kernels as the cross-compiled
library carries them."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest

import helpers

ROOT = helpers.ROOT
NEW_ENTRIES = ("mbls_verify_multiple_batches_locate_device", "mbls_verify_multiple_batches_locate_indexed_device", "mbls_verify_multiple_batches_locate",
               "mbls_verify_multiple_batches_locate_rng")
NEW_KERNELS = ("k_vml_keep_sig", "k_vml_keep_f", "k_vml_mark", "k_vml_miller", "k_vml_miller2", "k_vml_product", "k_vml_final", "k_vml_final2")
# include/mbls.h MBLS_ST_*
ST = {"BAD_SIG_ENCODING": 0x01, "SIG_NOT_IN_G2": 0x02, "BAD_PK_ENCODING": 0x04, "APK_INFINITY": 0x08, "NO_KEYS": 0x10, "PK_INFINITY": 0x20, "PAIRING_FAILED": 0x40,
      "BAD_SCALAR": 0x80, "BAD_MSG_RANGE": 0x100}
REJECTING = ("BAD_SIG_ENCODING", "SIG_NOT_IN_G2", "BAD_PK_ENCODING", "BAD_MSG_RANGE", "BAD_SCALAR")
FALSE, TRUE, CANDIDATE = 0, 1, 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vml") / "vml_harness")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "vml_emul", "mbls_vml_harness.cpp")])

    def run(mode, rows):
        out = subprocess.run([exe, mode], input="".join("%d %d %d\n" % tuple(r) for r in rows), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        got = [tuple(map(int, l.split())) for l in out.stdout.splitlines()]
        assert len(got) == len(rows)
        return got
    return run


def test_status_bits_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "mbls.h")).read()
    for name, v in ST.items():
        m = re.search(r"#define\s+MBLS_ST_%s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, hdr)
        assert m and int(m.group(1), 0) == v, name
    # the rule's mask is verify_multiple's: the bits of mbls_coop.h's COOP_REJECT_BATCH
    coop = open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_coop.h")).read()
    want = set(re.findall(r"MBLS_ST_([A-Z0-9_]+)", re.search(r"#define COOP_REJECT_BATCH \(([^)]*)\)", coop).group(1)))
    assert want == set(REJECTING)
    vml = open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_vml.h")).read()
    mask = re.search(r"#define MBLS_VML_REJECT \((.*)\)\s*$", vml, flags=re.M).group(1)
    assert sum(int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", mask)) == sum(ST[b] for b in REJECTING)
    assert sorted(re.findall(r"/\* ([A-Z0-9_]+) \*/", mask)) == sorted(REJECTING)


def test_marking_rule_over_all_combinations(harness):
    """(batch verdict, owned, every subset of the status bits a set can carry): no owner -> 0 with the table-fault bit, whatever else; an accepted batch -> 1
    without a look at the set; a rejecting bit -> 0; everything else is a candidate. The word reported is the set's own, plus the fault bit without an owner."""
    names = [n for n in ST if n != "PAIRING_FAILED"]           # (phase one never sets it on a set)
    rows, want = [], []
    for owned, ok in itertools.product((0, 1), (0, 1)):
        for r in range(len(names) + 1):
            for sub in itertools.combinations(names, r):
                st = sum(ST[n] for n in sub)
                rows.append((owned, ok, st))
                if not owned:
                    want.append((FALSE, st | ST["BAD_PK_ENCODING"]))
                elif ok:
                    want.append((TRUE, st))
                elif any(n in REJECTING for n in sub):
                    want.append((FALSE, st))
                else:
                    want.append((CANDIDATE, st))
    assert len(rows) == 4 * 2 ** len(names)
    assert harness("m", rows) == want
    # each rejecting bit alone rejects; each other bit alone does not (an infinite key, an empty key list: the reference multiplies them in like any other)
    for n in names:
        (v, st), = harness("m", [(1, 0, ST[n])])
        assert v == (FALSE if n in REJECTING else CANDIDATE) and st == ST[n], n


def test_workspace_figure(harness):
    """2 n + 2 B items -- 3 n where the lane-pair message phase's 2 n items are more than n + 2 B: the shadows lie behind everything phase one works on, the
    candidate flags fit the context's status words (one per item); mbls_plan_locate_workspace_items is that figure under the limits' choice of message phase"""
    from milagro_bls_amd import _native as N
    L = N.default_limits()
    R = L.round_items
    half = R // 2
    ns = [1, 2, 3, 64, 65, half // 2 - 1, half // 2, half // 2 + 1, half - 1, half, half + 1, R - 1, R, R + 1]
    rows = [(n, B, ph) for n in ns for B in sorted({1, n}) for ph in (0, 1)]
    got = harness("w", rows)
    for (n, B, ph), (first, items, flags) in zip(rows, got):
        phase_one = max(n + 2 * B, 2 * n if ph else n)
        assert first == phase_one and items == phase_one + n and flags == n + 2 * B
        assert items >= 2 * n + 2 * B and flags + n <= items
        assert items == (2 * n + 2 * B if not ph or n <= 2 * B else 3 * n)
    for n in ns:
        for B in sorted({1, n}):
            ph = n <= L.split_max_items and 2 * n <= R
            want = harness("w", [(n, B, int(ph))])[0][1]
            assert N.plan_locate_workspace_items(n, B, L) == want, (n, B)
            assert N.plan_locate_workspace_items(n, B) == want
    assert N.plan_locate_workspace_items(0, 5) == 10 and N.plan_locate_workspace_items(0, 0) == 0
    assert N.plan_locate_workspace_items(half, 1, L) == 3 * half and N.plan_locate_workspace_items(half + 1, 1, L) == 2 * (half + 1) + 2


# ---- the ABI and the kernels, as built
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
    for name in NEW_ENTRIES + ("mbls_plan_locate_workspace_items",):
        assert name in declared, name
        assert hasattr(l, name), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == len(protos[name]), name
        assert name in integ, name
    for name in NEW_ENTRIES:
        assert name in rust and all(len(v) == len(protos[name]) for v in rust[name]), name
    # the locate entries take the batches entries' parameters, then the two per-set outputs in front of the stream / the scalar source
    for a, b in (("mbls_verify_multiple_batches_device", "mbls_verify_multiple_batches_locate_device"),
                 ("mbls_verify_multiple_batches_indexed_device", "mbls_verify_multiple_batches_locate_indexed_device")):
        assert protos[b] == protos[a][:-1] + [("mut", "u8", 1), ("mut", "u32", 1)] + protos[a][-1:]
    assert protos["mbls_verify_multiple_batches_locate"] == protos["mbls_verify_multiple_batches"] + [("mut", "u8", 1), ("mut", "u32", 1)]
    assert protos["mbls_verify_multiple_batches_locate_rng"] == protos["mbls_verify_multiple_batches_rng"][:-2] + [("mut", "u8", 1), ("mut", "u32", 1)] + \
        protos["mbls_verify_multiple_batches_rng"][-2:]
    from milagro_bls_amd import api, batch
    assert hasattr(api.AggregateSignature, "verify_multiple_aggregate_signatures_batches_locate")
    assert all(hasattr(batch, f) for f in ("verify_multiple_batches_locate", "verify_multiple_batches_locate_device", "verify_multiple_batches_locate_indexed_device"))
    hpp = open(os.path.join(ROOT, "include", "milagro_bls.hpp")).read()
    assert "verify_multiple_aggregate_signatures_batches_locate" in hpp and "mbls_verify_multiple_batches_locate_rng" in hpp
    rs = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    assert "pub fn verify_multiple_aggregate_signatures_batches_locate" in rs


def test_new_kernels_have_no_private_memory_and_no_spills(lib_path):
    import test_build_cpu as T
    meta = T.kernel_metadata(lib_path)
    for k in NEW_KERNELS:
        prefix = "_Z%d%s" % (len(k), k)
        recs = [v for name, v in meta.items() if name.startswith(prefix)]
        assert len(recs) == 1, (k, [n for n in meta if k in n])
        assert int(recs[0]["private_segment_fixed_size"]) == 0 and int(recs[0]["vgpr_spill_count"]) == 0, (k, recs[0])
    # phase two's heavy kernels are one-wave-per-SIMD kernels like their twins, and their LDS fits four waves per CU
    for k in ("k_vml_miller", "k_vml_miller2", "k_vml_product", "k_vml_final", "k_vml_final2"):
        v = next(v for name, v in meta.items() if name.startswith("_Z%d%s" % (len(k), k)))
        assert int(v["vgpr_count"]) > 256 and int(v["group_segment_fixed_size"]) * 4 <= 160 * 1024, k


def test_locate_mode_adds_to_the_sequence_and_changes_none_of_it():
    """vmb_impl enqueues phase two and the two keeps only in locate mode: every launch of a k_vml_* kernel stands behind `if (loc` or inside the locate block"""
    src = open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_kernels.hip")).read()
    body = src.split("static int vmb_impl(", 1)[1].split("\nextern \"C\"", 1)[0]
    for line in body.splitlines():
        if "hipLaunchKernelGGL(k_vml_keep" in line:
            assert line.strip().startswith("if (loc)"), line
    tail = body.split("if (loc && n) {\n        hipLaunchKernelGGL(k_vml_mark", 1)
    assert len(tail) == 2 and "k_vml_" not in tail[0].replace("k_vml_keep", "")
    assert all(k in body for k in NEW_KERNELS)
