"""CPU checks of mbls_verify_multiple_batches* (include/mbls.h, "MANY verify_multiple BATCHES IN ONE CALL"): the segment arithmetic of
milagro_bls_amd/csrc/mbls_vmb.h, built with the host compiler (tests/vmb_emul/mbls_vmb_harness.cpp) and run over integers with `+` as the operation, and the
new symbols and kernels as the cross-compiled library carries them."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import helpers

ROOT = helpers.ROOT
NEW_ENTRIES = ("mbls_verify_multiple_batches_device", "mbls_verify_multiple_batches_indexed_device", "mbls_verify_multiple_batches",
               "mbls_verify_multiple_batches_rng")
NEW_KERNELS = ("k_vmb_set_map", "k_g2_seg_tree_d", "k_vmb_sigpair_setup", "k_vmb_status_fold", "k_vmb_gather", "k_vmb_final", "k_vmb_final2")
M64 = (1 << 64) - 1


def val(j):
    """the harness's start value of set j"""
    z = ((j + 1) * 0x9E3779B97F4A7C15) & M64
    z ^= z >> 29
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 32
    return z


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vmb") / "vmb_harness")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "vmb_emul", "mbls_vmb_harness.cpp")])

    def run(tables):
        """tables: (B, n, k, order, offsets or None) -> per table (list of (head, rejected, crossed) per batch, levels)"""
        text = "".join("%d %d %d %d %s\n" % (B, n, k, order, " ".join(map(str, off)) if off is not None else "") for B, n, k, order, off in tables)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        res = []
        for line in out.stdout.splitlines():
            body, lv = line.split("|")
            w = body.split()
            res.append(([(int(w[3 * i]), int(w[3 * i + 1]), int(w[3 * i + 2])) for i in range(len(w) // 3)], int(lv)))
        assert len(res) == len(tables)
        return res
    run.exe = exe
    return run


def sound_tables(rnd, count):
    """seeded offset tables: empty batches, batches of 1, 2, 3, 2^k +- 1, one batch holding everything, mixtures"""
    special = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1000]
    out = []
    for t in range(count):
        kind = t % 5
        if kind == 0:
            sizes = [rnd.choice(special) for _ in range(rnd.randrange(1, 40))]
        elif kind == 1:
            sizes = [rnd.choice([0, 0, 1, 1, 2, 3]) for _ in range(rnd.randrange(1, 200))]
        elif kind == 2:
            sizes = [0] * rnd.randrange(0, 4) + [rnd.choice(special[3:]) + rnd.randrange(0, 300)] + [0] * rnd.randrange(0, 4)      # one batch holds everything
        elif kind == 3:
            sizes = [rnd.randrange(0, 70) for _ in range(rnd.randrange(1, 64))]
        else:
            sizes = [rnd.choice([(1 << e) + d for e in range(1, 10) for d in (-1, 0, 1)]) for _ in range(rnd.randrange(1, 12))]
        off = [0]
        for s in sizes:
            off.append(off[-1] + s)
        out.append((len(sizes), off[-1], 0, t & 1, off))
    return out


def test_every_batch_sums_exactly_its_own_sets(harness):
    """after the levels the head of every range holds the sum of exactly its own elements, each taken once, and no step read across a boundary"""
    rnd = random.Random(20261)
    tables = sound_tables(rnd, 300)
    tables += [(B, B * k, k, 0, None) for k in (1, 2, 3, 4, 5, 10, 31, 32, 33, 63, 64, 65, 1000) for B in (1, 2, 7, 64)]          # uniform sets_per_batch
    tables += [(5, 0, 0, 0, [0] * 6), (1, 0, 0, 0, [0, 0]), (1, 4097, 0, 0, [0, 4097])]
    res = harness(tables)
    for (B, n, k, _order, off), (batches, levels) in zip(tables, res):
        assert len(batches) == B
        longest = n if off is not None else k
        assert levels == (0 if longest <= 1 else (longest - 1).bit_length())
        for b, (head, rej, crossed) in enumerate(batches):
            lo, hi = (off[b], off[b + 1]) if off is not None else (k * b, k * b + k)
            assert rej == 0 and crossed == 0, (B, n, k, b)
            assert head == sum(val(j) for j in range(lo, hi)) & M64, (B, n, k, b, lo, hi)


def test_a_faulty_table_rejects_every_batch_that_shares_or_loses_a_set(harness):
    """device-side tables are not seen by the host: a range that runs backwards or ends beyond n is never read and rejects its batch; every batch that shares a
    set with another is rejected, whichever claim arrives first; a batch whose sound range is its own alone is summed as if the table were sound"""
    rnd = random.Random(20262)
    tables = []
    for t in range(300):
        base = sound_tables(rnd, 1)[0]
        B, n, _, _, off = base
        off = list(off)
        for _ in range(rnd.randrange(1, 4)):
            i = rnd.randrange(0, B + 1)
            kind = rnd.randrange(4)
            if kind == 0:
                off[i] = rnd.randrange(0, n + 1)                       # anywhere: backwards here, overlapping there
            elif kind == 1:
                off[i] = n + rnd.randrange(1, 1000)                    # beyond the sets
            elif kind == 2:
                off[i] = max(0, off[i] - rnd.randrange(1, 40))         # a little back: the neighbours overlap
            else:
                off[i] = 0xFFFFFFFF
        tables.append((B, n, 0, t & 1, off))
    # does not start at 0 / ends below n: the sets nobody owns are simply not part of the call
    tables += [(3, 30, 0, 0, [5, 10, 20, 30]), (3, 30, 0, 1, [0, 10, 20, 25]), (2, 10, 0, 0, [0, 12, 10]), (2, 10, 0, 1, [0, 8, 4])]
    res = harness(tables)
    seen_rej = seen_ok = 0
    for (B, n, _k, _order, off), (batches, _lv) in zip(tables, res):
        rng = [(off[b], off[b + 1]) for b in range(B)]
        sound = [lo <= hi <= n for lo, hi in rng]
        claims = [0] * n
        for b in range(B):
            if sound[b]:
                for j in range(*rng[b]):
                    claims[j] += 1
        for b, (head, rej, crossed) in enumerate(batches):
            lo, hi = rng[b]
            must = (not sound[b]) or any(claims[j] > 1 for j in range(lo, hi))
            assert bool(rej) == must, (off, b)
            if not rej:
                assert crossed == 0 and head == sum(val(j) for j in range(lo, hi)) & M64, (off, b)
                seen_ok += 1
            else:
                seen_rej += 1
    assert seen_rej > 200 and seen_ok > 200


def test_host_table_validation(harness):
    """vmb_offsets_ok is what the host entries run before anything is enqueued: first 0, non-decreasing, last n_sets; it also finds the longest range, which
    sets the number of tree levels (the GPU tests exercise the refusals through the C ABI)"""
    cases = [([0, 2, 6], 6, True, 4), ([0, 0, 0], 0, True, 0), ([0, 6], 6, True, 6), ([0, 3, 3, 6], 6, True, 3), ([0, 4, 2, 6], 6, False, 0),
             ([1, 2, 6], 6, False, 0), ([0, 2, 5], 6, False, 0), ([0, 2, 7], 6, False, 0), ([0, 7, 6], 6, False, 0), ([0, 1, 2, 3, 70], 70, True, 67)]
    text = "".join("%d %d %s\n" % (len(off) - 1, n, " ".join(map(str, off))) for off, n, _, _ in cases)
    out = subprocess.run([harness.exe, "v"], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = [tuple(map(int, l.split())) for l in out.stdout.splitlines()]
    assert got == [(int(ok), longest) for _, _, ok, longest in cases]
    src = open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_kernels.hip")).read()
    assert src.count("vmb_host_check(c,") == 2 and "vmb_offsets_ok(boff, B, n, longest)" in src          # both host entries go through it


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
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(l, name), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == len(protos[name]), name
        assert name in rust and all(len(v) == len(protos[name]) for v in rust[name]), name
        assert name in integ, name
    # the mirrors
    from milagro_bls_amd import api, batch
    assert hasattr(api.AggregateSignature, "verify_multiple_aggregate_signatures_batches")
    assert hasattr(batch, "verify_multiple_batches") and hasattr(batch, "verify_multiple_batches_device")
    hpp = open(os.path.join(ROOT, "include", "milagro_bls.hpp")).read()
    assert "verify_multiple_aggregate_signatures_batches" in hpp and "mbls_verify_multiple_batches_rng" in hpp


def test_new_kernels_have_no_private_memory_and_no_spills(lib_path):
    import test_build_cpu as T
    meta = T.kernel_metadata(lib_path)
    for k in NEW_KERNELS:
        prefix = "_Z%d%s" % (len(k), k)
        recs = [v for name, v in meta.items() if name.startswith(prefix)]
        assert len(recs) == 1, (k, [n for n in meta if k in n])
        assert int(recs[0]["private_segment_fixed_size"]) == 0 and int(recs[0]["vgpr_spill_count"]) == 0, (k, recs[0])
    # the tail kernels are one-wave-per-SIMD kernels like their twins, and their LDS fits four waves per CU
    for k in ("k_vmb_final", "k_vmb_final2", "k_g2_seg_tree_d"):
        v = next(v for name, v in meta.items() if name.startswith("_Z%d%s" % (len(k), k)))
        assert int(v["group_segment_fixed_size"]) * 4 <= 160 * 1024, k


def test_batch_tail_uses_the_batch_mask():
    """lane_final rejects on the per-item mask (infinite key, no keys; not a zero scalar); a verify_multiple batch rejects on mbls_coop.h's COOP_REJECT_BATCH.
    final_fold_batch must name exactly the bits of COOP_REJECT_BATCH."""
    coop = open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_coop.h")).read()
    lanes = open(os.path.join(ROOT, "milagro_bls_amd", "csrc", "mbls_lanes.h")).read()
    want = set(re.findall(r"MBLS_ST_[A-Z0-9_]+", re.search(r"#define COOP_REJECT_BATCH \(([^)]*)\)", coop).group(1)))
    body = lanes.split("MBLS_FN void final_fold_batch", 1)[1].split("\n}\n", 1)[0]
    got = set(re.findall(r"MBLS_ST_[A-Z0-9_]+", body.split("const uint32_t reject =", 1)[1].split(";", 1)[0]))
    assert got == want and "MBLS_ST_BAD_SCALAR" in got and "MBLS_ST_APK_INFINITY" not in got and "MBLS_ST_NO_KEYS" not in got
