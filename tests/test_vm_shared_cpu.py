"""CPU checks of mbls_verify_multiple*_shared_msgs (include/mbls.h, "verify_multiple OVER A SHARED MESSAGE LIST"): the grouping arithmetic of
milagro_bls_amd/csrc/mbls_vms.h, built with the host compiler under AddressSanitizer and UBSan (tests/vms_emul/mbls_vms_harness.cpp, a stand-alone program)
and run over integers with `+`; the identity the grouped route rests on, on the Python model; and the new symbols and kernels as the library carries them."""
import os
import random
import subprocess

import pytest

import helpers

ROOT = helpers.ROOT
M64 = (1 << 64) - 1
NEW_ENTRIES = ("mbls_verify_multiple_shared_msgs_device", "mbls_verify_multiple_sets_indexed_shared_msgs_device", "mbls_verify_multiple_shared_msgs",
               "mbls_verify_multiple_shared_msgs_rng", "mbls_plan_verify_multiple_shared_msgs", "mbls_plan_verify_multiple_shared_msgs_workspace_items",
               "mbls_ctx_set_vm_grouping")
NEW_KERNELS = ("k_vms_count", "k_vms_scan", "k_vms_scatter", "k_g1_seg_tree_d", "k_vms_heads")


def val(j):
    """the harness's start value of set j"""
    z = ((j + 1) * 0x9E3779B97F4A7C15) & M64
    z ^= z >> 29
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 32
    return z


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vms") / "vms_harness")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "vms_emul", "mbls_vms_harness.cpp")])

    def run(cases):
        """cases: (n, n_msgs, order_seed, idx) -> per case ([(head, some)] per Miller item, levels, bad_sets, placed, wrong, outside)"""
        text = "".join("%d %d %d %s\n" % (n, M, seed, " ".join(map(str, idx))) for n, M, seed, idx in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-4000:]
        res = []
        for line in out.stdout.splitlines():
            body, tail = line.split("|")
            w = body.split()
            res.append(([(int(w[2 * i]), int(w[2 * i + 1])) for i in range(len(w) // 2)],) + tuple(int(x) for x in tail.split()))
        assert len(res) == len(cases)
        return res
    return run


def cases():
    """seeded index tables: bad indices, empty groups, one group holding everything, every set its own group, n not a power of two, lists longer than the scan
    has lanes; each in index order and in two seeded arrival orders"""
    rnd = random.Random(20270)
    out = []
    sizes = [1, 2, 3, 5, 7, 8, 9, 31, 33, 64, 65, 100, 127, 129, 150, 255, 257, 1000, 1023, 1025, 3001]
    for n in sizes:
        for M in (1, n, max(1, n // 2), n + 3, 7, 2):
            if M == n:
                idx = list(range(n)); rnd.shuffle(idx)                          # every set its own group
            elif M == 1:
                idx = [0] * n                                                    # one group holds everything
            else:
                idx = [rnd.randrange(M) for _ in range(n)]
            for seed in (0, 11 + n, 977 * n + M):
                out.append((n, M, seed, idx))
        # bad indices (>= n_msgs, 2^32 - 1), and an empty list
        idx = [rnd.choice([0, 1, 2, 3, 3, 4, 5, 0xFFFFFFFF, 9]) for _ in range(n)]
        out.append((n, 4, 5, idx))
        out.append((n, 0, 3, idx))
    out.append((5000, 2500, 1, [rnd.randrange(2500) for _ in range(5000)]))        # more messages than the scan has lanes: chunks of three
    out.append((10, 4097, 2, [4096, 0, 1024, 1023, 1025, 4096, 7, 7, 2048, 4097]))
    return out


def test_every_set_lands_once_and_group_sums_match_a_dict(harness):
    """every set with a good index lands in exactly one position of its message's range (whatever order the sets arrive in), no tree step reads outside a range,
    the head of every range holds the dict-based sum of its sets, a message nobody names is marked empty, sets with a bad index join no group, and the harness
    -- built with -fsanitize=address,undefined as a stand-alone program -- runs clean"""
    cs = cases()
    for (n, M, seed, idx), (heads, levels, bad, placed, wrong, outside) in zip(cs, harness(cs)):
        sums, count = {}, {}
        for i, j in enumerate(idx):
            if j < M:
                sums[j] = (sums.get(j, 0) + val(i)) & M64
                count[j] = count.get(j, 0) + 1
        assert bad == sum(1 for j in idx if j >= M), (n, M)
        assert placed == n - bad and wrong == 0 and outside == 0, (n, M, seed, placed, wrong, outside)
        assert levels == (0 if n <= 1 else (n - 1).bit_length())
        assert len(heads) == max(M, 1)
        for g, (head, some) in enumerate(heads):
            assert some == (1 if g in sums else 0), (n, M, g)
            assert head == sums.get(g, 0), (n, M, seed, g)


def test_new_symbols_and_kernels_are_in_the_library():
    from milagro_bls_amd import _native as N
    lib = N.lib()
    for name in NEW_ENTRIES:
        assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, "milagro_bls_amd", "libmbls_hip.so"), "rb") as f:
        blob = f.read()
    for k in NEW_KERNELS:
        assert k.encode() in blob, k
    assert b"mbls_g1_tree_d_asm_fn" in blob


# ------------------------------------------------------------------------------------------------ the identity itself, on the model
def test_grouped_product_equals_verify_multiple_on_the_model():
    """prod_i e([r_i] apk_i, H(m_i)) e(sum [r_i] sig_i, -G1) = prod_j e(sum_{i in j} [r_i] apk_i, H(m_j)) e(S, -G1) as bools, on oracle/pymodel: six sets over
    two messages -- an honest set, a key shifted by a point of order 3 (pk + T verifies what pk verifies), a pure-torsion set (infinity, T, m), and a pair
    (sig, pk, m) / (-sig, -pk, m) under one scalar, whose blinded keys cancel inside their group -- valid (True) and with one message tampered (False).
    Bilinearity in the key argument holds on all of E(Fp): the keys need not be in G1."""
    import bls12_381 as B
    import edge_points as E
    rnd = random.Random(88)
    m = [b"root-a" * 5, b"root-b" * 5]
    Hm = [B.hash_to_curve_g2(x) for x in m]
    tors = E.g1_torsion_points(rnd, orders=(3,), x0=True)
    T3, T0 = tors[0][1], tors[1][1]
    sk = [rnd.randrange(1, B.R) for _ in range(4)]
    pk = [B.g1_mul(B.G1, s) for s in sk]
    sig = lambda s, j: B.g2_mul(Hm[j], s)
    r_pair = 0x0807060504030201
    sets = [(sig(sk[0], 0), pk[0], 0, rnd.randrange(1, 1 << 63)),
            (sig(sk[1], 1), B.g1_add(pk[1], T3), 1, rnd.randrange(1, 1 << 63)),
            (None, T0, 0, 33),
            (sig(sk[2], 1), pk[2], 1, r_pair),
            (B.g2_neg(sig(sk[2], 1)), B.g1_neg(pk[2]), 1, r_pair),
            (sig(sk[3], 0), pk[3], 0, rnd.randrange(1, 1 << 63))]

    def grouped(sets, msgs_h):
        S, keys = None, {}
        for s, a, j, r in sets:
            S = B.g2_add(S, B.g2_mul(s, r))
            keys[j] = B.g1_add(keys.get(j), B.g1_mul(a, r))
        pairs = [(msgs_h[j], keys[j]) for j in sorted(keys)] + [(S, B.g1_neg(B.G1))]
        return B.pairing_product_is_one(pairs)
    # the cancelling pair sits in message 1 together with two other sets: the group sum is their two keys alone; alone in a group the sum would be infinity
    assert B.g1_add(B.g1_mul(sets[3][1], r_pair), B.g1_mul(sets[4][1], r_pair)) is None
    want = B.verify_multiple([(s, a, m[j]) for s, a, j, _r in sets], [r for *_x, r in sets])
    assert want is True and grouped(sets, Hm) is True
    bad_m = [m[0], b"root-c" * 5]
    bad = B.verify_multiple([(s, a, bad_m[j]) for s, a, j, _r in sets], [r for *_x, r in sets])
    assert bad is False and grouped(sets, [Hm[0], B.hash_to_curve_g2(bad_m[1])]) is False
