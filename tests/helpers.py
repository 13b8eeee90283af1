"""Shared test helpers: golden vectors, the host emulator of the lane bodies, synthetic batches (built with the
oracle, which is the checker here -- never the thing under test)."""
import ctypes as C
import json
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vectors.json")
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
G2_INF = bytes([0xC0]) + bytes(95)


def load_vectors():
    with open(GOLDEN) as f:
        return json.load(f)


def expand_msg(h):
    return bytes([42]) * 133700 if h == "2a*133700" else bytes.fromhex(h)


def load_emulator():
    """Build (amdclang++, plain C++) and load tests/host_emul/libmbls_emul.so."""
    d = os.path.join(ROOT, "tests", "host_emul")
    so = os.path.join(d, "libmbls_emul.so")
    src = [os.path.join(d, "mbls_emul.cpp")] + [os.path.join(ROOT, "milagro_bls_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "milagro_bls_amd", "csrc")) if f.endswith((".h", ".inc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src[0]])
    return C.CDLL(so)


def cb(x):
    x = bytes(x)
    return (C.c_uint8 * max(1, len(x))).from_buffer_copy(x if x else b"\0")


def ob(n):
    return (C.c_uint8 * max(1, n))()


class Batch:
    pass


NOT_IN_G2 = None


def make_batch(n, k, fmt=0, seed=1, pool_n=64, negatives=True, nthreads=8):
    """Synthetic fast_aggregate_verify batch in wire format + the expectation by construction.
    Negative kinds cycle over items with i % 4 == 3."""
    import orc
    rnd = random.Random(seed)
    pool = [rnd.randrange(1, R) for _ in range(pool_n)]
    sz = 48 if fmt == 0 else 96
    pkb = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for s in pool), pool_n, fmt, nthreads=nthreads)
    pk = [pkb[sz * j:sz * j + sz] for j in range(pool_n)]
    msgs = [rnd.randbytes(32) for _ in range(n)]
    idxs = [rnd.sample(range(pool_n), k) for _ in range(n)]
    aggs = [sum(pool[j] for j in idx) % R for idx in idxs]
    sigs = orc.batch_sign(b"".join(a.to_bytes(32, "big") for a in aggs), b"".join(msgs), n, nthreads=nthreads)
    sigs = [sigs[96 * i:96 * i + 96] for i in range(n)]
    keys = [[pk[j] for j in idx] for idx in idxs]
    expect = [True] * n
    kinds = ["valid"] * n
    if negatives:
        order = ["flip_msg", "wrong_key", "sig_not_in_g2", "sig_infinity", "apk_infinity", "bad_sig_bytes", "bad_pk_bytes"]
        c = 0
        for i in range(n):
            if i % 4 != 3:
                continue
            kind = order[c % len(order)]; c += 1
            if kind == "apk_infinity" and k < 2:
                kind = "flip_msg"
            kinds[i] = kind; expect[i] = False
            if kind == "flip_msg":
                msgs[i] = bytes([msgs[i][0] ^ 1]) + msgs[i][1:]
            elif kind == "wrong_key":
                other = [j for j in range(pool_n) if j not in idxs[i]][0]
                keys[i][0] = pk[other]
            elif kind == "sig_not_in_g2":
                sigs[i] = bytes.fromhex(load_vectors()["model"]["g2_subgroup_probes"][c % 3]["compressed"])
            elif kind == "sig_infinity":
                sigs[i] = G2_INF
            elif kind == "apk_infinity":
                e, partial = orc.aggregate_pks([orc.sk_to_pk(pool[j]) for j in idxs[i][:-1]])
                neg = orc.g1_mul(partial, R - 1)
                keys[i][-1] = orc.g1_compress(neg) if fmt == 0 else neg
            elif kind == "bad_sig_bytes":
                sigs[i] = bytes([sigs[i][0] & 0x7F]) + sigs[i][1:]      # compression flag cleared
            elif kind == "bad_pk_bytes":
                keys[i][0] = bytes([0x80 if fmt == 0 else 0x00]) + b"\xff" * (sz - 1)   # x >= p
    b = Batch()
    b.n, b.k, b.fmt = n, k, fmt
    b.sigs = b"".join(sigs); b.msgs = b"".join(msgs); b.pks = b"".join(b"".join(ks) for ks in keys)
    b.expect = expect; b.kinds = kinds
    return b


# ------------------------------------------------------------------------------------------------ full-scale sampling and checking
WG = 64                         # a workgroup of the verify kernels is one wave
ROUND_ITEMS = 65536             # items of one round of the batch engines


def oracle_threads():
    """Threads for the oracle's batch entries: at most 16 (what one command may use on a GPU machine), OMP_NUM_THREADS when set, the CPUs."""
    n = min(16, os.cpu_count() or 1)
    try:
        n = min(n, int(os.environ.get("OMP_NUM_THREADS", "")))
    except ValueError:
        pass
    return max(1, n)


def rejection_class(i):
    """bench.build_inputs corrupts item i with i % 16 == 7, in class (i // 16) % 5; None for an item it leaves intact"""
    return (i // 16) % 5 if i % 16 == 7 else None


def sample_indices(n, seed, count=1024, rounds=ROUND_ITEMS, per_class=8):
    """Sorted, de-duplicated, seeded sample of [0, n): `count` uniform indices, the wave edges 0 / 63 / 64, every round seam q*rounds - 1 / q*rounds /
    q*rounds + 1, the last 64 items and at least `per_class` items of each of bench.build_inputs' five rejection classes (as far as [0, n) holds them)."""
    rnd = random.Random(seed)
    s = set(rnd.sample(range(n), min(count, n)))
    s.update((0, WG - 1, WG))
    for q in range(1, n // rounds + 1):
        s.update((q * rounds - 1, q * rounds, q * rounds + 1))
    s.update(range(max(0, n - 64), n))
    nbad = len(range(7, n, 16))                         # bad item j is 7 + 16 j, of class j % 5
    for c in range(5):
        js = range(c, nbad, 5)
        s.update(7 + 16 * j for j in rnd.sample(js, min(per_class, len(js))))
    return sorted(i for i in s if 0 <= i < n)


def bitmap_bits(d_bm, n):
    """The accept bitmap (int64 words, device or host tensor) as n bits: bit i % 64 of word i // 64 is item i"""
    import numpy as np
    words = d_bm.cpu().numpy().view(np.uint64)
    return ((words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).reshape(-1)[:n].astype(np.uint8)


def _gather(t, idx):
    import torch
    return t[torch.as_tensor(idx, dtype=torch.long, device=t.device)].cpu().numpy().tobytes()


def _flags(x, idx):
    import numpy as np
    return [bool(v) for v in np.asarray(x.cpu() if hasattr(x, "cpu") else x)[np.asarray(idx)].tolist()]


def oracle_check_fav(d_sigs, d_msgs, d_pks, idx, k, fmt, expect, got):
    """fast_aggregate_verify of the items `idx` (device tensors [n, 96], [n, 32], [n, k, 48|96]) on the oracle: its verdicts equal both the device's
    results `got` and the expectation `expect` at those indices"""
    import orc
    want = orc.batch_fast_aggregate_verify(_gather(d_sigs, idx), _gather(d_msgs, idx), _gather(d_pks, idx), len(idx), k, fmt, nthreads=oracle_threads())
    dev, exp = _flags(got, idx), _flags(expect, idx)
    assert want == exp, [i for i, a, b in zip(idx, want, exp) if a != b][:8]
    assert want == dev, [i for i, a, b in zip(idx, want, dev) if a != b][:8]


def oracle_check_verify(d_sigs, d_msgs, d_pks, idx, expect, got):
    """Signature::verify of the items `idx` (device tensors [n, 96], [n, 32], [n, 48]) on the oracle, against `got` and `expect` at those indices"""
    import orc
    want = orc.batch_verify(_gather(d_sigs, idx), _gather(d_msgs, idx), _gather(d_pks, idx), len(idx), nthreads=oracle_threads())
    dev, exp = _flags(got, idx), _flags(expect, idx)
    assert want == exp, [i for i, a, b in zip(idx, want, exp) if a != b][:8]
    assert want == dev, [i for i, a, b in zip(idx, want, dev) if a != b][:8]


BUILD_INPUTS_FLAG = (0x40, 0x40, 0x02, 0x40, 0x08)     # bench.build_inputs' classes: msg bit, wrong key, sig not in G2, infinity sig (pairing fails), apk = infinity


def check_status_classes(st, expect, period=None):
    """Status words of a bench.build_inputs batch (numpy int32 [n], expectation [n]; period: the size of the batch that was repeated to make it): every
    rejected item carries its class's MBLS_ST_* bit and nothing beyond the defined bits, every accepted item carries none"""
    import numpy as np
    st = np.asarray(st)
    e = np.asarray(expect)
    bad = np.arange(7, len(st), 16)
    flag = np.array(BUILD_INPUTS_FLAG)[((bad % (period or len(st))) // 16) % 5]
    assert ((st[bad] & flag) != 0).all(), [(int(i), int(st[i])) for i in bad[(st[bad] & flag) == 0][:8]]
    assert ((st[bad] & ~0x1FF) == 0).all(), [(int(i), int(st[i])) for i in bad[(st[bad] & ~0x1FF) != 0][:8]]
    assert (st[e == 1] == 0).all(), [(int(i), int(st[i])) for i in np.flatnonzero((e == 1) & (st != 0))[:8]]
    assert (e[bad] == 0).all() and int((e == 0).sum()) == len(bad)
