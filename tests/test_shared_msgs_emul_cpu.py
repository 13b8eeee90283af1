"""The shared-message pipeline on the CPU, lane body by lane body (tests/host_emul/mbls_emul_shared.cpp: hash the list in pieces, lane_h_export, lane_h_gather, then the
rest of the pipeline) against the per-item pipeline of tests/host_emul/mbls_emul.cpp (emul_verify_batch) on the spelled-out messages -- results AND status words --
and against the oracle, over the shapes of the GPU tests: crossed indices over three messages, more messages than items with the list in pieces, indices that name
no message. The lane bodies are the ones the HIP kernels k_h_export_tab / k_h_gather wrap."""
import ctypes as C
import os
import random
import subprocess

import pytest

import helpers
import shared_msgs_cases as smc
from helpers import cb, ob

BAD = smc.ST_BAD_MSG_RANGE


@pytest.fixture(scope="module")
def emul_shared():
    d = os.path.join(helpers.ROOT, "tests", "host_emul")
    so = os.path.join(d, "libmbls_emul_shared.so")
    csrc = os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc")
    src = [os.path.join(d, "mbls_emul_shared.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src[0]])
    return C.CDLL(so)


def _msgs(count, seed):
    rnd = random.Random(seed)
    return [rnd.randbytes(32) for _ in range(count)]


def run_shared(lib, cs, idx=None, n_msgs=None, piece=0):
    res = ob(cs.n); st = (C.c_uint32 * cs.n)()
    idx = cs.idx if idx is None else idx
    lib.emul_verify_batch_shared(cb(cs.sigs), cb(cs.list_bytes), 32, None, C.c_uint64(cs.n_msgs if n_msgs is None else n_msgs), (C.c_uint32 * cs.n)(*idx),
                                 cb(cs.pks), cs.fmt, None, C.c_uint64(cs.n), cs.k, 0, C.c_uint64(piece), res, st)
    return [bool(x) for x in bytes(res)[:cs.n]], list(st)


def run_spelled(emul, cs):
    res = ob(cs.n); st = (C.c_uint32 * cs.n)()
    emul.emul_verify_batch(cb(cs.sigs), cb(cs.spelled_bytes), 32, cb(cs.pks), cs.fmt, None, C.c_uint64(cs.n), cs.k, 0, res, st)
    return [bool(x) for x in bytes(res)[:cs.n]], list(st)


@pytest.fixture(scope="module")
def crossed(emul):
    """n = 130, k = 2, three messages; item 0 names message 2 and item 2 names message 0; item 5 signed another message than it names"""
    n = 130
    idx = [2, 1, 0] + [(7 * i + 1) % 3 for i in range(3, n)]
    cs = smc.build(n, 2, _msgs(3, 11), idx, seed=501, signed_as={5: (idx[5] + 1) % 3})
    cs.want = smc.oracle(cs)
    cs.spelled_run = run_spelled(emul, cs)
    return cs


def test_crossed_indices_over_three_messages(emul_shared, crossed):
    cs = crossed
    got, st = run_shared(emul_shared, cs)
    assert (got, st) == cs.spelled_run
    assert got == cs.want == cs.expect
    assert not got[5] and st[5] == smc.ST_PAIRING_FAILED and got[0] and got[2]
    for i, kind in enumerate(cs.kinds):
        assert (st[i] == 0) if kind == "valid" else (kind not in smc.FLAG or st[i] & smc.FLAG[kind]), (i, kind, hex(st[i]))


def test_more_messages_than_items_in_pieces(emul, emul_shared):
    cs = smc.build(3, 2, _msgs(70, 13), [69, 0, 64], seed=503, negatives=False)
    old = run_spelled(emul, cs)
    assert old[0] == smc.oracle(cs) == [True] * 3
    for piece in (0, 64, 7):                      # all at once; 64 + 6 (the GPU test's rounds of 64); ten pieces
        assert run_shared(emul_shared, cs, piece=piece) == old


def test_indices_that_name_no_message(emul_shared, crossed):
    cs = crossed
    idx = list(cs.idx); idx[1] = cs.n_msgs; idx[66] = 0xFFFFFFFF
    got, st = run_shared(emul_shared, cs, idx=idx)
    for i in range(cs.n):
        if i in (1, 66):
            assert not got[i] and st[i] & BAD
        else:
            assert (got[i], st[i]) == (cs.spelled_run[0][i], cs.spelled_run[1][i]), i
    got, st = run_shared(emul_shared, cs, n_msgs=0)
    assert not any(got) and all(s & BAD for s in st)
