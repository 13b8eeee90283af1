"""CPU checks of the verify_multiple stream's pure parts (include/mbls.h, mbls_stream_create_vm_committee): the whole-call rule of
milagro_bls_amd/csrc/mbls_stream.h (stream_vm_fits, stream_take_whole, stream_vm_full; built with the host compiler by
tests/stream_vm_emul/mbls_stream_vm_harness.cpp, which walks a queue as the launcher does) and mbls_stream_cut_vm, which states it as data, against a Python model;
the ragged batch table of a round; the destination dwords of the gather for bits_len in {0, 1, 3, 4, 17, stride} at odd addresses against numpy; the harness
as a program of its own under the address and undefined-behaviour sanitizers; and what the entries refuse, or fail loudly at, on a machine without a GPU."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import helpers
from milagro_bls_amd import _native as N

CXX = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SRC = os.path.join(helpers.ROOT, "tests", "stream_vm_emul", "mbls_stream_vm_harness.cpp")
STRIDE = 20
POISON, PAD = 0xFF, 8


@pytest.fixture(scope="module")
def svh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stream_vm") / "libstream_vm_harness.so")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    h = C.CDLL(so)
    h.svh_fits.restype = C.c_int; h.svh_fits.argtypes = [C.c_uint64, C.c_uint64]
    h.svh_walk.restype = C.c_int64; h.svh_walk.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    h.svh_offsets.restype = None; h.svh_offsets.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    h.svh_tile.restype = None; h.svh_tile.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    return h


def model_cut_vm(call_sets, round_items, flush_after=None):
    """The rule in words: a call of n sets costs n + 1; it joins the open round if the round's cost stays within round_items, otherwise the open round is closed and
    the call opens the next one; a flush closes the round behind its call -> [(call, 0, n, round, first set in the round)]"""
    out, rnd, cost, sets = [], 0, 0, 0
    for j, n in enumerate(call_sets):
        assert 1 <= n and n + 1 <= round_items
        if cost + n + 1 > round_items:
            rnd, cost, sets = rnd + 1, 0, 0
        out.append((j, 0, n, rnd, sets))
        cost += n + 1; sets += n
        if (flush_after is not None and flush_after[j]) or round_items - cost < 2:       # (or nothing more can join: the smallest call costs 2)
            rnd, cost, sets = rnd + 1, 0, 0
    return out


def cut(call_sets, ri, flush_after=None):
    return [(p["call"], p["first"], p["items"], p["round"], p["round_first"]) for p in N.stream_cut_vm(call_sets, ri, flush_after)]


def walk(svh, call_sets, ri, flush_after=None):
    n = len(call_sets)
    sets = np.array(call_sets, dtype=np.uint64)
    fl = None if flush_after is None else np.array([int(bool(f)) for f in flush_after], dtype=np.uint32)
    rd, fs, bt = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    rounds = svh.svh_walk(ri, sets.ctypes.data, None if fl is None else fl.ctypes.data, n, rd.ctypes.data, fs.ctypes.data, bt.ctypes.data)
    return rounds, [(j, 0, int(sets[j]), int(rd[j]), int(fs[j])) for j in range(n)], bt.tolist()


def test_the_edges_of_the_whole_call_rule(svh):
    # a call of exactly round_items - 1 sets is accepted and fills a round alone; one of round_items sets is refused
    assert svh.svh_fits(16, 15) == 1 and svh.svh_fits(16, 16) == 0 and svh.svh_fits(16, 0) == 0 and svh.svh_fits(16, 1) == 1
    assert cut([15], 16) == [(0, 0, 15, 0, 0)] == model_cut_vm([15], 16)
    assert cut([15, 15, 1], 16) == [(0, 0, 15, 0, 0), (1, 0, 15, 1, 0), (2, 0, 1, 2, 0)]
    for bad in ([16], [3, 16], [0], [3, 0, 3]):
        with pytest.raises(N.MblsError) as e:
            cut(bad, 16)
        assert e.value.code == N.ERR_ARGUMENT
        assert walk(svh, bad, 16)[0] == -1
    # a call that closes a round holding one set: 1 set costs 2, the next call of 14 sets costs 15 > 14 left
    assert cut([1, 14, 1], 16) == [(0, 0, 1, 0, 0), (1, 0, 14, 1, 0), (2, 0, 1, 2, 0)] == model_cut_vm([1, 14, 1], 16)
    # ... and one set fewer joins it: 2 + 14 = 16 fills the round exactly
    assert cut([1, 13, 1], 16) == [(0, 0, 1, 0, 0), (1, 0, 13, 0, 1), (2, 0, 1, 1, 0)] == model_cut_vm([1, 13, 1], 16)
    # one item of the round left over: no call fits it, the round is full
    assert cut([1, 12, 1], 16) == [(0, 0, 1, 0, 0), (1, 0, 12, 0, 1), (2, 0, 1, 1, 0)] == model_cut_vm([1, 12, 1], 16)
    # flush_after
    assert cut([3, 3, 3], 16, [0, 1, 0]) == [(0, 0, 3, 0, 0), (1, 0, 3, 0, 3), (2, 0, 3, 1, 0)] == model_cut_vm([3, 3, 3], 16, [0, 1, 0])
    assert cut([3, 3, 3], 16) == [(0, 0, 3, 0, 0), (1, 0, 3, 0, 3), (2, 0, 3, 0, 6)]
    # the arguments mbls_stream_cut_vm refuses
    L = N.lib(); cnt = C.c_uint64(0)
    o = N.StreamOpts(16, 0, 0, 1, 1); sets = (C.c_uint64 * 2)(3, 3); out = (N.StreamPiece * 2)()
    assert L.mbls_stream_cut_vm(None, sets, None, 2, out, 2, C.byref(cnt)) == N.ERR_ARGUMENT
    assert L.mbls_stream_cut_vm(C.byref(o), None, None, 2, out, 2, C.byref(cnt)) == N.ERR_ARGUMENT
    assert L.mbls_stream_cut_vm(C.byref(o), sets, None, 0, out, 2, C.byref(cnt)) == N.ERR_ARGUMENT
    assert L.mbls_stream_cut_vm(C.byref(o), sets, None, 2, out, 1, C.byref(cnt)) == N.ERR_ARGUMENT and cnt.value == 2     # more pieces than max_pieces
    assert L.mbls_stream_cut_vm(C.byref(o), sets, None, 2, None, 0, C.byref(cnt)) == N.OK and cnt.value == 2              # counting
    z = N.StreamOpts(0, 0, 0, 1, 1)
    assert L.mbls_stream_cut_vm(C.byref(z), sets, None, 2, out, 2, C.byref(cnt)) == N.ERR_ARGUMENT


def test_random_queues_cut_vm_the_launchers_walk_and_the_model_agree(svh):
    rnd = random.Random(2024)
    for trial in range(300):
        ri = rnd.choice([2, 3, 4, 16, 17, 64, 257])
        sizes = [1, 2, 3, ri - 1, ri - 2, max(1, ri // 2), max(1, ri // 2 - 1), max(1, ri // 3)]
        calls = [max(1, min(ri - 1, rnd.choice(sizes + [rnd.randrange(1, ri)]))) for _ in range(rnd.randrange(1, 40))]
        fl = None if trial % 3 == 0 else [rnd.random() < 0.15 for _ in calls]
        want = model_cut_vm(calls, ri, fl)
        assert cut(calls, ri, fl) == want, (trial, ri, calls)
        rounds, pieces, batches = walk(svh, calls, ri, fl)
        assert pieces == want, (trial, ri, calls)
        assert rounds == want[-1][3] + 1
        # every call is one piece, never split; within a round the batches count up from 0 and the cost stays within the round
        for r in range(rounds):
            mine = [p for p in want if p[3] == r]
            assert mine and sum(p[2] + 1 for p in mine) <= ri
            assert [batches[p[0]] for p in mine] == list(range(len(mine)))


def test_the_batch_table_of_a_round(svh):
    rnd = random.Random(7)
    for sets in ([1], [5], [1, 1, 1], [3, 10, 63, 1, 2], [rnd.randrange(1, 600) for _ in range(50)]):
        a = np.array(sets, dtype=np.uint64)
        off = np.full(len(sets) + 3, 0xDEADBEEF, dtype=np.uint32)
        svh.svh_offsets(a.ctypes.data, len(sets), off[1:].ctypes.data)
        assert off[1:len(sets) + 2].tolist() == [0] + np.cumsum(a).tolist()
        assert off[0] == 0xDEADBEEF and off[-1] == 0xDEADBEEF                        # B + 1 words, nothing beside them
    # and of every round of a cut queue: the table's entries are the pieces' first sets
    calls = [3, 10, 2, 63, 1, 1, 7, 40, 40]
    pieces = model_cut_vm(calls, 64)
    for r in sorted({p[3] for p in pieces}):
        mine = [p for p in pieces if p[3] == r]
        a = np.array([p[2] for p in mine], dtype=np.uint64); off = np.zeros(len(mine) + 1, dtype=np.uint32)
        svh.svh_offsets(a.ctypes.data, len(mine), off.ctypes.data)
        assert off[:-1].tolist() == [p[4] for p in mine] and int(off[-1]) + len(mine) <= 64


def placed(fields, mis):
    """the fields back to back, `mis` bytes past a 16-byte boundary, 0xFF before and behind -> (array kept alive, address of the first field)"""
    total = fields.size
    raw = np.full(16 + PAD + 4 + total + PAD + 16, POISON, dtype=np.uint8)
    base = (-raw.ctypes.data) % 16 + 16 + mis
    raw[base:base + total] = fields.reshape(-1)
    return raw, raw.ctypes.data + base


@pytest.mark.parametrize("bits_len", [0, 1, 3, 4, 17, STRIDE])
def test_gather_destination_dwords(svh, bits_len):
    """fields of bits_len bytes at every misalignment (odd addresses included), between 0xFF bytes and holding no zero byte, into a destination that starts as
    0xA5: every byte of every set's stride is written, bytes at or beyond bits_len are zero, a byte read outside a field would show; bits_len = 0 reads nothing,
    from a null pointer too"""
    rnd = np.random.default_rng(100 + bits_len)
    for mis in range(4):
        for items in (1, 5):
            fields = rnd.integers(1, 255, size=(items, bits_len), dtype=np.uint8)
            raw, addr = placed(fields, mis)
            for src in ([addr] if bits_len else [addr, None]):
                out = np.full((items, STRIDE), 0xA5, dtype=np.uint8)
                svh.svh_tile(src, bits_len, items, STRIDE, out.ctypes.data)
                want = np.zeros((items, STRIDE), dtype=np.uint8)
                want[:, :bits_len] = fields
                assert np.array_equal(out, want), (bits_len, mis, items)


def test_harness_as_its_own_program_under_asan_and_ubsan():
    """the same functions over heap blocks that end with the last field and arrays exactly as long as they are used: a read past a field, a misaligned dword
    load, a write past the stride or past a round's table aborts the program"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "stream_vm_harness")
        subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMBLS_STREAM_VM_HARNESS_MAIN", "-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-300:], r.stderr[-2000:])


def test_entries_refuse_null_handles_and_fail_loudly_without_a_gpu():
    L = N.lib()
    out = C.c_void_p()
    t = C.c_uint64(0)
    res = (C.c_uint8 * 4)(9, 9, 9, 9)
    assert L.mbls_stream_create_vm_committee(None, None, None, 16, None, C.byref(out)) == N.ERR_ARGUMENT and not out.value
    assert L.mbls_stream_submit_vm(None, None, None, None, 16, None, None, 4, res, None, None, None, C.byref(t)) == N.ERR_ARGUMENT
    assert L.mbls_stream_submit_vm_device(None, None, None, None, 16, None, None, 4, res, None, None, None, None, C.byref(t)) == N.ERR_ARGUMENT
    assert t.value == 0 and list(res) == [9, 9, 9, 9]
    from milagro_bls_amd.stream import VerifyStream
    with pytest.raises(ValueError):                              # the mirror: a verify_multiple stream has both tables
        VerifyStream(object(), vm=True, committees=object(), bits_stride=16)
    with pytest.raises(ValueError):
        VerifyStream(object(), vm=True, msg_table=object(), bits_stride=16)
    import torch
    if not torch.cuda.is_available():                            # no CPU fallback: without a context there are no tables and no stream
        with pytest.raises(N.MblsError):
            VerifyStream(vm=True, committees=N.CommitteeTable(N.KeyTable()), msg_table=N.MsgTable(), bits_stride=16)
