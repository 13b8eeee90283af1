"""CPU checks of the committee stream's pure parts (include/mbls.h, mbls_stream_create_committee): the arithmetic of one destination dword of the gather
(milagro_bls_amd/csrc/mbls_stream.h stream_bits_fast / stream_bits_dword, the text k_stream_gather_cmt runs; built with the host compiler by
tests/stream_cmt_emul/mbls_stream_cmt_harness.cpp) against a numpy model, the harness as a program of its own under the address and undefined-behaviour
sanitizers, mbls_stream_cut on the shapes a committee call has, and what the three entries refuse, or fail loudly at, on a machine without a GPU."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import helpers
from milagro_bls_amd import _native as N
from test_stream_cpu import model_cut

CXX = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SRC = os.path.join(helpers.ROOT, "tests", "stream_cmt_emul", "mbls_stream_cmt_harness.cpp")
POISON = 0xFF
PAD = 8


@pytest.fixture(scope="module")
def sch(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stream_cmt") / "libstream_cmt_harness.so")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    h = C.CDLL(so)
    h.sch_fast.restype = C.c_int; h.sch_fast.argtypes = [C.c_void_p, C.c_uint32]
    h.sch_dword.restype = C.c_uint32; h.sch_dword.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    h.sch_tile.restype = None; h.sch_tile.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    return h


def placed(fields, mis):
    """the fields back to back, `mis` bytes past a 16-byte boundary, 0xFF before and behind -> (array kept alive, address of the first field)"""
    total = fields.size
    raw = np.full(16 + PAD + 4 + total + PAD + 16, POISON, dtype=np.uint8)
    base = (-raw.ctypes.data) % 16 + 16 + mis                  # 16-byte boundary + mis, at least PAD poisoned bytes in front
    raw[base:base + total] = fields.reshape(-1)
    return raw, raw.ctypes.data + base


def model_dword(field, bits_len, j):
    """bytes [4 j, 4 j + 4) of the field zero-extended, little-endian"""
    ext = np.zeros(4 * (j + 1), dtype=np.uint8)
    m = min(bits_len, ext.size)
    ext[:m] = field[:m]
    return int(ext[4 * j:4 * j + 4].view("<u4")[0])


def test_every_length_misalignment_and_destination_dword(sch):
    """bits_len 1 .. 24 x source misalignment 0 .. 3 x every destination dword of a 28-byte stride (dwords wholly past the field included), the field between
    0xFF bytes and holding no zero byte: a byte read outside [0, bits_len) shows as a bit where the model has none; with the fast decision as the kernel takes it
    and, wherever it is on, with it off as well"""
    rnd = np.random.default_rng(5)
    seen_fast = 0
    for bits_len in range(1, 25):
        for mis in range(4):
            field = rnd.integers(1, 255, size=bits_len, dtype=np.uint8)
            raw, addr = placed(field, mis)
            fast = sch.sch_fast(addr, bits_len)
            assert fast == int(mis == 0 and bits_len % 4 == 0)
            seen_fast += fast
            for j in range(7):
                want = model_dword(field, bits_len, j)
                assert sch.sch_dword(addr, bits_len, j, fast) == want, (bits_len, mis, j)
                assert sch.sch_dword(addr, bits_len, j, 0) == want, (bits_len, mis, j)
    assert seen_fast == 6


def test_a_tile_of_fields_is_zero_extended_to_the_stride(sch):
    """several fields back to back -- only the first one's address decides the fast path, the others follow from bits_len -- into every stride that holds them: every
    byte of the destination is written (it starts as 0xA5), bytes at or beyond bits_len are zero"""
    rnd = np.random.default_rng(6)
    for bits_len in range(1, 25):
        for mis in range(4):
            items = 5
            fields = rnd.integers(1, 255, size=(items, bits_len), dtype=np.uint8)
            raw, addr = placed(fields, mis)
            for stride in range((bits_len + 3) // 4 * 4, 29, 4):
                out = np.full((items, stride), 0xA5, dtype=np.uint8)
                sch.sch_tile(addr, bits_len, items, stride, out.ctypes.data)
                want = np.zeros((items, stride), dtype=np.uint8)
                want[:, :bits_len] = fields
                assert np.array_equal(out, want), (bits_len, mis, stride)


def test_harness_as_its_own_program_under_asan_and_ubsan():
    """the same functions over heap blocks that end with the last field: a read past a field, a misaligned dword load or a write past the stride aborts the program"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "stream_cmt_harness")
        subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMBLS_STREAM_CMT_HARNESS_MAIN", "-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-300:], r.stderr[-2000:])


def cut(calls, ri, rk, rm):
    return [(p["call"], p["first"], p["items"], p["round"], p["round_first"]) for p in N.stream_cut(calls, ri, rk, rm)]


def test_cut_of_committee_shapes_equals_the_model():
    """a committee call is {n, k = 0, msg_len = 4}: items and the 4 index bytes per item close a round, round_keys plays no part"""
    shapes = [dict(n=n, k=0, msg_len=4) for n in (1, 100, 300, 55)]
    shapes[-1]["flush_after"] = 1
    want = [(0, 0, 1, 0, 0), (1, 0, 100, 0, 1), (2, 0, 155, 0, 101), (2, 155, 145, 1, 0), (3, 0, 55, 1, 145)]
    for rk in (1, 256, 128 * 256):
        assert cut(shapes, 256, rk, 4 * 256) == want == model_cut(shapes, 256, rk, 4 * 256)
    # fewer index bytes than items: the bytes close the round
    assert cut([dict(n=100, k=0, msg_len=4)], 256, 1, 160) == [(0, 0, 40, 0, 0), (0, 40, 40, 1, 0), (0, 80, 20, 2, 0)]
    rnd = random.Random(11)
    for trial in range(40):
        calls = [dict(n=rnd.choice([1, 2, 16, 63, 64, 65, 255, 256, 257, 700]), k=0, msg_len=4, flush_after=rnd.random() < 0.2) for _ in range(rnd.randrange(1, 14))]
        ri = rnd.choice([64, 256, 512]); rm = rnd.choice([4 * ri, 4 * ri - 4, 200])
        assert cut(calls, ri, 1, rm) == model_cut(calls, ri, 1, rm), trial


def test_entries_refuse_null_handles_and_fail_loudly_without_a_gpu():
    L = N.lib()
    out = C.c_void_p()
    t = C.c_uint64(0)
    res = (C.c_uint8 * 4)(9, 9, 9, 9)
    assert L.mbls_stream_create_committee(None, None, None, 16, None, C.byref(out)) == N.ERR_ARGUMENT and not out.value
    assert L.mbls_stream_submit_committee(None, None, None, None, None, 16, 4, res, None, C.byref(t)) == N.ERR_ARGUMENT
    assert L.mbls_stream_submit_committee_device(None, None, None, None, None, 16, 4, res, None, None, None, C.byref(t)) == N.ERR_ARGUMENT
    assert t.value == 0 and list(res) == [9, 9, 9, 9]
    from milagro_bls_amd.stream import VerifyStream
    with pytest.raises(ValueError):                              # the mirror: a committee stream has a message table and no key table of its own
        VerifyStream(object(), committees=object(), bits_stride=16)
    import torch
    if not torch.cuda.is_available():                            # no CPU fallback: without a context there are no tables and no stream
        with pytest.raises(N.MblsError):
            N.Context(0)
        with pytest.raises(N.MblsError):
            VerifyStream(committees=N.CommitteeTable(N.KeyTable()), msg_table=N.MsgTable(), bits_stride=16)
