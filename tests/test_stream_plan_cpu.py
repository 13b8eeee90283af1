"""CPU checks of the verification stream's round plan and of the one step every walk over a queue takes (milagro_bls_amd/csrc/mbls_stream_plan.h and
mbls_stream.h, built with the host compiler by tests/stream_plan_emul/mbls_stream_plan_harness.cpp): the plan of hand-built rounds of every kind against a model
written here from the rules in the header's comments -- tile lists, host copies, offset tables, the places of the meta area --, with data pointers nothing is
mapped at; every plan the cutting rule can produce against meta_capacity; the step against mbls_stream_cut and mbls_stream_cut_vm over random queues; the harness
as a program of its own under the address and undefined-behaviour sanitizers."""
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
SRC = os.path.join(helpers.ROOT, "tests", "stream_plan_emul", "mbls_stream_plan_harness.cpp")
KEYS, COMMITTEE, VM = 0, 1, 2
GATHER_TILE, SCATTER_TILE, CMT_TILE = 128 * 1024, 4096, 256
SIGS, MSGS, KEYARR, CID, RANDS = range(5)                 # the arrays of a round
DIRECT, STAGE, WIDEN, UPLOAD = range(4)                   # the ways of a host copy
SIZEOF = {"gt": 24, "st": 48, "ct": 48, "vt": 56, "vst": 64}
STRIDE = 20
DEV = [0x7A0000000000 + (a << 36) for a in range(5)]      # a slot's device arrays: addresses only


class Opts(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("verify", C.c_uint32), ("unit", C.c_uint64), ("bits_stride", C.c_uint32), ("pad", C.c_uint32), ("round_items", C.c_uint64),
                ("round_keys", C.c_uint64), ("round_msg_bytes", C.c_uint64)]


class Call(C.Structure):
    _fields_ = [("n", C.c_uint64), ("k", C.c_uint32), ("msg_len", C.c_uint32), ("pk_offsets", C.c_void_p), ("msg_offsets", C.c_void_p), ("flush_after", C.c_uint32),
                ("host", C.c_uint32), ("bits_len", C.c_uint32), ("pad", C.c_uint32), ("groups", C.c_uint64)]


class Piece(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("call", "first", "items", "round", "round_first", "batch")]


@pytest.fixture(scope="module")
def sph(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stream_plan") / "libstream_plan_harness.so")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    h = C.CDLL(so)
    h.sph_capacity.restype = C.c_uint64; h.sph_capacity.argtypes = [C.c_void_p]
    h.sph_tile.restype = C.c_uint64; h.sph_tile.argtypes = [C.c_int]
    h.sph_addr.restype = C.c_uint64; h.sph_addr.argtypes = [C.c_uint64, C.c_uint64]
    h.sph_plan.restype = None; h.sph_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    h.sph_rows.restype = C.c_uint64; h.sph_rows.argtypes = [C.c_int, C.c_void_p]
    h.sph_scalars.restype = None; h.sph_scalars.argtypes = [C.c_void_p]
    h.sph_pack.restype = None; h.sph_pack.argtypes = [C.c_void_p]
    h.sph_widen.restype = None; h.sph_widen.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64]
    h.sph_walk.restype = C.c_int64; h.sph_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    assert [h.sph_tile(i) for i in range(3)] == [GATHER_TILE, SCATTER_TILE, CMT_TILE]
    return h


def addr(j, a):
    """the data address the harness gives array a of call j (0 sigs, 1 msgs, 2 keys, 3 bits, 4 rands, 5 res, 6 bm, 7 st, 8 set_res, 9 set_st)"""
    return 0x100000000000 * (a + 1) + (j << 24)


def c_calls(calls):
    """dicts (n, k, msg_len, pk_offsets, msg_offsets, flush_after, host, bits_len, groups) -> (Call array, the offset arrays kept alive, each exactly n + 1 long)"""
    arr, keep = (Call * len(calls))(), []
    for i, c in enumerate(calls):
        a = arr[i]
        a.n, a.k, a.msg_len, a.flush_after, a.host = c["n"], c.get("k", 0), c.get("msg_len", 0), int(c.get("flush_after", 0)), int(c.get("host", 0))
        a.bits_len, a.groups = c.get("bits_len", 0), c.get("groups", c["n"])
        for name, dt in (("pk_offsets", np.uint32), ("msg_offsets", np.uint64)):
            if c.get(name) is not None:
                t = c[name] if isinstance(c[name], np.ndarray) else np.array(c[name], dtype=dt)
                assert t.dtype == dt and len(t) == c["n"] + 1
                keep.append(t); setattr(a, name, t.ctypes.data)
    return arr, keep


def opts(kind, round_items=1 << 20, round_keys=None, round_msg_bytes=None, unit=48, verify=0):
    return Opts(kind, verify, unit if kind == KEYS else 0, 0 if kind == KEYS else STRIDE, 0, round_items, round_keys or 128 * round_items,
                round_msg_bytes or (64 if kind == KEYS else 4) * round_items)


def plan(sph, o, calls, pieces):
    """pieces: (call, first, items) in round order -> what the harness's plan holds, as lists of tuples and a dict of scalars"""
    cc, keep = c_calls(calls)
    pp, at = (Piece * len(pieces))(), 0
    for i, (j, first, items) in enumerate(pieces):
        pp[i] = Piece(j, first, items, 0, at, i)
        at += items
    dev = (C.c_uint64 * 5)(*DEV)
    sph.sph_plan(C.byref(o), cc, len(calls), pp, len(pieces), dev)
    out = {}
    for which, (name, cols) in enumerate([("gt", 3), ("ct", 7), ("vt", 8), ("st", 6), ("vst", 8), ("off32", 1), ("moff", 1), ("hc", 8)]):
        n = sph.sph_rows(which, None)
        buf = np.zeros(max(1, n * cols), dtype=np.uint64)
        assert sph.sph_rows(which, buf.ctypes.data) == n
        out[name] = [tuple(int(x) for x in buf[r * cols:(r + 1) * cols]) for r in range(n)]
    sc = np.zeros(15, dtype=np.uint64); sph.sph_scalars(sc.ctypes.data)
    names = ["keys_uniform", "msgs_uniform", "k", "msg_len", "n", "batches", "max_groups", "gathered", "any_host", "at_g", "at_s", "at_k", "at_m", "at_c", "bytes"]
    out.update({k: int(v) for k, v in zip(names, sc)})
    meta = np.full(out["bytes"], 0xEE, dtype=np.uint8)               # exactly the plan's bytes
    if out["bytes"]:
        sph.sph_pack(meta.ctypes.data)
    out["meta"] = meta
    return out


def up(x, a):
    return (x + a - 1) // a * a


def scatter_tiles(j, first, items, round_first):
    """a device piece's results go back in tiles cut at multiples of SCATTER_TILE in the CALL's item space"""
    out, a = [], first
    while a < first + items:
        b = min(first + items, (a // SCATTER_TILE + 1) * SCATTER_TILE)
        out.append((addr(j, 5), addr(j, 7), addr(j, 6), a, b - a, round_first + a - first))
        a = b
    return out


def model(o, calls, pieces):
    """the plan, from the rules in mbls_stream_plan.h's comments"""
    m = dict(gt=[], ct=[], vt=[], st=[], vst=[], off32=[], moff=[], hc=[], gathered=0, max_groups=0, batches=0, any_host=0)
    n = sum(p[2] for p in pieces)
    bs, unit, at = o.bits_stride, o.unit, 0

    def hc(how, i, src, arr, at, nbytes, ln=0, items=0):
        if nbytes:
            m["hc"].append((src, i, arr, how, ln, at, nbytes, items))
    if o.kind == KEYS:
        used = [calls[p[0]] for p in pieces]
        ku = all(c.get("pk_offsets") is None and c.get("k", 0) == used[0].get("k", 0) for c in used) or bool(o.verify)
        mu = all(c.get("msg_offsets") is None and c.get("msg_len", 0) == used[0].get("msg_len", 0) for c in used)
        koff, moff, key_cur, msg_cur = [], [], 0, 0
        for i, (j, first, items) in enumerate(pieces):
            c = calls[j]
            ko = c["pk_offsets"] if c.get("pk_offsets") is not None else [c.get("k", 0) * x for x in range(c["n"] + 1)]
            mo = c["msg_offsets"] if c.get("msg_offsets") is not None else [c.get("msg_len", 0) * x for x in range(c["n"] + 1)]
            ko, mo = [int(x) for x in ko[first:first + items + 1]], [int(x) for x in mo[first:first + items + 1]]
            for src, arr, to, nbytes in ((addr(j, 0) + 96 * first, SIGS, 96 * at, 96 * items), (addr(j, 1) + mo[0], MSGS, msg_cur, mo[-1] - mo[0]),
                                        (addr(j, 2) + unit * ko[0], KEYARR, unit * key_cur, unit * (ko[-1] - ko[0]))):
                m["gathered"] += nbytes
                if c.get("host"):
                    hc(DIRECT, i, src, arr, to, nbytes)
                else:
                    m["gt"] += [(src + x, DEV[arr] + to + x, min(GATHER_TILE, nbytes - x)) for x in range(0, nbytes, GATHER_TILE)]
            koff += [key_cur + x - ko[0] for x in ko[:-1]]; moff += [msg_cur + x - mo[0] for x in mo[:-1]]
            key_cur += ko[-1] - ko[0]; msg_cur += mo[-1] - mo[0]
            if not c.get("host"):
                m["st"] += scatter_tiles(j, first, items, at)
            m["any_host"] |= int(c.get("host", 0))
            at += items
        m["off32"] = [] if ku else [(x,) for x in koff + [key_cur]]
        m["moff"] = [] if mu else [(x,) for x in moff + [msg_cur]]
        m.update(keys_uniform=int(ku), msgs_uniform=int(mu), k=1 if o.verify else used[0].get("k", 0), msg_len=used[0].get("msg_len", 0))
    elif o.kind == COMMITTEE:
        for i, (j, first, items) in enumerate(pieces):
            c = calls[j]; bl = c["bits_len"]
            m["gathered"] += (96 + 4 + 4 + bl) * items
            if c.get("host"):                   # three arrays straight from the caller's memory; the fields widened in pinned memory, then uploaded
                hc(DIRECT, i, addr(j, 0) + 96 * first, SIGS, 96 * at, 96 * items); hc(DIRECT, i, addr(j, 1) + 4 * first, MSGS, 4 * at, 4 * items)
                hc(DIRECT, i, addr(j, 2) + 4 * first, CID, 4 * at, 4 * items)
                hc(WIDEN, i, addr(j, 3) + bl * first, KEYARR, bs * at, bs * items, bl, items); hc(UPLOAD, i, 0, KEYARR, bs * at, bs * items)
                m["any_host"] = 1
            else:
                for a in range(first, first + items, CMT_TILE):
                    m["ct"].append((addr(j, 0) + 96 * a, addr(j, 1) + 4 * a, addr(j, 2) + 4 * a, addr(j, 3) + bl * a, bl, min(CMT_TILE, first + items - a), at + a - first))
                m["st"] += scatter_tiles(j, first, items, at)
            at += items
        m.update(keys_uniform=1, msgs_uniform=1)
    else:
        run = None                              # the open run of neighbouring host calls: [first set, end)

        def flush(i):
            nonlocal run
            if run:
                a, cnt = run[0], run[1] - run[0]
                for arr, w in ((SIGS, 96), (CID, 4), (MSGS, 4), (RANDS, 8), (KEYARR, bs)):
                    hc(UPLOAD, i, 0, arr, w * a, w * cnt)
            run = None
        for i, (j, first, items) in enumerate(pieces):
            c = calls[j]; bl = c["bits_len"]
            assert first == 0 and items == c["n"]
            m["gathered"] += (96 + 4 + 4 + 8 + bl) * items; m["max_groups"] += c.get("groups", c["n"])
            m["off32"].append((at,))
            if c.get("host"):
                if run and run[1] != at:
                    flush(i)
                run = [run[0] if run else at, at + items]
                for a, arr, w in ((0, SIGS, 96), (2, CID, 4), (1, MSGS, 4), (4, RANDS, 8)):
                    hc(STAGE, i, addr(j, a), arr, w * at, w * items)
                hc(WIDEN, i, addr(j, 3) if bl else 0, KEYARR, bs * at, bs * items, bl, items)
                m["any_host"] = 1
            else:
                flush(i)
                for a in range(0, items, CMT_TILE):
                    m["vt"].append((addr(j, 0) + 96 * a, addr(j, 2) + 4 * a, addr(j, 3) + bl * a if bl else 0, addr(j, 1) + 4 * a, addr(j, 4) + 8 * a, bl, min(CMT_TILE, items - a), at + a))
                for a in range(0, items, SCATTER_TILE):
                    m["vst"].append((addr(j, 5), addr(j, 7), addr(j, 8), addr(j, 9), a, min(SCATTER_TILE, items - a), at + a, n + i))
            at += items
        flush(len(pieces))
        m["off32"].append((n,))
        m.update(keys_uniform=1, msgs_uniform=1, batches=len(pieces))
    m["n"] = n
    # the meta area: gather tiles | scatter tiles (16-aligned) | the 32-bit table | message offsets | committee tiles (16-aligned)
    if o.kind == VM:
        m["at_g"] = 0; m["at_s"] = up(len(m["vt"]) * SIZEOF["vt"], 16); m["at_k"] = up(m["at_s"] + len(m["vst"]) * SIZEOF["vst"], 16)
        m["bytes"] = m["at_k"] + 4 * len(m["off32"])
    else:
        m["at_g"] = 0; m["at_s"] = up(len(m["gt"]) * SIZEOF["gt"], 16); m["at_k"] = up(m["at_s"] + len(m["st"]) * SIZEOF["st"], 8)
        m["at_m"] = up(m["at_k"] + 4 * len(m["off32"]), 8); m["at_c"] = up(m["at_m"] + 8 * len(m["moff"]), 16); m["bytes"] = m["at_c"] + len(m["ct"]) * SIZEOF["ct"]
    return m


def agree(sph, o, calls, pieces):
    got, want = plan(sph, o, calls, pieces), model(o, calls, pieces)
    for k, v in want.items():
        assert got[k] == v, (k, got[k][:6] if isinstance(v, list) else got[k], v[:6] if isinstance(v, list) else v)
    # the packed meta area holds the tables where the plan says
    meta = got["meta"]
    if got["off32"]:
        assert meta[got["at_k"]:got["at_k"] + 4 * len(got["off32"])].view(np.uint32).tolist() == [x[0] for x in got["off32"]]
    if got["moff"]:
        assert meta[got["at_m"]:got["at_m"] + 8 * len(got["moff"])].view(np.uint64).tolist() == [x[0] for x in got["moff"]]
    tiles = got["gt"] or got["vt"]
    if got["gt"]:
        assert meta[:24 * len(tiles)].view(np.uint64).reshape(-1, 3).tolist() == [list(t) for t in tiles]
    if got["st"]:
        assert meta[got["at_s"]:got["at_s"] + 48 * len(got["st"])].view(np.uint64).reshape(-1, 6).tolist() == [list(t) for t in got["st"]]
    return got


def test_no_data_address_of_the_harness_is_mapped():
    """the calls' data pointers and the slot's arrays are addresses of nothing: a plan that read a call's data would end the test process"""
    spans = []
    with open("/proc/self/maps") as fh:
        for line in fh:
            lo, hi = (int(x, 16) for x in line.split()[0].split("-"))
            spans.append((lo, hi))
    for a in [addr(j, x) for j in (0, 1, 50, 9000) for x in range(10)] + DEV:
        assert not any(lo <= a < hi for lo, hi in spans), hex(a)


def test_keys_rounds_against_the_model(sph):
    ragged_k = np.array([0, 1, 3, 3, 6, 7], dtype=np.uint32)
    ragged_m = np.array([5, 5, 40, 41, 300], dtype=np.uint64)
    calls = [dict(n=1, k=1, msg_len=32),                              # 0: one item
             dict(n=9000, k=2, msg_len=32),                           # 1: a piece from item 4095 on straddles a scatter tile
             dict(n=5, msg_len=32, pk_offsets=ragged_k, host=1),      # 2: ragged keys, host
             dict(n=4096, k=1, msg_len=32),                           # 3: a message segment of exactly GATHER_TILE bytes
             dict(n=8193, k=0, msg_len=16),                           # 4: ... and of GATHER_TILE + 16
             dict(n=3, k=2, msg_len=32, host=1),                      # 5: uniform, host
             dict(n=4, k=1, msg_offsets=ragged_m),                    # 6: ragged messages, device
             dict(n=1, k=0, msg_len=0, host=1)]                       # 7: nothing but a signature
    o = opts(KEYS)
    got = agree(sph, o, calls, [(0, 0, 1), (1, 4095, 2), (2, 1, 3), (3, 0, 4096), (4, 0, 8193), (5, 0, 3), (6, 0, 4), (7, 0, 1), (1, 8191, 3)])
    assert not got["keys_uniform"] and not got["msgs_uniform"] and len(got["off32"]) == got["n"] + 1 == len(got["moff"])
    assert [t[2] for t in got["gt"] if t[0] == addr(3, 1)] == [GATHER_TILE] and [t[2] for t in got["gt"] if t[0] >= addr(4, 1) and t[0] < addr(5, 1)] == [GATHER_TILE, 16]
    assert [t[3:5] for t in got["st"] if t[0] == addr(1, 5)][:2] == [(4095, 1), (4096, 1)]
    # a ragged-keys piece next to a uniform one with the same messages: key offsets present, message offsets absent
    got = agree(sph, o, calls, [(5, 0, 3), (2, 0, 5), (0, 0, 1)])
    assert not got["keys_uniform"] and got["msgs_uniform"] and got["moff"] == [] and [x[0] for x in got["off32"]] == [0, 2, 4, 6, 7, 9, 9, 12, 13, 14]
    # every piece shares the layout: no tables; host and device alternate
    same = [dict(n=7, k=2, msg_len=32, host=h) for h in (0, 1, 0, 1, 0)]
    got = agree(sph, o, same, [(0, 3, 4), (1, 0, 7), (2, 0, 7), (3, 0, 7), (4, 0, 2)])
    assert got["keys_uniform"] and got["msgs_uniform"] and got["k"] == 2 and got["off32"] == [] and [h[1] for h in got["hc"]] == [1, 1, 1, 3, 3, 3]
    # verify mode: one key per item whatever the shapes say; 4-byte units (key-table indices)
    agree(sph, opts(KEYS, verify=1, unit=96), [dict(n=3, k=1, msg_len=8), dict(n=2, k=1, msg_len=8, host=1)], [(0, 0, 3), (1, 0, 2)])
    agree(sph, opts(KEYS, unit=4), calls, [(1, 0, 4097), (2, 0, 5)])


def test_committee_rounds_against_the_model(sph):
    calls = [dict(n=1, bits_len=1), dict(n=CMT_TILE, bits_len=STRIDE), dict(n=CMT_TILE + 1, bits_len=7), dict(n=4, bits_len=1, host=1), dict(n=5000, bits_len=17),
             dict(n=3, bits_len=STRIDE, host=1), dict(n=2, bits_len=19, host=1)]
    for c in calls:
        c.update(k=0, msg_len=4)
    o = opts(COMMITTEE)
    got = agree(sph, o, calls, [(0, 0, 1), (3, 0, 4), (1, 0, CMT_TILE), (5, 1, 2), (2, 0, CMT_TILE + 1), (4, 4095, 2), (6, 0, 2), (4, 4097, 600)])
    assert [t[5] for t in got["ct"]] == [1, CMT_TILE, CMT_TILE, 1, 2, 256, 256, 88] and got["gt"] == [] and got["off32"] == [] and got["moff"] == []
    assert [(t[3], t[4]) for t in got["st"] if t[0] == addr(4, 5)] == [(4095, 1), (4096, 1), (4097, 600)]
    assert [(h[3], h[4]) for h in got["hc"] if h[2] == KEYARR] == [(WIDEN, 1), (UPLOAD, 0), (WIDEN, STRIDE), (UPLOAD, 0), (WIDEN, 19), (UPLOAD, 0)]
    agree(sph, o, calls, [(3, 2, 1)])
    agree(sph, o, calls, [(0, 0, 1)])


def test_verify_multiple_rounds_against_the_model(sph):
    calls = [dict(n=1, bits_len=0), dict(n=2, bits_len=1, host=1), dict(n=3, bits_len=STRIDE - 1, host=1, groups=2), dict(n=CMT_TILE, bits_len=STRIDE),
             dict(n=CMT_TILE + 1, bits_len=1), dict(n=1, bits_len=STRIDE, host=1), dict(n=SCATTER_TILE + 1, bits_len=STRIDE - 1), dict(n=5, bits_len=0, host=1, groups=1),
             dict(n=4, bits_len=STRIDE, host=1)]
    for c in calls:
        c.update(k=0, msg_len=4)
    o = opts(VM)
    got = agree(sph, o, calls, [(j, 0, c["n"]) for j, c in enumerate(calls)])
    assert got["batches"] == len(calls) and [x[0] for x in got["off32"]][:4] == [0, 1, 3, 6] and got["off32"][-1][0] == got["n"]
    # runs of neighbouring host calls go up together: calls 1 and 2, call 5 alone, calls 7 and 8 behind the last piece
    ups = [(h[1], h[5] // 96, h[6] // 96) for h in got["hc"] if h[3] == UPLOAD and h[2] == SIGS]
    assert ups == [(3, 1, 5), (6, 6 + 2 * CMT_TILE + 1, 1), (9, got["n"] - 9, 9)]
    assert [h[4] for h in got["hc"] if h[3] == WIDEN] == [1, STRIDE - 1, STRIDE, 0, STRIDE]
    assert [t[2] for t in got["vt"]][0] == 0                                   # bits_len = 0: no field address at all
    assert [(t[4], t[5]) for t in got["vst"] if t[0] == addr(6, 5)] == [(0, SCATTER_TILE), (SCATTER_TILE, 1)]
    agree(sph, o, calls, [(1, 0, 2)])
    agree(sph, o, calls, [(0, 0, 1)])
    agree(sph, o, calls, [(1, 0, 2), (0, 0, 1), (2, 0, 3), (4, 0, CMT_TILE + 1), (5, 0, 1)])


@pytest.mark.parametrize("bits_len", [0, 1, STRIDE - 1, STRIDE])
def test_widening_fields_to_the_stride(sph, bits_len):
    rnd = np.random.default_rng(bits_len)
    for items in (1, 5):
        src = rnd.integers(1, 255, size=(items, bits_len), dtype=np.uint8)
        out = np.full((items, STRIDE), 0xA5, dtype=np.uint8)
        sph.sph_widen(out.ctypes.data, src.ctypes.data if bits_len else None, items, bits_len, STRIDE)
        want = np.zeros((items, STRIDE), dtype=np.uint8); want[:, :bits_len] = src
        assert np.array_equal(out, want)


def walk(sph, o, calls):
    cc, keep = c_calls(calls)
    cap = sum(c["n"] for c in calls)                                  # a piece and a round hold at least one item
    out, info, cnt = (Piece * cap)(), np.zeros(4 * cap, dtype=np.uint64), C.c_uint64(0)
    rounds = sph.sph_walk(C.byref(o), cc, len(calls), out, cap, C.byref(cnt), info.ctypes.data, cap)
    assert rounds >= 1 and cnt.value <= cap, rounds
    return rounds, [out[i] for i in range(cnt.value)], info[:4 * rounds].reshape(rounds, 4)


def worst_queues(kind, R):
    """the rounds that take the most meta bytes under the cutting rule"""
    dev = dict(k=0, msg_len=4, bits_len=STRIDE)
    if kind == VM:
        big = min(SCATTER_TILE + 1, R - 1)
        return [[dict(n=1, **dev) for _ in range(R)],                                       # R / 2 one-set calls per round
                [dict(n=R - 1, **dev)] * 2,                                                 # one call fills the round
                [dict(n=big, **dev) for _ in range(3 * R // (big + 1) + 2)]]                # calls that each straddle a scatter tile (where a round holds one)
    if kind == COMMITTEE:
        return [[dict(n=1, **dev) for _ in range(R + 3)], [dict(n=3 * R + 1, **dev)], [dict(n=SCATTER_TILE + 1, **dev) for _ in range(3 * R // (SCATTER_TILE + 1) + 3)]]
    one_k, one_m = np.array([0, 1], dtype=np.uint32), np.array([0, 1], dtype=np.uint64)
    full_k, full_m = np.array([0, 128], dtype=np.uint32), np.array([3, 67], dtype=np.uint64)
    return [[dict(n=1, k=1, msg_len=32) for _ in range(R + 3)],
            [dict(n=3 * R + 1, k=128, msg_len=64)],                                         # full rounds of the most bytes a round holds
            [dict(n=SCATTER_TILE + 1, k=1, msg_len=1) for _ in range(3 * R // (SCATTER_TILE + 1) + 3)],
            [dict(n=1, pk_offsets=one_k, msg_offsets=one_m) for _ in range(R + 3)],         # ragged tables, one key and one byte per item
            [dict(n=1, pk_offsets=full_k, msg_offsets=full_m) for _ in range(R + 3)],       # ... and 128 keys, 64 bytes
            [dict(n=1, k=1, msg_len=32), dict(n=2 * R, pk_offsets=np.arange(2 * R + 1, dtype=np.uint32), msg_len=3)]]


@pytest.mark.parametrize("round_items", [2, 3, 255, 256, 257, 4095, 4096, 4097, 8193])
@pytest.mark.parametrize("kind", [KEYS, COMMITTEE, VM])
def test_no_round_the_cutting_rule_makes_exceeds_meta_capacity(sph, kind, round_items):
    R = round_items
    settings = [opts(kind, R)] if kind != KEYS else [opts(KEYS, R, unit=u) for u in (96, 4)] + [opts(KEYS, R, R, R, unit=96)]
    for o in settings:
        cap = sph.sph_capacity(C.byref(o))
        for q in worst_queues(kind, R):
            if kind == KEYS and o.round_keys == R:                    # one key and one message byte per item is all such a round holds
                q = [c for c in q if c.get("k", 0) <= 1 and c.get("msg_len", 0) <= 1 and (c.get("pk_offsets") is None or int(c["pk_offsets"][1]) - int(c["pk_offsets"][0]) <= 1)
                     and (c.get("msg_offsets") is None or int(c["msg_offsets"][1]) - int(c["msg_offsets"][0]) <= 1)]
                if not q:
                    continue
            rounds, pieces, info = walk(sph, o, q)
            assert int(info[:, 0].max()) <= cap, (kind, R, int(info[:, 0].max()), cap)
            assert int(info[:, 1].max()) <= R


def test_the_step_against_the_cuts_over_random_queues(sph):
    rnd = random.Random(99)
    for trial in range(120):
        R = rnd.choice([2, 3, 4, 16, 17, 64, 257])
        # whole calls: the pieces of the step are mbls_stream_cut_vm's, no call is split, and the round's cost is its sets plus its calls
        sets = [rnd.randrange(1, R) for _ in range(rnd.randrange(1, 40))]
        fl = [rnd.random() < 0.15 for _ in sets]
        rounds, pieces, info = walk(sph, opts(VM, R), [dict(n=n, k=0, msg_len=4, flush_after=f) for n, f in zip(sets, fl)])
        want = N.stream_cut_vm(sets, R, fl)
        assert [(p.call, p.first, p.items, p.round, p.round_first) for p in pieces] == [(w["call"], w["first"], w["items"], w["round"], w["round_first"]) for w in want]
        assert all(p.first == 0 and p.items == sets[p.call] for p in pieces) and len(pieces) == len(sets)
        for r in range(rounds):
            mine = [p for p in pieces if p.round == r]
            assert [p.batch for p in mine] == list(range(len(mine)))
            assert int(info[r, 1]) == int(info[r, 2]) + int(info[r, 3]) == sum(p.items for p in mine) + len(mine) <= R
        # split calls, uniform and ragged
        rk, rm = rnd.randrange(1, 4 * R + 1), rnd.randrange(4, 8 * R + 1)
        calls = []
        for _ in range(rnd.randrange(1, 12)):
            n = rnd.randrange(1, 3 * R)
            c = dict(n=n, k=rnd.randrange(0, min(rk, 3) + 1), msg_len=rnd.randrange(0, 5), flush_after=rnd.random() < 0.2)
            if rnd.random() < 0.4:
                c["pk_offsets"] = np.cumsum([rnd.randrange(0, 5)] + [rnd.randrange(0, min(rk, 3) + 1) for _ in range(n)]).astype(np.uint32)
            if rnd.random() < 0.4:
                c["msg_offsets"] = np.cumsum([rnd.randrange(0, 5)] + [rnd.randrange(0, 5) for _ in range(n)]).astype(np.uint64)
            calls.append(c)
        rounds, pieces, info = walk(sph, opts(KEYS, R, rk, rm), calls)
        want = N.stream_cut([dict(c, pk_offsets=None if c.get("pk_offsets") is None else c["pk_offsets"].tolist(),
                                  msg_offsets=None if c.get("msg_offsets") is None else c["msg_offsets"].tolist()) for c in calls], R, rk, rm)
        assert [(p.call, p.first, p.items, p.round, p.round_first) for p in pieces] == [(w["call"], w["first"], w["items"], w["round"], w["round_first"]) for w in want], trial
        assert rounds == want[-1]["round"] + 1 and all(p.batch == 0 for p in pieces)


def test_harness_as_its_own_program_under_asan_and_ubsan():
    """random queues of every kind walked and planned with every offset table and output array exactly as long as it is used, and fields widened between blocks
    that end with the last field: a read past a table or through a data pointer, or a write past an array, aborts the program"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "stream_plan_harness")
        subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMBLS_STREAM_PLAN_HARNESS_MAIN", "-o", exe, SRC])
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-300:], r.stderr[-2000:])
