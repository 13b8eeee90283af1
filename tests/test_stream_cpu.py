"""CPU checks of the verification stream's pure parts (include/mbls.h, "verification stream"): the cutting rule mbls_stream_cut states (the
same stream_take the stream's launcher runs), the layout decision of a round and the scatter's bit arithmetic (milagro_bls_amd/csrc/mbls_stream.h,
built with the host compiler by tests/host_emul/mbls_stream_harness.cpp)."""
import ctypes as C
import os
import random
import subprocess

import pytest

import helpers
from milagro_bls_amd import _native as N

R = 4096


def cut(calls, round_items=R, round_keys=128 * R, round_msg_bytes=64 * R):
    return [(p["call"], p["first"], p["items"], p["round"], p["round_first"]) for p in N.stream_cut(calls, round_items, round_keys, round_msg_bytes)]


def model_cut(calls, round_items, round_keys, round_msg_bytes):
    """the rule in plain Python: dense, in order, item by item; a round closes when full or when the next item does not fit"""
    out, rnd, fi, fk, fm = [], 0, 0, 0, 0
    for j, c in enumerate(calls):
        ks = [c["pk_offsets"][i + 1] - c["pk_offsets"][i] for i in range(c["n"])] if c.get("pk_offsets") else [c.get("k", 0)] * c["n"]
        ms = [c["msg_offsets"][i + 1] - c["msg_offsets"][i] for i in range(c["n"])] if c.get("msg_offsets") else [c.get("msg_len", 0)] * c["n"]
        for i in range(c["n"]):
            if fi == round_items or fk + ks[i] > round_keys or fm + ms[i] > round_msg_bytes:
                rnd, fi, fk, fm = rnd + 1, 0, 0, 0
            if out and out[-1][0] == j and out[-1][3] == rnd:
                p = out[-1]; out[-1] = (p[0], p[1], p[2] + 1, p[3], p[4])
            else:
                out.append((j, i, 1, rnd, fi))
            fi, fk, fm = fi + 1, fk + ks[i], fm + ms[i]
        if c.get("flush_after") and fi:
            rnd, fi, fk, fm = rnd + 1, 0, 0, 0
        elif fi == round_items:
            rnd, fi, fk, fm = rnd + 1, 0, 0, 0
    return out


def test_dense_packing_in_submission_order():
    calls = [dict(n=n, k=1, msg_len=32) for n in (1000, 1000, 1000, 1096, 5)]
    assert cut(calls) == [(0, 0, 1000, 0, 0), (1, 0, 1000, 0, 1000), (2, 0, 1000, 0, 2000), (3, 0, 1096, 0, 3000), (4, 0, 5, 1, 0)]


def test_call_split_across_two_and_three_rounds():
    assert cut([dict(n=3000, k=2, msg_len=32), dict(n=3000, k=2, msg_len=32)]) == [(0, 0, 3000, 0, 0), (1, 0, 1096, 0, 3000), (1, 1096, 1904, 1, 0)]
    assert cut([dict(n=100, k=1), dict(n=9000, k=1)]) == [(0, 0, 100, 0, 0), (1, 0, 3996, 0, 100), (1, 3996, 4096, 1, 0), (1, 8092, 908, 2, 0)]


def test_closure_by_item_key_and_message_capacity():
    # items
    assert cut([dict(n=R, k=1)] * 2) == [(0, 0, R, 0, 0), (1, 0, R, 1, 0)]
    # keys: 10 keys per item, 1000 keys per round -> 100 items
    assert cut([dict(n=250, k=10)], round_keys=1000) == [(0, 0, 100, 0, 0), (0, 100, 100, 1, 0), (0, 200, 50, 2, 0)]
    # message bytes: 48-byte messages, 1000 bytes per round -> 20 items
    assert cut([dict(n=30, msg_len=48)], round_msg_bytes=1000) == [(0, 0, 20, 0, 0), (0, 20, 10, 1, 0)]
    # a ragged call whose keys run out before the item count does
    off = [0, 300, 600, 900, 1200, 1201]
    assert cut([dict(n=5, pk_offsets=off)], round_items=64, round_keys=1000) == [(0, 0, 3, 0, 0), (0, 3, 2, 1, 0)]
    moff = [0, 10, 500, 990, 995, 1500]
    assert cut([dict(n=5, k=1, msg_offsets=moff)], round_items=64, round_msg_bytes=1000) == [(0, 0, 4, 0, 0), (0, 4, 1, 1, 0)]


def test_forced_cut_at_flush_after():
    calls = [dict(n=10, k=1, flush_after=1), dict(n=10, k=1), dict(n=10, k=1, flush_after=1), dict(n=5, k=1)]
    assert cut(calls) == [(0, 0, 10, 0, 0), (1, 0, 10, 1, 0), (2, 0, 10, 1, 10), (3, 0, 5, 2, 0)]


def test_random_sequences_match_the_model():
    rnd = random.Random(7)
    for trial in range(60):
        calls = []
        for _ in range(rnd.randrange(1, 12)):
            n = rnd.choice([1, 3, 63, 64, 65, 200, 700])
            c = dict(n=n, flush_after=rnd.random() < 0.2)
            if rnd.random() < 0.5:
                ks = [rnd.randrange(0, 20) for _ in range(n)]
                c["pk_offsets"] = [0] + [sum(ks[:i + 1]) for i in range(n)]
            else:
                c["k"] = rnd.choice([0, 1, 3, 16])
            if rnd.random() < 0.5:
                ms = [rnd.randrange(0, 90) for _ in range(n)]
                c["msg_offsets"] = [5] + [5 + sum(ms[:i + 1]) for i in range(n)]
            else:
                c["msg_len"] = rnd.choice([0, 32, 48])
            calls.append(c)
        ri, rk, rm = rnd.choice([64, 128, 512]), rnd.choice([40, 300, 5000]), rnd.choice([90, 1000, 40000])
        assert cut(calls, ri, rk, rm) == model_cut(calls, ri, rk, rm), trial


def test_refusals():
    with pytest.raises(N.MblsError):                       # an item larger than an empty round (keys)
        cut([dict(n=2, k=200)], round_keys=100)
    with pytest.raises(N.MblsError):                       # ... (message bytes)
        cut([dict(n=2, msg_offsets=[0, 10, 2000])], round_msg_bytes=1000)
    with pytest.raises(N.MblsError):                       # n = 0
        cut([dict(n=0, k=1)])
    with pytest.raises(N.MblsError):                       # a backward offset table
        cut([dict(n=2, pk_offsets=[0, 5, 3])])
    with pytest.raises(N.MblsError):                       # no calls
        cut([])
    with pytest.raises(N.MblsError):                       # zero options
        cut([dict(n=1, k=1)], round_items=0)
    lib = N.lib()
    o = N.StreamOpts(R, R, R, 1, 1)
    shp = N.StreamCallShape(); shp.n = 1
    cnt = C.c_uint64(0)
    assert lib.mbls_stream_cut(None, C.byref(shp), 1, None, 0, C.byref(cnt)) == N.ERR_ARGUMENT
    assert lib.mbls_stream_cut(C.byref(o), None, 1, None, 0, C.byref(cnt)) == N.ERR_ARGUMENT
    assert lib.mbls_stream_cut(C.byref(o), C.byref(shp), 1, None, 0, None) == N.ERR_ARGUMENT
    assert lib.mbls_stream_cut(C.byref(o), C.byref(shp), 1, None, 0, C.byref(cnt)) == N.OK and cnt.value == 1
    two = (N.StreamCallShape * 2)(); two[0].n = two[1].n = 1; two[0].flush_after = 1
    out = (N.StreamPiece * 1)()
    assert lib.mbls_stream_cut(C.byref(o), two, 2, out, 1, C.byref(cnt)) == N.ERR_ARGUMENT and cnt.value == 2    # more pieces than room


def test_stream_entries_refuse_null_handles():
    lib = N.lib()
    t = C.c_uint64(0)
    assert lib.mbls_stream_create(None, 0, 1, None, None, None) == N.ERR_ARGUMENT
    assert lib.mbls_stream_submit(None, None, None, 0, None, None, None, None, 1, 1, None, None, C.byref(t)) == N.ERR_ARGUMENT
    assert lib.mbls_stream_wait(None, 1) == N.ERR_ARGUMENT and lib.mbls_stream_query(None, 1) == N.ERR_ARGUMENT
    assert lib.mbls_stream_flush(None) == N.ERR_ARGUMENT and lib.mbls_stream_get_stats(None, None) == N.ERR_ARGUMENT
    lib.mbls_stream_destroy(None)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stream") / "libstream_harness.so")
    cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(helpers.ROOT, "tests", "host_emul", "mbls_stream_harness.cpp")])
    h = C.CDLL(so)
    h.harness_scatter_bits.restype = C.c_uint64
    h.harness_scatter_bits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    h.harness_layout.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return h


def test_scatter_bit_arithmetic(harness):
    """every call offset mod 64, round offset mod 64 and piece length 1..130: the piece's bits land at call bits [first, first + len), bits outside
    stay as they were, and exactly the words entirely inside the piece are stored whole"""
    rnd = random.Random(3)
    vals = [rnd.choice([0, 1, 1, 2]) for _ in range(512)]                 # result bytes: any nonzero byte is an accept
    res = (C.c_uint8 * 512)(*vals)
    bits = "".join("1" if v else "0" for v in vals)
    WORDS = 6
    for cf in range(64):
        call_first = 64 + cf
        for rf in range(64):
            for ln in range(1, 131):
                before = rnd.getrandbits(64 * WORDS)
                bm = (C.c_uint64 * WORDS).from_buffer_copy(before.to_bytes(8 * WORDS, "little"))
                whole = harness.harness_scatter_bits(res, rf, call_first, ln, bm)
                piece = int(bits[rf:rf + ln][::-1], 2) << call_first
                lo_w, hi_w = -(-call_first // 64), (call_first + ln) // 64       # the words entirely inside the piece
                n_whole = max(0, hi_w - lo_w)
                mask = ((1 << (64 * n_whole)) - 1) << (64 * lo_w) if n_whole else 0
                want = (before & ~mask) | piece
                assert int.from_bytes(bytes(bm), "little") == want, (cf, rf, ln)
                assert whole == n_whole, (cf, rf, ln)


def test_round_layout_decision(harness):
    def layout(shapes):
        arr = (N.StreamCallShape * len(shapes))()
        keep = []
        for i, s in enumerate(shapes):
            arr[i].n, arr[i].k, arr[i].msg_len = 1, s.get("k", 0), s.get("msg_len", 0)
            if "pk_offsets" in s:
                a = (C.c_uint32 * 2)(0, 1); keep.append(a); arr[i].pk_offsets = C.cast(a, N.u32p)
            if "msg_offsets" in s:
                a = (C.c_uint64 * 2)(0, 1); keep.append(a); arr[i].msg_offsets = C.cast(a, N.u64p)
        ku, mu = C.c_int(), C.c_int()
        harness.harness_layout(arr, len(shapes), C.byref(ku), C.byref(mu))
        return ku.value, mu.value
    assert layout([dict(k=128, msg_len=32)] * 3) == (1, 1)                                   # the uniform layout: no offset tables
    assert layout([dict(k=128, msg_len=32), dict(k=3, msg_len=32)]) == (0, 1)               # k differs: ragged key table
    assert layout([dict(k=128, msg_len=32), dict(k=128, msg_len=31)]) == (1, 0)             # msg_len differs: ragged message table
    assert layout([dict(k=128, msg_len=32), dict(k=128, msg_len=32, pk_offsets=1)]) == (0, 1)
    assert layout([dict(k=128, msg_len=32, msg_offsets=1), dict(k=128, msg_len=32)]) == (1, 0)
    assert layout([dict(k=1, msg_len=32, msg_offsets=1, pk_offsets=1)]) == (0, 0)
