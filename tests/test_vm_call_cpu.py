"""The description of a verify_multiple call without a GPU (milagro_bls_amd/csrc/mbls_vmd.h through tests/batch_emul/mbls_vmd_harness.cpp): every maker is applied to
a description whose every field is already set, and every field is read back -- the maker writes what it is given, clears what its kind excludes and leaves the rest
alone. Each key kind excludes the others: exactly one of apks / wire / table / committee / span is what vm_key_kind, verify_multiple_impl's dispatch, sees, and it
asks in the order span, committee, table, wire, apks."""
import ctypes as C
import os
import subprocess

import pytest

import helpers

VD = ("sigs", "apks", "k", "rands", "n", "result", "status_or", "partial", "locate", "set_results", "set_status", "boff", "spb", "B", "longest", "max_groups", "sigs_resident",
      "hash_enqueued", "mt", "named")
KS = ("pks", "fmt", "key_off", "recs", "tsize", "key_idx", "indexed", "keytab", "committee", "crecs", "ccount", "members", "cmax", "cmt_idx", "bits", "bits_stride", "cmt",
      "span", "cmt_ids", "n_cmt_ids", "span_off")
MS = ("msg_kind", "msgs", "msg_len", "msg_off", "msg_idx", "n_msgs", "list", "tab", "tstride", "flags")
VH = ("sigs", "apks", "hc", "mt", "rands", "draw", "user", "n", "boff", "spb", "B", "result", "status", "locate", "set_results", "set_status")
BOOLS = ("locate", "sigs_resident", "hash_enqueued", "indexed", "committee", "span")
PER_ITEM, LIST, TABLE = 0, 1, 2
SPAN, COMMITTEE, KEYTABLE, WIRE, APKS = range(5)
(KEYS_APKS, KEYS_WIRE, KEYS_IN_TABLE, KEYS_IN_COMMITTEES, KEYS_IN_SPAN, MSGS, MSGS_IN, OUT, OUT_PARTIAL, OUT_SETS, BATCHES, COUNTED, SECOND_HALF) = range(13)
(H_KEYS_APKS, H_KEYS, H_MSGS, H_MSGS_IN, H_SCALARS, H_SOURCE, H_BATCHES, H_OUT, H_OUT_SETS) = range(9)
NO_KEYS = dict.fromkeys(KS, 0); NO_KEYS["fmt"] = 1            # a default keysrc: MBLS_PK_UNCOMPRESSED, everything else null
NO_MSGS = dict.fromkeys(MS, 0)


class Call(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in VD + KS + MS]


class Host(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in VH + MS]


@pytest.fixture(scope="module")
def vd():
    d = os.path.join(helpers.ROOT, "tests", "batch_emul")
    so = os.path.join(d, "libmbls_vmd_harness.so")
    csrc = os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc")
    src = [os.path.join(d, "mbls_vmd_harness.cpp"), os.path.join(csrc, "mbls_vmd.h"), os.path.join(csrc, "mbls_batch.h"), os.path.join(helpers.ROOT, "include", "mbls.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src[0]])
    lib = C.CDLL(so)
    lib.vd_sets.argtypes = [C.c_uint64] * 3 + [C.c_void_p]; lib.vd_sets.restype = None
    lib.vd_apply.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]; lib.vd_apply.restype = None
    lib.vd_key_kind.argtypes = [C.c_void_p]; lib.vd_key_kind.restype = C.c_int
    lib.vh_sets.argtypes = [C.c_uint64] * 2 + [C.c_void_p]; lib.vh_sets.restype = None
    lib.vh_apply.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]; lib.vh_apply.restype = None
    return lib


def full(fields):
    """every field set, every value its own (flags: 1; the format and the message kind: valid ones)"""
    v = {f: 1 if f in BOOLS else 0x1000 * (i + 3) for i, f in enumerate(fields)}
    if "fmt" in v:
        v["fmt"] = 0
    v["msg_kind"] = LIST
    return v


def apply(lib, fn, cls, v, op, *args):
    a = (C.c_uint64 * 8)(*args)
    out = cls()
    fn(C.byref(cls(**v)), op, a, C.byref(out))
    return {f: getattr(out, f) for f, _ in cls._fields_}


def check(got, base, **changed):
    want = dict(base); want.update(changed)
    assert got == want, {f: (hex(got[f]), hex(want[f])) for f in want if got[f] != want[f]}


def test_a_call_starts_from_its_sets_alone(vd):
    out = Call()
    vd.vd_sets(0xA0, 0xB0, 77, C.byref(out))
    want = dict.fromkeys(VD + KS + MS, 0); want.update(sigs=0xA0, rands=0xB0, n=77, fmt=1)
    assert {f: getattr(out, f) for f in want} == want
    out = Host()
    vd.vh_sets(0xA0, 77, C.byref(out))
    want = dict.fromkeys(VH + MS, 0); want.update(sigs=0xA0, n=77)
    assert {f: getattr(out, f) for f in want} == want


def test_every_maker_of_the_call_field_by_field(vd):
    F = full(VD + KS + MS)
    ap = lambda op, *a: apply(vd, vd.vd_apply, Call, F, op, *a)
    # the keys: each kind clears every other
    check(ap(KEYS_APKS, 0xAA0), F, apks=0xAA0, k=0, **NO_KEYS)
    check(ap(KEYS_WIRE, 0xAA0, 0, 0xBB0, 5), F, apks=0, k=5, **dict(NO_KEYS, pks=0xAA0, fmt=0, key_off=0xBB0))
    check(ap(KEYS_IN_TABLE, 0xAA0, 0xBB0, 0xCC0, 5), F, apks=0, k=5, **dict(NO_KEYS, indexed=1, keytab=0xAA0, key_idx=0xBB0, key_off=0xCC0))
    check(ap(KEYS_IN_COMMITTEES, 0xAA0, 0xBB0, 0xCC0, 64), F, apks=0, k=0, **dict(NO_KEYS, indexed=1, committee=1, cmt=0xAA0, cmt_idx=0xBB0, bits=0xCC0, bits_stride=64))
    check(ap(KEYS_IN_SPAN, 0xAA0, 0xBB0, 9, 0xCC0, 0xDD0, 64), F, apks=0, k=0,
          **dict(NO_KEYS, indexed=1, committee=1, span=1, cmt=0xAA0, cmt_ids=0xBB0, n_cmt_ids=9, span_off=0xCC0, bits=0xDD0, bits_stride=64))
    # the messages: a source of mbls_batch.h as it is (no table handle, no count of named entries), or the resident table by handle
    check(ap(MSGS, PER_ITEM, 0xAA0, 32, 0xBB0), F, mt=0, named=0, **dict(NO_MSGS, msg_kind=PER_ITEM, msgs=0xAA0, msg_len=32, msg_off=0xBB0))
    check(ap(MSGS, LIST, 0xAA0, 32, 0xBB0, 6, 0xCC0), F, mt=0, named=0, **dict(NO_MSGS, msg_kind=LIST, msgs=0xAA0, msg_len=32, msg_off=0xBB0, n_msgs=6, msg_idx=0xCC0))
    check(ap(MSGS_IN, 0xAA0, 0xBB0, 4), F, mt=0xAA0, named=4, **dict(NO_MSGS, msg_kind=TABLE, msg_idx=0xBB0))
    # the outputs: the call's byte and word or the shard's record, never both; the sets' answers switch locate mode on
    check(ap(OUT, 0xAA0, 0xBB0), F, result=0xAA0, status_or=0xBB0, partial=0)
    check(ap(OUT_PARTIAL, 0xAA0), F, result=0, status_or=0, partial=0xAA0)
    check(apply(vd, vd.vd_apply, Call, dict(F, locate=0), OUT_SETS, 0xAA0, 0xBB0), F, locate=1, set_results=0xAA0, set_status=0xBB0)
    check(apply(vd, vd.vd_apply, Call, dict(F, locate=0), OUT_SETS, 0, 0), F, locate=1, set_results=0, set_status=0)           # (a null pointer is the entry's to refuse: the mode stays asked for)
    # the batches, the host's count, the second half of an _rng call
    check(ap(BATCHES, 0xAA0, 3, 4, 11), F, boff=0xAA0, spb=3, B=4, max_groups=11)
    check(ap(COUNTED, 9), F, longest=9)
    check(apply(vd, vd.vd_apply, Call, dict(F, sigs_resident=0, hash_enqueued=0), SECOND_HALF, 0xAA0, 1), F, sigs=0, rands=0xAA0, sigs_resident=1, hash_enqueued=1)
    check(ap(SECOND_HALF, 0xAA0, 0), F, sigs=0, rands=0xAA0, sigs_resident=1, hash_enqueued=0)


def test_every_maker_of_the_host_form_field_by_field(vd):
    F = full(VH + MS)
    ap = lambda op, *a: apply(vd, vd.vh_apply, Host, F, op, *a)
    check(ap(H_KEYS_APKS, 0xAA0), F, apks=0xAA0, hc=0)
    check(ap(H_KEYS, 0xAA0), F, apks=0, hc=0xAA0)
    check(ap(H_MSGS, PER_ITEM, 0xAA0, 32, 0xBB0), F, mt=0, **dict(NO_MSGS, msg_kind=PER_ITEM, msgs=0xAA0, msg_len=32, msg_off=0xBB0))
    check(ap(H_MSGS, LIST, 0xAA0, 32, 0xBB0, 6, 0xCC0), F, mt=0, **dict(NO_MSGS, msg_kind=LIST, msgs=0xAA0, msg_len=32, msg_off=0xBB0, n_msgs=6, msg_idx=0xCC0))
    check(ap(H_MSGS_IN, 0xAA0, 0xBB0), F, mt=0xAA0, **dict(NO_MSGS, msg_kind=TABLE, msg_idx=0xBB0))
    check(ap(H_SCALARS, 0xAA0), F, rands=0xAA0, draw=0, user=0)
    check(ap(H_SOURCE, 0xAA0, 0xBB0), F, rands=0, draw=0xAA0, user=0xBB0)
    check(ap(H_BATCHES, 0xAA0, 3, 4), F, boff=0xAA0, spb=3, B=4)
    check(ap(H_OUT, 0xAA0, 0xBB0), F, result=0xAA0, status=0xBB0)
    check(apply(vd, vd.vh_apply, Host, dict(F, locate=0), H_OUT_SETS, 0xAA0, 0xBB0), F, locate=1, set_results=0xAA0, set_status=0xBB0)


def test_each_key_kind_excludes_the_others(vd):
    """whatever kind stood before, after a keys maker exactly that kind stands: the dispatch sees it, and the other kinds' marks are gone"""
    makers = {APKS: (KEYS_APKS, 0xAA0), WIRE: (KEYS_WIRE, 0xAA0, 1, 0, 3), KEYTABLE: (KEYS_IN_TABLE, 0xAA0, 0xBB0, 0, 3),
              COMMITTEE: (KEYS_IN_COMMITTEES, 0xAA0, 0xBB0, 0xCC0, 64), SPAN: (KEYS_IN_SPAN, 0xAA0, 0xBB0, 9, 0xCC0, 0xDD0, 64)}
    start = Call(); vd.vd_sets(0xA0, 0xB0, 12, C.byref(start))
    v0 = {f: getattr(start, f) for f, _ in Call._fields_}
    for first, m1 in makers.items():
        v1 = apply(vd, vd.vd_apply, Call, v0, *m1)
        assert vd.vd_key_kind(C.byref(Call(**v1))) == first
        for second, m2 in makers.items():
            v2 = apply(vd, vd.vd_apply, Call, v1, *m2)
            assert vd.vd_key_kind(C.byref(Call(**v2))) == second, (first, second)
            marks = {APKS: bool(v2["apks"]), WIRE: bool(v2["pks"]), KEYTABLE: bool(v2["indexed"]) and not v2["committee"], COMMITTEE: bool(v2["committee"]) and not v2["span"],
                     SPAN: bool(v2["span"])}
            assert [k for k, on in marks.items() if on] == [second], (first, second, marks)
            assert v2 == apply(vd, vd.vd_apply, Call, v0, *m2), (first, second)        # ... and nothing of the first kind is left anywhere


def test_the_dispatch_order(vd):
    """span, committee, table, wire, apks: with several marks standing (no maker leaves such a description) the earlier one in that order wins"""
    base = dict.fromkeys(VD + KS + MS, 0)
    kind = lambda **kw: vd.vd_key_kind(C.byref(Call(**dict(base, **kw))))
    assert kind(span=1, committee=1, indexed=1, pks=8, apks=8) == SPAN
    assert kind(committee=1, indexed=1, pks=8, apks=8) == COMMITTEE
    assert kind(indexed=1, pks=8, apks=8) == KEYTABLE
    assert kind(pks=8) == WIRE and kind() == WIRE              # no aggregate points: wire keys (an entry refuses the null buffer)
    assert kind(apks=8) == APKS and kind(apks=8, pks=8) == APKS
    assert kind(span=1) == SPAN and kind(committee=1) == COMMITTEE and kind(indexed=1) == KEYTABLE
