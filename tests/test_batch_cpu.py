"""The batch description of the per-item verification entries without a GPU (milagro_bls_amd/csrc/mbls_batch.h through tests/batch_emul/mbls_batch_harness.cpp):
`slice(batch, lo, hi)` is the one place that knows how each pointer advances when a pass starts at item lo. Every pointer and count it returns is compared with
the rule written out here: signatures advance by 96 lo, results and status words by lo, the bitmap by lo / 64 words; an offset table advances by lo and its base
stays; otherwise wire keys advance by unit k lo and key indices by k lo, uniform messages by msg_len lo; message indices advance by lo while the list or table
they name stays, and a slice never hashes a list; null stays null."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import helpers

N, K = 256, 3
FIELDS = ("sigs", "results", "bitmap", "status", "n", "k", "mode", "keys_indexed", "pks", "fmt", "key_off", "recs", "tsize", "key_idx", "keytab",
          "msg_kind", "msgs", "msg_len", "msg_off", "msg_idx", "n_msgs", "list", "tab", "tstride", "flags")
PER_ITEM, LIST, TABLE = 0, 1, 2


class Flat(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in FIELDS]


@pytest.fixture(scope="module")
def bt():
    d = os.path.join(helpers.ROOT, "tests", "batch_emul")
    so = os.path.join(d, "libmbls_batch_harness.so")
    src = [os.path.join(d, "mbls_batch_harness.cpp"), os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc", "mbls_batch.h"), os.path.join(helpers.ROOT, "include", "mbls.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        cxx = os.environ.get("MBLS_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src[0]])
    lib = C.CDLL(so)
    lib.bt_whole.argtypes = [C.c_void_p, C.c_void_p]
    lib.bt_slice.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.bt_slice_of_slice.argtypes = [C.c_void_p] + [C.c_uint64] * 4 + [C.c_void_p]
    return lib


# addresses far apart, each aligned for what it points to; nothing is dereferenced
A = {f: 0x10000000 * (i + 1) for i, f in enumerate(("sigs", "results", "bitmap", "status", "pks", "key_off", "recs", "key_idx", "keytab", "msgs", "msg_off", "msg_idx",
                                                      "list", "tab", "flags"))}
KEYS = {
    "wire48": dict(keys_indexed=0, pks=A["pks"], fmt=0),
    "wire96": dict(keys_indexed=0, pks=A["pks"], fmt=1),
    "wire_ragged": dict(keys_indexed=0, pks=A["pks"], fmt=0, key_off=A["key_off"]),
    "wire_not_uploaded": dict(keys_indexed=0, pks=0, fmt=1),
    "table": dict(keys_indexed=1, fmt=1, recs=A["recs"], tsize=1000, key_idx=A["key_idx"], keytab=A["keytab"]),
    "table_ragged": dict(keys_indexed=1, fmt=1, recs=A["recs"], tsize=1000, key_idx=A["key_idx"], keytab=A["keytab"], key_off=A["key_off"]),
    "table_not_uploaded": dict(keys_indexed=1, fmt=1, recs=A["recs"], tsize=1000, key_idx=0, keytab=A["keytab"]),
}
MSGS = {
    "uniform": dict(msg_kind=PER_ITEM, msgs=A["msgs"], msg_len=32),
    "ragged": dict(msg_kind=PER_ITEM, msgs=A["msgs"], msg_len=32, msg_off=A["msg_off"]),
    "empty": dict(msg_kind=PER_ITEM, msgs=0, msg_len=0),
    "list": dict(msg_kind=LIST, msgs=A["msgs"], msg_len=32, msg_idx=A["msg_idx"], n_msgs=5, list=A["list"], tab=A["tab"], tstride=6, flags=A["flags"]),
    "list_ragged": dict(msg_kind=LIST, msgs=A["msgs"], msg_off=A["msg_off"], msg_idx=A["msg_idx"], n_msgs=5, tab=A["tab"], tstride=6, flags=A["flags"]),
    "table": dict(msg_kind=TABLE, msg_idx=A["msg_idx"], n_msgs=70, tab=A["tab"], tstride=1025, flags=A["flags"]),
}
CASES = [(kn, mn, bm, st) for kn in KEYS for mn in MSGS for bm in (True, False) for st in (True, False)]
CUTS = [(lo, hi) for lo in (0, 64, 192) for hi in (lo + 1, N)]


def whole(kn, mn, bm, st):
    v = dict.fromkeys(FIELDS, 0)
    v.update(sigs=A["sigs"], results=A["results"], bitmap=A["bitmap"] if bm else 0, status=A["status"] if st else 0, n=N, k=K, mode=1)
    v.update(KEYS[kn]); v.update(MSGS[mn])
    return v


def want_slice(w, lo, hi):
    """the rule, field by field (addresses in bytes)"""
    s = dict(w)
    s["n"] = hi - lo
    s["sigs"] = w["sigs"] + 96 * lo
    s["results"] = w["results"] + lo
    s["bitmap"] = w["bitmap"] + 8 * (lo // 64) if w["bitmap"] else 0
    s["status"] = w["status"] + 4 * lo if w["status"] else 0
    if w["key_off"]:
        s["key_off"] = w["key_off"] + 4 * lo
    else:
        unit = 48 if w["fmt"] == 0 else 96
        s["pks"] = w["pks"] + unit * w["k"] * lo if w["pks"] else 0
        s["key_idx"] = w["key_idx"] + 4 * w["k"] * lo if w["key_idx"] else 0
    if w["msg_kind"] != PER_ITEM:
        s["msg_idx"] = w["msg_idx"] + 4 * lo
        s["list"] = 0
    elif w["msg_off"]:
        s["msg_off"] = w["msg_off"] + 8 * lo
    elif w["msgs"]:
        s["msgs"] = w["msgs"] + w["msg_len"] * lo
    return s


def flat(v):
    return Flat(**v)


def unflat(f):
    return {name: getattr(f, name) for name in FIELDS}


def test_the_makers_fill_what_they_are_given(bt):
    for kn, mn in itertools.product(KEYS, MSGS):
        w = whole(kn, mn, True, True)
        out = Flat()
        bt.bt_whole(C.byref(flat(w)), C.byref(out))
        assert unflat(out) == w, (kn, mn)


@pytest.mark.parametrize("lo,hi", CUTS)
def test_slice_against_the_rule(bt, lo, hi):
    for kn, mn, bm, st in CASES:
        w = whole(kn, mn, bm, st)
        out = Flat()
        bt.bt_slice(C.byref(flat(w)), lo, hi, C.byref(out))
        got, want = unflat(out), want_slice(w, lo, hi)
        assert got == want, (kn, mn, bm, st, {f: (hex(got[f]), hex(want[f])) for f in FIELDS if got[f] != want[f]})


def test_null_key_pointers_stay_null_and_tables_stay_put(bt):
    for kn, mn in itertools.product(KEYS, MSGS):
        w = whole(kn, mn, True, True)
        out = Flat()
        bt.bt_slice(C.byref(flat(w)), 64, N, C.byref(out))
        got = unflat(out)
        if kn.endswith("not_uploaded"):
            assert got["pks"] == 0 and got["key_idx"] == 0
        if w["key_off"]:
            assert (got["pks"], got["key_idx"]) == (w["pks"], w["key_idx"])
        for f in ("recs", "tsize", "keytab", "tab", "tstride", "flags", "n_msgs", "k", "mode", "fmt", "msg_len", "msg_kind", "keys_indexed"):
            assert got[f] == w[f], (kn, mn, f)
        if mn.startswith("list"):
            assert (got["msgs"], got["msg_off"]) == (w["msgs"], w["msg_off"]) and got["list"] == 0
        if mn == "empty":
            assert got["msgs"] == 0


def test_a_slice_of_a_slice_is_the_slice_of_the_sum(bt):
    for kn, mn, bm, st in CASES:
        w = flat(whole(kn, mn, bm, st))
        a, b = Flat(), Flat()
        bt.bt_slice_of_slice(C.byref(w), 64, 256, 64, 128, C.byref(a))
        bt.bt_slice(C.byref(w), 128, 192, C.byref(b))
        assert unflat(a) == unflat(b), (kn, mn, bm, st)
