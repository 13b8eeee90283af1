"""GPU tests of mbls_verify_multiple_committee_msgtable[_locate]_device / _rng (include/mbls.h, "verify_multiple OVER COMMITTEE BITFIELDS AND THE RESIDENT MESSAGE
TABLE"). The world is the one tests/test_gpu_committee.py builds once per session (136 key-table entries -- honest keys, the negative of key 0, an invalid record,
infinity, a point outside G1 --, committees of 1 .. 129 members and the special ones, 3 table messages), with one signature per (key, message) for the single-key
sets. Every call mixes committee sets with single-key sets and is compared with mbls_verify_multiple_sets_indexed_msgtable[_locate]_device on the same signatures,
scalars and message indices with every set's signers spelled out in member order through a ragged offset table: result byte, status word, and for the _locate
forms every set byte and word, under the 3 x 3 modes of mbls_ctx_set_vm_grouping and mbls_ctx_set_committee_route. Ground truth that does not lean on the
baseline: an all-valid call answers 1, and with one participation bit flipped in set j it answers 0 and the locate form reads 0 at j and 1 elsewhere."""
import ctypes as C
import random

import pytest

import test_gpu_committee as TC

pytestmark = pytest.mark.gpu

SINGLE = 0x80000000
BAD_SIG, NOT_G2, BAD_PK, APK_INF, NO_KEYS, PK_INF, PAIRING, BAD_SCALAR, BAD_MSG = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x100
STRIDE = TC.STRIDE
GROUPINGS = (0, 1, 2)
ROUTES = (0, 1, 2)
COUNTS = (1, 2, 3, 63, 64, 65, 200)
# the pool's committee items that verify: every set of an all-valid call is one of these or a single-key set
VALID_TAGS = ("first", "last", "everybody", "all_but_first", "all_but_last", "half", "half_plus_one", "doubling_fixup", "ppm_all", "dup_all", "dup_twice",
              "dup_all_but_first", "inf4_all", "inf4_all_but_one", "pm_first", "full_inf_one", "invalid_absent", "infinite_absent", "outside_absent")


class Set:
    """one set of a call: word (committee id, or SINGLE | key index), sel (selected member positions; None: single key), message number, signature, the
    key-table indices the baseline spells out"""
    def __init__(self, word, sel, msg, sig, keys, tag):
        self.word, self.sel, self.msg, self.sig, self.keys, self.tag = word, sel, msg, sig, keys, tag

    def bits(self):
        return TC.bits_of(self.sel) if self.sel is not None else b"\xa5" * STRIDE      # a single-key set's bytes are not read: any value


_P = None


def pool():
    """(valid committee sets, single-key sets, every committee item of the world's pool by tag) built once per session"""
    global _P
    if _P is not None:
        return _P
    from milagro_bls_amd import batch
    w = TC.world()
    as_set = lambda it: Set(it.cid, list(it.sel), it.msg, it.sig, [w.members[it.cid][j] for j in it.sel], it.tag)
    valid = [as_set(it) for it in w.pool if it.tag in VALID_TAGS and it.sel]
    by_tag = {}
    for it in w.pool:
        by_tag.setdefault(it.tag, []).append(as_set(it))
    nk = len(w.sks)                                             # the honest keys and the negative of key 0
    one = batch.sign_batch(b"".join(w.sks[i].to_bytes(32, "big") for _ in range(3) for i in range(nk)), b"".join(w.msgs[j] for j in range(3) for _ in range(nk)), 3 * nk,
                           msg_len=32)
    singles = [Set(SINGLE | k, None, m, one[96 * (m * nk + k):96 * (m * nk + k) + 96], [k], "single") for k in range(nk) for m in range(3)]
    random.Random(5).shuffle(singles)
    _P = (valid, singles, by_tag)
    return _P


def mixed(n, start=0):
    """n valid sets: two of five a single-key set, the others walk the valid committee sets (n = 200: every size and pattern)"""
    valid, singles, _ = pool()
    out, a, b = [], start, 3 * start
    for i in range(n):
        if (i + start) % 5 in (1, 3):
            out.append(singles[b % len(singles)]); b += 1
        else:
            out.append(valid[a % len(valid)]); a += 1
    return out


def scalars(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, 1 << 63) for _ in range(n)]


def i64(vals):
    import torch
    return torch.tensor(vals or [0], dtype=torch.int64, device="cuda:0")


def outputs(n):
    import torch
    return (torch.full((1,), 9, dtype=torch.uint8, device="cuda:0"), torch.full((1,), 0x7fffffff, dtype=torch.int32, device="cuda:0"),
            torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda:0"), torch.full((max(n, 1),), 0x7fffffff, dtype=torch.int32, device="cuda:0"))


def read(n, o, locate):
    import torch
    torch.cuda.synchronize()
    res, st = int(o[0].cpu()[0]), int(o[1].cpu()[0]) & 0xffffffff
    if not locate:
        return res, st
    return res, st, o[2].cpu().tolist()[:n], [x & 0xffffffff for x in o[3].cpu().tolist()[:n]]


def buffers_new(sets, rands, words=None, bits=None, midx=None, sigs=None):
    """the device buffers of a call of the new entry"""
    d_s = TC.dev(b"".join(sigs if sigs is not None else [s.sig for s in sets]))
    d_ci = TC.i32(words if words is not None else [s.word for s in sets])
    d_b = TC.dev(bits if bits is not None else b"".join(s.bits() for s in sets))
    d_mi = TC.i32(midx if midx is not None else [s.msg for s in sets]); d_r = i64(rands)
    return d_s, d_ci, d_b, d_mi, d_r, outputs(len(sets))


def call_new(sets, rands, locate, ct=None, stream=None, buffers=None, **kw):
    from milagro_bls_amd import _native as N
    w = TC.world(); ctx = N.default_context(); L = N.lib(); n = len(sets)
    d_s, d_ci, d_b, d_mi, d_r, o = buffers if buffers is not None else buffers_new(sets, rands, **kw)
    cth = (ct or w.ct).handle
    if locate:
        ctx.check(L.mbls_verify_multiple_committee_msgtable_locate_device(ctx.handle, cth, d_s.data_ptr(), d_ci.data_ptr(), d_b.data_ptr(), STRIDE, w.mt.handle, d_mi.data_ptr(),
                                                                          d_r.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), stream))
    else:
        ctx.check(L.mbls_verify_multiple_committee_msgtable_device(ctx.handle, cth, d_s.data_ptr(), d_ci.data_ptr(), d_b.data_ptr(), STRIDE, w.mt.handle, d_mi.data_ptr(),
                                                                   d_r.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), stream))
    return read(n, o, locate)


def call_base(sets, rands, locate, lists=None, midx=None, sigs=None):
    """the indexed entry on the spelled-out signers (`lists`: where the test changed a word or a field)"""
    from milagro_bls_amd import _native as N
    w = TC.world(); ctx = N.default_context(); L = N.lib(); n = len(sets)
    lists = lists if lists is not None else [s.keys for s in sets]
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    d_s = TC.dev(b"".join(sigs if sigs is not None else [s.sig for s in sets]))
    d_k = TC.i32([x for l in lists for x in l]); d_o = TC.i32(off)
    d_mi = TC.i32(midx if midx is not None else [s.msg for s in sets]); d_r = i64(rands)
    o = outputs(n)
    if locate:
        ctx.check(L.mbls_verify_multiple_sets_indexed_msgtable_locate_device(ctx.handle, w.kt.handle, d_s.data_ptr(), d_k.data_ptr(), d_o.data_ptr(), 0, w.mt.handle,
                                                                             d_mi.data_ptr(), d_r.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                                                                             None))
    else:
        ctx.check(L.mbls_verify_multiple_sets_indexed_msgtable_device(ctx.handle, w.kt.handle, d_s.data_ptr(), d_k.data_ptr(), d_o.data_ptr(), 0, w.mt.handle, d_mi.data_ptr(),
                                                                      d_r.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), None))
    return read(n, o, locate)


@pytest.fixture(autouse=True)
def _modes_back():
    yield
    from milagro_bls_amd import batch, _native as N
    N.default_context().set_committee_route(0)
    batch.set_vm_grouping(0)


def compare(sets, rands, lists=None, groupings=GROUPINGS, routes=ROUTES, **kw):
    """both forms of the new entry under every grouping x route mode against both forms of the baseline under the same grouping mode (the baseline knows no
    route) -> the locate form's (result, status, set results, set status), equal in every mode of one grouping and returned for grouping 0"""
    from milagro_bls_amd import batch, _native as N
    base_kw = {k: v for k, v in kw.items() if k in ("midx", "sigs")}
    out = None
    for g in groupings:
        batch.set_vm_grouping(g)
        b0 = call_base(sets, rands, False, lists=lists, **base_kw)
        b1 = call_base(sets, rands, True, lists=lists, **base_kw)
        assert b1[:2] == b0
        for r in routes:
            N.default_context().set_committee_route(r)
            n0 = call_new(sets, rands, False, **kw)
            n1 = call_new(sets, rands, True, **kw)
            assert n0 == b0, (g, r, n0, b0)
            assert n1[:2] == b1[:2], (g, r, n1[:2], b1[:2])
            bad = [(i, sets[i].tag, n1[2][i], b1[2][i], hex(n1[3][i]), hex(b1[3][i])) for i in range(len(sets)) if (n1[2][i], n1[3][i]) != (b1[2][i], b1[3][i])]
            assert not bad, (g, r, bad[:8])
        N.default_context().set_committee_route(0)
        if g == 0:
            out = b1
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_all_valid_calls_answer_one_and_equal_the_indexed_entry(n):
    sets = mixed(n, start=n)
    assert n < 3 or ({s.sel is None for s in sets} == {True, False})
    res, st, sres, sst = compare(sets, scalars(n, n))
    assert res == 1 and st == 0 and sres == [1] * n and sst == [0] * n


def test_the_largest_call_holds_every_size_and_pattern():
    sets = mixed(200, start=200)
    valid, _s, _t = pool()
    assert {(s.word, s.tag) for s in sets if s.sel is not None} == {(s.word, s.tag) for s in valid}
    assert {len(TC.world().members[s.word]) for s in sets if s.sel is not None} >= set(TC.SIZES)


@pytest.mark.parametrize("n", COUNTS)
def test_one_flipped_participation_bit_rejects_the_call_and_names_the_set(n):
    """one bit of one committee set flipped against its signers -- a signer dropped, or a non-signer added: the call answers 0, the locate form reads 0 at that
    set and 1 elsewhere, whatever the grouping and the route; and the indexed entry on the flipped list says the same"""
    w = TC.world()
    sets = list(mixed(n, start=n))
    cand = [i for i, s in enumerate(sets) if s.sel is not None and s.word < len(TC.SIZES) and len(w.members[s.word]) >= 2]      # (the committees of distinct honest keys)
    if not cand:                                                 # the smallest calls: put a larger honest committee set first
        valid, _s, _t = pool()
        sets[0] = next(s for s in valid if s.word < len(TC.SIZES) and len(w.members[s.word]) >= 31)
        cand = [0]
    j = cand[len(cand) // 2]
    s = sets[j]; m = len(w.members[s.word])
    flip = (m - 1) if n % 2 else 0
    sel = sorted(set(s.sel) ^ {flip})
    if not sel:                                                  # (never an empty field here: that is a kind of its own below)
        flip = 1; sel = sorted(set(s.sel) ^ {flip})
    bits = b"".join(TC.bits_of(sel) if i == j else x.bits() for i, x in enumerate(sets))
    lists = [[w.members[s.word][t] for t in sel] if i == j else x.keys for i, x in enumerate(sets)]
    res, st, sres, sst = compare(sets, scalars(n, 100 + n), lists=lists, bits=bits)
    assert res == 0 and st == 0
    assert sres == [0 if i == j else 1 for i in range(n)] and sst == [PAIRING if i == j else 0 for i in range(n)]


def faulty(kind, probe):
    """a 65-set call with the faulty kind planted -> (sets, rands, kwargs of the new entry, the baseline's lists, the positions that must read 0 -- None: as the
    baseline says --, status bits the call's word must hold)"""
    w = TC.world()
    _v, _s, by_tag = pool()
    n = 65
    sets = list(mixed(n, start=17)); rands = scalars(n, 900)
    kw, bad, bits_or = {}, None, 0
    com = [i for i, s in enumerate(sets) if s.sel is not None]
    p, q, r = com[1], com[len(com) // 2], com[-1]
    plant = lambda i, tag, k=-1: sets.__setitem__(i, by_tag[tag][k])
    if kind == "empty_bitfield":
        plant(p, "nobody", 7); bad = [p]
    elif kind == "sum_at_infinity":
        # P - P under the signature of another set: the key is the point at infinity, the signature is not. (The pool's own signatures over such subsets are the
        # point at infinity themselves -- key and signature both infinite: the set contributes 1 and reads 1, here as in the indexed entry.)
        sg = next(s for s in sets if s.sel is None)
        for i, tag in ((p, "p_minus_p"), (q, "inf4_pm"), (r, "full_inf_all")):
            t = by_tag[tag][-1]
            sets[i] = Set(t.word, t.sel, t.msg, sg.sig, t.keys, tag)
        plant(com[0], "ppm_inf_subset"); bad = [p, q, r]
    elif kind == "invalid_member":
        plant(p, "invalid_selected"); plant(q, "invalid_absent"); bad = [p]; bits_or = BAD_PK
    elif kind == "infinite_member":
        plant(p, "infinite_selected"); plant(q, "infinite_absent"); plant(r, "infinite_alone"); bad = [r]; bits_or = PK_INF
    elif kind == "outside_member":
        plant(p, "outside_selected"); plant(q, "outside_absent"); bad = [p]
    elif kind == "committee_id_at_the_count":
        words = [s.word for s in sets]; words[p] = len(w.members); words[q] = 0x7FFFFFFF
        kw["words"] = words; bad = [p, q]; bits_or = BAD_PK
    elif kind == "single_key_index_at_the_table_size":
        sg = [i for i, s in enumerate(sets) if s.sel is None]
        words = [s.word for s in sets]; words[sg[0]] = SINGLE | len(w.pk96); words[sg[-1]] = 0xFFFFFFFF
        kw["words"] = words; bad = [sg[0], sg[-1]]; bits_or = BAD_PK
    elif kind == "message_index_at_the_table_size":
        midx = [s.msg for s in sets]; midx[p] = len(w.msgs); midx[com[0] + 1] = 0xFFFFFFFF
        kw["midx"] = midx; bad = [p, com[0] + 1]; bits_or = BAD_MSG
    elif kind == "zero_scalar":
        rands[q] = 0; bad = [q]; bits_or = BAD_SCALAR
    elif kind == "signature_outside_g2":
        sigs = [s.sig for s in sets]; sigs[r] = probe
        kw["sigs"] = sigs; bad = [r]; bits_or = NOT_G2
    else:
        raise AssertionError(kind)
    lists = [s.keys for s in sets]
    for i, wd in enumerate(kw.get("words", [])):
        if wd != sets[i].word:
            lists[i] = [wd & 0x7FFFFFFF] if wd & SINGLE else [0xFFFFFFFF]
    return sets, rands, kw, lists, bad, bits_or


KINDS = ("empty_bitfield", "sum_at_infinity", "invalid_member", "infinite_member", "outside_member", "committee_id_at_the_count", "single_key_index_at_the_table_size",
         "message_index_at_the_table_size", "zero_scalar", "signature_outside_g2")


@pytest.mark.parametrize("kind", KINDS)
def test_each_faulty_kind_is_rejected_and_located_as_the_indexed_entry_does(kind, vectors):
    """one call per kind (a flipped bit: the test above): rejected by both entries, the same sets named, the same words -- under the 3 x 3 modes"""
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    sets, rands, kw, lists, bad, bits_or = faulty(kind, probe)
    res, st, sres, sst = compare(sets, rands, lists=lists, **kw)
    assert res == 0 and st & bits_or == bits_or, (res, hex(st))
    assert [i for i in range(len(sets)) if not sres[i]] == sorted(bad), kind
    # verify_multiple's key phase flags neither the empty list nor the sum at infinity (the indexed entries do not): such a set fails its pairing
    assert not st & (NO_KEYS | APK_INF) and not any(x & (NO_KEYS | APK_INF) for x in sst)
    if kind in ("empty_bitfield", "sum_at_infinity", "outside_member"):
        assert all(sst[i] == PAIRING for i in bad)


def test_a_call_behind_an_append_on_another_stream_sees_the_new_committees():
    """the append runs on the context's own stream, the call right behind it on a second one: committees_acquire orders them on the device"""
    import torch
    from milagro_bls_amd import batch, _native as N
    w = TC.world()
    sets = list(mixed(65, start=3)); rands = scalars(65, 31)
    want = call_base(sets, rands, True)
    sb = torch.cuda.Stream()
    for g in (1, 2):
        ct = N.CommitteeTable(w.kt, capacity_hint=2)
        try:
            batch.set_vm_grouping(g)
            buffers = buffers_new(sets, rands)
            torch.cuda.synchronize()
            off = [0]
            for mem in w.members:
                off.append(off[-1] + len(mem))
            assert ct.append([x for mem in w.members for x in mem], off) == 0
            got = call_new(sets, rands, True, ct=ct, stream=sb.cuda_stream, buffers=buffers)
            assert got == want and got[0] == 1, g
        finally:
            batch.set_vm_grouping(0)
            ct.close()


def test_a_pre_reserved_scratch_changes_no_byte():
    from milagro_bls_amd import _native as N
    sets = list(mixed(200, start=9)); rands = scalars(200, 77)
    j = next(i for i, s in enumerate(sets) if s.sel is not None and len(s.sel) > 40)
    bits = b"".join(TC.bits_of(s.sel[1:]) if i == j else s.bits() for i, s in enumerate(sets))
    before = (call_new(sets, rands, True, bits=bits), call_new(sets, rands, False, bits=bits))
    N.default_context().reserve_committee_items(3000, 160)       # more sets and a larger committee than any call so far: both arrays move
    after = (call_new(sets, rands, True, bits=bits), call_new(sets, rands, False, bits=bits))
    assert after == before and before[0][0] == 0 and [i for i in range(200) if not before[0][2][i]] == [j]


def spelled_apks(sets):
    from milagro_bls_amd import batch, _native as N
    w = TC.world()
    off = [0]
    for s in sets:
        off.append(off[-1] + len(s.keys))
    apks, st = batch.aggregate_public_keys_batch(b"".join(w.pk96[x] for s in sets for x in s.keys), len(sets), pk_format=N.PK_UNCOMPRESSED, pk_offsets=off)
    assert not any(st)
    return [apks[96 * i:96 * i + 96] for i in range(len(sets))]


@pytest.mark.parametrize("grouping", GROUPINGS)
def test_rng_entries_draw_as_the_msgtable_entry_does(grouping, vectors):
    """a counting draw: asked for the same counts as mbls_verify_multiple_msgtable_rng on the same signatures with the aggregate keys spelled out -- all n sets;
    the sets in front of a signature outside G2; not at all when set 0's signature fails -- and the same answers; the locate form names the bad set"""
    from milagro_bls_amd import batch
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    w = TC.world()
    n = 24
    sets = [s for s in mixed(n, start=40)]
    rands = scalars(n, 5)
    apks = spelled_apks(sets)
    words = [s.word for s in sets]; bits = b"".join(s.bits() for s in sets); midx = [s.msg for s in sets]
    batch.set_vm_grouping(grouping)
    for where in (None, 5, 0):
        sigs = [s.sig for s in sets]
        if where is not None:
            sigs[where] = probe
        asked_new, asked_old, asked_loc = [], [], []
        draw = lambda log: (lambda count: (log.append(count), rands[:count])[1])
        got = batch.verify_multiple_committee_msgtable_rng(w.ct, w.mt, b"".join(sigs), words, bits, STRIDE, midx, n, draw(asked_new))
        old = batch.verify_multiple_msgtable_rng(w.mt, b"".join(sigs), b"".join(apks), midx, n, draw(asked_old))
        assert asked_new == asked_old == ([n] if where is None else [where] if where else []), (where, asked_new, asked_old)
        assert got == old == (where is None)
        res, sres, sst = batch.verify_multiple_committee_msgtable_locate_rng(w.ct, w.mt, b"".join(sigs), words, bits, STRIDE, midx, n, draw(asked_loc))
        ores, osres, osst = batch.verify_multiple_msgtable_locate_rng(w.mt, b"".join(sigs), b"".join(apks), midx, n, draw([]))
        assert asked_loc == asked_new and (res, sres, sst) == (ores, osres, osst)
        assert sres == [where is None or i < where for i in range(n)]
    # a wrong field on the host path: located
    j = next(i for i, s in enumerate(sets) if s.sel is not None and len(s.sel) > 2)
    wrong = b"".join(TC.bits_of(s.sel[:-1]) if i == j else s.bits() for i, s in enumerate(sets))
    res, sres, sst = batch.verify_multiple_committee_msgtable_locate_rng(w.ct, w.mt, b"".join(s.sig for s in sets), words, wrong, STRIDE, midx, n, lambda c: rands[:c])
    assert res is False and sres == [i != j for i in range(n)] and sst[j] == PAIRING


def test_host_entries_refuse_what_names_nothing_and_device_entries_refuse_bad_arguments():
    from milagro_bls_amd import _native as N
    w = TC.world(); ctx = N.default_context(); L = N.lib()
    n = 6
    sets = mixed(n, start=2)
    S = N.cbuf(b"".join(s.sig for s in sets)); B = N.cbuf(b"".join(s.bits() for s in sets))
    words = [s.word for s in sets]; midx = [s.msg for s in sets]
    asked = []
    cb = N.SCALAR_SOURCE(lambda _u, _out, count: asked.append(count))
    u32 = lambda v: (C.c_uint32 * len(v))(*v)
    sg = next(i for i, s in enumerate(sets) if s.sel is None); cm = next(i for i, s in enumerate(sets) if s.sel is not None)
    put = lambda i, v: words[:i] + [v] + words[i + 1:]
    cases = [(put(cm, len(w.members)), midx), (put(sg, SINGLE | len(w.pk96)), midx), (put(sg, 0xFFFFFFFF), midx), (words, midx[:3] + [len(w.msgs)] + midx[4:])]
    for wl, mi in cases:
        res = N.outbuf(1); res[0] = 9; sres = N.outbuf(n); C.memset(sres, 7, n)
        assert L.mbls_verify_multiple_committee_msgtable_rng(ctx.handle, w.ct.handle, S, u32(wl), B, STRIDE, w.mt.handle, u32(mi), n, res, cb, None) == N.ERR_ARGUMENT
        assert L.mbls_verify_multiple_committee_msgtable_locate_rng(ctx.handle, w.ct.handle, S, u32(wl), B, STRIDE, w.mt.handle, u32(mi), n, res, sres, None, cb,
                                                                    None) == N.ERR_ARGUMENT
        assert bytes(res)[0] == 9 and bytes(sres)[:n] == b"\x07" * n and asked == []
    res = N.outbuf(1); res[0] = 9
    f = L.mbls_verify_multiple_committee_msgtable_rng
    assert f(ctx.handle, w.ct.handle, S, u32(words), B, 16, w.mt.handle, u32(midx), n, res, cb, None) == N.ERR_ARGUMENT          # 128 bits do not cover 129 members
    assert f(ctx.handle, w.ct.handle, S, u32(words), B, 22, w.mt.handle, u32(midx), n, res, cb, None) == N.ERR_ARGUMENT          # not a multiple of 4
    assert f(ctx.handle, w.ct.handle, S, u32(words), B, STRIDE, w.mt.handle, u32(midx), n, res, N.SCALAR_SOURCE(), None) == N.ERR_ARGUMENT   # no scalar source
    assert L.mbls_verify_multiple_committee_msgtable_locate_rng(ctx.handle, w.ct.handle, S, u32(words), B, STRIDE, w.mt.handle, u32(midx), n, res, None, None, cb,
                                                                None) == N.ERR_ARGUMENT                                          # set_results is required
    assert bytes(res)[0] == 9 and asked == []
    assert f(ctx.handle, w.ct.handle, None, None, None, STRIDE, w.mt.handle, None, 0, res, cb, None) == N.OK and bytes(res)[0] == 1 and asked == []
    # device entries
    d_s = TC.dev(b"".join(s.sig for s in sets)); d_ci = TC.i32(words); d_b = TC.dev(b"".join(s.bits() for s in sets) + bytes(4)); d_mi = TC.i32(midx)
    d_r = i64(scalars(n, 1)); o = outputs(n)
    g = L.mbls_verify_multiple_committee_msgtable_device
    args = lambda bits=d_b.data_ptr(), stride=STRIDE, rands=d_r.data_ptr(), res=o[0].data_ptr(): (
        ctx.handle, w.ct.handle, d_s.data_ptr(), d_ci.data_ptr(), bits, stride, w.mt.handle, d_mi.data_ptr(), rands, n, res, o[1].data_ptr(), None)
    assert g(*args(bits=d_b.data_ptr() + 1)) == N.ERR_ARGUMENT                                                                   # d_bits not 4-byte aligned
    assert g(*args(stride=16)) == N.ERR_ARGUMENT and g(*args(stride=18)) == N.ERR_ARGUMENT
    assert g(*args(rands=None)) == N.ERR_ARGUMENT and g(*args(res=None)) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_committee_msgtable_locate_device(*args()[:12], None, None, None) == N.ERR_ARGUMENT             # d_set_results is required
    other = N.Context(0)
    try:
        mt2 = N.MsgTable(other, capacity_hint=2)
        try:
            a = list(args()); a[6] = mt2.handle
            assert g(*a) == N.ERR_ARGUMENT                                                                                       # a message table of another context
        finally:
            mt2.close()
    finally:
        other.close()
    assert read(n, o, False) == (9, 0x7fffffff)                  # nothing was written by the refused calls
    # n = 0 answers as mbls_verify_multiple_msgtable_device does: 1, status 0
    assert g(ctx.handle, w.ct.handle, None, None, None, STRIDE, w.mt.handle, None, None, 0, o[0].data_ptr(), o[1].data_ptr(), None) == N.OK
    assert read(0, o, False) == (1, 0)
    assert g(*args()) == N.OK and read(n, o, False) == (1, 0)


class CountingRng:
    """random.Random behind the getrandbits the mirror draws through, counting the calls"""
    def __init__(self, seed):
        self.r, self.calls = random.Random(seed), 0

    def getrandbits(self, k):
        self.calls += 1
        return self.r.getrandbits(k)


def test_python_mirror_agrees_and_leaves_the_generator_where_the_msgtable_method_does():
    from milagro_bls_amd import AggregateSignature, AggregatePublicKey, SingleKey
    w = TC.world()
    n = 20
    sets = mixed(n, start=11)
    apks = spelled_apks(sets)

    as_sig = AggregateSignature

    as_apk = AggregatePublicKey
    mine = [(as_sig(s.sig), SingleKey(s.word & 0x7FFFFFFF), None, s.msg) if s.sel is None else (as_sig(s.sig), s.word, TC.bits_of(s.sel)[:17], s.msg) for s in sets]
    theirs = [(as_sig(s.sig), as_apk(a), s.msg) for s, a in zip(sets, apks)]
    r1, r2 = CountingRng(4), CountingRng(4)
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee(r1, mine, w.ct, w.mt) is True
    assert AggregateSignature.verify_multiple_aggregate_signatures_msgtable(r2, theirs, w.mt) is True
    assert r1.calls == r2.calls > 0 and r1.r.random() == r2.r.random()
    j = next(i for i, s in enumerate(sets) if s.sel is not None and len(s.sel) > 2)
    mine[j] = (mine[j][0], mine[j][1], TC.bits_of(sets[j].sel[1:]), mine[j][3])
    ok, per_set = AggregateSignature.verify_multiple_aggregate_signatures_committee_locate(CountingRng(4), mine, w.ct, w.mt)
    assert ok is False and per_set == [i != j for i in range(n)]
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee(CountingRng(4), mine, w.ct, w.mt) is False
