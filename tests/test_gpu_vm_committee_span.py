"""GPU tests of mbls_verify_multiple_committee_span_msgtable[_locate]_device / _rng (include/mbls.h, "verify_multiple OVER COMMITTEE SPANS AND THE RESIDENT MESSAGE
TABLE"; csrc/mbls_vcs.h). The world is the span tests' (test_gpu_committee_span.world: the committee tests' keys, key table and message table, a committee table
with the P0 / -P0 committees behind the others, the signed span pool, STRIDE = 44) with the single-key sets of test_gpu_vm_committee.pool beside it. Every call is
compared with mbls_verify_multiple_sets_indexed_msgtable[_locate]_device on the same signatures, scalars and message indices with every set's selected members
spelled out in (segment, member) order: result byte, status word, and for the _locate forms every set byte and word -- under the modes of mbls_ctx_set_vm_grouping,
mbls_ctx_set_committee_route and the split factors of mbls_ctx_set_vm_span_split. Ground truth that does not lean on the baseline: an all-valid call answers 1,
and with one participation bit flipped in set j it answers 0 and the locate form reads 0 at j and 1 elsewhere."""
import ctypes as C
import random

import pytest

import test_gpu_committee as TC
import test_gpu_committee_span as TS
import test_gpu_vm_committee as TV
from test_gpu_committee_span import STRIDE, Item
from test_gpu_vm_committee import SINGLE, BAD_PK, APK_INF, NO_KEYS, PK_INF, PAIRING, BAD_MSG, scalars, i64, outputs, read, call_base

pytestmark = pytest.mark.gpu

GROUPINGS = (0, 1, 2)
ROUTES = (0, 1, 2)
SPLITS = (1, 2, 16)
COUNTS = (1, 2, 3, 63, 64, 65, 200)
# the span pool's items that verify under verify_multiple: plain committees under every pattern that selects somebody, the two- and three-committee spans (mixed
# routes in the automatic mode), both 64-committee spans, the fix-up edges (P0 + (-P0) under the infinite signature contributes 1)
VALID_TAGS = tuple("one_" + p for p in TS.PATTERNS if p != "nobody") + ("multi", "span64_full", "span64_mixed", "same_id_twice", "sums_cancel", "cancel_beside_signers",
                                                                        "nobody_beside_signers", "no_absentee")


class VSet:
    """one set of a call: its ids (or the one word SINGLE | key index), its field, message number, signature, and the key-table indices the baseline spells out"""
    def __init__(self, ids, field, msg, sig, keys, tag, item=None):
        self.ids, self.field, self.msg, self.sig, self.keys, self.tag, self.item = list(ids), field, msg, sig, list(keys), tag, item

    @property
    def single(self):
        return self.item is None


_P = None


def as_set(it):
    return VSet(it.cids, TS.field_of(it), it.msg, it.sig, TS.keys_of(it), it.tag, it)


def pool():
    global _P
    if _P is not None:
        return _P
    s = TS.world()
    valid = [as_set(it) for it in s.pool if it.tag in VALID_TAGS and TS.keys_of(it, s)]      # (a one-member committee has patterns that select nobody)
    singles = [VSet([x.word], b"\xa5" * STRIDE, x.msg, x.sig, x.keys, "single") for x in TV.pool()[1]]      # a single-key set's bytes are not read: any value
    # the split edges, signed once: direct lists and missing lists of 1, 2, 3, 15, 16 and 17 entries; an ineligible committee behind 64 signers
    cid = {m: TC.SIZES.index(m) for m in TC.SIZES}
    sp = s.w.sid
    edge = []
    for k in (1, 2, 3, 15, 16, 17):
        edge.append(Item([cid[32]], [list(range(k))], k % 3, "direct_%d" % k))
        edge.append(Item([cid[33]], [list(range(k, 33))], (k + 1) % 3, "missing_%d" % k))
    for name in ("infinite", "invalid", "outside"):
        edge.append(Item([cid[64], sp[name]], [list(range(64)), list(range(len(s.members[sp[name]])))], 1, "last_chunk_" + name))
    TS.sign(s, edge)
    tags = {}                                                   # every item of the signed pool by tag (from the pool itself: by_tag also holds what single tests add)
    for it in s.pool:
        tags.setdefault(it.tag, []).append(as_set(it))
    _P = (valid, singles, {it.tag: as_set(it) for it in edge}, tags)
    return _P


def mixed(n, start=0):
    """n valid sets: two of five a single-key set, the others walk the valid span items"""
    valid, singles, _e, _t = pool()
    out, a, b = [], start, 3 * start
    for i in range(n):
        if (i + start) % 5 in (1, 3):
            out.append(singles[b % len(singles)]); b += 1
        else:
            out.append(valid[a % len(valid)]); a += 1
    return out


def arrays(sets):
    ids, off = [], [0]
    for x in sets:
        ids += x.ids; off.append(len(ids))
    return ids, off


def buffers_new(sets, rands, ids=None, off=None, bits=None, midx=None, sigs=None, pad=0):
    if ids is None:
        ids, off = arrays(sets)
    d_s = TC.dev(b"".join(sigs if sigs is not None else [x.sig for x in sets]))
    d_ids = TC.i32(ids); d_off = TC.i32(off)
    d_b = TC.dev((bits if bits is not None else b"".join(x.field for x in sets)) + bytes(pad))
    d_mi = TC.i32(midx if midx is not None else [x.msg for x in sets]); d_r = i64(rands)
    return d_s, d_ids, len(ids), d_off, d_b, d_mi, d_r, outputs(len(sets))


def call_new(sets, rands, locate, n_ids=None, stride=STRIDE, buffers=None, **kw):
    from milagro_bls_amd import _native as N
    s = TS.world(); ctx = N.default_context(); L = N.lib(); n = len(sets)
    d_s, d_ids, nid, d_off, d_b, d_mi, d_r, o = buffers if buffers is not None else buffers_new(sets, rands, **kw)
    nid = nid if n_ids is None else n_ids
    if locate:
        ctx.check(L.mbls_verify_multiple_committee_span_msgtable_locate_device(ctx.handle, s.ct.handle, d_s.data_ptr(), d_ids.data_ptr(), nid, d_off.data_ptr(), d_b.data_ptr(),
                                                                               stride, s.w.mt.handle, d_mi.data_ptr(), d_r.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(),
                                                                               o[2].data_ptr(), o[3].data_ptr(), None))
    else:
        ctx.check(L.mbls_verify_multiple_committee_span_msgtable_device(ctx.handle, s.ct.handle, d_s.data_ptr(), d_ids.data_ptr(), nid, d_off.data_ptr(), d_b.data_ptr(), stride,
                                                                        s.w.mt.handle, d_mi.data_ptr(), d_r.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), None))
    return read(n, o, locate)


@pytest.fixture(autouse=True)
def _modes_back():
    yield
    from milagro_bls_amd import batch, _native as N
    N.default_context().set_committee_route(0)
    batch.set_vm_grouping(0)
    batch.set_vm_span_split(0)


def compare(sets, rands, lists=None, modes=None, **kw):
    """both forms of the new entry under every (grouping, route, split) of `modes` against both forms of the baseline under the same grouping (the baseline knows
    neither route nor split) -> the baseline's locate answer (result, status, set results, set status) of the last grouping"""
    from milagro_bls_amd import batch, _native as N
    modes = modes if modes is not None else [(g, r, p) for g in GROUPINGS for r in ROUTES for p in SPLITS]
    base_kw = {k: v for k, v in kw.items() if k in ("midx", "sigs")}
    base = {}
    for g, r, p in modes:
        batch.set_vm_grouping(g)
        if g not in base:
            b0 = call_base(sets, rands, False, lists=lists, **base_kw)
            b1 = call_base(sets, rands, True, lists=lists, **base_kw)
            assert b1[:2] == b0
            base[g] = b1
        b1 = base[g]
        N.default_context().set_committee_route(r); batch.set_vm_span_split(p)
        n0 = call_new(sets, rands, False, **kw)
        n1 = call_new(sets, rands, True, **kw)
        assert n0 == b1[:2], (g, r, p, n0, b1[:2])
        assert n1[:2] == b1[:2], (g, r, p, n1[:2], b1[:2])
        bad = [(i, sets[i].tag, n1[2][i], b1[2][i], hex(n1[3][i]), hex(b1[3][i])) for i in range(len(sets)) if (n1[2][i], n1[3][i]) != (b1[2][i], b1[3][i])]
        assert not bad, (g, r, p, bad[:8])
    return base[modes[-1][0]]


def diagonal(n):
    """three (grouping, route, split) triples that between them touch every mode once, rotated by the call's size; auto split last"""
    return [((n + k) % 3, (2 * n + k) % 3, SPLITS[(n + 2 * k) % 3]) for k in range(3)] + [(0, 0, 0)]


@pytest.mark.parametrize("n", COUNTS)
def test_all_valid_calls_answer_one_and_equal_the_indexed_entry(n):
    sets = mixed(n, start=n)
    assert n < 3 or {x.single for x in sets} == {True, False}
    modes = None if n == 65 else diagonal(n)                    # the full cross of 3 groupings x 3 routes x 3 splits at n = 65
    res, st, sres, sst = compare(sets, scalars(n, n), modes=modes)
    assert res == 1 and st == 0 and sres == [1] * n and sst == [0] * n


def test_the_largest_call_holds_every_kind_of_valid_item():
    sets = mixed(200, start=200)
    assert {x.tag for x in sets} == set(VALID_TAGS) | {"single"}
    assert {len(x.ids) for x in sets} >= {1, 2, 3, 64}


@pytest.mark.parametrize("split", (1, 4))
@pytest.mark.parametrize("n", (3, 65))
def test_one_flipped_participation_bit_rejects_the_call_and_names_the_set(n, split):
    """one bit of one span set flipped against its signers -- a signer dropped (n odd) or a non-signer added: the call answers 0, the locate form reads 0 at that set
    and 1 elsewhere"""
    s = TS.world()
    sets = list(mixed(n, start=n))
    cand = [i for i, x in enumerate(sets) if x.tag == "multi"]
    if not cand:
        sets[0] = pool()[3]["multi"][4]; cand = [0]
    j = cand[len(cand) // 2]
    it = sets[j].item
    t = max(range(len(it.cids)), key=lambda u: len(it.sels[u]) * (len(s.members[it.cids[u]]) - len(it.sels[u])) + len(s.members[it.cids[u]]))
    m = len(s.members[it.cids[t]])
    flip = it.sels[t][-1] if (split == 1 and it.sels[t]) or len(it.sels[t]) == m else next(p for p in range(m) if p not in it.sels[t])
    bent = Item(it.cids, [sorted(set(sel) ^ ({flip} if u == t else set())) for u, sel in enumerate(it.sels)], it.msg, it.tag)
    bits = b"".join(TS.field_of(bent) if i == j else x.field for i, x in enumerate(sets))
    lists = [TS.keys_of(bent) if i == j else x.keys for i, x in enumerate(sets)]
    assert lists[j] != sets[j].keys
    modes = [(g, r, split) for g, r in ((0, 0), (1, 2), (2, 1))]
    res, st, sres, sst = compare(sets, scalars(n, 100 + n), lists=lists, bits=bits, modes=modes)
    assert res == 0 and st == 0
    assert sres == [0 if i == j else 1 for i in range(n)] and sst == [PAIRING if i == j else 0 for i in range(n)]


@pytest.mark.parametrize("split", (2, 16))
def test_split_edges(split):
    """lists shorter than P (a single-key set, q = 0, nobody, first), of exactly P and P +- 1 entries on either list, equal partial sums (the same id twice, forced
    direct), partial sums that cancel (P0 and -P0, forced direct, P = 2) and an ineligible committee whose special member falls in the LAST chunk"""
    valid, singles, edge, tags = pool()
    k = split
    sets = [singles[0], tags["q0"][0], tags["one_nobody"][2], tags["one_first"][7], edge["direct_%d" % (k - 1)], edge["direct_%d" % k], edge["direct_%d" % (k + 1)],
            edge["missing_%d" % (k - 1)], edge["missing_%d" % k], edge["missing_%d" % (k + 1)], tags["same_id_twice"][0], tags["sums_cancel"][0],
            edge["last_chunk_infinite"], edge["last_chunk_invalid"], edge["last_chunk_outside"], singles[1]]
    n = len(sets)
    for route in ROUTES:                                           # 1: everything direct; 2: the missing lists are the complement of 33 members
        res, st, sres, sst = compare(sets, scalars(n, 7 + split), modes=[(0, route, split), (1, route, split)])
        assert res == 0
        assert [i for i in range(n) if not sres[i]] == [1, 2, 13, 14]      # q = 0 and nobody under a signature; the invalid member; the key outside G1
        assert not st & (NO_KEYS | APK_INF) and not any(x & (NO_KEYS | APK_INF) for x in sst)
        assert sst[11] == 0 and sres[11] == 1                      # P0 + (-P0): infinity, and no bit says so
        assert sst[12] == PK_INF and sst[13] & BAD_PK and sst[14] == PAIRING and sst[10] == 0


def malformed_call():
    """a 12-set call with one set of every malformed kind and two single-key indices outside the key table -> (sets, raw ids, raw offsets, n_ids, the baseline's lists,
    the bad positions)"""
    s = TS.world(); w = s.w
    cid = {m: TC.SIZES.index(m) for m in TC.SIZES}
    sets = list(mixed(12, start=4))
    idl = [list(x.ids) for x in sets]
    multi = pool()[3]["multi"]
    idl[0] = multi[0].ids + [len(s.members)]                      # an id at the committee count
    idl[2] = pool()[3]["span64_full"][0].ids + [cid[1]]           # 65 ids
    idl[4] = [cid[129], cid[129], cid[128]]                       # M = 386 > 8 * 44
    idl[5] = [SINGLE | 5, cid[2]]                                 # bit 31 among two ids
    idl[6] = [SINGLE | len(w.pk96)]                               # a single-key index at the key table's size
    idl[7] = [0xFFFFFFFF]                                         # ... and key 0x7FFFFFFF
    ids, off = [], [0]
    for l in idl:
        ids += l; off.append(len(ids))
    # set 10's range ends one past n_ids; set 11's runs backwards
    n_ids = off[11] - 1
    off[12] = off[11] - 1
    bad = [0, 2, 4, 5, 6, 7, 10, 11]
    lists = [x.keys for x in sets]
    for i in bad:
        lists[i] = [0xFFFFFFFF]
    lists[6] = [len(w.pk96)]; lists[7] = [0x7FFFFFFF]
    return sets, ids, off, n_ids, lists, bad


@pytest.mark.parametrize("split", (0, 1, 4))
def test_malformed_sets_are_rejected_and_located_as_the_indexed_entry_does_on_0xffffffff(split):
    sets, ids, off, n_ids, lists, bad = malformed_call()
    n = len(sets)
    res, st, sres, sst = compare(sets, scalars(n, 55), lists=lists, ids=ids, off=off, n_ids=n_ids, modes=[(0, 0, split), (1, 2, split), (2, 1, split)])
    assert res == 0 and st & BAD_PK
    assert [i for i in range(n) if not sres[i]] == bad and all(sst[i] & BAD_PK for i in bad)
    assert all(sst[i] == 0 for i in range(n) if i not in bad)


def host_raw(sets, ids, off, n_ids, midx=None, stride=STRIDE, bits=None):
    """both _rng entries on raw arrays -> (return codes, result byte, set bytes, draws asked)"""
    from milagro_bls_amd import _native as N
    s = TS.world(); ctx = N.default_context(); L = N.lib(); n = len(sets)
    u32 = lambda v: (C.c_uint32 * max(1, len(v)))(*v)
    asked = []

    def source(_user, out, count):
        asked.append(int(count))
        for i in range(int(count)):
            out[i] = 3 + 2 * i
    cb = N.SCALAR_SOURCE(source)
    S = N.cbuf(b"".join(x.sig for x in sets)); B = N.cbuf(bits if bits is not None else b"".join(x.field for x in sets))
    mi = u32(midx if midx is not None else [x.msg for x in sets])
    res = N.outbuf(1); res[0] = 9; sres = N.outbuf(n); C.memset(sres, 7, n)
    r0 = L.mbls_verify_multiple_committee_span_msgtable_rng(ctx.handle, s.ct.handle, S, u32(ids), n_ids, u32(off), B, stride, s.w.mt.handle, mi, n, res, cb, None)
    r1 = L.mbls_verify_multiple_committee_span_msgtable_locate_rng(ctx.handle, s.ct.handle, S, u32(ids), n_ids, u32(off), B, stride, s.w.mt.handle, mi, n, res, sres, None, cb,
                                                                   None)
    return (r0, r1), bytes(res)[0], bytes(sres)[:n], asked


def test_host_entries_refuse_every_malformed_kind_and_leave_the_outputs_unwritten():
    from milagro_bls_amd import _native as N
    s = TS.world(); w = s.w
    cid = {m: TC.SIZES.index(m) for m in TC.SIZES}
    sets = list(mixed(6, start=2))
    good_ids, good_off = arrays(sets)
    com = next(i for i, x in enumerate(sets) if not x.single); sg = next(i for i, x in enumerate(sets) if x.single)

    def with_list(i, l):
        idl = [list(x.ids) for x in sets]; idl[i] = l
        ids, off = [], [0]
        for x in idl:
            ids += x; off.append(len(ids))
        return ids, off, len(ids)
    back = list(good_off); back[6] = back[5] - 1
    cases = [with_list(com, sets[com].ids + [len(s.members)]), with_list(com, [cid[1]] * 65), with_list(com, [cid[129], cid[129], cid[128]]),
             with_list(com, [SINGLE | 5, cid[2]]), with_list(sg, [SINGLE | len(w.pk96)]), with_list(sg, [0xFFFFFFFF]),
             (good_ids, back, len(good_ids)), (good_ids, good_off, len(good_ids) - 1)]
    for ids, off, n_ids in cases:
        rc, res, sres, asked = host_raw(sets, ids, off, n_ids)
        assert rc == (N.ERR_ARGUMENT, N.ERR_ARGUMENT) and res == 9 and sres == b"\x07" * 6 and asked == [], (ids[:6], off)
    rc, res, sres, asked = host_raw(sets, good_ids, good_off, len(good_ids), midx=[x.msg for x in sets[:3]] + [len(w.msgs)] + [0, 0])
    assert rc == (N.ERR_ARGUMENT, N.ERR_ARGUMENT) and res == 9 and asked == []
    rc, res, sres, asked = host_raw(sets, good_ids, good_off, len(good_ids), stride=STRIDE + 2, bits=bytes((STRIDE + 2) * 6))
    assert rc == (N.ERR_ARGUMENT, N.ERR_ARGUMENT) and res == 9 and asked == []
    rc, res, sres, asked = host_raw(sets, good_ids, good_off, len(good_ids))
    assert rc == (N.OK, N.OK) and res == 1 and sres == b"\x01" * 6 and asked == [6, 6]


def test_device_entries_refuse_bad_arguments_and_answer_an_empty_call():
    from milagro_bls_amd import _native as N
    s = TS.world(); ctx = N.default_context(); L = N.lib()
    n = 6
    sets = mixed(n, start=2)
    d_s, d_ids, nid, d_off, d_b, d_mi, d_r, o = buffers_new(sets, scalars(n, 1), pad=4)
    g = L.mbls_verify_multiple_committee_span_msgtable_device
    args = lambda bits=d_b.data_ptr(), stride=STRIDE, rands=d_r.data_ptr(), res=o[0].data_ptr(), off=d_off.data_ptr(), ct=s.ct.handle, mt=s.w.mt.handle: (
        ctx.handle, ct, d_s.data_ptr(), d_ids.data_ptr(), nid, off, bits, stride, mt, d_mi.data_ptr(), rands, n, res, o[1].data_ptr(), None)
    assert g(*args(bits=d_b.data_ptr() + 1)) == N.ERR_ARGUMENT                                  # d_bits not 4-byte aligned
    assert g(*args(stride=STRIDE - 2)) == N.ERR_ARGUMENT                                        # bits_stride not a multiple of 4
    assert g(*args(rands=None)) == N.ERR_ARGUMENT and g(*args(res=None)) == N.ERR_ARGUMENT and g(*args(off=None)) == N.ERR_ARGUMENT
    assert g(*args(ct=None)) == N.ERR_ARGUMENT and g(*args(mt=None)) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_committee_span_msgtable_locate_device(*args()[:14], None, None, None) == N.ERR_ARGUMENT       # d_set_results is required
    other = N.Context(0)
    try:
        mt2 = N.MsgTable(other, capacity_hint=2)
        try:
            assert g(*args(mt=mt2.handle)) == N.ERR_ARGUMENT                                    # a message table of another context
        finally:
            mt2.close()
    finally:
        other.close()
    for bad in (3, 5, 32, -1):
        assert L.mbls_ctx_set_vm_span_split(ctx.handle, bad) == N.ERR_ARGUMENT
    assert read(n, o, False) == (9, 0x7fffffff)                  # nothing was written by the refused calls
    # n = 0 answers as mbls_verify_multiple_msgtable_device does: 1, status 0
    assert g(ctx.handle, s.ct.handle, None, None, 0, None, None, STRIDE, s.w.mt.handle, None, None, 0, o[0].data_ptr(), o[1].data_ptr(), None) == N.OK
    assert read(0, o, False) == (1, 0)
    assert g(*args()) == N.OK and read(n, o, False) == (1, 0)


@pytest.mark.parametrize("split", (1, 2))
def test_a_set_of_one_plain_committee_equals_the_committee_msgtable_entry(split):
    """the one-committee items of the span pool (every pattern, the special committees) beside single-key sets: the _committee_msgtable entries over the span tests'
    table return the same bytes and words"""
    from milagro_bls_amd import batch, _native as N
    s = TS.world(); ctx = N.default_context(); L = N.lib()
    _v, singles, _e, _t = pool()
    sets = []
    for i, it in enumerate(s.pool[:s.n_single]):
        sets.append(as_set(it))
        if i % 4 == 0:
            sets.append(singles[i % len(singles)])
    n = len(sets); rands = scalars(n, 12)
    batch.set_vm_span_split(split)
    for route in ROUTES:
        ctx.set_committee_route(route)
        for locate in (False, True):
            new = call_new(sets, rands, locate)
            d_s = TC.dev(b"".join(x.sig for x in sets)); d_ci = TC.i32([x.ids[0] for x in sets]); d_b = TC.dev(b"".join(x.field for x in sets))
            d_mi = TC.i32([x.msg for x in sets]); d_r = i64(rands); o = outputs(n)
            if locate:
                ctx.check(L.mbls_verify_multiple_committee_msgtable_locate_device(ctx.handle, s.ct.handle, d_s.data_ptr(), d_ci.data_ptr(), d_b.data_ptr(), STRIDE, s.w.mt.handle,
                                                                                  d_mi.data_ptr(), d_r.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                                                  o[3].data_ptr(), None))
            else:
                ctx.check(L.mbls_verify_multiple_committee_msgtable_device(ctx.handle, s.ct.handle, d_s.data_ptr(), d_ci.data_ptr(), d_b.data_ptr(), STRIDE, s.w.mt.handle,
                                                                           d_mi.data_ptr(), d_r.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), None))
            assert new == read(n, o, locate), (route, locate)


def spelled_apks(sets):
    from milagro_bls_amd import batch, _native as N
    w = TC.world()
    off = [0]
    for x in sets:
        off.append(off[-1] + len(x.keys))
    apks, st = batch.aggregate_public_keys_batch(b"".join(w.pk96[k] for x in sets for k in x.keys), len(sets), pk_format=N.PK_UNCOMPRESSED, pk_offsets=off)
    assert not any(st)
    return [apks[96 * i:96 * i + 96] for i in range(len(sets))]


@pytest.mark.parametrize("split", (0, 1, 8))
def test_rng_entries_draw_as_the_msgtable_entry_does(split, vectors):
    """a counting draw: asked for the same counts as mbls_verify_multiple_msgtable_rng on the same signatures with the aggregate keys spelled out -- all n sets; the
    sets in front of a signature outside G2 in the middle; not at all when set 0's signature fails -- and the same answers; the locate form names the bad set"""
    from milagro_bls_amd import batch
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    s = TS.world(); w = s.w
    n = 24
    sets = [x for x in mixed(n, start=40) if x.tag != "sums_cancel"][:n]        # (an aggregate key at infinity has no 96-byte form to spell out)
    n = len(sets)
    rands = scalars(n, 5)
    apks = spelled_apks(sets)
    idl = [x.ids for x in sets]; fields = [x.field for x in sets]; midx = [x.msg for x in sets]
    batch.set_vm_span_split(split)
    for where in (None, n // 2, 0):
        sigs = [x.sig for x in sets]
        if where is not None:
            sigs[where] = probe
        asked_new, asked_old, asked_loc = [], [], []
        draw = lambda log: (lambda count: (log.append(count), rands[:count])[1])
        got = batch.verify_multiple_committee_span_msgtable_rng(s.ct, w.mt, b"".join(sigs), idl, fields, STRIDE, midx, draw(asked_new))
        old = batch.verify_multiple_msgtable_rng(w.mt, b"".join(sigs), b"".join(apks), midx, n, draw(asked_old))
        assert asked_new == asked_old == ([n] if where is None else [where] if where else []), (where, asked_new, asked_old)
        assert got == old == (where is None)
        res, sres, sst = batch.verify_multiple_committee_span_msgtable_locate_rng(s.ct, w.mt, b"".join(sigs), idl, fields, STRIDE, midx, draw(asked_loc))
        ores, osres, osst = batch.verify_multiple_msgtable_locate_rng(w.mt, b"".join(sigs), b"".join(apks), midx, n, draw([]))
        assert asked_loc == asked_new and (res, sres, sst) == (ores, osres, osst)
        assert sres == [where is None or i < where for i in range(n)]


def test_a_pre_reserved_scratch_and_workspace_change_no_byte_and_the_plan_is_what_the_call_reserves():
    from milagro_bls_amd import batch, _native as N
    ctx = N.default_context()
    sets = list(mixed(200, start=9)); rands = scalars(200, 77)
    j = next(i for i, x in enumerate(sets) if x.tag == "multi")
    it = sets[j].item
    t = next(u for u in range(len(it.cids)) if len(it.sels[u]) > 1)
    bent = Item(it.cids, [sel[1:] if u == t else sel for u, sel in enumerate(it.sels)], it.msg, it.tag)
    bits = b"".join(TS.field_of(bent) if i == j else x.field for i, x in enumerate(sets))
    batch.set_vm_span_split(4)
    before = (call_new(sets, rands, True, bits=bits), call_new(sets, rands, False, bits=bits))
    ctx.reserve_committee_span_items(3000, 400)                  # more sets and a wider region than any call so far: every array moves
    T = len(TC.world().mt)
    P, items = N.plan_verify_multiple_committee_span(200, T, 352, locate=True, split_mode=4, limits=ctx.limits())
    assert P == 4 and items == N.plan_verify_multiple_msgtable_locate_workspace_items(200, T, limits=ctx.limits()) + 2 * 4 * 200
    ctx.reserve(4 * items)                                       # the workspace grows: the partial sums' items move with the stride
    after = (call_new(sets, rands, True, bits=bits), call_new(sets, rands, False, bits=bits))
    assert after == before and before[0][0] == 0 and [i for i in range(200) if not before[0][2][i]] == [j]


def test_python_mirror_agrees_and_leaves_the_generator_where_the_msgtable_method_does():
    from milagro_bls_amd import AggregateSignature, AggregatePublicKey, SingleKey
    s = TS.world(); w = s.w
    sets = [x for x in mixed(20, start=11) if x.tag != "sums_cancel"]
    n = len(sets)
    apks = spelled_apks(sets)
    sig, apk = AggregateSignature, AggregatePublicKey
    used = lambda x: x.field[:(TS.total_bits(x.item) + 7) // 8]
    mine = [(sig(x.sig), SingleKey(x.ids[0] & 0x7FFFFFFF), None, x.msg) if x.single else (sig(x.sig), x.ids, used(x), x.msg) for x in sets]
    theirs = [(sig(x.sig), apk(a), x.msg) for x, a in zip(sets, apks)]
    r1, r2 = TV.CountingRng(4), TV.CountingRng(4)
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee_span(r1, mine, s.ct, w.mt) is True
    assert AggregateSignature.verify_multiple_aggregate_signatures_msgtable(r2, theirs, w.mt) is True
    assert r1.calls == r2.calls > 0 and r1.r.random() == r2.r.random()
    j = next(i for i, x in enumerate(sets) if not x.single and len(x.keys) > 2 and x.tag.startswith(("one_", "multi")))      # (distinct honest keys)
    f = bytearray(mine[j][2]); p = next(b for b in range(8 * len(f)) if (f[b >> 3] >> (b & 7)) & 1); f[p >> 3] ^= 1 << (p & 7)
    mine[j] = (mine[j][0], mine[j][1], bytes(f), mine[j][3])
    ok, per_set = AggregateSignature.verify_multiple_aggregate_signatures_committee_span_locate(TV.CountingRng(4), mine, s.ct, w.mt)
    assert ok is False and per_set == [i != j for i in range(n)]
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee_span(TV.CountingRng(4), mine, s.ct, w.mt) is False
