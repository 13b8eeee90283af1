"""GPU tests of mbls_verify_multiple_batches_committee_span_msgtable[_locate]_device / _rng (include/mbls.h, "MANY verify_multiple BATCHES PER CALL OVER COMMITTEE
SPANS AND THE RESIDENT MESSAGE TABLE"). The world is the span tests' (test_gpu_committee_span.world: committees of 1 .. 129 members and the special ones, the
P0 / -P0 committees, STRIDE = 44), the sets are test_gpu_vm_committee_span.mixed(n) and its edge pool, the layouts test_gpu_vm_batches_committee.cut(n, kind).
Every call is compared -- result byte, status word, every set byte and every set word -- with mbls_verify_multiple_batches_locate_indexed_device on the
spelled-out (segment, member) lists and message bytes, and with one call of mbls_verify_multiple_committee_span_msgtable_locate_device per non-empty batch, under
the modes of mbls_ctx_set_vm_grouping, mbls_ctx_set_committee_route and mbls_ctx_set_vm_span_split. The sizes are the smallest that cross the wave, the split
chunk edges and the coop / lane switches; none reproduces the workload."""
import ctypes as C

import pytest

import test_gpu_committee as TC
import test_gpu_committee_span as TS
import test_gpu_vm_batches_committee as TB
import test_gpu_vm_committee as TV
import test_gpu_vm_committee_span as SP
import vbg_cases as V
from test_gpu_committee_span import STRIDE, Item
from test_gpu_vm_batches_committee import cut, outputs, read, owner_of
from test_gpu_vm_committee import SINGLE, BAD_PK, PAIRING, BAD_MSG, scalars, i64
from test_gpu_vm_committee_span import GROUPINGS, ROUTES, SPLITS, COUNTS, mixed, pool, arrays, diagonal

pytestmark = pytest.mark.gpu

CUTS = TB.CUTS
FULL = [(g, r, p) for g in GROUPINGS for r in ROUTES for p in SPLITS]


@pytest.fixture(autouse=True)
def _modes_back():
    yield
    from milagro_bls_amd import batch, _native as N
    N.default_context().set_committee_route(0)
    batch.set_vm_grouping(0)
    batch.set_vm_span_split(0)


def call_new(sets, rands, layout, locate=True, max_groups=0, ids=None, off=None, n_ids=None, bits=None, midx=None, sigs=None, ctx=None, ct=None, mt=None, stride=STRIDE):
    from milagro_bls_amd import _native as N
    s = TS.world(); ctx = ctx or N.default_context(); L = N.lib(); n = len(sets)
    boff, spb, B = layout
    if ids is None:
        ids, off = arrays(sets)
    d_s = TC.dev(b"".join(sigs if sigs is not None else [x.sig for x in sets]))
    d_ids = TC.i32(ids); d_off = TC.i32(off)
    d_b = TC.dev(bits if bits is not None else b"".join(x.field for x in sets))
    d_mi = TC.i32(midx if midx is not None else [x.msg for x in sets]); d_r = i64(rands)
    d_o = TC.i32(boff) if boff is not None else None
    o = outputs(n, B)
    head = (ctx.handle, (ct or s.ct).handle, d_s.data_ptr(), d_ids.data_ptr(), len(ids) if n_ids is None else n_ids, d_off.data_ptr(), d_b.data_ptr(), stride,
            (mt or s.w.mt).handle, d_mi.data_ptr(), d_r.data_ptr(), n, d_o.data_ptr() if d_o is not None else None, spb, B, max_groups, o[0].data_ptr(), o[1].data_ptr())
    if locate:
        ctx.check(L.mbls_verify_multiple_batches_committee_span_msgtable_locate_device(*head, o[2].data_ptr(), o[3].data_ptr(), None))
        return read(n, B, o)
    ctx.check(L.mbls_verify_multiple_batches_committee_span_msgtable_device(*head, None))
    return read(n, B, o)[:2]


def call_base(sets, rands, layout, lists=None, sigs=None):
    """mbls_verify_multiple_batches_locate_indexed_device on the spelled-out (segment, member) lists and message bytes"""
    from milagro_bls_amd import _native as N
    w = TC.world(); ctx = N.default_context(); L = N.lib(); n = len(sets)
    boff, spb, B = layout
    lists = lists if lists is not None else [x.keys for x in sets]
    koff = [0]
    for l in lists:
        koff.append(koff[-1] + len(l))
    d_s = TC.dev(b"".join(sigs if sigs is not None else [x.sig for x in sets])); d_k = TC.i32([x for l in lists for x in l]); d_ko = TC.i32(koff)
    d_m = TC.dev(b"".join(w.msgs[x.msg] for x in sets)); d_r = i64(rands)
    d_o = TC.i32(boff) if boff is not None else None
    o = outputs(n, B)
    ctx.check(L.mbls_verify_multiple_batches_locate_indexed_device(ctx.handle, w.kt.handle, d_s.data_ptr(), d_k.data_ptr(), d_ko.data_ptr(), 0, d_m.data_ptr(), 32, None,
                                                                   d_r.data_ptr(), n, d_o.data_ptr() if d_o is not None else None, spb, B, o[0].data_ptr(),
                                                                   o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), None))
    return read(n, B, o)


def ranges(layout, n):
    boff, spb, B = layout
    return [(b * spb, (b + 1) * spb) if boff is None else (boff[b], boff[b + 1]) for b in range(B)]


def status_bits():
    """the MBLS_ST_* bits as include/mbls.h defines them"""
    import os
    import re
    import helpers
    txt = open(os.path.join(helpers.ROOT, "include", "mbls.h")).read()
    return {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define MBLS_ST_([A-Z0-9_]+)\s+0x([0-9a-fA-F]+)u", txt)}


ST = status_bits()
# the bits on which a batch rejects without a pairing check (include/mbls.h, "MANY verify_multiple BATCHES IN ONE CALL"), by the header's names
REJECTING = ST["BAD_SIG_ENCODING"] | ST["SIG_NOT_IN_G2"] | ST["BAD_PK_ENCODING"] | ST["BAD_MSG_RANGE"] | ST["BAD_SCALAR"]
# every bit the header knows is either rejecting, or one of the four that are not: a status bit added later fails here before it can bend call_loop's rule
assert ST["PAIRING_FAILED"] == PAIRING and ST["BAD_PK_ENCODING"] == BAD_PK and ST["BAD_MSG_RANGE"] == BAD_MSG
assert set(ST) == {"BAD_SIG_ENCODING", "SIG_NOT_IN_G2", "BAD_PK_ENCODING", "APK_INFINITY", "NO_KEYS", "PK_INFINITY", "PAIRING_FAILED", "BAD_SCALAR", "BAD_MSG_RANGE"}, sorted(ST)


def call_loop(sets, rands, layout, bits=None, sigs=None):
    """B separate calls of mbls_verify_multiple_committee_span_msgtable_locate_device, one per non-empty batch of a sound layout, with that batch's scalars; an
    empty batch is an empty iterator: 1, no bit. The one difference include/mbls.h states between a call's word and a batch's ("MANY verify_multiple BATCHES IN
    ONE CALL": the one-batch entries report a failed pairing check through the bool only) is applied here: a batch's word is the call's word plus
    MBLS_ST_PAIRING_FAILED exactly where the result is 0 and no rejecting bit is set. Every set byte and set word is compared as the call wrote it."""
    n = len(sets)
    fields = [bits[STRIDE * i:STRIDE * (i + 1)] for i in range(n)] if bits is not None else [x.field for x in sets]
    res, st, sres, sst = [], [], [None] * n, [None] * n
    for lo, hi in ranges(layout, n):
        if lo == hi:
            res.append(1); st.append(0)
            continue
        r, w, sr, sw = SP.call_new(sets[lo:hi], rands[lo:hi], True, bits=b"".join(fields[lo:hi]), sigs=sigs[lo:hi] if sigs is not None else None)
        assert not (w | PAIRING) & ~sum(ST.values()) and all(not x & ~sum(ST.values()) for x in sw), (hex(w), [hex(x) for x in sw])      # no bit the header does not name
        res.append(r); st.append(w | (PAIRING if not r and not w & REJECTING else 0)); sres[lo:hi] = sr; sst[lo:hi] = sw
    return res, st, sres, sst


def same(got, want, what):
    for name, a, b in zip(("results", "status", "set results", "set status"), got, want):
        bad = [(i, x, y if not isinstance(y, int) or name.endswith("results") else hex(y)) for i, (x, y) in enumerate(zip(a, b)) if x != y]
        assert not bad and len(a) == len(b), (name, what, bad[:8])


def compare(sets, rands, layout, lists=None, modes=None, sigs=None, base=None, **kw):
    """both forms of the new entry under every (grouping, route, split) of `modes` against the indexed batches entry -> its (results, status, set results, set status)"""
    from milagro_bls_amd import batch, _native as N
    base = base if base is not None else call_base(sets, rands, layout, lists=lists, sigs=sigs)
    for g, r, p in (modes if modes is not None else FULL):
        batch.set_vm_grouping(g); N.default_context().set_committee_route(r); batch.set_vm_span_split(p)
        got = call_new(sets, rands, layout, True, sigs=sigs, **kw)
        same(got, base, (g, r, p, layout[1:]))
        assert call_new(sets, rands, layout, False, sigs=sigs, **kw) == got[:2], (g, r, p)
    return base


def modes_for(n):
    return FULL if n in (3, 65) else diagonal(n)


# ---- 1. all-valid calls
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("n", COUNTS)
def test_all_valid_calls_equal_the_indexed_batches_entry(n, kind):
    sets = mixed(n, start=n)
    layout = cut(n, kind)
    res, st, sres, sst = compare(sets, scalars(n, n), layout, modes=modes_for(n))
    assert res == [1] * layout[2] and st == [0] * layout[2] and sres == [1] * n and sst == [0] * n


# ---- 2. one flipped participation bit
def bend(sets, where):
    """a copy of `sets` with the two-committee item (31 members all but the first: the complement route; 65 members, the first only: the direct route) in the
    middle, and one participation bit of it flipped -- a signer dropped from the complement segment, or a non-signer added to the direct one -> (sets, j, bits, lists)"""
    sets = list(sets)
    it = next(x.item for x in pool()[3]["multi"] if [len(TS.world().members[c]) for c in x.item.cids] == [31, 65])
    j = len(sets) // 2
    sets[j] = SP.as_set(it)
    t, flip = (0, it.sels[0][-1]) if where == "complement" else (1, 7)
    assert (flip in it.sels[t]) == (where == "complement") and (2 * len(it.sels[t]) > len(TS.world().members[it.cids[t]])) == (where == "complement")
    bent = Item(it.cids, [sorted(set(sel) ^ ({flip} if u == t else set())) for u, sel in enumerate(it.sels)], it.msg, it.tag)
    bits = b"".join(TS.field_of(bent) if i == j else x.field for i, x in enumerate(sets))
    lists = [TS.keys_of(bent) if i == j else x.keys for i, x in enumerate(sets)]
    return sets, j, bits, lists


@pytest.mark.parametrize("where", ("complement", "direct"))
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("n", (3, 65))
def test_one_flipped_participation_bit_rejects_its_batch_and_names_the_set(n, kind, where):
    sets, j, bits, lists = bend(mixed(n, start=n), where)
    layout = cut(n, kind)
    res, st, sres, sst = compare(sets, scalars(n, 100 + n), layout, lists=lists, bits=bits, modes=[(0, 0, 1), (1, 2, 4), (2, 1, 16), (0, 0, 0)])
    bj = owner_of(layout, n)[j]
    assert res == [0 if b == bj else 1 for b in range(layout[2])] and st == [PAIRING if b == bj else 0 for b in range(layout[2])]
    assert sres == [0 if i == j else 1 for i in range(n)] and sst == [PAIRING if i == j else 0 for i in range(n)]


# ---- 3. B separate calls of the one-call entry
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("n", (3, 65))
def test_calls_equal_one_call_of_the_span_entry_per_batch(n, kind):
    """ground truth that does not lean on the indexed entry: all valid, and with one set bent"""
    from milagro_bls_amd import batch
    layout = cut(n, kind)
    rands = scalars(n, 31 + n)
    plain = mixed(n, start=2 * n)
    bent, j, bits, _lists = bend(plain, "direct")
    for sets, b in ((plain, None), (bent, bits)):
        for g, p in ((0, 0), (1, 2), (2, 16)):
            batch.set_vm_grouping(g); batch.set_vm_span_split(p)
            want = call_loop(sets, rands, layout, bits=b)
            same(call_new(sets, rands, layout, True, bits=b), want, (g, p, kind))
    assert want[2] == [0 if i == j else 1 for i in range(n)]


def test_faults_that_would_cancel_in_a_merged_call_reject_both_batches():
    """two neighbouring batches hold the same two sets with their signatures exchanged across the boundary, under one scalar: merged into one call the two faults
    cancel (the signature sum is the same) and the call is accepted; as two batches both are rejected -- nothing crosses a batch boundary"""
    from milagro_bls_amd import batch
    fill = mixed(8, start=3)
    a, b = pool()[3]["multi"][0], pool()[3]["multi"][6]
    sets = fill[:3] + [a, b] + fill[3:]
    n = len(sets)
    rands = scalars(n, 12); rands[4] = rands[3]
    sigs = [x.sig for x in sets]; sigs[3], sigs[4] = sigs[4], sigs[3]
    assert SP.call_new(sets, rands, True, sigs=sigs)[:2] == (1, 0)            # the merged call cannot see it
    for layout in (([0, 4, n], 0, 2), ([0, 1, 4, 5, n], 0, 4), ([0, 3, 4, 5, 5, n], 0, 5)):
        bad = {owner_of(layout, n)[3], owner_of(layout, n)[4]}
        res, st, sres, sst = compare(sets, rands, layout, sigs=sigs, modes=[(0, 0, 0), (1, 1, 2), (2, 2, 16)])
        assert len(bad) == 2 and res == [0 if x in bad else 1 for x in range(layout[2])] and st == [PAIRING if x in bad else 0 for x in range(layout[2])]
        assert sres == [0 if i in (3, 4) else 1 for i in range(n)]
        for g, p in ((0, 0), (1, 4)):
            batch.set_vm_grouping(g); batch.set_vm_span_split(p)
            same(call_new(sets, rands, layout, True, sigs=sigs), call_loop(sets, rands, layout, sigs=sigs), (g, p, layout))


# ---- 3b. the split edges
@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("split", (2, 16))
def test_split_edges(split, kind):
    """test_gpu_vm_committee_span.test_split_edges' sets cut into batches: lists shorter than P (a single-key set, q = 0, nobody, first), of exactly P and P +- 1
    entries on either list, equal partial sums (the same id twice), partial sums that cancel (P0 and -P0) and an ineligible committee whose special member falls
    in the LAST chunk -- where a wrong chunk, or a wrong word among the partial sums' status words at their base behind the batches layout, would show. Under both
    forced routes and both forced groupings (and auto) against the indexed batches entry, and against one call of the span entry per batch"""
    from milagro_bls_amd import batch, _native as N
    valid, singles, edge, tags = pool()
    k = split
    sets = [singles[0], tags["q0"][0], tags["one_nobody"][2], tags["one_first"][7], edge["direct_%d" % (k - 1)], edge["direct_%d" % k], edge["direct_%d" % (k + 1)],
            edge["missing_%d" % (k - 1)], edge["missing_%d" % k], edge["missing_%d" % (k + 1)], tags["same_id_twice"][0], tags["sums_cancel"][0],
            edge["last_chunk_infinite"], edge["last_chunk_invalid"], edge["last_chunk_outside"], singles[1]]
    n = len(sets)
    layout = cut(n, kind)
    own = owner_of(layout, n)
    rands = scalars(n, 7 + split)
    modes = [(g, r, split) for g in (1, 2) for r in (1, 2)] + [(0, 0, split)]
    res, st, sres, sst = compare(sets, rands, layout, modes=modes)
    bad = [1, 2, 13, 14]                                          # q = 0 and nobody under a signature; the invalid member; the key outside G1
    assert [i for i in range(n) if not sres[i]] == bad
    assert res == [0 if b in {own[i] for i in bad} else 1 for b in range(layout[2])]
    assert not any(x & (ST["NO_KEYS"] | ST["APK_INFINITY"]) for x in st + sst)
    assert sst[11] == 0 and sres[11] == 1 and sst[10] == 0       # P0 + (-P0): infinity, and no bit says so
    assert sst[12] == ST["PK_INFINITY"] and sst[13] & BAD_PK and sst[14] == PAIRING
    for g, r, p in modes:
        batch.set_vm_grouping(g); N.default_context().set_committee_route(r); batch.set_vm_span_split(p)
        same(call_new(sets, rands, layout, True), call_loop(sets, rands, layout), (g, r, p, kind))


# ---- 4. one committee, one key
@pytest.mark.parametrize("split", (1, 2))
def test_sets_of_one_committee_and_single_key_sets_equal_the_committee_batches_entry(split):
    from milagro_bls_amd import batch, _native as N
    s = TS.world(); ctx = N.default_context(); L = N.lib()
    singles = pool()[1]
    sets = []
    for i, it in enumerate(s.pool[:s.n_single]):
        sets.append(SP.as_set(it))
        if i % 4 == 0:
            sets.append(singles[i % len(singles)])
    n = len(sets); rands = scalars(n, 12)
    batch.set_vm_span_split(split)
    for kind in CUTS:
        layout = cut(n, kind)
        boff, spb, B = layout
        for g, route in ((0, 0), (1, 1), (2, 2)):
            batch.set_vm_grouping(g); ctx.set_committee_route(route)
            d_s = TC.dev(b"".join(x.sig for x in sets)); d_ci = TC.i32([x.ids[0] if x.ids else 0 for x in sets]); d_b = TC.dev(b"".join(x.field for x in sets))
            d_mi = TC.i32([x.msg for x in sets]); d_r = i64(rands); d_o = TC.i32(boff) if boff is not None else None
            o = outputs(n, B)
            ctx.check(L.mbls_verify_multiple_batches_committee_msgtable_locate_device(ctx.handle, s.ct.handle, d_s.data_ptr(), d_ci.data_ptr(), d_b.data_ptr(), STRIDE,
                                                                                      s.w.mt.handle, d_mi.data_ptr(), d_r.data_ptr(), n,
                                                                                      d_o.data_ptr() if d_o is not None else None, spb, B, 0, o[0].data_ptr(),
                                                                                      o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), None))
            same(call_new(sets, rands, layout, True), read(n, B, o), (kind, g, route))


# ---- 5. malformed sets, indices, promises and tables on the device entries
@pytest.mark.parametrize("split", (0, 1, 4))
def test_each_malformed_kind_rejects_exactly_its_batch_and_is_named(split):
    """an id at the count, 65 ids, M > 8 * bits_stride, a bit-31 id among two, two single-key indices outside the key table, offsets past n_cmt_ids and offsets
    running backwards: as the indexed entry does on a set that lists 0xFFFFFFFF; the neighbours stand"""
    sets, ids, off, n_ids, lists, bad = SP.malformed_call()
    n = len(sets)
    for layout in ((None, 1, n), ([0, 1, 3, 4, 4, 6, 8, 10, 11, n], 0, 9), ([0, n], 0, 1)):
        own = owner_of(layout, n)
        res, st, sres, sst = compare(sets, scalars(n, 55), layout, lists=lists, ids=ids, off=off, n_ids=n_ids, modes=[(0, 0, split), (1, 2, split), (2, 1, split)])
        hit = {own[i] for i in bad}
        assert res == [0 if b in hit else 1 for b in range(layout[2])]
        assert all(bool(st[b] & BAD_PK) == (b in hit) for b in range(layout[2])) and all(st[b] == 0 for b in range(layout[2]) if b not in hit)
        assert [i for i in range(n) if not sres[i]] == bad and all(sst[i] & BAD_PK for i in bad) and all(sst[i] == 0 for i in range(n) if i not in bad)


def test_a_message_index_at_or_above_the_table_size():
    from milagro_bls_amd import batch
    n = 30
    sets = mixed(n, start=2)
    layout = cut(n, "tens")
    rands = scalars(n, 6)
    for bad_idx in (3, 0xFFFFFFFF):
        midx = [x.msg for x in sets]; midx[14] = bad_idx
        for g, p in ((0, 0), (1, 1), (2, 4)):
            batch.set_vm_grouping(g); batch.set_vm_span_split(p)
            res, st, sres, sst = call_new(sets, rands, layout, True, midx=midx)
            assert res == [1, 0, 1] and st == [0, BAD_MSG, 0]
            assert sres == [0 if i == 14 else 1 for i in range(n)] and sst == [BAD_MSG if i == 14 else 0 for i in range(n)]
            assert call_new(sets, rands, layout, False, midx=midx) == (res, st)


def test_a_max_groups_that_is_too_small_rejects_exactly_the_overflowing_batches():
    from milagro_bls_amd import batch
    n = 64
    sets = mixed(n, start=5)
    layout = cut(n, "tens")
    boff, _spb, B = layout
    rands = scalars(n, 8)
    goff = V.model([x.msg for x in sets], 3, B, None, boff)["off"]
    assert call_base(sets, rands, layout)[0] == [1] * B
    batch.set_vm_grouping(1)
    for split in (1, 4):
        batch.set_vm_span_split(split)
        for mg in (goff[-1], goff[-1] - 1, goff[3], 1):
            res, st, sres, sst = call_new(sets, rands, layout, True, max_groups=mg)
            over = [goff[b + 1] > mg for b in range(B)]
            assert res == [0 if o else 1 for o in over], (mg, res)
            assert [bool(x & BAD_MSG) for x in st] == over and all(x in (0, BAD_MSG) for x in st)
            assert sres == [1] * n
    assert any(goff[b + 1] > goff[3] for b in range(B))


def test_faulty_batch_tables_reject_what_the_batches_entry_rejects():
    n = 60
    sets = mixed(n, start=9)
    rands = scalars(n, 3)
    modes = [(0, 0, 0), (1, 0, 2)]
    for boff in ([0, 30, 20, 45, 60], [0, 10, 70, 60, 60], [0, 40, 10, 50, 61], [0, 60, 0, 60, 60], [60, 0, 0, 0, 0]):
        compare(sets, rands, (boff, 0, 4), modes=modes)
    res, st, _a, _b = compare(sets, rands, ([0, 20, 10, 30, 60], 0, 4), modes=modes)
    assert res == [0, 0, 0, 1] and st[1] & BAD_PK
    res, st, sres, sst = compare(sets, rands, ([5, 20, 20, 50, 55], 0, 4), modes=modes)
    assert res == [1, 1, 1, 1] and sres == [1 if 5 <= i < 55 else 0 for i in range(n)] and all(sst[i] & BAD_PK for i in (0, 4, 55, 59))


# ---- 6. a batch above the cap
def test_a_batch_larger_than_the_cap():
    """MBLS_VBG_MAX_SETS + 1 sets in one batch beside two small ones, mostly single-key sets: not grouped, the same verdict; with one span set of it bent, located"""
    valid, singles, _e, _t = pool()
    n = V.CAP + 1 + 7
    sets = [valid[(i // 16) % len(valid)] if i % 16 == 5 else singles[i % len(singles)] for i in range(n)]
    layout = ([0, 3, 3 + V.CAP + 1, n], 0, 3)
    rands = scalars(n, 41)
    modes = [(0, 0, 0), (1, 0, 1), (2, 0, 2)]
    res, st, sres, sst = compare(sets, rands, layout, modes=modes)
    assert res == [1, 1, 1] and sres == [1] * n
    j = next(i for i, x in enumerate(sets) if i > 500 and not x.single and x.tag == "multi" and len(x.keys) > 2)
    it = sets[j].item
    t = next(u for u in range(len(it.cids)) if len(it.sels[u]) > 1)
    bent = Item(it.cids, [sel[1:] if u == t else sel for u, sel in enumerate(it.sels)], it.msg, it.tag)
    bits = b"".join(TS.field_of(bent) if i == j else x.field for i, x in enumerate(sets))
    lists = [TS.keys_of(bent) if i == j else x.keys for i, x in enumerate(sets)]
    res, st, sres, sst = compare(sets, rands, layout, lists=lists, bits=bits, modes=modes)
    assert res == [1, 0, 1] and [i for i in range(n) if not sres[i]] == [j]


# ---- 7. host entries
def host_raw(sets, ids, off, n_ids, boff, spb, B, midx=None, stride=STRIDE, bits=None):
    """both _rng entries on raw arrays -> (return codes, batch bytes, set bytes, draws asked)"""
    from milagro_bls_amd import _native as N
    s = TS.world(); ctx = N.default_context(); L = N.lib(); n = len(sets)
    u32 = lambda v: (C.c_uint32 * max(1, len(v)))(*v)
    asked = []

    def source(_user, out, count):
        asked.append(int(count))
        for i in range(int(count)):
            out[i] = 3 + 2 * i
    cb = N.SCALAR_SOURCE(source)
    S = N.cbuf(b"".join(x.sig for x in sets)); Bf = N.cbuf(bits if bits is not None else b"".join(x.field for x in sets))
    mi = u32(midx if midx is not None else [x.msg for x in sets])
    res = N.outbuf(B); C.memset(res, 9, B); sres = N.outbuf(n); C.memset(sres, 7, n)
    bo = u32(boff) if boff is not None else None
    r0 = L.mbls_verify_multiple_batches_committee_span_msgtable_rng(ctx.handle, s.ct.handle, S, u32(ids), n_ids, u32(off), Bf, stride, s.w.mt.handle, mi, n, bo, spb, B, res,
                                                                    cb, None)
    r1 = L.mbls_verify_multiple_batches_committee_span_msgtable_locate_rng(ctx.handle, s.ct.handle, S, u32(ids), n_ids, u32(off), Bf, stride, s.w.mt.handle, mi, n, bo, spb,
                                                                           B, res, sres, None, cb, None)
    return (r0, r1), bytes(res)[:B], bytes(sres)[:n], asked


def test_host_entries_refuse_every_malformed_call_and_leave_the_outputs_unwritten():
    from milagro_bls_amd import _native as N
    s = TS.world(); w = s.w
    cid = {m: TC.SIZES.index(m) for m in TC.SIZES}
    sets = list(mixed(6, start=2))
    good_ids, good_off = arrays(sets)
    com = next(i for i, x in enumerate(sets) if not x.single); sg = next(i for i, x in enumerate(sets) if x.single)
    good = [0, 2, 6]

    def with_list(i, l):
        idl = [list(x.ids) for x in sets]; idl[i] = l
        ids, off = [], [0]
        for x in idl:
            ids += x; off.append(len(ids))
        return ids, off, len(ids)
    back = list(good_off); back[6] = back[5] - 1
    refused = (N.ERR_ARGUMENT, N.ERR_ARGUMENT)
    for ids, off, n_ids in [with_list(com, sets[com].ids + [len(s.members)]), with_list(com, [cid[1]] * 65), with_list(com, [cid[129], cid[129], cid[128]]),
                            with_list(com, [SINGLE | 5, cid[2]]), with_list(sg, [SINGLE | len(w.pk96)]), with_list(sg, [0xFFFFFFFF]),
                            (good_ids, back, len(good_ids)), (good_ids, good_off, len(good_ids) - 1)]:
        rc, res, sres, asked = host_raw(sets, ids, off, n_ids, good, 0, 2)
        assert rc == refused and res == b"\x09\x09" and sres == b"\x07" * 6 and asked == [], (ids[:6], off)
    for boff, spb in (([0, 4, 2], 0), ([0, 2, 5], 0), ([1, 2, 6], 0), (None, 4)):                      # a batch table that is not sound
        rc, res, sres, asked = host_raw(sets, good_ids, good_off, len(good_ids), boff, spb, 2)
        assert rc == refused and res == b"\x09\x09" and sres == b"\x07" * 6 and asked == [], boff
    rc, res, sres, asked = host_raw(sets, good_ids, good_off, len(good_ids), good, 0, 2, midx=[x.msg for x in sets[:3]] + [len(w.msgs)] + [0, 0])
    assert rc == refused and res == b"\x09\x09" and asked == []
    rc, res, sres, asked = host_raw(sets, good_ids, good_off, len(good_ids), good, 0, 2, stride=STRIDE + 2, bits=bytes((STRIDE + 2) * 6))
    assert rc == refused and res == b"\x09\x09" and asked == []
    rc, res, sres, asked = host_raw(sets, good_ids, good_off, len(good_ids), good, 0, 2)
    assert rc == (N.OK, N.OK) and res == b"\x01\x01" and sres == b"\x01" * 6 and asked == [6, 6]


@pytest.mark.parametrize("split", (0, 1, 8))
def test_rng_entries_draw_as_the_committee_batches_entry_does(split, vectors):
    """sets that both forms can state (one committee, or one key): a counting draw is asked for the same counts as
    mbls_verify_multiple_batches_committee_msgtable[_locate]_rng -- for every batch the sets in front of its first signature outside G2 -- and answers the same"""
    from milagro_bls_amd import batch
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    s = TS.world(); w = s.w
    singles = pool()[1]
    one = [SP.as_set(it) for it in s.pool[:s.n_single] if it.tag in SP.VALID_TAGS and TS.keys_of(it, s)]
    n = 24
    sets = [singles[i] if i % 5 in (1, 3) else one[(7 * i) % len(one)] for i in range(n)]
    boff = [0, 7, 7, 16, 24]; B = 4
    rands = scalars(n, 5)
    idl = [x.ids for x in sets]; fields = [x.field for x in sets]; midx = [x.msg for x in sets]
    words = [x.ids[0] for x in sets]; bits = b"".join(fields)
    batch.set_vm_span_split(split)
    for g, where in ((0, ()), (1, (9,)), (2, (0, 23)), (0, (7, 15, 16))):
        batch.set_vm_grouping(g)
        sigs = b"".join(probe if i in where else x.sig for i, x in enumerate(sets))
        asked_new, asked_loc, asked_old, asked_oldl = [], [], [], []
        draw = lambda log: (lambda count: (log.append(count), rands[:count])[1])
        got = batch.verify_multiple_batches_committee_span_msgtable_rng(s.ct, w.mt, sigs, idl, fields, STRIDE, midx, B, draw(asked_new), batch_offsets=boff)
        loc = batch.verify_multiple_batches_committee_span_msgtable_locate_rng(s.ct, w.mt, sigs, idl, fields, STRIDE, midx, B, draw(asked_loc), batch_offsets=boff)
        old = batch.verify_multiple_batches_committee_msgtable_rng(s.ct, w.mt, sigs, words, bits, STRIDE, midx, n, B, draw(asked_old), batch_offsets=boff)
        oldl = batch.verify_multiple_batches_committee_msgtable_locate_rng(s.ct, w.mt, sigs, words, bits, STRIDE, midx, n, B, draw(asked_oldl), batch_offsets=boff)
        reach = sum(min([i for i in where if boff[b] <= i < boff[b + 1]] + [boff[b + 1]]) - boff[b] for b in range(B))
        assert asked_new == asked_loc == asked_old == asked_oldl == ([reach] if reach else []), (where, asked_new, asked_old)
        assert got == old == loc[0] and loc == oldl
        assert got == [not any(boff[b] <= i < boff[b + 1] for i in where) for b in range(B)]


# ---- 8. the Python mirror
def test_python_mirror_agrees_and_leaves_the_generator_where_the_batches_method_does():
    from milagro_bls_amd import AggregateSignature, AggregatePublicKey, SingleKey
    s = TS.world(); w = s.w
    sets = [x for x in mixed(20, start=11) if x.tag != "sums_cancel"]        # (an aggregate key at infinity has no 96-byte form to spell out)
    n = len(sets)
    apks = SP.spelled_apks(sets)
    sig, apk = AggregateSignature, AggregatePublicKey
    used = lambda x: x.field[:(TS.total_bits(x.item) + 7) // 8]
    mine = [(sig(x.sig), SingleKey(x.ids[0] & 0x7FFFFFFF), None, x.msg) if x.single else (sig(x.sig), x.ids, used(x), x.msg) for x in sets]
    theirs = [(sig(x.sig), apk(a), w.msgs[x.msg]) for x, a in zip(sets, apks)]
    cuts = [0, 6, 6, 13, n]
    split = lambda xs: [xs[cuts[b]:cuts[b + 1]] for b in range(4)]
    r1, r2 = TV.CountingRng(4), TV.CountingRng(4)
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee_span_batches(r1, split(mine), s.ct, w.mt) == [True] * 4
    assert AggregateSignature.verify_multiple_aggregate_signatures_batches(r2, split(theirs)) == [True] * 4
    assert r1.calls == r2.calls > 0 and r1.r.random() == r2.r.random()
    # ... and agrees with the C entry on a bent set
    j = next(i for i, x in enumerate(sets) if i >= 6 and not x.single and len(x.keys) > 2 and x.tag.startswith(("one_", "multi")))
    f = bytearray(mine[j][2]); p = next(b for b in range(8 * len(f)) if (f[b >> 3] >> (b & 7)) & 1); f[p >> 3] ^= 1 << (p & 7)
    mine[j] = (mine[j][0], mine[j][1], bytes(f), mine[j][3])
    ok, per_set = AggregateSignature.verify_multiple_aggregate_signatures_committee_span_batches_locate(TV.CountingRng(4), split(mine), s.ct, w.mt)
    bj = 2 if j < 13 else 3
    assert ok == [b != bj for b in range(4)] and [x for b in per_set for x in b] == [i != j for i in range(n)]
    bits = b"".join(bytes(f).ljust(STRIDE, b"\0") if i == j else x.field for i, x in enumerate(sets))
    res, _st, sres, _sst = call_new(sets, scalars(n, 2), (cuts, 0, 4), True, bits=bits)
    assert [bool(x) for x in res] == ok and [bool(x) for x in sres] == [x for b in per_set for x in b]
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee_span_batches(TV.CountingRng(4), split(mine), s.ct, w.mt) == ok
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee_span_batches(TV.CountingRng(4), [], s.ct, w.mt) == []


# ---- 9. the workspace
def test_a_pre_reserved_workspace_changes_no_byte_and_the_plan_is_what_the_call_reserves():
    """P = 16 with locate on the grouped route, the largest layout: a fresh context holds the plan's items after one call (rounded up to whole waves, one spare
    item); a workspace reserved beforehand, larger than any call so far -- every region moves with the stride --, changes no output byte"""
    from milagro_bls_amd import batch, _native as N
    s = TS.world(); w = s.w
    for g, locate, split in ((1, True, 16), (2, True, 16), (1, False, 4), (2, False, 1)):
        other = N.Context(0)
        try:
            kt = N.KeyTable(other, capacity_hint=8); kt.append(b"".join(w.pk96[:4]), 4, pk_format=N.PK_UNCOMPRESSED, validate=False)
            ct = N.CommitteeTable(kt, capacity_hint=2); ct.append([0, 1, 2], [0, 3])
            mt = N.MsgTable(other, capacity_hint=4); mt.append(b"".join(w.msgs), 3, msg_len=32)
            other.check(N.lib().mbls_ctx_set_vm_grouping(other.handle, g)); other.check(N.lib().mbls_ctx_set_vm_span_split(other.handle, split))
            m, B = 40, 4
            some = mixed(m, start=1)
            call_new(some, [1] * m, (None, 10, B), locate, ids=[0] * m, off=list(range(m + 1)), bits=b"\x07\0\0\0" * m, midx=[i % 3 for i in range(m)], ctx=other, ct=ct,
                     mt=mt, stride=4)
            p, P = N.plan_verify_multiple_batches_committee_span(m, B, 10, 3, 0, g, locate, 32, split, limits=other.limits())
            assert P == split and p["route"] == (N.VM_ROUTE_GROUPED if g == 1 else N.VM_ROUTE_PER_SET)
            assert p["workspace_items"] == N.plan_verify_multiple_batches_committee(m, B, 10, 3, 0, g, locate, limits=other.limits())["workspace_items"] + (2 * P * m if P > 1 else 0)
            assert other.residue_regions()[1] == (p["workspace_items"] + 1 + 63) // 64 * 64, (g, locate, split)
            mt.close(); ct.close(); kt.close()
        finally:
            other.close()
    n = 200
    sets, j, bits, _lists = bend(mixed(n, start=9), "complement")
    rands = scalars(n, 77)
    layout = cut(n, "tens")
    batch.set_vm_grouping(1); batch.set_vm_span_split(16)
    before = (call_new(sets, rands, layout, True, bits=bits), call_new(sets, rands, layout, False, bits=bits))
    ctx = N.default_context()
    ctx.reserve_committee_span_items(3000, 400)
    p, P = N.plan_verify_multiple_batches_committee_span(n, layout[2], 0, len(w.mt), 0, 1, True, 352, 16, limits=ctx.limits())
    assert P == 16
    ctx.reserve(4 * p["workspace_items"])
    after = (call_new(sets, rands, layout, True, bits=bits), call_new(sets, rands, layout, False, bits=bits))
    assert after == before and [i for i in range(n) if not before[0][2][i]] == [j] and before[0][0] == [0 if b == j // 10 else 1 for b in range(layout[2])]


# ---- 10. no sets, no batches
def test_no_sets_and_no_batches_answer_as_the_batches_entry_does():
    from milagro_bls_amd import batch, _native as N
    s = TS.world(); ctx = N.default_context(); L = N.lib()
    for g in (0, 1, 2):
        batch.set_vm_grouping(g)
        assert call_new([], [], ([0, 0, 0, 0], 0, 3), True, ids=[], off=[0]) == call_base([], [], ([0, 0, 0, 0], 0, 3))
        assert call_new([], [], ([0, 0, 0, 0], 0, 3), True, ids=[], off=[0])[0] == [1, 1, 1]
        assert call_new([], [], (None, 0, 2), False, ids=[], off=[0]) == ([1, 1], [0, 0])
    o = outputs(0, 1)
    assert L.mbls_verify_multiple_batches_committee_span_msgtable_device(ctx.handle, s.ct.handle, None, None, 0, None, None, STRIDE, s.w.mt.handle, None, None, 0, None, 0, 0,
                                                                         0, o[0].data_ptr(), o[1].data_ptr(), None) == N.OK       # B = 0: nothing to answer
    assert read(0, 1, o)[:2] == ([9], [0x7fffffff])
    assert L.mbls_verify_multiple_batches_committee_span_msgtable_device(ctx.handle, s.ct.handle, None, None, 0, None, None, STRIDE, s.w.mt.handle, None, None, 4, None, 0, 0,
                                                                         0, o[0].data_ptr(), o[1].data_ptr(), None) == N.ERR_ARGUMENT      # sets without batches
    assert batch.verify_multiple_batches_committee_span_msgtable_rng(s.ct, s.w.mt, b"", [], [], STRIDE, [], 2, lambda c: [], batch_offsets=[0, 0, 0]) == [True, True]


def test_device_entries_refuse_bad_arguments():
    from milagro_bls_amd import _native as N
    s = TS.world(); ctx = N.default_context(); L = N.lib()
    n, B = 6, 2
    sets = mixed(n, start=2)
    ids, off = arrays(sets)
    d_s = TC.dev(b"".join(x.sig for x in sets)); d_ids = TC.i32(ids); d_off = TC.i32(off); d_b = TC.dev(b"".join(x.field for x in sets) + bytes(4))
    d_mi = TC.i32([x.msg for x in sets]); d_r = i64(scalars(n, 1)); o = outputs(n, B)
    g = L.mbls_verify_multiple_batches_committee_span_msgtable_device
    args = lambda bits=d_b.data_ptr(), stride=STRIDE, rands=d_r.data_ptr(), res=o[0].data_ptr(), spb=3, nb=B, offp=d_off.data_ptr(), ct=s.ct.handle, mt=s.w.mt.handle: (
        ctx.handle, ct, d_s.data_ptr(), d_ids.data_ptr(), len(ids), offp, bits, stride, mt, d_mi.data_ptr(), rands, n, None, spb, nb, 0, res, o[1].data_ptr(), None)
    assert g(*args(bits=d_b.data_ptr() + 1)) == N.ERR_ARGUMENT and g(*args(stride=STRIDE - 2)) == N.ERR_ARGUMENT
    assert g(*args(rands=None)) == N.ERR_ARGUMENT and g(*args(res=None)) == N.ERR_ARGUMENT and g(*args(offp=None)) == N.ERR_ARGUMENT
    assert g(*args(ct=None)) == N.ERR_ARGUMENT and g(*args(mt=None)) == N.ERR_ARGUMENT
    assert g(*args(spb=4)) == N.ERR_ARGUMENT and g(*args(nb=0)) == N.ERR_ARGUMENT
    assert L.mbls_verify_multiple_batches_committee_span_msgtable_locate_device(*args()[:18], None, None, None) == N.ERR_ARGUMENT       # d_set_results is required
    assert read(n, B, o) == ([9] * B, [0x7fffffff] * B, [9] * n, [0x7fffffff] * n)
    assert g(*args()) == N.OK and read(n, B, o)[:2] == ([1, 1], [0, 0])
