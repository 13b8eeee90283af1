"""GPU tests of committee spans (include/mbls.h, "committee spans"): mbls_fast_aggregate_verify_batch_committee_span[_msgtable][_device]. The keys, the key table,
the message table and the member lists are the committee tests' session world (test_gpu_committee.world); the span tests keep a committee table of their own over
the same key table -- the same committees under the same ids, and behind them one committee that holds P0 alone and one that holds -P0 alone -- and a pool of
signed span items. Every batch is compared with mbls_fast_aggregate_verify_batch_indexed[_msgtable]_device on the selected members spelled out in (segment, member)
order through a ragged offset table -- results, bitmap and status words equal --, under the three route modes and on both message forms, and every distinct item
the reference can hold goes to the oracle once per session."""
import random

import pytest

import test_gpu_committee as TC
from test_gpu_committee import NO_KEYS, APK_INF, PK_INF, BAD_PK, SIZES, NEG0, INVALID, MODES, FORMS, dev, i32, outputs, read_out

pytestmark = pytest.mark.gpu

STRIDE = 44                       # bytes per field: 352 bits cover the largest item of the pool (128 + 63 + 3 + 129 = 323), a multiple of 4
PATTERNS = ("nobody", "first", "last", "everybody", "all_but_first", "all_but_last", "half")


class Item:
    def __init__(self, cids, sels, msg, tag):
        self.cids, self.sels, self.msg, self.tag = list(cids), [sorted(s) for s in sels], msg, tag      # committee ids, selected member positions per segment
        self.cid = tuple(cids)
        self.sig = None


class World:
    pass


_S = None


def pattern(name, m, rnd):
    return {"nobody": [], "first": [0], "last": [m - 1], "everybody": list(range(m)), "all_but_first": list(range(1, m)), "all_but_last": list(range(m - 1)),
            "half": sorted(rnd.sample(range(m), m // 2))}[name]


def world():
    global _S
    if _S is not None:
        return _S
    from milagro_bls_amd import batch, _native as N
    w = TC.world()
    s = World()
    s.w = w
    rnd = random.Random(7549)
    s.members = [list(m) for m in w.members] + [[0], [NEG0]]
    s.P0, s.N0 = len(w.members), len(w.members) + 1
    s.ct = N.CommitteeTable(w.kt, capacity_hint=8)
    off = [0]
    for mem in s.members:
        off.append(off[-1] + len(mem))
    assert s.ct.append([x for mem in s.members for x in mem], off) == 0 and len(s.ct) == len(s.members)
    size = lambda c: len(s.members[c])
    cid = {m: SIZES.index(m) for m in SIZES}
    sp = w.sid
    full = lambda c: list(range(size(c)))
    pool = []
    # 1. spans of one committee: every plain committee under every pattern, the special ones full, first only and all but the first
    for c in range(len(SIZES)):
        for name in PATTERNS:
            pool.append(Item([c], [pattern(name, size(c), rnd)], (c + len(name)) % 3, "one_" + name))
    for name in ("pm", "ppm", "dup", "sum_inf4", "invalid", "infinite", "outside", "full_inf"):
        c = sp[name]
        pool += [Item([c], [full(c)], c % 3, "one_special_full"), Item([c], [[0]], (c + 1) % 3, "one_special_first"), Item([c], [full(c)[1:]], (c + 2) % 3, "one_special_rest")]
    s.n_single = len(pool)
    # 2. spans of two and three committees: boundaries at bits 1, 31, 33, 63, 65 and 129, independent patterns per segment
    multi = [((1, 64), ("everybody", "half")), ((31, 65), ("all_but_first", "first")), ((33, 32), ("half", "everybody")), ((63, 128), ("last", "all_but_last")),
             ((65, 33), ("everybody", "nobody")), ((129, 2), ("all_but_last", "everybody")), ((1, 32, 65), ("everybody", "all_but_first", "half")),
             ((31, 32, 2), ("half", "last", "first")), ((63, 2, 64), ("all_but_first", "everybody", "all_but_last")), ((129, 1, 2), ("first", "everybody", "last")),
             ((65, 64, 129), ("everybody", "everybody", "all_but_first")), ((33, 31, 1), ("nobody", "everybody", "nobody"))]
    for sizes, names in multi:
        pool.append(Item([cid[m] for m in sizes], [pattern(nm, m, rnd) for m, nm in zip(sizes, names)], len(sizes) % 3, "multi"))
    # 3. mixed routes in one item: everybody (complement), first only (direct), an ineligible committee fully selected (direct, its status bits), all but the first
    pool.append(Item([cid[128], cid[63], sp["infinite"], cid[129]], [full(cid[128]), [0], full(sp["infinite"]), full(cid[129])[1:]], 1, "mixed"))
    pool.append(Item([cid[128], cid[63], sp["outside"], cid[129]], [full(cid[128]), [0], full(sp["outside"]), full(cid[129])[1:]], 2, "mixed_outside"))
    pool.append(Item([cid[64], sp["invalid"], cid[65]], [full(cid[64]), full(sp["invalid"]), full(cid[65])[1:]], 0, "mixed_invalid"))
    # 4. a span of 64 committees: sizes 1, 2, 4, 2 sixteen times -- segment 63 has two members, both selected: complement in the automatic mode too
    ids64 = [cid[1], cid[2], sp["dup"], cid[2]] * 16
    pool.append(Item(ids64, [full(c) for c in ids64], 0, "span64_full"))
    pool.append(Item(ids64, [full(c) if t % 3 else full(c)[:1] for t, c in enumerate(ids64)], 1, "span64_mixed"))
    # 5. fix-up edges
    pool += [Item([cid[128], cid[128]], [full(cid[128])] * 2, 2, "same_id_twice"),
             Item([s.P0, s.N0], [[0], [0]], 0, "sums_cancel"), Item([cid[64], s.N0, s.P0], [full(cid[64]), [0], [0]], 1, "cancel_beside_signers"),
             Item([cid[33], cid[64]], [[], full(cid[64])[2:]], 2, "nobody_beside_signers"), Item([cid[128], cid[129]], [full(cid[128]), full(cid[129])], 0, "no_absentee"),
             Item([], [], 1, "q0")]
    # one signature per (signing key, message), then one aggregate per item over the spelled-out members that have a secret key
    nk = len(w.sks)
    one = batch.sign_batch(b"".join(w.sks[i].to_bytes(32, "big") for _ in range(3) for i in range(nk)), b"".join(w.msgs[j] for j in range(3) for _ in range(nk)), 3 * nk,
                           msg_len=32)
    s.sig_of = lambda key, msg: one[96 * (msg * nk + key):96 * (msg * nk + key) + 96]
    s.pool = pool
    sign(s, pool)
    s.by_tag = {}
    for i, it in enumerate(pool):
        s.by_tag.setdefault(it.tag, []).append(i)
    _S = s
    return s


def sign(s, items):
    from milagro_bls_amd import batch
    nk = len(s.w.sks)
    parts, off = [], [0]
    for it in items:
        parts += [s.sig_of(k, it.msg) for k in keys_of(it, s) if k < nk] or [s.sig_of(0, it.msg)]
        off.append(len(parts))
    agg, errs = batch.aggregate_signatures_batch(b"".join(parts), len(items), offsets=off)
    assert not any(errs)
    for i, it in enumerate(items):
        it.sig = agg[96 * i:96 * i + 96]


def keys_of(it, s=None):
    """the selected members spelled out in (segment, member) order"""
    s = s or world()
    return [s.members[c][j] for c, sel in zip(it.cids, it.sels) for j in sel]


def field_of(it, stride=STRIDE, stray=()):
    s = world()
    b = bytearray(stride)
    o = 0
    for c, sel in zip(it.cids, it.sels):
        for j in sel:
            b[(o + j) >> 3] |= 1 << ((o + j) & 7)
        o += len(s.members[c])
    for p in stray:
        b[p >> 3] |= 1 << (p & 7)
    return bytes(b)


def total_bits(it):
    s = world()
    return sum(len(s.members[c]) for c in it.cids)


def span_call(items, form, stride=STRIDE, ids=None, off=None, n_ids=None, bits=None):
    """the span device entry -> (results, status, bitmap bits); ids / off / n_ids / bits: the raw arrays where a test bends them"""
    from milagro_bls_amd import _native as N
    s = world(); w = s.w; ctx = N.default_context(); L = N.lib(); n = len(items)
    if ids is None:
        ids, off = [], [0]
        for it in items:
            ids += it.cids; off.append(len(ids))
    d_s = dev(b"".join(it.sig for it in items))
    d_ids = i32(ids); d_off = i32(off)
    d_b = dev(b"".join(field_of(it, stride) for it in items) if bits is None else bits)
    d_res, d_bm, d_st = outputs(n)
    n_ids = len(ids) if n_ids is None else n_ids
    if form == "msgtable":
        d_mi = i32([it.msg for it in items])
        ctx.check(L.mbls_fast_aggregate_verify_batch_committee_span_msgtable_device(ctx.handle, s.ct.handle, d_s.data_ptr(), w.mt.handle, d_mi.data_ptr(), d_ids.data_ptr(), n_ids,
                                                                                     d_off.data_ptr(), d_b.data_ptr(), stride, n, d_res.data_ptr(), d_bm.data_ptr(),
                                                                                     d_st.data_ptr(), None))
    else:
        d_m = dev(b"".join(w.msgs[it.msg] for it in items))
        ctx.check(L.mbls_fast_aggregate_verify_batch_committee_span_device(ctx.handle, s.ct.handle, d_s.data_ptr(), d_m.data_ptr(), 32, None, d_ids.data_ptr(), n_ids,
                                                                           d_off.data_ptr(), d_b.data_ptr(), stride, n, d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
    return read_out(n, d_res, d_bm, d_st)


def committee_call(items, form):
    """the one-committee device entry over the span tests' table, on items of one segment"""
    from milagro_bls_amd import _native as N
    s = world(); w = s.w; ctx = N.default_context(); L = N.lib(); n = len(items)
    d_s = dev(b"".join(it.sig for it in items)); d_ci = i32([it.cids[0] for it in items]); d_b = dev(b"".join(field_of(it) for it in items))
    d_res, d_bm, d_st = outputs(n)
    if form == "msgtable":
        d_mi = i32([it.msg for it in items])
        ctx.check(L.mbls_fast_aggregate_verify_batch_committee_msgtable_device(ctx.handle, s.ct.handle, d_s.data_ptr(), w.mt.handle, d_mi.data_ptr(), d_ci.data_ptr(),
                                                                                d_b.data_ptr(), STRIDE, n, d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
    else:
        d_m = dev(b"".join(w.msgs[it.msg] for it in items))
        ctx.check(L.mbls_fast_aggregate_verify_batch_committee_device(ctx.handle, s.ct.handle, d_s.data_ptr(), d_m.data_ptr(), 32, None, d_ci.data_ptr(), d_b.data_ptr(),
                                                                      STRIDE, n, d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
    return read_out(n, d_res, d_bm, d_st)


def host_call(items, form, stride=STRIDE, id_lists=None, fields=None):
    from milagro_bls_amd import batch
    s = world(); w = s.w
    id_lists = [it.cids for it in items] if id_lists is None else id_lists
    sigs = b"".join(it.sig for it in items); fields = [field_of(it, stride) for it in items] if fields is None else fields
    if form == "msgtable":
        return batch.fast_aggregate_verify_batch_committee_span_msgtable(s.ct, w.mt, sigs, [it.msg for it in items], id_lists, fields, stride)
    return batch.fast_aggregate_verify_batch_committee_span(s.ct, sigs, b"".join(w.msgs[it.msg] for it in items), id_lists, fields, stride)


@pytest.fixture(autouse=True)
def _route_back():
    yield
    from milagro_bls_amd import _native as N
    N.default_context().set_committee_route(0)


def check(items, form, mode, lists=None, **kw):
    """the span entry against the indexed entry on the spelled-out signers (`lists`: where the test bent an item) and every item against the oracle"""
    TC.set_mode(mode)
    new = span_call(items, form, **kw)
    lists = [keys_of(it) for it in items] if lists is None else lists
    old = TC.indexed_call(items, form, lists=lists)
    bad = [(i, items[i].tag, items[i].cids[:4], new[0][i], old[0][i], hex(new[1][i]), hex(old[1][i])) for i in range(len(items)) if (new[0][i], new[1][i]) != (old[0][i], old[1][i])]
    assert not bad, bad[:8]
    assert new[2] == old[2] == [int(x) for x in new[0]]
    TC.oracle_check(items, new[0], lists=lists)
    return new


def tagged(*tags):
    s = world()
    return [s.pool[i] for t in tags for i in s.by_tag[t]]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_spans_of_one_committee_equal_the_committee_entry(engine, mode, form):
    s = world()
    items = s.pool[:s.n_single]
    new = check(items, form, mode)
    assert new == committee_call(items, form)                  # (the route mode is still set)
    for i, it in enumerate(items):
        if not it.sels[0]:
            assert not new[0][i] and new[1][i] & NO_KEYS
        elif it.tag.startswith("one_") and it.cids[0] < len(SIZES):
            assert new[0][i] and new[1][i] == 0, (it.tag, it.cids)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_spans_of_two_and_three_committees(mode, form):
    items = tagged("multi")
    got, st, _ = check(items, form, mode)
    assert got == [True] * len(items) and st == [0] * len(items)


@pytest.mark.parametrize("form", FORMS)
def test_mixed_routes_in_one_item(form):
    """mode 0: complement, direct, an ineligible committee fully selected (direct: the infinity key's status bit, the invalid entry's rejection), complement"""
    from milagro_bls_amd import _native as N
    s = world()
    items = tagged("mixed", "mixed_outside", "mixed_invalid")
    got, st, _ = check(items, form, 0)
    assert got[0] and st[0] == PK_INF                          # the infinity key adds nothing and says so
    assert not got[1] and not st[1] & (BAD_PK | PK_INF)        # the key outside G1: a pairing failure
    assert not got[2] and st[2] & BAD_PK
    it = items[0]
    sizes = [len(s.members[c]) for c in it.cids]
    assert N.plan_committee_span(sizes, [1, 1, 0, 1], field_of(it), 0) == (0b1001, 1 + 3, 1)
    for mode in (1, 2):
        assert check(items, form, mode)[:2] == (got, st)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_a_span_of_64_committees_and_one_of_65(mode, form):
    from milagro_bls_amd import _native as N
    s = world()
    full64, mixed64 = tagged("span64_full", "span64_mixed")
    near = tagged("multi")[:2]
    items = [near[0], full64, mixed64, near[1]]
    got, st, _ = check(items, form, mode)
    assert got == [True] * 4 and st == [0] * 4
    if mode != 1:                                               # segment 63 goes complement: mask bit 63
        sizes = [len(s.members[c]) for c in full64.cids]
        assert N.plan_committee_span(sizes, [1] * 64, field_of(full64), mode)[0] >> 63 == 1
    # 65 ids: the same 64 and one more, the field unchanged -- rejected with the words of the one index 0xFFFFFFFF, the neighbours as before
    ids, off = [], [0]
    for k, it in enumerate(items):
        ids += it.cids + ([full64.cids[0]] if k == 1 else []); off.append(len(ids))
    lists = [keys_of(it) for it in items]; lists[1] = [0xFFFFFFFF]
    new = check(items, form, mode, lists=lists, ids=ids, off=off)
    assert new[0] == [True, False, True, True] and new[1][1] & BAD_PK and [new[1][i] for i in (0, 2, 3)] == [0, 0, 0]
    with pytest.raises(N.MblsError) as e:
        host_call(items, form, id_lists=[it.cids + ([full64.cids[0]] if k == 1 else []) for k, it in enumerate(items)])
    assert e.value.code == N.ERR_ARGUMENT
    assert host_call(items, form) == (got, st)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_fix_up_edges(mode, form):
    items = tagged("same_id_twice", "sums_cancel", "cancel_beside_signers", "nobody_beside_signers", "no_absentee", "q0")
    got, st, _ = check(items, form, mode)
    assert got == [True, False, True, True, True, False]
    assert st[0] == 0 and st[2] == 0 and st[3] == 0 and st[4] == 0
    assert st[1] & APK_INF and not st[1] & NO_KEYS             # P0 + (-P0): infinity from the final point under every mode
    assert st[5] & NO_KEYS                                      # q = 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_limits_of_the_field_the_ids_and_the_offsets(mode, form):
    """stride 20 (160 bits): M exactly 160 passes, M = 161 is rejected; an id at the count; offsets that run backwards; offsets past n_cmt_ids; stray bits.
    Every rejected item carries the words of an item that lists the one key index 0xFFFFFFFF, and its neighbours are untouched."""
    from milagro_bls_amd import _native as N
    s = world()
    c = {m: SIZES.index(m) for m in SIZES}
    stride = 20
    if "limits" not in s.by_tag:                                # signed once per session
        rnd = random.Random(160)
        mk = lambda cids, msg, tag: Item(cids, [pattern("all_but_first" if k else "half", len(s.members[x]), rnd) for k, x in enumerate(cids)], msg, tag)
        items = [mk([c[31], c[129]], 0, "exact"), mk([c[32], c[129]], 1, "one_above"), mk([c[33], c[64]], 2, "plain"), mk([c[2], c[1]], 0, "bad_id"),
                 mk([c[65], c[63]], 1, "plain2"), mk([c[2], c[1]], 2, "backwards"), mk([c[63], c[2]], 0, "after_backwards"), mk([c[2], c[33]], 1, "past_the_ids")]
        sign(s, items)
        s.by_tag["limits"] = items
    items = s.by_tag["limits"]
    assert total_bits(items[0]) == 8 * stride and total_bits(items[1]) == 8 * stride + 1
    # the raw arrays. Item 3's second id is the table's count. Item 5's range is [10, 9): backwards. Item 6's range [9, 11) shares id 9 with item 4 and is well
    # formed. Item 7's range [11, 14) ends past the 12 ids.
    ids = items[0].cids + items[1].cids + items[2].cids + [items[3].cids[0], len(s.members)] + items[4].cids + [items[6].cids[1], c[2]]
    off = [0, 2, 4, 6, 8, 10, 9, 11, 14]
    assert len(ids) == 12 and ids[9:11] == items[6].cids
    bits = b"".join(field_of(it, stride + 4)[:stride] for it in items)         # (item 1's last member has no bit in 20 bytes: it is rejected before the field is read)
    lists = [keys_of(it) for it in items]
    for i in (1, 3, 5, 7):
        lists[i] = [0xFFFFFFFF]
    new = check(items, form, mode, lists=lists, ids=ids, off=off, n_ids=12, bits=bits, stride=stride)
    assert new[0] == [True, False, True, False, True, False, True, False]
    for i in (1, 3, 5, 7):
        assert new[1][i] & BAD_PK
    assert [new[1][i] for i in (0, 2, 4, 6)] == [0] * 4
    # stray bits at and above M, a delimiter bit at M: nothing changes (item 0 fills its 20 bytes: its delimiter lies in the next byte, which a wider stride has)
    good = [items[0], items[2], items[4], items[6]]
    got, st, bm = span_call(good, form, stride=stride)
    assert got == [True] * 4 and st == [0] * 4
    stray = b"".join(field_of(it, stride, stray=range(total_bits(it), 8 * stride)) for it in good)
    assert span_call(good, form, stride=stride, bits=stray) == (got, st, bm)
    delim = b"".join(field_of(it, stride + 4, stray=[total_bits(it)]) for it in good)
    assert span_call(good, form, stride=stride + 4, bits=delim) == (got, st, bm)
    # the host entries refuse the call for what the device rejects per item
    with pytest.raises(N.MblsError) as e:
        host_call([items[0], items[1]], form, stride=stride, fields=[field_of(it, stride + 4)[:stride] for it in items[:2]])      # M one above 8 * bits_stride
    assert e.value.code == N.ERR_ARGUMENT
    with pytest.raises(N.MblsError) as e:
        host_call(good, form, stride=stride, id_lists=[good[0].cids, [good[1].cids[0], len(s.members)], good[2].cids, good[3].cids])      # an id at the count
    assert e.value.code == N.ERR_ARGUMENT
    assert host_call(good, form, stride=stride) == (got, st)


def test_arguments_the_entries_refuse():
    from milagro_bls_amd import _native as N
    s = world(); w = s.w; ctx = N.default_context(); L = N.lib()
    items = tagged("multi")[:4]
    n = 4
    ids, off = [], [0]
    for it in items:
        ids += it.cids; off.append(len(ids))
    d_s = dev(b"".join(it.sig for it in items)); d_m = dev(b"".join(w.msgs[it.msg] for it in items)); d_ids = i32(ids); d_off = i32(off)
    d_b = dev(bytes(STRIDE * n + 4)); d_res, d_bm, d_st = outputs(n)
    call = lambda bits_ptr, stride, off_ptr: L.mbls_fast_aggregate_verify_batch_committee_span_device(
        ctx.handle, s.ct.handle, d_s.data_ptr(), d_m.data_ptr(), 32, None, d_ids.data_ptr(), len(ids), off_ptr, bits_ptr, stride, n, d_res.data_ptr(), d_bm.data_ptr(),
        d_st.data_ptr(), None)
    assert call(d_b.data_ptr() + 1, STRIDE, d_off.data_ptr()) == N.ERR_ARGUMENT       # d_bits not 4-byte aligned
    assert call(d_b.data_ptr(), STRIDE - 2, d_off.data_ptr()) == N.ERR_ARGUMENT       # bits_stride not a multiple of 4
    assert call(d_b.data_ptr(), STRIDE, None) == N.ERR_ARGUMENT                       # no offsets
    import torch
    torch.cuda.synchronize()
    assert d_res.cpu().tolist() == [9] * n                                            # nothing written
    # n = 0: MBLS_OK, nothing needed
    assert L.mbls_fast_aggregate_verify_batch_committee_span_device(ctx.handle, s.ct.handle, None, None, 32, None, None, 0, None, None, STRIDE, 0, None, None, None, None) == N.OK
    assert host_call([], "per_item") == ([], []) and host_call([], "msgtable") == ([], [])
    ctx.reserve_committee_span_items(64, 352)
    assert L.mbls_ctx_reserve_committee_span_items(ctx.handle, 1, 64 * 2048 + 1) == N.ERR_ARGUMENT
    # the one-committee reserve call keeps its limit
    assert L.mbls_ctx_reserve_committee_items(ctx.handle, 1, 2049) == N.ERR_ARGUMENT


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_several_passes_give_every_pass_its_own_slice(mode, form):
    """round = 128 items, the pool cycled to 300 items on the lane engines with tracks from 32 items: a round, then a round and the remainder on the two tracks --
    three passes, each with its own slice of the offsets and the fields, the id array unmoved, and its own part of the span scratch"""
    from milagro_bls_amd import _native as N
    s = world(); ctx = N.default_context()
    items = [s.pool[(1 + 11 * i) % len(s.pool)] for i in range(300)]
    TC.set_mode(mode)
    want = TC.indexed_call(items, form, lists=[keys_of(it) for it in items])
    try:
        ctx.set_round_items(128)
        ctx.set_coop_max_items(0); ctx.set_coop_hash_max_items(0); ctx.set_tracks(32, 16)
        assert len(N.plan_batch(300, ctx.limits())[1]) >= 3
        TC.set_mode(mode)
        got = span_call(items, form)
        assert got == want
    finally:
        ctx.reset_tuning()
