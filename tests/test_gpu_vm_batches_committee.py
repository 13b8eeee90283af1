"""GPU tests of mbls_verify_multiple_batches_committee_msgtable[_locate]_device / _rng and mbls_vbg_group_probe (include/mbls.h, "MANY verify_multiple BATCHES PER
CALL OVER COMMITTEE BITFIELDS AND THE RESIDENT MESSAGE TABLE"). The world and the pool of sets are those of tests/test_gpu_vm_committee.py (136 key-table entries,
committees of 1 .. 129 members and the special ones, 3 table messages, committee sets and single-key sets mixed). Every call is compared with
mbls_verify_multiple_batches_locate_indexed_device on the same signatures, scalars and batch table with every set's signers spelled out in member order and every
set's message spelled out as the bytes of its table entry: every batch byte and word, every set byte and word, under the 3 x 3 modes of mbls_ctx_set_vm_grouping
and mbls_ctx_set_committee_route. The probe's arrays are held word for word to the model of tests/vbg_cases.py."""
import ctypes as C
import random

import pytest

import test_gpu_committee as TC
import test_gpu_vm_committee as VC
import vbg_cases as V

pytestmark = pytest.mark.gpu

STRIDE = TC.STRIDE
BAD_PK, PAIRING, BAD_MSG = VC.BAD_PK, VC.PAIRING, VC.BAD_MSG
COUNTS = (1, 2, 3, 63, 64, 65, 200)
CUTS = ("ones", "tens", "ragged")


@pytest.fixture(autouse=True)
def _modes_back():
    yield
    from milagro_bls_amd import batch, _native as N
    N.default_context().set_committee_route(0)
    batch.set_vm_grouping(0)


def cut(n, kind):
    """-> (batch offsets or None, sets_per_batch, n_batches): batches of 1 (uniform), of 10 (ragged table, the last one shorter), or seeded ragged ones with empty
    batches at both ends and in between"""
    if kind == "ones":
        return None, 1, n
    if kind == "tens":
        off = list(range(0, n, 10)) + [n]
        return off, 0, len(off) - 1
    rnd = random.Random(31 * n + 7)
    off = [0, 0]
    while off[-1] < n:
        off.append(min(n, off[-1] + rnd.choice([0, 1, 2, 5, 17, 40])))
    off.append(n)
    return off, 0, len(off) - 1


def outputs(n, B):
    import torch
    f8 = lambda k: torch.full((max(k, 1),), 9, dtype=torch.uint8, device="cuda:0")
    f32 = lambda k: torch.full((max(k, 1),), 0x7fffffff, dtype=torch.int32, device="cuda:0")
    return f8(B), f32(B), f8(n), f32(n)


def read(n, B, o):
    import torch
    torch.cuda.synchronize()
    u = lambda t, k: [x & 0xffffffff for x in t.cpu().tolist()[:k]]
    return o[0].cpu().tolist()[:B], u(o[1], B), o[2].cpu().tolist()[:n], u(o[3], n)


def call_new(sets, rands, layout, locate=True, max_groups=0, bits=None, midx=None, words=None):
    from milagro_bls_amd import _native as N
    w = TC.world(); ctx = N.default_context(); L = N.lib(); n = len(sets)
    off, spb, B = layout
    d_s = TC.dev(b"".join(s.sig for s in sets)); d_ci = TC.i32(words if words is not None else [s.word for s in sets])
    d_b = TC.dev(bits if bits is not None else b"".join(s.bits() for s in sets))
    d_mi = TC.i32(midx if midx is not None else [s.msg for s in sets]); d_r = VC.i64(rands)
    d_o = TC.i32(off) if off is not None else None
    o = outputs(n, B)
    head = (ctx.handle, w.ct.handle, d_s.data_ptr(), d_ci.data_ptr(), d_b.data_ptr(), STRIDE, w.mt.handle, d_mi.data_ptr(), d_r.data_ptr(), n,
            d_o.data_ptr() if d_o is not None else None, spb, B, max_groups, o[0].data_ptr(), o[1].data_ptr())
    if locate:
        ctx.check(L.mbls_verify_multiple_batches_committee_msgtable_locate_device(*head, o[2].data_ptr(), o[3].data_ptr(), None))
        return read(n, B, o)
    ctx.check(L.mbls_verify_multiple_batches_committee_msgtable_device(*head, None))
    return read(n, B, o)[:2]


def call_base(sets, rands, layout, lists=None):
    """mbls_verify_multiple_batches_locate_indexed_device on the spelled-out signers and message bytes"""
    from milagro_bls_amd import _native as N
    w = TC.world(); ctx = N.default_context(); L = N.lib(); n = len(sets)
    off, spb, B = layout
    lists = lists if lists is not None else [s.keys for s in sets]
    koff = [0]
    for l in lists:
        koff.append(koff[-1] + len(l))
    d_s = TC.dev(b"".join(s.sig for s in sets)); d_k = TC.i32([x for l in lists for x in l]); d_ko = TC.i32(koff)
    d_m = TC.dev(b"".join(w.msgs[s.msg] for s in sets)); d_r = VC.i64(rands)
    d_o = TC.i32(off) if off is not None else None
    o = outputs(n, B)
    ctx.check(L.mbls_verify_multiple_batches_locate_indexed_device(ctx.handle, w.kt.handle, d_s.data_ptr(), d_k.data_ptr(), d_ko.data_ptr(), 0, d_m.data_ptr(), 32, None,
                                                                   d_r.data_ptr(), n, d_o.data_ptr() if d_o is not None else None, spb, B, o[0].data_ptr(),
                                                                   o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), None))
    return read(n, B, o)


def compare(sets, rands, layout, lists=None, groupings=(0, 1, 2), routes=(0, 1, 2), **kw):
    """both forms of the new entry under every grouping x route mode against the baseline -> the baseline's (results, status, set results, set status)"""
    from milagro_bls_amd import batch, _native as N
    base = call_base(sets, rands, layout, lists=lists)
    for g in groupings:
        batch.set_vm_grouping(g)
        for r in routes:
            N.default_context().set_committee_route(r)
            got = call_new(sets, rands, layout, True, **kw)
            for name, a, b in zip(("results", "status", "set results", "set status"), got, base):
                bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
                assert not bad, (name, g, r, layout[1:], bad[:8])
            assert call_new(sets, rands, layout, False, **kw) == got[:2], (g, r)
    return base


def owner_of(layout, n):
    off, spb, B = layout
    if off is None:
        return [i // spb for i in range(n)]
    own = [None] * n
    for b in range(B):
        for i in range(off[b], off[b + 1]):
            own[i] = b
    return own


def test_probe_equals_the_model_word_for_word():
    from milagro_bls_amd import batch
    for idx, T, B, spb, off, _mg in V.cases():
        got = batch.vbg_group_probe(idx, T, B, batch_offsets=off, sets_per_batch=spb or 0)
        want = V.model(idx, T, B, spb, off)
        for name in ("pos", "status", "pos_lo", "pos_hi", "head", "entry", "count", "off"):
            assert got[name] == want[name], (name, len(idx), T, B, spb, off)


@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("n", COUNTS)
def test_all_valid_calls_equal_the_indexed_batches_entry(n, kind):
    sets = VC.mixed(n, start=n)
    layout = cut(n, kind)
    res, st, sres, sst = compare(sets, VC.scalars(n, n), layout)
    assert res == [1] * layout[2] and st == [0] * layout[2] and sres == [1] * n and sst == [0] * n


@pytest.mark.parametrize("kind", CUTS)
@pytest.mark.parametrize("n", COUNTS)
def test_one_flipped_participation_bit_rejects_its_batch_and_names_the_set(n, kind):
    w = TC.world()
    sets = list(VC.mixed(n, start=n))
    cand = [i for i, s in enumerate(sets) if s.sel is not None and s.word < len(TC.SIZES) and len(w.members[s.word]) >= 2]
    if not cand:
        valid, _s, _t = VC.pool()
        sets[0] = next(s for s in valid if s.word < len(TC.SIZES) and len(w.members[s.word]) >= 31)
        cand = [0]
    j = cand[len(cand) // 2]
    s = sets[j]; m = len(w.members[s.word])
    sel = sorted(set(s.sel) ^ {(m - 1) if n % 2 else 0}) or sorted(set(s.sel) ^ {1})
    bits = b"".join(TC.bits_of(sel) if i == j else x.bits() for i, x in enumerate(sets))
    lists = [[w.members[s.word][t] for t in sel] if i == j else x.keys for i, x in enumerate(sets)]
    layout = cut(n, kind)
    res, st, sres, sst = compare(sets, VC.scalars(n, 100 + n), layout, lists=lists, bits=bits)
    bj = owner_of(layout, n)[j]
    assert res == [0 if b == bj else 1 for b in range(layout[2])] and st == [PAIRING if b == bj else 0 for b in range(layout[2])]
    assert sres == [0 if i == j else 1 for i in range(n)] and sst == [PAIRING if i == j else 0 for i in range(n)]


def test_errors_that_cancel_only_inside_a_group():
    """(sig, pk, m) and (-sig, -pk, m) under ONE scalar in one batch: the group's key sum and the batch's signature sum are both the point at infinity; the same
    two sets in two batches are two groups"""
    _v, singles, _t = VC.pool()
    a = next(s for s in singles if s.keys == [0] and s.msg == 1)
    b = next(s for s in singles if s.keys == [TC.NEG0] and s.msg == 1)
    fill = VC.mixed(6, start=3)
    sets = fill[:2] + [a, b] + fill[2:]
    rands = VC.scalars(len(sets), 12); rands[3] = rands[2]
    for layout in (([0, 8], 0, 1), ([0, 2, 4, 8], 0, 3), ([0, 3, 8], 0, 2), (None, 2, 4)):
        res, st, sres, sst = compare(sets, rands, layout)
        assert res == [1] * layout[2] and sres == [1] * 8
    # the pair alone, and the pair with the second key NOT negated (the sums do not cancel: the batch is rejected, both sets are located)
    res, st, sres, sst = compare([a, b], [5, 5], ([0, 2], 0, 1))
    assert res == [1]
    wrong = VC.Set(a.word, None, b.msg, b.sig, a.keys, "single")
    res, st, sres, sst = compare([a, wrong], [5, 5], ([0, 2], 0, 1))
    assert res == [0] and sres == [1, 0]


def test_a_batch_larger_than_the_cap():
    """1 025 sets in one batch beside two small ones: not grouped (every set its own group), the same answers; with one set of it bent, located"""
    w = TC.world()
    n = V.CAP + 1 + 7
    sets = list(VC.mixed(n, start=1))
    layout = ([0, 3, 3 + V.CAP + 1, n], 0, 3)
    rands = VC.scalars(n, 41)
    res, st, sres, sst = compare(sets, rands, layout, routes=(0,))
    assert res == [1, 1, 1]
    j = next(i for i, s in enumerate(sets) if i > 500 and s.sel is not None and s.word < len(TC.SIZES) and len(s.sel) > 2)
    sel = sets[j].sel[1:]
    bits = b"".join(TC.bits_of(sel) if i == j else x.bits() for i, x in enumerate(sets))
    lists = [[w.members[x.word][t] for t in sel] if i == j else x.keys for i, x in enumerate(sets)]
    res, st, sres, sst = compare(sets, rands, layout, lists=lists, bits=bits, routes=(0,))
    assert res == [1, 0, 1] and [i for i in range(n) if not sres[i]] == [j]


def test_a_max_groups_that_is_too_small_rejects_exactly_the_overflowing_batches():
    from milagro_bls_amd import batch
    n = 64
    sets = VC.mixed(n, start=5)
    layout = cut(n, "tens")
    off, _spb, B = layout
    rands = VC.scalars(n, 8)
    goff = V.model([s.msg for s in sets], 3, B, None, off)["off"]
    base = call_base(sets, rands, layout)
    assert base[0] == [1] * B
    batch.set_vm_grouping(1)
    for mg in (goff[-1], goff[-1] - 1, goff[3], goff[1], 1):
        res, st, sres, sst = call_new(sets, rands, layout, True, max_groups=mg)
        over = [goff[b + 1] > mg for b in range(B)]
        assert res == [0 if o else 1 for o in over], (mg, res)
        assert [bool(x & BAD_MSG) for x in st] == over and all(x in (0, BAD_MSG) for x in st)
        # an overflowing batch is rejected as a batch; its sets are examined one by one and are sound
        assert sres == [1] * n
    assert any(goff[b + 1] > goff[3] for b in range(B))


def test_faulty_batch_tables_reject_what_the_batches_entry_rejects():
    n = 60
    sets = VC.mixed(n, start=9)
    rands = VC.scalars(n, 3)
    for off in ([0, 20, 10, 30, 60], [0, 30, 20, 45, 60], [5, 20, 20, 50, 55], [0, 10, 70, 60, 60], [0, 40, 10, 50, 61], [0, 60, 0, 60, 60], [60, 0, 0, 0, 0]):
        compare(sets, rands, (off, 0, 4), routes=(0,))
    res, st, _a, _b = compare(sets, rands, ([0, 20, 10, 30, 60], 0, 4), routes=(0,))
    assert res == [0, 0, 0, 1] and st[1] & BAD_PK                # [10, 30) overlaps [0, 20); [20, 10) runs backwards; [30, 60) is sound
    # sets nobody covers reject no batch: they read 0 with the table-fault bit, the batches around them stand
    res, st, sres, sst = compare(sets, rands, ([5, 20, 20, 50, 55], 0, 4), routes=(0,))
    assert res == [1, 1, 1, 1] and sres == [1 if 5 <= i < 55 else 0 for i in range(n)] and all(sst[i] & BAD_PK for i in (0, 4, 55, 59))


def test_a_message_index_at_or_above_the_table_size():
    from milagro_bls_amd import batch
    n = 30
    sets = VC.mixed(n, start=2)
    layout = cut(n, "tens")
    rands = VC.scalars(n, 6)
    base = call_base(sets, rands, layout)
    for bad_idx in (3, 0xFFFFFFFF):
        midx = [s.msg for s in sets]; midx[14] = bad_idx
        for g in (0, 1, 2):
            batch.set_vm_grouping(g)
            res, st, sres, sst = call_new(sets, rands, layout, True, midx=midx)
            assert res == [1, 0, 1] and st == [0, BAD_MSG, 0]
            assert sres == [0 if i == 14 else 1 for i in range(n)] and sst == [BAD_MSG if i == 14 else 0 for i in range(n)]
            assert call_new(sets, rands, layout, False, midx=midx) == (res, st)
    assert base[0] == [1, 1, 1]


def test_host_entries_refuse_malformed_calls_and_leave_the_outputs_unwritten():
    from milagro_bls_amd import _native as N
    w = TC.world(); ctx = N.default_context(); L = N.lib()
    n, B = 6, 2
    sets = VC.mixed(n, start=2)
    S = N.cbuf(b"".join(s.sig for s in sets)); Bf = N.cbuf(b"".join(s.bits() for s in sets))
    words = [s.word for s in sets]; midx = [s.msg for s in sets]
    asked = []
    cb = N.SCALAR_SOURCE(lambda _u, _out, count: asked.append(count))
    u32 = lambda v: (C.c_uint32 * len(v))(*v)
    sg = next(i for i, s in enumerate(sets) if s.sel is None); cm = next(i for i, s in enumerate(sets) if s.sel is not None)
    put = lambda i, v: words[:i] + [v] + words[i + 1:]
    good = [0, 2, 6]
    cases = [(put(cm, len(w.members)), midx, good, 0), (put(sg, VC.SINGLE | len(w.pk96)), midx, good, 0), (words, midx[:3] + [len(w.msgs)] + midx[4:], good, 0),
             (words, midx, [0, 4, 2], 0), (words, midx, [0, 2, 5], 0), (words, midx, [1, 2, 6], 0), (words, midx, None, 4)]
    for wl, mi, boff, spb in cases:
        res = N.outbuf(B); C.memset(res, 9, B); sres = N.outbuf(n); C.memset(sres, 7, n)
        bo = u32(boff) if boff is not None else None
        assert L.mbls_verify_multiple_batches_committee_msgtable_rng(ctx.handle, w.ct.handle, S, u32(wl), Bf, STRIDE, w.mt.handle, u32(mi), n, bo, spb, B, res, cb,
                                                                     None) == N.ERR_ARGUMENT
        assert L.mbls_verify_multiple_batches_committee_msgtable_locate_rng(ctx.handle, w.ct.handle, S, u32(wl), Bf, STRIDE, w.mt.handle, u32(mi), n, bo, spb, B, res,
                                                                            sres, None, cb, None) == N.ERR_ARGUMENT
        assert bytes(res)[:B] == b"\x09" * B and bytes(sres)[:n] == b"\x07" * n and asked == []
    res = N.outbuf(B); C.memset(res, 9, B)
    assert L.mbls_verify_multiple_batches_committee_msgtable_locate_rng(ctx.handle, w.ct.handle, S, u32(words), Bf, STRIDE, w.mt.handle, u32(midx), n, u32(good), 0, B, res,
                                                                        None, None, cb, None) == N.ERR_ARGUMENT         # set_results is required
    assert L.mbls_verify_multiple_batches_committee_msgtable_rng(ctx.handle, w.ct.handle, S, u32(words), Bf, STRIDE, w.mt.handle, u32(midx), n, u32(good), 0, B, res,
                                                                 N.SCALAR_SOURCE(), None) == N.ERR_ARGUMENT              # no scalar source
    assert bytes(res)[:B] == b"\x09" * B and asked == []
    # the device entries' argument checks
    d_s = TC.dev(b"".join(s.sig for s in sets)); d_ci = TC.i32(words); d_b = TC.dev(b"".join(s.bits() for s in sets) + bytes(4)); d_mi = TC.i32(midx)
    d_r = VC.i64(VC.scalars(n, 1)); o = outputs(n, B)
    g = L.mbls_verify_multiple_batches_committee_msgtable_device
    args = lambda bits=d_b.data_ptr(), stride=STRIDE, rands=d_r.data_ptr(), res=o[0].data_ptr(), spb=3, nb=B: (
        ctx.handle, w.ct.handle, d_s.data_ptr(), d_ci.data_ptr(), bits, stride, w.mt.handle, d_mi.data_ptr(), rands, n, None, spb, nb, 0, res, o[1].data_ptr(), None)
    assert g(*args(bits=d_b.data_ptr() + 1)) == N.ERR_ARGUMENT and g(*args(stride=16)) == N.ERR_ARGUMENT
    assert g(*args(rands=None)) == N.ERR_ARGUMENT and g(*args(res=None)) == N.ERR_ARGUMENT
    assert g(*args(spb=4)) == N.ERR_ARGUMENT and g(*args(nb=0)) == N.ERR_ARGUMENT                       # n != B x k; sets without batches
    assert L.mbls_verify_multiple_batches_committee_msgtable_locate_device(*args()[:16], None, None, None) == N.ERR_ARGUMENT     # d_set_results is required
    assert read(n, B, o) == ([9] * B, [0x7fffffff] * B, [9] * n, [0x7fffffff] * n)
    assert g(*args()) == N.OK and read(n, B, o)[:2] == ([1, 1], [0, 0])


def test_no_sets_and_no_batches_answer_as_the_batches_entry_does():
    from milagro_bls_amd import batch, _native as N
    w = TC.world(); ctx = N.default_context(); L = N.lib()
    for g in (0, 1, 2):
        batch.set_vm_grouping(g)
        # n = 0 with three (empty) batches: every batch is an empty iterator -- true
        assert call_new([], [], ([0, 0, 0, 0], 0, 3), True) == call_base([], [], ([0, 0, 0, 0], 0, 3))
        assert call_new([], [], ([0, 0, 0, 0], 0, 3), True)[0] == [1, 1, 1]
        assert call_new([], [], (None, 0, 2), False) == ([1, 1], [0, 0])
    o = outputs(0, 1)
    assert L.mbls_verify_multiple_batches_committee_msgtable_device(ctx.handle, w.ct.handle, None, None, None, STRIDE, w.mt.handle, None, None, 0, None, 0, 0, 0,
                                                                    o[0].data_ptr(), o[1].data_ptr(), None) == N.OK        # B = 0: nothing to answer
    assert read(0, 1, o)[:2] == ([9], [0x7fffffff])
    assert batch.verify_multiple_batches_committee_msgtable_rng(w.ct, w.mt, b"", [], b"", STRIDE, [], 0, 2, lambda c: [], batch_offsets=[0, 0, 0]) == [True, True]


@pytest.mark.parametrize("grouping", (0, 1, 2))
def test_rng_entries_draw_as_the_batches_entry_does(grouping, vectors):
    """a counting draw: asked for the same counts as mbls_verify_multiple_batches[_locate]_rng on the same signatures with aggregate keys and messages spelled
    out -- for every batch the sets in front of its first signature outside G2 --, and the same answers"""
    from milagro_bls_amd import batch, _native as N
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    w = TC.world(); ctx = N.default_context(); L = N.lib()
    n = 24
    sets = list(VC.mixed(n, start=40))
    off = [0, 7, 7, 16, 24]; B = 4
    rands = VC.scalars(n, 5)
    apks = VC.spelled_apks(sets)
    words = [s.word for s in sets]; bits = b"".join(s.bits() for s in sets); midx = [s.msg for s in sets]
    batch.set_vm_grouping(grouping)
    for where in ((), (9,), (0, 23), (7, 15, 16)):
        sigs = [probe if i in where else s.sig for i, s in enumerate(sets)]
        asked_new, asked_loc, asked_old = [], [], []
        draw = lambda log: (lambda count: (log.append(count), rands[:count])[1])
        got = batch.verify_multiple_batches_committee_msgtable_rng(w.ct, w.mt, b"".join(sigs), words, bits, STRIDE, midx, n, B, draw(asked_new), batch_offsets=off)
        res, sres, sst = batch.verify_multiple_batches_committee_msgtable_locate_rng(w.ct, w.mt, b"".join(sigs), words, bits, STRIDE, midx, n, B, draw(asked_loc),
                                                                                    batch_offsets=off)
        ores = N.outbuf(B); osres = N.outbuf(n); osst = (C.c_uint32 * n)()
        cb = batch._scalar_source(draw(asked_old))
        ctx.check(L.mbls_verify_multiple_batches_locate_rng(ctx.handle, N.cbuf(b"".join(sigs)), N.cbuf(b"".join(apks)), N.cbuf(b"".join(w.msgs[s.msg] for s in sets)), 32,
                                                            None, n, (C.c_uint32 * (B + 1))(*off), 0, B, ores, osres, osst, cb, None))
        reach = sum(min([i for i in where if off[b] <= i < off[b + 1]] + [off[b + 1]]) - off[b] for b in range(B))
        assert asked_new == asked_loc == asked_old == ([reach] if reach else []), (where, asked_new, asked_old)
        assert got == res == [bool(x) for x in bytes(ores)[:B]]
        assert sres == [bool(x) for x in bytes(osres)[:n]] and sst == list(osst)[:n]
        assert res == [not any(off[b] <= i < off[b + 1] for i in where) for b in range(B)]


def test_python_mirror_agrees_and_leaves_the_generator_where_the_batches_method_does():
    from milagro_bls_amd import AggregateSignature, AggregatePublicKey, SingleKey
    w = TC.world()
    n = 20
    sets = VC.mixed(n, start=11)
    apks = VC.spelled_apks(sets)
    sig, apk = AggregateSignature, AggregatePublicKey
    mine = [(sig(s.sig), SingleKey(s.word & 0x7FFFFFFF), None, s.msg) if s.sel is None else (sig(s.sig), s.word, TC.bits_of(s.sel)[:17], s.msg) for s in sets]
    theirs = [(sig(s.sig), apk(a), w.msgs[s.msg]) for s, a in zip(sets, apks)]
    cuts = [0, 6, 6, 13, 20]
    split = lambda xs: [xs[cuts[b]:cuts[b + 1]] for b in range(4)]
    r1, r2 = VC.CountingRng(4), VC.CountingRng(4)
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee_batches(r1, split(mine), w.ct, w.mt) == [True] * 4
    assert AggregateSignature.verify_multiple_aggregate_signatures_batches(r2, split(theirs)) == [True] * 4
    assert r1.calls == r2.calls > 0 and r1.r.random() == r2.r.random()
    j = next(i for i, s in enumerate(sets) if i >= 6 and s.sel is not None and len(s.sel) > 2)
    mine[j] = (mine[j][0], mine[j][1], TC.bits_of(sets[j].sel[1:]), mine[j][3])
    ok, per_set = AggregateSignature.verify_multiple_aggregate_signatures_committee_batches_locate(VC.CountingRng(4), split(mine), w.ct, w.mt)
    bj = 2 if j < 13 else 3
    assert ok == [b != bj for b in range(4)] and [x for b in per_set for x in b] == [i != j for i in range(n)]
    assert AggregateSignature.verify_multiple_aggregate_signatures_committee_batches(VC.CountingRng(4), [], w.ct, w.mt) == []


def test_a_pre_reserved_workspace_changes_no_byte_and_the_plan_is_what_the_call_reserves():
    from milagro_bls_amd import batch, _native as N
    w = TC.world()
    n = 200
    sets = list(VC.mixed(n, start=9)); rands = VC.scalars(n, 77)
    layout = cut(n, "tens")
    j = next(i for i, s in enumerate(sets) if s.sel is not None and s.word < len(TC.SIZES) and len(s.sel) > 2)
    bits = b"".join(TC.bits_of(s.sel[1:]) if i == j else s.bits() for i, s in enumerate(sets))
    # a fresh context with tables of its own: after one call its workspace holds exactly what the plan says (rounded up to whole waves, one spare item)
    for g, locate in ((1, True), (2, True), (1, False), (2, False)):
        other = N.Context(0)
        try:
            kt = N.KeyTable(other, capacity_hint=8); kt.append(b"".join(w.pk96[:4]), 4, pk_format=N.PK_UNCOMPRESSED, validate=False)
            ct = N.CommitteeTable(kt, capacity_hint=2); ct.append([0, 1, 2], [0, 3])
            mt = N.MsgTable(other, capacity_hint=4); mt.append(b"".join(w.msgs), 3, msg_len=32)
            other.check(N.lib().mbls_ctx_set_vm_grouping(other.handle, g))
            m, B = 40, 4
            d_s = TC.dev(b"".join(s.sig for s in sets[:m])); d_ci = TC.i32([0] * m); d_b = TC.dev(b"\x07\0\0\0" * m); d_mi = TC.i32([i % 3 for i in range(m)])
            d_r = VC.i64([1] * m); o = outputs(m, B)
            f = N.lib().mbls_verify_multiple_batches_committee_msgtable_locate_device if locate else N.lib().mbls_verify_multiple_batches_committee_msgtable_device
            tail = (o[2].data_ptr(), o[3].data_ptr(), None) if locate else (None,)
            other.check(f(other.handle, ct.handle, d_s.data_ptr(), d_ci.data_ptr(), d_b.data_ptr(), 4, mt.handle, d_mi.data_ptr(), d_r.data_ptr(), m, None, 10, B, 0,
                          o[0].data_ptr(), o[1].data_ptr(), *tail))
            read(m, B, o)
            p = N.plan_verify_multiple_batches_committee(m, B, 10, 3, 0, g, locate, limits=other.limits())
            assert p["route"] == (N.VM_ROUTE_GROUPED if g == 1 else N.VM_ROUTE_PER_SET)
            assert other.residue_regions()[1] == (p["workspace_items"] + 1 + 63) // 64 * 64, (g, locate)
            mt.close(); ct.close(); kt.close()
        finally:
            other.close()
    before = {}
    for g in (0, 1, 2):
        batch.set_vm_grouping(g)
        before[g] = (call_new(sets, rands, layout, True, bits=bits), call_new(sets, rands, layout, False, bits=bits))
    ctx = N.default_context()
    ctx.reserve_committee_items(3000, 400)
    ctx.reserve(8 * N.plan_verify_multiple_batches_committee(n, layout[2], 0, len(w.mt), 0, 1, True, limits=ctx.limits())["workspace_items"])
    for g in (0, 1, 2):
        batch.set_vm_grouping(g)
        assert (call_new(sets, rands, layout, True, bits=bits), call_new(sets, rands, layout, False, bits=bits)) == before[g]
    assert before[0] == before[1] == before[2] and [i for i in range(n) if not before[0][0][2][i]] == [j]
