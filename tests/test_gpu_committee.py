"""GPU tests of the committee table (include/mbls.h, "committee table"): mbls_committees_* and mbls_fast_aggregate_verify_batch_committee[_msgtable][_device].
Keys and signatures come from sk_to_pk_batch / sign_batch / aggregate_signatures_batch. Every batch is compared with
mbls_fast_aggregate_verify_batch_indexed[_msgtable]_device on the selected members spelled out in member order through a ragged offset table -- results, bitmap
and status words equal --, under the three route modes and on both message forms, and with the oracle item by item (every item whose keys the reference could
hold; every distinct item is put to the oracle once per session and the verdict shared). One world of keys,
committees and signed items is built once per session and shared."""
import random

import pytest

import bls12_381 as M
import edge_points as ep

pytestmark = pytest.mark.gpu

NO_KEYS, APK_INF, PK_INF, BAD_PK, PAIRING = 0x10, 0x08, 0x20, 0x04, 0x40
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 128, 129)
N_HONEST = 132
NEG0, INVALID, INFINITE, OUTSIDE = 132, 133, 134, 135          # key-table entries behind the honest keys
STRIDE = 20                                                     # bytes per bitfield: 160 bits cover the largest committee (129), a multiple of 4
MODES = (0, 1, 2)
FORMS = ("per_item", "msgtable")


class Item:
    def __init__(self, cid, sel, msg, tag):
        self.cid, self.sel, self.msg, self.tag = cid, sel, msg, tag       # committee id, selected member positions (sorted), message number
        self.sig = None


class World:
    pass


_W = None


def patterns(m, rnd):
    half = sorted(rnd.sample(range(m), m // 2))
    rest = [j for j in range(m) if j not in half]
    return [("nobody", []), ("first", [0]), ("last", [m - 1]), ("everybody", list(range(m))), ("all_but_first", list(range(1, m))),
            ("all_but_last", list(range(m - 1))), ("half", half), ("half_plus_one", sorted(half + rest[:1]))]


def world():
    """keys 0..131 honest, 132 = -key 0, 133 invalid, 134 infinity (unchecked), 135 a curve point outside G1 (unchecked); committees of every size and the special
    ones; a pool of signed items"""
    global _W
    if _W is not None:
        return _W
    from milagro_bls_amd import batch, _native as N
    rnd = random.Random(2048)
    w = World()
    sks = [rnd.randrange(1, M.R) for _ in range(N_HONEST)]
    sks.append(M.R - sks[0])                                    # the secret key of -P0
    w.sks = sks
    pk96 = batch.sk_to_pk_batch(b"".join(s.to_bytes(32, "big") for s in sks), len(sks), out_format=N.PK_UNCOMPRESSED)
    w.pk96 = [pk96[96 * i:96 * i + 96] for i in range(len(sks))]
    assert ep.g1_point(w.pk96[NEG0]) == M.g1_neg(ep.g1_point(w.pk96[0]))
    w.pk96 += [b"\xff" * 96, ep.G1_INF_U, ep.g1_bytes(ep.curve_point(rnd), 1)]
    w.kt = N.KeyTable(N.default_context(), capacity_hint=256)
    first, errs = w.kt.append(b"".join(w.pk96), len(w.pk96), pk_format=N.PK_UNCOMPRESSED, validate=False)
    assert first == 0 and [bool(e) for e in errs] == [False] * 133 + [True, False, False]
    w.msgs = [rnd.randbytes(32) for _ in range(3)]
    w.mt = N.MsgTable(N.default_context(), capacity_hint=8)
    assert w.mt.append(b"".join(w.msgs), 3, msg_len=32) == 0
    # committees
    w.members = [[(3 * c + j) % N_HONEST for j in range(m)] for c, m in enumerate(SIZES)]
    w.special = {"pm": [0, NEG0], "ppm": [0, 0, NEG0], "dup": [5, 6, 5, 7], "sum_inf4": [1, NEG0, 0, 2], "invalid": [0, 1, INVALID, 2], "infinite": [0, INFINITE, 1],
                 "outside": [0, OUTSIDE, 1, 2], "full_inf": [NEG0, 0]}
    w.sid = {}
    for name, mem in w.special.items():
        w.sid[name] = len(w.members); w.members.append(mem)
    w.ct = N.CommitteeTable(w.kt, capacity_hint=4)              # (a small hint: the appends below grow the table twice)
    off = [0]
    for mem in w.members[:7]:
        off.append(off[-1] + len(mem))
    assert w.ct.append([x for mem in w.members[:7] for x in mem], off) == 0
    pad = [9, 9, 9]                                             # an offset table that starts past 0
    off = [3]
    for mem in w.members[7:]:
        off.append(off[-1] + len(mem))
    assert w.ct.append(pad + [x for mem in w.members[7:] for x in mem], off) == 7 and len(w.ct) == len(w.members)
    assert w.ct.max_members == max(SIZES)
    # the item pool
    pool = []
    for c, m in enumerate(SIZES):
        for tag, sel in patterns(m, rnd):
            pool.append(Item(c, sel, (c + len(sel)) % 3, tag))
    sp = w.sid
    pool += [Item(sp["pm"], [0, 1], 0, "p_minus_p"), Item(sp["pm"], [0], 1, "pm_first"), Item(sp["ppm"], [0, 1], 2, "doubling_fixup"),
             Item(sp["ppm"], [0, 1, 2], 0, "ppm_all"), Item(sp["ppm"], [1, 2], 1, "ppm_inf_subset"), Item(sp["dup"], [0, 1, 2, 3], 2, "dup_all"),
             Item(sp["dup"], [0, 2], 0, "dup_twice"), Item(sp["dup"], [1, 2, 3], 1, "dup_all_but_first"), Item(sp["sum_inf4"], [0, 1, 2, 3], 0, "inf4_all"),
             Item(sp["sum_inf4"], [1, 2], 1, "inf4_pm"), Item(sp["sum_inf4"], [0, 1, 3], 2, "inf4_all_but_one"), Item(sp["full_inf"], [0, 1], 1, "full_inf_all"),
             Item(sp["full_inf"], [1], 2, "full_inf_one"),
             Item(sp["invalid"], [0, 1, 3], 0, "invalid_absent"), Item(sp["invalid"], [0, 1, 2, 3], 1, "invalid_selected"),
             Item(sp["infinite"], [0, 2], 2, "infinite_absent"), Item(sp["infinite"], [0, 1, 2], 0, "infinite_selected"), Item(sp["infinite"], [1], 1, "infinite_alone"),
             Item(sp["outside"], [0, 2, 3], 1, "outside_absent"), Item(sp["outside"], [0, 1, 2, 3], 2, "outside_selected")]
    # one signature per (signing key, message), then one aggregate per item over the selected members that have a secret key
    nk = len(sks)
    one = batch.sign_batch(b"".join(sks[i].to_bytes(32, "big") for _ in range(3) for i in range(nk)), b"".join(w.msgs[j] for j in range(3) for _ in range(nk)), 3 * nk,
                           msg_len=32)
    sig_of = lambda key, msg: one[96 * (msg * nk + key):96 * (msg * nk + key) + 96]
    parts, off = [], [0]
    for it in pool:
        signers = [w.members[it.cid][j] for j in it.sel if w.members[it.cid][j] < nk] or [0]
        parts += [sig_of(k, it.msg) for k in signers]
        off.append(len(parts))
    agg, errs = batch.aggregate_signatures_batch(b"".join(parts), len(pool), offsets=off)
    assert not any(errs)
    for i, it in enumerate(pool):
        it.sig = agg[96 * i:96 * i + 96]
    w.pool = pool
    w.by_tag = {}
    for i, it in enumerate(pool):
        w.by_tag.setdefault(it.tag, []).append(i)
    w.oracle = {}
    _W = w
    return w


def bits_of(sel, stray=()):
    b = bytearray(STRIDE)
    for j in list(sel) + list(stray):
        b[j >> 3] |= 1 << (j & 7)
    return bytes(b)


def dev(buf, dt=None):
    import torch
    return torch.frombuffer(bytearray(buf if buf else b"\0"), dtype=dt or torch.uint8).to("cuda:0")


def i32(vals):
    import torch
    return torch.tensor([x if x < 2 ** 31 else x - 2 ** 32 for x in vals] or [0], dtype=torch.int32, device="cuda:0")


def outputs(n):
    import torch
    d_res = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0"); d_bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda:0")
    d_st = torch.full((n,), 0x7fffffff, dtype=torch.int32, device="cuda:0")
    return d_res, d_bm, d_st


def read_out(n, d_res, d_bm, d_st):
    import torch
    torch.cuda.synchronize()
    got = [bool(x) for x in d_res.cpu().tolist()]
    bits = [(int(x) >> b) & 1 for x in d_bm.cpu().tolist() for b in range(64)][:n]
    return got, [x & 0xffffffff for x in d_st.cpu().tolist()], bits


def committee_call(items, form, cmt_idx=None, bits=None):
    """the committee device entry -> (results, status, bitmap bits)"""
    from milagro_bls_amd import _native as N
    w = world(); ctx = N.default_context(); L = N.lib(); n = len(items)
    d_s = dev(b"".join(it.sig for it in items))
    d_ci = i32([it.cid for it in items] if cmt_idx is None else cmt_idx)
    d_b = dev(b"".join(bits_of(it.sel) for it in items) if bits is None else bits)
    d_res, d_bm, d_st = outputs(n)
    if form == "msgtable":
        d_mi = i32([it.msg for it in items])
        ctx.check(L.mbls_fast_aggregate_verify_batch_committee_msgtable_device(ctx.handle, w.ct.handle, d_s.data_ptr(), w.mt.handle, d_mi.data_ptr(), d_ci.data_ptr(),
                                                                                d_b.data_ptr(), STRIDE, n, d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
    else:
        d_m = dev(b"".join(w.msgs[it.msg] for it in items))
        ctx.check(L.mbls_fast_aggregate_verify_batch_committee_device(ctx.handle, w.ct.handle, d_s.data_ptr(), d_m.data_ptr(), 32, None, d_ci.data_ptr(), d_b.data_ptr(),
                                                                      STRIDE, n, d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
    return read_out(n, d_res, d_bm, d_st)


def indexed_call(items, form, lists=None):
    """the indexed device entry on the selected members spelled out in member order (or on `lists`)"""
    from milagro_bls_amd import _native as N
    w = world(); ctx = N.default_context(); L = N.lib(); n = len(items)
    if lists is None:
        lists = [[w.members[it.cid][j] for j in it.sel] for it in items]
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    d_s = dev(b"".join(it.sig for it in items))
    d_k = i32([x for l in lists for x in l]); d_o = i32(off)
    d_res, d_bm, d_st = outputs(n)
    if form == "msgtable":
        d_mi = i32([it.msg for it in items])
        ctx.check(L.mbls_fast_aggregate_verify_batch_indexed_msgtable_device(ctx.handle, w.kt.handle, d_s.data_ptr(), w.mt.handle, d_mi.data_ptr(), d_k.data_ptr(),
                                                                              d_o.data_ptr(), n, 0, d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
    else:
        d_m = dev(b"".join(w.msgs[it.msg] for it in items))
        ctx.check(L.mbls_fast_aggregate_verify_batch_indexed_device(ctx.handle, w.kt.handle, d_s.data_ptr(), d_m.data_ptr(), 32, None, d_k.data_ptr(), d_o.data_ptr(), n, 0,
                                                                    d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
    return read_out(n, d_res, d_bm, d_st)


def set_mode(mode):
    from milagro_bls_amd import _native as N
    N.default_context().set_committee_route(mode)


@pytest.fixture(autouse=True)
def _route_back():
    yield
    from milagro_bls_amd import _native as N
    N.default_context().set_committee_route(0)


def check(items, form, mode, **kw):
    set_mode(mode)
    new = committee_call(items, form, **kw)
    old = indexed_call(items, form)
    bad = [(i, items[i].tag, items[i].cid, new[0][i], old[0][i], hex(new[1][i]), hex(old[1][i])) for i in range(len(items)) if (new[0][i], new[1][i]) != (old[0][i], old[1][i])]
    assert not bad, bad[:8]
    assert new[2] == old[2] == [int(x) for x in new[0]]
    oracle_check(items, new[0])
    return new


def oracle_verdict(sig96, msg, keys):
    """the oracle's fast_aggregate_verify of one (signature, message number, key-table indices) triple, cached for the session"""
    import orc
    w = world()
    k = (sig96, msg, tuple(keys))
    if k not in w.oracle:
        e, sig = orc.g2_from_compressed(sig96)
        assert e == 0
        w.oracle[k] = orc.fast_aggregate_verify(sig, w.msgs[msg], [w.pk96[x] for x in keys])
    return w.oracle[k]


def oracle_check(items, got, lists=None):
    """every item against the oracle on the keys its field names (`lists`: key-table indices per item, where the test changed the field or the id). Only an item
    that names a key the reference could not hold -- the invalid entry, an index outside the table -- is left out: the infinity key and the point outside G1 are
    keys from_uncompressed_bytes builds, and the oracle takes their bytes. Every distinct triple is computed once per session."""
    w = world()
    seen = 0
    for i, it in enumerate(items):
        keys = lists[i] if lists is not None else [w.members[it.cid][j] for j in it.sel]
        if any(x == INVALID or x >= len(w.pk96) for x in keys):
            continue
        assert got[i] == oracle_verdict(it.sig, it.msg, keys), (i, it.tag, it.cid)
        seen += 1
    return seen


def expectations(items, got, st):
    for i, it in enumerate(items):
        if not it.sel:                                           # (a committee of one has an empty "all but the first")
            assert not got[i] and st[i] & NO_KEYS, (i, hex(st[i]))
        elif it.tag in ("p_minus_p", "ppm_inf_subset", "inf4_pm", "full_inf_all"):
            assert not got[i] and st[i] & APK_INF and not st[i] & NO_KEYS, (it.tag, hex(st[i]))
        elif it.tag in ("first", "last", "everybody", "all_but_first", "all_but_last", "half", "half_plus_one", "doubling_fixup", "ppm_all", "dup_all", "dup_twice",
                        "dup_all_but_first", "inf4_all", "inf4_all_but_one", "pm_first", "full_inf_one", "invalid_absent", "infinite_absent", "outside_absent"):
            assert got[i] and st[i] == 0, (it.tag, it.cid, hex(st[i]))
        elif it.tag == "invalid_selected":
            assert not got[i] and st[i] & BAD_PK, hex(st[i])
        elif it.tag in ("infinite_selected", "infinite_alone"):
            assert st[i] & PK_INF, hex(st[i])
        elif it.tag == "outside_selected":
            assert not got[i] and st[i] & PAIRING, hex(st[i])


def batch_of(n, start=0, step=7):
    w = world()
    return [w.pool[(start + step * i) % len(w.pool)] for i in range(n)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_every_size_and_participation_against_the_indexed_entry_and_the_oracle(engine, mode, form):
    """the whole pool in one batch (committees of 1 .. 129 members x eight participation patterns, the exceptional and the ineligible committees): equal to the
    indexed entry word for word, the expected verdict per pattern, and the oracle on every item but the one that names the invalid entry: accepted items,
    MBLS_ST_NO_KEYS, MBLS_ST_APK_INFINITY, the infinity key (MBLS_ST_PK_INFINITY) and the pairing failure of the key outside G1"""
    w = world()
    got, st, _ = check(w.pool, form, mode)
    expectations(w.pool, got, st)
    assert oracle_check(w.pool, got) == len(w.pool) - 1
    for tag, verdict in (("infinite_selected", True), ("infinite_alone", False), ("outside_selected", False), ("p_minus_p", False), ("nobody", False)):
        assert got[w.by_tag[tag][-1]] == verdict, tag


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batches_mixing_committees(n, mode, form):
    items = batch_of(n, start=n, step=7)
    got, st, _ = check(items, form, mode)
    expectations(items, got, st)


def test_eligibility_sums_and_counts():
    """mbls_committees_get: the cached sum equals mbls_aggregate_public_keys over the members, the member count, the eligible flag"""
    from milagro_bls_amd import batch, _native as N
    w = world()
    for cid, mem in enumerate(w.members):
        s96, m, el = w.ct.get(cid)
        assert m == len(mem)
        assert el == (not any(x in (INVALID, INFINITE) for x in mem)), cid
        if INVALID in mem:
            continue
        want, st = batch.aggregate_public_keys_batch(b"".join(w.pk96[x] for x in mem), 1, k=len(mem), pk_format=N.PK_UNCOMPRESSED)
        assert s96 == want, cid
    assert w.ct.get(w.sid["full_inf"])[0] == ep.G1_INF_U
    with pytest.raises(N.MblsError):
        w.ct.get(len(w.members))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_a_signature_by_a_different_subset_is_a_pairing_failure_and_nothing_else(mode, form):
    """one bit flipped against the signers: nearly full and full 128-member fields (complement in the automatic mode), a half-full one (direct) and a small one"""
    w = world()
    c128 = SIZES.index(128)
    items = [w.pool[w.by_tag["all_but_first"][c128]], w.pool[w.by_tag["everybody"][c128]], w.pool[w.by_tag["half"][c128]], w.pool[w.by_tag["half_plus_one"][SIZES.index(33)]]]
    flips = [[j for j in it.sel if j != 5] if 5 in it.sel else it.sel + [5] for it in items]          # drop signer 5, or add non-signer 5
    flips[1] = [j for j in items[1].sel if j != 127]
    bits = b"".join(bits_of(f) for f in flips)
    set_mode(mode)
    got, st, bm = committee_call(items, form, bits=bits)
    assert got == [False] * 4 and st == [PAIRING] * 4 and bm == [0] * 4
    # the oracle on the members the flipped fields name, and the indexed entry on the same lists
    lists = [[w.members[it.cid][j] for j in sorted(f)] for it, f in zip(items, flips)]
    assert oracle_check(items, got, lists=lists) == 4
    assert indexed_call(items, form, lists=lists) == (got, st, bm)
    # and the honest fields of the same items pass
    got, st, _ = committee_call(items, form)
    assert got == [True] * 4 and st == [0] * 4 and oracle_check(items, got) == 4


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_stray_bits_above_the_size_change_nothing(mode, form):
    """every bit from the committee's size to the end of the field set (a Bitlist's delimiter among them)"""
    w = world()
    plain = check(w.pool, form, mode)
    stray = b"".join(bits_of(it.sel, stray=range(len(w.members[it.cid]), 8 * STRIDE)) for it in w.pool)
    assert committee_call(w.pool, form, bits=stray) == plain
    delim = b"".join(bits_of(it.sel, stray=[len(w.members[it.cid])]) for it in w.pool)
    assert committee_call(w.pool, form, bits=delim) == plain


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_a_committee_id_that_names_nothing(mode, form):
    """device entry: the item is rejected like one that lists a key index outside the table, its neighbours are untouched; host entry: the call is refused"""
    from milagro_bls_amd import batch, _native as N
    w = world()
    items = batch_of(70, start=3, step=5)
    ids = [it.cid for it in items]; ids[2] = len(w.members); ids[66] = 0xFFFFFFFF
    set_mode(mode)
    new = committee_call(items, form, cmt_idx=ids)
    lists = [[w.members[it.cid][j] for j in it.sel] for it in items]; lists[2] = [0xFFFFFFFF]; lists[66] = [0xFFFFFFFF]
    assert new == indexed_call(items, form, lists=lists)
    for i in (2, 66):
        assert not new[0][i] and new[1][i] & BAD_PK and not new[2][i]
    assert oracle_check(items, new[0], lists=lists) >= len(items) - 4          # (the two bad ids and the items that name the invalid entry have no oracle form)
    sigs = b"".join(it.sig for it in items); bits = b"".join(bits_of(it.sel) for it in items)
    host = (lambda ci: batch.fast_aggregate_verify_batch_committee_msgtable(w.ct, w.mt, sigs, [it.msg for it in items], ci, bits, STRIDE, len(items))) if form == "msgtable" \
        else (lambda ci: batch.fast_aggregate_verify_batch_committee(w.ct, sigs, b"".join(w.msgs[it.msg] for it in items), ci, bits, STRIDE, len(items)))
    with pytest.raises(N.MblsError) as e:
        host(ids)
    assert e.value.code == N.ERR_ARGUMENT
    good = committee_call(items, form)
    assert host([it.cid for it in items]) == (good[0], good[1])


def test_arguments_the_entries_refuse():
    from milagro_bls_amd import batch, _native as N
    w = world(); ctx = N.default_context(); L = N.lib()
    items = batch_of(4)
    sigs = b"".join(it.sig for it in items); msgs = b"".join(w.msgs[it.msg] for it in items); ids = [it.cid for it in items]
    for stride in (16, 18, 0):                                   # 128 bits do not cover 129 members; not a multiple of 4
        with pytest.raises(N.MblsError) as e:
            batch.fast_aggregate_verify_batch_committee(w.ct, sigs, msgs, ids, bytes(stride * 4), stride, 4)
        assert e.value.code == N.ERR_ARGUMENT
    d_b = dev(bytes(STRIDE * 4 + 4)); d_s = dev(sigs); d_m = dev(msgs); d_ci = i32(ids); d_res, d_bm, d_st = outputs(4)
    rc = L.mbls_fast_aggregate_verify_batch_committee_device(ctx.handle, w.ct.handle, d_s.data_ptr(), d_m.data_ptr(), 32, None, d_ci.data_ptr(), d_b.data_ptr() + 1, STRIDE, 4,
                                                             d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None)
    assert rc == N.ERR_ARGUMENT
    # n = 0: MBLS_OK, nothing written
    assert L.mbls_fast_aggregate_verify_batch_committee_device(ctx.handle, w.ct.handle, None, None, 32, None, None, None, STRIDE, 0, None, None, None, None) == N.OK
    assert batch.fast_aggregate_verify_batch_committee(w.ct, b"", b"", [], b"", STRIDE, 0) == ([], [])
    # appends that append nothing
    before = len(w.ct)
    for idx, off in (([0, 1, 2], [0, 2, 1]), ([0, 1], [0, 0, 2]), ([0] * 2049, [0, 2049]), ([0, len(w.kt)], [0, 2])):
        with pytest.raises(N.MblsError) as e:
            w.ct.append(idx, off)
        assert e.value.code == N.ERR_ARGUMENT
    assert len(w.ct) == before and w.ct.append([], [0]) == before
    with pytest.raises(N.MblsError):
        ctx.set_committee_route(3)


def test_a_key_table_destroyed_first_unbinds_the_committee_table():
    """the committee table outlives its key table as a handle that answers count, get and clear and refuses appends and verifications"""
    from milagro_bls_amd import batch, _native as N
    w = world()
    kt = N.KeyTable(N.default_context(), capacity_hint=4)
    kt.append(b"".join(w.pk96[:3]), 3, pk_format=N.PK_UNCOMPRESSED, validate=False)
    ct = N.CommitteeTable(kt, capacity_hint=2)
    try:
        assert ct.append([0, 1, 2], [0, 3]) == 0 and ct.max_members == 3
        before = ct.get(0)
        kt.close()
        assert len(ct) == 1 and ct.get(0) == before and ct.max_members == 3
        with pytest.raises(N.MblsError) as e:
            ct.append([0], [0, 1])
        assert e.value.code == N.ERR_ARGUMENT
        it = w.pool[0]
        with pytest.raises(N.MblsError) as e:
            batch.fast_aggregate_verify_batch_committee(ct, it.sig, w.msgs[it.msg], [0], bytes([7, 0, 0, 0]), 4, 1)
        assert e.value.code == N.ERR_ARGUMENT
        ct.clear()
        assert len(ct) == 0
    finally:
        ct.close()


def test_clear_then_append_reuses_the_ids():
    from milagro_bls_amd import _native as N
    w = world()
    ct = N.CommitteeTable(w.kt, capacity_hint=2)
    try:
        assert ct.append([0, 1, 2, 3, 4], [0, 2, 5]) == 0 and len(ct) == 2
        before = ct.get(1)
        ct.clear()
        assert len(ct) == 0
        with pytest.raises(N.MblsError):
            ct.get(0)
        assert ct.append([2, 3, 4], [0, 3]) == 0 and len(ct) == 1
        assert ct.get(0) == before                               # the same members: the same sum, now under id 0
        assert ct.append([7], [0, 1]) == 1
    finally:
        ct.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tracks", [False, True])
def test_a_small_round_gives_every_pass_its_own_slice(tracks, mode, form):
    """round = 128 items, a 300-item batch: two rounds and a remainder of 44 -- one after the other, or (lane engines, tracks from 32 items) the last round and the
    remainder side by side on the two tracks, each with its own slice of ids and bits and its own part of the scratch"""
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    items = batch_of(300, start=1, step=11)
    want = indexed_call(items, form)
    try:
        ctx.set_round_items(128)
        if tracks:
            ctx.set_coop_max_items(0); ctx.set_coop_hash_max_items(0); ctx.set_tracks(32, 16)
            mode_, passes = N.plan_batch(300, ctx.limits())
            assert mode_ in (N.BATCH_ROUND_BESIDE_REST, N.BATCH_TWO_HALVES) and len(passes) == 3
        else:
            assert N.plan_batch(300, ctx.limits())[0] == N.BATCH_ROUNDS_THEN_REST
        set_mode(mode)
        got = committee_call(items, form)
        assert got == want and oracle_check(items, got[0]) >= 290
    finally:
        ctx.reset_tuning()
