"""GPU tests of mbls_verify_multiple_batches* (include/mbls.h, "MANY verify_multiple BATCHES IN ONE CALL"): B independent batches of
AggregateSignature::verify_multiple_aggregate_signatures (reference src/aggregates.rs:261-316) in one call -- against the oracle, against the one-batch entries,
for isolation between batches, the reference's RNG order, the routing at scale and the argument handling."""
import ctypes as C
import random

import numpy as np
import pytest

import helpers
import orc

pytestmark = pytest.mark.gpu

G1_INF_U = bytes([0x40]) + bytes(95)
ST_PAIRING_FAILED = 0x40
REJECT_BATCH = 0x01 | 0x02 | 0x04 | 0x100 | 0x80          # the bits that reject a verify_multiple batch (mbls_coop.h COOP_REJECT_BATCH)


@pytest.fixture(scope="module")
def N():
    from milagro_bls_amd import _native
    _native.default_context()
    return _native


def _dev(b, dtype=np.uint8):
    import torch
    a = np.frombuffer(bytes(b), dtype=dtype).copy() if not isinstance(b, np.ndarray) else b
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


# ------------------------------------------------------------------------------------------------ the oracle-judged mix
SIZES_32 = [0, 1, 2, 3, 10, 64, 5, 1, 2, 3, 10, 64, 7, 0, 9, 1, 2, 3, 10, 33, 17, 0, 12, 6]
SIZES_RAGGED = [64, 3, 0, 10, 2, 1, 13, 64, 1, 2, 3, 10, 0, 8, 21, 4, 3, 10, 2, 1, 11, 19, 5, 0]
DEFECTS = ("wrong_key", "swapped_sig", "inf_sig", "inf_key", "both_inf", "not_in_g2", "undecodable", "zero_scalar")


class Mix:
    pass


def _build_mix(seed, sizes, ragged, probe):
    """every set has two keys: sig = [sk1 + sk2] H(msg), apk = pk1 + pk2 (aggregate-key form) = the wire keys (pk1, pk2) (wire-key form, k = 2).
    A third of the non-empty batches carry one defect each."""
    rnd = random.Random(seed)
    m = Mix()
    m.sizes, m.off = sizes, _offsets(sizes)
    n = m.off[-1]
    sks = [(rnd.randrange(1, helpers.R), rnd.randrange(1, helpers.R)) for _ in range(n)]
    flat = b"".join(s.to_bytes(32, "big") for pair in sks for s in pair)
    pk96 = orc.batch_sk_to_pk(flat, 2 * n, 1, nthreads=8)
    wire = [[pk96[192 * i:192 * i + 96], pk96[192 * i + 96:192 * i + 192]] for i in range(n)]
    apks = [orc.g1_add(w[0], w[1]) for w in wire]
    msgs = [rnd.randbytes(rnd.choice([0, 1, 31, 32, 33, 55, 56, 64, 65, 100, 200]) if ragged else 32) for _ in range(n)]
    sigs = [orc.g2_compress(orc.sign(mm, (a + b) % helpers.R)) for mm, (a, b) in zip(msgs, sks)]
    rands = [rnd.randrange(1, 1 << 63) for _ in range(n)]
    spare_wire = [orc.sk_to_pk(111), orc.sk_to_pk(222)]          # members of no batch: what a one-set batch takes its wrong key / wrong signature from
    spare_apk, spare_sig = orc.g1_add(*spare_wire), orc.g2_compress(orc.sign(b"spare", 999))
    nonempty = [b for b, s in enumerate(sizes) if s]
    bad = sorted(rnd.sample(nonempty, (len(sizes) + 2) // 3))
    m.defect = {}
    for t, b in enumerate(bad):
        d = DEFECTS[t % len(DEFECTS)]
        lo, hi = m.off[b], m.off[b + 1]
        i = rnd.randrange(lo, hi)
        other = (i + 1 - lo) % (hi - lo) + lo if hi - lo > 1 else None               # a neighbour inside the batch when it has one
        if d == "wrong_key":
            apks[i], wire[i] = (apks[other], list(wire[other])) if other is not None else (spare_apk, list(spare_wire))
        elif d == "swapped_sig":
            sigs[i] = sigs[other] if other is not None else spare_sig
        elif d == "inf_sig":
            sigs[i] = helpers.G2_INF
        elif d == "inf_key":
            apks[i] = G1_INF_U; wire[i] = [wire[i][0], orc.g1_mul(wire[i][0], helpers.R - 1)]
        elif d == "both_inf":
            sigs[i] = helpers.G2_INF; apks[i] = G1_INF_U; wire[i] = [wire[i][0], orc.g1_mul(wire[i][0], helpers.R - 1)]
        elif d == "not_in_g2":
            sigs[i] = probe
        elif d == "undecodable":
            sigs[i] = bytes([sigs[i][0] & 0x7F]) + sigs[i][1:]
        elif d == "zero_scalar":
            rands[i] = 0
        m.defect[b] = (d, i)
    m.n, m.B, m.sigs, m.apks, m.wire, m.msgs, m.rands, m.ragged = n, len(sizes), sigs, apks, wire, msgs, rands, ragged
    m.moff = _offsets([len(x) for x in msgs])
    # the oracle's answers, once per module: batch by batch, with the batch's own scalars
    m.want = []
    for b in range(m.B):
        lo, hi = m.off[b], m.off[b + 1]
        if any(r == 0 for r in rands[lo:hi]):
            m.want.append(False)                  # the reference never draws a zero (src/aggregates.rs:280-287); the ABI rejects it
            continue
        dec = [orc.g2_from_compressed(s) for s in sigs[lo:hi]]
        if any(e for e, _ in dec):
            m.want.append(False)
            continue
        m.want.append(orc.verify_multiple([(d[1], a, mm) for d, a, mm in zip(dec, apks[lo:hi], msgs[lo:hi])], rands[lo:hi]))
    return m


@pytest.fixture(scope="module")
def mixes(vectors):
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    return [_build_mix(2026, SIZES_32, False, probe), _build_mix(2027, SIZES_RAGGED, True, probe)]


class DevMix:
    """a mix resident on the device, in both key forms"""

    def __init__(self, m):
        self.sigs = _dev(b"".join(m.sigs)); self.apks = _dev(b"".join(m.apks)); self.wire = _dev(b"".join(k for w in m.wire for k in w))
        self.msgs = _dev(b"".join(m.msgs)); self.rands = _dev(np.array(m.rands, dtype=np.uint64))
        self.moff = _dev(np.array(m.moff, dtype=np.uint64)) if m.ragged else None
        self.boff = _dev(np.array(m.off, dtype=np.uint32))
        self.msg_len = 0 if m.ragged else 32

    def p(self, t):
        return None if t is None else t.data_ptr()


def _outputs(m):
    import torch
    return torch.full((max(1, m.B),), 7, dtype=torch.uint8, device="cuda:0"), torch.full((max(1, m.B),), -1, dtype=torch.int32, device="cuda:0")


def _run_batches(N, m, d, wire, stream=None, sync=True, out=None):
    import torch
    res, st = out or _outputs(m)
    ctx = N.default_context()
    rc = N.lib().mbls_verify_multiple_batches_device(ctx.handle, d.sigs.data_ptr(), None if wire else d.apks.data_ptr(), d.wire.data_ptr() if wire else None,
                                                     N.PK_UNCOMPRESSED, None, 2, d.msgs.data_ptr(), d.msg_len, d.p(d.moff), d.rands.data_ptr(), m.n,
                                                     d.boff.data_ptr(), 0, m.B, res.data_ptr(), st.data_ptr(), stream)
    assert rc == 0, ctx.last_error()
    if not sync:
        return res, st
    torch.cuda.synchronize()
    return [int(x) for x in res.cpu().numpy()[:m.B]], [int(x) & 0xFFFFFFFF for x in st.cpu().numpy()[:m.B]]


def _run_single(N, m, d, wire, b):
    """batch b alone through the existing one-batch _device entries, same scalars -> (bool byte, status word)"""
    import torch
    lo, hi = m.off[b], m.off[b + 1]
    res = torch.full((8,), 7, dtype=torch.uint8, device="cuda:0"); st = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    ctx = N.default_context()
    moff = None if d.moff is None else d.moff.data_ptr() + 8 * lo           # absolute offsets into the whole message buffer
    msgs = d.msgs.data_ptr() + (0 if d.moff is not None else 32 * lo)
    if wire:
        rc = N.lib().mbls_verify_multiple_sets_device(ctx.handle, d.sigs.data_ptr() + 96 * lo, d.wire.data_ptr() + 192 * lo, N.PK_UNCOMPRESSED, None, 2, msgs, d.msg_len, moff,
                                                      d.rands.data_ptr() + 8 * lo, hi - lo, res.data_ptr(), st.data_ptr(), None)
    else:
        rc = N.lib().mbls_verify_multiple_aggregate_signatures_device(ctx.handle, d.sigs.data_ptr() + 96 * lo, d.apks.data_ptr() + 96 * lo, msgs, d.msg_len, moff,
                                                                      d.rands.data_ptr() + 8 * lo, hi - lo, res.data_ptr(), st.data_ptr(), None)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    return int(res[0].item()), int(st[0].item()) & 0xFFFFFFFF


@pytest.mark.usefixtures("engine")
@pytest.mark.parametrize("which", [0, 1], ids=["msg32", "ragged"])
def test_mix_vs_oracle_and_single_batch_entries(N, mixes, which):
    """every results[b] equals the oracle's verify_multiple on that batch with the same scalars and the one-batch entry's bool; every status[b] equals the
    one-batch _device entry's word in every bit but MBLS_ST_PAIRING_FAILED, which is set exactly in the batches that carry no rejecting bit and are false"""
    m = mixes[which]
    d = DevMix(m)
    assert m.want.count(False) >= 6 and m.want.count(True) >= 12            # (both_inf batches stay true)
    for wire in (False, True):
        got, st = _run_batches(N, m, d, wire)
        assert got == [int(w) for w in m.want], (wire, [(b, m.sizes[b], m.defect.get(b)) for b in range(m.B) if got[b] != int(m.want[b])])
        for b in range(m.B):
            r1, s1 = _run_single(N, m, d, wire, b)
            assert r1 == got[b], (wire, b, m.defect.get(b))
            assert st[b] & ~ST_PAIRING_FAILED == s1 & ~ST_PAIRING_FAILED, (wire, b, m.defect.get(b), hex(st[b]), hex(s1))
            assert bool(st[b] & ST_PAIRING_FAILED) == (not (st[b] & REJECT_BATCH) and not got[b]), (wire, b, m.defect.get(b), hex(st[b]))
            if m.sizes[b] == 0:
                assert got[b] == 1 and st[b] == 0
    # the status words say why: the defects that are malformed members carry their bit, the others only the pairing verdict
    got, st = _run_batches(N, m, d, False)
    for b, (kind, _i) in m.defect.items():
        if kind == "not_in_g2":
            assert st[b] & 0x02 and not st[b] & ST_PAIRING_FAILED
        elif kind == "undecodable":
            assert st[b] & 0x01 and not st[b] & ST_PAIRING_FAILED
        elif kind == "zero_scalar":
            assert st[b] & 0x80 and not st[b] & ST_PAIRING_FAILED
        elif kind == "both_inf":
            assert got[b] == 1 and not st[b] & (ST_PAIRING_FAILED | REJECT_BATCH)
        else:
            assert got[b] == 0 and st[b] & ST_PAIRING_FAILED, (b, kind, hex(st[b]))
    # the host entry (aggregate keys) gives the same
    from milagro_bls_amd import batch
    hres, hst = batch.verify_multiple_batches(b"".join(m.sigs), b"".join(m.apks), b"".join(m.msgs), m.rands, m.n, m.B, batch_offsets=m.off,
                                              msg_len=0 if m.ragged else 32, msg_offsets=m.moff if m.ragged else None)
    assert [int(x) for x in hres] == got and hst == st


def test_uniform_layout_and_indexed_form(N, mixes):
    """sets_per_batch instead of a table, and the resident-key-table form: the same answers as the table / wire-key forms over the same sets"""
    import torch
    from milagro_bls_amd import batch
    m = mixes[0]
    # 21 batches of 3 sets cut from the mix's first sets, defects and all
    B, spb = 21, 3
    n = B * spb
    d = DevMix(m)
    rands = list(m.rands[:n]); rands[4] = 0                       # batch 1 is false whatever else the cut holds
    d_r = _dev(np.array(rands, dtype=np.uint64))
    res = torch.full((B,), 7, dtype=torch.uint8, device="cuda:0"); st = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    batch.verify_multiple_batches_device(d.sigs.data_ptr(), d.msgs.data_ptr(), d_r.data_ptr(), n, B, res.data_ptr(), st.data_ptr(), d_apks=d.apks.data_ptr(),
                                         sets_per_batch=spb)
    torch.cuda.synchronize()
    uni = [int(x) for x in res.cpu().numpy()]
    want, _ = batch.verify_multiple_batches(b"".join(m.sigs[:n]), b"".join(m.apks[:n]), b"".join(m.msgs[:n]), rands, n, B, batch_offsets=list(range(0, n + 1, spb)))
    assert uni == [int(x) for x in want] and uni[1] == 0 and 1 in uni
    # indexed: the wire keys of all sets appended to a table, set i = indices (2 i, 2 i + 1)
    tab = N.KeyTable()
    first, errs = tab.append(b"".join(k for w in m.wire for k in w), 2 * m.n, pk_format=N.PK_UNCOMPRESSED, validate=False)
    assert not any(errs)
    idx = _dev(np.arange(first, first + 2 * m.n, dtype=np.uint32))
    res2 = torch.full((m.B,), 7, dtype=torch.uint8, device="cuda:0"); st2 = torch.zeros(m.B, dtype=torch.int32, device="cuda:0")
    batch.verify_multiple_batches_indexed_device(tab, d.sigs.data_ptr(), idx.data_ptr(), d.msgs.data_ptr(), d.rands.data_ptr(), m.n, m.B, res2.data_ptr(), st2.data_ptr(), k=2,
                                                 d_batch_offsets=d.boff.data_ptr())
    torch.cuda.synchronize()
    assert [int(x) for x in res2.cpu().numpy()] == [int(w) for w in m.want]


# ------------------------------------------------------------------------------------------------ isolation
def _plain_sets(rnd, n):
    sks = [rnd.randrange(1, helpers.R) for _ in range(n)]
    pk96 = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for s in sks), n, 1, nthreads=8)
    pks = [pk96[96 * i:96 * i + 96] for i in range(n)]
    msgs = [rnd.randbytes(32) for _ in range(n)]
    sigs = [orc.g2_compress(orc.sign(mm, s)) for mm, s in zip(msgs, sks)]
    rands = [rnd.randrange(1, 1 << 63) for _ in range(n)]
    return pks, msgs, sigs, rands


def _host(sigs, pks, msgs, rands, off):
    from milagro_bls_amd import batch
    res, _ = batch.verify_multiple_batches(b"".join(sigs), b"".join(pks), b"".join(msgs), rands, len(sigs), len(off) - 1, batch_offsets=off)
    return res


def test_no_value_crosses_a_batch_boundary(N):
    """the forged pair (sig1 + D, sig2 - D) passes any check that sums the two signatures together: placed as the LAST set of batch b and the FIRST set of
    batch b + 1 both batches are false and all others true (a signature sum that leaked across the boundary would accept both); inside one batch the
    blinding rejects that batch. And flipping one batch at a time in a 33-batch call never changes another batch's result."""
    rnd = random.Random(77)
    sizes = [3, 1, 4, 2, 5, 1, 1, 3, 8, 2, 3]
    off = _offsets(sizes)
    pks, msgs, sigs, rands = _plain_sets(rnd, off[-1])
    assert _host(sigs, pks, msgs, rands, off) == [True] * len(sizes)
    D = orc.sign(b"d" * 32, 12345)
    negD = orc.g2_mul(D, helpers.R - 1)

    def forged(i, j):
        s = list(sigs)
        s[i] = orc.g2_compress(orc.g2_add(orc.g2_from_compressed(sigs[i])[1], D))
        s[j] = orc.g2_compress(orc.g2_add(orc.g2_from_compressed(sigs[j])[1], negD))
        return s
    for b in (0, 2, 4, 5, 8):                                     # last set of batch b, first set of batch b + 1 (batches of one set included)
        want = [x not in (b, b + 1) for x in range(len(sizes))]
        assert _host(forged(off[b + 1] - 1, off[b + 1]), pks, msgs, rands, off) == want, b
        # the same two sets with EQUAL scalars would cancel if they were summed together: still both false
        r = list(rands); r[off[b + 1]] = r[off[b + 1] - 1]
        assert _host(forged(off[b + 1] - 1, off[b + 1]), pks, msgs, r, off) == want, b
    for b in (2, 4, 8):                                           # the pair inside one batch
        assert _host(forged(off[b], off[b] + 1), pks, msgs, rands, off) == [x != b for x in range(len(sizes))], b
    # 33 batches, one flipped at a time
    sizes = [rnd.choice([1, 2, 3, 4]) for _ in range(33)]
    off = _offsets(sizes)
    pks, msgs, sigs, rands = _plain_sets(rnd, off[-1])
    assert _host(sigs, pks, msgs, rands, off) == [True] * 33
    for b in range(33):
        s = list(sigs)
        i = rnd.randrange(off[b], off[b + 1])
        s[i] = sigs[(i + 1) % off[-1]]                            # another set's signature: in G2, wrong
        assert _host(s, pks, msgs, rands, off) == [x != b for x in range(33)], b


# ------------------------------------------------------------------------------------------------ the reference's RNG order
def _rng_entry(N, sigs, pks, msgs, off, scalars):
    """mbls_verify_multiple_batches_rng with a counting source that hands out `scalars` in order -> (results, [counts asked for], the scalars handed out)"""
    asked, handed = [], []

    def draw(_user, out, count):
        for i in range(count):
            out[i] = scalars[i]; handed.append(scalars[i])
        asked.append(int(count))
    cb = N.SCALAR_SOURCE(draw)
    B = len(off) - 1
    res = N.outbuf(max(1, B))
    boff = (C.c_uint32 * len(off))(*off)
    ctx = N.default_context()
    rc = N.lib().mbls_verify_multiple_batches_rng(ctx.handle, N.cbuf(b"".join(sigs)), N.cbuf(b"".join(pks)), N.cbuf(b"".join(msgs)), 32, None, len(sigs), boff, 0, B, res, cb, None)
    assert rc == 0, ctx.last_error()
    return [bool(x) for x in bytes(res)[:B]], asked, handed


def test_rng_entry_keeps_the_reference_order(N, vectors):
    """the source is asked ONCE, for exactly sum_b (index of batch b's first signature outside G2, or its size) scalars, handed out in set order; and
    api.AggregateSignature.verify_multiple_aggregate_signatures_batches(rng, batches) returns what one verify_multiple_aggregate_signatures(rng, batch) call
    per batch returns and leaves random.Random(seed) in the same state"""
    from milagro_bls_amd import AggregateSignature, AggregatePublicKey
    probe = bytes.fromhex(vectors["model"]["g2_subgroup_probes"][0]["compressed"])
    rnd = random.Random(91)
    sizes = [4, 1, 6, 0, 5, 3]
    off = _offsets(sizes)
    n = off[-1]
    pks, msgs, sigs, rands = _plain_sets(rnd, n)
    cases = {
        "all good": [],
        "middle of a middle batch": [off[2] + 3],
        "set 0 of batch 0": [0],
        "every batch": [off[0] + 2, off[1], off[2] + 5, off[4], off[5] + 1],
        "two in one batch and a wrong (in G2) signature elsewhere": [off[2] + 1, off[2] + 4],
    }
    for name, bad in cases.items():
        s = list(sigs)
        for i in bad:
            s[i] = probe
        if name.startswith("two"):
            s[off[4]] = sigs[off[4] + 1]                          # rejected by the pairing check: every scalar of the batch is drawn
        reach = []
        for b in range(len(sizes)):
            firsts = [i - off[b] for i in bad if off[b] <= i < off[b + 1]]
            reach.append(min(firsts) if firsts else sizes[b])
        got, asked, handed = _rng_entry(N, s, pks, msgs, off, rands)
        assert asked == ([sum(reach)] if sum(reach) else []), (name, asked, reach)
        assert handed == rands[:sum(reach)]
        want = [not any(off[b] <= i < off[b + 1] for i in bad) for b in range(len(sizes))]
        if name.startswith("two"):
            want[4] = False
        assert got == want, name
        # in set order: the same results from the entry that takes the scalars, with the drawn ones placed where the reference would have used them
        placed, pos = [], 0
        for b in range(len(sizes)):
            placed += rands[pos:pos + reach[b]] + [1] * (sizes[b] - reach[b]); pos += reach[b]
        assert _host(s, pks, msgs, placed, off) == want, name
        # the Python mirror against one call per batch, on generators with the same seed
        batches = [[(AggregateSignature(s[i]), AggregatePublicKey(pks[i]), msgs[i]) for i in range(off[b], off[b + 1])] for b in range(len(sizes))]
        r1, r2 = random.Random(4242), random.Random(4242)
        one_call = AggregateSignature.verify_multiple_aggregate_signatures_batches(r1, batches)
        per_batch = [AggregateSignature.verify_multiple_aggregate_signatures(r2, b) for b in batches]
        assert one_call == per_batch == want, name
        assert r1.getstate() == r2.getstate(), name
    assert AggregateSignature.verify_multiple_aggregate_signatures_batches(random.Random(1), []) == []
    assert AggregateSignature.verify_multiple_aggregate_signatures_batches(random.Random(1), [[], []]) == [True, True]


# ------------------------------------------------------------------------------------------------ scale and routing
SHAPES = [(1024, 63), (1040, 63), (4, 20000), (2600, 1), (1, 33000)]


@pytest.mark.parametrize("B,spb", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_scale_and_routing_vs_single_batch_entry(N, B, spb):
    """1 024 x 63: sets + signature pairs are exactly one round; 1 040 x 63 crosses a round; 4 x 20 000: long ranges, more than a round; 2 600 x 1: as many
    signature pairs as sets; one batch of 33 000. A seeded handful of batches get a swapped signature (in G2, wrong): every batch is compared with the
    expectation by construction, and at least 64 seeded batches (all the damaged ones) with the existing one-batch _device entry on the same scalars."""
    import torch, bench
    ctx = N.default_context(); dev = torch.device("cuda:0")
    n = B * spb
    d_sigs, d_msgs, d_pks, _ = bench.build_inputs(ctx, dev, n, 1, N.PK_UNCOMPRESSED, rank=9, negatives=False)
    rnd = random.Random(1000 * B + spb)
    damaged = sorted(rnd.sample(range(B), max(1, min(5, B // 2))))
    sig_rows = d_sigs.view(n, 96).clone()
    for b in damaged:
        i = b * spb + rnd.randrange(spb)
        j = i + 1 if (i + 1) < (b + 1) * spb else (i - 1 if spb > 1 else (i + 1) % n)
        sig_rows[i] = d_sigs.view(n, 96)[j]
    d_s = sig_rows.contiguous()
    rands = np.array([rnd.randrange(1, 1 << 64) for _ in range(n)], dtype=np.uint64)
    d_r = _dev(rands)
    res = torch.full((B,), 7, dtype=torch.uint8, device=dev); st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    rc = N.lib().mbls_verify_multiple_batches_device(ctx.handle, d_s.data_ptr(), d_pks.data_ptr(), None, 0, None, 0, d_msgs.data_ptr(), 32, None, d_r.data_ptr(), n,
                                                     None, spb, B, res.data_ptr(), st.data_ptr(), None)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    got = [int(x) for x in res.cpu().numpy()]
    want = [0 if b in damaged else 1 for b in range(B)]
    assert got == want, [b for b in range(B) if got[b] != want[b]][:20]
    stw = [int(x) & 0xFFFFFFFF for x in st.cpu().numpy()]
    assert all((stw[b] == ST_PAIRING_FAILED) if b in damaged else (stw[b] == 0) for b in range(B)), [(b, hex(stw[b])) for b in range(B) if stw[b]][:10]
    # the same table given explicitly (device-side, all levels) agrees
    boff = _dev(np.arange(0, n + 1, spb, dtype=np.uint32))
    res2 = torch.full((B,), 7, dtype=torch.uint8, device=dev)
    rc = N.lib().mbls_verify_multiple_batches_device(ctx.handle, d_s.data_ptr(), d_pks.data_ptr(), None, 0, None, 0, d_msgs.data_ptr(), 32, None, d_r.data_ptr(), n,
                                                     boff.data_ptr(), 0, B, res2.data_ptr(), None, None)
    assert rc == 0, ctx.last_error()
    torch.cuda.synchronize()
    assert [int(x) for x in res2.cpu().numpy()] == want
    # one by one through the existing entry
    others = [b for b in range(B) if b not in damaged]
    rnd.shuffle(others)
    check = damaged + others[:max(0, 64 - len(damaged))]
    r1 = torch.full((8,), 7, dtype=torch.uint8, device=dev)
    for b in check:
        lo = b * spb
        rc = N.lib().mbls_verify_multiple_aggregate_signatures_device(ctx.handle, d_s.data_ptr() + 96 * lo, d_pks.data_ptr() + 96 * lo, d_msgs.data_ptr() + 32 * lo, 32, None,
                                                                      d_r.data_ptr() + 8 * lo, spb, r1.data_ptr(), None, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(r1[0].item()) == got[b], b
    assert len(check) >= min(B, 64)


def test_two_calls_on_two_streams_without_a_host_sync(N, mixes):
    """the device entry only enqueues and hands the workspace over on the device: two calls back to back on two streams give what they give alone"""
    import torch
    m0, m1 = mixes
    d0, d1 = DevMix(m0), DevMix(m1)
    oa, ob, oc = _outputs(m0), _outputs(m1), _outputs(m0)
    torch.cuda.synchronize()                                      # inputs and outputs exist before the side streams start
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ra, _ = _run_batches(N, m0, d0, False, stream=sa.cuda_stream, sync=False, out=oa)
    rb, _ = _run_batches(N, m1, d1, True, stream=sb.cuda_stream, sync=False, out=ob)
    rc, _ = _run_batches(N, m0, d0, True, stream=sa.cuda_stream, sync=False, out=oc)
    torch.cuda.synchronize()
    assert [int(x) for x in ra.cpu().numpy()[:m0.B]] == [int(w) for w in m0.want]
    assert [int(x) for x in rb.cpu().numpy()[:m1.B]] == [int(w) for w in m1.want]
    assert [int(x) for x in rc.cpu().numpy()[:m0.B]] == [int(w) for w in m0.want]


# ------------------------------------------------------------------------------------------------ argument handling
def test_argument_handling(N):
    import torch
    rnd = random.Random(5)
    pks, msgs, sigs, rands = _plain_sets(rnd, 6)
    ctx = N.default_context()
    S, A, M = N.cbuf(b"".join(sigs)), N.cbuf(b"".join(pks)), N.cbuf(b"".join(msgs))
    rr = (C.c_uint64 * 6)(*rands)
    f = N.lib().mbls_verify_multiple_batches
    res = N.outbuf(8); st = (C.c_uint32 * 8)()
    off = lambda *v: (C.c_uint32 * len(v))(*v)
    marker = bytes([9] * 8)
    C.memmove(res, marker, 8)
    assert f(ctx.handle, S, A, M, 32, None, None, 6, off(0, 2, 6), 0, 2, res, st) == N.ERR_ARGUMENT            # no scalars
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 2, 6), 0, 2, None, st) == N.ERR_ARGUMENT            # no results
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 4, 2, 6), 0, 3, res, st) == N.ERR_ARGUMENT          # runs backwards
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(1, 2, 6), 0, 2, res, st) == N.ERR_ARGUMENT             # does not start at 0
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 2, 5), 0, 2, res, st) == N.ERR_ARGUMENT             # does not end at n_sets
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, None, 4, 2, res, st) == N.ERR_ARGUMENT                      # 2 x 4 != 6
    assert bytes(res)[:8] == marker                                                                             # nothing written
    assert f(ctx.handle, S, A, M, 32, None, rr, 0, None, 0, 0, res, st) == 0 and bytes(res)[:8] == marker       # B = 0: OK, nothing written
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, off(0, 2, 6), 0, 2, res, st) == 0 and bytes(res)[:2] == b"\x01\x01" and list(st)[:2] == [0, 0]
    assert f(ctx.handle, S, A, M, 32, None, rr, 6, None, 3, 2, res, None) == 0 and bytes(res)[:2] == b"\x01\x01"
    # the rng form validates the same way and refuses a missing source
    g = N.lib().mbls_verify_multiple_batches_rng
    cb = N.SCALAR_SOURCE(lambda _u, out, count: [out.__setitem__(i, rands[i]) for i in range(count)] and None)
    assert g(ctx.handle, S, A, M, 32, None, 6, off(0, 7, 6), 0, 2, res, cb, None) == N.ERR_ARGUMENT
    assert g(ctx.handle, S, A, M, 32, None, 6, off(0, 2, 6), 0, 2, res, N.SCALAR_SOURCE(0), None) == N.ERR_ARGUMENT
    assert g(ctx.handle, S, A, M, 32, None, 6, off(0, 2, 6), 0, 2, res, cb, None) == 0 and bytes(res)[:2] == b"\x01\x01"
    # device entries: NULL scalars / NULL results are refused on the host, B = 0 writes nothing
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")
    d_s, d_a, d_m = t(b"".join(sigs)), t(b"".join(pks)), t(b"".join(msgs))
    d_r = _dev(np.array(rands, dtype=np.uint64)); d_o = _dev(np.array([0, 2, 6], dtype=np.uint32))
    d_res = torch.full((8,), 7, dtype=torch.uint8, device="cuda:0")
    fd = N.lib().mbls_verify_multiple_batches_device
    assert fd(ctx.handle, d_s.data_ptr(), d_a.data_ptr(), None, 0, None, 0, d_m.data_ptr(), 32, None, None, 6, d_o.data_ptr(), 0, 2, d_res.data_ptr(), None, None) == N.ERR_ARGUMENT
    assert fd(ctx.handle, d_s.data_ptr(), d_a.data_ptr(), None, 0, None, 0, d_m.data_ptr(), 32, None, d_r.data_ptr(), 6, d_o.data_ptr(), 0, 2, None, None, None) == N.ERR_ARGUMENT
    assert fd(ctx.handle, d_s.data_ptr(), d_a.data_ptr(), None, 0, None, 0, d_m.data_ptr(), 32, None, d_r.data_ptr(), 6, None, 4, 2, d_res.data_ptr(), None, None) == N.ERR_ARGUMENT
    assert fd(ctx.handle, d_s.data_ptr(), d_a.data_ptr(), None, 0, None, 0, d_m.data_ptr(), 32, None, d_r.data_ptr(), 0, None, 0, 0, d_res.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in d_res.cpu().numpy()] == [7] * 8
    # a faulty DEVICE-side table rejects the batches involved and nothing else: batch 1 runs backwards, batches 2 and 3 share set 4
    d_bad = _dev(np.array([0, 2, 1, 3, 5, 4, 6], dtype=np.uint32))          # ranges: [0,2) [2,1)! [1,3)~[0,2) share set 1 ...
    d_st = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    assert fd(ctx.handle, d_s.data_ptr(), d_a.data_ptr(), None, 0, None, 0, d_m.data_ptr(), 32, None, d_r.data_ptr(), 6, d_bad.data_ptr(), 0, 6, d_res.data_ptr(), d_st.data_ptr(), None) == 0
    torch.cuda.synchronize()
    # [0,2) and [1,3) share set 1; [2,1) runs backwards; [3,5) owns 3, 4 alone; [5,4) runs backwards; [4,6) shares set 4 with [3,5)
    assert [int(x) for x in d_res.cpu().numpy()[:6]] == [0, 0, 0, 0, 0, 0]
    d_ok = _dev(np.array([0, 2, 1, 3, 5, 6], dtype=np.uint32))              # [0,2) [2,1)! [1,3) [3,5) [5,6): only [3,5) and [5,6) are sound and alone
    assert fd(ctx.handle, d_s.data_ptr(), d_a.data_ptr(), None, 0, None, 0, d_m.data_ptr(), 32, None, d_r.data_ptr(), 6, d_ok.data_ptr(), 0, 5, d_res.data_ptr(), d_st.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert [int(x) for x in d_res.cpu().numpy()[:5]] == [0, 0, 0, 1, 1]
    assert [int(x) & 0x04 for x in d_st.cpu().numpy()[:5]] == [4, 4, 4, 0, 0]
