"""Seeded randomised GPU-vs-oracle cases, shared by the stress scripts (scripts/stress_parity.py, stress_vm.py, stress_tracks.py: long runs over many
seeds) and the suite's slices of them (tests/test_gpu_stress_slices.py): the same generators and the same checks. Every run_* function takes a seed,
runs its cases on the device and returns (work done, [mismatch descriptions]); an empty list means the device agreed everywhere."""
import ctypes as C
import random

import helpers
import orc

G1_INF_U = bytes([0x40]) + bytes(95)


def _probe(which=0):
    return bytes.fromhex(helpers.load_vectors()["model"]["g2_subgroup_probes"][which]["compressed"])


# ------------------------------------------------------------------------------------------------ fast_aggregate_verify either side of every engine crossover
PARITY_SHAPES = ((1, 3, 1), (63, 5, 0), (65, 2, 1), (129, 7, 1), (1000, 4, 1), (333, 16, 0), (1537, 3, 1))
BIG_SHAPES = ((8193, 2, 1), (2049, 9, 0))
ENGINES = ("default", "pairs", "lanes2pair", "waves")


def parity_shapes(seed, big=True):
    """(n, k, pk_format) of one seed: the small shapes always, the two above the cooperative engine's default range on every fourth seed"""
    return PARITY_SHAPES + (BIG_SHAPES if big and seed % 4 == 0 else ())


def set_engines(ctx, engines, n):
    """'default': the library's routing; 'pairs': the one-lane kernels in the form the batch size takes (lane pairs / split); 'lanes2pair': the two-pair
    loop of the headline; 'waves': the cooperative engine at any size, its message phase capped at 6 144 items above 8 192"""
    ctx.reset_tuning()
    if engines in ("pairs", "lanes2pair"):
        ctx.set_coop_max_items(0); ctx.set_coop_hash_max_items(0)
    if engines == "lanes2pair":
        ctx.set_lane_shaping(0, (1 << 64) - 1)
    elif engines == "waves":
        ctx.set_coop_max_items(1 << 20); ctx.set_coop_hash_max_items(1 << 20 if n <= 8192 else 6144)


def run_fav_engines(ctx, seed, nthreads, big=True, shapes=None):
    """Every shape of the seed (make_batch: seven rejection classes on every fourth item) under each of ENGINES, every item against the oracle"""
    from milagro_bls_amd import batch as mb
    items, bad = 0, []
    for n, k, fmt in (shapes or parity_shapes(seed, big)):
        b = helpers.make_batch(n, k, fmt=fmt, seed=seed * 7 + n, pool_n=64, nthreads=nthreads)
        want = orc.batch_fast_aggregate_verify(b.sigs, b.msgs, b.pks, b.n, b.k, fmt, nthreads=nthreads)
        if want != b.expect:
            bad.append("oracle against construction: seed %d n %d k %d fmt %d" % (seed, n, k, fmt))
        for engines in ENGINES:
            try:
                set_engines(ctx, engines, n)
                got, _ = mb.fast_aggregate_verify_batch(b.sigs, b.msgs, b.pks, b.n, b.k, pk_format=fmt)
            finally:
                ctx.reset_tuning()
            items += n
            if got != want:
                bad.append("fast_aggregate_verify seed %d n %d k %d fmt %d %s: items %s" % (seed, n, k, fmt, engines, [i for i in range(n) if got[i] != want[i]][:8]))
    return items, bad


def run_sign_keys(ctx, seed, nthreads):
    """257 .. 320 secret keys: device signatures and compressed public keys byte-identical to the oracle's; the device's Signature::verify accepts them"""
    from milagro_bls_amd import batch as mb
    rnd = random.Random(seed)
    n = 257 + seed % 64
    sk = b"".join(rnd.randrange(1, helpers.R).to_bytes(32, "big") for _ in range(n))
    msgs = rnd.randbytes(32 * n)
    sigs = mb.sign_batch(sk, msgs, n); pks = mb.sk_to_pk_batch(sk, n)
    bad = []
    if sigs != orc.batch_sign(sk, msgs, n, nthreads=nthreads):
        bad.append("sign_batch seed %d n %d" % (seed, n))
    if pks != orc.batch_sk_to_pk(sk, n, 0, nthreads=nthreads):
        bad.append("sk_to_pk_batch seed %d n %d" % (seed, n))
    res, _ = mb.verify_batch(sigs, msgs, pks, n, pk_format=0)
    if not all(res):
        bad.append("verify of device-made signatures seed %d: items %s" % (seed, [i for i in range(n) if not res[i]][:8]))
    return 2 * n, bad


# ------------------------------------------------------------------------------------------------ the n-pairing paths, shards, two contexts
def run_vm_shards(ctx, m2, dev, seed, nthreads):
    """verify_multiple at 1 / 9 / 70 / 260 sets with one random spoil, through the one-call entry, the two-context handle m2 and the shard records
    (verify_multiple_partial_device cut at random points + verify_multiple_finish_device), against the oracle with the same scalars; then one batched
    aggregate_verify of 40 ragged items with spoiled members, item by item against the oracle"""
    import torch
    from milagro_bls_amd import _native as N, batch as mb
    probe = _probe(0)
    t = lambda b: torch.frombuffer(bytearray(b if b else b"\0"), dtype=torch.uint8).to(dev)
    rnd = random.Random(seed * 13)
    work, bad = 0, []
    for n in (1, 9, 70, 260):
        sks = [rnd.randrange(1, helpers.R) for _ in range(n)]
        pk96 = orc.batch_sk_to_pk(b"".join(x.to_bytes(32, "big") for x in sks), n, 1, nthreads=nthreads)
        pks = [pk96[96 * i:96 * i + 96] for i in range(n)]
        msgs = [rnd.randbytes(32) for _ in range(n)]
        sg = orc.batch_sign(b"".join(x.to_bytes(32, "big") for x in sks), b"".join(msgs), n, nthreads=nthreads)
        sigs = [sg[96 * i:96 * i + 96] for i in range(n)]
        rands = [rnd.randrange(1, 1 << 64) for _ in range(n)]
        kind = rnd.choice(["valid", "valid", "msg", "key", "swap", "outside", "sig inf", "both inf", "zero scalar"])
        i, j = rnd.randrange(n), rnd.randrange(n)
        if kind == "msg":
            msgs[i] = bytes([msgs[i][0] ^ 1]) + msgs[i][1:]
        elif kind == "key":
            pks[i] = pks[(i + 1) % n] if n > 1 else G1_INF_U
        elif kind == "swap" and n > 1 and i != j:
            sigs[i], sigs[j] = sigs[j], sigs[i]
        elif kind == "outside":
            sigs[i] = probe
        elif kind == "sig inf":
            sigs[i] = helpers.G2_INF
        elif kind == "both inf":
            sigs[i] = helpers.G2_INF; pks[i] = G1_INF_U
        elif kind == "zero scalar":
            rands[i] = 0
        want = False if kind == "zero scalar" else orc.verify_multiple([(orc.g2_from_compressed(s_)[1], a, m) for s_, a, m in zip(sigs, pks, msgs)], rands)
        rr = (C.c_uint64 * n)(*rands)
        got1 = bool(N.lib().mbls_verify_multiple_aggregate_signatures(ctx.handle, N.cbuf(b"".join(sigs)), N.cbuf(b"".join(pks)), N.cbuf(b"".join(msgs)), 32, None, rr, n))
        got2 = mb.multi_verify_multiple_aggregate_signatures(m2, b"".join(sigs), b"".join(pks), b"".join(msgs), rands, n)
        cuts = sorted([0, n] + [rnd.randrange(n + 1) for _ in range(rnd.randrange(4))])
        recs = torch.zeros((len(cuts) - 1) * N.VM_PARTIAL_BYTES, dtype=torch.uint8, device=dev)
        keep = []
        for g in range(len(cuts) - 1):
            lo, hi = cuts[g], cuts[g + 1]
            d = [t(b"".join(sigs[lo:hi])), t(b"".join(pks[lo:hi])), t(b"".join(msgs[lo:hi])),
                 torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in rands[lo:hi]] or [0], dtype=torch.int64, device=dev)]
            keep += d
            mb.verify_multiple_partial_device(d[0].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), hi - lo, recs.data_ptr() + g * N.VM_PARTIAL_BYTES, d_apks=d[1].data_ptr())
        got3 = mb.verify_multiple_finish_device(recs.data_ptr(), len(cuts) - 1)
        work += 3 * n
        if not (got1 == got2 == got3 == want):
            bad.append("verify_multiple seed %d n %d %s cuts %s: one-call %s two contexts %s shards %s oracle %s" % (seed, n, kind, cuts, got1, got2, got3, want))
    # batched aggregate_verify: ragged items, spoiled members
    n = 40
    items = []
    for _ in range(n):
        k = rnd.choice([0, 1, 1, 2, 3, 5])
        sks = [rnd.randrange(1, helpers.R) for _ in range(k)]
        ms = [rnd.randbytes(rnd.choice([0, 7, 32, 100])) for _ in range(k)]
        pk = [orc.sk_to_pk(x) for x in sks]
        agg = None
        for x, m_ in zip(sks, ms):
            sgn = orc.sign(m_, x)
            agg = sgn if agg is None else orc.g2_add(agg, sgn)
        sig = orc.g2_compress(agg) if agg is not None else helpers.G2_INF
        kind = rnd.choice(["valid", "valid", "msg", "key", "outside"])
        if k and kind == "msg":
            ms[0] = ms[0] + b"x"
        elif k and kind == "key":
            pk[-1] = orc.sk_to_pk(sks[-1] % (helpers.R - 1) + 1)
        elif kind == "outside":
            sig = probe
        items.append((sig, ms, pk))
    off, moff, allm, allp = [0], [0], b"", b""
    for sig, ms, pk in items:
        for m_, q in zip(ms, pk):
            allm += m_; moff.append(len(allm)); allp += q
        off.append(len(moff) - 1)
    got, _ = mb.aggregate_verify_batch(b"".join(x[0] for x in items), allm, allp, n, pair_offsets=off, msg_len=0, msg_offsets=moff)
    want = []
    for sig, ms, pk in items:
        e, pt = orc.g2_from_compressed(sig)
        want.append(bool(not e and len(ms) and orc.aggregate_verify(pt, ms, pk)))
    work += sum(len(x[1]) + 1 for x in items)
    if got != want:
        bad.append("aggregate_verify_batch seed %d: items %s" % (seed, [i_ for i_ in range(n) if got[i_] != want[i_]]))
    return work, bad


# ------------------------------------------------------------------------------------------------ verify_multiple: three entries and the scalar draws
class VmPool:
    """64 key pairs, messages and signatures made on the oracle, from which run_vm draws its sets"""
    SIZE = 64

    def __init__(self, rnd):
        self.sks = [rnd.randrange(1, helpers.R) for _ in range(self.SIZE)]
        self.pks = [orc.sk_to_pk(s) for s in self.sks]
        self.msgs = [rnd.randbytes(32) for _ in range(self.SIZE)]
        self.sigs = [orc.g2_compress(orc.sign(m, s)) for m, s in zip(self.msgs, self.sks)]


def vm_batches(count, seed):
    """`count` random verify_multiple batches of 1 .. 299 sets (mostly up to 48: the lane-pair signature chain), each with 0 .. 3 random spoils (a wrong /
    infinite / non-subgroup signature, an infinite or wrong key, both infinite, a zero scalar). Yields (sigs, apks, msgs, rands, first_bad, want):
    first_bad = the first set whose signature does not decode into G2 (n if none), want = the oracle's verdict with the same scalars."""
    rnd = random.Random(seed)
    pool = VmPool(rnd)
    probe = _probe(0)
    P = VmPool.SIZE
    for _ in range(count):
        n = rnd.choice([rnd.randrange(1, 12), rnd.randrange(1, 49), rnd.randrange(1, 49), rnd.randrange(49, 300)])
        idx = [rnd.randrange(P) for _ in range(n)]
        sigs = [pool.sigs[i] for i in idx]; apks = [pool.pks[i] for i in idx]; msgs = [pool.msgs[i] for i in idx]
        rands = [rnd.randrange(1, 1 << 64) for _ in range(n)]
        for _ in range(rnd.choice([0, 0, 1, 1, 2, 3])):
            j = rnd.randrange(n); what = rnd.randrange(7)
            if what == 0: sigs[j] = pool.sigs[(idx[j] + 1) % P]
            elif what == 1: sigs[j] = helpers.G2_INF
            elif what == 2: sigs[j] = probe
            elif what == 3: apks[j] = G1_INF_U
            elif what == 4: apks[j] = pool.pks[(idx[j] + 1) % P]
            elif what == 5: sigs[j] = helpers.G2_INF; apks[j] = G1_INF_U
            else: rands[j] = 0
        dec = [orc.g2_from_compressed(s) for s in sigs]
        first_bad = next((i for i, (e, p) in enumerate(dec) if e or not orc.g2_subgroup_check(p)), n)
        want = bool(orc.verify_multiple([(d[1], a, m) for d, a, m in zip(dec, apks, msgs)], rands)) if all(r for r in rands) else False
        yield sigs, apks, msgs, rands, first_bad, want


def run_vm(ctx, dev, count, seed):
    """vm_batches through the entry that takes the scalars, the one-call entry with the caller's scalar source (its verdict AND the draws it asks for:
    sum(asked) == first_bad, one draw or none -- reference src/aggregates.rs:272-287) and the device entry. Returns ((batches, sets), mismatches)."""
    import torch
    from milagro_bls_amd import _native as N
    lib = N.lib()
    sets, bad = 0, []
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    for sigs, apks, msgs, rands, first_bad, want in vm_batches(count, seed):
        n = len(sigs)
        S, A, M = N.cbuf(b"".join(sigs)), N.cbuf(b"".join(apks)), N.cbuf(b"".join(msgs))
        rr = (C.c_uint64 * n)(*rands)
        got_plain = bool(lib.mbls_verify_multiple_aggregate_signatures(ctx.handle, S, A, M, 32, None, rr, n))
        asked = []

        def draw(_u, out, cnt):
            C.memmove(out, rr, 8 * cnt); asked.append(int(cnt))
        cb = N.SCALAR_SOURCE(draw)
        got_rng = bool(lib.mbls_verify_multiple_aggregate_signatures_rng(ctx.handle, S, A, M, 32, None, n, cb, None))
        d_s, d_a, d_m = t(b"".join(sigs)), t(b"".join(apks)), t(b"".join(msgs))
        d_r = torch.tensor([r - (1 << 64) if r >> 63 else r for r in rands], dtype=torch.int64, device=dev)
        d_res = torch.full((8,), 7, dtype=torch.uint8, device=dev)
        ctx.check(lib.mbls_verify_multiple_aggregate_signatures_device(ctx.handle, d_s.data_ptr(), d_a.data_ptr(), d_m.data_ptr(), 32, None, d_r.data_ptr(), n,
                                                                       d_res.data_ptr(), None, None))
        torch.cuda.synchronize()
        got_dev = int(d_res[0].item())
        ok = got_plain == want and got_rng == want and got_dev == int(want)
        ok = ok and sum(asked) == first_bad and len(asked) == (1 if first_bad else 0)
        if not ok:
            bad.append("verify_multiple n %d oracle %s plain %s rng %s device %d asked %s first_bad %d" % (n, want, got_plain, got_rng, got_dev, asked, first_bad))
        sets += n
    return (count, sets), bad


# ------------------------------------------------------------------------------------------------ two tracks above a round
class TrackInputs:
    """One bench.build_inputs batch of 2^16 items x k keys (every 16th item corrupted over five rejection classes), repeated up to nmax items, as byte keys
    and as indices into its resident key table"""

    def __init__(self, ctx, dev, nbase=1 << 16, k=8, nmax=3 * (1 << 16) + 5000):
        import torch
        import bench
        from milagro_bls_amd import _native as N
        d_sigs, d_msgs, d_pks, expect, d_idx, self.table = bench.build_inputs(ctx, dev, nbase, k, N.PK_UNCOMPRESSED, rank=5, return_indices=True)
        reps = -(-nmax // nbase)
        self.sigs = d_sigs.repeat(reps, 1)[:nmax].contiguous(); self.msgs = d_msgs.repeat(reps, 1)[:nmax].contiguous()
        self.pks = d_pks.repeat(reps, 1, 1)[:nmax].contiguous(); self.idx = d_idx.repeat(reps, 1)[:nmax].to(torch.int32).contiguous()
        self.expect = expect.repeat(reps)[:nmax]
        self.k, self.nmax, self.nbase = k, nmax, nbase
        ctx.reserve(nmax)


def track_cases(count, seed, nmax):
    """`count` random (n, mode, set_tracks arguments, indexed, with bitmap, with status) above a round: mode 0 / 3 = default routing, 1 = random
    set_tracks limits, 2 = tracks off"""
    rnd = random.Random(seed)
    for _ in range(count):
        n = rnd.choice([rnd.randrange(65537, 70000), rnd.randrange(65537, 131072), rnd.randrange(131073, nmax)])
        mode = rnd.randrange(4)
        tracks = (rnd.choice([1, 1000, 3584, 20000]), rnd.choice([0, 4096, 16384])) if mode == 1 else (0,) if mode == 2 else None
        indexed = rnd.random() < 0.3
        want_bm = rnd.random() < 0.5
        want_st = rnd.random() < 0.5
        yield n, mode, tracks, indexed, want_bm, want_st


def run_tracks(ctx, dev, inp, count, seed, oracle_count=0):
    """track_cases through the device entries (byte keys / table indices) against the expectation by construction: every result, every bitmap bit and
    every status word (its rejection class's bit, none on an accepted item); with oracle_count > 0 also a sample of the round seams, the tail and
    oracle_count uniform items against the oracle. Returns ((sizes, items), mismatches)."""
    import numpy as np
    import torch
    from milagro_bls_amd import _native as N
    lib = N.lib()
    items, bad = 0, []
    p = lambda x: x.data_ptr() if x is not None else None
    for it, (n, mode, tracks, indexed, want_bm, want_st) in enumerate(track_cases(count, seed, inp.nmax)):
        ctx.reset_tuning()
        if tracks is not None:
            ctx.set_tracks(*tracks)
        d_res = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        d_bm = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev) if want_bm else None
        d_st = torch.full((n,), -1, dtype=torch.int32, device=dev) if want_st else None
        try:
            if indexed:
                ctx.check(lib.mbls_fast_aggregate_verify_batch_indexed_device(ctx.handle, inp.table.handle, inp.sigs.data_ptr(), inp.msgs.data_ptr(), 32, None,
                                                                              inp.idx.data_ptr(), None, n, inp.k, d_res.data_ptr(), p(d_bm), p(d_st), None))
            else:
                ctx.check(lib.mbls_fast_aggregate_verify_batch_device(ctx.handle, inp.sigs.data_ptr(), inp.msgs.data_ptr(), 32, None, inp.pks.data_ptr(),
                                                                      N.PK_UNCOMPRESSED, None, n, inp.k, d_res.data_ptr(), p(d_bm), p(d_st), None))
            torch.cuda.synchronize()
        finally:
            ctx.reset_tuning()
        what = "n %d mode %d tracks %s indexed %s" % (n, mode, tracks, indexed)
        E = inp.expect[:n]
        res = d_res.cpu()
        if not torch.equal(res, E):
            bad.append("results %s: items %s" % (what, torch.nonzero(res != E).flatten()[:8].tolist()))
        if want_bm:
            bits = helpers.bitmap_bits(d_bm, n)
            if not (bits == E.numpy()).all():
                bad.append("bitmap %s: items %s" % (what, np.flatnonzero(bits != E.numpy())[:8].tolist()))
        if want_st:
            try:
                helpers.check_status_classes(d_st.cpu().numpy(), E.numpy(), period=inp.nbase)
            except AssertionError as e:
                bad.append("status %s: %s" % (what, e))
        if oracle_count:
            sel = helpers.sample_indices(n, seed * 1000 + it, count=oracle_count, rounds=inp.nbase, per_class=2)
            try:
                helpers.oracle_check_fav(inp.sigs, inp.msgs, inp.pks, sel, inp.k, N.PK_UNCOMPRESSED, E, res)
            except AssertionError as e:
                bad.append("oracle %s: %s" % (what, e))
        items += n
    return (count, items), bad
