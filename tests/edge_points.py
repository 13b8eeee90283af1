"""Legal but adversarial inputs of the verify entries, shared by the CPU and the GPU tests: public keys outside G1 (the verifiers of the reference do not
run KeyValidate -- src/signature.rs:27-40, src/aggregates.rs:130-170, 177-215, 261-316 --, and PublicKey::from_bytes_unchecked / from_uncompressed_bytes build
such keys, src/keys.rs:150, 170), verify_multiple batches whose blinded points coincide, and the blinding scalars whose signed 4-bit digits are extreme.

A point T of prime order ell dividing the G1 cofactor pairs to 1 with everything in G2 (the value is an ell-th root of unity AND an r-th one), so a key
pk + T verifies exactly what pk verifies, and a key T alone verifies the infinite signature. What such inputs drive is the mask-selected exceptional cases of
the incomplete Jacobian additions: for T of order 3 the table 1 T .. 8 T of the windowed scalar multiplication is built through opposite operands (3 T), an
accumulator at infinity (4 T) and EQUAL operands (5 T = T + T: the doubling fix-up), and the sum tree of a batch meets equal / opposite partners when sets
repeat with one scalar. window_case_census / tree_case_census replay those schedules on the Python model's integers and say which case each addition is.

Points are the model's (affine integer pairs, None = infinity); *_bytes turn them into the wire formats. Signing goes through the oracle (orc)."""
import random
from collections import Counter

import bls12_381 as M

import helpers
import orc

TORSION_ORDERS = (3, 11, 10177, 859267, 52437899)                # the primes dividing the G1 cofactor (x - 1)^2 / 3
G1_COFACTOR = (M.X_ABS + 1) ** 2 // 3
assert G1_COFACTOR * M.R == M.P + 1 - (-M.X_ABS + 1)             # #E(Fp) = p + 1 - t, t = x + 1
assert all(G1_COFACTOR % ell == 0 for ell in TORSION_ORDERS)
G1_INF_U = bytes([0x40]) + bytes(95)
CASES = ("general", "equal", "opposite", "acc_inf", "addend_inf")


def curve_point(rnd):
    """a random point of E(Fp) (outside G1 with probability 1 - 1/h)"""
    while True:
        x = rnd.randrange(M.P); y = M.fp_sqrt((x * x * x + 4) % M.P)
        if y is not None:
            return (x, y if rnd.getrandbits(1) else (-y) % M.P)


def g1_torsion_points(rnd, per_order=1, orders=TORSION_ORDERS, x0=True):
    """[(ell, T, g)]: per_order points T of each prime order ell, each with a random G1 point g drawn after it (for pk + T style shifts), then -- x0 -- the two
    3-torsion points with x = 0, (0, 2) and (0, p - 2), with g = None: they put a zero coordinate into every line evaluation and every product with x."""
    out = []
    for ell in orders:
        assert G1_COFACTOR % ell == 0
        for _ in range(per_order):
            t = None
            while t is None:
                t = M.g1_mul(curve_point(rnd), G1_COFACTOR * M.R // (ell if ell == 3 else ell * ell))   # E[ell] is rational for ell | x - 1, ell != 3
            out.append((ell, t, M.g1_mul(M.G1, rnd.randrange(1, M.R))))
    if x0:
        out += [(3, (0, 2), None), (3, (0, M.P - 2), None)]
    return out


G2_COFACTOR = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5


def g2_torsion_points(curve_points, orders=(13, 23, 2713)):
    """[(ell, T)]: from curve points of E'(Fp2) outside G2 (the golden file's g2_subgroup_probes are such points, of large composite order), one point of
    each prime order ell dividing the G2 cofactor: [h2 r / ell^e] Q with ell^e the power of ell in h2"""
    out = []
    for ell, q in zip(orders, curve_points):
        assert G2_COFACTOR % ell == 0
        e = ell
        while G2_COFACTOR % (e * ell) == 0:
            e *= ell
        t = M.g2_mul(q, G2_COFACTOR * M.R // e)
        while t is not None and M.g2_mul(t, ell) is not None:           # a point of order ell^j, j > 1: down to order ell
            t = M.g2_mul(t, ell)
        assert t is not None and M.g2_mul(t, ell) is None, ell
        out.append((ell, t))
    return out


def g1_bytes(pt, fmt):
    """a model point in the key format fmt (0: 48 bytes compressed, 1: 96 bytes uncompressed)"""
    return M.g1_compress(pt) if fmt == 0 else M.g1_serialize_uncompressed(pt)


def g1_point(b96):
    """the oracle's 96-byte key -> model point"""
    e, pt = M.g1_deserialize_uncompressed(bytes(b96))
    assert e == 0
    return pt


def g2_point(sig96c):
    e, pt = M.g2_decompress(bytes(sig96c))
    assert e == 0
    return pt


# ------------------------------------------------------------------------------------------------ keys outside G1: the classes
def outside_key_classes(rnd, torsion):
    """One instance of every class per entry (ell, T, g) of `torsion`: dicts with name, ell, sk, msg (32 bytes), keys (model points, in order), sig_inf
    (the item's signature is the infinite one instead of sign(msg, sk)) and expect (the verdict by construction: the torsion part of the key sum pairs
    to 1, a key sum at infinity is refused, reference src/aggregates.rs:199-202). Items with one key also serve verify / pre_aggregated / one pair of
    aggregate_verify."""
    out = []
    for ell, T, _g in torsion:
        sk = rnd.randrange(1, M.R)
        pk = M.g1_mul(M.G1, sk)
        nT, T2 = M.g1_neg(T), M.g1_mul(T, 2)
        def item(name, keys, expect, sig_inf=False):
            out.append(dict(name=name, ell=ell, sk=sk, msg=rnd.randbytes(32), keys=keys, sig_inf=sig_inf, expect=expect))
        item("pk+T", [M.g1_add(pk, T)], True)
        item("pk,T", [pk, T], True)
        item("T", [T], False)
        if ell <= 11:
            item("ell*T", [T] * ell, False)                              # the sum is infinity
        item("T,pk,T,T,T", [T, pk, T, T, T], True)
        item("T,pk,-T", [T, pk, nT], True)
        item("-T,T", [nT, T], False)                                     # opposite operands on the first addition; infinity
        item("2T+pk", [M.g1_add(T2, pk)], True)
        item("curve point", [curve_point(rnd)], False)
        item("inf sig,T", [T], True, sig_inf=True)                       # both pairings are 1
        item("inf sig,pk+T", [M.g1_add(pk, T)], False, sig_inf=True)
    return out


def class_wire(c, fmt):
    """(compressed signature, message, [key bytes]) of a class instance"""
    sig = helpers.G2_INF if c["sig_inf"] else orc.g2_compress(orc.sign(c["msg"], c["sk"]))
    return sig, c["msg"], [g1_bytes(k, fmt) for k in c["keys"]]


def honest_items(rnd, count):
    """`count` one- to four-key items of honest keys in the class format, every third one rejected (wrong message / wrong key / infinite signature)"""
    out = []
    for i in range(count):
        sks = [rnd.randrange(1, M.R) for _ in range(rnd.randrange(1, 5))]
        keys = [g1_point(orc.sk_to_pk(s)) for s in sks]
        c = dict(name="honest", ell=0, sk=sum(sks) % M.R, msg=rnd.randbytes(32), keys=keys, sig_inf=False, expect=True)
        if i % 3 == 2:
            kind = (i // 3) % 3
            c["expect"] = False
            if kind == 0:
                c["name"] = "honest wrong sk"; c["sk"] = c["sk"] % (M.R - 1) + 1
            elif kind == 1:
                c["name"] = "honest wrong key"; c["keys"] = keys[:-1] + [g1_point(orc.sk_to_pk(rnd.randrange(1, M.R)))]
            else:
                c["name"] = "honest inf sig"; c["sig_inf"] = True
        out.append(c)
    return out


FAV_SEED = 4711


def fav_items(seed, honest=104):
    """the items of the GPU test of fast_aggregate_verify: every class for every torsion order (orders 3 and 11 twice) and the x = 0 points, `honest` honest
    items, in seeded order"""
    rnd = random.Random(seed)
    items = outside_key_classes(rnd, g1_torsion_points(rnd) + g1_torsion_points(rnd, orders=(3, 11), x0=False)) + honest_items(rnd, honest)
    rnd.shuffle(items)
    return items


# ------------------------------------------------------------------------------------------------ blinding scalars
BLIND_EDGE_SCALARS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 1 << 60, 1 << 63, (1 << 63) - 1, (1 << 64) - 1, 0x7777777777777777, 0x7777777777777778,
                      0x8888888888888888, 0x0807060504030201, 0xF00000000000000F, 0x1000000000000001)


def edge_scalars(orders=(3, 11)):
    """BLIND_EDGE_SCALARS and, per torsion order used, ell, ell +- 1 and 16 ell (the multiples of ell send [r] T to infinity), without repeats"""
    out = list(BLIND_EDGE_SCALARS)
    for ell in orders:
        out += [ell, ell - 1, ell + 1, 16 * ell]
    seen = set()
    return [r for r in out if not (r in seen or seen.add(r))]


def signed_digits(r):
    """(carry digit, [16 digits in [-8, 7], most significant first]) of r' = r + 0x8888888888888888: r = carry 2^64 + sum d_j 16^j"""
    assert 0 <= r < 1 << 64
    rp = r + 0x8888888888888888
    ds = [((rp >> s) & 15) - 8 for s in range(60, -4, -4)]
    assert (rp >> 64) * (1 << 64) + sum(d << (4 * (15 - j)) for j, d in enumerate(ds)) == r
    return rp >> 64, ds


def _classify(add, acc, addend, dropped=False):
    """the case of acc + addend in the order the routines select it: the addend infinite (or its digit zero) wins over the accumulator at infinity"""
    if addend is None or dropped:
        return "addend_inf"
    if acc is None:
        return "acc_inf"
    s = add(acc, addend)
    if s is None:
        return "opposite"
    return "equal" if acc == addend else "general"


def window_case_census(point, r, g2=False):
    """Replay of the signed-window [r] point of g1_blind_routine / g2_blind_routine (tools/gen_tower_d.py) on the model: the table 1 P, 2 P = dbl(P), then six
    times acc += P; acc = infinity; acc += carry P; sixteen windows of acc = 16 acc, acc += d_j P (the record |d_j|, negated for d_j < 0, dropped for
    d_j = 0). -> ({"table": Counter, "window": Counter} over CASES, [r] point)"""
    add, neg, mul = (M.g2_add, M.g2_neg, M.g2_mul) if g2 else (M.g1_add, M.g1_neg, M.g1_mul)
    census = {"table": Counter(), "window": Counter()}
    tab = [point, add(point, point)]
    acc = tab[1]
    for _ in range(6):
        census["table"][_classify(add, acc, point)] += 1
        acc = add(acc, point)
        tab.append(acc)
    carry, ds = signed_digits(r)
    acc = None
    census["window"][_classify(add, acc, tab[0], dropped=carry == 0)] += 1
    if carry:
        acc = add(acc, tab[0])
    for d in ds:
        for _ in range(4):
            acc = add(acc, acc)
        q = tab[max(abs(d), 1) - 1]
        q = neg(q) if d < 0 else q
        census["window"][_classify(add, acc, q, dropped=d == 0)] += 1
        if d:
            acc = add(acc, q)
    assert acc == mul(point, r)
    return census, acc


def tree_case_census(blinded_points):
    """Replay of the sum tree of g2_tree_levels (milagro_bls_amd/csrc/mbls_kernels.hip) over the blinded signatures in workspace order (one call, one device:
    set i = item i): per level half = (m + 1) / 2, item i < m - half takes item i + half. -> ([(pairs, Counter over CASES)] per level, the total)"""
    pts = list(blinded_points)
    levels = []
    memo = {}
    while len(pts) > 1:
        m = len(pts); half = (m + 1) // 2
        c = Counter()
        for i in range(m - half):
            a, b = pts[i], pts[i + half]
            if (a, b) not in memo:
                memo[(a, b)] = (_classify(M.g2_add, a, b), M.g2_add(a, b))
            case, pts[i] = memo[(a, b)]
            c[case] += 1
        levels.append((m - half, c))
        pts = pts[:half]
    return levels, (pts[0] if pts else None)


# ------------------------------------------------------------------------------------------------ verify_multiple: sets that coincide
class CoincidencePool:
    """`nbase` honest sets (sig, pk, msg), each with ONE scalar (scalars[b % len]) shared by all its variants: 'plain', 'neg' = (-sig, -pk, msg) (a valid
    set too: e(-sig, -G1) e(H, -pk) = 1), 'shift' = (sig, pk + T, msg); and per torsion point the pure-torsion set 'torsion' = (infinity, T, msg) with a
    scalar of its own. entries: dicts kind, base, sig (96 bytes compressed), apk (96 bytes), msg, r."""

    def __init__(self, rnd, nbase, torsion, scalars):
        self.entries = []
        for b in range(nbase):
            sk = rnd.randrange(1, M.R); msg = rnd.randbytes(32)
            r = scalars[b % len(scalars)]
            pk = g1_point(orc.sk_to_pk(sk))
            sig = orc.sign(msg, sk)
            T = torsion[b % len(torsion)][1]
            e = lambda kind, s, a: self.entries.append(dict(kind=kind, base=b, sig=orc.g2_compress(s), apk=g1_bytes(a, 1), msg=msg, r=r))
            e("plain", sig, pk)
            e("neg", orc.g2_mul(sig, M.R - 1), M.g1_neg(pk))
            e("shift", sig, M.g1_add(pk, T))
        for j, (ell, T, _g) in enumerate(torsion):
            self.entries.append(dict(kind="torsion", base=nbase + j, sig=helpers.G2_INF, apk=g1_bytes(T, 1), msg=rnd.randbytes(32),
                                     r=scalars[(nbase + j) % len(scalars)]))
        self.by_kind = {k: [e for e in self.entries if e["kind"] == k] for k in ("plain", "neg", "shift", "torsion")}


def vm_coincidence_batch(rnd, n, pool, torsion_share=0.10):
    """n sets drawn from the pool: torsion_share of them pure-torsion sets (their blinded signature is infinity), the others plain / negation / shifted
    variants of the base sets. Two draws of one base give equal blinded signatures, a draw of its negation the opposite one.
    -> (sigs, apks, msgs, rands), lists of n"""
    rest = [e for e in pool.entries if e["kind"] != "torsion"]
    picks = [rnd.choice(pool.by_kind["torsion"]) if rnd.random() < torsion_share else rnd.choice(rest) for _ in range(n)]
    return [e["sig"] for e in picks], [e["apk"] for e in picks], [e["msg"] for e in picks], [e["r"] for e in picks]


def blinded_signatures(sigs, rands):
    """[r_i] sig_i as model points (distinct (sig, r) computed once)"""
    memo = {}
    out = []
    for s, r in zip(sigs, rands):
        if (s, r) not in memo:
            memo[(s, r)] = M.g2_mul(g2_point(s), r)
        out.append(memo[(s, r)])
    return out


def spoil(batch, i):
    """the batch with set i's message changed: its verdict is False whenever the batch's own is True and set i's key is not pure torsion"""
    sigs, apks, msgs, rands = [list(x) for x in batch]
    msgs[i] = bytes([msgs[i][0] ^ 1]) + msgs[i][1:]
    return sigs, apks, msgs, rands


def oracle_verify_multiple(batch, nthreads=1, chunk=64):
    """The oracle's verify_multiple with the same scalars. Above `chunk` sets the batch is cut into chunks evaluated on nthreads threads: the product over
    the batch is the product of the chunks' products, so a batch whose chunks all verify verifies, and one with exactly one failing chunk does not. -> bool"""
    sigs, apks, msgs, rands = batch
    dec = [orc.g2_from_compressed(s) for s in dict.fromkeys(sigs)]
    assert not any(e for e, _ in dec)
    pt = dict(zip(dict.fromkeys(sigs), (p for _, p in dec)))
    sets = [(pt[s], a, m) for s, a, m in zip(sigs, apks, msgs)]
    if len(sets) <= chunk:
        return orc.verify_multiple(sets, rands)
    from concurrent.futures import ThreadPoolExecutor
    cuts = range(0, len(sets), chunk)
    with ThreadPoolExecutor(max(1, nthreads)) as ex:
        ok = list(ex.map(lambda lo: orc.verify_multiple(sets[lo:lo + chunk], rands[lo:lo + chunk]), cuts))
    bad = ok.count(False)
    assert bad <= 1, "chunk algebra needs at most one failing chunk, got %d" % bad
    return bad == 0


# the seeded coincidence batches of the GPU tests (tests/test_gpu_unchecked_points.py) and of the census conditions (tests/test_edge_points_cpu.py)
VM_POOL_SEED = 2024
VM_POOL_BASES = 2
VM_POOL_SCALARS = (0x7777777777777778, 0xF00000000000000F, 3, 0x0807060504030201, 33, 0x8888888888888888, 16, (1 << 64) - 1)


def vm_pool():
    rnd = random.Random(VM_POOL_SEED)
    torsion = g1_torsion_points(rnd, orders=(3, 11))
    return CoincidencePool(rnd, VM_POOL_BASES, torsion, VM_POOL_SCALARS)


def vm_batch_sizes(coop_max_items, tree_pairs):
    """(on the lane-pair signature chain, above it with every tree level on the wave engine, first tree level above tree_pairs pairs) -- from the library's
    thresholds: 2 n <= coop_max_items takes k_blind_sig2_d, a level of more than tree_pairs pairs takes k_g2_tree_d (verify_multiple_impl, g2_tree_levels)"""
    small = coop_max_items // 2 - 60
    mid = coop_max_items // 2 + 40
    big = 2 * tree_pairs + 404
    assert 2 * small <= coop_max_items < 2 * mid and mid - (mid + 1) // 2 <= tree_pairs < big - (big + 1) // 2
    return small, mid, big


def vm_seeded_batch(pool, n):
    """-> (batch, index of a set whose key is honest or shifted: spoiling it turns a True verdict into False)"""
    b = vm_coincidence_batch(random.Random(7000 + n), n, pool)
    return b, next(i for i in range(n // 3, n) if b[0][i] != helpers.G2_INF)


def vm_structured_batches():
    """[(name, batch, spoil_at)]: every set identical with one scalar (n = 2, 3, 4, 5, 8, 64, 65: every tree addition has equal operands); set / negation
    alternating with one scalar (64 sets: equal partners down to the last level, where S meets -S and the total is infinity; 65 sets: opposite partners on the
    first level, infinities below); a set and its negation; per edge scalar one honest set and, in the lanes next to it, pure-torsion sets (infinity, T, msg)
    with T of order 3 / 11 / x = 0 (two sets infinite on both sides at the end); apk = pk + T with scalars that are and are not multiples of ell.
    A pure-torsion key's blinded point pairs to 1 whichever multiple of T it is: what those sets can show is that the exceptional branches leave a valid point
    and leave the neighbouring lanes alone -- the value itself is the simulator's business (tests/test_asm_sim_d_cpu.py). spoil_at: a set with an honest
    signature."""
    rnd = random.Random(515)
    torsion = g1_torsion_points(rnd, orders=(3, 11))
    sk = rnd.randrange(1, M.R); msg = rnd.randbytes(32)
    pk = g1_point(orc.sk_to_pk(sk))
    sig = orc.sign(msg, sk)
    S = (orc.g2_compress(sig), g1_bytes(pk, 1), msg)
    NS = (orc.g2_compress(orc.g2_mul(sig, M.R - 1)), g1_bytes(M.g1_neg(pk), 1), msg)
    out = []

    def batch(name, sets, rands, spoil_at):
        out.append((name, ([s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets], list(rands)), spoil_at))
    for i, n in enumerate((2, 3, 4, 5, 8, 64, 65)):
        batch("identical x %d" % n, [S] * n, [BLIND_EDGE_SCALARS[-1 - i]] * n, n - 1)
    for n in (2, 64, 65):
        batch("alternating x %d" % n, [(S, NS)[i & 1] for i in range(n)], [0xF00000000000000F] * n, n // 2)
    honest = []
    for _ in range(4):
        sk_j = rnd.randrange(1, M.R); msg_j = rnd.randbytes(32)
        honest.append((orc.g2_compress(orc.sign(msg_j, sk_j)), orc.sk_to_pk(sk_j), msg_j))
    sets, rands = [], []
    for j, r in enumerate(edge_scalars()):                                # every edge scalar on an honest set, and on torsion keys in the lanes next to it
        sets.append(honest[j % 4]); rands.append(r)
        for _ell, T, _g in torsion[j % 2::2] if j % 3 else torsion:
            sets.append((helpers.G2_INF, g1_bytes(T, 1), rnd.randbytes(32))); rands.append(r)
    for r in (0x7777777777777778, 5):
        sets.append((helpers.G2_INF, G1_INF_U, rnd.randbytes(32))); rands.append(r)
    batch("edge scalars", sets, rands, 0)
    sets, rands = [], []
    for ell, T, _g in torsion:
        for r in (ell, 16 * ell, ell + 1, ell - 1, 3 * 11 * 16, (1 << 64) - 1, 0x7777777777777778):
            sets.append((S[0], g1_bytes(M.g1_add(pk, T), 1), msg)); rands.append(r)
    batch("apk = pk + T", sets, rands, 1)
    return out


def coop_tree_pairs():
    """MBLS_COOP_TREE_PAIRS as the library's source defines it (a tree level with more pairs runs one lane per sum: k_g2_tree_d)"""
    import os
    import re
    with open(os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc", "mbls_kernels.hip")) as f:
        return int(re.search(r"^#define MBLS_COOP_TREE_PAIRS (\d+)\s*$", f.read(), re.M).group(1))
