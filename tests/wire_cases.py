"""Keys and signatures at the edges of the wire encodings, shared by the CPU and the GPU tests: one seeded case list per format -- G1 compressed (48 bytes),
G1 uncompressed (96 bytes), G2 compressed (96 bytes) -- built on the Python model alone (oracle/pymodel/bls12_381.py; signing goes through the oracle).

The library promises the reference's from_bytes rule: canonical encodings only. What random blobs never reach is listed here by family:

  range      a coordinate field holding p -+ 2^(32 j) for every limb j, p - 1, p, p + 1, 2^381 - 1 (and 2^384 - 1 where the field is not masked), the
             other coordinate chosen so that the REDUCED point is on the curve wherever such a partner exists
  alias      non-canonical encodings of valid points: x = p + k with k^3 + 4 a square, (x + p, y), (x, y + p), (x + 2 p, y), x.c0 + p, x.c1 + p;
             every alias names its canonical twin (Case.canon)
  flags      all eight values of the top three bits over an honest body, a zero body and zero bodies with one stray bit
  fp_sign    G1 points whose y sits next to (p - 1) / 2, and for every limb j a point whose y differs from (p - 1) / 2 first in limb j
  fp2_sqrt   G2 curve points whose radicand x^3 + 4 (1 + i) is real (y real, or purely imaginary: the t = 0 branch of the complex method), and points
             whose y.c1 sits next to (p - 1) / 2
  off_curve  (x, y +- 1), (y, x), single bit flips, an x whose radicand is a non-residue
  control    honest keys and signatures, canonical infinity

A case carries its bytes, a tag, the class the model assigns (OK_FINITE with the affine point, OK_INF, SIZE, POINT) and the library's error code.
ROUTES names, for every call site of a decoder in milagro_bls_amd/csrc, the entries that reach it (tests/test_wire_cases_cpu.py holds the table
complete against the sources and the named test functions present)."""
import os
import random
import re

import bls12_381 as M

import helpers
import orc

P = M.P
HALF = (P - 1) // 2
SEED = 381
OK_FINITE, OK_INF, SIZE, POINT = "ok_finite", "ok_inf", "size", "point"
G1C, G1U, G2C = "g1c", "g1u", "g2c"
FORMATS = (G1C, G1U, G2C)
LEN = {G1C: 48, G1U: 96, G2C: 96}
ERR_OK, ERR_G1_SIZE, ERR_G2_SIZE, ERR_INVALID_POINT = 0, 1, 2, 3      # include/mbls.h MBLS_ERR_*; the oracle's codes are the same
ALIAS_K = (0, 4, 5, 6, 8, 9, 10, 11)                                  # k^3 + 4 is a square: x = p + k aliases a curve point
FAMILIES = ("range", "alias", "flags", "fp_sign", "fp2_sqrt", "off_curve", "control")
assert (1 << 381) - P > P // 5 and P % 3 == 1 and P % 4 == 3


class Case:
    __slots__ = ("fmt", "family", "tag", "data", "cls", "point", "err", "canon", "info")

    def __init__(self, fmt, family, tag, data, canon=None, **info):
        self.fmt, self.family, self.tag, self.data, self.canon, self.info = fmt, family, tag, bytes(data), canon, info
        assert len(self.data) == LEN[fmt], tag
        self.cls, self.point = classify(fmt, self.data)
        self.err = {OK_FINITE: ERR_OK, OK_INF: ERR_OK, SIZE: ERR_G2_SIZE if fmt == G2C else ERR_G1_SIZE, POINT: ERR_INVALID_POINT}[self.cls]

    @property
    def ok(self):
        return self.cls in (OK_FINITE, OK_INF)

    def __repr__(self):
        return "<%s %s/%s %s>" % (self.fmt, self.family, self.tag, self.cls)


MODEL_DECODE = {G1C: M.g1_decompress, G1U: M.g1_deserialize_uncompressed, G2C: M.g2_decompress}


def classify(fmt, data):
    """the model's answer -> (class, affine point or None)"""
    e, pt = MODEL_DECODE[fmt](data)
    if e == M.ERR_SIZE:
        return SIZE, None
    if e == M.ERR_POINT:
        return POINT, None
    assert e == M.ERR_OK
    return (OK_INF, None) if pt is None else (OK_FINITE, pt)


def canonical(fmt, pt):
    """the model's canonical bytes of a point in the format"""
    return {G1C: M.g1_compress, G1U: M.g1_serialize_uncompressed, G2C: M.g2_compress}[fmt](pt)


def uncompressed(fmt, pt):
    """the decoded form the library and the oracle hand out: 96 bytes x || y for a key, 192 bytes x.c1 || x.c0 || y.c1 || y.c0 for a signature"""
    if fmt != G2C:
        return M.g1_serialize_uncompressed(pt)
    if pt is None:
        return bytes([0x40]) + bytes(191)
    (x0, x1), (y0, y1) = pt
    return b"".join(v.to_bytes(48, "big") for v in (x1, x0, y1, y0))


def be48(v):
    return int(v).to_bytes(48, "big")


def with_flags(body, f):
    """the top three bits of byte 0 replaced by f (0 .. 7)"""
    return bytes([(body[0] & 0x1F) | (f << 5)]) + bytes(body[1:])


def top_limb_diff(a, b):
    """the most significant 32-bit limb in which a and b differ (None: equal)"""
    d = a ^ b
    return None if d == 0 else (d.bit_length() - 1) // 32


# ------------------------------------------------------------------------------------------------ cube roots (Adleman-Manders-Miller, q = 1 mod 3)
def _amm3(a, mul, one, q, seed_nonres):
    """a cube root of a in the field of q elements given by mul / one, or None; seed_nonres(i) -> candidates for a cubic non-residue"""
    def pw(x, e):
        r = one
        while e:
            if e & 1:
                r = mul(r, x)
            x = mul(x, x); e >>= 1
        return r
    if pw(a, (q - 1) // 3) != one:
        return None
    s, t = 0, q - 1
    while t % 3 == 0:
        s += 1; t //= 3
    c = next(c for c in (seed_nonres(i) for i in range(2, 64)) if pw(c, (q - 1) // 3) != one)
    g = pw(c, t)                                   # generates the 3-Sylow subgroup (order 3^s)
    gi = pw(g, 3 ** s - 1)
    e = pow(3, -1, t)
    x = pw(a, e)                                   # x^3 = a * (a^t)^k with 3 e = 1 + k t
    b = pw(pw(a, t), (3 * e - 1) // t)             # in the Sylow subgroup, and a cube there
    w = pw(g, 3 ** (s - 1))
    m, bb = 0, b
    for i in range(s):                             # b = g^m, digit by digit
        d = pw(bb, 3 ** (s - 1 - i))
        dig = 0 if d == one else 1 if d == w else 2
        m += dig * 3 ** i
        bb = mul(bb, pw(gi, dig * 3 ** i))
    assert m % 3 == 0
    return mul(x, pw(gi, m // 3))


def fp_cbrt(a):
    a %= P
    if a == 0:
        return 0
    r = _amm3(a, lambda x, y: x * y % P, 1, P, lambda i: i)
    assert r is None or pow(r, 3, P) == a
    return r


def f2_cbrt(a):
    a = M.f2(*a)
    if M.f2_is_zero(a):
        return M.F2_ZERO
    r = _amm3(a, M.f2_mul, M.F2_ONE, P * P, lambda i: (i, 1))
    assert r is None or M.f2_mul(M.f2_sqr(r), r) == a
    return r


# ------------------------------------------------------------------------------------------------ building blocks
def g1_enc(fmt, x, y=None, flags=None):
    """raw field contents -> bytes; G1C: flags = the top three bits (x < 2^381); G1U: x, y < 2^384, flags OR-ed into byte 0 when given"""
    if fmt == G1C:
        assert x < 1 << 381
        return with_flags(be48(x), flags)
    b = be48(x) + be48(y)
    return b if flags is None else bytes([b[0] | (flags << 5)]) + b[1:]


def g2_enc(x0, x1, flags):
    assert x1 < 1 << 381 and x0 < 1 << 384
    return with_flags(be48(x1) + be48(x0), flags)


def sign_flag(y):
    return 5 if M.fp_lex_largest(y) else 4


def range_values(bits):
    """the values a coordinate field of `bits` bits takes in the range family: (name, value)"""
    out = []
    for j in range(12):
        out.append(("p-2^%d" % (32 * j), P - (1 << 32 * j)))
        if P + (1 << 32 * j) < 1 << bits:
            out.append(("p+2^%d" % (32 * j), P + (1 << 32 * j)))
    out += [("p", P), ("2^381-1", (1 << 381) - 1)]
    if bits == 384:
        out.append(("2^384-1", (1 << 384) - 1))
    return out


class _Build:
    def __init__(self):
        self.rnd = random.Random(SEED)
        self.cases = {f: [] for f in FORMATS}
        self.honest = []                                # (sk, msg, pk point, sig point)
        for _ in range(6):
            sk = self.rnd.randrange(1, M.R); msg = self.rnd.randbytes(32)
            e, pk = M.g1_deserialize_uncompressed(orc.sk_to_pk(sk)); assert e == 0
            self.honest.append((sk, msg, pk, self._sign(msg, sk)))
        while self.honest[-1][2][0] + P >> 381:         # the last signer's x leaves room for x + p below 2^381
            sk = self.rnd.randrange(1, M.R)
            e, pk = M.g1_deserialize_uncompressed(orc.sk_to_pk(sk)); assert e == 0
            self.honest[-1] = (sk, self.honest[-1][1], pk, self._sign(self.honest[-1][1], sk))

    @staticmethod
    def _sign(msg, sk):
        e, pt = M.g2_decompress(orc.g2_compress(orc.sign(msg, sk))); assert e == 0
        return pt

    def add(self, fmt, family, tag, data, canon=None, **info):
        self.cases[fmt].append(Case(fmt, family, tag, data, canon, **info))

    # -- controls
    def controls(self):
        for i, (sk, msg, pk, sig) in enumerate(self.honest):
            self.add(G1C, "control", "honest %d" % i, M.g1_compress(pk), sk=sk, msg=msg)
            self.add(G1U, "control", "honest %d" % i, M.g1_serialize_uncompressed(pk), sk=sk, msg=msg)
            self.add(G2C, "control", "honest %d" % i, M.g2_compress(sig), sk=sk, msg=msg)
        for fmt in FORMATS:
            self.add(fmt, "control", "infinity", canonical(fmt, None))

    # -- range, limb by limb
    def ranges(self):
        _, _, pk, sig = self.honest[0]
        for name, v in range_values(381):                       # G1C: the one field
            for f in (4, 5):
                self.add(G1C, "range", "x=%s flag %d" % (name, f), g1_enc(G1C, v, flags=f), value=v)
        for name, v in range_values(381):                       # G1U x (its top three bits are flags: a value with one of them set is a flag case)
            y = M.fp_sqrt((pow(v, 3, P) + 4) % P)               # the partner that puts the REDUCED point on the curve, where there is one
            self.add(G1U, "range", "x=%s" % name, g1_enc(G1U, v, pk[1] if y is None else y), value=v, field="x", partner=y is not None)
        for name, v in range_values(384):                       # G1U y (unmasked)
            x = fp_cbrt(v * v - 4)
            self.add(G1U, "range", "y=%s" % name, g1_enc(G1U, pk[0] if x is None else x, v), value=v, field="y", partner=x is not None)
        for name, v in range_values(381):                       # G2 x.c1 (masked) and x.c0 (unmasked), the other half honest
            for f in (4, 5):
                self.add(G2C, "range", "x.c1=%s flag %d" % (name, f), g2_enc(sig[0][0], v, f), value=v, field="c1")
        for name, v in range_values(384):
            for f in (4, 5):
                self.add(G2C, "range", "x.c0=%s flag %d" % (name, f), g2_enc(v, sig[0][1], f), value=v, field="c0")

    # -- aliases of valid points
    def aliases(self):
        for k in ALIAS_K:
            y = M.fp_sqrt(k ** 3 + 4); assert y is not None
            for f in (4, 5):
                e, pt = M.g1_decompress(g1_enc(G1C, k, flags=f)); assert e == 0 and pt[0] == k
                self.add(G1C, "alias", "x=p+%d flag %d" % (k, f), g1_enc(G1C, P + k, flags=f), canon=g1_enc(G1C, k, flags=f), k=k, of=pt)
        for i, (sk, msg, pk, sig) in enumerate(self.honest):
            x, y = pk
            canon = M.g1_serialize_uncompressed(pk)
            # (the top three bits of x are flags: x + p stays below 2^381 for a quarter of the keys -- the last honest signer is one --, x + 2 p never does,
            # so that alias is refused by the sign-flag rule as well)
            for tag, ax, ay in (("x+p", x + P, y), ("y+p", x, y + P), ("x+2p", x + 2 * P, y)):
                self.add(G1U, "alias", "%s of honest %d" % (tag, i), g1_enc(G1U, ax, ay), canon=canon, of=pk, sk=sk, msg=msg, flagless=not ax >> 381)
        assert any(c.family == "alias" and c.tag.startswith("x+p") and c.info["flagless"] for c in self.cases[G1U])
        n0 = n1 = 0
        pool = list(self.honest)
        while n0 < 3 or n1 < 3:
            if not pool:
                sk = self.rnd.randrange(1, M.R); msg = self.rnd.randbytes(32)
                pool.append((sk, msg, None, self._sign(msg, sk)))
            sk, msg, _pk, sig = pool.pop(0)
            (x0, x1), y = sig
            f = 5 if M.f2_lex_largest(y) else 4
            canon = M.g2_compress(sig)
            if n0 < 3:
                self.add(G2C, "alias", "x.c0+p #%d" % n0, g2_enc(x0 + P, x1, f), canon=canon, of=sig, sk=sk, msg=msg); n0 += 1
            if n1 < 3 and x1 + P < 1 << 381:
                self.add(G2C, "alias", "x.c1+p #%d" % n1, g2_enc(x0, x1 + P, f), canon=canon, of=sig, sk=sk, msg=msg); n1 += 1

    # -- flags
    def flags(self):
        _, _, pk, sig = self.honest[1]
        for fmt, honest in ((G1C, be48(pk[0])), (G1U, be48(pk[0]) + be48(pk[1])), (G2C, be48(sig[0][1]) + be48(sig[0][0]))):
            n = LEN[fmt]
            bodies = [("honest", honest), ("zero", bytes(n)), ("stray last", bytes(n - 1) + b"\x01"), ("stray first", b"\x01" + bytes(n - 1)),
                      ("stray middle", bytes(n // 2) + b"\x80" + bytes(n - n // 2 - 1))]
            for name, body in bodies:
                for f in range(8):
                    self.add(fmt, "flags", "0x%02X on %s" % (f << 5, name), with_flags(body, f), flag=f, body=name)

    # -- sign choice in Fp
    def fp_sign(self):
        pts = []
        for side in (-1, 1):                                    # the two nearest j on each side of (p - 1) / 2 (j <= 0: not the larger root)
            found, j = 0, 0 if side < 0 else 1
            while found < 2:
                x = fp_cbrt((HALF + j) ** 2 - 4)
                if x is not None:
                    pts.append(("y=half%+d" % j, (x, HALF + j), dict(j=j))); found += 1
                j += side
        for limb in range(12):                                  # y differs from (p - 1) / 2 first in limb `limb`
            for side in (-1, 1):
                d = 0
                while True:
                    y = HALF + side * ((1 << 32 * limb) + d)
                    x = fp_cbrt(y * y - 4) if top_limb_diff(y, HALF) == limb and 0 < y < P else None
                    if x is not None:
                        break
                    d += 1
                pts.append(("y=half%s(2^%d+%d)" % ("+" if side > 0 else "-", 32 * limb, d), (x, y), dict(limb=limb)))
        for tag, (x, y), info in pts:
            assert M.g1_on_curve((x, y))
            for f in (4, 5):                                    # the flag that names this root, and the one that names the other
                self.add(G1C, "fp_sign", "%s flag %d" % (tag, f), g1_enc(G1C, x, flags=f), y=y, **info)
            self.add(G1U, "fp_sign", tag, g1_enc(G1U, x, y), y=y, **info)
            self.add(G1U, "fp_sign", tag + " negated", g1_enc(G1U, x, P - y), y=P - y, **info)

    # -- Fp2 square root and sign
    def fp2_sqrt(self):
        # the complex method starts from s = sqrt(a0^2), which the exponentiation returns as the root that is itself a residue: s = a0 for a residue a0 (y real,
        # t = (a0 + s) / 2 = a0) and s = -a0 for a non-residue (y purely imaginary: t = 0, the branch that substitutes (a0 - s) / 2)
        want = {"real": 4, "imag": 4}
        while any(want.values()):
            x1 = self.rnd.randrange(1, P)
            x0 = M.fp_sqrt((pow(x1, 3, P) - 4) * M.fp_inv(3 * x1) % P)
            if x0 is None:
                continue
            x = (x0, x1)
            a = M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.B2)
            assert a[1] == 0 and a[0] != 0
            y = M.f2_sqrt(a)
            kind = "real" if y[1] == 0 else "imag"
            tz = (a[0] + M.fp_sqrt(a[0] * a[0] % P)) % P == 0
            assert tz == (kind == "imag")
            if not want[kind]:
                continue
            want[kind] -= 1
            for f in (4, 5):
                self.add(G2C, "fp2_sqrt", "radicand real, y %s, flag %d" % (kind, f), g2_enc(x0, x1, f), radicand=a, kind=kind, t_zero=tz)
        for side in (-1, 1):                                    # y.c1 next to (p - 1) / 2: fix y.c1, vary y.c0 until y^2 - 4 (1 + i) is a cube
            for n in range(2):
                j = (1 + n) if side > 0 else -n
                while True:
                    y = (self.rnd.randrange(P), HALF + j)
                    x = f2_cbrt(M.f2_sub(M.f2_sqr(y), M.B2))
                    if x is not None:
                        break
                assert M.g2_on_curve((x, y))
                for f in (4, 5):
                    self.add(G2C, "fp2_sqrt", "y.c1=half%+d flag %d" % (j, f), g2_enc(x[0], x[1], f), y=y, j=j)

    # -- not on the curve
    def off_curve(self):
        _, _, pk, sig = self.honest[2]
        x, y = pk
        cand = [("y+1", x, (y + 1) % P), ("y-1", x, (y - 1) % P), ("swapped", y, x)]
        for name, bit in (("low", 3), ("middle", 32 * 5 + 7), ("top", 352)):
            cand.append(("x bit %s limb" % name, x ^ (1 << bit), y))
            cand.append(("y bit %s limb" % name, x, y ^ (1 << bit)))
        for tag, cx, cy in cand:
            assert cx < P and cy < P, tag
            self.add(G1U, "off_curve", tag, g1_enc(G1U, cx, cy))
        cx = x
        while M.fp_sqrt((pow(cx, 3, P) + 4) % P) is not None:
            cx += 1
        for f in (4, 5):
            self.add(G1C, "off_curve", "radicand non-residue flag %d" % f, g1_enc(G1C, cx, flags=f))
        (x0, x1), _y = sig
        for name, bit in (("low", 3), ("middle", 32 * 5 + 7), ("top", 352)):
            for half in (0, 1):
                c0, c1 = (x0 ^ (1 << bit), x1) if half == 0 else (x0, x1 ^ (1 << bit))
                while c0 >= P or c1 >= P or M.f2_is_square(M.f2_add(M.f2_mul(M.f2_sqr((c0, c1)), (c0, c1)), M.B2)):
                    c0, c1 = (c0 ^ (2 << bit), c1) if half == 0 else (c0, c1 ^ (2 << bit))
                    bit += 1
                self.add(G2C, "off_curve", "x.c%d bit %s limb: radicand no square" % (half, name), g2_enc(c0, c1, 4))


_CASES = None


def cases():
    """{format: [Case]} -- built once per process"""
    global _CASES
    if _CASES is None:
        b = _Build()
        b.controls(); b.ranges(); b.aliases(); b.flags(); b.fp_sign(); b.fp2_sqrt(); b.off_curve()
        _CASES = b.cases
        _CASES["honest"] = b.honest
    return _CASES


def honest():
    """[(sk, msg, pk point, sig point)]: the signers of the controls"""
    return cases()["honest"]


# ------------------------------------------------------------------------------------------------ items of the verify entries
class Item:
    """one item of a verify entry built around a case: compressed signature, message, keys in the case's own key format (0 / 1), and which of them is the case"""
    __slots__ = ("case", "sig", "msg", "keys", "fmt", "at", "twin")

    def __init__(self, case, sig, msg, keys, fmt, at, twin=None):
        self.case, self.sig, self.msg, self.keys, self.fmt, self.at, self.twin = case, bytes(sig), bytes(msg), [bytes(k) for k in keys], fmt, at, twin


def _sig_bytes(msg, sk):
    return orc.g2_compress(orc.sign(msg, sk))


def key_items(fmt, k=1):
    """one item per key case of the format (G1C / G1U): the case at position (index mod k) among k - 1 honest keys, under a real signature of the honest signers
    (and the case's own signer where it has one: an alias or a control then verifies exactly when the decoder takes it for its point). Twins: an alias case
    also yields the item with its canonical bytes (Item.twin = the alias item's index); a compressed alias, whose point has no known secret key, comes
    with its negative when k >= 3 (the two cancel) and, for k = 1 and the 3-torsion points x = 0, under the infinite signature."""
    hs = honest()
    kf = 0 if fmt == G1C else 1
    items = []
    for n, c in enumerate(cases()[fmt]):
        msg = c.info.get("msg") or random.Random(n).randbytes(32)
        at = n % k
        signers = [hs[(n + t) % len(hs)] for t in range(k - 1)]
        fill = [canonical(fmt, s[2]) for s in signers]
        sks = [s[0] for s in signers] + ([c.info["sk"]] if "sk" in c.info else [])
        datas = [c.data] + ([c.canon] if c.family == "alias" else [])
        if c.family == "alias" and fmt == G1C:
            if k >= 3:                                                  # [.., Q, -Q, ..]: the two cancel, the sum is the other signers' key
                at = min(at, k - 2)
                fill[-1] = canonical(G1C, M.g1_neg(c.info["of"]))
                sks = sks[:-1]
            elif c.info["k"] == 0:
                sks = None                                              # the 3-torsion points (0, +-2) verify the infinite signature
            else:
                datas = datas[:1]                                       # no secret key, no partner: the alias alone
        sig = helpers.G2_INF if sks is None else _sig_bytes(msg, sum(sks or [hs[n % len(hs)][0]]) % M.R)
        for t, data in enumerate(datas):
            keys = list(fill); keys.insert(at, data)
            items.append(Item(c, sig, msg, keys, kf, at, twin=len(items) - 1 if t else None))
    return items


def sig_items(k=1, fmt=0):
    """one item per signature case: the case as the signature over its signer's message (a fresh message where it has none) under k honest keys whose first is
    the signer's; an alias also yields its canonical twin"""
    hs = honest()
    items = []
    for n, c in enumerate(cases()[G2C]):
        msg = c.info.get("msg") or random.Random(1000 + n).randbytes(32)
        first = M.g1_mul(M.G1, c.info["sk"]) if "sk" in c.info else hs[n % len(hs)][2]
        others = [hs[(n + 1 + t) % len(hs)] for t in range(k - 1)]
        keys = [canonical(G1C if fmt == 0 else G1U, p) for p in [first] + [o[2] for o in others]]
        items.append(Item(c, c.data, msg, keys, fmt, None))
        if c.family == "alias":
            assert k == 1                                               # (the twin's signature is the signer's alone)
            items.append(Item(c, c.canon, msg, keys, fmt, None, twin=len(items) - 1))
    return items


# ------------------------------------------------------------------------------------------------ the route table
# call site (file : enclosing function : decoder) -> (what its routes make visible, the TEST FUNCTIONS that send every case of the site's format through it:
# names of tests/test_gpu_wire.py, or -- "host": a site compiled for the host emulation only -- of tests/test_wire_cases_cpu.py). "value": the decoded point
# comes back (bytes compared with the model's); "verdict": the accept bit and the status word. tests/test_wire_cases_cpu.py asserts that the sites are
# exactly the ones in the sources and that every named function exists.
DECODERS = ("g1_decode_compressed", "g1_decode_uncompressed", "g1_decode_uncompressed_w", "g2_decode_compressed", "g2_decode_compressed_t")
RAW_ROUTINE = "mbls_g1_aggregate_rawiso_d_asm_fn"                       # the generated key sum that embeds g1_decode_raw (tools/gen_tower_d.py)
ROUTES = {
    "mbls_ops.h:op_g1_decode:g1_decode_compressed": ("value", ("test_pk_decode_batch",)),
    "mbls_ops.h:op_g1_decode:g1_decode_uncompressed": ("value", ("test_pk_decode_batch",)),
    "mbls_ops.h:op_g1_key_validate:g1_decode_uncompressed": ("value", ("test_pk_compress_batch_and_single_key_entries",)),
    "mbls_ops.h:op_g1_compress:g1_decode_uncompressed": ("value", ("test_pk_compress_batch_and_single_key_entries",)),
    "mbls_ops.h:op_g2_check:g2_decode_compressed": ("host", ("test_emulated_g2_check_and_add",)),
    "mbls_ops.h:op_keytable_append:g1_decode_compressed": ("value", ("test_keytable_append_and_export",)),
    "mbls_ops.h:op_keytable_append:g1_decode_uncompressed": ("value", ("test_keytable_append_and_export",)),
    "mbls_ops.h:op_g2_decode_affine:g2_decode_compressed": ("value", ("test_aggregate_signatures_decode_then_encode",)),
    "mbls_ops.h:op_g2_add:g2_decode_compressed": ("value", ("test_aggregate_signatures_decode_then_encode",)),
    "mbls_ops.h:op_g1_add:g1_decode_uncompressed": ("value", ("test_pk_compress_batch_and_single_key_entries",)),
    "mbls_lanes.h:lane_aggregate:g1_decode_compressed": ("value", ("test_aggregate_public_keys_batch", "test_verify_batch")),
    "mbls_lanes.h:lane_aggregate:g1_decode_uncompressed_w": ("verdict", ("test_fast_aggregate_verify_device_on_a_shifted_key_buffer",)),
    "mbls_lanes.h:lane_aggregate_d:" + RAW_ROUTINE: ("value", ("test_aggregate_public_keys_batch", "test_verify_batch", "test_fast_aggregate_verify_batch")),
    "mbls_lanes.h:lane_pk_decompress:g1_decode_compressed": ("verdict", ("test_fast_aggregate_verify_batch",)),
    "mbls_lanes.h:lane_sig:g2_decode_compressed_t": ("verdict", ("test_verify_batch", "test_fast_aggregate_verify_batch", "test_verify_multiple_rng_entry_one_set_per_batch")),
    "mbls_lanes.h:lane_sig:g2_decode_compressed": ("host", ("test_emulated_verify_batch_signature_phase",)),
    "mbls_kernels.hip:k_blind_g1:g1_decode_uncompressed": ("verdict", ("test_aggregate_verify_batch",)),
    "mbls_kernels.hip:k_blind_g1_d:g1_decode_uncompressed": ("verdict", ("test_verify_multiple_batches_of_one_set", "test_verify_multiple_rng_entry_one_set_per_batch")),
    "mbls_kernels.hip:k_blind_sig_d:g2_decode_compressed_t": ("verdict", ("test_verify_multiple_batches_of_one_set",)),
    "mbls_kernels.hip:k_blind_sig2_d:g2_decode_compressed_t": ("verdict", ("test_verify_multiple_batches_of_one_set",)),
    "mbls_kernels.hip:k_sig2:g2_decode_compressed_t": ("verdict", ("test_verify_batch", "test_verify_multiple_rng_entry_one_set_per_batch")),
    "mbls_kernels.hip:k_g2_check:g2_decode_compressed_t": ("value", ("test_sig_check_batch",)),
}
ROUTE_MODULES = {"value": "test_gpu_wire.py", "verdict": "test_gpu_wire.py", "host": "test_wire_cases_cpu.py"}


def decode_sites():
    """the call sites of the decoders in milagro_bls_amd/csrc/*.h, *.hip as ROUTES spells them (a decoder calling a decoder is a wrapper, not a site). The
    enclosing function is the last definition head in front of the call: a line that starts with a function qualifier, names the function in front of its first
    parenthesis (launch bounds and attributes set aside) and is not a prototype; a body on the head's own line belongs to it."""
    d = os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc")
    call = re.compile(r"\b(%s)\s*(?:<[^<>()]*>)?\s*\(" % "|".join(sorted(DECODERS, key=len, reverse=True)))
    asm_call = re.compile(r'MBLS_ASM_CALL\("(%s)"\)' % RAW_ROUTINE)
    aside = re.compile(r"__launch_bounds__\s*\([^()]*\)|__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)|extern\s+\"C\"")
    head = re.compile(r"^(?:template\s*<[^>]*>\s*)?\s*(?:MBLS_FN|MBLS_NOINLINE|__global__|__device__|static|inline)\b[^;{(=]*?\b(\w+)\s*\(")
    sites = set()
    for name in sorted(os.listdir(d)):
        if not name.endswith((".h", ".hip")):
            continue
        fn = None
        with open(os.path.join(d, name)) as f:
            for line in f:
                code = aside.sub(" ", line.split("//")[0]).strip()
                m = head.match(code)
                defined = None
                if m and not code.endswith(");"):
                    fn = defined = m.group(1)
                for c in list(call.finditer(code)) + list(asm_call.finditer(code)):
                    if c.group(1) == defined or fn in DECODERS:
                        continue
                    sites.add("%s:%s:%s" % (name, fn, c.group(1)))
    return sites
