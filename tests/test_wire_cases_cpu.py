"""The wire-encoding case lists (tests/wire_cases.py) without a GPU: every family's predicate on the model, the C oracle against the model on every case,
the compiled decoders on the host (tests/host_emul) against the model on every case, the hand-written 96-byte decoder g1_decode_raw in the interpreter on
every 96-byte case, and the route table against the call sites of the decoders in the sources."""
import ctypes as C
import os
import re
import sys

import bls12_381 as M

import helpers
import orc
import wire_cases as W

sys.path.insert(0, os.path.join(helpers.ROOT, "tools"))

P = M.P
CS = W.cases()
EMUL_ERR = {W.OK_FINITE: 0, W.OK_INF: 0, W.SIZE: 1, W.POINT: 3}            # MBLS_DEC_* of mbls_curve.h, as the bodies return them
ST_BAD_PK, ST_APK_INF, ST_PK_INF = 0x04, 0x08, 0x20


def fam(fmt, family):
    out = [c for c in CS[fmt] if c.family == family]
    assert out, (fmt, family)
    return out


def field(c, name):
    """the raw integer a coordinate field of the case holds (flag bits masked where the format masks them)"""
    d = c.data
    if c.fmt == W.G1C:
        return int.from_bytes(bytes([d[0] & 0x1F]) + d[1:], "big")
    if c.fmt == W.G1U:
        return int.from_bytes(d[:48] if name == "x" else d[48:], "big")
    return int.from_bytes(bytes([d[0] & 0x1F]) + d[1:48], "big") if name == "c1" else int.from_bytes(d[48:], "big")


# ------------------------------------------------------------------------------------------------ the families are what they say
def test_every_family_is_present_in_every_list():
    for fmt in W.FORMATS:
        have = {c.family for c in CS[fmt]}
        assert have == set(W.FAMILIES) - {"fp2_sqrt" if fmt != W.G2C else "fp_sign"}, (fmt, have)
        assert len(CS[fmt]) <= 500


def test_range_family():
    for fmt, fields in ((W.G1C, ("x",)), (W.G1U, ("x", "y")), (W.G2C, ("c1", "c0"))):
        cs = fam(fmt, "range")
        for f in fields:
            bits = 384 if (fmt, f) in ((W.G1U, "y"), (W.G2C, "c0")) else 381
            mine = [c for c in cs if c.info.get("field", "x") == f]
            vals = {field(c, f) for c in mine}
            assert vals == {v for _, v in W.range_values(bits)}, (fmt, f)
            for j in range(12):
                assert P - (1 << 32 * j) in vals and P + (1 << 32 * j) in vals
            assert {P - 1, P, P + 1, (1 << 381) - 1} <= vals and ((1 << 384) - 1 in vals) == (bits == 384)
            for c in mine:
                assert c.info["value"] == field(c, f)
                if c.info["value"] >= P:
                    assert c.cls == W.POINT, c
            assert any(c.ok for c in mine if c.info["value"] < P) or fmt == W.G1U
    # 96-byte keys: at least one value above p per field whose REDUCED point is on the curve (a decoder that reduces takes it for a valid key)
    for f in ("x", "y"):
        hit = [c for c in fam(W.G1U, "range") if c.info["field"] == f and c.info["value"] >= P and c.info["partner"]]
        assert hit, f
        for c in hit:
            assert M.g1_on_curve((field(c, "x") % P, field(c, "y") % P)) and c.cls == W.POINT


def test_alias_family():
    for c in fam(W.G1C, "alias"):
        x = field(c, "x")
        assert x - P == c.info["k"] and c.info["k"] in W.ALIAS_K and c.cls == W.POINT
        e, pt = M.g1_decompress(c.canon)
        assert e == 0 and pt == c.info["of"] and pt[0] == x % P and M.g1_on_curve(pt) and bool(c.data[0] & 0x20) == bool(c.canon[0] & 0x20)
    assert {c.info["k"] for c in fam(W.G1C, "alias")} == set(W.ALIAS_K)
    tags = set()
    for c in fam(W.G1U, "alias"):
        x, y = field(c, "x"), field(c, "y")
        assert (x % P, y % P) == c.info["of"] and (x, y) != c.info["of"] and c.cls == W.POINT and W.classify(W.G1U, c.canon) == (W.OK_FINITE, c.info["of"])
        assert M.subgroup_check_g1(c.info["of"]) if c.tag.endswith("honest 0") else True
        tags.add(c.tag.split(" ")[0] + ("" if c.info["flagless"] else " flagged"))
    assert {"x+p", "y+p", "x+2p flagged"} <= tags
    kinds = set()
    for c in fam(W.G2C, "alias"):
        x0, x1 = field(c, "c0"), field(c, "c1")
        assert (x0 % P, x1 % P) == c.info["of"][0] and (x0 >= P) != (x1 >= P) and c.cls == W.POINT
        assert W.classify(W.G2C, c.canon) == (W.OK_FINITE, c.info["of"]) and (c.data[0] & 0xE0) == (c.canon[0] & 0xE0)
        kinds.add("c0" if x0 >= P else "c1")
    assert kinds == {"c0", "c1"}


def test_flags_family():
    for fmt in W.FORMATS:
        cs = fam(fmt, "flags")
        assert {(c.info["flag"], c.info["body"]) for c in cs} == {(f, b) for f in range(8) for b in ("honest", "zero", "stray last", "stray first", "stray middle")}
        by = {(c.info["flag"], c.info["body"]): c for c in cs}
        for (f, body), c in by.items():
            assert c.data[0] >> 5 == f
            compressed = fmt != W.G1U
            if bool(f & 4) != compressed:
                assert c.cls == W.SIZE, c
            elif f & 2:
                assert c.cls == (W.OK_INF if body == "zero" and not f & 1 else W.POINT), c          # 0xC0 || 0 (0x40 || 0) alone is infinity; 0xE0 || 0 is not
            elif fmt == W.G1U and f & 1:
                assert c.cls == W.POINT, c                                                           # the sign flag on a 96-byte key
        if fmt == W.G1C:                                                                             # 0x80 || 0 and 0xA0 || 0: the points (0, +-2), outside G1
            assert by[(4, "zero")].point == (0, 2) and by[(5, "zero")].point == (0, P - 2) and not M.subgroup_check_g1((0, 2))
            assert by[(5, "honest")].point == M.g1_neg(by[(4, "honest")].point)
        if fmt == W.G1U:
            assert by[(0, "honest")].cls == W.OK_FINITE and by[(1, "honest")].cls == W.POINT


def test_fp_sign_family():
    near = sorted({c.info["j"] for c in fam(W.G1C, "fp_sign") if "j" in c.info})
    assert len([j for j in near if j <= 0]) == 2 and len([j for j in near if j > 0]) == 2
    for j in range(min(near), max(near) + 1):                              # ... and they are the NEAREST: no curve point in between
        if j not in near:
            assert W.fp_cbrt((W.HALF + j) ** 2 - 4) is None
    for fmt in (W.G1C, W.G1U):
        limbs = set()
        for c in fam(fmt, "fp_sign"):
            assert c.cls == W.OK_FINITE and c.point[1] in (c.info["y"], P - c.info["y"])
            if fmt == W.G1U:
                assert c.point[1] == c.info["y"]
            else:
                assert M.fp_lex_largest(c.point[1]) == bool(c.data[0] & 0x20)
            if "limb" in c.info:
                y = c.info["y"] if fmt == W.G1C or "negated" not in c.tag else P - c.info["y"]
                assert W.top_limb_diff(y, W.HALF) == c.info["limb"]
                limbs.add((c.info["limb"], y > W.HALF))
        assert limbs == {(j, s) for j in range(12) for s in (False, True)}


def test_fp2_sqrt_family():
    kinds = {"real": 0, "imag": 0}
    near = set()
    for c in fam(W.G2C, "fp2_sqrt"):
        assert c.cls == W.OK_FINITE and M.g2_on_curve(c.point) and M.f2_lex_largest(c.point[1]) == bool(c.data[0] & 0x20)
        x = c.point[0]
        a = M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.B2)
        if "kind" in c.info:
            assert a[1] == 0 and a == c.info["radicand"]
            residue = M.fp_sqrt(a[0]) is not None
            assert (c.point[1][1] == 0) == residue == (c.info["kind"] == "real") and (c.point[1][0] == 0) == (not residue)
            assert c.info["t_zero"] == (not residue)                      # fp2_sqrt_inl: t = (a0 + s) / 2 with s = sqrt(a0^2) the residue among +-a0
            kinds[c.info["kind"]] += 1
        else:
            assert c.point[1][1] in (W.HALF + c.info["j"], P - W.HALF - c.info["j"]) and abs(c.info["j"]) <= 2
            near.add(c.info["j"])
    assert kinds["real"] >= 8 and kinds["imag"] >= 8                      # four points of each kind, both flag values
    assert len([j for j in near if j <= 0]) == 2 and len([j for j in near if j > 0]) == 2


def test_off_curve_family():
    for fmt in W.FORMATS:
        for c in fam(fmt, "off_curve"):
            assert c.cls == W.POINT
            for f in {W.G1C: ("x",), W.G1U: ("x", "y"), W.G2C: ("c0", "c1")}[fmt]:
                assert field(c, f) < P                                     # in range, flags in order: only the curve equation refuses it
            assert c.data[0] >> 5 in ((0,) if fmt == W.G1U else (4, 5))


# ------------------------------------------------------------------------------------------------ the C oracle agrees with the model
def test_oracle_decoders_agree_with_the_model():
    for c in CS[W.G1C]:
        assert orc.g1_from_compressed(c.data) == (c.err, W.uncompressed(W.G1C, c.point) if c.ok else None), c
        e, out = orc.pk_from_bytes(c.data)
        # in G1 by construction: the honest keys (and their negatives); every other decodable case is a curve point found by its coordinates, in G1 with
        # probability 1 / cofactor -- the model's [r] P is run on the honest ones and on a sample of the others (it costs 0.1 s a point)
        valid = c.cls == W.OK_FINITE and (c.family == "control" or (c.family == "flags" and c.info["body"] == "honest"))
        if c.cls == W.OK_FINITE and (valid or c.tag.endswith("flag 4") and c.family == "range"):
            assert M.subgroup_check_g1(c.point) == valid, c
        assert (e, out) == ((0, W.uncompressed(W.G1C, c.point)) if valid else (c.err or W.ERR_INVALID_POINT, None)), c
    for c in CS[W.G1U]:
        assert orc.g1_from_uncompressed(c.data) == (c.err, W.uncompressed(W.G1U, c.point) if c.ok else None), c
    for c in CS[W.G2C]:
        assert orc.g2_from_compressed(c.data) == (c.err, W.uncompressed(W.G2C, c.point) if c.ok else None), c


# ------------------------------------------------------------------------------------------------ the compiled bodies on the host
def _g1_valid(c):
    return c.cls == W.OK_FINITE and orc.g1_key_validate(W.uncompressed(c.fmt, c.point))


def test_emulated_g1_decode_and_compress(emul):
    for fmt, kf in ((W.G1C, 0), (W.G1U, 1)):
        cs = CS[fmt]
        n = len(cs)
        blob = b"".join(c.data for c in cs)
        for validate in (0, 1):
            out, err = helpers.ob(96 * n), helpers.ob(n)
            emul.emul_g1_decode(helpers.cb(blob), kf, validate, C.c_uint64(n), out, err)
            for i, c in enumerate(cs):
                good = _g1_valid(c) if validate else c.ok
                want = (0, W.uncompressed(fmt, c.point)) if good else (EMUL_ERR[c.cls] or 3, bytes(96))
                assert (err[i], bytes(out[96 * i:96 * i + 96])) == want, (c, validate)
    cs = CS[W.G1U]
    n = len(cs)
    out, err = helpers.ob(48 * n), helpers.ob(n)
    emul.emul_g1_compress(helpers.cb(b"".join(c.data for c in cs)), C.c_uint64(n), out, err)
    for i, c in enumerate(cs):
        assert (err[i], bytes(out[48 * i:48 * i + 48])) == (EMUL_ERR[c.cls], M.g1_compress(c.point) if c.ok else bytes(48)), c


def test_emulated_g1_add_pins_the_root(emul):
    """case + an honest key: the sum shows WHICH root a compressed key decoded to even if decoder and encoder shared a wrong sign rule (96-byte keys: the point as given)"""
    g = W.honest()[0][2]
    cs = CS[W.G1U]
    n = len(cs)
    out, err = helpers.ob(96 * n), helpers.ob(n)
    emul.emul_g1_add(helpers.cb(b"".join(c.data for c in cs)), helpers.cb(M.g1_serialize_uncompressed(g) * n), C.c_uint64(n), out, err)
    for i, c in enumerate(cs):
        want = (0, M.g1_serialize_uncompressed(M.g1_add(c.point, g))) if c.ok else (EMUL_ERR[c.cls], bytes(96))
        assert (err[i], bytes(out[96 * i:96 * i + 96])) == want, c


def test_emulated_g2_check_and_add(emul):
    cs = CS[W.G2C]
    n = len(cs)
    blob = helpers.cb(b"".join(c.data for c in cs))
    err, ing2 = helpers.ob(n), helpers.ob(n)
    emul.emul_g2_check(blob, C.c_uint64(n), err, ing2)
    for i, c in enumerate(cs):
        assert err[i] == EMUL_ERR[c.cls], c
        assert bool(ing2[i]) == (c.ok and orc.g2_subgroup_check(W.uncompressed(W.G2C, c.point))), c
    # decode -> + honest signature -> encode: the sum pins the root the decoder chose (decode -> encode alone would hide a sign rule that is wrong on both sides)
    g = W.honest()[0][3]
    out = helpers.ob(96 * n)
    emul.emul_g2_add(blob, helpers.cb(M.g2_compress(g) * n), C.c_uint64(n), out, err)
    for i, c in enumerate(cs):
        want = (0, M.g2_compress(M.g2_add(c.point, g))) if c.ok else (EMUL_ERR[c.cls], bytes(96))
        assert (err[i], bytes(out[96 * i:96 * i + 96])) == want, c
    emul.emul_g2_add(blob, helpers.cb(helpers.G2_INF * n), C.c_uint64(n), out, err)          # + infinity: the canonical bytes of the model's point
    for i, c in enumerate(cs):
        assert (err[i], bytes(out[96 * i:96 * i + 96])) == ((0, M.g2_compress(c.point)) if c.ok else (EMUL_ERR[c.cls], bytes(96))), c


def test_emulated_verify_batch_signature_phase(emul):
    """lane_sig as the host emulation compiles it (no LDS: the out-of-line g2_decode_compressed) inside the whole verify pipeline: every signature case under its
    signer's key -> the status bits of the model's class and the oracle's verdict"""
    items = W.sig_items()
    n = len(items)
    res, st = helpers.ob(n), (C.c_uint32 * n)()
    emul.emul_verify_batch(helpers.cb(b"".join(it.sig for it in items)), helpers.cb(b"".join(it.msg for it in items)), C.c_uint32(32),
                           helpers.cb(b"".join(it.keys[0] for it in items)), 0, None, C.c_uint64(n), C.c_uint32(1), 1, res, st)
    twins = 0
    for i, it in enumerate(items):
        cls, pt = W.classify(W.G2C, it.sig)
        ok = cls in (W.OK_FINITE, W.OK_INF)
        outside = cls == W.OK_FINITE and not orc.g2_subgroup_check(W.uncompressed(W.G2C, pt))
        assert (st[i] & 0x3F) == (0 if ok else 0x01) | (0x02 if outside else 0), (it.case, hex(st[i]))
        es, sig = orc.g2_from_compressed(it.sig)
        want = es == 0 and orc.verify(sig, it.msg, orc.g1_from_compressed(it.keys[0])[1])
        assert bool(res[i]) == want, (it.case, hex(st[i]))
        if it.twin is not None:                                           # the canonical twin is accepted with a clean word, its alias refused for its encoding
            assert res[i] and st[i] == 0 and not res[it.twin] and st[it.twin] & 0x01, it.case
            twins += 1
    assert twins >= 6


def aggregate_expectation(cases_at, honest_pts):
    """(status, sum bytes) of a key sum in MBLS_MODE_FAST_AGGREGATE whose keys are model points / Cases: an undecodable key counts as infinity and sets both bits"""
    st, acc = 0, None
    for k in cases_at:
        if isinstance(k, W.Case):
            if not k.ok:
                st |= ST_BAD_PK | ST_PK_INF
            elif k.point is None:
                st |= ST_PK_INF
            acc = M.g1_add(acc, k.point if k.ok else None)
        else:
            acc = M.g1_add(acc, k)
    if acc is None:
        st |= ST_APK_INF
    return st, M.g1_serialize_uncompressed(acc)


def test_emulated_aggregate_alone_and_among_three(emul):
    h = [s[2] for s in W.honest()]
    for fmt, kf in ((W.G1C, 0), (W.G1U, 1)):
        for k, at in ((1, 0), (3, 0), (3, 1), (3, 2)):
            cs = CS[fmt]
            n = len(cs)
            rows = []
            for i, c in enumerate(cs):
                keys = [h[(i + t) % len(h)] for t in range(k - 1)]
                keys.insert(at, c)
                rows.append(keys)
            blob = b"".join(x.data if isinstance(x, W.Case) else W.canonical(fmt, x) for r in rows for x in r)
            out, st = helpers.ob(96 * n), (C.c_uint32 * n)()
            emul.emul_aggregate(helpers.cb(blob), kf, None, C.c_uint64(n), C.c_uint32(k), out, st)
            for i, r in enumerate(rows):
                assert (st[i], bytes(out[96 * i:96 * i + 96])) == aggregate_expectation(r, None), (cs[i], k, at)


# ------------------------------------------------------------------------------------------------ the hand-written decoder in the interpreter
def test_g1_decode_raw_on_every_96_byte_case():
    """g1_decode_raw (tools/gen_tower_d.py: flag tests and the 12-limb borrow chains against p, inside the generated key sum) on every 96-byte case: the
    infinity / undecodable masks and, for a key that passes flags and range, the plain digits of x and y. The curve equation is the routine body's business
    (tests/test_asm_sim_d_cpu.py), so a case the model refuses for that alone comes out of the decoder unflagged."""
    import gen_fpd_asm as d
    import gen_tower_d as t
    from asm_sim import Machine, from_digits_signed
    rout = {k: f() for k, f in d.ROUTINE_BODIES.items()}
    dec = t.g1_decode_raw()
    const = t.shell_constants()
    seen = set()
    for c in CS[W.G1U]:
        blob = c.data
        x, y = field(c, "x"), field(c, "y")
        f = blob[0] >> 5
        if f & 4:
            inf, bad = 1, 1
        elif f & 2:
            bad = int(blob != bytes([0x40]) + bytes(95)); inf = 1
        else:
            bad = int(bool(f & 1) or x >= P or y >= P); inf = bad
        if not bad:
            assert (c.cls == W.OK_INF) if inf else (c.ok == M.g1_on_curve((x, y))), c
        else:
            assert not c.ok, c
        m = Machine(rout); m.run(const); m.s[77] = 0x00010203
        for j in range(24):
            m.v[224 + j] = int.from_bytes(blob[4 * j:4 * j + 4], "little")
        for j in range(12):
            m.v[196 + j] = t.P_LIMBS[j]
        m.run(dec)
        assert (m.s[("pair", 48)], m.s[("pair", 88)]) == (inf, bad), c
        if not inf:
            assert from_digits_signed(m.v[112:126]) == x and from_digits_signed(m.v[126:140]) == y, c
        seen.add((inf, bad))
    assert seen == {(0, 0), (1, 0), (1, 1)}


# ------------------------------------------------------------------------------------------------ the route table is complete
def test_every_decode_site_has_a_route():
    sites = W.decode_sites()
    assert sites == set(W.ROUTES), (sorted(sites - set(W.ROUTES)), sorted(set(W.ROUTES) - sites))
    assert all(kind in ("value", "verdict", "host") and routes for kind, routes in W.ROUTES.values())
    # every route is a test function that exists in the module its kind names
    for site, (kind, routes) in W.ROUTES.items():
        with open(os.path.join(helpers.ROOT, "tests", W.ROUTE_MODULES[kind])) as f:
            src = f.read()
        for r in routes:
            assert re.search(r"^def %s\(" % re.escape(r), src, re.M), (site, r)
    # the generated key sums: the one over 96-byte keys is built from g1_decode_raw's lines, the one over table indices decodes nothing
    import gen_tower_d as t
    assert t.g1_aggregate_d_routine("rawiso")[1]["decode"] == t.g1_decode_raw() != t.g1_aggregate_d_routine("indexed")[1]["decode"]
