"""The two halves of the pairing on the GPU, value for value (tests/pairing_cases.py): the Miller loop through mbls_miller_probe in its six forms -- the compiled
body, k_miller, k_miller_single on one lane and on a lane pair, the wave programs miller1 and smiller -- and the final exponentiation through
mbls_final_exp_probe -- the compiled body, k_final's and k_final2's routines, the wave program vmfinal (a verdict only). Every comparison is against the Python
model's value from the case list: the final exponentiation bit-exact on all 12 coefficients, a Miller value after the easy part of the exponentiation (which kills
exactly the subfield factors the projective formulas drop). No GPU form is ever the reference of another; which forms agree is reported in failure messages only."""
import pytest

import pairing_cases as pc
from pymodel import bls12_381 as M

pytestmark = pytest.mark.gpu

# form -> (which of the case's expectations it computes, the exported value is the conjugate): include/mbls.h, mbls_miller_probe
MILLER_FORMS = {"body": ("two", False), "two_pair": ("two", False), "one_pair": ("one", False), "one_pair_lane_pair": ("one", False), "miller1": ("one", False),
                "smiller": ("s", True)}
FE_VALUE_FORMS = ("body", "lane", "lane_pair")
ONE = pc.pack12(M.F12_ONE)


@pytest.fixture(scope="module")
def mb():
    from milagro_bls_amd import batch, _native
    _native.default_context()
    return batch


def split(b, n):
    return [b[576 * i:576 * i + 576] for i in range(n)]


def run_miller(mb, form, items):
    return split(mb.miller_probe(b"".join(c.packed for c in items), len(items), form), len(items))


def run_fe(mb, form, items):
    """(values or None, is_one bits, equal-lanes bits or None) of the probe on a list of cases (or of packed elements)"""
    buf = b"".join(c if isinstance(c, bytes) else c.packed for c in items)
    values, bits, equal = mb.final_exp_probe(buf, len(items), form)
    return (None if values is None else split(values, len(items))), bits, equal


def miller_wrong(form, items, got):
    kind, conj = MILLER_FORMS[form]
    return [(i, c.name) for i, (c, g) in enumerate(zip(items, got)) if not pc.miller_value_matches(c, kind, g, conj)]


def fe_wrong(items, values, bits, equal):
    """(index, case, what) wherever a value form differs from the model: the value (none is asserted for 0), the bit, the equal-lanes flag"""
    bad = []
    for i, c in enumerate(items):
        if c.expected is not None and values[i] != c.expected_packed:
            bad.append((i, c.name, "value"))
        if bits[i] != c.is_one:
            bad.append((i, c.name, "is_one"))
        if equal is not None and not equal[i]:
            bad.append((i, c.name, "lanes differ"))
    return bad


# ---------------------------------------------------------------------------------------------- every case in every form
def test_final_exponentiation_every_case_in_every_value_form(mb):
    items = list(pc.fe_cases())
    assert len(items) <= pc.MAX_CASES
    got = {form: run_fe(mb, form, items) for form in FE_VALUE_FORMS}
    wrong = {form: fe_wrong(items, *got[form]) for form in FE_VALUE_FORMS}
    agree = {c.name: len({got[f][0][i] for f in FE_VALUE_FORMS}) == 1 for i, c in enumerate(items)}
    names = {n for w in wrong.values() for _, n, _ in w}
    assert not any(wrong.values()), "forms that differ from the model: %r; all three forms equal there: %r" % (wrong, {n: agree[n] for n in names})


def test_final_exponentiation_verdict_form(mb):
    """program vmfinal, a wave per case: slot F = f, 1 beside it"""
    items = list(pc.fe_cases())
    values, bits, equal = run_fe(mb, "vmfinal", items)
    assert values is None and equal is None
    bad = [c.name for c, b in zip(items, bits) if b != c.is_one]
    assert not bad, bad


def test_miller_loop_every_case_in_every_form(mb):
    items = list(pc.miller_cases())
    assert len(items) <= pc.MAX_CASES
    got = {form: run_miller(mb, form, items) for form in MILLER_FORMS}
    wrong = {form: miller_wrong(form, items, got[form]) for form in MILLER_FORMS}
    groups = (("body", "two_pair"), ("one_pair", "one_pair_lane_pair", "miller1"))
    agree = {c.name: [len({got[f][i] for f in g}) == 1 for g in groups] for i, c in enumerate(items)}
    names = {n for w in wrong.values() for _, n in w}
    assert not any(wrong.values()), "forms that differ from the model: %r; the two-pair forms / the one-pair forms byte-equal there: %r" % (
        wrong, {n: agree[n] for n in names})
    # an infinite member contributes exactly 1: as a value, not only after the easy part
    by = {c.name: i for i, c in enumerate(items)}
    for form, (kind, _) in MILLER_FORMS.items():
        for c in items:
            if c.contributes_one(kind):
                assert got[form][by[c.name]] == ONE, (form, c.name)


# ---------------------------------------------------------------------------------------------- lane layouts
def placements(n, per_wave):
    """name -> the indices of n items that hold the special case; the rest are general cases in turn"""
    sets = {"none": (), "first": (0,), "all": tuple(range(n)), "odd": tuple(range(1, n, 2)), "last_live": (n - 1,)}
    if n > per_wave:
        sets["wave_edge"] = (per_wave - 1, per_wave)              # the last item of the first workgroup, the first of the second
    elif n == per_wave:
        sets["wave_edge"] = (per_wave - 1,)
    seen, out = set(), {}
    for name, at in sets.items():
        if at not in seen:
            seen.add(at); out[name] = at
    return out


def layouts(forms_sizes, specials):
    out = []
    for form, sizes, per_wave in forms_sizes:
        for n in sizes:
            for where, at in placements(n, per_wave).items():
                for sp in specials(form) if where != "none" else (None,):
                    out.append((form, n, where, sp, at))
    return out


def lay(n, at, special, general):
    return [special if i in at else general[i % len(general)] for i in range(n)]


FE_LAYOUTS = layouts([("body", (1, 64, 65, 130), 64), ("lane", (1, 64, 65, 130), 64), ("lane_pair", (1, 32, 33, 130), 32), ("vmfinal", (1, 3), 1)],
                     lambda form: ("in_fp6",) if form != "lane_pair" else ("in_fp6", "rth_power"))


@pytest.mark.parametrize("form,n,where,special,at", FE_LAYOUTS, ids=["%s-%d-%s-%s" % x[:4] for x in FE_LAYOUTS])
def test_final_exponentiation_lane_layouts(mb, form, n, where, special, at):
    """one item, one full wave, a wave and one item, two waves and two items (workgroups of 64 lanes: 32 items each for the lane-pair form); an element
    the easy part sends to 1 -- the all-zero compressed state -- at the first lane, at the edge between two workgroups, on every odd item, on the last live
    item, on all items, among general elements. The lane pairs also with an r-th power: the value 1 behind a general chain on one pair of a wave"""
    items = lay(n, set(at), pc.fe_by_name().get(special), pc.fe_general())
    values, bits, equal = run_fe(mb, form, items)
    if form == "vmfinal":
        assert [c.name for c, b in zip(items, bits) if b != c.is_one] == []
    else:
        assert fe_wrong(items, values, bits, equal) == []


def miller_specials(form):
    if form == "smiller":
        return ("h_infinite",)
    return ("apk_infinite", "sig_infinite") if MILLER_FORMS[form][0] == "two" else ("apk_infinite",)


MILLER_LAYOUTS = layouts([("body", (1, 64, 65, 130), 64), ("two_pair", (1, 64, 65, 130), 64), ("one_pair", (1, 64, 65, 130), 64), ("one_pair_lane_pair", (1, 32, 33, 130), 32),
                          ("miller1", (1, 3), 1), ("smiller", (1, 3), 1)], miller_specials)


@pytest.mark.parametrize("form,n,where,special,at", MILLER_LAYOUTS, ids=["%s-%d-%s-%s" % x[:4] for x in MILLER_LAYOUTS])
def test_miller_loop_lane_layouts(mb, form, n, where, special, at):
    """the same shapes for the Miller forms, the special item a pair with an infinite member (its skip flag set on single lanes of a wave, on the odd item of
    a lane pair's workgroup, everywhere) and, in the two-pair forms, an infinite signature beside a finite (H, apk)"""
    items = lay(n, set(at), pc.miller_by_name().get(special), pc.miller_general())
    assert miller_wrong(form, items, run_miller(mb, form, items)) == []


# ---------------------------------------------------------------------------------------------- the forms compose
def pair_as_h_apk(sig, g1):
    """the operands that make a one-pair form walk (sig, g1): sig as H (Z = 1), g1 as the key"""
    vals = [g1[0], g1[1], 1, 0, 0, 0, 0, sig[0][0], sig[0][1], sig[1][0], sig[1][1], 1, 0]
    return b"".join(v.to_bytes(48, "big") for v in vals)


@pytest.mark.parametrize("form", list(MILLER_FORMS))
def test_miller_forms_feed_the_final_exponentiation(mb, form):
    """the valid and the spoiled item: each Miller form's value -- for the one-pair forms the product of its two values, for smiller the conjugate of its value
    times the model's f(H, apk): the conventions include/mbls.h states -- through every form of the final exponentiation: 1 and not 1"""
    by = pc.miller_by_name()
    items = [by["valid_item"], by["spoiled_item"]]
    kind, conj = MILLER_FORMS[form]
    got = [pc.unpack12(g) for g in run_miller(mb, form, items)]
    if kind == "one":
        sig_pair = b"".join(pair_as_h_apk(c.sig, pc.NEG_G1) for c in items)
        other = [pc.unpack12(g) for g in split(mb.miller_probe(sig_pair, 2, form), 2)]
        got = [M.f12_mul(a, b) for a, b in zip(got, other)]
    elif kind == "s":             # the form read H as S: f(H, -G1); the items as (S = sig) need the probe again
        s_items = b"".join(pair_as_h_apk(c.sig, pc.NEG_G1) for c in items)
        got = [M.f12_mul(M.f12_conj(pc.unpack12(g)), c.model["one"]) for g, c in zip(split(mb.miller_probe(s_items, 2, form), 2), items)]
    packed = [pc.pack12(f) for f in got]
    for fe_form in FE_VALUE_FORMS + ("vmfinal",):
        values, bits, equal = run_fe(mb, fe_form, packed)
        assert bits == [True, False], (form, fe_form)
        if values is not None:
            assert values[0] == ONE and values[1] != ONE
            assert values[1] == pc.pack12(M.f12_pow(pc.fe(items[1].model["two"]), 3)), (form, fe_form)        # the subfield factors are gone: the model's value itself


# ---------------------------------------------------------------------------------------------- nothing leaks, refusals
@pytest.mark.parametrize("form", list(MILLER_FORMS))
def test_miller_probe_after_a_call_of_zeros(mb, form):
    """64 items of all-zero operands (every member infinite: every value exactly 1), then the list in the same context and form: the workspace slots, the
    running points and the skip flags a call leaves behind are the next call's to overwrite"""
    assert split(mb.miller_probe(bytes(624 * 64), 64, form), 64) == [ONE] * 64
    items = list(pc.miller_cases())
    assert miller_wrong(form, items, run_miller(mb, form, items)) == []


@pytest.mark.parametrize("form", FE_VALUE_FORMS + ("vmfinal",))
def test_final_exp_probe_after_a_call_of_zeros(mb, form):
    values, bits, equal = run_fe(mb, form, [bytes(576)] * 64)
    assert bits == [False] * 64 and (equal is None or all(equal))
    items = list(pc.fe_cases())
    values, bits, equal = run_fe(mb, form, items)
    if form == "vmfinal":
        assert [c.name for c, b in zip(items, bits) if b != c.is_one] == []
    else:
        assert fe_wrong(items, values, bits, equal) == []


def test_argument_refusals(mb):
    """a coefficient not below p, a mode that does not exist and null buffers: MBLS_ERR_ARGUMENT, nothing written"""
    from milagro_bls_amd import _native as N
    lib, h = N.lib(), N.default_context().handle
    good_m, good_f = pc.miller_general()[0].packed, pc.fe_general()[0].packed
    p48 = pc.P.to_bytes(48, "big")
    canary = bytes([0xA5]) * 576

    def miller(buf, out, mode, n=1):
        return lib.mbls_miller_probe(h, buf, n, out, mode)

    def fexp(buf, out, bits, mode, n=1):
        return lib.mbls_final_exp_probe(h, buf, n, out, bits, mode)
    for k in range(13):                                           # p itself in each of the 13 operands, in the second of two items
        out = N.cbuf(canary * 2)
        bad = good_m[:48 * k] + p48 + good_m[48 * k + 48:]
        assert miller(N.cbuf(good_m + bad), out, 1, 2) == N.ERR_ARGUMENT and bytes(out) == canary * 2, k
    for k in range(12):
        out, bits = N.cbuf(canary * 2), N.cbuf(b"\x07\x07")
        bad = good_f[:48 * k] + bytes([0xFF]) * 48 + good_f[48 * k + 48:]
        assert fexp(N.cbuf(good_f + bad), out, bits, 1, 2) == N.ERR_ARGUMENT and bytes(out) == canary * 2 and bytes(bits) == b"\x07\x07", k
    out, bits = N.cbuf(canary), N.cbuf(b"\x07")
    for mode in (-1, 6):
        assert miller(N.cbuf(good_m), out, mode) == N.ERR_ARGUMENT
    for mode in (-1, 4):
        assert fexp(N.cbuf(good_f), out, bits, mode) == N.ERR_ARGUMENT
    assert miller(None, out, 1) == N.ERR_ARGUMENT and miller(N.cbuf(good_m), None, 1) == N.ERR_ARGUMENT
    assert lib.mbls_miller_probe(None, N.cbuf(good_m), 1, out, 1) == N.ERR_ARGUMENT
    assert fexp(None, out, bits, 1) == N.ERR_ARGUMENT and fexp(N.cbuf(good_f), None, bits, 1) == N.ERR_ARGUMENT and fexp(N.cbuf(good_f), out, None, 1) == N.ERR_ARGUMENT
    assert fexp(N.cbuf(good_f), out, None, 3) == N.ERR_ARGUMENT
    assert bytes(out) == canary and bytes(bits) == b"\x07"
    # the verdict form takes no value buffer; n = 0 is a call that does nothing
    assert fexp(N.cbuf(good_f), None, bits, 3) == N.OK and bytes(bits) == b"\x00"
    assert miller(None, out, 1, 0) == N.OK and fexp(None, out, bits, 1, 0) == N.OK and bytes(out) == canary
