"""The generated digit-form leaves (tools/gen_fpd_asm.py) and passes (tools/gen_tower_d.py) on tools/asm_sim.py at the inputs their own generator admits
(tests/dform_cases.py): the interpreter's overflow assertions stay silent, values agree with big-integer arithmetic, digits 0..12 come out normalised, results
lie inside the bound the allocator goes on with, operands survive where the contract says so. The same cases run on the GPU in tests/test_gpu_dform.py.
Also here: mutants of the bodies that the cases must catch, and the walk over every site that emits a quotient-estimate pass (gen_tower_d.QSITES)."""
import pytest

import dform_cases as dc
from dform_cases import t, P


@pytest.mark.parametrize("name", list(dc.OP))
def test_cases_on_the_interpreter(name):
    cs, sim = dc.cases(name), dc.simulated(name)            # simulate() raises where a 64-bit column or a shift count leaves its range
    assert len(cs) % 64 != 0 and len(cs) > 64
    assert len({c.cls for c in cs[:8]}) >= 3                # neighbouring lanes hold different classes
    for c, words in zip(cs, sim):
        dc.check(c, words)


def _caught(name, lines):
    """does at least one case of the probe notice the mutated instruction list? Noticing means an assertion of the interpreter or a failed check of the
    stored registers' VALUES (dform_cases.check): registers that merely differ from the unmutated run do not count"""
    for c in dc.cases(name):
        try:
            dc.check(c, dc.simulate(c, lines))
        except (AssertionError, KeyError):
            return True
    return False


def _mutants(name):
    """one v_ashrrev_i64 as a logical shift, one v_and_b32 mask dropped, one quotient product removed -- each at two of the places where the body has such an
    instruction: a third and two thirds of the way through for the shifts and the products, two thirds and the end for the masks. (The LAST arithmetic shift
    of a pass feeds only the low word of the top digit, where both shifts agree; a mask in the first half of a scan is the mask of a Montgomery quotient digit,
    without which that digit merely grows by a multiple of 2^28 and the result stays a normalised representative of the same residue. Neither changes a checked
    property, so neither is a mutant these tests could be asked to catch.)"""
    lines = dc.LINES[name]
    sp0 = t.SP28(0)
    picks = {"ashr->lshr": [i for i, l in enumerate(lines) if l.startswith("v_ashrrev_i64")],
             "mask dropped": [i for i, l in enumerate(lines) if l.startswith("v_and_b32") and l.rstrip().endswith(t.SMASK28)],
             "quotient product removed": [i for i, l in enumerate(lines) if l.startswith("v_mad_i64_i32") and (", %s, " % sp0 in l or ", %s, " % t.NQ in l)]}
    for what, idx in picks.items():
        for i in sorted({idx[2 * len(idx) // 3], idx[-1]} if what == "mask dropped" else {idx[len(idx) // 3], idx[2 * len(idx) // 3]}) if idx else []:
            m = list(lines)
            if what == "ashr->lshr":
                m[i] = m[i].replace("v_ashrrev_i64", "v_lshrrev_b64")
            elif what == "mask dropped":
                dst, src = [x.strip() for x in m[i].split(None, 1)[1].split(",")[:2]]
                m[i] = "v_mov_b32_e64 %s, %s" % (dst, src)
            else:
                del m[i]
            yield "%s at line %d" % (what, i), m
    assert all(picks[w] for w in picks) or name in ("norm", "canon32"), (name, {w: len(v) for w, v in picks.items()})


@pytest.mark.parametrize("name", ["fp2_mul_d", "fp_mul1_d", "fp_redc7_d", "fp4_sqr0_d", "reduce", "pack32", "conv_reduce"])
def test_mutants_of_the_bodies_are_caught(name):
    n = 0
    for what, lines in _mutants(name):
        assert _caught(name, lines), (name, what, "survives every case")
        n += 1
    assert n == 6


def test_quotient_estimate_sites_are_inside_what_is_proved():
    """every site that emits seq_reduce / seq_pack_pass while the routines are generated: the result bound it goes on with contains (1/2 + eps) p for the input
    bound it records, eps derived in gen_tower_d.estimate_error; where it goes on with the fixed REDUCED / PACKED the input lies in the domain where
    eps p <= p / 1024; and every site of the generator's text is in the list"""
    sites = dc.recorded_sites()
    assert {s for s, _ in sites} >= {"do_reduce", "do_iszero", "do_storep", "do_sgn0", "miller_prologue", "f_out_epilogue", "csqr2_body", "pstart2_body",
                                     "psave2_body", "g1_aggregate_epilogue", "g2_dbl_prologue", "g2_dbl_epilogue", "g2_group_epilogue", "g2_blind_epilogue",
                                     "g1_blind_epilogue"}
    assert dc.PASSES_EMITTED[0] == len(dc.SITE_LIST) > 1000, "a place that emits a quotient-estimate pass records no input bound"
    for site, kind, B, res in dc.SITE_LIST:
        eps = t.estimate_error(B.vabs(), B.dlo, B.dhi, kind == "pack", max(abs(B.tlo), abs(B.thi)))
        need = -((-eps.numerator * P) // eps.denominator)                                   # ceil(eps p)
        centre = P if kind == "pack" else 0
        assert res.vlo <= centre - P // 2 - need and centre + P // 2 + need <= res.vhi, (site, B, res)
        fixed = t.PACKED if kind == "pack" else t.REDUCED
        if (res.vlo, res.vhi) == (fixed.vlo, fixed.vhi):
            assert need <= P >> 10, (site, "fixed bound outside its domain", B)
        assert res.dlo == 0 and res.dhi == (1 << 28) - 1


def test_estimate_error_terms():
    """the derived error against the figures it is made of: per p of input about pi / PTOP^2 ... (1.12e-6) for the neglected digits of p plus 3 * 2^-24 for the
    three f32 roundings; the fixed slack p / 1024 is proved up to about 740 p and not at 1024 p; REDUCED_ANY holds up to the largest top digit"""
    e = lambda k, **kw: float(t.estimate_error(k * P, **kw))
    per_p = (e(2000) - e(1000)) / 1000
    assert 1.25e-6 < per_p < 1.35e-6
    assert e(700) < 1 / 1024 < e(800)
    assert e(100) < 2e-4
    assert e(20163, tmag=(1 << 31) - 1) < 1 / 32
    assert e(100, pack=True) > e(100)
    assert t.reduced_bound(t.Bound.normalised(-700 * P, 700 * P)) is t.REDUCED
    wide = t.reduced_bound(t.Bound.normalised(-4000 * P, 4000 * P))
    assert wide.vhi > t.REDUCED.vhi and wide.vhi <= t.REDUCED_ANY.vhi
