"""The message phase after hash_to_field on the GPU, at the field elements no hashed message reaches (tests/map_cases.py): the exceptional denominator of the
simplified SWU map, sgn0 with a zero real part, q0 = q1 (the doubling fix-up under a partial exec mask) and q0 = -q1 (the cofactor clearing on infinity) --
through mbls_map_to_g2_probe in all four hand-scheduled forms and the compiled body. Every comparison is bit-exact on the 96 compressed bytes against the
Python model's point from the case list; no GPU form is ever the reference of another. Last: hash_to_field at SHA-256's own block boundaries."""
import random

import pytest

import helpers
import map_cases as mc
import orc

pytestmark = pytest.mark.gpu

NEVER = 1 << 62
# name -> (probe mode, message-phase packing limit or None): hashg2 takes a wave per item, hashg2x4 four items per wave above the limit
FORMS = {"body": (0, None), "lane": (1, None), "wave": (2, NEVER), "wave_x4": (2, 0), "pair": (3, None)}


@pytest.fixture(scope="module")
def mb():
    from milagro_bls_amd import batch, _native
    _native.default_context()
    return batch


@pytest.fixture(scope="module")
def ctx():
    from milagro_bls_amd import _native
    return _native.default_context()


def run_form(mb, ctx, form, items):
    """the probe on a list of cases in one named form; the 96-byte outputs, one per item"""
    mode, pack = FORMS[form]
    buf = b"".join(c.packed for c in items)
    try:
        if pack is not None:
            ctx.set_coop_packing(NEVER, NEVER, pack)
        out = mb.map_to_g2_batch(buf, len(items), mode=mode)
    finally:
        ctx.reset_tuning()
    return [out[96 * i:96 * i + 96] for i in range(len(items))]


def check(got, items, what):
    bad = [(i, c.name) for i, (g, c) in enumerate(zip(got, items)) if g != c.expected]
    assert not bad, "%s: %d of %d items differ from the model, first (index, case): %r" % (what, len(bad), len(items), bad[:8])


def layout(n, at, special):
    """n items: case `special` at the indices in `at`, the plain cases (in turn) everywhere else"""
    plain, sp = mc.plain(), mc.by_name()[special]
    return [sp if i in at else plain[i % len(plain)] for i in range(n)]


def test_every_case_in_every_form(mb, ctx):
    """the whole list through the compiled body, the one-lane routine, hashg2, hashg2x4 and the lane-pair routine; each form against the model, and -- for
    the message's sake only -- which forms agree with each other where one is wrong"""
    items = list(mc.cases())
    assert len(items) <= 48
    got = {form: run_form(mb, ctx, form, items) for form in FORMS}
    wrong = {c.name: sorted(f for f in FORMS if got[f][i] != c.expected) for i, c in enumerate(items)}
    wrong = {k: v for k, v in wrong.items() if v}
    agree = {name: len({got[f][i] for f in FORMS}) == 1 for i, name in enumerate(c.name for c in items)}
    assert not wrong, "forms that differ from the model, per case: %r; all five forms equal there: %r" % (wrong, {k: agree[k] for k in wrong})
    assert all(agree.values())


def lane_sets(n):
    sets = {"none": set(), "all": set(range(n)), "first": {0}, "last_of_wave": {63}, "middle": {31, 32}, "odd": set(range(1, n, 2))}
    if n > 129:
        sets["last_live"] = {129}
    return sets


LANE_LAYOUTS = [(n, name, "same") for n in (64, 130) for name in lane_sets(n)] + \
               [(n, name, sp) for n in (64, 130) for sp in ("neg", "zero_both") for name in ("first", "last_of_wave", "all")]


@pytest.mark.parametrize("n,where,special", LANE_LAYOUTS, ids=["%d-%s-%s" % x for x in LANE_LAYOUTS])
def test_fixup_lane_layouts_one_lane_routine(mb, ctx, n, where, special):
    """k_hash's routine on one full wave and on three waves whose last holds two live lanes: the doubling fix-up taken by no lane (the wave-level branch
    round it), by every lane, and by single lanes at the edges of the wave under a partial exec mask; the same layouts with q0 = -q1 and with u = 0"""
    items = layout(n, lane_sets(n)[where], special)
    check(run_form(mb, ctx, "lane", items), items, "%s at %s of %d lanes" % (special, where, n))


def pair_sets(n):
    sets = {"first": {0}, "m31": {31}, "all": set(range(n)), "alternating": set(range(0, n, 2))}
    if n > 64:
        sets["m64"] = {64}
    return sets


PAIR_LAYOUTS = [(n, name, sp) for n in (32, 65) for sp in ("same", "neg", "zero_both", "zero_first", "zero_second", "twin_same") for name in pair_sets(n)]


@pytest.mark.parametrize("n,where,special", PAIR_LAYOUTS, ids=["%d-%s-%s" % x for x in PAIR_LAYOUTS])
def test_degenerate_messages_lane_pair_routine(mb, ctx, n, where, special):
    """k_hash2's routine, two lanes per message (one wave; three waves, the last with one live pair): degenerate messages at the edges, everywhere, and at
    every other message so that a pair's neighbour pair differs. zero_first / zero_second: only the even / only the odd lane meets the exceptional denominator"""
    items = layout(n, pair_sets(n)[where], special)
    check(run_form(mb, ctx, "pair", items), items, "%s at messages %s of %d" % (special, where, n))


@pytest.mark.parametrize("n", [32, 65])
@pytest.mark.parametrize("order", [("zero_first", "zero_second"), ("zero_second", "zero_first")], ids=["first-second", "second-first"])
def test_exceptional_denominator_in_either_lane_of_a_pair(mb, ctx, n, order):
    """zero_first and zero_second side by side, in both orders: neighbouring pairs meet u = 0 in opposite lanes"""
    by = mc.by_name()
    items = [by[order[i & 1]] for i in range(n)]
    check(run_form(mb, ctx, "pair", items), items, "%s / %s alternating over %d messages" % (order + (n,)))


def wave_layouts():
    out = []
    for form, sizes, places in (("wave_x4", (1, 3, 4, 5, 9), (("item0", {0}), ("item3", {3}), ("all4", {0, 1, 2, 3}))), ("wave", (1, 3), (("first", {0}), ("all", {0, 1, 2, 3})))):
        for n in sizes:
            for name, pos in places:
                at = frozenset(i for i in range(n) if i % 4 in pos)          # the place within a wave of four items
                if not at or (n == 1 and name in ("all4", "all")):          # (at n = 1 that is item0 / first again)
                    continue
                for sp in ("same", "neg", "zero_both", "zero_second"):
                    out.append((form, n, name, at, sp))
    return out


WAVE_LAYOUTS = wave_layouts()


@pytest.mark.parametrize("form,n,where,at,special", WAVE_LAYOUTS, ids=["%s-%d-%s-%s" % (f, n, w, s) for f, n, w, _, s in WAVE_LAYOUTS])
def test_degenerate_items_wave_programs(mb, ctx, form, n, where, at, special):
    """hashg2x4 (four items per wave, batch sizes that leave the last wave partly empty) with degenerate items in the first and the last place of a wave and in
    all four; hashg2 (a wave per item) at n = 1 and 3"""
    items = layout(n, at, special)
    check(run_form(mb, ctx, form, items), items, "%s: %s at %s of %d items" % (form, special, where, n))


@pytest.mark.parametrize("form", ["lane", "wave", "wave_x4", "pair"])
def test_nothing_leaks_into_the_next_call(mb, ctx, form):
    """after a call whose every lane ended at infinity, 64 ordinary messages hash as the oracle says in the same context and form: exec and status registers
    are the wave's own, but the workspace slots a call leaves at infinity are the next call's to overwrite"""
    items = layout(64, set(range(64)), "neg")
    check(run_form(mb, ctx, form, items), items, "all lanes neg")
    msgs = random.Random(51).randbytes(32 * 64)
    mode, pack = FORMS[form]
    try:
        if pack is not None:
            ctx.set_coop_packing(NEVER, NEVER, pack)
        got = mb.hash_to_g2_batch(msgs, 64, mode=mode)
    finally:
        ctx.reset_tuning()
    assert got == orc.batch_hash_to_g2(msgs, 64)


def hash_lengths(mb, ctx, form, lengths):
    mode, pack = FORMS[form]
    rnd = random.Random(52)
    bad = []
    try:
        if pack is not None:
            ctx.set_coop_packing(NEVER, NEVER, pack)
        for ln in lengths:
            msgs = rnd.randbytes(2 * ln)
            if mb.hash_to_g2_batch(msgs, 2, msg_len=ln, mode=mode) != orc.batch_hash_to_g2(msgs, 2, msg_len=ln):
                bad.append(ln)
    finally:
        ctx.reset_tuning()
    assert not bad, "message lengths whose H differs from the oracle's (%s): %r" % (form, bad)


def test_every_message_length_up_to_200(mb, ctx):
    """b_0 of expand_message_xmd hashes 64 + len + 3 + 44 bytes, so SHA-256's padding changes shape at len mod 64 = 8 / 9 (the length field just fits / no
    longer fits the last block) and 16 / 17 (the data ends one byte before / exactly at a block boundary): every length 0 .. 200 through the one-lane form, two messages a call"""
    hash_lengths(mb, ctx, "lane", range(201))


@pytest.mark.parametrize("form", ["wave", "wave_x4", "pair"])
def test_padding_boundary_lengths_other_forms(mb, ctx, form):
    hash_lengths(mb, ctx, form, (0, 8, 9, 16, 17, 72, 73, 80, 81))
