"""Seeded slices of the stress runs (tests/stress_cases.py; scripts/stress_*.py run the same cases over many seeds): every engine at its crossovers,
verify_multiple through all its entries, shards and two contexts, and batches above a round on two tracks -- against the oracle item by item.
Each slice sets its own engine settings and restores the library's defaults (the `engine` fixture would run it three times over)."""
import pytest

import helpers
import stress_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from milagro_bls_amd import _native as N
    c = N.default_context()
    yield c
    c.reset_tuning()


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda:0")


@pytest.mark.parametrize("seed", [100, 101, 102])
def test_engines_at_their_crossovers_vs_oracle(ctx, seed):
    # stress_parity's shapes (seed 100 adds 8 193 x 2 and 2 049 x 9, above the cooperative engine's default range) under the default routing, lane pairs,
    # the two-pair loop and the cooperative engine forced to any size; then signing and sk -> pk at 257 .. 320 items
    nt = helpers.oracle_threads()
    items, bad = sc.run_fav_engines(ctx, seed, nt)
    assert not bad, bad[:4]
    assert items == 4 * sum(n for n, _, _ in sc.parity_shapes(seed))
    if seed == 100:
        assert set(sc.BIG_SHAPES) <= set(sc.parity_shapes(seed))
    items, bad = sc.run_sign_keys(ctx, seed, nt)
    assert not bad, bad


@pytest.mark.parametrize("seed", [100, 101])
def test_verify_multiple_shards_two_contexts_and_aggregate_verify_vs_oracle(ctx, dev, seed):
    from milagro_bls_amd import _native as N
    m2 = N.MultiContext([0, 0])
    try:
        _, bad = sc.run_vm_shards(ctx, m2, dev, seed, helpers.oracle_threads())
    finally:
        m2.close()
    assert not bad, bad


def test_verify_multiple_three_entries_and_scalar_draws_vs_oracle(ctx, dev):
    # 80 random batches of 1 .. 299 sets with random spoils: the entry taking the scalars, the one with the caller's scalar source (verdict and the
    # draws it asks for) and the device entry
    (batches, sets), bad = sc.run_vm(ctx, dev, 80, seed=21)
    assert not bad, bad[:4]
    assert batches == 80 and sets > 80


def test_two_tracks_above_a_round_vs_construction_and_oracle(dev):
    # 40 random sizes in (65 536, 3 x 65 536 + 5 000]: random track limits, byte keys or table indices, with or without bitmap and status; every result,
    # bitmap bit and status class by construction, the round seams and the tail against the oracle. A context of its own: its workspace for
    # 201 608 items goes with it.
    from milagro_bls_amd import _native as N
    c = N.Context(0)
    inp = None
    try:
        inp = sc.TrackInputs(c, dev)
        (sizes, items), bad = sc.run_tracks(c, dev, inp, 40, seed=9, oracle_count=32)
    finally:
        if inp is not None:
            inp.table.close()
        c.close()
    assert not bad, bad[:4]
    assert sizes == 40 and items > 40 * 65536
