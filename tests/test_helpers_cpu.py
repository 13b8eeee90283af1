"""The sampling helper the full-scale GPU tests pick their oracle items with (tests/helpers.py): deterministic per seed, in range, and holding every
boundary the batch engines cut at and every rejection class of bench.build_inputs."""
import os

import numpy as np
import pytest
import torch

import helpers


@pytest.mark.parametrize("n", [1 << 13, 1 << 16, 1 << 17, 200_000])
def test_sample_indices_holds_every_boundary_and_class(n):
    s = helpers.sample_indices(n, seed=5)
    assert s == helpers.sample_indices(n, seed=5)
    assert s != helpers.sample_indices(n, seed=6)
    assert s == sorted(set(s)) and 0 <= s[0] and s[-1] < n
    assert len(s) >= 1024
    have = set(s)
    assert {0, 63, 64} <= have
    assert set(range(n - 64, n)) <= have
    for q in range(1, n // 65536 + 1):
        assert {q * 65536 - 1, q * 65536, q * 65536 + 1} & set(range(n)) <= have, q
    classes = [helpers.rejection_class(i) for i in s]
    for c in range(5):
        assert classes.count(c) >= 8, c
    # the uniform part reaches the whole range, not only the boundaries
    assert all(len([i for i in s if q * n // 8 <= i < (q + 1) * n // 8]) >= 64 for q in range(8))


def test_sample_indices_count_and_small_ranges():
    s = helpers.sample_indices(1 << 13, seed=1, count=512)
    assert 512 <= len(s) < 1024
    assert helpers.sample_indices(100, seed=1) == list(range(100))
    assert helpers.sample_indices(65537, seed=3).count(65536) == 1


def test_rejection_class_matches_build_inputs_layout():
    # bench.build_inputs: bad = arange(7, n, 16), kinds = arange(len(bad)) % 5
    bad = np.arange(7, 4096, 16)
    assert [helpers.rejection_class(int(i)) for i in bad] == (np.arange(len(bad)) % 5).tolist()
    assert all(helpers.rejection_class(i) is None for i in range(4096) if i % 16 != 7)


def test_bitmap_bits_unpacks_low_bit_first():
    n = 200
    bits = np.random.default_rng(1).integers(0, 2, n).astype(np.uint8)
    words = np.zeros((n + 63) // 64, dtype=np.uint64)
    for i in np.flatnonzero(bits):
        words[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    assert np.array_equal(helpers.bitmap_bits(torch.from_numpy(words.view(np.int64)), n), bits)


def test_oracle_threads_is_capped(monkeypatch):
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert 1 <= helpers.oracle_threads() <= min(16, os.cpu_count() or 1)
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert helpers.oracle_threads() == min(3, os.cpu_count() or 1)
    monkeypatch.setenv("OMP_NUM_THREADS", "")
    assert helpers.oracle_threads() <= 16
