"""pcgmix_partner_permutation_i64 — the library's restatement of ``random.Random(seed).sample`` per label
group (augmentations.py:500-514) — against CPython's own sampler, bit for bit.  The library tempers the
first 624 output words of the seeded generator once and lets every group read them from the start; a
group that needs more goes on with an ordinary generator.  The sizes here sit on both sides of that
block (a group of ~430 uses it up in expectation; 1000 and 5000 cross it more than once), and every
case compares whole permutations, so a block read one word off cannot pass."""
import ctypes
import random

import numpy as np
import pytest

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, hostprep

SEEDS = [0, 1, 2**32 - 1, 2**32, 2**40 + 3]
SIZES = [1, 2, 3, 127, 128, 129, 255, 256] + list(range(400, 481, 10)) + [624, 1000, 5000]


def library(gid, n_groups, seed):
    gid = np.ascontiguousarray(gid, dtype=np.int32)
    mix = np.full(gid.shape[0], -1, dtype=np.int64)
    err = _lib.load().pcgmix_partner_permutation_i64(gid.ctypes.data, gid.shape[0], n_groups,
                                                     ctypes.c_uint64(seed), mix.ctypes.data)
    assert err == 0
    return mix


def cpython(gid, n_groups, seed):
    mix = np.full(len(gid), -1, dtype=np.int64)
    for g in range(n_groups):
        members = [int(b) for b in np.flatnonzero(np.asarray(gid) == g)]
        mix[members] = random.Random(seed).sample(members, len(members))
    return mix


@pytest.mark.parametrize("n", SIZES)
def test_one_group_of_every_size(n):
    gid = np.zeros(n, dtype=np.int32)
    for seed in SEEDS:
        assert np.array_equal(library(gid, 1, seed), cpython(gid, 1, seed)), (n, seed)


@pytest.mark.parametrize("n_groups", [1, 2, 7, 256])
def test_groups_of_unequal_size(n_groups):
    rs = np.random.RandomState(n_groups)
    for B in (n_groups, 256, 1300, 6000):
        if B < n_groups:
            continue
        weights = rs.dirichlet(np.full(n_groups, 0.6))
        gid = rs.choice(n_groups, size=B, p=weights).astype(np.int32)
        gid[:n_groups] = rs.permutation(n_groups)          # every group has a member
        for seed in SEEDS:
            assert np.array_equal(library(gid, n_groups, seed), cpython(gid, n_groups, seed)), (B, seed)


def test_two_thousand_consecutive_steps():
    rs = np.random.RandomState(5)
    gid = rs.randint(0, 2, 256).astype(np.int32)
    big = np.zeros(700, dtype=np.int32)
    for step in range(2000):
        assert np.array_equal(library(gid, 2, step), cpython(gid, 2, step)), step
        if step % 50 == 0:
            assert np.array_equal(library(big, 1, step), cpython(big, 1, step)), step


def test_shuffle_within_groups_keeps_its_result():
    rs = np.random.RandomState(9)
    for B, K in ((256, 2), (256, 17), (1000, 3), (31, 31)):
        keys = rs.randint(0, K, B).astype(np.int64)
        for step in (0, 5, 2**32 + 1):
            want = np.arange(B)
            groups = {}
            for i, k in enumerate(keys):
                groups.setdefault(int(k), []).append(i)
            for idx in groups.values():
                want[idx] = random.Random(step).sample(idx, len(idx))
            assert np.array_equal(hostprep.shuffle_within_groups(keys, step), want)
