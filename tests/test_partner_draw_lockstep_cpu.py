"""The lock-step partner draw (pcgmix_partner_permutation_i64): up to four label groups advance together
through the seeded generator's first 624 tempered words, further groups in further rounds, a group that
uses the block up goes on alone with an ordinary generator, and the pool holds sample indices as int16
up to B = 32767 and as int32 beyond.  Every case compares whole permutations with CPython's own
``random.Random(seed).sample(members, len(members))`` per group, exactly: a group that read another
group's word, a round that did not restart at word 0 or a narrowed index cannot pass."""
import ctypes
import random

import numpy as np
import pytest

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

SEEDS = [1, 2, 2**32 - 1, 2**32, 2**40 + 7]
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257]


def library(gid, n_groups, seed):
    gid = np.ascontiguousarray(gid, dtype=np.int32)
    mix = np.full(gid.shape[0], -1, dtype=np.int64)
    err = _lib.load().pcgmix_partner_permutation_i64(gid.ctypes.data, gid.shape[0], n_groups,
                                                     ctypes.c_uint64(seed), mix.ctypes.data)
    return err, mix


def cpython(gid, n_groups, seed):
    gid = np.asarray(gid)
    mix = np.full(len(gid), -1, dtype=np.int64)
    for g in range(n_groups):
        members = np.flatnonzero(gid == g).tolist()
        mix[members] = random.Random(seed).sample(members, len(members))
    return mix


def scrambled(B, K):
    """K groups (as many as B allows) of unequal size whose ids first appear in a scrambled order."""
    rs = np.random.RandomState(100 * K + B)
    K = min(K, B)
    gid = rs.choice(K, size=B, p=rs.dirichlet(np.full(K, 0.7)))
    gid[rs.permutation(B)[:K]] = rs.permutation(K)            # every group has a member
    return gid.astype(np.int32), K


def layouts(B):
    yield "one class", np.zeros(B, dtype=np.int32), 1
    yield "alternating", (np.arange(B) % 2).astype(np.int32), min(B, 2)
    if B >= 2:
        single = np.zeros(B, dtype=np.int32)
        single[B // 2] = 1
        yield "one singleton", single, 2
    for K in (3, 4, 5, 6):
        if B >= K:
            yield ("%d scrambled" % K,) + scrambled(B, K)


@pytest.mark.parametrize("B", SIZES)
def test_every_layout_at_every_batch_edge(B):
    for name, gid, n_groups in layouts(B):
        for seed in SEEDS:
            err, mix = library(gid, n_groups, seed)
            assert err == 0
            assert np.array_equal(mix, cpython(gid, n_groups, seed)), (B, name, seed)


def test_a_group_beyond_the_block_beside_small_ones():
    # 900 members need about 1,300 words: the block's 624 in lock step with three small groups, the rest alone
    rs = np.random.RandomState(7)
    gid = np.zeros(1024, dtype=np.int32)
    gid[rs.permutation(1024)[:124]] = rs.randint(1, 4, 124)
    assert int((gid == 0).sum()) == 900 and set(gid.tolist()) == {0, 1, 2, 3}
    for seed in SEEDS:
        err, mix = library(gid, 4, seed)
        assert err == 0
        assert np.array_equal(mix, cpython(gid, 4, seed)), seed


def test_two_groups_with_the_wide_pool():
    rs = np.random.RandomState(11)
    gid = (rs.rand(40000) < 0.3).astype(np.int32)
    for seed in SEEDS:
        err, mix = library(gid, 2, seed)
        assert err == 0
        assert np.array_equal(mix, cpython(gid, 2, seed)), seed


def test_empty_groups_between_the_lanes():
    gid = np.array([5, 0, 5, 9, 0, 9, 9, 2], dtype=np.int32)      # ids 1, 3, 4, 6, 7, 8 have no member
    for seed in SEEDS:
        err, mix = library(gid, 10, seed)
        assert err == 0
        assert np.array_equal(mix, cpython(gid, 10, seed)), seed


@pytest.mark.parametrize("bad", [-1, 2, 2**31 - 1])
def test_group_id_out_of_range_is_refused(bad):
    gid = np.array([0, 1, bad, 0], dtype=np.int32)
    err, mix = library(gid, 2, 1)
    assert err == 1                                              # hipErrorInvalidValue
    assert (mix == -1).all()                                     # nothing was written
