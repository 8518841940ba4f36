"""The big Potes conv stacks (layers [64,32] and [128,64], csrc/pcgmix_potes_big.hip): what can be
checked without a device — the ABI's names, the host-only helpers and their zero-for-refused rules,
the dispatch table of ``models._stack_calls``, and that the generalised float64 reference
(tests/potes_big_ref.py) is tests/potes_ref.py at (8,4)."""
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, models

import potes_big_ref as RB
import potes_ref as R

NEW = ["pcgmix_potes_big_supported", "pcgmix_potes_big_grad_len", "pcgmix_potes_big_bwd_blocks",
       "pcgmix_potes_big_mask_bytes", "pcgmix_potes_big_fwd_f32", "pcgmix_potes_big_bwd_mask_f32",
       "pcgmix_potes_big_input_grad_mask_f32"]
OTHER = [(8, 4), (2, 1), (32, 64), (64, 64)]
MAX_N = 65535


def test_entry_points_are_declared_and_exported():
    lib = _lib.load()
    for n in NEW:
        assert n in _lib.SIGNATURES
        assert hasattr(lib, n)


def test_supported_and_grad_len():
    lib = _lib.load()
    assert [lib.pcgmix_potes_big_supported(*w) for w in RB.WIDTHS] == [1, 1]
    assert [lib.pcgmix_potes_big_supported(*w) for w in OTHER] == [0, 0, 0, 0]
    assert [lib.pcgmix_potes_big_grad_len(*w) for w in RB.WIDTHS] == [10656, 41792]
    assert [RB.grad_len(*w) for w in RB.WIDTHS] == [10656, 41792]
    assert [lib.pcgmix_potes_big_grad_len(*w) for w in OTHER] == [0, 0, 0, 0]
    # the narrow family keeps its own table
    assert [lib.pcgmix_potes_narrow_supported(*w) for w in RB.WIDTHS] == [0, 0]


@pytest.mark.parametrize("widths", RB.WIDTHS, ids=str)
@pytest.mark.parametrize("N,T", [(1, 14), (3, 23), (2, 258), (5, 527), (4, 2500)])
def test_mask_bytes_match_the_packings(widths, N, T):
    C1, C2 = widths
    lib = _lib.load()
    P1, P2 = R.dims(T)
    assert lib.pcgmix_potes_big_mask_bytes(N, T, C1, C2, 2) == R.pack_m2(torch.zeros(N, C2, P2, dtype=torch.uint8), P2).numel()
    assert lib.pcgmix_potes_big_mask_bytes(N, T, C1, C2, 1) == R.pack_s1(torch.zeros(N, C1, P1, dtype=torch.uint8), P1).numel()
    assert lib.pcgmix_potes_big_mask_bytes(N, T, C1, C2, 0) == 0
    assert lib.pcgmix_potes_big_mask_bytes(N, T, C1, C2, 3) == 0
    G = lib.pcgmix_potes_big_bwd_blocks(N, T, C1, C2)
    assert 1 <= G <= N * ((P2 + 63) // 64)


def test_helpers_answer_zero_for_what_the_launchers_refuse():
    lib = _lib.load()
    for C1, C2 in RB.WIDTHS:
        for N, T in ((4, 13), (0, 64), (-1, 64), (MAX_N + 1, 64)):
            assert lib.pcgmix_potes_big_bwd_blocks(N, T, C1, C2) == 0, (N, T)
            assert lib.pcgmix_potes_big_mask_bytes(N, T, C1, C2, 1) == 0, (N, T)
            assert lib.pcgmix_potes_big_mask_bytes(N, T, C1, C2, 2) == 0, (N, T)
        assert lib.pcgmix_potes_big_bwd_blocks(MAX_N, 14, C1, C2) > 0
    for C1, C2 in OTHER:
        assert lib.pcgmix_potes_big_bwd_blocks(4, 64, C1, C2) == 0
        assert lib.pcgmix_potes_big_mask_bytes(4, 64, C1, C2, 2) == 0


def test_block_cap_is_read_from_the_environment(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("PCGMIX_POTES_BIG_BWD_BLOCKS", raising=False)
    for C1, C2 in RB.WIDTHS:
        work = 1024 * ((R.dims(2500)[1] + 63) // 64)
        assert 1 <= lib.pcgmix_potes_big_bwd_blocks(1024, 2500, C1, C2) <= work
    monkeypatch.setenv("PCGMIX_POTES_BIG_BWD_BLOCKS", "2")
    assert lib.pcgmix_potes_big_bwd_blocks(5, 526, 64, 32) == 2
    assert lib.pcgmix_potes_big_bwd_blocks(1, 14, 64, 32) == 1          # never more blocks than items
    monkeypatch.setenv("PCGMIX_POTES_BIG_BWD_BLOCKS", "0")              # out of range: ignored
    assert lib.pcgmix_potes_big_bwd_blocks(5, 526, 64, 32) >= 1


def test_stack_calls_map_the_widths():
    lib = _lib.load()
    for C1, C2 in RB.WIDTHS:
        calls = models._stack_calls(lib, C1, C2)
        assert calls.fwd is None and calls.bwd is None and calls.input_grad is None
        assert calls.fwd_save == "pcgmix_potes_big_fwd_f32"
        assert calls.mask_bytes == "pcgmix_potes_big_mask_bytes"
        assert calls.bwd_blocks == "pcgmix_potes_big_bwd_blocks"
        assert calls.bwd_mask == "pcgmix_potes_big_bwd_mask_f32"
        assert calls.input_grad_mask == "pcgmix_potes_big_input_grad_mask_f32"
        assert calls.tail == (C1, C2) and calls.grad_len == RB.grad_len(C1, C2) and calls.defer is False
    assert models._stack_calls(lib, 8, 4).fwd_save == "pcgmix_potes_stack_fwd_save_f32"
    assert models._stack_calls(lib, 2, 1).fwd_save == "pcgmix_potes_narrow_fwd_f32"


@pytest.mark.parametrize("N,T", [(3, 23), (2, 526)])
def test_reference_at_8_4_is_potes_ref(N, T):
    c = R.rand_case(N, T)
    mine = RB.stack_ref(c.x, c.w1, c.b1, c.w2, c.b2, c.r)
    for name in ("h2", "gx", "grads", "code1", "code2"):
        assert torch.equal(getattr(mine, name), getattr(c.ref, name)), name
    # given its own codes back, the reference reproduces itself
    again = RB.stack_ref(c.x, c.w1, c.b1, c.w2, c.b2, c.r, codes=(mine.code1, mine.code2))
    for name in ("h2", "gx", "grads"):
        assert torch.equal(getattr(again, name), getattr(mine, name)), name
    und = RB.undecidable(c.x, c.w1, c.b1, c.w2, c.b2)
    assert int(und.frag1.sum()) + int(und.frag2.sum()) == R.undecidable(c.x, c.w1, c.b1, c.w2, c.b2)
    # the allowed set always holds the float64 decision
    assert bool(torch.gather(und.allowed2, -1, mine.code2.long()[..., None]).all())


@pytest.mark.parametrize("widths", RB.WIDTHS, ids=str)
def test_int_case_is_exact_and_has_ties(widths):
    sparse = RB.int_case(widths, 3, 258, 1 / 32)
    dense = RB.int_case(widths, 3, 258, 1.0)
    assert min(sparse.ties) >= 0.01
    assert sparse.ref.grads.numel() == dense.ref.grads.numel() == RB.grad_len(*widths)
    for c in (sparse, dense):
        assert torch.equal(c.ref.h2, c.ref.h2.round()) and torch.equal(c.ref.grads, c.ref.grads.round())
