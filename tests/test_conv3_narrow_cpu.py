"""The host-only part of the narrow Conv1d(k = 3) C ABI (csrc/pcgmix_conv3_narrow.hip): the width
predicate, the tile constants and the split plan, beside the unchanged predicates of the matrix kernels;
and the restatements (tests/conv3_ref.py, tests/conv3_wgrad_ref.py) against torch in float64 at the ten
narrow pairs.  The library is loaded with ctypes.CDLL alone: no device call is made."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import conv3_ref as R
import conv3_wgrad_ref as W

NAMES = ("pcgmix_conv3_narrow_supported", "pcgmix_conv3_narrow_tile", "pcgmix_conv3_narrow_nlc_f32",
         "pcgmix_conv3_narrow_wgrad_plan", "pcgmix_conv3_narrow_wgrad_nlc_f32")
PAIRS = [(2, 2), (2, 4), (2, 8), (2, 16), (4, 2), (8, 2), (16, 2), (4, 8), (8, 8), (16, 8)]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES + ("pcgmix_conv3_supported", "pcgmix_conv3_wgrad_supported", "pcgmix_abi_version"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def plan(lib, B, L, Cin, Cout):
    """(return code, splits, workspace bytes) of pcgmix_conv3_narrow_wgrad_plan."""
    s, n = ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = lib.pcgmix_conv3_narrow_wgrad_plan(B, L, Cin, Cout, ctypes.byref(s), ctypes.byref(n))
    return int(rc), int(s.value), int(n.value)


def test_the_five_entry_points_are_bound_and_exported(lib):
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["pcgmix_conv3_narrow_nlc_f32"] == _lib.SIGNATURES["pcgmix_conv3_nlc_f32"]
    assert _lib.SIGNATURES["pcgmix_conv3_narrow_wgrad_plan"] == _lib.SIGNATURES["pcgmix_conv3_wgrad_plan"]
    assert _lib.SIGNATURES["pcgmix_conv3_narrow_wgrad_nlc_f32"] == _lib.SIGNATURES["pcgmix_conv3_wgrad_nlc_f32"]


def test_predicate_is_the_ten_pairs_and_disjoint_from_the_matrix_kernel_s(lib):
    assert len(set(PAIRS)) == 10
    for cin in range(1, 65):
        for cout in range(1, 65):
            narrow = lib.pcgmix_conv3_narrow_supported(cin, cout)
            assert narrow == int((cin, cout) in PAIRS), (cin, cout)
            assert not (narrow and lib.pcgmix_conv3_supported(cin, cout)), (cin, cout)
            assert not (narrow and lib.pcgmix_conv3_wgrad_supported(cin, cout)), (cin, cout)
    for c in (0, -2, -8, 32, 1028):
        for other in (2, 8):
            assert lib.pcgmix_conv3_narrow_supported(c, other) == 0, (c, other)
            assert lib.pcgmix_conv3_narrow_supported(other, c) == 0, (other, c)


def test_the_matrix_kernels_predicates_are_unchanged(lib):
    for fn in (lib.pcgmix_conv3_supported, lib.pcgmix_conv3_wgrad_supported):
        for cin, cout in [(1, 64), (4, 8), (6, 16), (1028, 16), (0, 16), (-4, 16), (16, 0), (16, -16), (16, 2),
                          (3, 4), (16, 1040)] + PAIRS:
            assert fn(cin, cout) == 0, (cin, cout)
        for cin, cout in [(4, 4), (4, 16), (8, 4), (8, 16), (16, 16), (16, 32), (64, 4), (1024, 1024)]:
            assert fn(cin, cout) == 1, (cin, cout)


def test_abi_version_is_unchanged(lib):
    assert lib.pcgmix_abi_version() == 25 == _lib.ABI_VERSION


def test_tile_constants(lib):
    assert lib.pcgmix_conv3_narrow_tile(0) > 0 and lib.pcgmix_conv3_narrow_tile(1) > 0
    for which in (2, 3, -1, 100):
        assert lib.pcgmix_conv3_narrow_tile(which) == 0


def test_plan_properties(lib):
    TK = lib.pcgmix_conv3_narrow_tile(1)
    for B in (1, 2, 3, 5, 8, 256):
        for L in (1, 2, TK - 1, TK, TK + 1, 2 * TK + 3, 312, 625, 1250, 2500):
            for cin, cout in PAIRS:
                rc, s, n = plan(lib, B, L, cin, cout)
                assert rc == 0
                assert 1 <= s <= B * -(-L // TK), (B, L, cin, cout, s)
                assert n == (s * cout * 3 * cin * 4 if s > 1 else 0)
                assert plan(lib, B, L, cin, cout) == (rc, s, n)            # the same answer twice
    assert plan(lib, 0, 9, 8, 8) == (0, 1, 0)                              # an empty batch still plans
    # one block for the whole sum is no plan at the paper's batch, and some B <= 256 splits three K tiles
    assert all(plan(lib, 256, 2500, cin, cout)[1] > 1 for cin, cout in PAIRS)
    assert any(plan(lib, B, 2 * TK + 3, 8, 8)[1] >= 2 for B in range(1, 257))
    for cin, cout in [(4, 4), (4, 16), (16, 16), (1, 2), (2, 3), (2, 32), (32, 8), (0, 8), (8, -8), (1028, 2)]:
        assert plan(lib, 2, 9, cin, cout)[0] != 0, (cin, cout)
    assert plan(lib, -1, 9, 8, 8)[0] != 0 and plan(lib, 2, 0, 8, 8)[0] != 0 and plan(lib, 2, -5, 8, 8)[0] != 0
    # either output pointer may be left out
    assert lib.pcgmix_conv3_narrow_wgrad_plan(2, 9, 8, 8, None, None) == 0


@pytest.mark.parametrize("Cin,Cout", PAIRS)
def test_restatements_match_torch_at_the_narrow_widths(Cin, Cout):
    B, L = 2, 7
    rs = np.random.RandomState(0)
    x, w = rs.standard_normal((B, L, Cin)), rs.standard_normal((Cout, 3, Cin))
    dy = rs.standard_normal((B, L, Cout))
    xt = torch.from_numpy(x).permute(0, 2, 1).requires_grad_(True)
    wt = torch.from_numpy(w).permute(0, 2, 1).requires_grad_(True)          # Conv1d's (O, I, 3)
    y = F.conv1d(xt, wt, padding=1)
    dx, dw = torch.autograd.grad(y, (xt, wt), torch.from_numpy(dy).permute(0, 2, 1))
    got, mag = R.conv3_f64(x, w)
    assert np.abs(got - y.detach().permute(0, 2, 1).numpy()).max() <= 1e-12 * max(1.0, mag.max())
    got, mag = R.conv3_f64(dy, R.flip_transpose(w))
    assert got.shape == (B, L, Cin)
    assert np.abs(got - dx.permute(0, 2, 1).numpy()).max() <= 1e-12 * max(1.0, mag.max())
    got, mag = W.wgrad_f64(x, dy)
    assert got.shape == (Cout, 3, Cin)
    assert (np.abs(got - dw.permute(0, 2, 1).numpy()) <= 1e-12 * mag).all()
