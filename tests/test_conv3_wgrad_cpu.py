"""The restatement of the k = 3 convolution's weight gradient (tests/conv3_wgrad_ref.py) against torch's
float64 autograd, and the host-only part of its C ABI (csrc/pcgmix_conv3_wgrad.hip): the width
predicate, the tile constants and the split plan.  The library is loaded with ctypes.CDLL alone: no
device call is made."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import conv3_wgrad_ref as W

SHAPES = [(1, 1, 4, 16), (2, 2, 4, 4), (3, 5, 8, 16), (2, 37, 12, 48), (2, 130, 20, 32)]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pcgmix_conv3_supported", "pcgmix_conv3_wgrad_supported", "pcgmix_conv3_wgrad_tile",
                 "pcgmix_conv3_wgrad_plan", "pcgmix_conv3_wgrad_nlc_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


@pytest.mark.parametrize("B,L,Cin,Cout", SHAPES)
def test_restatement_matches_torch_autograd(B, L, Cin, Cout):
    rs = np.random.RandomState(0)
    x, dy = rs.standard_normal((B, L, Cin)), rs.standard_normal((B, L, Cout))
    w = torch.zeros(Cout, Cin, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(torch.from_numpy(x).permute(0, 2, 1), w, padding=1)
    (want,) = torch.autograd.grad(y, w, torch.from_numpy(dy).permute(0, 2, 1))
    want = want.permute(0, 2, 1).numpy()                    # Conv1d's (O, I, 3) -> [o][tap][i]
    got, mag = W.wgrad_f64(x, dy)
    assert got.shape == mag.shape == (Cout, 3, Cin)
    assert (np.abs(got - want) <= 1e-12 * mag).all()
    assert (mag >= np.abs(got) - 1e-12 * mag).all()
    xi, dyi = W.int_case(B, L, Cin, Cout)
    dwi = W.wgrad_int(xi, dyi)
    assert dwi.dtype == np.int64 and dwi.shape == (Cout, 3, Cin)
    assert np.array_equal(dwi, W.wgrad_f64(xi, dyi)[0])     # integers: float64 is exact as well
    assert np.abs(dwi).max() <= 8 * B * L < 2 ** 24


def test_predicate_equals_the_forward_kernel_s(lib):
    for cin in range(1, 1025):
        for cout in range(1, 1025):
            assert lib.pcgmix_conv3_wgrad_supported(cin, cout) == lib.pcgmix_conv3_supported(cin, cout), (cin, cout)
    for cin, cout in [(0, 16), (-4, 16), (16, 0), (16, -16), (1028, 16), (16, 1040)]:
        assert lib.pcgmix_conv3_wgrad_supported(cin, cout) == 0, (cin, cout)


def test_tile_constants(lib):
    TK, MO, NI = W.tile(lib)
    assert TK >= 2 and TK % 2 == 0 and MO % 32 == 0 and MO >= 32 and NI % 32 == 0 and NI >= 32
    for which in (-1, 3, 4, 100):
        assert lib.pcgmix_conv3_wgrad_tile(which) == 0


def test_plan_properties(lib):
    TK = W.tile(lib)[0]
    widths = [(4, 16), (4, 64), (16, 32), (64, 4), (64, 128), (96, 192), (128, 128), (256, 512), (512, 512),
              (1024, 16), (16, 1024), (1024, 1024)]
    for B in (1, 2, 3, 5, 8, 256):
        for L in (1, 2, TK - 1, TK, TK + 1, 2 * TK + 3, 312, 625, 1250, 2500):
            for cin, cout in widths:
                rc, s, n = W.plan(lib, B, L, cin, cout)
                assert rc == 0
                assert 1 <= s <= B * -(-L // TK), (B, L, cin, cout, s)
                if s > 1:
                    assert n >= s * cout * 3 * cin * 4
                assert n % 16 == 0
                assert W.plan(lib, B, L, cin, cout) == (rc, s, n)          # the same answer twice
    assert W.plan(lib, 0, 9, 16, 32)[:2] == (0, 1)                         # an empty batch still plans
    for cin, cout in [(1, 64), (4, 8), (6, 16), (1028, 16), (0, 16), (16, 2)]:
        assert W.plan(lib, 2, 9, cin, cout)[0] != 0, (cin, cout)
    assert W.plan(lib, -1, 9, 16, 32)[0] != 0 and W.plan(lib, 2, 0, 16, 32)[0] != 0
    # either output pointer may be left out
    assert lib.pcgmix_conv3_wgrad_plan(2, 9, 16, 32, None, None) == 0
