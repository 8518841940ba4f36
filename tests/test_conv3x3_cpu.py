"""The restatement of the 3x3 convolution (tests/conv3x3_ref.py) against torch in float64, and the
host-only part of its C ABI (csrc/pcgmix_conv3x3.hip): the shape predicate, the tile constants and
the ABI number."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import conv3x3_ref as R

# every (Cin, Cout) ResNet9-2D runs, forward and as the input gradient
NETWORK = [(1, 64), (64, 128), (128, 128), (128, 256), (256, 512), (512, 512), (128, 64), (256, 128),
           (512, 256), (64, 1)]
SHAPES = [(1, 1, 1, 1, 16), (2, 2, 3, 4, 4), (3, 5, 4, 8, 16), (2, 7, 9, 12, 1), (2, 9, 20, 20, 32)]


def _rand(B, H, W, Cin, Cout, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((B, H, W, Cin)), rs.standard_normal((Cout, 3, 3, Cin))


def _nchw(a):
    return torch.from_numpy(a).permute(0, 3, 1, 2)          # (.., H, W, C) memory -> torch's (.., C, H, W)


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_restatement_matches_torch_conv2d(B, H, W, Cin, Cout):
    x, w = _rand(B, H, W, Cin, Cout, 0)
    want = F.conv2d(_nchw(x), _nchw(w), padding=1).permute(0, 2, 3, 1).numpy()
    got, mag = R.conv3x3_f64(x, w)
    assert got.shape == (B, H, W, Cout)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, mag.max())
    assert (mag >= np.abs(got) - 1e-12 * mag).all()
    xi, wi = R.int_case(B, H, W, Cin, Cout)
    yi = R.conv3x3_int(xi, wi)
    assert yi.dtype == np.int64
    assert np.array_equal(yi, R.conv3x3_f64(xi, wi)[0])     # integers: float64 is exact as well
    assert np.abs(yi).max() < 2 ** 24
    assert np.abs(xi).max() <= 4 and np.abs(wi).max() <= 2 and 9 * 1024 * 8 < 2 ** 24


@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_flipped_transposed_weights_give_the_input_gradient(B, H, W, Cin, Cout):
    x, w = _rand(B, H, W, Cin, Cout, 1)
    dy = np.random.RandomState(2).standard_normal((B, H, W, Cout))
    xt = _nchw(x).requires_grad_(True)
    y = F.conv2d(xt, _nchw(w), padding=1)
    (want,) = torch.autograd.grad(y, xt, _nchw(dy))
    wt = R.flip_transpose(w)
    assert wt.shape == (Cin, 3, 3, Cout)
    got, mag = R.conv3x3_f64(dy, wt)
    assert np.abs(got - want.permute(0, 2, 3, 1).numpy()).max() <= 1e-12 * max(1.0, mag.max())


def test_supported_predicate_of_the_built_library():
    lib = ctypes.CDLL(_lib.LIB_PATH)                        # no device call is made
    fn = lib.pcgmix_conv3x3_supported
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
    for cin, cout in NETWORK:
        assert fn(cin, cout) == 1, (cin, cout)
    for cin, cout in [(1, 1), (4, 16), (16, 8), (1040, 16)]:
        assert fn(cin, cout) == 0, (cin, cout)
    for cin, cout in [(0, 16), (-16, 16), (16, 0), (16, -16), (0, 0), (-1, 16), (16, -1)]:
        assert fn(cin, cout) == 0, (cin, cout)
    assert fn(1024, 1024) == 1 and fn(16, 1040) == 0 and fn(1, 1024) == 1 and fn(1024, 1) == 1


def test_tile_constants_and_signatures():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    th, tw, kc = (lib.pcgmix_conv3x3_tile(i) for i in range(3))
    assert R.tile(_lib.load()) == (th, tw, kc)
    assert th >= 1 and tw >= 1 and th * tw % 32 == 0        # whole 32-row matrix operands
    assert (-(-16 // th) * th) * (-(-16 // tw) * tw) < 2 * 256   # the tiles over a 16 x 16 map are not half waste
    assert kc % 4 == 0 and 16 % kc == 0                     # every supported Cin is whole K groups
    assert lib.pcgmix_conv3x3_tile(3) == 0 and lib.pcgmix_conv3x3_tile(-1) == 0
    for n in ("pcgmix_conv3x3_supported", "pcgmix_conv3x3_tile", "pcgmix_conv3x3_nhwc_f32"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)


def test_abi_version_is_unchanged():
    assert _lib.load().pcgmix_abi_version() == 25 == _lib.ABI_VERSION
