"""The restatement of the k = 3 convolution (tests/conv3_ref.py) against torch in float64, and the
host-only part of its C ABI (csrc/pcgmix_conv3.hip): the shape predicate and the ABI number."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import conv3_ref as R

# every width of resnet9 and of resnet9-150k .. resnet9-9m, and the four input channels
WIDTHS = (4, 16, 32, 64, 96, 128, 192, 256, 384, 512, 768, 1024)
SHAPES = [(1, 1, 4, 16), (2, 2, 4, 4), (3, 5, 8, 16), (2, 37, 12, 48), (2, 130, 20, 32)]


def _rand(B, L, Cin, Cout, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((B, L, Cin)), rs.standard_normal((Cout, 3, Cin))


def _torch_w(w):
    return torch.from_numpy(w).permute(0, 2, 1)           # (O, 3, I) memory -> Conv1d's (O, I, 3)


@pytest.mark.parametrize("B,L,Cin,Cout", SHAPES)
def test_restatement_matches_torch_conv1d(B, L, Cin, Cout):
    x, w = _rand(B, L, Cin, Cout, 0)
    want = F.conv1d(torch.from_numpy(x).permute(0, 2, 1), _torch_w(w), padding=1).permute(0, 2, 1).numpy()
    got, mag = R.conv3_f64(x, w)
    assert got.shape == (B, L, Cout)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, mag.max())
    assert (mag >= np.abs(got) - 1e-12 * mag).all()
    xi, wi = R.int_case(B, L, Cin, Cout)
    yi = R.conv3_int(xi, wi)
    assert yi.dtype == np.int64
    assert np.array_equal(yi, R.conv3_f64(xi, wi)[0])       # integers: float64 is exact as well
    assert np.abs(yi).max() < 2 ** 24


@pytest.mark.parametrize("B,L,Cin,Cout", SHAPES)
def test_flipped_transposed_weights_give_the_input_gradient(B, L, Cin, Cout):
    x, w = _rand(B, L, Cin, Cout, 1)
    dy = np.random.RandomState(2).standard_normal((B, L, Cout))
    xt = torch.from_numpy(x).permute(0, 2, 1).requires_grad_(True)
    y = F.conv1d(xt, _torch_w(w), padding=1)
    (want,) = torch.autograd.grad(y, xt, torch.from_numpy(dy).permute(0, 2, 1))
    wt = R.flip_transpose(w)
    assert wt.shape == (Cin, 3, Cout)
    got, mag = R.conv3_f64(dy, wt)
    assert np.abs(got - want.permute(0, 2, 1).numpy()).max() <= 1e-12 * max(1.0, mag.max())


def test_supported_predicate_of_the_built_library():
    lib = ctypes.CDLL(_lib.LIB_PATH)                        # no device call is made
    fn = lib.pcgmix_conv3_supported
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
    for cin in WIDTHS:
        for cout in WIDTHS:
            assert fn(cin, cout) == 1, (cin, cout)
    for cin, cout in [(1, 64), (4, 8), (6, 16), (1028, 16)]:
        assert fn(cin, cout) == 0, (cin, cout)
    for cin, cout in [(0, 16), (-4, 16), (16, 0), (16, -16), (16, 2), (3, 4)]:
        assert fn(cin, cout) == 0, (cin, cout)
    assert R.tile(_lib.load()) == (lib.pcgmix_conv3_tile(0), lib.pcgmix_conv3_tile(1))
    assert lib.pcgmix_conv3_tile(0) % 32 == 0 and lib.pcgmix_conv3_tile(1) % 4 == 0 and lib.pcgmix_conv3_tile(2) == 0
    for n in ("pcgmix_conv3_supported", "pcgmix_conv3_tile", "pcgmix_conv3_nlc_f32"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)


def test_abi_version_is_unchanged():
    assert _lib.load().pcgmix_abi_version() == 25 == _lib.ABI_VERSION
