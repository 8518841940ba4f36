"""pcgmix_conv3x3_nhwc_f32 (csrc/pcgmix_conv3x3.hip: Conv2d(k = 3x3, pad = 1), channels innermost, on
the f32 matrix instruction, with a VALU kernel each for Cin == 1 and Cout == 1) through the C ABI
against the restatement of tests/conv3x3_ref.py.

  * integer data (x in [-4,4], w in [-2,2]): |any partial sum| <= 9 * 1024 * 8 = 73728 < 2**24, every
    order of summation is exact in float32, so y equals the int64 restatement BIT FOR BIT; one variant
    has no zero weight, so that any wrong neighbour shows (a row's end reading the next row's start);
  * the halo: a sample between two samples filled with 1000 keeps zero padding on all four sides;
  * y as a slice of a sentinel-filled buffer: nothing outside the slice is written;
  * random data: |y - float64| <= (K + 1) * 2**-24 * sum|x w|, K = 9 Cin — the bound of a K-term fmaf
    chain, which also covers the Cout == 1 kernel's 16 chains + 4 + 9 adds (fewer roundings per element);
  * determinism: two launches give the same bits, and a sample's bits do not depend on B or its place;
  * refusals leave y untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import conv3x3_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -1.5e9                        # no result holds it: integer results are below 2**24
GUARD = 256
TH, TW, KC = R.tile(_lib.load())     # the built kernel's own tile: 8 x 16 pixels, 16 channels a K group
# (B, H, W, Cin, Cout):
#   (2,1,1,16,16) (2,1,2,1,16) (2,2,1,16,1)   one-pixel / one-row / one-column samples: a tile that is
#                                             nearly all halo, in each of the three kernels
#   (3,3,5,16,32)                             odd sizes below a tile
#   H, W = TH-1, TW+1 / TH, TW / TH+1, TW-1   a tile minus one, exact, plus one in either direction
#   (2,16,16,64,1)                            the last hop of the input gradient
#   (1,32,20,1,64)                            the first layer; W no multiple of TW
#   (2,9,17,128,128)                          the 128-column N tile, 8 K groups, 2 x 2 tiles
#   (1,16,16,96,192)                          64-column N tiles; 96 = 6 K groups
#   (1,5,7,1024,16)                           the longest K (64 groups), 16 of 32 columns stored
#   (1,4,6,512,512)                           the network's widest layer at its smallest map
SHAPES = [(2, 1, 1, 16, 16), (2, 1, 2, 1, 16), (2, 2, 1, 16, 1), (3, 3, 5, 16, 32),
          (2, TH - 1, TW + 1, 16, 32), (2, TH, TW, 16, 32), (2, TH + 1, TW - 1, 16, 32),
          (2, 16, 16, 64, 1), (1, 32, 20, 1, 64), (2, 9, 17, 128, 128), (1, 16, 16, 96, 192),
          (1, 5, 7, 1024, 16), (1, 4, 6, 512, 512)]


def _conv3x3(x, w, y, B, H, W, Cin, Cout):
    return _lib.load().pcgmix_conv3x3_nhwc_f32(
        x.data_ptr() if x is not None else None, w.data_ptr() if w is not None else None,
        y.data_ptr() if y is not None else None, B, H, W, Cin, Cout,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _run(x, w, device):
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    y = torch.full((B, H, W, Cout), SENT, dtype=torch.float32, device=device)
    assert _conv3x3(_dev(x, device), _dev(w, device), y, B, H, W, Cin, Cout) == 0
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_shapes_sit_at_the_kernel_s_tile_edges():
    assert TH >= 2 and TW >= 2 and KC >= 4
    main = [s for s in SHAPES if s[3] > 1 and s[4] > 1]
    Hs, Ws = {s[1] for s in main}, {s[2] for s in main}
    assert {1, TH - 1, TH, TH + 1} <= Hs and {1, TW - 1, TW, TW + 1} <= Ws
    cins = {s[3] for s in main}
    assert min(cins) <= KC and any(c > KC and c % KC == 0 for c in cins) and max(cins) == 1024
    assert any(s[3] == 1 for s in SHAPES) and any(s[4] == 1 for s in SHAPES)        # both narrow ends
    assert any(s[4] % 128 == 0 for s in main) and any(s[4] % 64 == 0 and s[4] % 128 for s in main)
    assert any(s[4] % 32 for s in main)                                              # a half-empty N tile


@pytest.mark.parametrize("nonzero", [False, True], ids=["any-w", "nonzero-w"])
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_integer_data_is_exact(device, B, H, W, Cin, Cout, nonzero):
    x, w = R.int_case(B, H, W, Cin, Cout)
    if nonzero:
        w[:] = np.where(w == 0, 1, w)                      # every neighbour value shows
        x[:] = np.where(x == 0, 3, x)
    want = R.conv3x3_int(x, w)
    assert np.abs(want).max() < 2 ** 24
    got = _run(x, w, device)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("H,W,Cin,Cout", [(1, 1, 16, 16), (TH, TW, 16, 32), (TH + 1, TW + 1, 64, 1),
                                          (5, 7, 1, 16), (9, 17, 128, 128)])
def test_halo_is_zero_padding_not_the_neighbour(device, H, W, Cin, Cout):
    x, w = R.int_case(3, H, W, Cin, Cout, seed=1)
    w[:] = np.where(w == 0, 1, w)                          # every neighbour value would show
    x[0] = 1000
    x[2] = 1000
    got = _run(x, w, device)
    want = R.conv3x3_int(x[1:2], w)[0]
    for edge in (np.s_[0], np.s_[H - 1], np.s_[:, 0], np.s_[:, W - 1]):      # top, bottom, left, right
        assert np.array_equal(got[1][edge], want[edge])
    assert np.array_equal(got[1], want)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 3, 5, 16, 32), (2, TH + 1, TW - 1, 16, 32), (2, 16, 16, 64, 1),
                                            (1, 32, 20, 1, 64), (2, 9, 17, 128, 128)])
def test_nothing_outside_y_is_written(device, B, H, W, Cin, Cout):
    x, w = R.int_case(B, H, W, Cin, Cout, seed=2)
    n = B * H * W * Cout
    pad = (-n) % 4                                          # the guard behind y starts 16-byte aligned or not: both fine
    buf = torch.full((GUARD + n + pad + GUARD,), SENT, dtype=torch.float32, device=device)
    y = buf[GUARD:GUARD + n]
    assert y.data_ptr() % 16 == 0
    assert _conv3x3(_dev(x, device), _dev(w, device), y, B, H, W, Cin, Cout) == 0
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == np.float32(SENT)).all() and (out[GUARD + n:] == np.float32(SENT)).all()
    assert np.array_equal(out[GUARD:GUARD + n].reshape(B, H, W, Cout), R.conv3x3_int(x, w).astype(np.float32))


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 16, 24, 128, 256), (2, 32, 48, 64, 1)])
def test_float_data_within_the_fmaf_chain_bound(device, B, H, W, Cin, Cout, record_property):
    rs = np.random.RandomState(3)
    x = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = rs.standard_normal((Cout, 3, 3, Cin)).astype(np.float32)
    want, mag = R.conv3x3_f64(x, w)
    got = _run(x, w, device)
    K = 9 * Cin
    bound = (K + 1) * 2.0 ** -24 * mag
    ratio = float((np.abs(got.astype(np.float64) - want) / bound).max())
    record_property("max_err_over_bound", ratio)
    print(f"conv3x3 float ({B},{H},{W},{Cin},{Cout}): max |err| / bound = {ratio:.4f}, "
          f"max |err| = {np.abs(got - want).max():.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(5, 16, 24, 128, 256), (3, 16, 16, 64, 1)])
def test_two_launches_and_any_batch_give_the_same_bits(device, B, H, W, Cin, Cout):
    rs = np.random.RandomState(4)
    x = _dev(rs.standard_normal((B, H, W, Cin)), device)
    w = _dev(rs.standard_normal((Cout, 3, 3, Cin)), device)
    ys = [torch.full((B, H, W, Cout), SENT, dtype=torch.float32, device=device) for _ in range(2)]
    for y in ys:
        assert _conv3x3(x, w, y, B, H, W, Cin, Cout) == 0
    y1 = torch.full((1, H, W, Cout), SENT, dtype=torch.float32, device=device)
    assert _conv3x3(x[:1].contiguous(), w, y1, 1, H, W, Cin, Cout) == 0
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])
    assert torch.equal(y1[0], ys[0][0])
    # and a sample's bits do not depend on its place in the batch
    yl = torch.full((2, H, W, Cout), SENT, dtype=torch.float32, device=device)
    assert _conv3x3(x[B - 2:].contiguous(), w, yl, 2, H, W, Cin, Cout) == 0
    torch.cuda.synchronize()
    assert torch.equal(yl[1], ys[0][B - 1]) and torch.equal(yl[0], ys[0][B - 2])


def test_refusals_leave_y_untouched(device):
    B, H, W, Cin, Cout = 2, 3, 5, 16, 32
    x = torch.ones((B, H, W, Cin), dtype=torch.float32, device=device)
    w = torch.ones((Cout, 3, 3, Cin), dtype=torch.float32, device=device)
    n = B * H * W * Cout
    buf = torch.full((n + 4,), SENT, dtype=torch.float32, device=device)
    y = buf[:n]
    xo = torch.ones((B * H * W * Cin + 4,), dtype=torch.float32, device=device)
    wo = torch.ones((Cout * 9 * Cin + 4,), dtype=torch.float32, device=device)
    assert x.data_ptr() % 16 == 0 and xo[1:].data_ptr() % 16 == 4
    bad = [
        (x, w, y, B, H, W, 1, 1), (x, w, y, B, H, W, 4, 16), (x, w, y, B, H, W, 16, 8),
        (x, w, y, B, H, W, 1040, 16), (x, w, y, B, H, W, 0, 16), (x, w, y, B, H, W, 16, -16),
        (None, w, y, B, H, W, Cin, Cout), (x, None, y, B, H, W, Cin, Cout), (x, w, None, B, H, W, Cin, Cout),
        (xo[1:], w, y, B, H, W, Cin, Cout), (x, wo[1:], y, B, H, W, Cin, Cout), (x, w, buf[1:], B, H, W, Cin, Cout),
        (x, w, y, B, 0, W, Cin, Cout), (x, w, y, B, H, 0, Cin, Cout), (x, w, y, B, -3, W, Cin, Cout),
        (x, w, y, B, H, -1, Cin, Cout), (x, w, y, -1, H, W, Cin, Cout),
        (x, w, y, B, 1 << 14, 1 << 14, Cin, Cout),                  # H * W * max(Cin, Cout) = 2**33
        (x, w, y, B, 46341, 46341, Cin, Cout),                      # H * W alone above INT_MAX
        (x, w, y, 1 << 30, 1 << 11, 1 << 11, 1, 16),                # 2**30 * 2**22 * 4 / 1024 blocks
    ]
    for a in bad:
        assert _conv3x3(*a) == INVALID, a[3:]
    assert _conv3x3(x, w, y, 0, H, W, Cin, Cout) == 0       # an empty batch: success, no launch
    torch.cuda.synchronize()
    assert (buf == SENT).all()
    assert _conv3x3(x, w, y, B, H, W, Cin, Cout) == 0
    torch.cuda.synchronize()
    got = y.view(B, H, W, Cout).cpu().numpy()
    want = R.conv3x3_int(np.ones((B, H, W, Cin)), np.ones((Cout, 3, 3, Cin))).astype(np.float32)
    assert np.array_equal(got, want)
