"""pcgmix_conv3_nlc_f32 (csrc/pcgmix_conv3.hip: Conv1d(k = 3, pad = 1), channels innermost, on the f32
matrix instruction) through the C ABI against the restatement of tests/conv3_ref.py.

  * integer data (x in [-4,4], w in [-2,2]): |any partial sum| <= 3 * 1024 * 8 = 24576 < 2**24, every
    order of summation is exact in float32, so y equals the int64 restatement BIT FOR BIT;
  * the halo: a sample between two samples filled with 1000 keeps zero padding at both ends;
  * y as a slice of a sentinel-filled buffer: nothing outside the slice is written;
  * random data: |y - float64| <= (K + 1) * 2**-24 * sum|x w|, K = 3 Cin — the bound of a K-term fmaf chain;
  * determinism: two launches give the same bits, and a sample's bits do not depend on B;
  * refusals leave y untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import conv3_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -1.5e9                        # no result holds it: integer results are below 2**24
GUARD = 256
TM, KC = R.tile(_lib.load())         # the built kernel's own tile: 128 positions, 16 channels a K group
# (B, L, Cin, Cout):
#   L = 1, 2, 5             one-row samples and a tile that is nearly all halo
#   L = TM-1, TM, TM+1      the M tile minus one, exact, plus one (second tile: one row)
#   (2,313,64,4)            the last hop of the input gradient: 4 of 32 columns stored
#   (2,130,128,128)         the 128-column tile, 8 K groups
#   (2,625,96,192)          64-column tiles; 96 = 6 K groups
#   (1,2500,4,64)           the first layer: one K group of 4 channels, 20 tiles
#   (1,78,1024,16)          the longest K (64 groups), 16 of 32 columns stored
SHAPES = [(2, 1, 4, 16), (2, 2, 4, 16), (3, 5, 4, 16), (2, TM - 1, 16, 32), (2, TM, 16, 32),
          (2, TM + 1, 16, 32), (2, 313, 64, 4), (2, 130, 128, 128), (2, 625, 96, 192), (1, 2500, 4, 64),
          (1, 78, 1024, 16)]


def _conv3(x, w, y, B, L, Cin, Cout):
    return _lib.load().pcgmix_conv3_nlc_f32(
        x.data_ptr() if x is not None else None, w.data_ptr() if w is not None else None,
        y.data_ptr() if y is not None else None, B, L, Cin, Cout,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _run(x, w, device):
    B, L, Cin = x.shape
    Cout = w.shape[0]
    y = torch.full((B, L, Cout), SENT, dtype=torch.float32, device=device)
    assert _conv3(_dev(x, device), _dev(w, device), y, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_shapes_sit_at_the_kernel_s_tile_edges():
    assert TM >= 8 and KC >= 4
    Ls = {L for _, L, _, _ in SHAPES}
    assert {1, TM - 1, TM, TM + 1} <= Ls and max(Ls) > 2 * TM
    cins = {c for _, _, c, _ in SHAPES}
    assert min(cins) < KC and any(c > KC and c % KC == 0 for c in cins) and max(cins) == 1024
    assert {4, 16} <= {o for _, _, _, o in SHAPES} and any(o % 128 == 0 for _, _, _, o in SHAPES)


@pytest.mark.parametrize("B,L,Cin,Cout", SHAPES)
def test_integer_data_is_exact(device, B, L, Cin, Cout):
    x, w = R.int_case(B, L, Cin, Cout)
    want = R.conv3_int(x, w)
    assert np.abs(want).max() < 2 ** 24
    got = _run(x, w, device)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("L,Cin,Cout", [(1, 4, 16), (TM, 16, 32), (TM + 1, 64, 4), (300, 128, 128)])
def test_halo_is_zero_padding_not_the_neighbour(device, L, Cin, Cout):
    x, w = R.int_case(3, L, Cin, Cout, seed=1)
    w[:] = np.where(w == 0, 1, w)                          # every neighbour value would show
    x[0] = 1000
    x[2] = 1000
    got = _run(x, w, device)
    want = R.conv3_int(x[1:2], w)[0]
    assert np.array_equal(got[1, 0], want[0]) and np.array_equal(got[1, L - 1], want[L - 1])
    assert np.array_equal(got[1], want)


@pytest.mark.parametrize("B,L,Cin,Cout", [(2, 5, 4, 16), (2, TM + 1, 16, 32), (2, 313, 64, 4),
                                          (2, 130, 128, 128)])
def test_nothing_outside_y_is_written(device, B, L, Cin, Cout):
    x, w = R.int_case(B, L, Cin, Cout, seed=2)
    n = B * L * Cout
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=device)
    y = buf[GUARD:GUARD + n]
    assert y.data_ptr() % 16 == 0
    assert _conv3(_dev(x, device), _dev(w, device), y, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == np.float32(SENT)).all() and (out[GUARD + n:] == np.float32(SENT)).all()
    assert np.array_equal(out[GUARD:GUARD + n].reshape(B, L, Cout), R.conv3_int(x, w).astype(np.float32))


@pytest.mark.parametrize("B,L,Cin,Cout", [(2, 313, 128, 256), (2, 1250, 64, 4)])
def test_float_data_within_the_fmaf_chain_bound(device, B, L, Cin, Cout, record_property):
    rs = np.random.RandomState(3)
    x = rs.standard_normal((B, L, Cin)).astype(np.float32)
    w = rs.standard_normal((Cout, 3, Cin)).astype(np.float32)
    want, mag = R.conv3_f64(x, w)
    got = _run(x, w, device)
    K = 3 * Cin
    bound = (K + 1) * 2.0 ** -24 * mag
    ratio = float((np.abs(got.astype(np.float64) - want) / bound).max())
    record_property("max_err_over_bound", ratio)
    print(f"conv3 float ({B},{L},{Cin},{Cout}): max |err| / bound = {ratio:.4f}, "
          f"max |err| = {np.abs(got - want).max():.3e}")
    assert ratio <= 1.0


def test_two_launches_and_any_batch_give_the_same_bits(device):
    B, L, Cin, Cout = 5, 313, 128, 256
    rs = np.random.RandomState(4)
    x = _dev(rs.standard_normal((B, L, Cin)), device)
    w = _dev(rs.standard_normal((Cout, 3, Cin)), device)
    ys = [torch.full((B, L, Cout), SENT, dtype=torch.float32, device=device) for _ in range(2)]
    for y in ys:
        assert _conv3(x, w, y, B, L, Cin, Cout) == 0
    y1 = torch.full((1, L, Cout), SENT, dtype=torch.float32, device=device)
    assert _conv3(x[:1].contiguous(), w, y1, 1, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])
    assert torch.equal(y1[0], ys[0][0])
    # and a sample's bits do not depend on its place in the batch
    y4 = torch.full((1, L, Cout), SENT, dtype=torch.float32, device=device)
    assert _conv3(x[4:5].contiguous(), w, y4, 1, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    assert torch.equal(y4[0], ys[0][4])


def test_refusals_leave_y_untouched(device):
    B, L, Cin, Cout = 2, 9, 16, 32
    x = torch.ones((B, L, Cin), dtype=torch.float32, device=device)
    w = torch.ones((Cout, 3, Cin), dtype=torch.float32, device=device)
    buf = torch.full((B * L * Cout + 4,), SENT, dtype=torch.float32, device=device)
    y = buf[:B * L * Cout]
    xo = torch.ones((B * L * Cin + 4,), dtype=torch.float32, device=device)
    wo = torch.ones((Cout * 3 * Cin + 4,), dtype=torch.float32, device=device)
    assert x.data_ptr() % 16 == 0 and xo[1:].data_ptr() % 16 == 4
    bad = [
        (x, w, y, B, L, 1, 64), (x, w, y, B, L, 4, 8), (x, w, y, B, L, 6, 16), (x, w, y, B, L, 1028, 16),
        (None, w, y, B, L, Cin, Cout), (x, None, y, B, L, Cin, Cout), (x, w, None, B, L, Cin, Cout),
        (xo[1:], w, y, B, L, Cin, Cout), (x, wo[1:], y, B, L, Cin, Cout), (x, w, buf[1:], B, L, Cin, Cout),
        (x, w, y, B, 0, Cin, Cout), (x, w, y, B, -3, Cin, Cout), (x, w, y, -1, L, Cin, Cout),
    ]
    for a in bad:
        assert _conv3(*a) == INVALID, a[3:]
    assert _conv3(x, w, y, 0, L, Cin, Cout) == 0            # an empty batch: success, no launch
    torch.cuda.synchronize()
    assert (buf == SENT).all()
    assert _conv3(x, w, y, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    got = y.view(B, L, Cout).cpu().numpy()
    assert np.array_equal(got, R.conv3_int(np.ones((B, L, Cin)), np.ones((Cout, 3, Cin))).astype(np.float32))
