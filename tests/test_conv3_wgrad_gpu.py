"""pcgmix_conv3_wgrad_nlc_f32 (csrc/pcgmix_conv3_wgrad.hip: the weight gradient of Conv1d(k = 3, pad = 1),
channels innermost, split-K in a fixed order on the f32 matrix instruction) through the C ABI against
the restatement of tests/conv3_wgrad_ref.py.

  * integer data (x in [-4,4], dy in [-2,2]): |any partial sum| <= 8 B L <= 20,000 < 2**24, every order of
    summation is exact in float32, so dw equals the int64 restatement BIT FOR BIT;
  * the halo: a sample between two samples whose x is 1000 and whose dy is 0 gives its own dw;
  * dw as a slice of a sentinel-filled buffer, the workspace likewise guarded beyond the planned bytes:
    nothing outside is written;
  * the workspace pre-filled with NaN and with 1e30 gives the same bits: it is never read before written;
  * random data: |dw - float64| <= (B L + 1) * 2**-24 * sum|dy x| — the bound of ANY order of summation
    over B L products;
  * determinism: two launches and a launch on a side stream give the same bits;
  * refusals leave dw untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import conv3_wgrad_ref as W

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -1.5e9                        # no result holds it: integer results are below 2**24
GUARD = 256
TK, MO, NI = W.tile(_lib.load())     # the built kernel's own tile: 64 positions, 128 x 64 channels
# (B, L, Cin, Cout):
#   L = 1, 2, 5             one-row samples: a K tile that is nearly all zero rows
#   L = TK-1, TK, TK+1      the K tile minus one, exact, plus one (second tile: one row)
#   (5,2TK+3,16,32)         15 K tiles, ragged against the split
#   (2,313,64,4)            4 of 128 output rows stored
#   (5,130,128,128)         one full block tile of output channels, two of input channels
#   (3,157,96,192)          two M tiles (the second half full), 96 = one and a half N tiles
#   (1,2500,4,64)           the first layer: 4 of 32 columns, 40 K tiles of one sample
#   (7,39,1024,16)          the widest N (16 tiles), 16 of 128 rows
#   (2,39,16,1024)          the widest M (8 tiles)
SHAPES = [(1, 1, 4, 16), (2, 2, 4, 16), (3, 5, 4, 16), (2, TK - 1, 16, 32), (2, TK, 16, 32),
          (2, TK + 1, 16, 32), (5, 2 * TK + 3, 16, 32), (2, 313, 64, 4), (5, 130, 128, 128),
          (3, 157, 96, 192), (1, 2500, 4, 64), (7, 39, 1024, 16), (2, 39, 16, 1024)]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _call(x, dy, dw, ws, nbytes, B, L, Cin, Cout):
    return _lib.load().pcgmix_conv3_wgrad_nlc_f32(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), nbytes, B, L, Cin,
                                                  Cout, _stream())


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _plan(B, L, Cin, Cout):
    rc, s, n = W.plan(_lib.load(), B, L, Cin, Cout)
    assert rc == 0 and n % 4 == 0
    return s, n


def _workspace(nbytes, device, fill=SENT):
    """(guarded buffer, the workspace inside it or None): GUARD floats of ``fill`` on either side."""
    buf = torch.full((GUARD + nbytes // 4 + GUARD,), fill, dtype=torch.float32, device=device)
    return buf, (buf[GUARD:GUARD + nbytes // 4] if nbytes else None)


def _run(x, dy, device, fill=SENT):
    """dw (Cout, 3, Cin) as numpy; asserts that nothing outside dw and the planned workspace is written."""
    B, L, Cin = x.shape
    Cout = dy.shape[2]
    n = Cout * 3 * Cin
    _, nbytes = _plan(B, L, Cin, Cout)
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=device)
    dw = buf[GUARD:GUARD + n]
    wbuf, ws = _workspace(nbytes, device, fill)
    assert dw.data_ptr() % 16 == 0 and (ws is None or ws.data_ptr() % 16 == 0)
    assert _call(_dev(x, device), _dev(dy, device), dw, ws, nbytes, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    out, wout = buf.cpu().numpy(), wbuf.cpu().numpy()
    assert (out[:GUARD] == np.float32(SENT)).all() and (out[GUARD + n:] == np.float32(SENT)).all()
    for edge in (wout[:GUARD], wout[GUARD + nbytes // 4:]):
        assert np.array_equal(edge.view(np.uint32), np.full(GUARD, fill, np.float32).view(np.uint32))
    return out[GUARD:GUARD + n].reshape(Cout, 3, Cin)


def test_shapes_sit_at_the_kernel_s_tile_edges():
    assert TK >= 8 and MO >= 32 and NI >= 32
    Ls = {L for _, L, _, _ in SHAPES}
    assert {1, TK - 1, TK, TK + 1, 2 * TK + 3} <= Ls and max(Ls) > 2 * TK
    cins = {c for _, _, c, _ in SHAPES}
    couts = {o for _, _, _, o in SHAPES}
    assert min(cins) == 4 and max(cins) == 1024 and any(c > NI and c % NI for c in cins)
    assert any(c % NI == 0 and c > NI for c in cins)
    assert {4, 16} <= couts and max(couts) == 1024 and any(o == MO for o in couts)
    assert any(o > MO and o % MO for o in couts)
    # the split: one shape with a single range, one whose K tiles do not divide among the splits
    lib = _lib.load()
    splits = {s: W.plan(lib, *s)[1] for s in SHAPES}
    assert min(splits.values()) == 1 and max(splits.values()) > 1
    B, L, _, _ = ragged = (5, 2 * TK + 3, 16, 32)
    assert B * -(-L // TK) == 15 and splits[ragged] > 1 and 15 % splits[ragged] != 0


@pytest.mark.parametrize("B,L,Cin,Cout", SHAPES)
def test_integer_data_is_exact(device, B, L, Cin, Cout):
    x, dy = W.int_case(B, L, Cin, Cout)
    want = W.wgrad_int(x, dy)
    assert 8 * B * L <= 20000 and np.abs(want).max() < 2 ** 24
    got = _run(x, dy, device)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("L,Cin,Cout", [(1, 4, 16), (TK, 16, 32), (TK + 1, 64, 4), (300, 128, 128)])
def test_halo_is_zero_padding_not_the_neighbour(device, L, Cin, Cout):
    x, dy = W.int_case(3, L, Cin, Cout, seed=1)
    dy[1] = np.where(dy[1] == 0, 1, dy[1])                 # every neighbour value would show
    x[0] = 1000
    x[2] = 1000
    dy[0] = 0
    dy[2] = 0
    want = W.wgrad_int(x[1:2], dy[1:2])
    assert np.array_equal(want, W.wgrad_int(x, dy))
    got = _run(x, dy, device)
    assert np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("B,L,Cin,Cout", [(3, 5, 4, 16), (5, 2 * TK + 3, 16, 32), (2, 313, 64, 4),
                                          (5, 130, 128, 128), (3, 157, 96, 192)])
def test_nothing_outside_dw_and_the_workspace_is_written(device, B, L, Cin, Cout):
    x, dy = W.int_case(B, L, Cin, Cout, seed=2)
    got = _run(x, dy, device)                              # _run checks both guards
    assert np.array_equal(got, W.wgrad_int(x, dy).astype(np.float32))


@pytest.mark.parametrize("B,L,Cin,Cout", [(5, 2 * TK + 3, 16, 32), (5, 130, 128, 128), (3, 157, 96, 192),
                                          (1, 2500, 4, 64)])
def test_workspace_is_never_read_before_it_is_written(device, B, L, Cin, Cout):
    assert _plan(B, L, Cin, Cout)[0] > 1
    rs = np.random.RandomState(5)
    x = rs.standard_normal((B, L, Cin)).astype(np.float32)
    dy = rs.standard_normal((B, L, Cout)).astype(np.float32)
    a = _run(x, dy, device, fill=float("nan"))
    b = _run(x, dy, device, fill=1e30)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("B,L,Cin,Cout", [(5, 313, 128, 256), (4, 1250, 4, 64)])
def test_float_data_within_the_bound_of_any_order(device, B, L, Cin, Cout, record_property):
    rs = np.random.RandomState(3)
    x = rs.standard_normal((B, L, Cin)).astype(np.float32)
    dy = rs.standard_normal((B, L, Cout)).astype(np.float32)
    want, mag = W.wgrad_f64(x, dy)
    got = _run(x, dy, device)
    bound = (B * L + 1) * 2.0 ** -24 * mag
    ratio = float((np.abs(got.astype(np.float64) - want) / bound).max())
    record_property("max_err_over_bound", ratio)
    print(f"conv3 wgrad float ({B},{L},{Cin},{Cout}): max |err| / bound = {ratio:.5f}, "
          f"max |err| = {np.abs(got - want).max():.3e}")
    assert ratio <= 1.0


def test_two_launches_and_a_side_stream_give_the_same_bits(device):
    B, L, Cin, Cout = 5, 313, 128, 256
    rs = np.random.RandomState(4)
    x = _dev(rs.standard_normal((B, L, Cin)), device)
    dy = _dev(rs.standard_normal((B, L, Cout)), device)
    splits, nbytes = _plan(B, L, Cin, Cout)
    assert splits > 1
    outs = [torch.full((Cout, 3, Cin), SENT, dtype=torch.float32, device=device) for _ in range(3)]
    wss = [torch.empty(nbytes // 4, dtype=torch.float32, device=device) for _ in range(3)]
    for dw, ws in zip(outs[:2], wss[:2]):
        assert _call(x, dy, dw, ws, nbytes, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert _call(x, dy, outs[2], wss[2], nbytes, B, L, Cin, Cout) == 0
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_refusals_leave_dw_untouched(device):
    B, L, Cin, Cout = 5, 2 * TK + 3, 16, 32
    n = Cout * 3 * Cin
    splits, nbytes = _plan(B, L, Cin, Cout)
    assert splits > 1 and nbytes > 0
    x = torch.ones((B, L, Cin), dtype=torch.float32, device=device)
    dy = torch.ones((B, L, Cout), dtype=torch.float32, device=device)
    buf = torch.full((n + 4,), SENT, dtype=torch.float32, device=device)
    dw = buf[:n]
    wbuf = torch.full((nbytes // 4 + 4,), SENT, dtype=torch.float32, device=device)
    ws = wbuf[:nbytes // 4]
    xo = torch.ones((B * L * Cin + 4,), dtype=torch.float32, device=device)
    dyo = torch.ones((B * L * Cout + 4,), dtype=torch.float32, device=device)
    assert x.data_ptr() % 16 == 0 and xo[1:].data_ptr() % 16 == 4
    big = (2 ** 31) // 1024 + 1                            # L * max(Cin, Cout) > INT_MAX at 1024 channels
    bad = [
        (x, dy, dw, ws, nbytes, B, L, 1, 64), (x, dy, dw, ws, nbytes, B, L, 4, 8),
        (x, dy, dw, ws, nbytes, B, L, 6, 16), (x, dy, dw, ws, nbytes, B, L, 1028, 16),
        (None, dy, dw, ws, nbytes, B, L, Cin, Cout), (x, None, dw, ws, nbytes, B, L, Cin, Cout),
        (x, dy, None, ws, nbytes, B, L, Cin, Cout), (x, dy, dw, None, nbytes, B, L, Cin, Cout),
        (xo[1:], dy, dw, ws, nbytes, B, L, Cin, Cout), (x, dyo[1:], dw, ws, nbytes, B, L, Cin, Cout),
        (x, dy, buf[1:], ws, nbytes, B, L, Cin, Cout), (x, dy, dw, wbuf[1:], nbytes, B, L, Cin, Cout),
        (x, dy, dw, ws, nbytes - 4, B, L, Cin, Cout), (x, dy, dw, ws, 0, B, L, Cin, Cout),
        (x, dy, dw, ws, nbytes, B, 0, Cin, Cout), (x, dy, dw, ws, nbytes, B, -3, Cin, Cout),
        (x, dy, dw, ws, nbytes, -1, L, Cin, Cout),
        (x, dy, dw, None, 0, 0, big, 1024, 16), (x, dy, dw, None, 0, 0, big, 16, 1024),
    ]
    for a in bad:
        assert _call(*a) == INVALID, a[4:]
    torch.cuda.synchronize()
    assert (buf == SENT).all() and (wbuf == SENT).all()
    # an empty batch: zeros, no workspace needed
    assert W.plan(_lib.load(), 0, L, Cin, Cout) == (0, 1, 0)
    assert _call(x, dy, dw, None, 0, 0, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    assert (dw == 0).all() and (buf[n:] == SENT).all() and (wbuf == SENT).all()
    # a single split needs no workspace at all
    assert _plan(1, 1, 4, 16) == (1, 0)
    assert _call(x, dy, dw, ws, nbytes, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    want = W.wgrad_int(np.ones((B, L, Cin)), np.ones((B, L, Cout))).astype(np.float32)
    assert np.array_equal(dw.view(Cout, 3, Cin).cpu().numpy(), want) and (buf[n:] == SENT).all()
