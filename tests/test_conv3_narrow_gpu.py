"""pcgmix_conv3_narrow_nlc_f32 and pcgmix_conv3_narrow_wgrad_nlc_f32 (csrc/pcgmix_conv3_narrow.hip:
Conv1d(k = 3, pad = 1) and its weight gradient at the ten narrow width pairs, on the vector ALU) through
the C ABI against the restatements of tests/conv3_ref.py and tests/conv3_wgrad_ref.py.

Every property runs at all ten pairs and at every (B, L) of the lists below, placed at the edges of the
built kernel's own tiles (TM forward positions, TK weight-gradient positions):

  * integer data: every partial sum is below 2**24, any order is exact in float32, so the result equals
    the int64 restatement BIT FOR BIT — forward, input gradient (the forward on dy with the flipped,
    transposed weights) and weight gradient;
  * the halo: a sample between two samples filled with 1000 keeps zero padding at both ends;
  * outputs (and the workspace) are slices of sentinel-filled buffers: nothing outside is written;
  * random data: |y - float64| <= (3 Cin + 1) 2**-24 sum|x w| (one fmaf chain of 3 Cin terms from +0) and
    |dw - float64| <= (B L + 1) 2**-24 sum|dy x| (the bound of ANY order of summation over B L products);
  * determinism: two launches and a launch on a side stream give the same bits; a sample's y does not
    depend on B or its place in the batch; a workspace pre-filled with NaN or with 1e30 changes nothing;
  * refusals leave the outputs untouched; B == 0 launches nothing (forward) or zeros dw.
"""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import conv3_ref as R
import conv3_wgrad_ref as W

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -1.5e9                        # no result holds it: integer results are below 2**24
GUARD = 256
TM, TK = (int(_lib.load().pcgmix_conv3_narrow_tile(k)) for k in (0, 1))
PAIRS = [(2, 2), (2, 4), (2, 8), (2, 16), (4, 2), (8, 2), (16, 2), (4, 8), (8, 8), (16, 8)]
FWD_BL = [(1, 1), (1, 2), (2, 3), (3, TM - 1), (2, TM), (2, TM + 1), (5, 2 * TM + 3)]
WGRAD_BL = [(1, 1), (1, 2), (3, TK - 1), (2, TK), (2, TK + 1), (5, 2 * TK + 3)]
pairs = pytest.mark.parametrize("Cin,Cout", PAIRS)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------- forward
def _conv3(x, w, y, B, L, Cin, Cout):
    return _lib.load().pcgmix_conv3_narrow_nlc_f32(_ptr(x), _ptr(w), _ptr(y), B, L, Cin, Cout, _stream())


def _fwd(x, w, device):
    """y (B, L, Cout) as numpy, from a slice of a sentinel-filled buffer whose guards stay untouched."""
    B, L, Cin = x.shape
    Cout = w.shape[0]
    n = B * L * Cout
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=device)
    y = buf[GUARD:GUARD + n]
    assert y.data_ptr() % 16 == 0
    assert _conv3(_dev(x, device), _dev(w, device), y, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == np.float32(SENT)).all() and (out[GUARD + n:] == np.float32(SENT)).all()
    return out[GUARD:GUARD + n].reshape(B, L, Cout)


def test_the_shapes_sit_at_the_tile_edges():
    assert TM >= 8 and TK >= 8
    assert {1, TM - 1, TM, TM + 1, 2 * TM + 3} <= {L for _, L in FWD_BL}
    assert {1, TK - 1, TK, TK + 1, 2 * TK + 3} <= {L for _, L in WGRAD_BL}
    lib = _lib.load()
    assert all(lib.pcgmix_conv3_narrow_supported(*p) == 1 and lib.pcgmix_conv3_supported(*p) == 0 for p in PAIRS)


@pairs
def test_forward_integer_data_is_exact_and_stays_inside_y(device, Cin, Cout):
    for B, L in FWD_BL:
        x, w = R.int_case(B, L, Cin, Cout)
        want = R.conv3_int(x, w)
        assert np.abs(want).max() < 2 ** 24
        got = _fwd(x, w, device)
        assert np.array_equal(got.astype(np.int64), want), (B, L)
        assert np.array_equal(got, want.astype(np.float32)), (B, L)


@pairs
def test_forward_halo_is_zero_padding_not_the_neighbour(device, Cin, Cout):
    for _, L in FWD_BL:
        x, w = R.int_case(3, L, Cin, Cout, seed=1)
        w[:] = np.where(w == 0, 1, w)                      # every neighbour value would show
        x[0] = 1000
        x[2] = 1000
        got = _fwd(x, w, device)
        want = R.conv3_int(x[1:2], w)[0]
        assert np.array_equal(got[1, 0], want[0]) and np.array_equal(got[1, L - 1], want[L - 1]), L
        assert np.array_equal(got[1], want), L


@pairs
def test_forward_float_data_within_the_fmaf_chain_bound(device, Cin, Cout, record_property):
    worst = 0.0
    for B, L in FWD_BL:
        rs = np.random.RandomState(3)
        x = rs.standard_normal((B, L, Cin)).astype(np.float32)
        w = rs.standard_normal((Cout, 3, Cin)).astype(np.float32)
        want, mag = R.conv3_f64(x, w)
        got = _fwd(x, w, device)
        bound = (3 * Cin + 1) * 2.0 ** -24 * mag
        err = np.abs(got.astype(np.float64) - want)
        ratio = float((err / bound).max())
        print(f"conv3 narrow float ({B},{L},{Cin},{Cout}): max |err| / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        assert (bound > 0).all() and (err <= bound).all(), (B, L)
    record_property("max_err_over_bound", worst)


@pairs
def test_forward_repeats_side_stream_and_any_batch_give_the_same_bits(device, Cin, Cout):
    for B, L in FWD_BL:
        rs = np.random.RandomState(4)
        x = _dev(rs.standard_normal((B, L, Cin)), device)
        w = _dev(rs.standard_normal((Cout, 3, Cin)), device)
        ys = [torch.full((B, L, Cout), SENT, dtype=torch.float32, device=device) for _ in range(3)]
        for y in ys[:2]:
            assert _conv3(x, w, y, B, L, Cin, Cout) == 0
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            assert _conv3(x, w, ys[2], B, L, Cin, Cout) == 0
        side.synchronize()
        assert torch.isfinite(ys[0]).all()
        assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2]), (B, L)
        if B == 5:                                         # sample 4 of 5, alone
            y4 = torch.full((1, L, Cout), SENT, dtype=torch.float32, device=device)
            assert _conv3(x[4:5].contiguous(), w, y4, 1, L, Cin, Cout) == 0
            torch.cuda.synchronize()
            assert torch.equal(y4[0], ys[0][4])
    assert any(B == 5 for B, _ in FWD_BL)


@pairs
def test_forward_on_flipped_weights_is_the_integer_input_gradient(device, Cin, Cout):
    """(Cin, Cout) as the kernel call takes them: the input gradient of the layer Cout -> Cin, whose
    weights are (Cin, 3, Cout).  dx is restated directly, not through conv3_ref."""
    for B, L in FWD_BL:
        rs = np.random.RandomState(6)
        w = rs.randint(-2, 3, size=(Cin, 3, Cout)).astype(np.int64)         # [o][tap][i] of the layer
        dy = rs.randint(-4, 5, size=(B, L, Cin)).astype(np.int64)
        # dx[b, l, i] = sum over tap, o of dy[b, l - tap + 1, o] * w[o, tap, i]
        dyp = np.zeros((B, L + 2, Cin), dtype=np.int64)
        dyp[:, 1:L + 1] = dy
        want = np.zeros((B, L, Cout), dtype=np.int64)
        for tap in range(3):
            want += dyp[:, 2 - tap:2 - tap + L] @ w[:, tap, :]
        wt = R.flip_transpose(w)
        assert wt.shape == (Cout, 3, Cin) and np.array_equal(R.conv3_int(dy, wt), want)
        got = _fwd(dy, wt, device)
        assert np.array_equal(got, want.astype(np.float32)), (B, L)


@pairs
def test_forward_refusals_leave_y_untouched(device, Cin, Cout):
    B, L = 2, 9
    x = torch.ones((B, L, Cin), dtype=torch.float32, device=device)
    w = torch.ones((Cout, 3, Cin), dtype=torch.float32, device=device)
    buf = torch.full((B * L * 16 + 4,), SENT, dtype=torch.float32, device=device)
    y = buf[:B * L * Cout]
    xo = torch.ones((B * L * 16 + 4,), dtype=torch.float32, device=device)
    wo = torch.ones((16 * 3 * 16 + 4,), dtype=torch.float32, device=device)
    assert x.data_ptr() % 16 == 0 and xo[1:].data_ptr() % 16 == 4 and xo[2:].data_ptr() % 16 == 8
    big = (2 ** 31) // max(Cin, Cout) + 1                  # L * max(Cin, Cout) > INT_MAX
    bad = [
        (x, w, y, B, L, 4, 4), (x, w, y, B, L, 4, 16), (x, w, y, B, L, 16, 16), (x, w, y, B, L, 1, 2),
        (x, w, y, B, L, 2, 3), (x, w, y, B, L, 2, 32), (x, w, y, B, L, 32, 8), (x, w, y, B, L, 0, 8),
        (x, w, y, B, L, -2, 2), (x, w, y, B, L, 1028, 2),
        (None, w, y, B, L, Cin, Cout), (x, None, y, B, L, Cin, Cout), (x, w, None, B, L, Cin, Cout),
        (xo[1:], w, y, B, L, Cin, Cout), (xo[2:], w, y, B, L, Cin, Cout), (x, wo[1:], y, B, L, Cin, Cout),
        (x, wo[2:], y, B, L, Cin, Cout), (x, w, buf[1:], B, L, Cin, Cout), (x, w, buf[2:], B, L, Cin, Cout),
        (x, w, y, B, 0, Cin, Cout), (x, w, y, B, -3, Cin, Cout), (x, w, y, -1, L, Cin, Cout),
        (x, w, y, 0, big, Cin, Cout), (x, w, y, 1, big, Cin, Cout),
        (x, w, y, 2 ** 31 - 1, TM + 1, Cin, Cout),         # more than INT_MAX blocks
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
    assert (buf[B * L * Cout:] == SENT).all()


# --------------------------------------------------------------------------------- weight gradient
def _wgrad(x, dy, dw, ws, nbytes, B, L, Cin, Cout):
    return _lib.load().pcgmix_conv3_narrow_wgrad_nlc_f32(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), nbytes, B, L,
                                                         Cin, Cout, _stream())


def _plan(B, L, Cin, Cout):
    s, n = ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = _lib.load().pcgmix_conv3_narrow_wgrad_plan(B, L, Cin, Cout, ctypes.byref(s), ctypes.byref(n))
    assert rc == 0 and n.value % 16 == 0
    assert n.value == (s.value * Cout * 3 * Cin * 4 if s.value > 1 else 0)
    return int(s.value), int(n.value)


def _batched_case():
    """The smallest B in 1..256 whose plan splits at L = 2 TK + 3 (three K tiles a sample)."""
    L = 2 * TK + 3
    found = [B for B in range(1, 257) if _plan(B, L, 8, 8)[0] >= 2]
    assert found, "no B <= 256 splits at L = 2 TK + 3"
    return found[0], L


def _wgrad_bl():
    return WGRAD_BL + [_batched_case()]


def _run_wgrad(x, dy, device, fill=SENT):
    """dw (Cout, 3, Cin) as numpy; asserts that nothing outside dw and the planned workspace is written
    (GUARD words on either side of both, the word just past the planned bytes among them)."""
    B, L, Cin = x.shape
    Cout = dy.shape[2]
    n = Cout * 3 * Cin
    _, nbytes = _plan(B, L, Cin, Cout)
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=device)
    dw = buf[GUARD:GUARD + n]
    wbuf = torch.full((GUARD + nbytes // 4 + GUARD,), fill, dtype=torch.float32, device=device)
    ws = wbuf[GUARD:GUARD + nbytes // 4] if nbytes else None
    assert dw.data_ptr() % 16 == 0 and (ws is None or ws.data_ptr() % 16 == 0)
    assert _wgrad(_dev(x, device), _dev(dy, device), dw, ws, nbytes, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    out, wout = buf.cpu().numpy(), wbuf.cpu().numpy()
    assert (out[:GUARD] == np.float32(SENT)).all() and (out[GUARD + n:] == np.float32(SENT)).all()
    for edge in (wout[:GUARD], wout[GUARD + nbytes // 4:]):
        assert np.array_equal(_bits(edge), _bits(np.full(GUARD, fill, np.float32)))
    return out[GUARD:GUARD + n].reshape(Cout, 3, Cin)


def test_the_weight_gradient_shapes_hold_one_split_and_a_ragged_split():
    B, L = _batched_case()
    assert 1 <= B <= 256
    splits = {bl: _plan(*bl, 8, 8)[0] for bl in _wgrad_bl()}
    assert min(splits.values()) == 1 and max(splits.values()) > 1
    units = 5 * 3
    assert splits[(5, 2 * TK + 3)] > 1 and units % splits[(5, 2 * TK + 3)] != 0


@pairs
def test_wgrad_integer_data_is_exact_and_stays_inside_dw_and_the_workspace(device, Cin, Cout):
    for B, L in _wgrad_bl():
        x, dy = W.int_case(B, L, Cin, Cout)
        want = W.wgrad_int(x, dy)
        assert 8 * B * L < 2 ** 24
        got = _run_wgrad(x, dy, device)
        assert np.array_equal(got.astype(np.int64), want), (B, L)
        assert np.array_equal(got, want.astype(np.float32)), (B, L)


@pairs
def test_wgrad_halo_is_zero_padding_not_the_neighbour(device, Cin, Cout):
    for _, L in WGRAD_BL:
        x, dy = W.int_case(3, L, Cin, Cout, seed=1)
        dy[1] = np.where(dy[1] == 0, 1, dy[1])             # every neighbour value would show
        x[0] = 1000
        x[2] = 1000
        dy[0] = 0
        dy[2] = 0
        want = W.wgrad_int(x[1:2], dy[1:2])
        assert np.array_equal(want, W.wgrad_int(x, dy))
        assert np.array_equal(_run_wgrad(x, dy, device), want.astype(np.float32)), L


@pairs
def test_wgrad_workspace_is_never_read_before_it_is_written(device, Cin, Cout):
    split = 0
    for B, L in _wgrad_bl():
        rs = np.random.RandomState(5)
        x = rs.standard_normal((B, L, Cin)).astype(np.float32)
        dy = rs.standard_normal((B, L, Cout)).astype(np.float32)
        a = _run_wgrad(x, dy, device, fill=float("nan"))
        b = _run_wgrad(x, dy, device, fill=1e30)
        assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(b)), (B, L)
        split += int(_plan(B, L, Cin, Cout)[0] > 1)
    assert split >= 2


@pairs
def test_wgrad_float_data_within_the_bound_of_any_order(device, Cin, Cout, record_property):
    worst = 0.0
    for B, L in _wgrad_bl():
        rs = np.random.RandomState(3)
        x = rs.standard_normal((B, L, Cin)).astype(np.float32)
        dy = rs.standard_normal((B, L, Cout)).astype(np.float32)
        want, mag = W.wgrad_f64(x, dy)
        got = _run_wgrad(x, dy, device)
        bound = (B * L + 1) * 2.0 ** -24 * mag
        err = np.abs(got.astype(np.float64) - want)
        live = bound > 0                                   # L = 1: taps 0 and 2 see only padding, exact zeros
        ratio = float((err[live] / bound[live]).max())
        print(f"conv3 narrow wgrad float ({B},{L},{Cin},{Cout}): max |err| / bound = {ratio:.5f}")
        worst = max(worst, ratio)
        assert (err <= bound).all() and ratio <= 1.0, (B, L)
    record_property("max_err_over_bound", worst)


@pairs
def test_wgrad_repeats_and_a_side_stream_give_the_same_bits(device, Cin, Cout):
    for B, L in _wgrad_bl():
        rs = np.random.RandomState(4)
        x = _dev(rs.standard_normal((B, L, Cin)), device)
        dy = _dev(rs.standard_normal((B, L, Cout)), device)
        _, nbytes = _plan(B, L, Cin, Cout)
        outs = [torch.full((Cout, 3, Cin), SENT, dtype=torch.float32, device=device) for _ in range(3)]
        wss = [torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None for _ in range(3)]
        for dw, ws in zip(outs[:2], wss[:2]):
            assert _wgrad(x, dy, dw, ws, nbytes, B, L, Cin, Cout) == 0
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            assert _wgrad(x, dy, outs[2], wss[2], nbytes, B, L, Cin, Cout) == 0
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (B, L)


@pairs
def test_wgrad_refusals_leave_dw_and_the_workspace_untouched(device, Cin, Cout):
    B, L = 5, 2 * TK + 3
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
    assert x.data_ptr() % 16 == 0 and xo[1:].data_ptr() % 16 == 4 and xo[2:].data_ptr() % 16 == 8
    big = (2 ** 31) // max(Cin, Cout) + 1                  # L * max(Cin, Cout) > INT_MAX
    bad = [
        (x, dy, dw, ws, nbytes, B, L, 4, 4), (x, dy, dw, ws, nbytes, B, L, 4, 16),
        (x, dy, dw, ws, nbytes, B, L, 16, 16), (x, dy, dw, ws, nbytes, B, L, 1, 2),
        (x, dy, dw, ws, nbytes, B, L, 2, 32), (x, dy, dw, ws, nbytes, B, L, 32, 8),
        (x, dy, dw, ws, nbytes, B, L, 0, 8), (x, dy, dw, ws, nbytes, B, L, 1028, 2),
        (None, dy, dw, ws, nbytes, B, L, Cin, Cout), (x, None, dw, ws, nbytes, B, L, Cin, Cout),
        (x, dy, None, ws, nbytes, B, L, Cin, Cout), (x, dy, dw, None, nbytes, B, L, Cin, Cout),
        (xo[1:], dy, dw, ws, nbytes, B, L, Cin, Cout), (xo[2:], dy, dw, ws, nbytes, B, L, Cin, Cout),
        (x, dyo[1:], dw, ws, nbytes, B, L, Cin, Cout), (x, dyo[2:], dw, ws, nbytes, B, L, Cin, Cout),
        (x, dy, buf[1:], ws, nbytes, B, L, Cin, Cout), (x, dy, dw, wbuf[1:], nbytes, B, L, Cin, Cout),
        (x, dy, dw, wbuf[2:], nbytes, B, L, Cin, Cout),
        (x, dy, dw, ws, nbytes - 4, B, L, Cin, Cout), (x, dy, dw, ws, 0, B, L, Cin, Cout),
        (x, dy, dw, ws, nbytes, B, 0, Cin, Cout), (x, dy, dw, ws, nbytes, B, -3, Cin, Cout),
        (x, dy, dw, ws, nbytes, -1, L, Cin, Cout),
        (x, dy, dw, None, 0, 0, big, Cin, Cout),
    ]
    for a in bad:
        assert _wgrad(*a) == INVALID, a[4:]
    torch.cuda.synchronize()
    assert (buf == SENT).all() and (wbuf == SENT).all()
    # an empty batch: zeros, no workspace needed
    assert _plan(0, L, Cin, Cout) == (1, 0)
    assert _wgrad(x, dy, dw, None, 0, 0, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    assert (dw == 0).all() and (buf[n:] == SENT).all() and (wbuf == SENT).all()
    # a single split needs no workspace at all
    assert _plan(1, 1, Cin, Cout) == (1, 0)
    assert _wgrad(x, dy, dw, ws, nbytes, B, L, Cin, Cout) == 0
    torch.cuda.synchronize()
    want = W.wgrad_int(np.ones((B, L, Cin)), np.ones((B, L, Cout))).astype(np.float32)
    assert np.array_equal(dw.view(Cout, 3, Cin).cpu().numpy(), want) and (buf[n:] == SENT).all()
    assert (wbuf[nbytes // 4:] == SENT).all()
