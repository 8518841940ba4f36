"""The armed plain kernel as one wide block per sample slice (csrc/pcgmix_mix.hip mix_armed_kernel): wave 0 of
every block polls its sample's record and hands it to the block through LDS; a block holds kArmedHold quads
per lane across the wait and covers 4,096 elements per quad row.  Through the C ABI, into an output full of
NaN, at the planes where a block's reach ends (one quad row, the U = 1 / U = 2 switch, two, four, five and six
held rows, and one element past them), compared bit for bit with the two-launch path (host labels) and with
the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, augmentations, hostprep
from oracle import pcgmix_oracle as O

pytestmark = pytest.mark.gpu

METHOD = "durratiomixup"
_NAME, _P, ALPHA, SIGMA, _N = hostprep.plain_recipe(METHOD, False)

PLANES = [4092, 4096, 4100, 8188, 8192, 8196, 16380, 16384, 16388, 20476, 20480, 20484, 24580]
SHAPES = [(3, 1, T, 2) for T in PLANES] + [(3, 3, 6828, 2), (1, 4, 5000, 2), (256, 1, 8, 2), (5, 1, 64, 3)]


def _rows(B, C, T, seed, classes):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, C, T)).astype(np.float32)       # nothing is zero: a misplaced copy shows
    labels = rs.randint(0, classes, B).astype(np.int64)
    return rs, x, labels, ["a%04d" % i for i in range(B)]


def _odd_frames(rs, B, T):
    """Per sample index: cycle up to the row's end | empty cycle | odd edges | a zero-length state | a short
    cycle | anything monotone; starts > 0 and edges off the multiples of 4 wherever T allows."""
    frames = np.empty((B, 5), np.int64)
    for b in range(B):
        kind = b % 6
        lo = int(rs.randint(1, T // 3 + 1))
        hi = int(rs.randint(lo, T + 1))
        if kind == 0:
            hi = T
        elif kind == 1:
            hi = lo
        elif kind == 2:
            lo |= 1
            hi = max(lo, hi)
            hi += 1 if hi % 4 == 0 and hi < T else 0
        elif kind == 4:
            hi = min(T, lo + int(rs.randint(1, 7)))
        cuts = np.sort(rs.randint(lo, hi + 1, 3))
        if kind == 3:
            cuts[1] = cuts[0]
        frames[b] = [lo, cuts[0], cuts[1], cuts[2], hi]
    return frames


def _boundary_frames(kind, rs, B, T):
    frames = np.empty((B, 5), np.int64)
    for b in range(B):
        if kind == "empty":                                     # an empty cycle at an odd position
            lo = min(T, int(rs.randint(0, T + 1)) | 1)
            frames[b] = [lo] * 5
        elif kind == "whole":                                   # [0, T): nothing is final before the record
            cuts = np.sort(np.minimum(rs.randint(1, T, 3) | 1, T))
            frames[b] = [0, cuts[0], cuts[1], cuts[2], T]
        else:                                                   # [T - 4, T): the row's last quad
            frames[b] = [T - 4, T - 3, T - 2, T - 1, T] if b % 2 == 0 else [T - 4, T - 4, T - 1, T - 1, T]
    return frames


def _check_frames(frames, T):
    assert (np.diff(frames, axis=1) >= 0).all() and frames.min() >= 0 and frames.max() <= T


def _ctx_stream(device):
    return (_lib.load(), augmentations.step_context(device.index),
            ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))


def _lam(step):
    lam, _ = hostprep.draw_lambda_knots(step, ALPHA, SIGMA, 0)
    return ctypes.c_float(lam)


def _armed(device, data, tgt, frames, step, begin_frames="same", out=None):
    """begin_edges (or begin without boundaries) + finish into a NaN-filled output, as the binding calls them."""
    lib, ctx, st = _ctx_stream(device)
    B, C, T = data.shape
    out = torch.full_like(data, float("nan")) if out is None else out
    fr = frames.ctypes.data if begin_frames == "same" else None
    err = lib.pcgmix_augment_plain_begin_edges(ctx, data.data_ptr(), out.data_ptr(), tgt.data_ptr(), tgt.shape[1],
                                               B, C, T, fr, st)
    assert err == 0, "not armed: %d" % err
    mix = np.empty(B, dtype=np.int64)
    assert lib.pcgmix_augment_plain_finish(ctx, frames.ctypes.data, step, _lam(step), mix.ctypes.data) == 0
    return out, mix


def _two_launch(device, data, labels, frames, step):
    """pcgmix_augment_plain_f32 with host labels: label pick-up on the host, then the unarmed splice launch."""
    lib, ctx, st = _ctx_stream(device)
    B, C, T = data.shape
    out = torch.full_like(data, float("nan"))
    mix = np.empty(B, dtype=np.int64)
    err = lib.pcgmix_augment_plain_f32(ctx, data.data_ptr(), out.data_ptr(), None, 0, labels.ctypes.data,
                                       frames.ctypes.data, step, _lam(step), None, 0, mix.ctypes.data, B, C, T, st)
    assert err == 0
    return out, mix


def _stats(device):
    lib, ctx, _ = _ctx_stream(device)
    out = (ctypes.c_longlong * 3)()
    _lib.check(lib.pcgmix_ctx_armed_stats(ctx, out), "stats")
    return list(out)


def _compare(device, x, labels, frames, wav, step, classes, begin_frames="same"):
    data = torch.from_numpy(x).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), classes).to(device)
    before = _stats(device)
    y_a, mix_a = _armed(device, data, tgt, frames, step, begin_frames)
    after = _stats(device)
    y_h, mix_h = _two_launch(device, data, labels, frames, step)
    assert after[0] - before[0] == 1 and after[2] == before[2], "not the armed kernel, or it gave up"
    got = y_a.cpu().numpy()
    assert not np.isnan(got).any(), "an element was never stored"
    assert np.array_equal(mix_a, mix_h) and torch.equal(y_a, y_h)
    ref = O.augment(METHOD, x, labels, frames, wav, step, num_classes=classes)
    assert np.array_equal(mix_a, ref["mix"])
    assert np.abs(got - ref["y"]).max() <= 1e-4


@pytest.mark.parametrize("B,C,T,classes", SHAPES)
def test_block_reach_equals_two_launch_path_and_oracle(B, C, T, classes, device):
    rs, x, labels, wav = _rows(B, C, T, B + C + T, classes)
    frames = _odd_frames(rs, B, T)
    _check_frames(frames, T)
    _compare(device, x, labels, frames, wav, 5, classes)


@pytest.mark.parametrize("kind", ["empty", "whole", "last quad"])
@pytest.mark.parametrize("B,C,T,classes", [(3, 1, 20480, 2), (3, 1, 24580, 2), (3, 3, 6828, 2), (256, 1, 8, 2),
                                           (5, 1, 64, 3)])
def test_cycle_boundaries(B, C, T, classes, kind, device):
    rs, x, labels, wav = _rows(B, C, T, 7 * B + T, classes)
    frames = _boundary_frames(kind, rs, B, T)
    _check_frames(frames, T)
    _compare(device, x, labels, frames, wav, 11, classes)


def test_begin_without_boundaries(device):
    B, C, T = 3, 1, 20484
    rs, x, labels, wav = _rows(B, C, T, 41, 2)
    _compare(device, x, labels, _odd_frames(rs, B, T), wav, 4, 2, begin_frames=None)


def test_step_into_the_same_buffer_after_an_abort(device):
    """An aborted begin leaves the buffer partly written (the early phase); the next step into it is exact."""
    B, C, T = 3, 1, 20484
    rs, x, labels, wav = _rows(B, C, T, 43, 2)
    frames = _odd_frames(rs, B, T)
    data = torch.from_numpy(x).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(device)
    lib, ctx, st = _ctx_stream(device)
    out = torch.full_like(data, float("nan"))
    before = _stats(device)
    assert lib.pcgmix_augment_plain_begin_edges(ctx, data.data_ptr(), out.data_ptr(), tgt.data_ptr(), 2, B, C, T,
                                                frames.ctypes.data, st) == 0
    assert lib.pcgmix_augment_plain_abort(ctx) == 0
    torch.cuda.synchronize()                   # returns: nobody is waiting any more
    assert _stats(device)[2] - before[2] == 1
    y, mix = _armed(device, data, tgt, frames, 2, out=out)
    ref = O.augment(METHOD, x, labels, frames, wav, 2)
    got = y.cpu().numpy()
    assert y.data_ptr() == out.data_ptr() and not np.isnan(got).any()
    assert np.array_equal(mix, ref["mix"]) and np.abs(got - ref["y"]).max() <= 1e-4
    y_h, mix_h = _two_launch(device, data, labels, frames, 2)
    assert np.array_equal(mix, mix_h) and torch.equal(y, y_h)
