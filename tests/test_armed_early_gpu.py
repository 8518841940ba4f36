"""The armed plain kernel's early phase (csrc/pcgmix_kernels.h EdgePack; include/pcgmix_hip.h
pcgmix_augment_plain_begin_edges): what lies outside a sample's own cycle [frames[b,0], frames[b,4]) is
a copy of the own row whatever partner is drawn, so the kernel stores it — and loads the rest of its own
rows — before the records arrive.  Every element must still be written exactly once and every result
must stay what it was: all comparisons here are exact, against the two-launch path (host labels) and
against the CPU oracle, on boundaries the synthetic generator never makes."""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, augmentations, augmentations2d, hostprep
from conftest import Args, StepCounter
from oracle import pcgmix_oracle as O

pytestmark = pytest.mark.gpu

METHOD = "durratiomixup"


def odd_batch(B, C, T, seed, classes=2):
    """Random rows (nothing is zero outside the cycle, so a misplaced copy shows) and boundaries by sample
    index: cycle up to the row's end | empty cycle | odd edges | a zero-length state | a cycle of a few
    samples | anything monotone.  Starts are > 0 and edges are not multiples of 4 wherever T allows."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, C, T)).astype(np.float32)
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
    assert (np.diff(frames, axis=1) >= 0).all() and frames.min() >= 0 and frames.max() <= T
    labels = rs.randint(0, classes, B).astype(np.int64)
    wav = ["a%04d" % i for i in range(B)]
    return x, frames, labels, wav


def _step(mod, data, labels, frames, wav, step, device, host_labels=None, classes=None):
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), classes or int(labels.max()) + 1).to(device)
    return mod.augment(Args(METHOD), data, tgt, torch.from_numpy(frames), wav, StepCounter(step), None,
                       device, "", host_labels=host_labels)


def _stats(device):
    out = (ctypes.c_longlong * 3)()
    _lib.check(_lib.load().pcgmix_ctx_armed_stats(augmentations.step_context(device.index), out), "stats")
    return list(out)


# (256, 4, 12000): six blocks per sample, four chunks each — more than a lane holds across the wait;
# (256, 4, 32764): eight chunks per block
SHAPES = [(B, C, T) for T in (8, 128, 5000, 32764) for C in (1, 4) for B in (1, 7, 200, 256)] + [(256, 4, 12000)]


@pytest.mark.parametrize("B,C,T", SHAPES)
def test_odd_boundaries_equal_two_launch_path_and_oracle(B, C, T, device):
    x, frames, labels, wav = odd_batch(B, C, T, seed=B + C + T)
    data = torch.from_numpy(x).to(device)
    before = _stats(device)
    for step in (2, 19):
        ref = O.augment(METHOD, x, labels, frames, wav, step)        # the reference takes these boundaries
        y_a, _, mix_a, _ = _step(augmentations, data, labels, frames, wav, step, device, classes=2)
        y_h, _, mix_h, _ = _step(augmentations, data, labels, frames, wav, step, device, host_labels=labels,
                                 classes=2)
        assert np.array_equal(mix_a, mix_h) and torch.equal(y_a, y_h)
        assert np.array_equal(mix_a, ref["mix"]) and np.array_equal(y_a.cpu().numpy(), ref["y"])
    after = _stats(device)
    assert after[0] - before[0] == 2 and after[2] == before[2], "not the armed kernel, or it gave up"


def test_spectrogram_shape_with_odd_boundaries(device):
    B, F, W = 256, 128, 128
    x, frames, labels, wav = odd_batch(B, F, W, seed=77)
    data = torch.from_numpy(x.reshape(B, 1, F, W)).to(device)
    before = _stats(device)
    y_a, _, mix_a, _ = _step(augmentations2d, data, labels, frames, wav, 9, device, classes=2)
    y_h, _, mix_h, _ = _step(augmentations2d, data, labels, frames, wav, 9, device, host_labels=labels, classes=2)
    assert np.array_equal(mix_a, mix_h) and torch.equal(y_a, y_h) and not torch.equal(y_a, data)
    ref = O.augment(METHOD, x.reshape(B, 1, F, W), labels, frames, wav, 9)
    assert np.array_equal(mix_a, ref["mix"]) and np.array_equal(y_a.cpu().numpy(), ref["y"])
    assert _stats(device)[0] - before[0] == 1


@pytest.mark.parametrize("B,C,T", [(256, 4, 5000), (200, 1, 128), (7, 4, 8), (256, 4, 12000)])
def test_every_element_is_written(B, C, T, device):
    """The output buffer comes in full of NaN: none is left, and the result is the oracle's."""
    x, frames, labels, wav = odd_batch(B, C, T, seed=3 * B + T)
    data = torch.from_numpy(x).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(device)
    out = torch.full_like(data, float("nan"))
    before = _stats(device)
    y, mix = augmentations.splice_plain(hostprep.plain_recipe(METHOD, False), data, None, torch.from_numpy(frames),
                                        5, out=out, target_ohe=tgt)
    assert y.data_ptr() == out.data_ptr() and not torch.isnan(out).any()
    ref = O.augment(METHOD, x, labels, frames, wav, 5)
    assert np.array_equal(np.asarray(mix), ref["mix"]) and np.array_equal(out.cpu().numpy(), ref["y"])
    assert _stats(device)[0] - before[0] == 1


@pytest.mark.parametrize("classes", [3, 17, 256])
def test_partners_for_many_classes(classes, device):
    B, C, T = 256, 4, 5000
    x, frames, labels, wav = odd_batch(B, C, T, seed=classes, classes=classes)
    data = torch.from_numpy(x).to(device)
    for step in (0, 7):
        y_a, _, mix_a, _ = _step(augmentations, data, labels, frames, wav, step, device, classes=classes)
        assert np.array_equal(mix_a, hostprep.shuffle_within_groups(labels, step))
        y_h, _, mix_h, _ = _step(augmentations, data, labels, frames, wav, step, device, host_labels=labels,
                                 classes=classes)
        assert np.array_equal(mix_a, mix_h) and torch.equal(y_a, y_h)


def _two_calls(begin_frames, frames, data, tgt, step, device):
    """begin (without boundaries: begin_frames is None, or with these) + finish, as the binding makes them."""
    lib = _lib.load()
    ctx = augmentations.step_context(device.index)
    B, C, T = data.shape
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    out = torch.full_like(data, float("nan"))
    if begin_frames is None:
        err = lib.pcgmix_augment_plain_begin(ctx, data.data_ptr(), out.data_ptr(), tgt.data_ptr(), tgt.shape[1],
                                             B, C, T, st)
    else:
        err = lib.pcgmix_augment_plain_begin_edges(ctx, data.data_ptr(), out.data_ptr(), tgt.data_ptr(),
                                                   tgt.shape[1], B, C, T, begin_frames.ctypes.data, st)
    assert err == 0
    _name, _p, alpha, sigma, _n = hostprep.plain_recipe(METHOD, False)
    lam, _ = hostprep.draw_lambda_knots(step, alpha, sigma, 0)
    mix = np.empty(B, dtype=np.int64)
    assert lib.pcgmix_augment_plain_finish(ctx, frames.ctypes.data, step, ctypes.c_float(lam), mix.ctypes.data) == 0
    return out, mix


def test_begin_without_boundaries_still_exact(device):
    B, C, T = 256, 4, 5000
    x, frames, labels, wav = odd_batch(B, C, T, seed=31)
    data = torch.from_numpy(x).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(device)
    out, mix = _two_calls(None, frames, data, tgt, 4, device)
    ref = O.augment(METHOD, x, labels, frames, wav, 4)
    assert np.array_equal(mix, ref["mix"]) and np.array_equal(out.cpu().numpy(), ref["y"])


def test_finish_with_other_boundaries_than_begin(device):
    """Cycles that reach outside the ones the kernel was launched with: the library gives the kernel up
    and runs the step unarmed; narrower ones go through the armed kernel.  Same result either way."""
    B, C, T = 200, 4, 5000
    x, frames, labels, wav = odd_batch(B, C, T, seed=32)
    _, other, _, _ = odd_batch(B, C, T, seed=33)
    data = torch.from_numpy(x).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(device)
    ref = O.augment(METHOD, x, labels, frames, wav, 6)
    before = _stats(device)
    out, mix = _two_calls(other, frames, data, tgt, 6, device)
    assert np.array_equal(mix, ref["mix"]) and np.array_equal(out.cpu().numpy(), ref["y"])
    assert _stats(device)[2] - before[2] == 1
    wide = frames.copy()
    wide[:, 0], wide[:, 4] = 0, T
    wide[:, 1:4] = np.clip(wide[:, 1:4], 0, T)
    out, mix = _two_calls(wide, frames, data, tgt, 6, device)
    assert np.array_equal(mix, ref["mix"]) and np.array_equal(out.cpu().numpy(), ref["y"])
    assert _stats(device)[2] - before[2] == 1


def test_step_after_an_abort_into_the_same_buffer(device):
    """Malformed boundaries are refused after the launch: the released kernel has stored part of the
    buffer by then.  The next step into the same buffer is exact."""
    B, C, T = 64, 4, 5000
    x, frames, labels, wav = odd_batch(B, C, T, seed=8)
    data = torch.from_numpy(x).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(device)
    recipe = hostprep.plain_recipe(METHOD, False)
    bad = frames.copy()
    bad[3, 4] = T + 1
    out = torch.full_like(data, float("nan"))
    with pytest.raises(ValueError):
        augmentations.splice_plain(recipe, data, None, torch.from_numpy(bad), 2, out=out, target_ohe=tgt)
    torch.cuda.synchronize()                   # returns: nobody is waiting any more
    y, mix = augmentations.splice_plain(recipe, data, None, torch.from_numpy(frames), 2, out=out, target_ohe=tgt)
    ref = O.augment(METHOD, x, labels, frames, wav, 2)
    assert np.array_equal(np.asarray(mix), ref["mix"]) and np.array_equal(out.cpu().numpy(), ref["y"])
