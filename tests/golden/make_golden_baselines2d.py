#!/usr/bin/env python3
"""Golden vectors of the paper's spectrogram comparison baselines, recorded by RUNNING the reference.

Run in the build container only (needs the reference checkout, see _ref_import.py):

    python tests/golden/make_golden_baselines2d.py

The reference's own ``augmentations2d.augment`` is called on small synthetic (B, C, F, W) batches for
timemask, freqmask, mixup(same), mixup(mix), cutmix, (rand)cutmix, durratiocutmix,
(rand)durratiocutmix and latentmixup.  Files are named ``base2d_*.npz`` (a prefix none of the other
golden globs match).  Recorded per case:

  x                    the input, cloned BEFORE the call (timemask and freqmask zero it in place)
  frames, labels       the other inputs (state boundaries in spectrogram columns)
  method, step         args.method, step_counter.count
  fired                1 if the probability gate let the method run
  raised               1 if the reference raised (a shape error); y etc. are then empty
  same_object          1 if augment() returned the very input tensor
  y, target_out, mix   augment()'s outputs (mix: [] -> empty array)
  cut                  augment()'s fourth return value (None -> -1)
  lam                  get_lambda's value (when called)
  depth                args.depth after the call (latentmixup's mixing depth; 0 otherwise)
  probe_cl             latentmixup: 1 if the probe model returned channels-last features
  np_before, np_after  numpy's global MT19937 state around the call: key (624 uint32), then
                       pos, has_gauss and the cached Gaussian in np_*_tail

latentmixup runs on ``ProbeNet``, a stand-in for ResNet9-2D's first half (whose weights are far too
large to commit) that is exact in fp32 on any device; tests/test_baselines2d_gpu.py defines the same
network.
"""
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import StepCounter, base_args  # noqa: E402  (also puts the repo on sys.path)
from _ref_import import import_reference  # noqa: E402


class ProbeNet(torch.nn.Module):
    """``forward(x, depth, pass_part='first')`` with ResNet9-2D's ranks — 4D features at depths 1
    and 2, (B, n) at depth 3 — from strided subsampling, channel repetition and multiplication by
    powers of two only, so every value is exact in fp32 on any device."""

    def __init__(self, channels_last=False):
        super().__init__()
        self.channels_last = channels_last

    def _layout(self, h):
        return h.contiguous(memory_format=torch.channels_last) if self.channels_last else h.contiguous()

    def forward(self, x, depth=None, pass_part=None):
        assert pass_part == "first" and depth in (1, 2, 3)
        h = self._layout(x[:, :, ::2, ::2].repeat(1, 3, 1, 1) * 2.0)
        if depth == 1:
            return h
        h = self._layout(h[:, :, 1::2, ::2].repeat(1, 2, 1, 1) * 0.25)
        if depth == 2:
            return h
        return h.flatten(1) * 4.0


def np_state():
    _, key, pos, has_gauss, cached = np.random.get_state()
    return np.asarray(key, dtype=np.uint32).copy(), np.array([pos, has_gauss, cached], dtype=np.float64)


def make_frames(rs, B, W, max_cut2=None):
    """int64 (B, 5) cumulative boundaries, the cycle inside W columns (and f[2] <= max_cut2)."""
    out = np.zeros((B, 5), dtype=np.int64)
    for b in range(B):
        while True:
            lens = np.array([rs.randint(1, W // 8 + 2), rs.randint(1, W // 4 + 2), rs.randint(1, W // 8 + 2),
                             rs.randint(1, W // 3 + 2)])
            f = np.concatenate([[0], np.cumsum(lens)])
            if f[4] <= W and (max_cut2 is None or f[2] <= max_cut2):
                out[b] = f
                break
    return out


def make_batch(seed, B, C, F, W, max_cut2=None, min_cut2=None):
    rs = np.random.RandomState(seed)
    frames = make_frames(rs, B, W, max_cut2)
    if min_cut2 is not None:
        frames[0] = [0, 6, min_cut2, min_cut2 + 3, min(W, min_cut2 + 10)]
    x = rs.standard_normal((B, C, F, W)).astype(np.float32)
    x[np.broadcast_to(np.arange(W)[None, None, None, :] >= frames[:, 4][:, None, None, None], x.shape)] = 0
    labels = rs.randint(0, 2, size=B).astype(np.int64)
    labels[:2] = (0, 1)
    return x, frames, labels


def run_case(aug, x, frames, labels, method, step, np_seed, tmp, probe_cl=False):
    rec = {"lam": np.nan}
    data = torch.from_numpy(x.copy())
    target_ohe = torch.nn.functional.one_hot(torch.from_numpy(labels), 2)
    args = base_args(method, x.shape[1], x.shape[0], tmp, model="resnet9")
    args.dataset = "PhysioNet(spec128)"
    orig_get_lambda = aug.get_lambda

    def get_lambda(*a, **k):
        rec["lam"] = float(orig_get_lambda(*a, **k))
        return rec["lam"]

    np.random.seed(np_seed)
    np.random.normal(size=np_seed % 5)   # (an odd count leaves numpy's Gaussian cache full)
    before = np_state()
    py_before = random.getstate()
    aug.get_lambda = get_lambda
    raised = 0
    try:
        y, t_out, mix, cut = aug.augment(args, data, target_ohe, torch.from_numpy(frames.copy()), None,
                                         StepCounter(step), ProbeNet(probe_cl), torch.device("cpu"), tmp)
    except RuntimeError:
        raised = 1
    finally:
        aug.get_lambda = orig_get_lambda
    after = np_state()
    assert random.getstate() == py_before
    p = float(method.split("+")[-1]) if "+" in method else 1.0
    out = {
        "x": x, "frames": frames, "labels": labels,
        "method": np.array(method), "step": np.int64(step),
        "fired": np.int64(random.Random(step).uniform(0, 1) < p), "raised": np.int64(raised),
        "np_before": before[0], "np_before_tail": before[1],
        "np_after": after[0], "np_after_tail": after[1],
        "lam": np.float64(rec["lam"]), "depth": np.int64(args.depth), "probe_cl": np.int64(probe_cl),
    }
    if raised:
        out.update(same_object=np.int64(0), y=np.zeros((0,), np.float32), mix=np.zeros((0,), np.int64),
                   target_out=np.zeros((0,), np.float32), cut=np.int64(-1))
    else:
        out.update(same_object=np.int64(y is data), y=y.detach().numpy().astype(np.float32).copy(),
                   mix=np.asarray(mix, dtype=np.int64), target_out=t_out.detach().numpy().copy(),
                   cut=np.int64(-1 if cut is None else cut))
    return out


def steps_covering(fn, values, start):
    """The first steps from ``start`` on whose draw ``fn(step)`` takes every one of ``values``."""
    out, seen, s = [], set(), start
    while seen != set(values):
        v = fn(s)
        if v not in seen:
            seen.add(v)
            out.append(s)
        s += 1
    return out


def main():
    ref = import_reference()
    tmp = tempfile.mkdtemp(prefix="pcgmix_golden2d_")
    batches = {
        "s6x1x32x32": make_batch(31, 6, 1, 32, 32),
        "q8x2x32x32": make_batch(32, 8, 2, 32, 32),
        "t6x1x40x32": make_batch(33, 6, 1, 40, 32),      # F > W: cutmix's new tensor is (F, F)
        "w5x2x24x40": make_batch(34, 5, 2, 24, 40, max_cut2=24),   # F < W, every cut at 2 fits
        "z4x1x16x40": make_batch(35, 4, 1, 16, 40, min_cut2=20),   # F < W, a cut beyond F: raises
    }
    rand_cut_steps = steps_covering(lambda s: random.Random(s * 131071).randint(1, 3), (1, 2, 3), 40)
    depth_steps = steps_covering(lambda s: random.Random(s).randint(1, 3), (1, 2, 3), 60)
    cases = [
        # timemask: default 0.2, 0.1 (the paper's row), a clamped maximum, F != W, the gate
        ("s6x1x32x32", "timemask", 3), ("q8x2x32x32", "timemask(0.1)", 4),
        ("w5x2x24x40", "timemask(1.5)", 5), ("t6x1x40x32", "timemask(0.3)", 6),
        ("s6x1x32x32", "timemask(0.1)+0.5", 1), ("s6x1x32x32", "timemask(0.1)+0.5", 2),
        # freqmask
        ("s6x1x32x32", "freqmask", 7), ("q8x2x32x32", "freqmask(0.1)", 8),
        ("w5x2x24x40", "freqmask(0.5)", 9), ("t6x1x40x32", "freqmask(0.9)", 10),
        ("q8x2x32x32", "freqmask(0.1)+0.5", 1), ("q8x2x32x32", "freqmask(0.1)+0.5", 2),
        # mixup: same label, all labels, F != W, the gate
        ("s6x1x32x32", "mixup(same)", 11), ("q8x2x32x32", "mixup(same)", 12),
        ("s6x1x32x32", "mixup(mix)", 13), ("w5x2x24x40", "mixup(mix)", 14),
        ("q8x2x32x32", "mixup(same)+0.5", 1), ("q8x2x32x32", "mixup(same)+0.5", 2),
        # cutmix: F == W, C = 2, F > W (the F cap), F < W, the gate, a cut beyond F
        ("s6x1x32x32", "cutmix", 15), ("q8x2x32x32", "cutmix", 16), ("t6x1x40x32", "cutmix", 17),
        ("w5x2x24x40", "cutmix", 18), ("s6x1x32x32", "cutmix+0.5", 1), ("s6x1x32x32", "cutmix+0.5", 2),
        ("z4x1x16x40", "cutmix", 19),
    ] + [("q8x2x32x32", "(rand)cutmix", s) for s in rand_cut_steps] + [
        ("t6x1x40x32", "(rand)cutmix", rand_cut_steps[0]),
        # durratiocutmix: plain, '(rand)' (frequency rows), the gate, W != F (raises)
        ("s6x1x32x32", "durratiocutmix", 20), ("q8x2x32x32", "durratiocutmix", 21),
        ("s6x1x32x32", "(rand)durratiocutmix", 22), ("s6x1x32x32", "(rand)durratiocutmix", 23),
        ("q8x2x32x32", "(rand)durratiocutmix", 24), ("q8x2x32x32", "(rand)durratiocutmix", 25),
        ("s6x1x32x32", "durratiocutmix+0.5", 1), ("s6x1x32x32", "durratiocutmix+0.5", 2),
        ("w5x2x24x40", "durratiocutmix", 26), ("t6x1x40x32", "(rand)durratiocutmix", 27),
    ] + [("q8x2x32x32", "latentmixup", s) for s in depth_steps] + [
        ("s6x1x32x32", "latentmixup", depth_steps[0]),
        ("s6x1x32x32", "latentmixup+0.5", 1), ("s6x1x32x32", "latentmixup+0.5", 2),
    ]
    for i, (tag, method, step) in enumerate(cases):
        x, frames, labels = batches[tag]
        case = run_case(ref.augmentations2d, x, frames, labels, method, step, 200 + i, tmp,
                        probe_cl=(method == "latentmixup" and i % 2 == 1))
        name = f"base2d_{tag}_{i:02d}"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **case)
        print(f"{name:26s} {method:24s} {os.path.getsize(path) / 1024:6.1f} KiB  fired={int(case['fired'])} "
              f"raised={int(case['raised'])} cut={int(case['cut'])} depth={int(case['depth'])}")


if __name__ == "__main__":
    main()
