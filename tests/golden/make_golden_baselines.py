#!/usr/bin/env python3
"""Golden vectors of the paper's 1D comparison baselines, recorded by RUNNING the reference.

Run in the build container only (needs the reference checkout, see _ref_import.py):

    python tests/golden/make_golden_baselines.py

The reference's own ``augmentations.augment`` is called on synthetic batches for mixup(same),
mixup(mix), magnitudewarp, timewarp, timemask and respiratoryscale.  Files are named
``base1d_*.npz`` (a prefix none of the other golden globs match).  Recorded per case:

  x                    the input, cloned BEFORE the call (timemask zeroes it in place)
  frames, labels, wav  the other inputs
  method, step         args.method, step_counter.count; sample_rate = args.sample_rate
  fired                1 if the probability gate let the method run
  same_object          1 if augment() returned the very input tensor
  y, target_out, mix   augment()'s outputs (mix: [] -> empty array)
  np_before, np_after  numpy's global MT19937 state around the call: key (624 uint32), then
                       pos, has_gauss and the cached Gaussian in np_*_tail
  lam, knots           get_lambda's value and the np.random.normal draw (when made)
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
from pcgmix_amd import synthetic  # noqa: E402
from _ref_import import import_reference  # noqa: E402

SAMPLE_RATE = 1000


def np_state():
    _, key, pos, has_gauss, cached = np.random.get_state()
    return np.asarray(key, dtype=np.uint32).copy(), np.array([pos, has_gauss, cached], dtype=np.float64)


def run_case(aug, x, frames, labels, wav, method, step, np_seed, tmp):
    rec = {"lam": np.nan, "knots": np.zeros((0,))}
    data = torch.from_numpy(x.copy())
    target_ohe = torch.nn.functional.one_hot(torch.from_numpy(labels), 2)
    args = base_args(method, x.shape[1], x.shape[0], tmp, sample_rate=SAMPLE_RATE)
    orig_get_lambda, orig_normal = aug.get_lambda, np.random.normal

    def get_lambda(*a, **k):
        rec["lam"] = float(orig_get_lambda(*a, **k))
        return rec["lam"]

    def normal(*a, **k):
        out = orig_normal(*a, **k)
        rec["knots"] = np.array(out, dtype=np.float64, copy=True)
        return out

    np.random.seed(np_seed)              # the global stream the warps draw from, as it is
    np.random.normal(size=np_seed % 5)   # (an odd count leaves numpy's Gaussian cache full)
    before = np_state()
    py_before = random.getstate()
    aug.get_lambda, np.random.normal = get_lambda, normal
    try:
        y, t_out, mix, cut = aug.augment(args, data, target_ohe, torch.from_numpy(frames.copy()), wav,
                                         StepCounter(step), None, torch.device("cpu"), tmp)
    finally:
        aug.get_lambda, np.random.normal = orig_get_lambda, orig_normal
    after = np_state()
    assert cut is None and random.getstate() == py_before
    p = float(method.split("+")[-1]) if "+" in method else 1.0
    return {
        "x": x, "frames": frames, "labels": labels, "wav": np.array(wav),
        "method": np.array(method), "step": np.int64(step), "sample_rate": np.int64(SAMPLE_RATE),
        "fired": np.int64(random.Random(step).uniform(0, 1) < p),
        "same_object": np.int64(y is data),
        "y": y.detach().numpy().astype(np.float32).copy(),
        "mix": np.asarray(mix, dtype=np.int64),
        "target_out": t_out.detach().numpy().copy(),
        "np_before": before[0], "np_before_tail": before[1],
        "np_after": after[0], "np_after_tail": after[1],
        "lam": np.float64(rec["lam"]), "knots": rec["knots"],
    }


def main():
    ref = import_reference()
    tmp = tempfile.mkdtemp(prefix="pcgmix_golden_")
    batches = {
        "s12x2x640": synthetic.make_batch(12, 2, 640, seed=21, rate_scale=0.4),
        "a8x4x2500": synthetic.make_batch(8, 4, 2500, sample_rate=1000, seed=22),
        "o7x1x641": synthetic.make_batch(7, 1, 641, seed=23, rate_scale=0.4),
        "c5x3x333": synthetic.make_batch(5, 3, 333, seed=24, rate_scale=0.2),
    }
    cases = [
        # mixup: same label, all labels; the gate firing and rejecting
        ("s12x2x640", "mixup(same)", 3), ("s12x2x640", "mixup(mix)", 4),
        ("a8x4x2500", "mixup(same)", 9), ("o7x1x641", "mixup(mix)", 10),
        ("s12x2x640", "mixup(same)+0.5", 1), ("s12x2x640", "mixup(same)+0.5", 2),
        ("c5x3x333", "(samePCG)mixup(same)", 6),
        # magnitudewarp: defaults, the experiments' parameters, other knots, the gate
        ("s12x2x640", "magnitudewarp", 5), ("a8x4x2500", "magnitudewarp(0.2,4)", 6),
        ("o7x1x641", "magnitudewarp(0.3,1)", 7), ("c5x3x333", "magnitudewarp(0.2,4)+0.5", 1),
        ("c5x3x333", "magnitudewarp(0.2,4)+0.5", 2),
        # timewarp: default (0.05, 2), the experiments' (0.05, 4), sigma 0.2 (non-monotone xp)
        ("s12x2x640", "timewarp", 8), ("a8x4x2500", "timewarp(0.05,4)", 9),
        ("s12x2x640", "timewarp(0.2,4)", 10), ("s12x2x640", "timewarp(0.2,4)", 11),
        ("o7x1x641", "timewarp(0.2,3)", 12), ("c5x3x333", "timewarp(0.05,4)+0.5", 1),
        ("c5x3x333", "timewarp(0.05,4)+0.5", 2), ("c5x3x333", "timewarp(0.3,6)", 13),
        # timemask: default 0.2, the experiments' 0.2 and 0.1, a clamped maximum, the gate
        ("s12x2x640", "timemask", 14), ("a8x4x2500", "timemask(0.2)", 15),
        ("s12x2x640", "timemask(0.1)", 16), ("o7x1x641", "timemask(1.5)", 17),
        ("c5x3x333", "timemask(0.1)+0.5", 1), ("c5x3x333", "timemask(0.1)+0.5", 2),
        # respiratoryscale: defaults, the experiments' (12,20), other rates, the gate
        ("s12x2x640", "respiratoryscale", 18), ("a8x4x2500", "respiratoryscale(12,20)", 19),
        ("o7x1x641", "respiratoryscale(8.5,30)", 20), ("c5x3x333", "respiratoryscale(12,20)+0.5", 1),
        ("c5x3x333", "respiratoryscale(12,20)+0.5", 2),
    ]
    for i, (tag, method, step) in enumerate(cases):
        x, frames, labels, wav = batches[tag]
        case = run_case(ref.augmentations, x, frames, labels, wav, method, step, 100 + i, tmp)
        name = f"base1d_{tag}_{i:02d}"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **case)
        print(f"{name:24s} {method:28s} {os.path.getsize(path) / 1024:7.1f} KiB  fired={int(case['fired'])}")


if __name__ == "__main__":
    main()
