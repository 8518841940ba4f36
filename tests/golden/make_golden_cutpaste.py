#!/usr/bin/env python3
"""Golden vectors of the heart-cycle cut-and-paste family, durmixrespscale and bare cutout (1D and
2D), recorded by RUNNING the reference.

Run in the build container only (needs the reference checkout, see _ref_import.py):

    python tests/golden/make_golden_cutpaste.py

The reference's own ``augmentations.augment`` / ``augmentations2d.augment`` are called on small
synthetic batches.  Files are named ``cutpaste_*.npz`` (1D) and ``cutout2d_*.npz`` (prefixes none of
the other golden globs match).  Recorded per case:

  x                    the input, cloned BEFORE the call (cutout zeroes it in place)
  frames, labels, wav  the other inputs (2D: wav is empty)
  method, step         args.method, step_counter.count
  batch_size           args.batch_size (lengthcutmix derives its bins from it, not from B)
  sample_rate          args.sample_rate
  fired                1 if the probability gate let the method run
  same_object          1 if augment() returned the very input tensor
  y, target_out, mix   augment()'s outputs (mix: [] -> empty array)
  cut                  the fourth return value, -1 for None
  np_before, np_after  numpy's global MT19937 state around the call (key; pos, has_gauss and the
                       cached Gaussian in np_*_tail)
  lam                  get_lambda's value (durmixrespscale), NaN when it was not called

The generator asserts that the reference ran every case without raising and that the partners are
not the identity wherever partners are drawn.
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


def run_case(aug, x, frames, labels, wav, method, step, np_seed, tmp, batch_size=None, is2d=False):
    rec = {"lam": np.nan}
    data = torch.from_numpy(x.copy())
    target_ohe = torch.nn.functional.one_hot(torch.from_numpy(labels), 2)
    batch_size = x.shape[0] if batch_size is None else batch_size
    args = base_args(method, x.shape[1], batch_size, tmp, sample_rate=SAMPLE_RATE,
                     model="resnet9" if is2d else "Potes")
    if is2d:
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
    devnull = open(os.devnull, "w")
    stdout, sys.stdout = sys.stdout, devnull          # cutout(ch) prints its fractions
    try:
        y, t_out, mix, cut = aug.augment(args, data, target_ohe, torch.from_numpy(frames.copy()),
                                         None if is2d else wav, StepCounter(step), None,
                                         torch.device("cpu"), tmp)
    finally:
        sys.stdout = stdout
        devnull.close()
        aug.get_lambda = orig_get_lambda
    after = np_state()
    assert random.getstate() == py_before
    p = float(method.split("+")[-1]) if "+" in method else 1.0
    return {
        "x": x, "frames": frames, "labels": labels, "wav": np.array(wav if wav is not None else (), dtype=str),
        "method": np.array(method), "step": np.int64(step), "batch_size": np.int64(batch_size),
        "sample_rate": np.int64(SAMPLE_RATE),
        "fired": np.int64(random.Random(step).uniform(0, 1) < p),
        "same_object": np.int64(y is data),
        "y": y.detach().numpy().astype(np.float32).copy(),
        "mix": np.asarray(mix, dtype=np.int64),
        "target_out": t_out.detach().numpy().copy(),
        "cut": np.int64(-1 if cut is None else cut),
        "np_before": before[0], "np_before_tail": before[1],
        "np_after": after[0], "np_after_tail": after[1],
        "lam": np.float64(rec["lam"]),
    }


def with_wav(batch, wav):
    x, frames, labels, _ = batch
    assert len(wav) == x.shape[0]
    return x, frames, labels, tuple(wav)


def tiny_states_batch(seed, B, C, T):
    """Every heart state 1-9 samples long (none 0): '(smooth)' runs with an overlap below 10."""
    rs = np.random.RandomState(seed)
    lens = rs.randint(1, 10, size=(B, 4))
    frames = np.zeros((B, 5), dtype=np.int64)
    frames[:, 1:] = np.cumsum(lens, axis=1)
    assert int(frames.max()) <= T
    x = rs.standard_normal((B, C, T)).astype(np.float32)
    x[np.broadcast_to(np.arange(T)[None, None, :] >= frames[:, 4][:, None, None], x.shape)] = 0
    labels = (np.arange(B) % 2).astype(np.int64)
    wav = tuple(f"{'ab'[i % 2]}{i // 3:04d}" for i in range(B))
    return x, frames, labels, wav


def clipped_batch(seed, B, C):
    """Cycles of very different lengths in a signal no longer than the longest one: for several
    samples ``f1[cut] + f2[4] - f2[cut]`` exceeds T and the paste is clipped."""
    rs = np.random.RandomState(seed)
    lens = np.stack([rs.randint(10, 40, B), rs.randint(20, 120, B), rs.randint(10, 30, B),
                     rs.randint(20, 160, B)], axis=1)
    frames = np.zeros((B, 5), dtype=np.int64)
    frames[:, 1:] = np.cumsum(lens, axis=1)
    T = int(frames[:, 4].max())
    x = rs.standard_normal((B, C, T)).astype(np.float32)
    x[np.broadcast_to(np.arange(T)[None, None, :] >= frames[:, 4][:, None, None], x.shape)] = 0
    labels = np.zeros(B, dtype=np.int64)
    labels[B // 2:] = 1
    wav = tuple(f"{'ab'[i % 2]}{i // 4:04d}" for i in range(B))
    return x, frames, labels, wav


def batch2d(seed, B, C, F, W):
    rs = np.random.RandomState(seed)
    lens = np.stack([rs.randint(1, W // 8 + 2, B), rs.randint(1, W // 4 + 2, B), rs.randint(1, W // 8 + 2, B),
                     rs.randint(1, W // 3 + 2, B)], axis=1)
    frames = np.zeros((B, 5), dtype=np.int64)
    frames[:, 1:] = np.cumsum(lens, axis=1)
    assert int(frames.max()) <= W
    x = rs.standard_normal((B, C, F, W)).astype(np.float32)
    labels = rs.randint(0, 2, size=B).astype(np.int64)
    return x, frames, labels, None


def steps_for_cuts(seed_of_step):
    """The first steps at which ``Random(seed_of_step(step)).randint(1, 3)`` gives 1, 2 and 3."""
    found = {}
    for step in range(3, 200):
        found.setdefault(random.Random(seed_of_step(step)).randint(1, 3), step)
        if len(found) == 3:
            return [found[c] for c in (1, 2, 3)]
    raise AssertionError


def main():
    ref = import_reference()
    tmp = tempfile.mkdtemp(prefix="pcgmix_golden_")
    rec4 = tuple(f"{'abc'[i // 4]}{i // 4:04d}" for i in range(12))            # 4 cycles per recording
    set2 = tuple(f"{'ab'[i % 2]}{i:04d}" for i in range(12))                   # 2 data sets x 2 labels
    batches = {
        "s12x2x320": with_wav(synthetic.make_batch(12, 2, 320, seed=41, rate_scale=0.2), rec4),
        "d12x2x320": with_wav(synthetic.make_batch(12, 2, 320, seed=41, rate_scale=0.2), set2),
        "o7x3x321": with_wav(synthetic.make_batch(7, 3, 321, seed=42, rate_scale=0.2),
                             ("a0", "a0", "a0", "b1", "b1", "b1", "b1")),
        "c9x4x250": with_wav(synthetic.make_batch(9, 4, 250, seed=43, rate_scale=0.15),
                             ("a0", "a0", "a0", "b1", "b1", "b1", "a2", "a2", "a2")),
        "u5x1x322": with_wav(synthetic.make_batch(5, 1, 322, seed=44, rate_scale=0.2),
                             ("a0", "a0", "a0", "a0", "a0")),
        "l40x1x160": synthetic.make_batch(40, 1, 160, seed=47, rate_scale=0.1),   # enough cycles for 10 bins
        "t8x2x40": tiny_states_batch(45, 8, 2, 40),
        "k8x2": clipped_batch(46, 8, 2),
    }
    own_seed = lambda s: s                 # noqa: E731
    label_seed = lambda s: s * 131071      # noqa: E731
    cases = [
        # keep-duration swap: same label, same recording; '(rand)' placement; the gate
        ("s12x2x320", "durratiocutmix", 3), ("o7x3x321", "durratiocutmix", 4),
        ("c9x4x250", "(rand)durratiocutmix", 5), ("s12x2x320", "(rand)durratiocutmix", 6),
        ("s12x2x320", "durratiocutmix+0.5", 1), ("s12x2x320", "durratiocutmix+0.5", 2),
        ("s12x2x320", "wav-durratiocutmix", 7), ("o7x3x321", "(rand)wav-durratiocutmix", 8),
        ("c9x4x250", "wav-durratiocutmix+0.5", 1), ("c9x4x250", "wav-durratiocutmix+0.5", 2),
        # labelcutmix: the middle cut, its suffixes, the gate
        ("s12x2x320", "labelcutmix", 9), ("o7x3x321", "labelcutmix", 10), ("u5x1x322", "labelcutmix", 11),
        ("s12x2x320", "labelcutmix(cutout)", 12), ("c9x4x250", "labelcutmix(smooth)", 13),
        ("o7x3x321", "labelcutmix(smooth)", 14),
        ("s12x2x320", "labelcutmix+0.5", 1), ("s12x2x320", "labelcutmix+0.5", 2),
        ("t8x2x40", "labelcutmix(smooth)", 15), ("t8x2x40", "(rand)labelcutmix(smooth)(cutout)", 16),
        ("k8x2", "labelcutmix", 17), ("k8x2", "labelcutmix(smooth)(cutout)", 18),
    ]
    for step in steps_for_cuts(label_seed):
        cases += [("s12x2x320", "(rand)labelcutmix", step),
                  ("c9x4x250", "(rand)labelcutmix(smooth)(cutout)", step)]
    # lengthcutmix: args.batch_size 12 and 250 (0 and 2 bins), '(5bins)', '(10bins)'
    cases += [("s12x2x320", "lengthcutmix", 19, 12), ("s12x2x320", "lengthcutmix", 20, 250),
              ("s12x2x320", "lengthcutmix(5bins)", 21, 12), ("l40x1x160", "lengthcutmix(10bins)", 22, 40),
              ("o7x3x321", "lengthcutmix(cutout)", 23, 250), ("k8x2", "lengthcutmix", 24, 12),
              ("s12x2x320", "lengthcutmix+0.5", 1, 12), ("s12x2x320", "lengthcutmix+0.5", 2, 12)]
    for step in steps_for_cuts(own_seed):
        cases += [("s12x2x320", "(rand)lengthcutmix", step, 12), ("d12x2x320", "(rand)datasetcutmix", step),
                  ("s12x2x320", "(rand)wavcutmix", step)]
    cases += [
        ("d12x2x320", "datasetcutmix", 25), ("d12x2x320", "datasetcutmix(smooth)", 26),
        ("d12x2x320", "datasetcutmix+0.5", 1), ("d12x2x320", "datasetcutmix+0.5", 2),
        ("s12x2x320", "wavcutmix", 27), ("c9x4x250", "wavcutmix(cutout)", 28),
        ("s12x2x320", "wavcutmix+0.5", 1), ("s12x2x320", "wavcutmix+0.5", 2),
        # durmixrespscale: defaults, other rates, '(rand)', the gate
        ("s12x2x320", "durmixrespscale", 29), ("o7x3x321", "durmixrespscale(8.5,30)", 30),
        ("c9x4x250", "(rand)durmixrespscale", 31), ("u5x1x322", "durmixrespscale(12,20)", 32),
        ("c9x4x250", "durmixrespscale+0.5", 1), ("c9x4x250", "durmixrespscale+0.5", 2),
        # bare cutout: the parameters in the string are ignored in 1D; one span per channel
        ("s12x2x320", "cutout", 33), ("o7x3x321", "cutout(0.25,0.25)", 34), ("c9x4x250", "cutout(ch)", 35),
        ("o7x3x321", "cutout(ch)", 36), ("s12x2x320", "cutout+0.5", 1), ("s12x2x320", "cutout+0.5", 2),
    ]
    clipped = 0
    for i, case in enumerate(cases):
        tag, method, step = case[:3]
        x, frames, labels, wav = batches[tag]
        g = run_case(ref.augmentations, x, frames, labels, wav, method, step, 300 + i, tmp,
                     batch_size=case[3] if len(case) > 3 else None)
        if int(g["fired"]) and "cutout" != method.split("(")[0].split("+")[0] and "durmixrespscale" not in method:
            assert not np.array_equal(g["mix"], np.arange(len(labels))), (tag, method, "identity partners")
        if int(g["fired"]) and int(g["cut"]) > 0:
            c, f2 = int(g["cut"]), frames[g["mix"]]
            clipped += int(((frames[:, c] + f2[:, 4] - f2[:, c]) > x.shape[2]).sum())
        name = f"cutpaste_{tag}_{i:02d}"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **g)
        print(f"{name:26s} {method:36s} {os.path.getsize(path) / 1024:7.1f} KiB  fired={int(g['fired'])} "
              f"cut={int(g['cut'])}")
    assert clipped > 0, "no case clips its paste at T"

    batches2d = {
        "q6x2x32x32": batch2d(51, 6, 2, 32, 32),       # F == W
        "w5x1x24x40": batch2d(52, 5, 1, 24, 40),       # F != W
        "t4x3x40x28": batch2d(53, 4, 3, 40, 28),
    }
    cases2d = [
        ("q6x2x32x32", "cutout", 3), ("w5x1x24x40", "cutout", 4), ("t4x3x40x28", "cutout", 5),
        ("q6x2x32x32", "cutout(0.25,0.25)", 6), ("w5x1x24x40", "cutout(0.25,0.25)", 7),
        ("q6x2x32x32", "cutout(0.9,1.0)", 8), ("w5x1x24x40", "cutout(0.9,1.0)", 9),
        ("t4x3x40x28", "cutout(0.9,1.0)", 10),
        ("q6x2x32x32", "cutout(0.25,0.25)+0.5", 1), ("q6x2x32x32", "cutout(0.25,0.25)+0.5", 2),
    ]
    for i, (tag, method, step) in enumerate(cases2d):
        x, frames, labels, _ = batches2d[tag]
        g = run_case(ref.augmentations2d, x, frames, labels, None, method, step, 400 + i, tmp, is2d=True)
        name = f"cutout2d_{tag}_{i:02d}"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **g)
        print(f"{name:26s} {method:36s} {os.path.getsize(path) / 1024:7.1f} KiB  fired={int(g['fired'])}")


if __name__ == "__main__":
    main()
