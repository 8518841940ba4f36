#!/usr/bin/env python3
"""Golden vectors for ``saliency.saliency_map`` (saliency.py:132-202), recorded by RUNNING the
reference's function on the CPU in the build container.

    python tests/golden/make_golden_salmap.py        (needs /root/reference)

The model is the reference's ``CNN_potes_TS`` with the weights of potes_state_seed1234.npz
(make_golden.py wrote them).  Only data is written: no reference source is copied.

salmap_{tag}.npz: x (B,4,2500), labels, frames, grad (the raw ``data.grad`` the reference's backward
left), saliency (B,1,T), saliency_bins (B,1,T), out (B,2), bin_values (B,14) float64, bin_frames
(B,15) int64, and gauss (the 57 weights ``gaussian_kernel(57, 7.54)`` returned, float64).

  ordinary   B = 6, synthetic state lengths
  short      the same batch; row 2's states are shorter than their bin counts (lengths 3, 2, 1, 7)
  fullrow    B = 2; row 1's cycle ends exactly at T
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import pcgmix_amd  # noqa: E402,F401
from pcgmix_amd import synthetic  # noqa: E402
from _ref_import import import_reference  # noqa: E402

T = 2500


def cases():
    x, frames, labels, _ = synthetic.make_batch(6, 4, T, sample_rate=1000, seed=57)
    yield "ordinary", x, frames, labels
    short = frames.copy()
    short[2] = np.cumsum([0, 3, 2, 1, 7])
    yield "short", x, short, labels
    x2, f2, l2, _ = synthetic.make_batch(2, 4, T, sample_rate=1000, seed=58)
    f2[1] = np.array([0, 310, 1100, 1420, T])
    x2[1] = np.random.RandomState(59).standard_normal((4, T)).astype(np.float32)
    yield "fullrow", x2, f2, np.array([1, 0], dtype=np.int64)


def main():
    ref = import_reference()
    sd = np.load(os.path.join(HERE, "potes_state_seed1234.npz"))
    model = ref.models.CNN_potes_TS(num_channels=4, num_classes=2, dataset="PhysioNet")
    model.load_state_dict({k: torch.from_numpy(sd[k]) for k in sd.files})
    gauss = np.array(ref.saliency.gaussian_kernel(n=57, sigma=7.54), dtype=np.float64)
    for tag, x, frames, labels in cases():
        data = torch.from_numpy(x.copy())
        tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2)
        sal, sal_bins, out, values, bounds = ref.saliency.saliency_map(
            data, tgt, torch.from_numpy(frames.copy()), model, "cpu")
        path = os.path.join(HERE, f"salmap_{tag}.npz")
        np.savez_compressed(
            path, x=x, labels=labels, frames=frames, grad=data.grad.detach().numpy(),
            saliency=sal.detach().numpy(), saliency_bins=sal_bins.detach().numpy(),
            out=out.detach().numpy(), bin_values=np.stack(values).astype(np.float64),
            bin_frames=np.stack(bounds).astype(np.int64), gauss=gauss)
        print(f"salmap_{tag:10s} {os.path.getsize(path) / 1024:8.1f} KiB")


if __name__ == "__main__":
    main()
