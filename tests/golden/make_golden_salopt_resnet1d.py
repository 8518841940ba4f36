#!/usr/bin/env python3
"""Golden vectors for saliency-guided mixing with a ResNet9-1D saliency model (saliency.py:39-40,
``args.model == 'resnet9'``), recorded by RUNNING the reference's ``augmentations.augment`` with
'(saloptenv)durratiomixup' on the CPU in the build container.

    python tests/golden/make_golden_salopt_resnet1d.py        (needs /root/reference)

The frozen saliency model is the reference's ``models.ResNet9(4, 2)`` initialised with
``torch.manual_seed(SEED1D)`` (4.9 M parameters: not stored — this package's models.ResNet9 draws
the same weights from the same seed, which is asserted here) and written as 'model.pth' where
``utils.experiment_dir`` expects the 'base' run.  The batch is dense noise over the whole row (no flat
stretch: no ReLU / max-pool ties), the cycle boundaries are synthetic.make_batch's.

resnet1d_salopt_4x4x2500.npz: x, frames, labels, wav, method, step, fired, y, mix, target_out, lam,
sal (the maps ``get_saliency_maps`` returned), disp (what each optimal_displacement_* call returned,
placed per (sample, state)).  The raw gradient is not kept.
"""
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import pcgmix_amd  # noqa: E402,F401
from pcgmix_amd import models, synthetic  # noqa: E402

SEED1D = 2468
B1D, T1D = 4, 2500
METHOD, STEP = "(saloptenv)durratiomixup", 6
NAME = f"resnet1d_salopt_{B1D}x4x{T1D}"


def inputs():
    """Four (4, 2500) rows of dense noise with make_batch's cycle boundaries; classes 0, 1, 0, 0 (the singleton mixes with itself)."""
    _, frames, _, wav = synthetic.make_batch(B1D, 4, T1D, sample_rate=1000, seed=41)
    x = np.random.RandomState(42).standard_normal((B1D, 4, T1D)).astype(np.float32)
    labels = np.array([0, 1, 0, 0], dtype=np.int64)
    return x, frames, labels, wav


def main():
    mg = importlib.import_module("make_golden")
    ref = importlib.import_module("_ref_import").import_reference()
    tmp = tempfile.mkdtemp(prefix="pcgmix_golden_resnet1d_")
    x, frames, labels, wav = inputs()
    a = mg.base_args("base", 4, B1D, tmp, model="resnet9")
    exp = ref.utils.experiment_dir(a)
    os.makedirs(exp, exist_ok=True)
    torch.manual_seed(SEED1D)
    net = ref.models.ResNet9(in_channels=4, num_classes=2)
    torch.manual_seed(SEED1D)
    own = models.ResNet9(4, 2)
    sd, od = net.state_dict(), own.state_dict()
    assert list(sd) == list(od) and all(torch.equal(sd[k], od[k]) for k in sd), "the seed draws other weights"
    torch.save({"module." + k: v for k, v in sd.items()}, os.path.join(exp, "model.pth"))

    orig_base_args = mg.base_args
    mg.base_args = lambda method, c, b, d, **kw: orig_base_args(method, c, b, d, model="resnet9")
    try:
        case = mg.run_case(ref, ref.augmentations, x, frames, labels, wav, METHOD, STEP, tmp,
                           record_salopt=True)
    finally:
        mg.base_args = orig_base_args
    case.pop("grad", None)
    case.pop("knots", None)
    assert int(case["fired"]) == 1 and np.abs(case["disp"]).max() > 0
    mg.save(NAME, case)


if __name__ == "__main__":
    main()
