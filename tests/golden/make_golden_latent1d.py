#!/usr/bin/env python3
"""Golden vectors of the 1D ``latentmixup`` branch (augmentations.py:1472-1506), recorded by RUNNING
the reference on the CPU.

Run in the build container only (needs the reference checkout, see _ref_import.py):

    python tests/golden/make_golden_latent1d.py [augment] [train]

``latent1d_*.npz`` — one call of the reference's ``augmentations.augment`` each (latent_cases.py:
AUGMENT_CASES): the Potes model in eval() with the weights of potes_state_seed1234.npz, a narrow
ResNet9-1D (filters [4,8,8,16]) in eval() whose state_dict travels in the file (``state.*``).

  x, frames, labels, wav   the inputs;  method, step, model (args.model)
  fired, same_object       the gate's verdict; 1 if augment() returned the very input tensor
  y, mix, target_out       augment()'s outputs (the blended features; mix: [] -> empty array)
  depth                    args.depth after the call (0 = untouched)
  lam                      get_lambda's value (nan when the gate rejected)
  np_before, np_after      numpy's global MT19937 state around the call (+ *_tail: pos, has_gauss,
                           cached Gaussian), as base1d_* records them

``train_latent1d_ref.npz`` — the reference's ``train_epoch`` with method 'latentmixup':

  potes_*   10 steps, set up exactly as traj_* of train_ref.npz (Potes seed 7, dropout 0, the
            batches of train_cases.traj_batches()): losses, lrs, depths, final parameters
  r1d_*     ResNet9-1D full width, set up exactly as r1d_* of train_resnet_ref.npz
            (train_cases.resnet1d_args(), lr_max = RESNET_LR_MAX, digests of the large tensors) with
            the step counter started at 8: depths 1, 2, 3
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
import latent_cases as LC  # noqa: E402
import train_cases as TC  # noqa: E402


def augment_cases(ref):
    aug = ref.augmentations
    tmp = tempfile.mkdtemp(prefix="pcgmix_golden_")
    x, frames, labels, wav = LC.augment_batch()
    sd = np.load(os.path.join(HERE, "potes_state_seed1234.npz"))
    potes = ref.models.CNN_potes_TS(num_channels=4, num_classes=2, dataset="PhysioNet")
    potes.load_state_dict({k: torch.from_numpy(sd[k]) for k in sd.files})
    nets = {"potes": potes.eval(), "resnet": LC.narrow_resnet(ref.models.ResNet9)}
    for i, (tag, model_name, method, step) in enumerate(LC.AUGMENT_CASES):
        rec = {"lam": np.nan}
        data = torch.from_numpy(x.copy())
        target_ohe = torch.nn.functional.one_hot(torch.from_numpy(labels), 2)
        args = base_args(method, 4, 8, tmp, model=model_name)
        orig = aug.get_lambda

        def get_lambda(*a, **k):
            rec["lam"] = float(orig(*a, **k))
            return rec["lam"]
        np.random.seed(100 + i)
        np.random.normal(size=i % 5)         # (an odd count leaves numpy's Gaussian cache full)
        before = LC.np_state()
        py_before = random.getstate()
        aug.get_lambda = get_lambda
        try:
            with torch.no_grad():
                y, t_out, mix, cut = aug.augment(args, data, target_ohe, torch.from_numpy(frames.copy()), wav,
                                                 StepCounter(step), nets[tag], torch.device("cpu"), tmp)
        finally:
            aug.get_lambda = orig
        after = LC.np_state()
        assert cut is None and random.getstate() == py_before and t_out is target_ohe
        p = float(method.split("+")[-1]) if "+" in method else 1.0
        case = {
            "x": x, "frames": frames, "labels": labels, "wav": np.array(wav),
            "method": np.array(method), "step": np.int64(step), "model": np.array(model_name),
            "fired": np.int64(random.Random(step).uniform(0, 1) < p),
            "same_object": np.int64(y is data),
            "y": (np.zeros(0, np.float32) if y is data else y.detach().numpy().astype(np.float32).copy()),
            "mix": np.asarray(mix, dtype=np.int64), "target_out": t_out.numpy().copy(),
            "depth": np.int64(args.depth), "lam": np.float64(rec["lam"]),
            "np_before": before[0], "np_before_tail": before[1],
            "np_after": after[0], "np_after_tail": after[1],
        }
        if tag == "resnet":
            for k, v in nets[tag].state_dict().items():
                case["state." + k] = v.numpy().copy()
        name = f"latent1d_{tag}_{i:02d}"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **case)
        print(f"{name:20s} {method:24s} step {step} depth {int(args.depth)} y {tuple(case['y'].shape)} "
              f"fired={int(case['fired'])} {os.path.getsize(path) / 1024:7.1f} KiB")


def run_epoch(T, A, args, model, batches, first_count):
    opt = torch.optim.Adam(model.parameters(), lr=args.lr_max, weight_decay=args.weight_decay)   # :405
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=args.lr_max, total_steps=args.num_steps)  # :410
    ce = T.CELoss(2)
    losses, depths = [], []

    def criterion(logits_, target_, index_, epoch_, mode_):
        loss_ = ce(logits_, target_)
        losses.append(float(loss_.item()))
        return loss_
    orig_augment = A.augment

    def augment(args_, *a, **k):             # train_epoch resets args.depth behind the second half (:538)
        res = orig_augment(args_, *a, **k)
        depths.append(int(args_.depth))
        return res
    sc = T.step_counter_class()
    sc.count = first_count
    A.augment = augment
    try:
        mean_loss, acc, lrs = T.train_epoch(args, model, batches, torch.device("cpu"), opt, sched, criterion,
                                            1, sc, None, "")
    finally:
        A.augment = orig_augment
    assert sc.count == first_count + len(batches) == first_count + len(losses) and args.depth == 0
    return (np.asarray(losses, dtype=np.float64), np.asarray(lrs, dtype=np.float64),
            np.asarray(depths, dtype=np.int64), np.float64(mean_loss), np.float64(acc))


def trajectories(ref):
    T, A = ref.train_model, ref.augmentations
    out = {}
    args = LC.potes_traj_args()
    torch.manual_seed(7)
    model = ref.models.CNN_potes_TS(num_channels=4, num_classes=2, dataset="PhysioNet")
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    res = run_epoch(T, A, args, model, TC.traj_batches(), 0)
    for k, v in zip(("losses", "lrs", "depths", "mean_loss", "acc"), res):
        out["potes_" + k] = v
    for k, v in model.state_dict().items():
        if not k.startswith(("cnn2", "cnn3", "cnn4")):
            out["potes_final." + k] = v.numpy().copy()
    print("potes losses", res[0], "depths", res[2])

    args = LC.resnet_traj_args()
    torch.manual_seed(7)
    model = ref.models.ResNet9(in_channels=4, num_classes=2)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    res = run_epoch(T, A, args, model, LC.resnet_traj_batches(), LC.RESNET_FIRST_COUNT)
    for k, v in zip(("losses", "lrs", "depths", "mean_loss", "acc"), res):
        out["r1d_" + k] = v
    for k, v in model.state_dict().items():
        if "running_" in k or "num_batches" in k:
            out[f"r1d_buf.{k}"] = v.numpy().copy()
        else:
            out[f"r1d_par.{k}"] = TC.tensor_digest(v.numpy())
            out[f"r1d_ini.{k}"] = TC.tensor_digest(init[k].numpy())[:2]
    print("r1d losses", res[0], "lrs", res[1], "depths", res[2])
    path = os.path.join(HERE, "train_latent1d_ref.npz")
    np.savez_compressed(path, **out)
    print(f"train_latent1d_ref.npz {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    ref = import_reference(extra=("train_model",))
    which = sys.argv[1:] or ["augment", "train"]
    if "augment" in which:
        augment_cases(ref)
    if "train" in which:
        trajectories(ref)


if __name__ == "__main__":
    main()
