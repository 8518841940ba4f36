"""Inputs of the SELC-phase golden (train_selc_ref.npz), shared by the script that records it from
the reference (make_golden_selc.py) and the tests that replay it.  Pure data builders on this
project's synthetic generator: nothing here touches the reference."""
import numpy as np
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import synthetic

import train_cases

SELC_B, SELC_BATCHES, SELC_EPOCHS, SELC_ES = 16, 3, 4, 1
SELC_STEPS = SELC_BATCHES * SELC_EPOCHS
SELC_METHOD = "SELCdurratiomixup"


def selc_args():
    """train_epoch's fields (train_model.py:490-589) for four epochs of three batches; the turning
    point behind the first epoch (``es = 1``; the reference's own rule, :394-402, gives
    int(4 * 0.4) = 1 for this method name)."""
    a = train_cases.traj_args()
    a.__dict__.update(method=SELC_METHOD, num_epochs=SELC_EPOCHS, num_steps=SELC_STEPS)
    return a


def selc_batches():
    """Three fixed batches of 16 at (4, 2500); sample indices 0..47, every one exactly once."""
    out = []
    for i in range(SELC_BATCHES):
        x, frames, labels, wav = synthetic.make_batch(SELC_B, 4, 2500, sample_rate=1000, seed=700 + i)
        out.append((torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(frames), wav,
                    torch.ones(SELC_B, dtype=torch.long), torch.arange(SELC_B) + SELC_B * i))
    return out


def selc_labels(batches):
    return np.concatenate([b[1].numpy() for b in batches])
