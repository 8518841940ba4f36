"""Inputs of the 1D latentmixup goldens (latent1d_*.npz, train_latent1d_ref.npz), shared by the
script that records them from the reference (make_golden_latent1d.py) and the tests that replay
them.  Pure data builders on this project's synthetic generator and ``train_cases``: nothing here
touches the reference."""
import numpy as np
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import synthetic

import train_cases as TC

# ---- augment() cases ---------------------------------------------------------------------------
BATCH_SEED = 22                      # synthetic.make_batch(8, 4, 2500, sample_rate=1000, seed=22)
NARROW_FILTERS = [4, 8, 8, 16]       # a ResNet9-1D whose state_dict fits in a fixture
NARROW_LINEAR = NARROW_FILTERS[3] * (2500 // 2 // 2 // 2 // 4)
NARROW_SEED = 31

# (tag, args.model, method, step).  Random(step).randint(1, 3) is 2,1,1,1,1,3,3,2 for steps 0..7;
# Random(step).uniform(0,1) < 0.5 at step 1 (fires) and not at step 2.
AUGMENT_CASES = (
    ("potes", "Potes", "latentmixup", 3),
    ("potes", "Potes", "latentmixup+0.5", 1),
    ("potes", "Potes", "latentmixup+0.5", 2),
    ("potes", "Potes", "latentmixup cutmix", 7),
    ("resnet", "resnet9", "latentmixup", 1),            # depth 1: (8, 8, 1250)
    ("resnet", "resnet9", "latentmixup", 0),            # depth 2: (8, 16, 312)
    ("resnet", "resnet9", "latentmixup", 5),            # depth 3: (8, 1248)
    ("resnet", "resnet9", "latentmixup(same)+0.5", 2),  # the gate rejects
)


def augment_batch():
    return synthetic.make_batch(8, 4, 2500, sample_rate=1000, seed=BATCH_SEED)


def narrow_resnet(factory):
    """``factory(in_channels, num_classes, filters=, linear=)`` -> the narrow ResNet9-1D in eval
    mode with seeded weights and non-trivial BatchNorm running statistics."""
    torch.manual_seed(NARROW_SEED)
    m = factory(4, 2, filters=list(NARROW_FILTERS), linear=NARROW_LINEAR)
    g = torch.Generator().manual_seed(NARROW_SEED + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return m.eval()


# ---- train_epoch trajectories ------------------------------------------------------------------
LATENT_METHOD = "latentmixup"
# Random(count).randint(1, 3) is 2,1,1,1,1,3,3,2,1,2,3,2 for counts 0..11: counts 8, 9, 10 are the
# first three consecutive ones that cover every depth, so the three batches (and with them the
# learning rates and the tolerances) of the existing ResNet9-1D trajectory serve unchanged.
RESNET_FIRST_COUNT = 8               # counts 8..10 -> depths 1, 2, 3


def potes_traj_args():
    a = TC.traj_args()
    a.method = LATENT_METHOD
    return a


def resnet_traj_args():
    a = TC.resnet1d_args()
    a.method = LATENT_METHOD
    return a


def resnet_traj_batches():
    return TC.resnet1d_batches()


def np_state():
    _, key, pos, has_gauss, cached = np.random.get_state()
    return np.asarray(key, dtype=np.uint32).copy(), np.array([pos, has_gauss, cached], dtype=np.float64)
