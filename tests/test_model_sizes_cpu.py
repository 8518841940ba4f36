"""The model-size ladders of the reference's dispatcher (train_model.py:337-370) through
``build_model``: every name builds the reference's network (parameter count and logits recorded
from the reference's own classes, tests/golden/model_sizes.npz), on the CPU."""
import argparse
import os

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, models, train_model as tm
from conftest import GOLDEN

G = np.load(os.path.join(GOLDEN, "model_sizes.npz"))
NAMES = [str(n) for n in G["names"]]
POTES = [n for n in NAMES if n.startswith("Potes")]
# measured on the reference when the golden file was recorded; a second, independent record
COUNTS = {"Potes0.02": 49950, "Potes0.1": 49994, "Potes(noDropout)": 200270,
          "PotesBig64and32": 1637566, "resnet9-5k": 4868, "resnet9-5m": 5052386}


def make_args(model, **kw):
    a = argparse.Namespace(dataset="PhysioNet", model=model, num_classes=2, num_channels=4, sig_len=2500)
    a.__dict__.update(kw)
    return a


def test_golden_covers_both_ladders():
    assert set(NAMES) == (set(tm.POTES_LADDER) | set(tm.RESNET9_LADDER)) - {"Potes"}
    for name, n in COUNTS.items():
        assert int(G["params"][NAMES.index(name)]) == n


@pytest.mark.parametrize("name", NAMES)
def test_build_model_matches_reference(name):
    torch.manual_seed(11)
    m = tm.build_model(make_args(name)).eval()
    i = NAMES.index(name)
    assert sum(p.numel() for p in m.parameters()) == int(G["params"][i])
    x = torch.from_numpy(np.random.RandomState(3).randn(3, 4, 2500).astype(np.float32))
    with torch.no_grad():
        out = m(x).numpy()
    err = float(np.abs(out - G["logits"][i]).max())
    assert err <= 1e-6, (name, err)


@pytest.mark.parametrize("name", POTES + ["Potes"])
def test_unused_branches_are_frozen(name):
    m = tm.build_model(make_args(name))
    for branch in ("cnn2", "cnn3", "cnn4"):
        assert all(not p.requires_grad for p in getattr(m, branch).parameters())
    assert all(p.requires_grad for p in m.cnn1.parameters())
    assert all(p.requires_grad for p in list(m.dimreduc.parameters()) + list(m.linear.parameters()))


@pytest.mark.parametrize("name,width", [("Potes0.02", 1), ("Potes0.1", 1), ("Potes(noDropout)", 4),
                                        ("PotesBig64and32", 32), ("PotesBig128and64", 64)])
def test_potes_head_scales_with_sig_len(name, width):
    assert tm.build_model(make_args(name)).dimreduc.in_features == 4 * width * 623
    m = tm.build_model(make_args(name, sig_len=5000))
    assert m.dimreduc.in_features == models.potes_flat_features(5000, width=width) == 4 * width * 1248
    with torch.no_grad():
        assert m.eval()(torch.zeros(1, 4, 5000)).shape == (1, 2)


@pytest.mark.parametrize("name", ["resnet9-5k", "resnet9-1.4m"])
def test_resnet_head_scales_with_sig_len(name):
    last = tm.RESNET9_LADDER[name][-1]
    assert tm.build_model(make_args(name)).linear.in_features == last * 78
    m = tm.build_model(make_args(name, sig_len=5000))
    assert m.linear.in_features == models.resnet9_flat_features(5000, last) == last * 156
    if name == "resnet9-5k":
        with torch.no_grad():
            assert m.eval()(torch.zeros(2, 4, 5000)).shape == (2, 2)


def test_no_dropout_variant_has_no_dropout_in_the_branch():
    m = tm.build_model(make_args("Potes(noDropout)"))
    assert not any(isinstance(mod, torch.nn.Dropout) for mod in m.cnn1.modules())
    ref = tm.build_model(make_args("Potes"))
    assert any(isinstance(mod, torch.nn.Dropout) for mod in ref.cnn1.modules())
    assert [k for k in m.state_dict()] == [k for k in ref.state_dict()]


@pytest.mark.parametrize("name", ["Potes0.5", "resnet9-1m", "FCN", "potes0.1"])
def test_unknown_names_still_raise(name):
    with pytest.raises(NotImplementedError):
        tm.build_model(make_args(name))


def test_latentmixup_stays_refused_for_the_new_names():
    from pcgmix_amd import hostprep
    assert set(hostprep.LATENT_MAX_DEPTH_1D) == {"Potes", "resnet9"}


def test_library_exports_the_narrow_entry_points():
    names = ["pcgmix_potes_narrow_supported", "pcgmix_potes_narrow_grad_len",
             "pcgmix_potes_narrow_bwd_blocks", "pcgmix_potes_narrow_mask_bytes",
             "pcgmix_potes_narrow_fwd_f32", "pcgmix_potes_narrow_bwd_mask_f32",
             "pcgmix_potes_narrow_input_grad_mask_f32"]
    for n in names:
        assert n in _lib.SIGNATURES
    lib = _lib.load()                                   # host-only entry points: no device needed
    assert [lib.pcgmix_potes_narrow_supported(a, b) for a, b in ((1, 1), (2, 1), (3, 2), (8, 4), (2, 2))] \
        == [1, 1, 0, 0, 0]
    assert lib.pcgmix_potes_narrow_grad_len(1, 1) == 12 and lib.pcgmix_potes_narrow_grad_len(2, 1) == 23
    assert lib.pcgmix_potes_narrow_grad_len(3, 2) == 0
    P1, P2 = 1249, 623                                  # T = 2500
    assert lib.pcgmix_potes_narrow_mask_bytes(8, 2500, 2, 1, 2) == 8 * 1 * ((P2 + 3) // 4)
    assert lib.pcgmix_potes_narrow_mask_bytes(8, 2500, 2, 1, 1) == 8 * 2 * (P1 // 4 + 1)
    assert lib.pcgmix_potes_narrow_mask_bytes(8, 13, 2, 1, 2) == 0
    assert lib.pcgmix_potes_narrow_mask_bytes(8, 2500, 3, 2, 2) == 0
    assert 0 < lib.pcgmix_potes_narrow_bwd_blocks(1024, 2500, 2, 1) <= 1024
    assert lib.pcgmix_potes_narrow_bwd_blocks(1, 14, 1, 1) == 1
