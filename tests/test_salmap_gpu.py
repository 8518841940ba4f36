"""``saliency.saliency_map`` on the GPU: the kernel (``saliency_map_post``) on the reference's
recorded gradients and at its edges, and the whole call end to end (tests/golden/salmap_*.npz,
recorded from the reference by make_golden_salmap.py; tests/salmap_ref.py restates the kernel)."""
import argparse
import os

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import models, saliency, train_model
from conftest import GOLDEN, golden_files
import salmap_ref as R

pytestmark = pytest.mark.gpu
CASES = golden_files("salmap_")
ids = lambda p: os.path.basename(p)[:-4]  # noqa: E731


def run_post(grad, frames, device, **kw):
    out = saliency.saliency_map_post(torch.from_numpy(grad).to(device), frames, **kw)
    assert all(t.device.type == "cuda" for t in out)
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.float32, torch.int32]
    return [t.cpu().numpy() for t in out]


def check_support(sal_bins, frames):
    """No element of sal_bins outside [f[0], f[4]) is non-zero."""
    t = np.arange(sal_bins.shape[1])[None, :]
    outside = (t < frames[:, 0:1]) | (t >= frames[:, 4:5])
    assert not sal_bins[outside].any()


@pytest.mark.parametrize("path", CASES, ids=ids)
def test_kernel_on_the_reference_gradient(path, device):
    g = np.load(path)
    sal, sal_bins, values, bounds = run_post(g["grad"], g["frames"], device)
    B, _, T = g["grad"].shape
    assert sal.shape == sal_bins.shape == (B, T) and values.shape == (B, 14) and bounds.shape == (B, 15)
    errs = (np.abs(sal - g["saliency"][:, 0]).max(), np.abs(sal_bins - g["saliency_bins"][:, 0]).max(),
            np.abs(values - g["bin_values"]).max())
    print("max |kernel - reference|: map %.3g, bins %.3g, values %.3g" % errs)
    # the bound test_saliency_post_matches_reference holds the same convolution to: only the
    # summation order against oneDNN differs
    assert max(errs) <= 2e-6
    assert np.array_equal(bounds.astype(np.int64), g["bin_frames"])
    assert (sal.min(1) == 0.0).all() and (sal.max(1) == 1.0).all()
    check_support(sal_bins, g["frames"])


def random_frames(rs, B, T, end=None):
    """(B,5) boundaries from 0 with four non-empty states that fit in T."""
    cuts = np.stack([np.sort(rs.choice(np.arange(1, T if end is None else end), 3, replace=False))
                     for _ in range(B)])
    last = np.full((B, 1), T if end is None else end)
    if end is None:
        last = cuts[:, 2:3] + 1 + rs.randint(0, T - cuts[:, 2:3])
    return np.concatenate([np.zeros((B, 1), int), cuts, last], axis=1).astype(np.int64)


EDGES = {
    "taps-longer-than-row": dict(shape=(1, 1, 40)),
    "odd-T": dict(shape=(3, 4, 61)),
    "cycle-ends-at-T": dict(shape=(2, 2, 64), end=64),
    "zero-row-and-short-states": dict(shape=(5, 4, 2500)),
    "other-bins-and-taps": dict(shape=(3, 4, 333), bins=(2, 3, 5, 7), gauss=(19, 2.54)),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_kernel_edges_against_the_restatement(name, device):
    e = EDGES[name]
    B, C, T = e["shape"]
    bins, gauss = e.get("bins", R.BINS), e.get("gauss", R.GAUSS)
    rs = np.random.RandomState(len(name))
    grad = rs.standard_normal((B, C, T)).astype(np.float32)
    frames = random_frames(rs, B, T, e.get("end"))
    if name == "zero-row-and-short-states":
        grad[1] = 0
        frames[3] = np.cumsum([0, 3, 2, 1, 7]) + 11            # and a cycle that does not start at 0
    if name == "cycle-ends-at-T":
        assert (frames[:, 4] == T).all()
    sal, sal_bins, values, bounds = run_post(grad, frames, device, bins=bins, gauss=gauss)
    want = R.post(grad, frames, gauss)
    want_bins, want_values, want_bounds = R.bins(want, frames, bins)
    N = sum(bins)
    assert values.shape == (B, N) and bounds.shape == (B, N + 1)
    errs = (np.abs(sal - want).max(), np.abs(sal_bins - want_bins).max(), np.abs(values - want_values).max())
    print("max |kernel - restatement|: map %.3g, bins %.3g, values %.3g" % errs)
    assert max(errs) <= 2e-6
    assert np.array_equal(bounds.astype(np.int64), want_bounds)
    # the bins are the kernel's own map binned: the restatement's rule on the RETURNED map
    own_bins, own_values, _ = R.bins(sal, frames, bins)
    assert np.abs(sal_bins - own_bins).max() <= 2e-6 and np.abs(values - own_values).max() <= 2e-6
    check_support(sal_bins, frames)
    assert np.isfinite(sal).all() and np.isfinite(sal_bins).all() and np.isfinite(values).all()
    if name == "zero-row-and-short-states":
        assert not sal[1].any() and not sal_bins[1].any() and not values[1].any()
        live = np.arange(B) != 1
        assert (sal[live].min(1) == 0.0).all() and (sal[live].max(1) == 1.0).all()
    again = run_post(grad, frames, device, bins=bins, gauss=gauss)
    for a, b in zip((sal, sal_bins, values, bounds), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))       # equal bits


def golden_potes(device):
    sd = np.load(GOLDEN + "/potes_state_seed1234.npz")
    model = models.CNN_potes_TS(4, 2, "PhysioNet")
    model.load_state_dict({k: torch.from_numpy(sd[k]) for k in sd.files})
    return model.to(device)


def check_return_types(res, B, T, classes, N, device):
    sal, sal_bins, out, values, bounds = res
    assert sal.shape == (B, 1, T) and sal.dtype == torch.float32 and sal.device == device
    assert sal_bins.shape == (B, 1, T) and sal_bins.dtype == torch.float32 and sal_bins.device.type == "cpu"
    assert out.shape == (B, classes) and out.device == device and not out.requires_grad
    assert isinstance(values, list) and len(values) == B
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape == (N,) for v in values)
    assert isinstance(bounds, list) and len(bounds) == B
    assert all(isinstance(v, np.ndarray) and v.dtype == np.int64 and v.shape == (N + 1,) for v in bounds)


@pytest.mark.parametrize("path", CASES, ids=ids)
def test_saliency_map_end_to_end_potes(path, device):
    g = np.load(path)
    model = golden_potes(device).train()
    data = torch.from_numpy(g["x"]).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(g["labels"]), 2).to(device)
    res = saliency.saliency_map(data, tgt, torch.from_numpy(g["frames"]), model, device)
    B, C, T = data.shape
    check_return_types(res, B, T, 2, 14, device)
    sal, sal_bins, out, values, bounds = res
    assert not model.training                                   # left in eval mode (saliency.py:137)
    assert data.grad is None and not data.requires_grad         # documented deviation
    errs = (np.abs(sal.cpu().numpy() - g["saliency"]).max(), np.abs(sal_bins.numpy() - g["saliency_bins"]).max(),
            np.abs(np.stack(values) - g["bin_values"]).max(), np.abs(out.cpu().numpy() - g["out"]).max())
    print("max |saliency_map - reference|: map %.3g, bins %.3g, values %.3g, logits %.3g" % errs)
    # 1e-5: what test_saliency_gpu holds this model's input-gradient chain to; 1e-4 on the logits:
    # test_models_match_reference_logits_on_hip_path
    assert max(errs[:3]) <= 1e-5 and errs[3] <= 1e-4
    assert np.array_equal(np.stack(bounds), g["bin_frames"])
    with torch.no_grad():
        assert torch.equal(out, model(data))
    # DataParallel is looked through
    res2 = saliency.saliency_map(data, tgt, g["frames"], torch.nn.DataParallel(model, device_ids=[device.index]),
                                 device)
    assert torch.equal(res2[0], sal) and torch.equal(res2[1], sal_bins) and torch.equal(res2[2], out)


@pytest.mark.parametrize("name", ["Potes0.1", "PotesBig64and32", "resnet9-5k"])
def test_saliency_map_other_models(name, device):
    """The call runs on the autograd paths (other Potes widths, ResNet9-1D); what it returns is
    consistent: bins, values and boundaries are the restatement's binning of the returned map.
    (No claim against the reference for ResNet9: MIOpen's default backward is not reproducible.)"""
    from pcgmix_amd import synthetic
    B, C, T = 4, 4, 2500
    torch.manual_seed(3)
    model = train_model.build_model(argparse.Namespace(dataset="PhysioNet", model=name, num_channels=C,
                                                       num_classes=2, sig_len=T)).to(device)
    x, frames, labels, _ = synthetic.make_batch(B, C, T, seed=23)
    data = torch.from_numpy(x).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(device)
    res = saliency.saliency_map(data, tgt, torch.from_numpy(frames), model, device)
    check_return_types(res, B, T, 2, 14, device)
    sal, sal_bins, out, values, bounds = res
    assert not model.training and data.grad is None
    s = sal[:, 0].cpu().numpy()
    assert np.isfinite(s).all() and (s.min(1) == 0.0).all() and (s.max(1) == 1.0).all()
    want_bins, want_values, want_bounds = R.bins(s, frames)
    assert np.abs(sal_bins[:, 0].numpy() - want_bins).max() <= 2e-6
    assert np.abs(np.stack(values) - want_values).max() <= 2e-6
    assert np.array_equal(np.stack(bounds), want_bounds)
    with torch.no_grad():
        assert torch.equal(out, model(data))


def test_refusals(device):
    g = np.load(CASES[1])
    model = golden_potes(device)
    data = torch.from_numpy(g["x"]).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(g["labels"]), 2).to(device)
    frames = g["frames"]
    beyond = frames.copy()
    beyond[0, 4] = data.shape[2] + 1
    empty = frames.copy()
    empty[1, 2] = empty[1, 1]
    for d, f in ((data.double(), frames), (data.transpose(1, 2).contiguous().transpose(1, 2), frames),
                 (data, beyond), (data, empty)):
        with pytest.raises(ValueError):
            saliency.saliency_map(d, tgt, f, model, device)
        with pytest.raises(ValueError):
            saliency.saliency_map_post(d, f)
    for kw in (dict(gauss=(56, 7.0)), dict(gauss=(257, 7.0)), dict(gauss=(57, 0.0)), dict(bins=(1, 4, 1)),
               dict(bins=(0, 4, 1, 8)), dict(bins=(16, 16, 16, 17))):
        with pytest.raises(ValueError):
            saliency.saliency_map_post(data, frames, **kw)
    lib = pcgmix_amd._lib.load()                                # and the C entry point itself
    import ctypes
    z = torch.zeros(64, device=device)
    nb = np.array([1, 4, 1, 8], dtype=np.int32)
    args = lambda ksize, nbp, T: (z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),  # noqa: E731
                                  z.data_ptr(), ksize, ctypes.c_double(7.54), nbp, 1, 1, T, None)
    assert lib.pcgmix_saliency_map_f32(*args(56, nb.ctypes.data, 8)) != 0           # even tap count
    assert lib.pcgmix_saliency_map_f32(*args(57, None, 8)) != 0                     # no bin counts
    assert lib.pcgmix_saliency_map_f32(*args(57, nb.ctypes.data, 20000)) != 0       # row beyond the LDS
