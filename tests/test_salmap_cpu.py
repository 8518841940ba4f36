"""``saliency.saliency_map`` without a GPU: the numpy restatement of the kernel (tests/salmap_ref.py)
and the torch-op helpers against goldens recorded from the reference (tests/golden/salmap_*.npz,
make_golden_salmap.py), the C ABI surface, and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, saliency
from conftest import ROOT, golden_files
import salmap_ref as R

CASES = golden_files("salmap_")
ids = lambda p: os.path.basename(p)[:-4]  # noqa: E731


def test_goldens_are_the_three_cases():
    assert [ids(p) for p in CASES] == ["salmap_fullrow", "salmap_ordinary", "salmap_short"]
    short = np.load(CASES[2])["frames"]
    assert np.diff(short[2]).tolist() == [3, 2, 1, 7]          # states shorter than 1, 4, 1, 8 bins
    full = np.load(CASES[0])
    assert full["frames"][1, 4] == full["x"].shape[2]          # a cycle that ends exactly at T


@pytest.mark.parametrize("path", CASES, ids=ids)
def test_restatement_matches_reference(path):
    """|grad| -> ... -> bins in numpy, on the reference's recorded ``data.grad``, against what the
    reference returned: map, bins and values within 2e-6 (float32 convolution in another
    summation order than oneDNN's), boundaries exact."""
    g = np.load(path)
    sal = R.post(g["grad"], g["frames"])
    sal_bins, values, bounds = R.bins(sal, g["frames"])
    assert np.abs(sal - g["saliency"][:, 0]).max() <= 2e-6
    assert np.abs(sal_bins - g["saliency_bins"][:, 0]).max() <= 2e-6
    assert np.abs(values - g["bin_values"]).max() <= 2e-6
    assert np.array_equal(bounds, g["bin_frames"])
    # binning alone, on the reference's own map: its interpolation rule in float32
    sal_bins2, values2, _ = R.bins(g["saliency"][:, 0], g["frames"])
    assert np.abs(sal_bins2 - g["saliency_bins"][:, 0]).max() <= 2e-6
    assert np.abs(values2 - g["bin_values"]).max() <= 2e-6


def test_gaussian_kernel_matches_reference():
    g = np.load(CASES[0])
    k = saliency.gaussian_kernel(n=57, sigma=7.54)
    assert isinstance(k, list) and len(k) == 57 and all(type(v) is float for v in k)
    assert np.array_equal(np.array(k), g["gauss"])
    assert np.array_equal(np.array(k, dtype=np.float32), R.taps(57, 7.54))
    assert len(saliency.gaussian_kernel()) == 11
    assert saliency.SALMAP_GAUSS == (57, 7.54) and saliency.SALMAP_BINS == (1, 4, 1, 8)


@pytest.mark.parametrize("path", CASES, ids=ids)
def test_bin_tensor_matches_reference(path):
    """The torch-op helper on the CPU, state by state on the reference's map, against the
    reference's recorded bins, values and boundaries."""
    g = np.load(path)
    sal = torch.from_numpy(g["saliency"])
    for b, f in enumerate(g["frames"]):
        values, bounds = [], []
        for k, n in enumerate((1, 4, 1, 8)):
            new, v, fr = saliency.bin_tensor(sal[b][:, f[k]:f[k + 1]], n, "cpu")
            assert new.shape == (1, f[k + 1] - f[k]) and new.dtype == torch.float32
            assert torch.equal(new, torch.from_numpy(g["saliency_bins"][b][:, f[k]:f[k + 1]]))
            assert isinstance(v, list) and len(v) == n and len(fr) == n
            values += v
            bounds += [int(x) + int(f[k]) for x in fr]
        assert np.array_equal(np.array(values), g["bin_values"][b])
        assert bounds + [int(f[4])] == g["bin_frames"][b].tolist()


def test_symbol_is_declared_bound_and_exported():
    name = "pcgmix_saliency_map_f32"
    text = open(os.path.join(ROOT, "include", "pcgmix_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b" + name + r"\s*\(", text)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.ABI_VERSION == 25 and "#define PCGMIX_ABI_VERSION 25" in open(
        os.path.join(ROOT, "include", "pcgmix_hip.h")).read()
    for fn in ("saliency_map", "saliency_map_post", "bin_tensor", "gaussian_kernel"):
        assert callable(getattr(saliency, fn))


def test_frames_refusals():
    ok = np.array([[0, 5, 9, 12, 20], [0, 1, 2, 3, 4]])
    assert np.array_equal(saliency.salmap_frames(torch.from_numpy(ok), 2, 20), ok)
    zero = ok.copy()
    zero[1] = [0, 5, 5, 12, 20]                                 # an empty systole
    for bad, B, T in ((zero, 2, 20), (ok, 2, 19), (ok, 3, 20), (ok[:, :4], 2, 20),
                      (np.array([[0, 5, 4, 12, 20]]), 1, 30)):
        with pytest.raises(ValueError):
            saliency.salmap_frames(bad, B, T)


def test_host_tensors_are_refused():
    x = torch.zeros(1, 4, 64)
    fr = np.array([[0, 5, 9, 12, 20]])
    with pytest.raises(ValueError):
        saliency.saliency_map_post(x, fr)
    with pytest.raises(ValueError):
        saliency.saliency_map(x, torch.tensor([[1, 0]]), fr, torch.nn.Identity(), "cpu")
