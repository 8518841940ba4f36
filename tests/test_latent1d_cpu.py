"""1D latentmixup on the host: which method strings reach the reference's branch
(augmentations.py:1472-1506) and the host draws — gate, partners, depth, lambda, numpy's global
stream — against the reference's own recordings (tests/golden/latent1d_*).  No GPU needed."""
import glob
import os

import numpy as np
import pytest

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, hostprep as H

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "latent1d_*.npz")))


def load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def set_np_state(g, which):
    tail = g[which + "_tail"]
    np.random.set_state(("MT19937", g[which].astype(np.uint32), int(tail[0]), int(tail[1]), float(tail[2])))


def assert_np_state(g, which="np_after"):
    _, key, pos, has_gauss, cached = np.random.get_state()
    tail = g[which + "_tail"]
    assert np.array_equal(key, g[which]) and pos == int(tail[0])
    assert has_gauss == int(tail[1]) and (not has_gauss or cached == tail[2])


@pytest.mark.parametrize("method, p", [
    ("latentmixup", 1.0), ("latentmixup+0.5", 0.5), ("latentmixup(same)", 1.0),
    ("latentmixup(same)+0.25", 0.25),
    # names whose branch comes later in the reference's chain do not take it away
    ("latentmixup cutmix", 1.0), ("latentmixup cutout+0.8", 0.8), ("manifold-cutmix latentmixup", 1.0),
])
def test_latent_recipe_reaches_the_branch(method, p):
    assert H.latent_recipe(method) == (p,)
    assert H.soft_targets(method) is False                      # targets are not blended (:1506)


@pytest.mark.parametrize("method", [
    "latentmixup timewarp", "durratiomixup latentmixup", "latentmixup timemask(0.2)",
    "latentmixup respiratoryscale", "latentmixup gaussiannoise", "latentmixup durmixmagwarp(0.2,4)",
    "latentmixup magnitudewarp", "latentmixup durratiocutmix", "latentmixup swapsysdia",
    "latentmixup saliency-cutmix", "latentmixup labelcutmix", "mixup(same)", "mixup(mix)", "base",
    "durratiomixup", "",
])
def test_latent_recipe_leaves_earlier_branches_alone(method):
    assert H.latent_recipe(method) is None


def test_select_method_keeps_its_contract():
    for m in ("latentmixup", "latentmixup(same)", "latentmixup cutmix"):
        with pytest.raises(NotImplementedError):
            H.select_method(m, False)
    assert H.select_method("latentmixup timewarp", False) == "timewarp"
    with pytest.raises(NotImplementedError):
        H.select_method("latentmixup gaussiannoise", False)
    assert H.select_method("latentmixup", True) == "latentmixup"          # the 2D chain serves it


def test_depth_draw_is_pythons_randint():
    import random
    for step in list(range(40)) + [12345, 2**31]:
        assert H.latent_depth("resnet9", step) == random.Random(step).randint(1, 3)
        assert H.latent_depth("Potes", step) == 1
    # the reference's documented sequence for steps 0..11
    assert [H.latent_depth("resnet9", s) for s in range(12)] == [2, 1, 1, 1, 1, 3, 3, 2, 1, 2, 3, 2]
    for name in ("FCN", "ResCNN", "Singstad", None, "potes"):
        with pytest.raises(NotImplementedError):
            H.latent_depth(name, 0)
        with pytest.raises(NotImplementedError):
            H.latent_plan("latentmixup", name, np.zeros(4, np.int64), 0, 4)


def test_goldens_cover_the_cases():
    assert len(FILES) >= 8
    g = [load(f) for f in FILES]
    assert {int(c["depth"]) for c in g if str(c["model"]) == "resnet9"} == {0, 1, 2, 3}
    assert {int(c["fired"]) for c in g if "+0.5" in str(c["method"])} == {0, 1}
    assert any(str(c["method"]) == "latentmixup cutmix" for c in g)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_host_plan_against_the_reference(path):
    g = load(path)
    method, step, model = str(g["method"]), int(g["step"]), str(g["model"])
    B = g["x"].shape[0]
    asked = []

    def labels():
        asked.append(1)
        return g["labels"]
    set_np_state(g, "np_before")
    plan = H.latent_plan(method, model, labels, step, B)
    assert plan.fired == bool(g["fired"])
    assert_np_state(g)                                           # bit-exact, fired or not
    if not plan.fired:
        assert_np_state(g, "np_before")                          # untouched
        assert not asked and int(g["depth"]) == 0 and int(g["same_object"]) == 1
        return
    assert np.array_equal(plan.mix, g["mix"]) and plan.mix.dtype == np.int64
    assert plan.depth == int(g["depth"])
    assert plan.lam64 == float(g["lam"])                         # float64, exact
    assert plan.lam32 == np.float32(g["lam"])
    assert np.array_equal(g["target_out"], np.eye(2, dtype=np.int64)[g["labels"]])   # targets unchanged


def test_latent_plan_refuses_other_methods():
    with pytest.raises(ValueError):
        H.latent_plan("mixup(same)", "Potes", np.zeros(4, np.int64), 0, 4)
    with pytest.raises(ValueError):
        H.latent_plan("latentmixup", "Potes", np.zeros(3, np.int64), 0, 4)     # labels vs batch


def test_abi_exports_the_latent_entry_point():
    lib = _lib.load()
    assert lib.pcgmix_abi_version() == _lib.ABI_VERSION >= 20
    assert "pcgmix_potes_head_loss_latent_fwd_f32" in _lib.SIGNATURES
    assert lib.pcgmix_potes_head_loss_latent_fwd_f32 is not None


def test_pack_partners_is_the_permutation_and_its_inverse():
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for B in (0, 1, 2, 7, 256):
        mix = rng.permutation(B).astype(np.int64)
        out = np.full(2 * B, -7, dtype=np.int32)
        assert lib.pcgmix_pack_partners_i32(mix.ctypes.data, B, out.ctypes.data) == 0
        assert np.array_equal(out[:B], mix) and np.array_equal(out[B:][mix], np.arange(B))
    out = np.empty(8, dtype=np.int32)
    for bad, err in ((np.array([0, 0, 1, 2]), -4), (np.array([0, 1, 2, 4]), -3), (np.array([-1, 1, 2, 3]), -3)):
        bad = bad.astype(np.int64)
        assert lib.pcgmix_pack_partners_i32(bad.ctypes.data, 4, out.ctypes.data) == err
    assert lib.pcgmix_pack_partners_i32(None, 4, out.ctypes.data) != 0
