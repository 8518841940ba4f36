"""Host logic of the cut-and-paste family, durmixrespscale and bare cutout: the recipe function
against the reference's if-chain, and ``hostprep.cutpaste_plan`` against the reference's recordings
(tests/golden/cutpaste_*, cutout2d_*): gate, partners, cut, and the plan's tables replayed in numpy
(tests/cutpaste_ref.py) reproduce the recorded output bit for bit; numpy's global stream ends where
the reference leaves it."""
import os
import random

import numpy as np
import pytest

import pcgmix_amd  # noqa: F401
from pcgmix_amd import hostprep as H
from cutpaste_ref import (CUTOUT2D_FILES, CUTPASTE_FILES, assert_np_state, load, replay_cutpaste,
                          replay_plan, set_np_state)


@pytest.mark.parametrize("method,expect", [
    ("durmixrespscale", "durmixrespscale"), ("durmixrespscale(12,20)+0.5", "durmixrespscale"),
    ("(rand)durmixrespscale timemask", "durmixrespscale"),          # the chain's first branch
    ("respiratoryscale labelcutmix", None), ("labelcutmix timewarp", None),
    ("labelcutmix timemask(0.1)", None), ("labelcutmix magnitudewarp", None),
    ("durratiocutmix", "durratiocutmix"), ("(rand)durratiocutmix+0.3", "durratiocutmix"),
    ("durratiocutmix(plus)", None), ("durratiocutmix(plusplus)", None), ("(UMC-subset)durratiocutmix", None),
    ("(UMC)durratiocutmix", None), ("durratiocutmix gaussiannoise", None),
    ("wav-durratiocutmix", "wav-durratiocutmix"), ("wav-durratiocutmix timewarp", "wav-durratiocutmix"),
    ("durratiomixup wav-durratiocutmix", None),
    ("lengthcutmix(5bins)", "lengthcutmix"), ("lengthcutmix labelcutmix", "lengthcutmix"),
    ("datasetcutmix", "datasetcutmix"), ("wavcutmix", "wavcutmix"), ("durratiowavcutmix", None),
    ("labelcutmix", "labelcutmix"), ("(rand)labelcutmix(smooth)(cutout)", "labelcutmix"),
    ("lc-nointrusion labelcutmix", None), ("labelcutmix swapsysdia", "labelcutmix"),
    ("mixup labelcutmix", "labelcutmix"),                            # a bare mixup falls through (:829-862)
    ("mixup(same) labelcutmix", None), ("mixup(mix) cutout", None),
    ("swapsysdia", None), ("cont-cutmix", None), ("saliency-cutmix", None), ("cutmix", None),
    ("cutmix(ch)", None), ("s1s2mask", None), ("lc-nointrusion", None),
    ("latentmixup cutout", None), ("latentmixup", None),
    ("cutout", "cutout"), ("cutout(0.25,0.25)", "cutout"), ("cutout(ch)+0.5", "cutout"),
    ("saliency-cutout", None), ("manifold-cutout", None), ("manifold-cutout(ch)", None),
    ("cutmix cutout", None),                                         # plain cutmix comes first (:1508)
    ("gaussiannoise", None), ("none", None), ("", None),
])
def test_recipe_follows_the_reference_chain_1d(method, expect):
    assert H.cutpaste_recipe(method, False) == expect
    if expect is not None:
        assert H.latent_recipe(method) is None


@pytest.mark.parametrize("method,expect", [
    ("cutout", "cutout"), ("cutout(0.25,0.25)+0.5", "cutout"), ("cutout timemask", "cutout"),
    ("freqmask cutout", "cutout"), ("durmixcutout(0.2,0.2)", None), ("durmixtimemask cutout", None),
    ("durratiomixup cutout", None), ("timemask", None), ("cutmix", None), ("none", None),
])
def test_recipe_follows_the_reference_chain_2d(method, expect):
    assert H.cutpaste_recipe(method, True) == expect


@pytest.mark.parametrize("method", ["durmixrespscale", "labelcutmix", "durratiocutmix", "wavcutmix",
                                    "lengthcutmix", "datasetcutmix", "cutout", "cutout(ch)", "cutmix",
                                    "swapsysdia", "manifold-cutout", "durratiocutmix gaussiannoise"])
def test_select_method_raises_where_it_did(method):
    with pytest.raises(NotImplementedError):
        H.select_method(method, False)


def test_select_method_2d_cutout_still_raises_and_served_names_are_untouched():
    with pytest.raises(NotImplementedError):
        H.select_method("cutout(0.25,0.25)", True)
    with pytest.raises(NotImplementedError):
        H.select_method("wav-durratiocutmix timewarp", False)
    assert H.select_method("labelcutmix timewarp", False) == "timewarp"
    assert H.select_method("timemask cutout", False) == "timemask"


def test_parsers():
    assert H.parse_durmixrespscale("durmixrespscale") == (12 / 60, 20 / 60)
    assert H.parse_durmixrespscale("(rand)durmixrespscale(8.5,30)+0.5") == (8.5 / 60, 30 / 60)
    with pytest.raises(ValueError):
        H.parse_durmixrespscale("durmixrespscale(12,20.5)")        # int('20.5'), as the reference
    tab = H.sigmoid_table()
    assert tab.shape == (10, 20) and tab.dtype == np.float64
    for ov in range(1, 11):
        ref = np.array([1.0 / (1.0 + np.exp(-v)) for v in np.linspace(-8, 8, ov * 2)])
        ref[0], ref[-1] = 0, 1
        assert np.array_equal(tab[ov - 1, :2 * ov], ref) and not tab[ov - 1, 2 * ov:].any()


def test_fixture_set():
    methods = [load(p)["method"] for p in CUTPASTE_FILES]
    assert len(CUTPASTE_FILES) >= 60 and len(CUTOUT2D_FILES) >= 10
    for name in H.CUTPASTE_METHODS_1D:
        assert any(H.cutpaste_recipe(m, False) == name for m in methods), name
    biggest = max(os.path.getsize(p) for p in CUTPASTE_FILES + CUTOUT2D_FILES)
    assert biggest <= 242076                                      # the largest base1d_*.npz


def make_plan(g, is2d=False):
    x = g["x"]
    if is2d:
        B, C, F, W = x.shape
        return H.cutpaste_plan(g["method"], None, g["frames"], None, g["step"], B, C, W, is2d=True,
                               n_freq=F, n_cols=W)
    B, C, T = x.shape
    return H.cutpaste_plan(g["method"], g["labels"], g["frames"], g["wav"], g["step"], B, C, T,
                           batch_size=g["batch_size"], sample_rate=g["sample_rate"])


@pytest.mark.parametrize("path", CUTPASTE_FILES + CUTOUT2D_FILES, ids=os.path.basename)
def test_plan_matches_the_reference(path):
    g = load(path)
    is2d = os.path.basename(path).startswith("cutout2d")
    set_np_state(g)
    py = random.getstate()
    plan = make_plan(g, is2d)
    assert random.getstate() == py
    assert_np_state(g)
    assert plan.fired == bool(g["fired"])
    if not plan.fired:
        assert g["same_object"] == 1 and np.array_equal(g["y"], g["x"])
        return
    name = H.cutpaste_recipe(g["method"], is2d)
    if plan.kind == "cutpaste":
        assert np.array_equal(plan.mix, g["mix"])
        assert (plan.cut if plan.cut is not None else -1) == g["cut"]
    else:
        assert g["mix"].size == 0 and g["cut"] == -1
    if plan.kind == "mixscale":
        assert plan.lam64 == float(g["lam"])
    assert g["same_object"] == int(name == "cutout")
    y = replay_plan(plan, g["x"], g["frames"], H.sigmoid_table())
    assert np.array_equal(y, g["y"])
    assert np.array_equal(g["target_out"], np.eye(2, dtype=np.int64)[g["labels"]])


def test_goldens_cover_small_overlaps_clipping_and_every_cut():
    ovs, clipped, cuts = set(), 0, set()
    for p in CUTPASTE_FILES:
        g = load(p)
        if not g["fired"] or g["cut"] < 0:
            continue
        cuts.add(g["cut"])
        plan = make_plan(g)
        if plan.junctions is not None:
            ovs.update(int(v) for v in plan.junctions[:, 2])
        f1, f2, c = g["frames"], g["frames"][g["mix"]], g["cut"]
        clipped += int((f1[:, c] + f2[:, 4] - f2[:, c] > g["x"].shape[2]).sum())
    assert cuts == {1, 2, 3} and clipped > 0
    assert min(ovs) < 10 and max(ovs) == 10


def test_rejected_step_draws_nothing():
    x, frames, labels, wav = pcgmix_amd.synthetic.make_batch(6, 2, 320, seed=3, rate_scale=0.2)
    for method in ("durmixrespscale+0.5", "labelcutmix+0.5", "cutout+0.5"):
        np.random.seed(7)
        before = np.random.get_state()[1].copy()
        asked = []
        plan = H.cutpaste_plan(method, lambda: asked.append(1) or labels, frames, wav, 2, 6, 2, 320,
                               batch_size=6, sample_rate=1000)
        assert not plan.fired and not asked and np.array_equal(np.random.get_state()[1], before)


def test_only_durmixrespscale_touches_numpys_stream():
    x, frames, labels, wav = pcgmix_amd.synthetic.make_batch(6, 2, 320, seed=3, rate_scale=0.2)
    for method in ("labelcutmix(smooth)(cutout)", "(rand)durratiocutmix", "lengthcutmix", "cutout(ch)"):
        np.random.seed(7)
        before = np.random.get_state()
        H.cutpaste_plan(method, labels, frames, wav, 3, 6, 2, 320, batch_size=6, sample_rate=1000)
        after = np.random.get_state()
        assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    np.random.seed(3)                      # get_lambda(alpha=1, random_seed=step)
    np.random.beta(1, 1)
    want = np.random.get_state()
    np.random.seed(7)
    H.cutpaste_plan("durmixrespscale", labels, frames, wav, 3, 6, 2, 320, sample_rate=1000)
    got = np.random.get_state()
    assert np.array_equal(want[1], got[1]) and want[2:] == got[2:]


def test_malformed_input_is_refused_on_the_host():
    x, frames, labels, wav = pcgmix_amd.synthetic.make_batch(6, 2, 320, seed=3, rate_scale=0.2)
    bad = frames.copy()
    bad[:, 0] = 1
    with pytest.raises(ValueError, match="must be 0"):
        H.cutpaste_plan("labelcutmix", labels, bad, wav, 3, 6, 2, 320)
    with pytest.raises(ValueError, match="signal length"):
        H.cutpaste_plan("durratiocutmix", labels, frames, wav, 3, 6, 2, int(frames.max()) - 1)
    with pytest.raises(ValueError, match="batch size"):
        H.cutpaste_plan("labelcutmix", labels[:5], frames, wav, 3, 6, 2, 320)
    with pytest.raises(ValueError, match="batch_size"):
        H.cutpaste_plan("lengthcutmix", labels, frames, wav, 3, 6, 2, 320)
    with pytest.raises(ValueError, match="sample_rate"):
        H.cutpaste_plan("durmixrespscale", labels, frames, wav, 3, 6, 2, 320)
    with pytest.raises(NotImplementedError, match="sameCVD"):
        H.cutpaste_plan("(sameCVD)durmixrespscale", labels, frames, wav, 3, 6, 2, 320, sample_rate=1000)
    with pytest.raises(ValueError):
        H.cutpaste_plan("timemask", labels, frames, wav, 3, 6, 2, 320)


def test_smooth_with_an_empty_part_raises_index_error():
    """ov == 0: the reference's sigmoid(0) indexes an empty array."""
    frames = np.array([[0, 0, 0, 4, 9], [0, 0, 0, 3, 8]], dtype=np.int64)       # f[cut=2] == 0
    labels = np.zeros(2, dtype=np.int64)
    with pytest.raises(IndexError):
        H.cutpaste_plan("labelcutmix(smooth)", labels, frames, ("a", "a"), 3, 2, 1, 16)
    plan = H.cutpaste_plan("labelcutmix", labels, frames, ("a", "a"), 3, 2, 1, 16)   # without: fine
    assert plan.fired and plan.junctions is None


def test_replay_range_checks_give_zeros():
    """Tables whose sources point outside the row: zeros there (what the kernel's checks do)."""
    x = np.arange(1, 2 * 1 * 8 + 1, dtype=np.float32).reshape(2, 1, 8)
    segs = np.zeros((2, 5, 4), dtype=np.int32)
    segs[:, 0] = (0, 4, 0, -2)            # own at t-2: t = 0, 1 outside
    segs[:, 1] = (4, 8, 1, 3)             # partner at t+3: t = 5, 6, 7 outside
    segs[:, 2:, :2] = 8
    y = replay_cutpaste(x, segs, np.array([1, 0]))
    assert np.array_equal(y[0, 0], [0, 0, 1, 2, 16, 0, 0, 0])
