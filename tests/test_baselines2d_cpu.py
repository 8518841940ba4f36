"""The paper's spectrogram comparison baselines on the host: the reference's ordered 2D if-chain,
the method-string parsers, and the plans against the reference's own recordings
(tests/golden/base2d_*): partners, lambda, rectangles, cuts, segment tables, '(rand)' offsets,
latentmixup's depth and numpy's global stream.  No GPU needed."""
import glob
import os
import random

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import hostprep as H
from cutpaste_ref import replay_pieces

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BASE2D_FILES = sorted(glob.glob(os.path.join(GOLDEN, "base2d_*.npz")))


def load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def set_np_state(g, which):
    tail = g[which + "_tail"]
    np.random.set_state(("MT19937", g[which].astype(np.uint32), int(tail[0]), int(tail[1]), float(tail[2])))


def np_state_is(g, which):
    _, key, pos, has_gauss, cached = np.random.get_state()
    tail = g[which + "_tail"]
    return (np.array_equal(key, g[which]) and pos == int(tail[0]) and has_gauss == int(tail[1])
            and (not has_gauss or cached == tail[2]))


class ProbeNet(torch.nn.Module):
    """The generator's stand-in for ResNet9-2D's first half (tests/golden/make_golden_baselines2d.py):
    subsampling, channel repetition and powers of two only — exact in fp32 on any device."""

    def __init__(self, channels_last=False):
        super().__init__()
        self.channels_last = channels_last

    def _layout(self, h):
        return h.contiguous(memory_format=torch.channels_last) if self.channels_last else h.contiguous()

    def forward(self, x, depth=None, pass_part=None):
        assert pass_part == "first" and depth in (1, 2, 3)
        h = self._layout(x[:, :, ::2, ::2].repeat(1, 3, 1, 1) * 2.0)
        if depth == 1:
            return h
        h = self._layout(h[:, :, 1::2, ::2].repeat(1, 2, 1, 1) * 0.25)
        if depth == 2:
            return h
        return h.flatten(1) * 4.0


def plan_for(g):
    x = g["x"]
    B, C, F, W = x.shape
    return H.make_plan(str(g["method"]), g["labels"], g["frames"], None, int(g["step"]), B, C, is2d=True,
                       n_cols=W, n_freq=F)


def test_fixtures_cover_the_issue_matrix():
    gs = [load(p) for p in BASE2D_FILES]
    names = {H.select_method(str(g["method"]), True) for g in gs}
    assert names == set(H.BASELINE_METHODS_2D)
    assert {int(g["cut"]) for g in gs if "(rand)cutmix" in str(g["method"])} == {1, 2, 3}
    assert {int(g["depth"]) for g in gs if "latentmixup" in str(g["method"])} >= {1, 2, 3}
    assert any(not int(g["fired"]) for g in gs) and any(int(g["raised"]) for g in gs)
    assert any(g["x"].shape[1] == 2 for g in gs) and any(g["x"].shape[2] > g["x"].shape[3] for g in gs)
    assert any(g["x"].shape[2] < g["x"].shape[3] and not int(g["raised"]) for g in gs)
    assert all(os.path.getsize(p) < 1 << 20 for p in BASE2D_FILES)


# ------------------------------------------------------------------ selection and parsing
@pytest.mark.parametrize("method, expect", [
    ("timemask", "timemask"), ("timemask(0.1)+0.5", "timemask"), ("freqmask(0.1)", "freqmask"),
    ("mixup(same)", "mixup"), ("mixup(mix)+0.3", "mixup"), ("latentmixup", "latentmixup"),
    ("latentmixup+0.5", "latentmixup"), ("cutmix", "cutmix"), ("(rand)cutmix", "cutmix"),
    ("durratiocutmix", "durratiocutmix"), ("(rand)durratiocutmix+0.5", "durratiocutmix"),
    # several names in one string: the reference's order decides
    ("timemask(0.1) mixup(same)", "timemask"), ("freqmask cutmix", "freqmask"),
    ("cutmix timemask", "timemask"), ("latentmixup mixup(same)", "latentmixup"),
    ("mixup(same) cutmix", "mixup"), ("mixup cutmix", "cutmix"),       # bare mixup falls through
    ("mixup durratiocutmix", "durratiocutmix"), ("cutmix durratiocutmix", "durratiocutmix"),
    ("freqmask timemask", "timemask"), ("durmixtimemask freqmask", "durmixtimemask"),
    ("timemask durmixfreqmask", "durmixfreqmask"), ("durratiomixup latentmixup", "durratiomixup"),
    ("base", None), ("", None),
])
def test_select_method_follows_the_reference_2d_chain(method, expect):
    assert H.select_method(method, True) == expect


@pytest.mark.parametrize("method", ["mixup", "mixup+0.5", "cutout", "cutout(0.25,0.25)",
                                    "cutout timemask", "cutout(0.25,0.25) mixup(same)", "cutout cutmix"])
def test_bare_mixup_and_cutout_still_raise(method):
    with pytest.raises(NotImplementedError):
        H.select_method(method, True)


@pytest.mark.parametrize("method, expect", [
    ("durmixcutout", "durmixcutout"), ("durmixcutout(0.5,0.6)", "durmixcutout"),
    ("durmixtimemask(0.7)", "durmixtimemask"), ("durmixfreqmask(0.8)+0.5", "durmixfreqmask"),
    ("durratiomixup", "durratiomixup"), ("(saloptenv)durratiomixup", "durratiomixup"),
    ("durmixcutout timemask", "durmixcutout"), ("durratiomixup cutmix", "durratiomixup"),
])
def test_the_existing_2d_names_resolve_as_before(method, expect):
    assert H.select_method(method, True) == expect
    plan_recipe = H.plain_recipe(method, True)
    if expect == "durratiomixup" and "(salopt" not in method:
        assert plan_recipe == ("durratiomixup", H.parse_probability(method), 1.0, 0.0, 0)
    else:
        assert plan_recipe is None


@pytest.mark.parametrize("method", ["timemask", "freqmask(0.1)", "mixup(same)", "mixup(mix)",
                                    "latentmixup", "cutmix", "(rand)cutmix", "durratiocutmix",
                                    "(rand)durratiocutmix"])
def test_no_plain_recipe_and_2d_kinds(method):
    assert H.plain_recipe(method, True) is None
    frames = np.array([[0, 2, 5, 7, 12], [0, 3, 6, 8, 14]], np.int64)
    plan = H.make_plan(method, np.array([0, 0]), frames, None, 3, 2, 1, is2d=True, n_cols=16, n_freq=16)
    assert plan.fired and plan.kind == H.select_method(method, True) + "2d" and plan.is2d
    assert plan.spans is None                               # never the 1D timemask span path
    assert H.MixPlan(fired=True, name="timemask").kind == "timemask"   # the 1D kind is unchanged


def test_mask_rectangles_plain_names_parse_like_the_reference():
    frames = np.array([[0, 2, 5, 7, 12], [0, 3, 6, 8, 30]], np.int64)
    for method, name in (("timemask(0.4)", "timemask"), ("timemask(7)", "timemask"), ("timemask", "timemask"),
                         ("freqmask(0.4)", "freqmask"), ("freqmask(-1)", "freqmask"), ("freqmask", "freqmask")):
        step = 9
        t = 0.2 if "(" not in method else min(max(float(method.split("(")[1][:-1]), 0), 1)
        gap = random.Random(step + 131071).uniform(0, t)
        u = random.Random(step + 13119).uniform(0, 1 - gap)
        r = H.mask_rectangles(method, name, frames, step, 24, 20)
        if name == "timemask":
            assert (r[:, 0] == 0).all() and (r[:, 1] == 24).all()
            assert r[:, 2].tolist() == [int(u * f) for f in frames[:, 4]]
            assert r[:, 3].tolist() == [int((u + gap) * f) for f in frames[:, 4]]
        else:
            h1 = int(24 * u)
            assert (r[:, 0] == h1).all() and (r[:, 1] == min(24, h1 + int(gap * 24))).all()
            assert (r[:, 2] == 0).all() and (r[:, 3] == 20).all()


def test_mask_rectangles_durmix_callers_unchanged():
    """The durmix variants keep their key and their flattened row axis."""
    frames = np.array([[0, 3, 9, 12, 25], [0, 4, 11, 15, 30]], np.int64)
    for method in ("durmixtimemask(0.7)", "durmixfreqmask(0.8)", "durmixcutout(0.5,0.6)"):
        name = H.select_method(method, True)
        r = H.mask_rectangles(method, name, frames, 4, 64, 32)
        gap_t = random.Random(4 + 131071).uniform(0, {"durmixtimemask": 0.7, "durmixcutout": 0.5}.get(name, 0))
        if name != "durmixfreqmask":
            u = random.Random(4 + 13119).uniform(0, 1 - gap_t)
            assert r[:, 2].tolist() == [int(u * f) for f in frames[:, 4]]
        else:
            assert (r[:, 2] == 0).all() and (r[:, 3] == 32).all()


def test_cut_and_depth_draws_match_random():
    from pcgmix_amd import _lib
    lib = _lib.load()
    for step in list(range(0, 200)) + [2**31 + 5, 10**9 + 7]:
        assert 1 + lib.pcgmix_py_randint0(step * 131071, 2) == random.Random(step * 131071).randint(1, 3)
        assert 1 + lib.pcgmix_py_randint0(step, 2) == random.Random(step).randint(1, 3)


@pytest.mark.parametrize("method", ["timemask(0.1)+0.5", "freqmask+0.5", "mixup(same)+0.5", "mixup(mix)+0.5",
                                    "latentmixup+0.5", "cutmix+0.5", "(rand)durratiocutmix+0.5"])
def test_a_rejected_step_draws_nothing(method):
    step = 2                                                # Random(2).uniform(0, 1) = 0.956 >= 0.5
    assert random.Random(step).uniform(0, 1) >= 0.5
    np.random.seed(77)
    before = np.random.get_state()
    py = random.getstate()

    def labels():
        raise AssertionError("labels asked for on a rejected step")

    plan = H.make_plan(method, labels, np.zeros((4, 5), np.int64), None, step, 4, 1, is2d=True,
                       n_cols=8, n_freq=8)
    assert not plan.fired and plan.depth == 0
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and random.getstate() == py


def test_durratiocutmix_refuses_w_not_f_and_frames_beyond_w():
    frames = np.array([[0, 2, 5, 7, 12], [0, 3, 6, 8, 14]], np.int64)
    with pytest.raises(ValueError, match="W == F"):
        H.make_plan("durratiocutmix", np.array([0, 0]), frames, None, 3, 2, 1, is2d=True, n_cols=16, n_freq=20)
    with pytest.raises(ValueError):
        H.make_plan("cutmix", np.array([0, 0]), frames, None, 3, 2, 1, is2d=True, n_cols=12, n_freq=20)
    with pytest.raises(ValueError, match="cut at column"):
        H.make_plan("cutmix", np.array([0, 0]), frames, None, 3, 2, 1, is2d=True, n_cols=16, n_freq=5)


# ------------------------------------------------------------------ plans against the recordings
@pytest.mark.parametrize("path", BASE2D_FILES, ids=os.path.basename)
def test_plan_matches_the_reference(path):
    g = load(path)
    method = str(g["method"])
    x = g["x"]
    set_np_state(g, "np_before")
    py = random.getstate()
    if int(g["raised"]):
        with pytest.raises(ValueError):
            plan_for(g)
        return
    plan = plan_for(g)
    assert random.getstate() == py
    assert np_state_is(g, "np_after")
    assert plan.fired == bool(int(g["fired"]))
    if not plan.fired:
        assert int(g["same_object"]) and g["mix"].size == 0 and int(g["cut"]) == -1
        return
    kind = plan.kind
    if kind in ("timemask2d", "freqmask2d"):
        assert int(g["same_object"])
        want = x.copy()
        for b, (r0, r1, c0, c1) in enumerate(plan.zero_rect):
            want[b, :, r0:r1, c0:c1] = 0
        assert np.array_equal(want, g["y"])
        return
    assert np.array_equal(plan.mix, g["mix"])
    assert int(g["cut"]) == (-1 if plan.cut is None else plan.cut)
    if kind in ("mixup2d", "latentmixup2d"):
        assert plan.lam64 == float(g["lam"]) and plan.lam32 == np.float32(g["lam"])
        lam = plan.lam32
        if kind == "latentmixup2d":
            assert plan.depth == int(g["depth"])
            h = ProbeNet()(torch.from_numpy(x), depth=plan.depth, pass_part="first").numpy()
        else:
            h = x
        assert np.array_equal(h * lam + h[plan.mix] * (np.float32(1) - lam), g["y"])
        if plan.mix_all:
            t = np.eye(2, dtype=np.float32)[g["labels"]]          # torch: int64 * float32 -> float32
            lt = np.full((x.shape[0], 1), lam, np.float32)
            assert np.array_equal(t * lt + t[plan.mix] * (np.float32(1) - lt), g["target_out"])
        return
    assert np.isnan(g["lam"])                               # cutmix draws no lambda
    assert plan.segs.shape == (x.shape[0], 5, 4)
    segs = plan.segs
    assert (segs[:, 0, 0] == 0).all() and (segs[:, :-1, 1] == segs[:, 1:, 0]).all()
    assert (segs[:, -1, 1] == (plan.out_cols if plan.seg_axis == 0 else x.shape[2])).all()
    assert np.array_equal(replay_pieces(x, segs, plan.mix, plan.seg_axis, plan.out_cols), g["y"])
    if "(rand)" in method and "durratiocutmix" in method:
        assert plan.seg_axis == 1
        off = H.rand_offsets(g["frames"], plan.mix, int(g["step"]))
        f1, f2 = g["frames"], g["frames"][plan.mix]
        for b in range(x.shape[0]):
            for k, seg in ((1, 1), (3, 3)):
                gap = (f2[b, k + 1] - f2[b, k]) - (f1[b, k + 1] - f1[b, k])
                assert off[b, k] == random.Random(int(g["step"])).randint(0, abs(gap))
                lo, hi, src, sh = segs[b, seg]
                if gap >= 0:
                    assert (lo, hi, sh) == (f1[b, k], f1[b, k + 1], f2[b, k] + off[b, k] - f1[b, k])
                else:
                    assert (lo, sh) == (f1[b, k] + off[b, k], f2[b, k] - f1[b, k] - off[b, k])
