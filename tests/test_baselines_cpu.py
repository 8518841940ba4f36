"""The paper's 1D comparison baselines on the host: the reference's ordered if-chain, the
method-string parsers, the plans against the reference's own recordings (tests/golden/base1d_*),
and the host twins of the time-warp kernel (numpy's interp, one time-warped row) against numpy
and scipy.  No GPU needed."""
import glob
import os
import random

import numpy as np
import pytest

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, hostprep as H

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BASE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "base1d_*.npz")))


def load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def set_np_state(g, which):
    tail = g[which + "_tail"]
    np.random.set_state(("MT19937", g[which].astype(np.uint32), int(tail[0]), int(tail[1]), float(tail[2])))


def assert_np_state(g):
    _, key, pos, has_gauss, cached = np.random.get_state()
    tail = g["np_after_tail"]
    assert np.array_equal(key, g["np_after"]) and pos == int(tail[0])
    assert has_gauss == int(tail[1]) and (not has_gauss or cached == tail[2])


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


# ------------------------------------------------------------------ selection and parsing
@pytest.mark.parametrize("method, expect", [
    ("mixup(same)", "mixup"), ("mixup(mix)+0.5", "mixup"), ("(samePCG)mixup(same)", "mixup"),
    ("(sameCVD)mixup(same)", "mixup"),            # selectors refuse only on the splices
    ("magnitudewarp", "magnitudewarp"), ("magnitudewarp(0.2,4)+0.3", "magnitudewarp"),
    ("timewarp(0.05,4)", "timewarp"), ("timemask(0.1)", "timemask"),
    ("respiratoryscale(12,20)", "respiratoryscale"),
    # several names in one string: the reference's order decides
    ("timemask mixup(same)", "timemask"), ("respiratoryscale timemask", "respiratoryscale"),
    ("mixup(same) durratiomixup", "durratiomixup"),   # 'durratiomixup' excludes the mixup branch
    ("mixup(same) durmixmagwarp", "mixup"), ("durmixmagwarp timewarp", "durmixmagwarp"),
    ("timewarp magnitudewarp", "timewarp"), ("mixup timewarp", "timewarp"),  # bare mixup falls through
    ("magnitudewarp gaussiannoise", "magnitudewarp"),
    ("durratiomixup", "durratiomixup"), ("durmixmagwarp(0.2,4)", "durmixmagwarp"),
    ("base", None),
])
def test_select_method_follows_the_reference_chain(method, expect):
    assert H.select_method(method, False) == expect


@pytest.mark.parametrize("method", [
    "gaussiannoise(25,40)", "latentmixup", "durmixrespscale", "durmixrespscale(12,20)", "cutmix",
    "mixup", "mixup+0.5", "durmixrespscale timewarp", "wav-durratiocutmix timewarp",
    "(sameCVD)durratiomixup", "(closestknn=3)durmixmagwarp", "latentmixup(same)",
])
def test_out_of_scope_methods_still_raise(method):
    with pytest.raises(NotImplementedError):
        H.select_method(method, False)


def test_2d_cutout_still_raises():
    with pytest.raises(NotImplementedError):
        H.select_method("cutout", True)


def test_recipes_never_take_a_baseline():
    for m in ("mixup(same)", "mixup(mix)", "magnitudewarp", "timewarp", "timemask",
              "respiratoryscale", "(saloptenv)mixup(same)"):
        assert H.plain_recipe(m, False) is None
        assert H.salopt_recipe(m) is None


def test_parsers():
    assert H.parse_warp("magnitudewarp", "magnitudewarp") == (0.2, 4)
    assert H.parse_warp("timewarp", "timewarp") == (0.05, 2)
    assert H.parse_warp("timewarp(0.1,5)+0.5", "timewarp") == (0.1, 5)
    assert H.parse_warp("magnitudewarp(0.3,1)", "magnitudewarp") == (0.3, 1)
    assert H.parse_timemask("timemask") == 0.2
    assert H.parse_timemask("timemask(0.1)+0.5") == 0.1
    assert H.parse_timemask("timemask(1.5)") == 1 and H.parse_timemask("timemask(-2)") == 0
    assert H.parse_respscale("respiratoryscale") == (12 / 60, 20 / 60)
    assert H.parse_respscale("respiratoryscale(8.5,30)+0.2") == (8.5 / 60, 30 / 60)
    with pytest.raises(ValueError):                # max goes through int(), as in the reference
        H.parse_respscale("respiratoryscale(12,20.5)")
    # the knot count / max rate is read behind the string's FIRST comma
    assert H.parse_warp("(a,7)timewarp(0.1,5)", "timewarp") == (0.1, 7)
    assert H.parse_respscale("(x,40)respiratoryscale(12,20)") == (12 / 60, 40 / 60)


def test_respiratoryscale_with_a_float_maximum_raises_from_make_plan():
    fr = np.array([[0, 10, 20, 30, 40]] * 2)
    with pytest.raises(ValueError):
        H.make_plan("respiratoryscale(12,20.5)", np.zeros(2, int), fr, ["a", "b"], 3, 2, 1,
                    sample_rate=1000, sig_len=64)


def test_rejected_step_draws_nothing():
    fr = np.array([[0, 10, 20, 30, 40]] * 2)
    step = next(s for s in range(100) if random.Random(s).uniform(0, 1) >= 0.5)
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    plan = H.make_plan("timewarp+0.5", lambda: 1 / 0, fr, ["a", "b"], step, 2, 1, sig_len=64)
    assert not plan.fired and np.array_equal(np.random.get_state()[1], before)


# ------------------------------------------------------------------ plans against the reference
def test_fixture_set():
    names = [str(load(f)["method"]) for f in BASE_FILES]
    for m in ("mixup(same)", "mixup(mix)", "magnitudewarp", "timewarp", "timemask", "respiratoryscale"):
        assert any(n.startswith(m) or m in n for n in names), m
    fired = [int(load(f)["fired"]) for f in BASE_FILES]
    assert 0 in fired and 1 in fired


@pytest.mark.parametrize("path", BASE_FILES, ids=os.path.basename)
def test_plan_matches_the_reference(path):
    g = load(path)
    method, step = str(g["method"]), int(g["step"])
    x = g["x"]
    B, C, T = x.shape
    set_np_state(g, "np_before")
    py = random.getstate()
    plan = H.make_plan(method, g["labels"], g["frames"], list(g["wav"]), step, B, C,
                       sample_rate=int(g["sample_rate"]), sig_len=T)
    assert random.getstate() == py
    assert_np_state(g)
    assert plan.fired == bool(g["fired"])
    if not plan.fired:
        return
    y = g["y"]
    if plan.kind == "mixup":
        assert np.array_equal(plan.mix, g["mix"]) and plan.lam64 == float(g["lam"])
        assert plan.mix_all == ("(mix)" in method)
        lam = np.float32(plan.lam32)
        ref = x * lam + x[plan.mix] * (np.float32(1) - lam)        # fp32, three roundings
        assert np.array_equal(ref, y)
    elif plan.kind in ("magnitudewarp", "timewarp"):
        assert np.array_equal(plan.knots.reshape(-1), g["knots"].reshape(-1))
    elif plan.kind == "timemask":
        ref = x.copy()
        for b, (s0, s1) in enumerate(plan.spans):
            ref[b, :, s0:s1] = 0
        assert np.array_equal(ref, y)
    elif plan.kind == "respiratoryscale":
        assert np.array_equal((x.astype(np.float64) * plan.scale_row).astype(np.float32), y)


# ------------------------------------------------------------------ numpy's interp, restated
def lib_interp(x, xp, fp):
    x, xp, fp = (np.ascontiguousarray(a, np.float64) for a in (x, xp, fp))
    out = np.empty_like(x)
    assert _lib.load().pcgmix_np_interp_f64(x.ctypes.data, x.size, xp.ctypes.data, fp.ctypes.data,
                                            xp.size, out.ctypes.data) == 0
    return out


def test_np_interp_fuzz():
    rng = np.random.default_rng(2024)
    for it in range(4000):
        n = int(rng.integers(1, 5)) if it % 5 == 0 else int(rng.integers(5, 80))
        kind = it % 6
        if kind == 0:
            xp = rng.normal(size=n)                                  # random order
        elif kind == 1:
            xp = np.sort(rng.normal(size=n))                         # increasing
        elif kind == 2:
            xp = np.round(rng.normal(size=n).cumsum() * 2) / 2       # plateaus (ties)
        elif kind == 3:
            xp = np.clip(rng.normal(size=n).cumsum(), -1, 1)         # clipped flat ends
        elif kind == 4:
            xp = np.sort(rng.normal(size=n))                         # mostly increasing ...
            if n > 2:
                i = int(rng.integers(1, n))
                xp[i] = xp[i - 1] - abs(rng.normal()) * 0.1          # ... with one decreasing step
        else:
            xp = np.repeat(rng.normal(size=(n + 2) // 3), 3)[:n]     # triples of equal xp
        fp = rng.normal(size=n)
        if it % 4 == 0:
            fp[rng.integers(0, n)] = rng.choice([np.inf, -np.inf])   # inf / nan slopes
        if it % 9 == 0 and n > 1:
            fp[1:] = fp[0]                                           # equal fp at ties
        nx = int(rng.integers(0, 120))
        x = rng.normal(size=nx) * 2.5                                # keys out of range too
        if nx and it % 3 == 0:
            x[: nx // 2] = xp[rng.integers(0, n, size=nx // 2)]      # keys ON knots
        if it % 2 == 0:
            x = np.sort(x)
        got, want = lib_interp(x, xp, fp), np.interp(x, xp, fp)
        assert np.array_equal(got, want, equal_nan=True), (it, n, kind)


def test_np_interp_integer_keys_like_time_warp():
    rng = np.random.default_rng(7)
    for it in range(300):
        T = int(rng.integers(2, 400))
        xp = np.clip(np.cumsum(rng.normal(1, 1.2, size=T)) - 3, 0, T - 1)
        fp = rng.normal(size=T).astype(np.float32).astype(np.float64)
        assert np.array_equal(lib_interp(np.arange(T, dtype=np.float64), xp, fp),
                              np.interp(np.arange(T), xp, fp))


# ------------------------------------------------------------------ one time-warped row
def spline_op(T, n):
    lib = _lib.load()
    op = np.empty(lib.pcgmix_spline_operator_size(n))
    assert lib.pcgmix_spline_operator_f64(T, n, op.ctypes.data) == 0
    return op


def host_row(op, knots, x):
    T = x.shape[0]
    y, xp = np.empty(T, np.float32), np.empty(T)
    knots = np.ascontiguousarray(knots, np.float64)
    x = np.ascontiguousarray(x, np.float32)
    assert _lib.load().pcgmix_time_warp_row_f64(op.ctypes.data, knots.ctypes.data, knots.size,
                                                x.ctypes.data, T, y.ctypes.data, xp.ctypes.data) == 0
    return y, xp


def scipy_row(knots, x):
    from scipy.interpolate import CubicSpline
    T = x.shape[0]
    ws = np.linspace(0, T - 1., num=knots.size)
    tw = CubicSpline(ws, ws * knots)(np.arange(T))
    xp = np.clip((T - 1) / tw[-1] * tw, 0, T - 1)
    return np.interp(np.arange(T), xp, x).astype(np.float32), xp


def check_warped(got, want, x_rows):
    """The time warp's tolerance: within 1 fp32 ulp everywhere except where the output cancels
    (|y| far below the row's scale) — there the difference is the fp64 xp difference (the
    operator's spline vs scipy's banded solve, ~1e-12) times the local slope, and the absolute
    error stays at that level.  Such elements must stay below 0.1 %."""
    d = ulp_diff(got, want)
    scale = np.abs(x_rows).max(axis=-1, keepdims=True)
    out = d > 1
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err[out] <= 1e-9 * np.broadcast_to(scale, got.shape)[out]).all()
    assert out.sum() <= max(2, 0.001 * got.size)
    return int(out.sum())


@pytest.mark.parametrize("T, n, sigma", [(640, 6, 0.2), (641, 3, 0.2), (2500, 6, 0.05),
                                         (5000, 6, 0.05), (7, 2, 0.3), (2, 4, 0.2), (333, 8, 0.3)])
def test_time_warp_row_against_scipy(T, n, sigma):
    rng = np.random.default_rng(T * 100 + n)
    op = spline_op(T, n)
    rows, got, want, nonmono = [], [], [], 0
    for _ in range(30):
        x = rng.normal(size=T).astype(np.float32)
        kn = rng.normal(1.0, sigma, size=n)
        y, xp = host_row(op, kn, x)
        yr, xr = scipy_row(kn, x)
        assert np.abs(xp - xr).max() <= 1e-9 * T
        nonmono += bool((np.diff(xr) < 0).any())
        rows.append(x), got.append(y), want.append(yr)
    check_warped(np.stack(got), np.stack(want), np.stack(rows))
    if sigma >= 0.2 and n >= 6:
        assert nonmono > 0          # the sequential walk is exercised


@pytest.mark.parametrize("path", [f for f in BASE_FILES if "timewarp" in str(load(f)["method"])],
                         ids=os.path.basename)
def test_time_warp_rows_against_the_reference(path):
    g = load(path)
    if not int(g["fired"]):
        return
    x, y = g["x"], g["y"]
    B, C, T = x.shape
    n = g["knots"].shape[1]
    op = spline_op(T, n)
    got = np.stack([np.stack([host_row(op, g["knots"][b, :, c], x[b, c])[0] for c in range(C)])
                    for b in range(B)])
    check_warped(got, y, x)


def test_time_warp_fixtures_cover_non_monotone_and_flat_rows():
    from scipy.interpolate import CubicSpline
    nonmono = flat = 0
    for f in BASE_FILES:
        g = load(f)
        if "timewarp" not in str(g["method"]) or not int(g["fired"]):
            continue
        B, C, T = g["x"].shape
        n = g["knots"].shape[1]
        ws = np.linspace(0, T - 1., num=n)
        for b in range(B):
            for c in range(C):
                tw = CubicSpline(ws, ws * g["knots"][b, :, c])(np.arange(T))
                xp = np.clip((T - 1) / tw[-1] * tw, 0, T - 1)
                nonmono += bool((np.diff(xp) < 0).any())
                flat += bool((np.diff(xp) == 0).any())
    assert nonmono >= 3 and flat >= 3, (nonmono, flat)
