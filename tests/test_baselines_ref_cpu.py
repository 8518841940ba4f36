"""tests/baselines_ref.py against the project's oracle: warp_rows against oracle.pcgmix_oracle.magnitude_warp
(scipy's CubicSpline) on the same numpy stream, time_warp_row against the host twin and scipy, the walk of
numpy's search against pcgmix_np_interp_f64 and np.interp, which search paths and flat ends the time-warp
cases reach, and what the shape lists cover in terms of the constants of csrc/pcgmix_baselines.hip.
No GPU."""
import os
import re

import numpy as np
import pytest

import baselines_ref as R
from test_baselines_cpu import check_warped, scipy_row, ulp_diff

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(os.path.dirname(HERE), "pcgmix-a-data-augmentation-method-for-heart-sound-classification-extended_amd",
                      "csrc", "pcgmix_baselines.hip")


# ---- warp_rows against the oracle ------------------------------------------------------------------------
def oracle_warp(x, n, sigma, seed):
    """(oracle's y, the knots it drew): x (B, C, T)."""
    from oracle import pcgmix_oracle as O
    np.random.seed(seed)
    with np.errstate(all="ignore"):                    # planted non-finite samples
        y, knots = O.magnitude_warp(np.ascontiguousarray(np.transpose(x, (0, 2, 1))), sigma, n - 2, return_knots=True)
    return np.ascontiguousarray(np.transpose(y, (0, 2, 1))), knots


@pytest.mark.parametrize("n", R.KNOTS)
@pytest.mark.parametrize("T", [T for T, _ in R.STREAM_T if T >= 2])
def test_warp_rows_is_the_oracles_magnitude_warp(T, n):
    """C = 3, sigma 0.2, the knots the oracle draws from numpy's stream: at most 1 ulp apart, fewer than
    1e-3 of the elements differing (the project's bound for this pair; scipy solves a banded system where
    the operator is one constant linear map).  Seen: 0 differing elements at every one of the combinations."""
    x = R._rng("oracle", (R.B, 3, T)).standard_normal((R.B, 3, T)).astype(np.float32)
    want, knots = oracle_warp(x, n, 0.2, 1000 * n + T)
    got = R.warp_rows(x, knots)
    d = ulp_diff(got, want)
    print(f"T = {T}, n = {n}: {int((d > 0).sum())} of {d.size} differ, max {int(d.max())} ulp")
    assert d.max() <= 1 and (d > 0).mean() < 1e-3


@pytest.mark.parametrize("shape", R.integer_break_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_zero_knot_on_an_integer_break_is_an_exact_zero(shape):
    """zero_knots: at a sample ON a break whose knot is 0.0 the spline is +0.0 exactly, as scipy's is (a piece
    search with `<` for `<=` would give the previous cubic's ~1e-17 instead), so y there is x * 0."""
    from scipy.interpolate import CubicSpline
    Bn, C, T, n = shape
    knots = R.zero_knots(R.knots_for(Bn, n, C))
    op = R.spline_op(T, n)
    S = R.spline_rows(op, n, np.transpose(knots, (0, 2, 1)).reshape(Bn * C, n), T).reshape(Bn, C, T)
    step = (T - 1) // (n - 1)
    at = np.arange(1, n - 1) * step
    assert np.array_equal(op[:n][1:-1], at)
    assert not S[:, 0, at].any() and not np.signbit(S[:, 0, at]).any() and not S[:, 1, at[0]].any() and S[:, 2, at].all()
    brk = np.linspace(0, T - 1.0, num=n)
    assert not CubicSpline(brk, knots[0, :, 0])(at).any()
    x = R.samples((Bn, C, T))
    y = R.warp_rows(x, knots, op)
    fin = np.isfinite(x[:, 0, at])
    assert not y[:, 0, at][fin].any() and np.array_equal(np.signbit(y[:, 0, at][fin]), np.signbit(x[:, 0, at][fin]))


# ---- time_warp_row against the twin and scipy ------------------------------------------------------------------
@pytest.mark.parametrize("T, n, sigma", R.tw_cases())
def test_time_warp_row_is_the_twin_and_scipy(T, n, sigma):
    """numpy's interp on the twin's xp gives the twin's y bit for bit on the six rows of every case, and
    passes check_warped against scipy_row.  Seen: at most 1 excused element per case."""
    op = R.spline_op(T, n)
    rows, got, want = [], [], []
    for b, c, x, kn in R.tw_rows(T, n, sigma):
        y, xp, y_twin = R.time_warp_row(op, kn, x)
        assert np.array_equal(y.view(np.int32), y_twin.view(np.int32)), (b, c)
        ys, xs = scipy_row(kn, x)
        assert np.abs(xp - xs).max() <= 1e-9 * T
        rows.append(x), got.append(y), want.append(ys)
    excused = check_warped(np.stack(got), np.stack(want), np.stack(rows))
    print(f"T = {T}, n = {n}, sigma = {sigma}: {excused} of {6 * T} excused")


def _paths():
    """{(T, n, sigma): (non-monotone rows, rows with a flat step)} over the time-warp cases."""
    out = {}
    for T, n, sigma in R.tw_cases():
        op = R.spline_op(T, n)
        xps = [R.host_row(op, kn, x)[1] for _, _, x, kn in R.tw_rows(T, n, sigma)]
        out[T, n, sigma] = (sum(bool((np.diff(xp) < 0).any()) for xp in xps),
                            sum(bool((np.diff(xp) == 0).any()) for xp in xps))
    return out


def test_cases_cover_both_search_paths_and_the_flat_ends():
    """Rows whose xp decreases somewhere take numpy's walk on one lane, the others the block-parallel search:
    the cases hold both kinds at n = 6 with sigma 0.3 and at n = 64, on both sides of the LDS threshold, and
    only monotone rows at n = 2 (two knots give a straight line).  Flat steps (xp clipped at 0 or T - 1)
    occur as well."""
    P = _paths()
    for key, v in sorted(P.items()):
        print(key, "non-monotone rows %d, rows with a flat step %d of 6" % v)
    big = [T for T, _ in R.TW_T if T >= 255]
    for T in big:
        assert P[T, 6, 0.3][0] > 0, T
        assert P[T, 64, 0.3][0] > 0 and P[T, 64, 0.05][0] > 0, T
        # both kinds in one launch somewhere at this T
        assert any(0 < P[T, n, s][0] < 6 for n in R.TW_KNOTS for s in R.TW_SIGMA), T
        assert any(P[T, n, s][0] == 0 for n in R.TW_KNOTS for s in R.TW_SIGMA), T
        assert sum(P[T, n, s][1] for n in R.TW_KNOTS for s in R.TW_SIGMA) > 0, T
    assert all(P[T, 2, s][0] == 0 for T, _ in R.TW_T for s in R.TW_SIGMA)
    assert sum(v[1] for v in P.values()) > 0


@pytest.mark.parametrize("T, n, sigma", [(257, 6, 0.3), (257, 64, 0.3), (5121, 6, 0.3), (5121, 64, 0.05), (3, 6, 0.3)])
def test_search_walk_is_numpys(T, n, sigma):
    """The walk's results, put through numpy's interpolation rule, are pcgmix_np_interp_f64's output and
    np.interp's bit for bit, on monotone and non-monotone rows; on a row that never decreases they are the
    count of xp <= t, less one."""
    op = R.spline_op(T, n)
    keys = np.arange(T, dtype=np.float64)
    nonmono = 0
    for _, _, x, kn in R.tw_rows(T, n, sigma):
        xp = R.host_row(op, kn, x)[1]
        fp = x.astype(np.float64)
        j = R.search_walk(xp)
        got = R.pick(j, xp, fp)
        assert np.array_equal(got, R.lib_interp(keys, xp, fp)) and np.array_equal(got, np.interp(keys, xp, fp))
        if (np.diff(xp) < 0).any():
            nonmono += 1
        else:
            last_le = np.searchsorted(xp, keys, side="right") - 1
            assert np.array_equal(R.pick(last_le, xp, fp), got)
    assert nonmono > 0 or T == 3


# ---- the other rules ----------------------------------------------------------------------------------------
def test_planted_samples_hold_every_special():
    for shape in R.stream_shapes():
        x = R.samples(shape)
        T = shape[2]
        assert x.dtype == np.float32 and x.shape == shape
        if T >= 64:
            for row in x.reshape(-1, T):
                bits = row.view(np.int32)
                assert np.isnan(row).sum() == 1 and np.isposinf(row).sum() == 1
                assert (bits == 0).sum() >= 1 and (bits == np.int32(-2 ** 31)).sum() >= 1
                sub = (np.abs(row) > 0) & (np.abs(row) < np.finfo(np.float32).tiny)
                assert sub.sum() == 4 and (np.abs(row) == R.F32_MAX).sum() == 2
        if T > R.EPB:                                   # both sides of the first block seam
            pos = {(r + o) % T for r in range(shape[0] * shape[1]) for o in R.planted_positions(T)}
            assert {R.EPB - 1, R.EPB} <= pos


def test_blend_scale_and_zero_rules():
    x = R.samples((3, 2, 64))
    mix = np.array([2, 0, 1])
    y = R.blend(x, mix, 0.25)
    assert y.dtype == np.float32
    fin = np.isfinite(x) & np.isfinite(x[mix]) & (np.abs(x) < 1e30) & (np.abs(x[mix]) < 1e30)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)    # noqa: E731
    # three roundings, restated in float64 (products of float32 values are exact there, and a float64 sum
    # of two float32 values rounds to float32 as their float32 sum does: 53 >= 2 * 24 + 2)
    want = r32(x.astype(np.float64) * 0.25) + r32(x[mix].astype(np.float64) * 0.75)
    assert np.array_equal(y[fin], want.astype(np.float32)[fin])
    assert (y[fin] != (x.astype(np.float64) * 0.25 + x[mix].astype(np.float64) * 0.75).astype(np.float32)[fin]).any()
    assert np.array_equal(R.blend(x, [0, 1, 2], 1.0)[np.isfinite(x)], x[np.isfinite(x)])
    s = R.scale_row(64)
    y = R.scale(x, s)
    assert y.dtype == np.float32 and np.signbit(y[0, 0, 32]) != np.signbit(x[0, 0, 32])       # s = -0.0 there
    z = R.zero_spans(np.ones((2, 2, 10), np.float32), [(-3, 2), (8, 15)])
    assert z[0].sum() == 16 and z[1].sum() == 16 and not z[0, :, :2].any() and not z[1, :, 8:].any()
    z = R.zero_rects(np.ones((1, 2, 4, 5), np.float32), [(-1, 2, 3, 9)])
    assert z.sum() == 2 * (20 - 4) and not z[0, :, :2, 3:].any()


# ---- the shape lists ------------------------------------------------------------------------------------------
def _constant(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def test_shapes_cover_the_block_edges():
    """What the lists cover, in terms of the constants read from csrc/pcgmix_baselines.hip: a retune of any
    of them fails here instead of silently moving the seams away from the lists."""
    text = open(SOURCE).read()
    assert _constant(text, r"constexpr int kThreadsB = (\d+);") == R.THREADS
    assert _constant(text, r"constexpr int kUnrollB = (\d+);") == R.UNROLL
    assert re.search(r"constexpr int kEpbB = kThreadsB \* 4 \* kUnrollB;", text) and R.EPB == 4096
    assert re.search(r"constexpr int kZeroChunk = kThreadsB \* 4;", text) and R.ZERO_CHUNK == 1024
    assert _constant(text, r"constexpr int kMaxKnotsB = (\d+);") == R.MAX_KNOTS
    assert _constant(text, r"constexpr int kTwLdsMaxT = (\d+);") == R.TW_LDS_MAX_T
    assert re.search(r"T \* \(long long\)\(sizeof\(double\) \+ sizeof\(int\)\)", text)
    Ts = [T for T, _ in R.STREAM_T]
    assert len(set(Ts)) == len(Ts) and all(why for _, why in R.STREAM_T + R.TW_T)
    # the streaming blocks: a row (C = 1: also a plane) on both sides of one block and of two, by one quad
    # (vector path) and by one and three elements (scalar path)
    E = R.EPB
    assert {E - 4, E, E + 1, E + 3, E + 4, 2 * E + 4} <= set(Ts)
    assert {1, 3, 4, 5, 8} <= set(Ts)                   # below, at and above one quad
    assert any(T % 4 == 0 for T in Ts) and any(T % 4 for T in Ts)
    # the blend runs over the plane C * T: planes on both sides of a seam that the rows are not
    planes = {C * T for C in R.CHANNELS for T in Ts}
    assert any(p % 4 == 0 and p % E == 4 for p in planes) and any(p % 4 and p > E for p in planes)
    assert any(p > 2 * E and (p - 1) // E >= 2 for p in planes)
    assert max(R.B * C * T for C in R.CHANNELS for T in Ts) == 3 * 3 * 8196
    assert all(T % 4 == 0 and T in Ts for T in R.ALIGN_T) and any(T > E for T in R.ALIGN_T) and E in R.ALIGN_T
    assert {2, R.MAX_KNOTS} <= set(R.KNOTS) and {2, R.MAX_KNOTS} <= set(R.TW_KNOTS)
    assert 1 in R.CHANNELS and any(C > 1 for C in R.CHANNELS)
    # integer interior breaks occur (the piece search's >= decides there): (T - 1) / (n - 1) an integer
    assert any((T - 1) % (n - 1) == 0 and n > 2 for T in Ts if T > 8 for n in R.KNOTS)
    ib = R.integer_break_shapes()
    assert {n for *_, n in ib} == {3, 6, R.MAX_KNOTS} and any(T > E for _, _, T, _ in ib)
    # the time warp: the smallest row, numpy's linear branch (len <= 4), the block stride, the LDS threshold
    tw = [T for T, _ in R.TW_T]
    L, S = R.TW_LDS_MAX_T, R.THREADS
    assert {2, 3, S - 1, S, S + 1, L - 1, L, L + 1} == set(tw)
    assert L * 12 + ((R.MAX_KNOTS - 1) * 4 + 2 * R.MAX_KNOTS) * 8 <= 64 * 1024    # dynamic + static LDS (coef, brk, yv) of the last LDS row
    # spans: starts and lengths around the block stride, both parities of T
    assert {T % 2 for T in R.SPAN_T} == {0, 1}
    for T in R.SPAN_T:
        sp = R.span_list(T)
        assert {S - 1, S, S + 1} <= {s0 for s0, _, _ in sp} and {S - 1, S, S + 1} <= {s1 - s0 for s0, s1, _ in sp}
        assert any(s1 <= s0 for s0, s1, _ in sp) and (0, T) in [(a, b) for a, b, _ in sp]
        assert any(s0 < 0 for s0, _, _ in sp) and any(s1 > T for _, s1, _ in sp)
        assert any(T < s0 <= T + 16 for s0, _, _ in sp) and any(s1 - s0 == 1 for s0, s1, _ in sp)
        assert max(abs(v) for s0, s1, _ in sp for v in (s0, s1)) < 1 << 16     # nothing near the int32 limits
    # rectangles: clipped areas on both sides of one and two blocks of kZeroChunk
    Z = R.ZERO_CHUNK
    assert {0, 1, Z - 1, Z, Z + 1, 2 * Z, 2 * Z + 2} == set(R.SEAM_AREAS)
    seen = set()
    for F, W in R.PLANES:
        batches = R.rect_batches(F, W)
        areas = [[R.rect_area(r, F, W) for r in rect] for rect, _ in batches]
        seen |= {max(a) for a in areas}
        assert F * W in {max(a) for a in areas} and {0, 1} <= {max(a) for a in areas}
        rects = np.concatenate([rect for rect, _ in batches])
        assert (rects[:, 0] < 0).any() and (rects[:, 1] > F).any() and (rects[:, 2] < 0).any() and (rects[:, 3] > W).any()
        assert (rects[:, 1] <= rects[:, 0]).any() and (rects[:, 3] <= rects[:, 2]).any()
        assert all(len({tuple(r) for r in rect}) == 3 for rect, _ in batches)         # they differ per sample
        assert len({int(np.argmax(a)) for a in areas if max(a) > 1}) > 1 or len(areas) <= 3
    assert set(R.SEAM_AREAS) <= seen
    assert any((w := R.clip_rect(r, F, W))[3] - w[2] < W and R.rect_area(r, F, W) > Z
               for F, W in R.PLANES for rect, _ in R.rect_batches(F, W) for r in rect)   # rows of a rectangle narrower than the plane
