"""Plain numpy restatements of the comparison-baseline entry points (csrc/pcgmix_baselines.hip:
pcgmix_blend_rows_f32, pcgmix_warp_rows_f32, pcgmix_scale_rows_f32, pcgmix_zero_spans_f32,
pcgmix_zero_rects_f32, pcgmix_time_warp_f32), the data the edge suite feeds them and the shapes it
runs.  Written from what include/pcgmix_hip.h promises, not from the kernels' loops.  Batches are
(B, C, T) or (B, C, F, W) float32; knots are (B, n_knots, C) float64 as numpy draws them.

The rules
  blend          y[b] = x[b]*lam + x[mix[b]]*(1-lam), float32 multiply, multiply, add, (1-lam) formed in
                 float32: three roundings (tests/test_baselines_cpu.py::test_plan_matches_the_reference).
  scale          y = float32(float64(x) * s[t]): one float64 product, one rounding to float32.
  zero_spans     x[b, :, s0:s1] = 0 after clipping the span to [0, T].
  zero_rects     x[b, :, f0:f1, t0:t1] = 0 after clipping the rectangle to the plane.
  warp_rows      op = pcgmix_spline_operator_f64(T, n): break points op[:n], then the linear map knots ->
                 coefficients.  coef[p][j] = sum_i op[n + (p*4 + j)*n + i] * knots[i], accumulated over the
                 knots in index order from 0.0; the piece of t is the number of INTERIOR breaks <= t;
                 S(t) = c3 + c2 s, + c1 s^2, + c0 s^3 with s = t - brk[piece] and a running power; all of it
                 float64 and unfused.  y = float32(float64(x) * S(t)).
  time_warp_row  xp from the host twin pcgmix_time_warp_row_f64 (its xp_out), then numpy's own interp:
                 y = float32(np.interp(arange(T), xp, float64(x))).
  search_walk    numpy's binary_search_with_guess walked over the keys 0..T-1, the previous result as
                 the guess: what the time warp keeps per sample when xp decreases somewhere
                 (tests/test_baselines_ref_cpu.py ties it to pcgmix_np_interp_f64 and to np.interp).
"""
import numpy as np

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

F32, F64 = np.float32, np.float64

# ---- the kernels' constants (tests/test_baselines_ref_cpu.py reads them back from the source) -------
THREADS = 256             # kThreadsB
UNROLL = 4                # kUnrollB
EPB = THREADS * 4 * UNROLL    # kEpbB = 4096: elements of a row (blend: of a plane) per streaming block
ZERO_CHUNK = THREADS * 4      # kZeroChunk = 1024: rectangle elements per block
MAX_KNOTS = 64            # kMaxKnotsB
TW_LDS_MAX_T = 5120       # kTwLdsMaxT: the last time-warp row that lives in LDS

# ---- shapes ------------------------------------------------------------------------------------------
B = 3
CHANNELS = [1, 3]         # 3 shows the knot stride C and the row -> (b, c) split
STREAM_T = [              # (T, reason)
    (1, "one element: scalar path, one lane"),
    (3, "below one quad, scalar"),
    (4, "one quad, vector path"),
    (5, "one quad and one, scalar"),
    (8, "two quads"),
    (4092, "one quad short of a block"),
    (4096, "exactly one block (kEpbB)"),
    (4097, "blockIdx.y seam on the scalar path: one element in the second block"),
    (4099, "seam, scalar, three elements in the second block"),
    (4100, "seam on the vector path: one quad in the second block"),
    (8196, "two seams: two full blocks and one quad"),
]
KNOTS = [2, 3, 6, 64]     # the limits 2 and kMaxKnotsB, one interior break, the usual 6
ALIGN_T = [4096, 8196]    # T % 4 == 0: the vector path as allocated, the scalar one 4 bytes further on
BLEND_LAM = [0.0, 1.0, float(F32(0.2718))]

TW_T = [                  # (T, reason)
    (2, "the smallest row: numpy's search is its linear branch (len <= 4)"),
    (3, "len <= 4, odd"),
    (255, "one lane short of a block stride (kThreadsB)"),
    (256, "one block stride"),
    (257, "one sample in the second stride"),
    (5119, "one below the LDS threshold"),
    (5120, "kTwLdsMaxT: the last row in LDS (61440 B dynamic)"),
    (5121, "the first row in the caller's workspace"),
]
TW_KNOTS = [2, 6, 64]
TW_SIGMA = [0.05, 0.3]
TW_B, TW_C = 2, 3

SPAN_T = [600, 601]       # even and odd; long enough for spans that start at 255, 256, 257
PLANES = [(5, 7), (32, 32), (33, 41), (40, 130)]
# 2049 = 3 * 683 is no h * w inside any of these planes: the second seam of kZeroChunk is taken from
# both sides with 2048 = 16 * 128 (exactly two blocks) and 2050 = 25 * 82 (two elements in a third)
SEAM_AREAS = [0, 1, 1023, 1024, 1025, 2048, 2050]


def stream_shapes():
    """(B, C, T) of the streaming kernels."""
    return [(B, C, T) for T, _ in STREAM_T for C in CHANNELS]


def warp_shapes():
    """(B, C, T, n) of warp_rows: T >= 2."""
    return [(B, C, T, n) for T, _ in STREAM_T if T >= 2 for C in CHANNELS for n in KNOTS]


def integer_break_shapes():
    """The (B, 3, T, n) of warp_shapes whose interior breaks are integers, (T - 1) % (n - 1) == 0: a sample
    sits ON a break there, and the piece search's `<=` decides which cubic it takes."""
    return [s for s in warp_shapes() if s[1] == 3 and s[3] > 2 and (s[2] - 1) % (s[3] - 1) == 0]


def tw_cases():
    return [(T, n, s) for T, _ in TW_T for n in TW_KNOTS for s in TW_SIGMA]


# ---- the host side of the library ------------------------------------------------------------------------
def spline_op(T, n):
    lib = _lib.load()
    op = np.empty(lib.pcgmix_spline_operator_size(n))
    assert lib.pcgmix_spline_operator_f64(T, n, op.ctypes.data) == 0
    return op


def host_row(op, knots, x):
    """The host twin: (y float32, xp float64) of one row."""
    T = x.shape[0]
    y, xp = np.empty(T, F32), np.empty(T)
    knots = np.ascontiguousarray(knots, F64)
    x = np.ascontiguousarray(x, F32)
    assert _lib.load().pcgmix_time_warp_row_f64(op.ctypes.data, knots.ctypes.data, knots.size, x.ctypes.data, T,
                                                y.ctypes.data, xp.ctypes.data) == 0
    return y, xp


def lib_interp(x, xp, fp):
    x, xp, fp = (np.ascontiguousarray(a, F64) for a in (x, xp, fp))
    out = np.empty_like(x)
    assert _lib.load().pcgmix_np_interp_f64(x.ctypes.data, x.size, xp.ctypes.data, fp.ctypes.data, xp.size,
                                            out.ctypes.data) == 0
    return out


# ---- the rules -------------------------------------------------------------------------------------------
def blend(x, mix, lam):
    x = np.asarray(x, F32)
    lam = F32(lam)
    with np.errstate(all="ignore"):
        return x * lam + x[np.asarray(mix)] * (F32(1) - lam)


def scale(x, s):
    """x (..., T) float32, s (T) float64."""
    with np.errstate(all="ignore"):
        return (np.asarray(x, F32).astype(F64) * np.asarray(s, F64)).astype(F32)


def zero_spans(x, spans):
    """x (B, C, T), spans (B, 2)."""
    y = np.array(x, copy=True)
    T = y.shape[-1]
    for b, (s0, s1) in enumerate(np.asarray(spans).tolist()):
        s0, s1 = min(max(s0, 0), T), min(max(s1, 0), T)
        if s1 > s0:
            y[b, :, s0:s1] = 0
    return y


def clip_rect(r, F, W):
    f0, f1, t0, t1 = (int(v) for v in r)
    return min(max(f0, 0), F), min(max(f1, 0), F), min(max(t0, 0), W), min(max(t1, 0), W)


def rect_area(r, F, W):
    f0, f1, t0, t1 = clip_rect(r, F, W)
    return max(f1 - f0, 0) * max(t1 - t0, 0)


def zero_rects(x, rect):
    """x (B, C, F, W), rect (B, 4) = [f0, f1, t0, t1)."""
    y = np.array(x, copy=True)
    F, W = y.shape[-2:]
    for b, r in enumerate(np.asarray(rect)):
        f0, f1, t0, t1 = clip_rect(r, F, W)
        if f1 > f0 and t1 > t0:
            y[b, :, f0:f1, t0:t1] = 0
    return y


def spline_rows(op, n, v, T):
    """v (rows, n) float64 knot values -> S (rows, T): the spline of the header at t = 0..T-1."""
    brk = op[:n]
    M = op[n:].reshape((n - 1) * 4, n)
    coef = np.zeros((v.shape[0], (n - 1) * 4))
    for i in range(n):                                 # in index order from 0.0, one product and one sum each
        coef = coef + M[:, i] * v[:, i:i + 1]
    coef = coef.reshape(-1, n - 1, 4)
    t = np.arange(T, dtype=F64)
    p = np.searchsorted(brk[1:n - 1], t, side="right")  # the number of interior breaks <= t
    c = coef[:, p, :]                                  # (rows, T, 4)
    s = t - brk[p]
    r = c[..., 3] + c[..., 2] * s
    z = s * s
    r = r + c[..., 1] * z
    z = z * s
    return r + c[..., 0] * z


def warp_rows(x, knots, op=None):
    """x (B, C, T) float32, knots (B, n, C) float64."""
    Bn, C, T = x.shape
    n = knots.shape[1]
    op = spline_op(T, n) if op is None else op
    v = np.transpose(np.asarray(knots, F64), (0, 2, 1)).reshape(Bn * C, n)
    S = spline_rows(op, n, v, T).reshape(Bn, C, T)
    with np.errstate(all="ignore"):
        return (np.asarray(x, F32).astype(F64) * S).astype(F32)


def time_warp_row(op, knots, x):
    """(y, xp, y of the host twin): numpy's interp on the twin's xp."""
    y_twin, xp = host_row(op, knots, x)
    T = x.shape[0]
    with np.errstate(all="ignore"):
        y = np.interp(np.arange(T), xp, np.asarray(x, F32).astype(F64)).astype(F32)
    return y, xp, y_twin


def _bsearch_guess(key, arr, n, guess):
    """numpy/_core/src/multiarray/compiled_base.c: binary_search_with_guess."""
    imin, imax = 0, n
    if key > arr[n - 1]:
        return n
    if key < arr[0]:
        return -1
    if n <= 4:
        i = 1
        while i < n and key >= arr[i]:
            i += 1
        return i - 1
    guess = max(1, min(guess, n - 3))
    if key < arr[guess]:
        if key < arr[guess - 1]:
            imax = guess - 1
            if guess > 8 and key >= arr[guess - 8]:
                imin = guess - 8
        else:
            return guess - 1
    else:
        if key < arr[guess + 1]:
            return guess
        if key < arr[guess + 2]:
            return guess + 1
        imin = guess + 2
        if guess < n - 8 - 1 and key < arr[guess + 8]:
            imax = guess + 8
    while imin < imax:
        imid = imin + ((imax - imin) >> 1)
        if key >= arr[imid]:
            imin = imid + 1
        else:
            imax = imid
    return imin - 1


def search_walk(xp):
    """j[t] of numpy's interp for the keys t = 0..T-1 in order (int32, -1 and T included)."""
    arr = np.asarray(xp, F64).tolist()
    n, j, out = len(arr), 0, []
    for t in range(n):
        j = _bsearch_guess(float(t), arr, n, j)
        out.append(j)
    return np.array(out, np.int32)


def pick(j, xp, fp):
    """What numpy's interp stores for the search results j at the keys 0..T-1 (finite fp)."""
    xp, fp = np.asarray(xp, F64), np.asarray(fp, F64)
    n = xp.size
    key = np.arange(n, dtype=F64)
    j = np.asarray(j, np.int64)
    jc = np.clip(j, 0, n - 2) if n > 1 else np.zeros_like(j)
    with np.errstate(all="ignore"):
        slope = (fp[jc + 1] - fp[jc]) / (xp[jc + 1] - xp[jc])
        r = slope * (key - xp[jc]) + fp[jc]
    r = np.where(xp[np.clip(j, 0, n - 1)] == key, fp[np.clip(j, 0, n - 1)], r)
    r = np.where(j >= n - 1, fp[n - 1], r)
    return np.where(j < 0, fp[0], r)


# ---- data ----------------------------------------------------------------------------------------------
SUB_MIN = float(np.frombuffer(np.int32(1).tobytes(), F32)[0])          # the smallest float32 subnormal
SUB_BIG = float(np.frombuffer(np.int32(0x007FFFFF).tobytes(), F32)[0])  # the largest
F32_MAX = float(np.finfo(F32).max)
SPECIALS = [0.0, -0.0, SUB_MIN, -SUB_BIG, F32_MAX, -F32_MAX, np.inf, np.nan, SUB_BIG, -SUB_MIN]


def _rng(kind, shape):
    return np.random.RandomState((sum((i + 3) * 7919 ** i * int(v) for i, v in enumerate(shape)) + 101 * len(kind)) % 2 ** 31)


def planted_positions(T):
    """Where the k-th special of row r goes: (r + offsets[k]) % T.  The offsets cover the row's ends and
    both sides of every block seam the row has."""
    cand = [0, T - 1] + ([EPB - 1, EPB, EPB - 4, EPB + 1] if T > EPB else [])
    cand += [T // 2, T // 3, 1, 2, T // 5, T // 7, 3, T - 2] + list(range(4, 4 + len(SPECIALS)))
    off = []
    for o in cand:                                     # distinct modulo T, in this order
        if o % T not in off:
            off.append(o % T)
    return (off * len(SPECIALS))[:len(SPECIALS)]       # rows shorter than the list: the later specials win


def samples(shape, kind="x"):
    """Gaussian float32 (B, C, T) with +-0.0, float32 subnormals, +-the largest finite value, +inf and NaN
    planted at fixed positions of every row (rows shorter than the list keep the last ones planted)."""
    Bn, C, T = shape
    rs = _rng(kind, shape)
    x = rs.standard_normal(shape).astype(F32)
    off = planted_positions(T)
    for r in range(Bn * C):
        for k, v in enumerate(SPECIALS):
            x[r // C, r % C, (r + off[k]) % T] = v
    return x


def knots_for(Bn, n, C, sigma=0.2, kind="knots"):
    return _rng(kind, (Bn, n, C, int(sigma * 1000))).normal(1.0, sigma, size=(Bn, n, C))


def zero_knots(knots):
    """Knots that are exactly 0.0 at every interior break of channel 0 and at the first one of channel 1.
    Both cubics that meet at a break agree there only to float64 rounding, which float32(x * S) hides — except
    where the knot is 0: the piece that STARTS at the break gives S = c3 = +0.0 exactly (y = +-0.0), the piece
    that ends there a value around 1e-17 (y = x * 1e-17)."""
    k = np.array(knots, copy=True)
    k[:, 1:-1, 0] = 0.0
    k[:, 1, 1] = 0.0
    return k


def scale_row(T):
    """A sinusoid as respiratoryscale draws it, with an exact +0.0, a -0.0 and a negative factor planted."""
    s = 1.0 + 0.3 * np.sin(2 * np.pi * 0.25 * np.arange(T) / 1000.0 + 0.7)
    for i, v in ((0, 0.0), (T // 2, -0.0), (T - 1, -1.5)):
        s[i] = v
    return s


def mixes(Bn):
    """A permutation without fixed points, the identity, all zeros."""
    return [("perm", np.roll(np.arange(Bn), 1).astype(np.int32)), ("identity", np.arange(Bn, dtype=np.int32)),
            ("zeros", np.zeros(Bn, np.int32))]


def span_list(T):
    """(s0, s1, reason), one per sample of a batch."""
    return [
        (5, 5, "empty: s1 == s0"),
        (9, 3, "empty: s1 < s0"),
        (0, T, "the whole row"),
        (T // 2, T // 2 + 1, "one element"),
        (-4, 3, "s0 < 0"),
        (-9, -2, "wholly below the row"),
        (T - 3, T + 6, "s1 > T"),
        (T + 5, T + 9, "s0 a little above T"),
        (-7, T + 7, "both ends outside"),
        (255, 300, "starts at 255"),
        (256, 256 + THREADS, "starts at 256, one stride long"),
        (257, 257 + THREADS + 1, "starts at 257, one stride and one"),
        (1, THREADS, "255 long"),
        (T - 1, T, "the last element"),
        (0, 1, "the first element"),
    ]


def rect_batches(F, W):
    """[(rect (3, 4) int32, reason)]: per batch one rectangle whose CLIPPED area is a seam value of
    SEAM_AREAS (those that fit the plane) or F * W, next to an empty one and a small one that sticks out;
    the three change places from batch to batch, so the sample an area sits on differs."""
    def with_area(a):
        if a == 0:
            return (2, 2, 1, 5)
        for h in range(1, F + 1):
            if a % h == 0 and a // h <= W:
                w = a // h
                f0, t0 = F - h, W - w                  # flush with the far corner ...
                return (f0, f0 + h + 3, t0, t0 + w + 5)  # ... and sticking out of it
        return None

    empties = [(3, 1, 0, W), (0, F, 4, 4), (F + 2, F + 5, 0, W), (0, F, W + 1, W + 9), (-5, 0, 0, W), (1, 3, -8, -1)]
    smalls = [(-3, 1, -2, 1), (F - 1, F + 4, -6, 1), (-1, 1, W - 1, W + 2), (F - 1, F + 1, W - 1, W + 1)]  # clipped area 1
    out = []
    for k, a in enumerate(SEAM_AREAS + [F * W]):
        r = with_area(a) if a != F * W else (-2, F + 2, -3, W + 3)
        if r is None:
            continue
        trio = [r, empties[k % len(empties)], smalls[k % len(smalls)] if a > 1 else empties[(k + 1) % len(empties)]]
        trio = trio[k % 3:] + trio[:k % 3]
        out.append((np.array(trio, np.int32), f"area {a}"))
    return out


def tw_case(T, n, sigma):
    """x (2, 3, T) Gaussian float32 and knots (2, n, 3) ~ N(1, sigma), seeded by the case."""
    rs = _rng("tw", (T, n, int(sigma * 1000)))
    x = rs.standard_normal((TW_B, TW_C, T)).astype(F32)
    kn = rs.normal(1.0, sigma, size=(TW_B, n, TW_C))
    return x, kn


def tw_rows(T, n, sigma):
    """[(b, c, x row, knots of the row)] of tw_case."""
    x, kn = tw_case(T, n, sigma)
    return [(b, c, x[b, c], np.ascontiguousarray(kn[b, :, c])) for b in range(TW_B) for c in range(TW_C)]


def same_bits(got, want):
    """Indices where two float32 arrays differ: by bit pattern (so -0.0 != +0.0), any NaN equal to any NaN."""
    got, want = np.ascontiguousarray(got, F32).reshape(-1), np.ascontiguousarray(want, F32).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.flatnonzero((gn != wn) | (~gn & ~wn & (got.view(np.int32) != want.view(np.int32))))
