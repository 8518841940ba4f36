"""Float64 restatement of the fused BatchNorm + ReLU + MaxPool entry points (csrc/pcgmix_bnrp.hip:
pcgmix_bnrp_fwd_f32, pcgmix_bnrp_bwd_f32, pcgmix_bnrp_eval_fwd_f32, pcgmix_bnrp_eval_bwd_f32), the
data the edge suite feeds them, and the shapes it runs.  Plain numpy, written from the rule and not
from the kernels' loops.  Arrays are NHWC: y (B, H, W, C), z / dz / skip (B, H/ph, W/pw, C).

The rule
  a        = scale * y + shift                     per channel
  z        = max over each ph x pw window of relu(a)  [+ skip]
  arg-max  = the FIRST maximum of relu(a) in (i, j) order; the gradient passes only where it is > 0
  training : scale = gamma * invstd, shift = beta - mean * scale, each product and the difference
             rounded to float32 (the kernels form them in float32 from the float32 mean and invstd);
             mean and invstd are the batch's (biased variance), rounded to float32 once;
             running_mean <- (1 - mom) * running_mean + mom * (mean + mean_shift);
             running_var  <- (1 - mom) * running_var  + mom * float32(unbiased variance);
             batches_tracked += 1
             dbeta = sum dy, dgamma = sum dy * xhat, dzero = +0, coef = float32(sum / n),
             dx = scale * (dy - c1 - xhat * c2) everywhere (dy = 0 off the arg-max and at positions
             no window covers, where this is scale * (-c1 - xhat * c2))
  eval     : invstd = float32(1 / sqrt(running_var + eps)), mean = running_mean - conv_bias;
             dx = scale * dz at the arg-max, +0.0 everywhere else.

Three kinds of data
  eval_int_case   small integers, power-of-two 1/sqrt(running_var), eps = 0: every product and sum
                  is exact in float32, so the kernels must give the float64 values BIT FOR BIT.
  train_int_case  y = m_c +- 2^k_c with as many plus as minus signs: mean, variance, 1/std and every
                  partial sum are exact (see its docstring for what is bit-exact and the one bound).
  margin_case     Gaussian data moved off every ReLU / arg-max decision that lies within 2e-3 of a
                  tie, so that no element is excused from the project's tolerances.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64

# ---- the kernels' constants (tests/test_bnrp_ref_cpu.py reads them back from the source) ---------
BN_THREADS = 256          # kBnThreads
BN_MAX_BLOCKS = 1024      # kBnMaxBlocks
BN_MAX_C = 1024           # kBnMaxC
FIN_CH = 16               # kFinCh
BLOCK_VECS = 8            # bn_blocks: vectors per thread a block is sized for
FIN_LANES = 16            # partial_sums: lanes per channel
FIN_UNROLL = 8            # partial_sums: loads in flight per lane

MARGIN = 2e-3             # twice the forward tolerance 1e-4 * |a| + 2e-5 at |a| = 10


ROUND = True              # False: nothing is rounded to float32 (the comparison with torch float64 autograd)


def f32(x):
    """Round to float32, return as float64."""
    x = np.asarray(x, F64)
    return x.astype(F32).astype(F64) if ROUND else x


# ---- shapes --------------------------------------------------------------------------------------
# (B, C, H, W, ph, pw, reason).  B * H * W is even everywhere (train_int_case needs it).
BNRP_EDGE = [
    (1, 2, 1, 8, 1, 2, "float2"),                 # C = 2: one float2 per row; n_rows = 4 < R = 256
    (2, 2, 1, 9, 1, 2, "float2-ragged"),          # W % pw != 0 with float2
    (3, 4, 1, 6, 1, 1, "Q1-nopool"),              # C = 4: finalize lanes c >= C, window (1,1)
    (1, 4, 1, 8, 1, 4, "generic-1x4"),
    (1, 12, 1, 170, 1, 2, "Q3-rows-eq-R"),        # Q = 3, A = 255, R = 85: n_rows = R * grid
    (1, 12, 1, 172, 1, 2, "Q3-rows-R-plus-1"),    # n_rows = R * grid + 1
    (1, 64, 1, 32, 1, 2, "Q16-rows-eq-R"),        # n_rows = 16 = R, n = 32 a power of two
    (1, 64, 1, 34, 1, 2, "Q16-rows-R-plus-1"),
    (1, 64, 1, 130, 1, 2, "three-strides"),       # grid 2, stride 32, 65 rows: 3 strides
    (2, 64, 9, 7, 2, 2, "ragged-2x2"),            # H % ph != 0 and W % pw != 0
    (1, 8, 4, 4, 2, 2, "2x2-pow2"),
    (4, 8, 2, 3, 2, 2, "Wo1-H-eq-ph"),            # Wo = 1, H = ph
    (2, 8, 5, 3, 2, 1, "generic-2x1"),            # H % ph != 0, generic
    (2, 12, 7, 5, 3, 2, "generic-3x2"),           # both ragged, generic, Q = 3
    (2, 16, 1, 10, 1, 3, "generic-1x3"),
    (2, 96, 1, 700, 1, 2, "Q24-nblk17"),          # A = 240, R = 10; 5 strides; nblk = 17
    (2, 516, 1, 6, 1, 2, "Q129-idle-lanes"),      # A = 129: R = 1 with 127 idle lanes
    (2, 768, 1, 18, 1, 1, "Q192"),
    (2, 1020, 1, 5, 1, 2, "Q255-ragged"),         # A = 255, R = 1
    (2, 1020, 3, 4, 2, 3, "Q255-generic-2x3"),
    (1, 1024, 1, 120, 1, 2, "nblk15"),
    (1, 64, 1, 2048, 1, 2, "nblk16"),
    (1, 1024, 1, 896, 1, 2, "nblk112"),
    (1, 1024, 1, 898, 1, 2, "nblk113"),
    (2, 512, 1, 1024, 1, 2, "nblk128"),
    (1, 1024, 1, 1032, 1, 2, "nblk129"),
    (1, 1024, 1, 8202, 1, 1, "stats-cap"),        # 1026 blocks of bn_stats_kernel capped at 1024; 9 strides
    (4, 1024, 1, 2051, 1, 2, "pooled-cap"),       # 4100 pooled rows: 1025 blocks capped at 1024
]
EDGE_IDS = [f"{t[6]}-{'x'.join(map(str, t[:6]))}" for t in BNRP_EDGE]
BIG = 1 << 21             # the two capped entries lie above it: the Gaussian eval case without conv_bias (a second
                          # generated case) is left to the exact data there; every other variant runs on every entry

Geometry = namedtuple("Geometry", "Q A R n n_rows fixed stats_nblk stats_uncapped pool_nblk pool_uncapped "
                                  "stride n_strides edge")


def _blocks(n4):
    return max(1, -(-n4 // (BN_THREADS * BLOCK_VECS)))


def geometry(B, C, H, W, ph, pw, *_):
    """The launch geometry the kernels derive from a shape (bn_shape, bn_blocks, pooled_blocks)."""
    Q = 1 if C == 2 else C // 4
    A = (BN_THREADS // Q) * Q
    R = A // Q
    n, n_rows = B * H * W, B * (H // ph) * (W // pw)
    su, pu = _blocks(n * Q), _blocks(n_rows * Q * 2)
    sn, pn = min(su, BN_MAX_BLOCKS), min(pu, BN_MAX_BLOCKS)
    fixed = (ph, pw) in ((1, 1), (1, 2), (2, 2))
    stride = pn * R                                    # pooled rows per grid step of the fixed-window loops
    # a thread starts an iteration at r with r + stride == n_rows (the last pair has one row only)
    edge = n_rows >= stride and ((n_rows - stride) // stride) % 2 == 0
    return Geometry(Q, A, R, n, n_rows, fixed, sn, su, pn, pu, stride, -(-n_rows // stride), edge)


def slack(B, C, H, W, ph, pw, *_):
    """Floats behind y (and behind dx) that a fixed-window pass would reach if it took the second row
    of its last pair one stride too far: the guards are at least this long where that is affordable,
    so such a slip lands in a guard and not outside the allocation."""
    g = geometry(B, C, H, W, ph, pw)
    Ho, Wo = H // ph, W // pw
    r = g.n_rows + g.stride - 1
    row = ((r // (Ho * Wo)) * H + (r // Wo % Ho) * ph + ph - 1) * W + (r % Wo) * pw + pw      # rows up to the window's end
    return max(0, row * C - B * H * W * C)


# ---- the rule ------------------------------------------------------------------------------------
def _windows(t, ph, pw):
    """(B, H, W, C) -> (B, Ho, Wo, C, ph * pw), window position i * pw + j last."""
    B, H, W, C = t.shape
    Ho, Wo = H // ph, W // pw
    t = t[:, :Ho * ph, :Wo * pw].reshape(B, Ho, ph, Wo, pw, C)
    return t.transpose(0, 1, 3, 5, 2, 4).reshape(B, Ho, Wo, C, ph * pw)


def _unwindows(w, shape, ph, pw):
    """The inverse: positions no window covers are 0."""
    B, H, W, C = shape
    Ho, Wo = H // ph, W // pw
    out = np.zeros(shape, w.dtype)
    out[:, :Ho * ph, :Wo * pw] = w.reshape(B, Ho, Wo, C, ph, pw).transpose(0, 1, 4, 2, 5, 3).reshape(B, Ho * ph, Wo * pw, C)
    return out


def affine32(gamma, beta, mean, invstd):
    """scale and shift as the kernels form them: float32 products and difference."""
    g, b, m, i = (np.asarray(t, F64) for t in (gamma, beta, mean, invstd))
    scale = f32(g * i)
    shift = f32(b - f32(m * scale))
    return scale, shift


def pool_fwd(y, scale, shift, ph, pw, skip=None):
    """(z, arg, best): arg the first maximum of relu(scale * y + shift) per window, best its value."""
    a = _windows(np.asarray(y, F64) * scale + shift, ph, pw)
    r = np.maximum(a, 0.0)
    arg = r.argmax(-1)                                  # numpy: the first of equal maxima
    best = np.take_along_axis(r, arg[..., None], -1)[..., 0]
    z = best if skip is None else best + np.asarray(skip, F64)
    return z, arg, best


def pool_bwd(dz, arg, best, shape, ph, pw):
    """dy (shape of y): dz at the arg-max of every window whose maximum is > 0, 0 elsewhere; and the
    mask of those positions."""
    hit = np.zeros(arg.shape + (ph * pw,), bool)
    np.put_along_axis(hit, arg[..., None], True, -1)
    hit &= (best > 0.0)[..., None]
    dy = np.where(hit, np.asarray(dz, F64)[..., None], 0.0)
    return _unwindows(dy, shape, ph, pw), _unwindows(hit, shape, ph, pw)


def batch_stats(y, eps):
    y = np.asarray(y, F64)
    n = y.shape[0] * y.shape[1] * y.shape[2]
    m = y.mean((0, 1, 2))
    var = ((y - m) ** 2).mean((0, 1, 2))
    return n, m, var, 1.0 / np.sqrt(var + eps)


def train_fwd(y, gamma, beta, running_mean, running_var, momentum, eps, mean_shift, batches_tracked, skip, ph, pw):
    n, m, var, istd = batch_stats(y, eps)
    out = SimpleNamespace(mean=f32(m), invstd=f32(istd), running_mean=None, running_var=None, batches_tracked=None)
    mom = float(F32(momentum))
    if running_mean is not None:
        shift = 0.0 if mean_shift is None else np.asarray(mean_shift, F64)
        out.running_mean = (1.0 - mom) * np.asarray(running_mean, F64) + mom * (m + shift)
        out.running_mean_unshifted = (1.0 - mom) * np.asarray(running_mean, F64) + mom * m
    if running_var is not None:
        unbiased = var * n / (n - 1.0) if n > 1 else var
        out.running_var = (1.0 - mom) * np.asarray(running_var, F64) + mom * f32(unbiased)
    if batches_tracked is not None:
        out.batches_tracked = int(batches_tracked) + 1
    out.scale, out.shift = affine32(gamma, beta, out.mean, out.invstd)
    out.z, out.arg, out.best = pool_fwd(y, out.scale, out.shift, ph, pw, skip)
    return out


def train_bwd(y, dz, gamma, beta, mean, invstd, ph, pw):
    """mean, invstd: the float32 values the forward left.  Also returns the three terms of the dx bound
    (train_int_case): |dy|, |c1|, |xhat * c2|."""
    y = np.asarray(y, F64)
    n = y.shape[0] * y.shape[1] * y.shape[2]
    scale, shift = affine32(gamma, beta, mean, invstd)
    _, arg, best = pool_fwd(y, scale, shift, ph, pw)
    dy, _ = pool_bwd(dz, arg, best, y.shape, ph, pw)
    xhat = (y - np.asarray(mean, F64)) * np.asarray(invstd, F64)
    out = SimpleNamespace(dbeta=dy.sum((0, 1, 2)), dgamma=(dy * xhat).sum((0, 1, 2)))
    out.coef = np.concatenate([f32(out.dbeta / n), f32(out.dgamma / n)])
    c1, c2 = out.coef[:len(scale)], out.coef[len(scale):]
    out.dx = scale * (dy - c1 - xhat * c2)
    out.dx_terms = np.abs(scale) * (np.abs(dy) + np.abs(c1) + np.abs(xhat * c2))
    out.dzero = np.zeros_like(scale)
    return out


def eval_affine(gamma, beta, running_mean, running_var, eps, conv_bias):
    mu = np.asarray(running_mean, F64)
    if conv_bias is not None:
        mu = f32(mu - np.asarray(conv_bias, F64))
    istd = f32(1.0 / np.sqrt(f32(np.asarray(running_var, F64) + float(F32(eps)))))
    return affine32(gamma, beta, mu, istd)


def eval_fwd(y, gamma, beta, running_mean, running_var, eps, conv_bias, skip, ph, pw):
    scale, shift = eval_affine(gamma, beta, running_mean, running_var, eps, conv_bias)
    return pool_fwd(y, scale, shift, ph, pw, skip)[0]


def eval_bwd(y, dz, gamma, beta, running_mean, running_var, eps, conv_bias, ph, pw):
    """dx = scale * dz at the arg-max, +0.0 elsewhere (np.where keeps the sign of no product)."""
    scale, shift = eval_affine(gamma, beta, running_mean, running_var, eps, conv_bias)
    _, arg, best = pool_fwd(y, scale, shift, ph, pw)
    dy, hit = pool_bwd(dz, arg, best, np.shape(y), ph, pw)
    return np.where(hit, scale * dy, 0.0)


# ---- data ----------------------------------------------------------------------------------------
def _rng(kind, shape):
    """A generator seeded by the kind of data and the shape."""
    return np.random.RandomState((sum((i + 3) * 7919 ** i * int(v) for i, v in enumerate(shape[:6])) + len(kind)) % 2 ** 31)


def _ints(rs, lo, hi, size, nonzero=False):
    v = rs.randint(lo, hi + 1, size=size).astype(F64)
    if nonzero:
        v[v == 0] = hi
    return v


def eval_int_case(B, C, H, W, ph, pw, *_):
    """Integer y, dz, skip, gamma (both signs), beta, running_mean, conv_bias; running_var in
    {1, 4, 16, 0.25}; eps = 0.  scale is +-{1, 2, 3} * {1, 1/2, 1/4, 2}, shift an integer multiple of
    1/4 below 64, so fma(y, scale, shift) and scale * dz are exact: float32 == float64 bit for bit.
    Windows are planted in turn (pooled row index mod 5): 0 whole window equal, 1 the maximum at the last position only, 2 every pre-activation < 0, 3 one
    pre-activation exactly 0 and the rest below it (where scale lets y hit it exactly), 4 as drawn."""
    shape = (B, C, H, W, ph, pw)
    rs = _rng("eval", shape)
    Ho, Wo = H // ph, W // pw
    c = SimpleNamespace(shape=shape, eps=0.0)
    sign = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    rs.shuffle(sign)
    if C >= 2:
        sign[0], sign[1] = 1.0, -1.0
    c.gamma = sign * _ints(rs, 1, 3, C)
    c.beta = _ints(rs, -1, 1, C)
    c.beta[0] = 0.0                                    # a == 0 exactly at y == mean in channel 0, whatever its scale
    c.running_mean = _ints(rs, -2, 2, C)
    c.conv_bias = _ints(rs, -1, 1, C)
    c.running_var = np.array([1.0, 4.0, 16.0, 0.25])[rs.randint(0, 4, size=C)]
    scale, shift = eval_affine(c.gamma, c.beta, c.running_mean, c.running_var, 0.0, c.conv_bias)
    mu = c.running_mean - c.conv_bias
    y = _ints(rs, -4, 4, (B, H, W, C))
    win = _windows(y, ph, pw).copy()                   # (B, Ho, Wo, C, N)
    kind = (np.arange(B * Ho * Wo) % 5).reshape(B, Ho, Wo)
    up = np.sign(scale)                                # the direction of y that raises a
    below = mu - up * 8.0                              # a = -8 |scale| + beta <= -2 + 1 < 0
    above = mu + up * 8.0
    win[kind == 0] = win[kind == 0][..., :1]
    win[kind == 1] = below[:, None]
    w1 = win[kind == 1]
    w1[..., -1] = above
    win[kind == 1] = w1
    win[kind == 2] = below[:, None] - up[:, None] * rs.randint(0, 3, size=win[kind == 2].shape)
    zero_at = mu - c.beta / scale                      # a == 0 there if representable
    hits = f32(zero_at) * scale + shift == 0.0
    w3 = np.broadcast_to(below[:, None], win[kind == 3].shape).copy()
    pos = rs.randint(0, ph * pw, size=w3.shape[:-1])
    np.put_along_axis(w3, pos[..., None], np.where(hits, f32(zero_at), below)[None, :, None], -1)
    win[kind == 3] = w3
    y[:, :Ho * ph, :Wo * pw] = _unwindows(win, (B, Ho * ph, Wo * pw, C), ph, pw)
    c.y = y
    c.dz = _ints(rs, -7, 7, (B, Ho, Wo, C), nonzero=True)
    c.skip = _ints(rs, -5, 5, (B, Ho, Wo, C))
    c.kind = kind
    return c


# (gamma, beta) of the first channels of train_int_case: with xhat = +-1 the two pre-activations are
# beta + gamma and beta - gamma — one positive; one exactly 0 and one positive; both positive; both
# negative; the lower exactly 0 with gamma < 0; both exactly <= 0 with one 0
_TRAIN_PAIRS = [(1, 0), (-2, 2), (3, 4), (2, -3), (-1, 1), (2, -2), (-3, 0), (1, 2)]


def train_int_case(B, C, H, W, ph, pw, *_):
    """y = m_c +- 2^k_c per channel (m_c an integer in [-3, 3], k_c in {0, 1}) with exactly n/2 plus
    signs, n = B * H * W even, placed by a seeded permutation per channel; eps = 0; momentum 0.5 or
    0.25; running statistics and mean_shift dyadic; gamma, beta, dz, skip integers.

    Then sum y = n m_c and sum y^2 = n (m_c^2 + 4^k_c), so mean = m_c, var = 4^k_c, invstd = 2^-k_c
    exactly, xhat = +-1, and every float32 partial sum the kernels form — of y, y^2 (also about a pivot
    K_c = y[0, c]: y - K_c is 0 or +-2^(k_c+1)), dy and dy * xhat — is an integer whose magnitude is at
    most the sum of |addend| over the channel, asserted below 2^24 here: exact in any order.
    BIT FOR BIT in every case: mean, invstd, running_mean, running_var (one float32 rounding of the
    unbiased variance, then exact), z, dbeta, dgamma, coef (one rounding of sum / n).
    dx = scale * (dy - c1 - xhat * c2) with c1 = float32(dbeta / n), c2 = float32(dgamma / n):
      * n a power of two: c1, c2 are multiples of 1/n below 8, dy an integer, xhat = +-1, scale a small
        multiple of 1/2 — every intermediate fits 24 bits: bit for bit;
      * otherwise the kernel rounds four times (-ffp-contract=off, nothing fuses): p = xhat * c2 is
        exact (xhat = +-1); t1 = fl(dy - c1), t2 = fl(t1 - p), dx = fl(scale * t2), and dx_uncovered's
        fl(-c1 - p), fl(scale * .) likewise.  With u = 2^-24, |t1| <= (1 + u)(|dy| + |c1|), each rounding
        adds at most u times the magnitude it rounds, all of which are below (1 + u)^2 S with
        S = |dy| + |c1| + |xhat * c2|; the error of dx is therefore below
        |scale| * S * ((1 + u)^3 - 1) < 3.01 u |scale| S, and allowing a fourth rounding (the product
        xhat * c2, exact here) 4 u |scale| S = 2^-22 |scale| S.  The test holds every element to
        2^-21 |scale| S, a factor 2 to spare."""
    shape = (B, C, H, W, ph, pw)
    rs = _rng("train", shape)
    n = B * H * W
    assert n % 2 == 0, shape
    Ho, Wo = H // ph, W // pw
    c = SimpleNamespace(shape=shape, eps=0.0, n=n, pow2=(n & (n - 1)) == 0)
    c.momentum = 0.5 if (B + W) % 2 else 0.25
    c.m = _ints(rs, -3, 3, C)
    c.k = rs.randint(0, 2, size=C)
    pairs = np.array([_TRAIN_PAIRS[i] if i < len(_TRAIN_PAIRS) else
                      (rs.choice([-3, -2, -1, 1, 2, 3]), rs.randint(-4, 5)) for i in range(C)], F64)
    order = rs.permutation(C)
    c.gamma, c.beta = pairs[order, 0], pairs[order, 1]
    signs = np.where(np.arange(n) < n // 2, 1.0, -1.0)
    y = np.empty((n, C))
    for ch in range(C):
        y[:, ch] = c.m[ch] + rs.permutation(signs) * 2.0 ** c.k[ch]
    c.y = y.reshape(B, H, W, C)
    c.running_mean = _ints(rs, -8, 8, C) / 4.0
    c.running_var = 2.0 ** rs.randint(-1, 3, size=C)
    c.mean_shift = _ints(rs, -6, 6, C) / 4.0
    c.batches_tracked = 41
    c.dz = _ints(rs, -7, 7, (B, Ho, Wo, C), nonzero=True)
    c.skip = _ints(rs, -5, 5, (B, Ho, Wo, C))
    # every float32 sum is an exact integer: sum |addend| per channel below 2^24
    pivot = c.y - c.y[0, 0, 0]
    for name, t in (("y", c.y), ("y^2", c.y ** 2), ("y - K", pivot), ("(y - K)^2", pivot ** 2), ("dz", c.dz)):
        top = float(np.abs(t).reshape(-1, C).sum(0).max())
        assert top < 2 ** 24 and np.array_equal(t, np.round(t)), (name, top, shape)
    return c


def margin_case(B, C, H, W, ph, pw, *_, mode="train", bias=True, max_rounds=60):
    """Gaussian y (mean 0.3, std 1.7, float32) and parameters as in tests/test_bnrp_gpu.py, then every
    element whose pre-activation a = scale * y + shift lies within MARGIN of 0, and the leader of every
    window whose two largest activations lie within MARGIN of each other (while the larger is > 0), is
    moved by 3 MARGIN / |scale| away from the band; statistics (training mode: the batch's own) and
    decisions are recomputed until no element is left inside.  Raises if that takes more than
    max_rounds.  c.rounds: how many it took.  bias=False: conv_bias is None (eval mode decides without it)."""
    shape = (B, C, H, W, ph, pw)
    rs = _rng("margin" + mode, shape)
    Ho, Wo = H // ph, W // pw
    c = SimpleNamespace(shape=shape, eps=1e-5, momentum=0.1, mode=mode)
    y = (rs.standard_normal((B, H, W, C)) * 1.7 + 0.3).astype(F32).astype(F64)
    c.gamma = f32((rs.rand(C) + 0.5) * np.where(rs.rand(C) < 0.25, -1.0, 1.0))
    c.beta = f32(rs.standard_normal(C) * 0.3)
    c.running_mean = f32(rs.standard_normal(C) * 0.1)
    c.running_var = f32(rs.rand(C) + 0.5)
    c.mean_shift = c.conv_bias = f32(rs.standard_normal(C) * 0.2)
    if not bias:
        c.conv_bias = None
    c.batches_tracked = 7
    c.dz = f32(rs.standard_normal((B, Ho, Wo, C)))
    c.skip = f32(rs.standard_normal((B, Ho, Wo, C)))
    N = ph * pw
    for c.rounds in range(max_rounds + 1):
        if mode == "train":
            _, m, _, istd = batch_stats(y, c.eps)
            scale, shift = affine32(c.gamma, c.beta, f32(m), f32(istd))
        else:
            scale, shift = eval_affine(c.gamma, c.beta, c.running_mean, c.running_var, c.eps, c.conv_bias)
        a = y * scale + shift
        step = 3 * MARGIN / np.abs(scale)
        move = np.where(np.abs(a) < MARGIN, np.where(a >= 0, 1.0, -1.0) * np.sign(scale) * step, 0.0)
        if N > 1:
            r = np.maximum(_windows(a, ph, pw), 0.0)
            top2 = np.partition(r, N - 2, -1)[..., N - 2:]
            close = (top2[..., 1] > 0) & (top2[..., 1] - top2[..., 0] < MARGIN)
            lead = np.zeros(r.shape, bool)
            np.put_along_axis(lead, r.argmax(-1)[..., None], True, -1)
            lead &= close[..., None]
            up = _unwindows(lead, y.shape, ph, pw)
            move = np.where(up, np.sign(scale) * step, move)
        if not move.any():
            break
        y = (y + move).astype(F32).astype(F64)
    else:
        raise AssertionError(f"margin_case{shape}, {mode}: no fixed point in {max_rounds} rounds")
    c.y = y
    return c


def conditioning_case(r, shape=(8, 64, 1, 250, 1, 2), sigma=1.7):
    """y ~ N(r * sigma, sigma) in float32: the batch mean is r standard deviations away from 0, which
    is what makes var = E[y^2] - E[y]^2 from float32 sums cancel.  Parameters as in margin_case."""
    B, C, H, W, ph, pw = shape
    rs = _rng("cond%d" % r, shape)
    c = SimpleNamespace(shape=shape, eps=1e-5, momentum=0.1, r=r)
    c.y = ((rs.standard_normal((B, H, W, C)) + r) * sigma).astype(F32).astype(F64)
    c.gamma = f32(rs.rand(C) + 0.5)
    c.beta = f32(rs.standard_normal(C) * 0.3)
    c.dz = f32(rs.standard_normal((B, H // ph, W // pw, C)))
    return c
