"""numpy restatement of what ``pcgmix_saliency_map_f32`` computes behind the model's backward pass
(include/pcgmix_hip.h): |grad| -> tail zeroed -> channel sum -> Gaussian -> per-row min/max
normalisation -> per-heart-state bins.  float32 throughout, in the kernel's order of operations;
a fused multiply-add is one float64 product and sum rounded to float32 (the product is exact in
float64, so this differs from a true fma only by a double rounding, far below the tolerances)."""
import math

import numpy as np

GAUSS = (57, 7.54)
BINS = (1, 4, 1, 8)
f32 = np.float32


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def taps(ksize, sigma):
    half = ksize // 2
    return np.array([1.0 / (sigma * math.sqrt(2.0 * math.pi)) * math.exp(-(x * x) / (2.0 * (sigma * sigma)))
                     for x in range(-half, half + 1)], dtype=np.float64).astype(f32)


def post(grad, frames, gauss=GAUSS):
    """(B,C,T) gradient -> (B,T) normalised map; the tail is zeroed once, BEFORE the smoothing."""
    ksize, sigma = gauss
    B, C, T = grad.shape
    a = np.abs(grad.astype(f32))
    a[np.broadcast_to(np.arange(T)[None, None, :] >= np.asarray(frames)[:, 4][:, None, None], a.shape)] = 0
    acc = np.zeros((B, T), f32)
    for c in range(C):
        acc = (acc + a[:, c]).astype(f32)
    half = ksize // 2
    pad = np.zeros((B, T + ksize - 1), f32)
    pad[:, half:half + T] = acc
    s = np.zeros((B, T), f32)
    for j, w in enumerate(taps(ksize, sigma)):
        s = fma32(w, pad[:, j:j + T], s)
    s = (s - s.min(1, keepdims=True)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (s / s.max(1, keepdims=True)).astype(f32)
    s[np.isnan(s)] = 0
    return s


def bins(sal, frames, n_bins=BINS):
    """(B,T) map -> (sal_bins (B,T) float32, values (B,N) float32, boundaries (B,N+1) int64)."""
    B, T = sal.shape
    N = int(sum(n_bins))
    out = np.zeros((B, T), f32)
    values = np.zeros((B, N), f32)
    bounds = np.zeros((B, N + 1), np.int64)
    for b in range(B):
        f = [int(v) for v in frames[b]]
        off = 0
        for k, n in enumerate(n_bins):
            lo, hi = f[k], f[k + 1]
            L = hi - lo
            spb = -(-L // n)
            scale = f32(L) / f32(n)
            i = np.arange(n)
            src = np.maximum((scale * (i.astype(f32) + f32(0.5))).astype(f32) - f32(0.5), f32(0)).astype(f32)
            i0 = src.astype(np.int64)
            i1 = np.minimum(i0 + 1, L - 1)
            l1 = (src - i0.astype(f32)).astype(f32)
            l0 = (f32(1) - l1).astype(f32)
            v = fma32(l0, sal[b, lo + i0], (l1 * sal[b, lo + i1]).astype(f32))
            values[b, off:off + n] = v
            bounds[b, off:off + n] = lo + i * spb
            out[b, lo:hi] = v[(np.arange(L)) // spb]
            off += n
        bounds[b, N] = f[4]
    return out, values, bounds
