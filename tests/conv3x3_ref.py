"""numpy restatement of pcgmix_conv3x3_nhwc_f32 (csrc/pcgmix_conv3x3.hip): Conv2d(k = 3x3, pad = 1,
stride 1) with the channels innermost.

    x (B, H, W, Cin), w (Cout, 3, 3, Cin) = [o][kh][kw][i]  ->  y (B, H, W, Cout)
    y[b, h, v, o] = sum over kh, kw, i of x[b, h + kh - 1, v + kw - 1, i] * w[o, kh, kw, i],
    zeros outside [0, H) x [0, W)

``conv3x3_int`` is exact in int64; ``conv3x3_f64`` also returns sum |x * w| per output, the scale of
the float32 rounding bound.  ``flip_transpose`` gives the weights with which the same convolution is
the layer's input gradient."""
import numpy as np


def tile(lib):
    """(TH, TW, KC) of the built library: the rows and columns of one tile of output pixels and the
    input channels of one K group (pcgmix_conv3x3_tile), so that shapes placed at tile edges stay
    there when the kernel changes."""
    return tuple(int(lib.pcgmix_conv3x3_tile(i)) for i in range(3))


def _padded(x):
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    return xp


def conv3x3_int(x, w):
    """int64 in, int64 out."""
    x = np.asarray(x, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    B, H, W, _ = x.shape
    xp = _padded(x)
    y = np.zeros((B, H, W, w.shape[0]), dtype=np.int64)
    for kh in range(3):
        for kw in range(3):
            y += xp[:, kh:kh + H, kw:kw + W] @ w[:, kh, kw, :].T
    return y


def conv3x3_f64(x, w):
    """(y, mag) in float64: mag[b, h, v, o] = sum |x * w| over the same products."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    B, H, W, _ = x.shape
    xp, ap, aw = _padded(x), _padded(np.abs(x)), np.abs(w)
    y = np.zeros((B, H, W, w.shape[0]))
    mag = np.zeros_like(y)
    for kh in range(3):
        for kw in range(3):
            y += xp[:, kh:kh + H, kw:kw + W] @ w[:, kh, kw, :].T
            mag += ap[:, kh:kh + H, kw:kw + W] @ aw[:, kh, kw, :].T
    return y, mag


def flip_transpose(w):
    """w'[i][kh][kw][o] = w[o][2 - kh][2 - kw][i]: conv3x3(dy, w') is the input gradient of conv3x3(x, w)."""
    return np.ascontiguousarray(np.asarray(w)[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


def int_case(B, H, W, Cin, Cout, seed=0):
    """x in [-4, 4], w in [-2, 2]: every partial sum is at most 9 * 1024 * 8 < 2**24 in magnitude, so
    float32 is exact in any order."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-4, 5, size=(B, H, W, Cin)).astype(np.int64)
    w = rs.randint(-2, 3, size=(Cout, 3, 3, Cin)).astype(np.int64)
    return x, w
