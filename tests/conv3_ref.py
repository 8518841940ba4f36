"""numpy restatement of pcgmix_conv3_nlc_f32 (csrc/pcgmix_conv3.hip): Conv1d(k = 3, pad = 1, stride 1)
with the channels innermost.

    x (B, L, Cin), w (Cout, 3, Cin) = [o][tap][i]  ->  y (B, L, Cout)
    y[b, l, o] = sum over tap, i of x[b, l + tap - 1, i] * w[o, tap, i],   zeros outside [0, L)

``conv3_int`` is exact in int64; ``conv3_f64`` also returns sum |x * w| per output, the scale of the
float32 rounding bound.  ``flip_transpose`` gives the weights with which the same convolution is the
layer's input gradient."""
import numpy as np


def tile(lib):
    """(TM, KC) of the built library: the positions of one M tile and the input channels of one K
    group (pcgmix_conv3_tile), so that shapes placed at tile edges stay there when the kernel changes."""
    return int(lib.pcgmix_conv3_tile(0)), int(lib.pcgmix_conv3_tile(1))


def _padded(x):
    B, L, C = x.shape
    xp = np.zeros((B, L + 2, C), dtype=x.dtype)
    xp[:, 1:L + 1] = x
    return xp


def conv3_int(x, w):
    """int64 in, int64 out."""
    x = np.asarray(x, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    B, L, _ = x.shape
    xp = _padded(x)
    y = np.zeros((B, L, w.shape[0]), dtype=np.int64)
    for tap in range(3):
        y += xp[:, tap:tap + L] @ w[:, tap, :].T
    return y


def conv3_f64(x, w):
    """(y, mag) in float64: mag[b, l, o] = sum |x * w| over the same products."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    B, L, _ = x.shape
    xp, ap, aw = _padded(x), _padded(np.abs(x)), np.abs(w)
    y = np.zeros((B, L, w.shape[0]))
    mag = np.zeros_like(y)
    for tap in range(3):
        y += xp[:, tap:tap + L] @ w[:, tap, :].T
        mag += ap[:, tap:tap + L] @ aw[:, tap, :].T
    return y, mag


def flip_transpose(w):
    """w'[i][tap][o] = w[o][2 - tap][i]: conv3(dy, w') is the input gradient of conv3(x, w)."""
    return np.ascontiguousarray(np.asarray(w)[:, ::-1, :].transpose(2, 1, 0))


def int_case(B, L, Cin, Cout, seed=0):
    """x in [-4, 4], w in [-2, 2]: every partial sum is at most 3 * 1024 * 8 < 2**24 in magnitude, so
    float32 is exact in any order."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-4, 5, size=(B, L, Cin)).astype(np.int64)
    w = rs.randint(-2, 3, size=(Cout, 3, Cin)).astype(np.int64)
    return x, w
