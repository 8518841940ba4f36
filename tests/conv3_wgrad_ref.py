"""numpy restatement of pcgmix_conv3_wgrad_nlc_f32 (csrc/pcgmix_conv3_wgrad.hip): the weight gradient of
Conv1d(k = 3, pad = 1, stride 1) with the channels innermost.

    x (B, L, Cin), dy (B, L, Cout)  ->  dw (Cout, 3, Cin) = [o][tap][i]
    dw[o, tap, i] = sum over b, l of dy[b, l, o] * x[b, l + tap - 1, i],   x zero outside [0, L)

``wgrad_int`` is exact in int64; ``wgrad_f64`` also returns sum |dy * x| per output, the scale of the
float32 rounding bound."""
import ctypes

import numpy as np

from conv3_ref import _padded


def tile(lib):
    """(TK, MO, NI) of the built library: the positions of one K tile and the output and input channels
    of one block tile (pcgmix_conv3_wgrad_tile), so that shapes placed at tile edges stay there when the
    kernel changes."""
    return tuple(int(lib.pcgmix_conv3_wgrad_tile(k)) for k in range(3))


def plan(lib, B, L, Cin, Cout):
    """(return code, splits, workspace bytes) of pcgmix_conv3_wgrad_plan."""
    s, n = ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = lib.pcgmix_conv3_wgrad_plan(B, L, Cin, Cout, ctypes.byref(s), ctypes.byref(n))
    return int(rc), int(s.value), int(n.value)


def _wgrad(x, dy):
    B, L, _ = x.shape
    xp = _padded(x)
    flat = dy.reshape(B * L, -1)
    return np.stack([flat.T @ xp[:, tap:tap + L].reshape(B * L, -1) for tap in range(3)], axis=1)


def wgrad_int(x, dy):
    """int64 in, int64 out."""
    return _wgrad(np.asarray(x, dtype=np.int64), np.asarray(dy, dtype=np.int64))


def wgrad_f64(x, dy):
    """(dw, mag) in float64: mag[o, tap, i] = sum |dy * x| over the same products."""
    x = np.asarray(x, dtype=np.float64)
    dy = np.asarray(dy, dtype=np.float64)
    return _wgrad(x, dy), _wgrad(np.abs(x), np.abs(dy))


def int_case(B, L, Cin, Cout, seed=0):
    """x in [-4, 4], dy in [-2, 2]: every partial sum is at most 8 * B * L in magnitude, below 2**24
    for B * L <= 2**21, so float32 is exact in any order."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-4, 5, size=(B, L, Cin)).astype(np.int64)
    dy = rs.randint(-2, 3, size=(B, L, Cout)).astype(np.int64)
    return x, dy
