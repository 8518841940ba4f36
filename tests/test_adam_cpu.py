"""The Adam entry points without a GPU: the host-side argument checks (tests/test_sgd_cpu.py has
the SGD ones; both optimisers' multi-tensor launches go through one table fill)."""
import ctypes

import numpy as np

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

INVALID = 1                     # hipErrorInvalidValue


def test_adam_entry_points_refuse_bad_arguments():
    """Every refusal comes before anything is launched: fake addresses are never dereferenced."""
    lib = _lib.load()
    f = ctypes.c_float
    one = (ctypes.c_void_p * 1)(0x1000)
    null1 = (ctypes.c_void_p * 1)(None)
    n_ok, n_neg = (ctypes.c_longlong * 1)(4), (ctypes.c_longlong * 1)(-1)
    hp = (f(0.1), f(0.01), f(0.9), f(0.999), f(1e-8), f(1e-4))        # clip, lr, b1, b2, eps, wd
    eager, dev, red = (lib.pcgmix_adam_clip_multi_f32, lib.pcgmix_adam_clip_multi_dev_f32,
                       lib.pcgmix_adam_clip_multi_reduce_dev_f32)
    H = P = GR = 0x1000                                               # hyper block, partial, grads
    ok = (one, one, one, one, n_ok)                                   # p, g, m, v, n
    assert eager(-1, *ok, *hp, 1, None) == INVALID
    assert dev(-1, *ok, H, None) == INVALID
    assert red(-1, *ok, H, P, GR, 3, None) == INVALID
    for k in range(5):                                                # each table itself null
        tabs = ok[:k] + (None,) + ok[k + 1:]
        assert eager(1, *tabs, *hp, 1, None) == INVALID, k
        assert dev(1, *tabs, H, None) == INVALID, k
        assert red(1, *tabs, H, P, GR, 3, None) == INVALID, k
    for k in range(4):                                                # a null entry, n[i] > 0
        tabs = ok[:k] + (null1,) + ok[k + 1:]
        assert eager(1, *tabs, *hp, 1, None) == INVALID, k
        assert dev(1, *tabs, H, None) == INVALID, k
        assert red(1, *tabs, H, P, GR, 3, None) == INVALID, k
    neg = (one, one, one, one, n_neg)
    assert eager(1, *neg, *hp, 1, None) == INVALID
    assert dev(1, *neg, H, None) == INVALID
    assert red(1, *neg, H, P, GR, 3, None) == INVALID
    assert eager(1, *ok, *hp, 0, None) == INVALID                     # step < 1
    assert eager(1, *ok, *hp, -5, None) == INVALID
    assert dev(1, *ok, None, None) == INVALID                         # no hyper block
    assert red(1, *ok, None, P, GR, 3, None) == INVALID
    assert red(1, *ok, H, P, GR, 0, None) == INVALID                  # G <= 0
    assert red(1, *ok, H, P, GR, -1, None) == INVALID
    assert red(1, *ok, H, None, GR, 3, None) == INVALID
    assert red(1, *ok, H, P, None, 3, None) == INVALID
    assert eager(0, None, None, None, None, None, *hp, 1, None) == 0  # nothing to do
    assert dev(0, None, None, None, None, None, H, None) == 0
    assert red(0, *ok, H, P, GR, 3, None) == INVALID
    many = (ctypes.c_void_p * 33)(*[0x1000] * 33)
    assert red(33, many, many, many, many, (ctypes.c_longlong * 33)(*[4] * 33), H, P, GR, 3,
               None) == INVALID                                       # one table only
    out = np.full(8, 7.0, dtype=np.float32)
    assert lib.pcgmix_adam_hyper(*hp, 1, None) == INVALID
    assert lib.pcgmix_adam_hyper(*hp, 0, out.ctypes.data) == INVALID
    assert np.array_equal(out, np.full(8, 7.0, dtype=np.float32))     # refused: nothing written
    assert lib.pcgmix_adam_hyper(*hp, 1, out.ctypes.data) == 0
