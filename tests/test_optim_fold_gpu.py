"""The gradient reduction folded into the multi-tensor optimiser launch, for both update rules of
csrc/pcgmix_optim.hip (one kernel body, AdamRule / SgdRule), through the raw entry points: the
folded launch against ``pcgmix_potes_reduce_f32`` followed by ``*_multi_dev_f32``, on the layout of
test_train_gpu.py::test_adam_entry_points_share_one_update plus free tensors around a table block's
1024 elements.  G runs over the 256 threads that stride the partial rows."""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib
from test_sgd_cpu import EXACT, _dyadic, sgd_f64

pytestmark = pytest.mark.gpu

NGRAD = 212
STACK, OFFS = (40, 8, 160, 4), (0, 40, 48, 208)      # the conv stack's tensors inside grads[0 .. 212)
FREE = (1, 1024, 1025, 0)                            # gradients of their own; table blocks
ADAM = dict(clip=0.1, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4, step=3)
CASES = [(rule, G, True) for rule in ("adam", "sgd") for G in (1, 255, 256, 257, 513)]
CASES.append(("sgd", 257, False))                    # NULL momentum entries, momentum 0


def _hyper(lib, rule, mom, device):
    host = np.zeros(8, dtype=np.float32)
    f = ctypes.c_float
    if rule == "adam":
        a = ADAM
        _lib.check(lib.pcgmix_adam_hyper(f(a["clip"]), f(a["lr"]), f(a["b1"]), f(a["b2"]), f(a["eps"]),
                                         f(a["wd"]), a["step"], host.ctypes.data), "pcgmix_adam_hyper")
    else:
        _lib.check(lib.pcgmix_sgd_hyper(f(EXACT["clip"]), f(EXACT["lr"]), f(mom), f(EXACT["wd"]),
                                        host.ctypes.data), "pcgmix_sgd_hyper")
    return torch.from_numpy(host).to(device)


@pytest.mark.parametrize("rule,G,buffers", CASES)
def test_folded_reduction_equals_reduce_then_update(rule, G, buffers, device):
    """Dyadic partial rows (multiples of 2^-4, |x| <= 8: a column of 513 sums to a multiple of 2^-4
    below 2^13, exact in float32 in any order).  (1) the folded launch leaves grads == the float64
    column sums; (2) p and the state tensors == reduce, then update, on clones; (3) SGD with the
    power-of-two scalars of test_sgd_cpu.EXACT == the float64 rule, every intermediate being a
    float32 number."""
    lib = _lib.load()
    rs = np.random.RandomState(G)
    sizes = STACK + FREE
    mom = EXACT["mom"] if buffers else 0.0
    partial_h = _dyadic(rs, G * NGRAD).reshape(G, NGRAD)
    sums = partial_h.astype(np.float64).sum(axis=0)
    p_h = [_dyadic(rs, n) for n in sizes]
    gfree_h = [_dyadic(rs, n) for n in FREE]
    # state columns: Adam's exp_avg and exp_avg_sq (>= 0), SGD's momentum buffer (or none at all)
    if rule == "adam":
        state_h = [[_dyadic(rs, n) for n in sizes], [_dyadic(rs, n) ** 2 for n in sizes]]
    else:
        state_h = [[_dyadic(rs, n) if buffers else None for n in sizes]]
    up = lambda a: None if a is None else torch.from_numpy(a).to(device)      # noqa: E731
    partial, p0, gfree = up(partial_h), [up(a) for a in p_h], [up(a) for a in gfree_h]
    state0 = [[up(a) for a in col] for col in state_h]
    hyper = _hyper(lib, rule, mom, device)
    n = (ctypes.c_longlong * len(sizes))(*sizes)
    arr = ctypes.c_void_p * len(sizes)
    ptrs = lambda ts: arr(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    fold, dev = ((lib.pcgmix_adam_clip_multi_reduce_dev_f32, lib.pcgmix_adam_clip_multi_dev_f32)
                 if rule == "adam" else
                 (lib.pcgmix_sgd_clip_multi_reduce_dev_f32, lib.pcgmix_sgd_clip_multi_dev_f32))

    def run(folded):
        p = [t.clone() for t in p0]
        state = [[None if t is None else t.clone() for t in col] for col in state0]
        flat = torch.zeros(NGRAD, device=device)
        g = [flat[o:o + k] for o, k in zip(OFFS, STACK)] + gfree
        args = (len(p), ptrs(p), ptrs(g), *[ptrs(col) for col in state], n, hyper.data_ptr())
        if folded:
            _lib.check(fold(*args, partial.data_ptr(), flat.data_ptr(), G, stream), "folded")
        else:
            _lib.check(lib.pcgmix_potes_reduce_f32(partial.data_ptr(), flat.data_ptr(), G, stream),
                       "pcgmix_potes_reduce_f32")
            _lib.check(dev(*args, stream), "reduce, then update")
        return p, state, flat

    got, ref = run(True), run(False)
    torch.cuda.synchronize(device)
    host = lambda ts: [None if t is None else t.cpu().numpy() for t in ts]     # noqa: E731
    (p_a, st_a, flat_a), (p_b, st_b, flat_b) = ((host(p), [host(c) for c in st], f.cpu().numpy())
                                                for p, st, f in (got, ref))
    assert np.array_equal(flat_a.astype(np.float64), sums)                     # (1)
    assert np.array_equal(flat_b, flat_a)
    for i, k in enumerate(sizes):                                              # (2)
        assert np.array_equal(p_a[i], p_b[i]), ("p", i, k)
        for c, (ca, cb) in enumerate(zip(st_a, st_b)):
            assert (ca[i] is None and cb[i] is None) or np.array_equal(ca[i], cb[i]), ("state", c, i, k)
    assert not any(np.array_equal(a, b) for a, b, k in zip(p_a, p_h, sizes) if k >= 8)   # a step was made
    if rule == "sgd":                                                          # (3)
        g_h = [sums[o:o + k] for o, k in zip(OFFS, STACK)] + gfree_h
        for i, k in enumerate(sizes):
            want_p, want_buf = sgd_f64(p_h[i], g_h[i], state_h[0][i], EXACT["clip"], EXACT["lr"], mom,
                                       EXACT["wd"])
            assert np.array_equal(p_a[i].astype(np.float64), want_p), ("p", i, k)
            if buffers:
                assert np.array_equal(st_a[0][i].astype(np.float64), want_buf), ("buffer", i, k)
            else:
                assert want_buf is None and st_a[0][i] is None
