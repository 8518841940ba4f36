"""ClipSGD without a GPU: the ABI additions, the host-side argument checks, the optimiser choice,
and the float64 restatement of the kernel's per-element rule against clip_grad_value_ +
torch.optim.SGD on inputs whose arithmetic is exact (tests/test_sgd_gpu.py runs the kernel on
the same inputs)."""
import argparse
import ctypes
import functools

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, train_model as tm

SGD_SYMBOLS = ("pcgmix_sgd_hyper", "pcgmix_sgd_clip_multi_f32", "pcgmix_sgd_clip_multi_dev_f32",
               "pcgmix_sgd_clip_multi_reduce_dev_f32")
INVALID = 1                     # hipErrorInvalidValue

# ------------------------------------------------------------------ the rule, restated in float64
def sgd_f64(p, g, buf, clip, lr, mom, wd):
    """One step of the rule of csrc/pcgmix_optim.hip (sgd_clip_update) on float64 arrays: returns
    (p, buf).  ``buf`` None: no buffer yet (a zero buffer gives the same: mom * 0 + g == g)."""
    g = np.asarray(g, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    if clip > 0:
        g = np.clip(g, -clip, clip)
    if wd != 0:
        g = g + wd * p
    if mom != 0:
        buf = g.copy() if buf is None else mom * np.asarray(buf, dtype=np.float64) + g
        g = buf
    return p - lr * g, buf


# ------------------------------------------------------------------ exact-arithmetic inputs
SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049)      # and 0: the tensor in the middle
EXACT = dict(clip=2.0, lr=0.25, mom=0.5, wd=0.5)        # powers of two
EXACT_STEPS = 4
VARIANTS = {"all": {}, "clip0": {"clip": 0.0}, "wd0": {"wd": 0.0}, "mom0": {"mom": 0.0}}


def exact_sizes(count):
    sizes = [SIZES[-1 - i % len(SIZES)] for i in range(count)]
    if count > 1:
        sizes[count // 2] = 0
    return sizes


def _dyadic(rs, n):
    return (rs.randint(-128, 129, size=n) / 16.0).astype(np.float32)     # multiples of 2^-4, |x| <= 8


@functools.lru_cache(maxsize=None)
def exact_case(count, variant="all"):
    """Inputs and the torch CPU result: dict(hp, p0, grads[step][tensor], p, buf) — float32 numpy
    arrays; ``buf`` entries are None without momentum.  Gradients are dyadic draws times the step
    number, so clip = 2 bites on some elements and not on others."""
    hp = dict(EXACT, **VARIANTS[variant])
    rs = np.random.RandomState(1000 + count)
    sizes = exact_sizes(count)
    p0 = [_dyadic(rs, n) for n in sizes]
    grads = [[(s * _dyadic(rs, n)).astype(np.float32) for n in sizes] for s in range(1, EXACT_STEPS + 1)]
    params = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in p0]
    opt = torch.optim.SGD(params, lr=hp["lr"], momentum=hp["mom"], weight_decay=hp["wd"])
    for step in grads:
        for q, g in zip(params, step):
            q.grad = torch.from_numpy(g.copy())
        if hp["clip"] > 0:
            torch.nn.utils.clip_grad_value_(params, hp["clip"])
        opt.step()
    buf = [opt.state.get(q, {}).get("momentum_buffer") for q in params]    # (no entry without momentum)
    return dict(hp=hp, sizes=sizes, p0=p0, grads=grads, p=[q.detach().numpy() for q in params],
                buf=[None if b is None else b.numpy() for b in buf], state_dict=opt.state_dict())


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("count", [1, 32, 33, 65])
def test_f64_rule_equals_torch_cpu_bit_for_bit(count, variant):
    """The float64 restatement == clip_grad_value_ + torch.optim.SGD in float32 on the CPU, bit for
    bit: every intermediate of these inputs is a float32 number, so a kernel that follows the rule
    must give the same bits whatever it contracts."""
    case = exact_case(count, variant)
    hp = case["hp"]
    p = [a.astype(np.float64) for a in case["p0"]]
    buf = [None] * len(p)
    for step in case["grads"]:
        for i, g in enumerate(step):
            p[i], buf[i] = sgd_f64(p[i], g, buf[i], hp["clip"], hp["lr"], hp["mom"], hp["wd"])
    clipped = sum(int((np.abs(g) > hp["clip"]).sum()) for s in case["grads"] for g in s)
    total = sum(g.size for s in case["grads"] for g in s)
    assert hp["clip"] == 0 or 0 < clipped < total
    for i, want in enumerate(case["p"]):
        assert np.array_equal(p[i].astype(np.float32), want) and np.array_equal(p[i], want.astype(np.float64)), i
        if hp["mom"] != 0:
            assert np.array_equal(buf[i], case["buf"][i].astype(np.float64)), i
        else:
            assert buf[i] is None and case["buf"][i] is None
    if hp["mom"] == 0:
        assert case["state_dict"]["state"] == {}


def test_four_element_case_of_the_issue():
    p = torch.nn.Parameter(torch.tensor([1.5, -8.0, 0.0625, 3.25]))
    g0 = np.array([0.5, -3.0, 7.9375, -0.0625], dtype=np.float32)
    opt = torch.optim.SGD([p], lr=0.25, momentum=0.5, weight_decay=0.5)
    q, buf = p.detach().numpy().astype(np.float64), None
    for s in range(1, 5):
        p.grad = torch.from_numpy(s * g0)
        q, buf = sgd_f64(q, s * g0, buf, 2.0, 0.25, 0.5, 0.5)
        torch.nn.utils.clip_grad_value_([p], 2.0)
        opt.step()
    assert np.array_equal(q, p.detach().numpy().astype(np.float64))


# ------------------------------------------------------------------ ABI
def test_sgd_symbols_exported_and_abi_unchanged():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in SGD_SYMBOLS:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert _lib.ABI_VERSION == 25 and _lib.load().pcgmix_abi_version() == 25


def test_sgd_hyper_layout():
    lib = _lib.load()
    out = np.full(8, 7.0, dtype=np.float32)
    f = ctypes.c_float
    assert lib.pcgmix_sgd_hyper(f(0.1), f(0.01), f(0.95), f(1e-4), out.ctypes.data) == 0
    assert np.array_equal(out, np.array([0.1, 1e-4, 0.95, 0.01, 0, 0, 0, 0], dtype=np.float32))
    assert lib.pcgmix_sgd_hyper(f(0.1), f(0.01), f(0.95), f(1e-4), None) == INVALID


def test_sgd_entry_points_refuse_bad_arguments():
    """Every refusal comes before anything is launched: fake addresses are never dereferenced."""
    lib = _lib.load()
    f = ctypes.c_float
    one = (ctypes.c_void_p * 1)(0x1000)
    null1 = (ctypes.c_void_p * 1)(None)
    n_ok, n_neg = (ctypes.c_longlong * 1)(4), (ctypes.c_longlong * 1)(-1)
    hp = (f(0.1), f(0.01))
    eager, dev, red = (lib.pcgmix_sgd_clip_multi_f32, lib.pcgmix_sgd_clip_multi_dev_f32,
                       lib.pcgmix_sgd_clip_multi_reduce_dev_f32)
    assert eager(-1, one, one, one, n_ok, *hp, f(0.5), f(0.0), None) == INVALID
    assert eager(1, None, one, one, n_ok, *hp, f(0.5), f(0.0), None) == INVALID
    assert eager(1, one, None, one, n_ok, *hp, f(0.5), f(0.0), None) == INVALID
    assert eager(1, one, one, one, None, *hp, f(0.5), f(0.0), None) == INVALID
    assert eager(1, one, one, one, n_neg, *hp, f(0.5), f(0.0), None) == INVALID
    assert eager(1, one, one, None, n_ok, *hp, f(0.5), f(0.0), None) == INVALID      # momentum without buffers
    assert eager(1, one, one, null1, n_ok, *hp, f(0.5), f(0.0), None) == INVALID
    assert eager(1, null1, one, one, n_ok, *hp, f(0.0), f(0.0), None) == INVALID
    assert eager(0, None, None, None, None, *hp, f(0.5), f(0.0), None) == 0           # nothing to do
    assert dev(1, one, one, one, n_ok, None, None) == INVALID                        # no hyper block
    assert dev(1, one, one, None, n_ok, 0x1000, None) == INVALID                     # the table itself
    assert dev(1, one, one, one, n_neg, 0x1000, None) == INVALID
    assert red(1, one, one, one, n_ok, 0x1000, 0x1000, 0x1000, 0, None) == INVALID   # G <= 0
    assert red(1, one, one, one, n_ok, 0x1000, None, 0x1000, 3, None) == INVALID
    assert red(1, one, one, one, n_ok, 0x1000, 0x1000, None, 3, None) == INVALID
    assert red(0, one, one, one, n_ok, 0x1000, 0x1000, 0x1000, 3, None) == INVALID
    assert red(1, one, one, one, n_neg, 0x1000, 0x1000, 0x1000, 3, None) == INVALID
    many = (ctypes.c_void_p * 33)(*[0x1000] * 33)
    assert red(33, many, many, many, (ctypes.c_longlong * 33)(*[4] * 33), 0x1000, 0x1000, 0x1000, 3,
               None) == INVALID                                                       # one table only


# ------------------------------------------------------------------ the optimiser class
def _args(**kw):
    a = argparse.Namespace(op="SGD", lr_max=0.01, weight_decay=1e-4, grad_clip=0.1, use_sched=True,
                           num_steps=10)
    a.__dict__.update(kw)
    return a


def test_make_optimizer_on_cpu_parameters_stays_torch_sgd():
    assert tm.FUSED_SGD is True
    net = torch.nn.Linear(3, 2)
    opt, sched = tm.make_optimizer(_args(), net)
    assert type(opt) is torch.optim.SGD and sched is not None
    assert tm.clips_outside_optimizer(_args(), opt)
    assert opt.param_groups[0]["momentum"] == pytest.approx(0.95)        # OneCycleLR cycles it


def test_clip_sgd_refuses_what_the_kernel_does_not_implement():
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError):
        tm.ClipSGD(p, lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(NotImplementedError):
        tm.ClipSGD(p, lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(NotImplementedError):
        tm.ClipSGD(p, lr=0.1, maximize=True)
    opt = tm.ClipSGD(p, lr=0.1, weight_decay=1e-4, clip_value=0.1)
    assert isinstance(opt, torch.optim.SGD) and opt.can_capture()
    assert set(opt.param_groups[0]) == set(torch.optim.SGD(p, lr=0.1).param_groups[0])
    assert not tm.clips_outside_optimizer(_args(), opt)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=0.1, total_steps=10)
    assert opt.param_groups[0]["momentum"] == pytest.approx(0.95) and sched is not None
    bad = torch.optim.SGD(p, lr=0.1, momentum=0.9, nesterov=True).state_dict()
    with pytest.raises(NotImplementedError):
        opt.load_state_dict(bad)
