"""BatchNorm + ReLU + pool kernels for every ResNet9 ladder width and for eval mode: what can be
checked without a device — the ABI, the host-only support query, the refusals of the two eval entry
points (all of them come before any launch), and that CPU tensors keep the torch composition."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, models, train_model as tm

HIP_ERROR_INVALID_VALUE = 1
NEW = ["pcgmix_bnrp_supported", "pcgmix_bnrp_eval_fwd_f32", "pcgmix_bnrp_eval_bwd_f32"]
MAX_C = 1024          # documented limit (include/pcgmix_hip.h): C = 2 or a multiple of 4 up to 1024


def test_new_entry_points_are_declared_and_exported():
    lib = _lib.load()
    for n in NEW:
        assert n in _lib.SIGNATURES
        assert hasattr(lib, n)


def test_supported_covers_the_ladder_and_the_2d_model():
    lib = _lib.load()
    for name, widths in tm.RESNET9_LADDER.items():
        for c in widths:
            assert lib.pcgmix_bnrp_supported(c) == 1, (name, c)
    for c in (64, 128, 256, 512):
        assert lib.pcgmix_bnrp_supported(c) == 1
    assert all(lib.pcgmix_bnrp_supported(c) == 1 for c in range(4, MAX_C + 1, 4))


@pytest.mark.parametrize("c", [0, -4, 1, 3, 6, MAX_C + 4, MAX_C + 1, 2048, 4096])
def test_supported_refuses_other_widths(c):
    assert _lib.load().pcgmix_bnrp_supported(c) == 0


class _Buffers:
    """Host memory standing in for device pointers: every call below is refused before a launch."""

    def __init__(self):
        self.raw = ctypes.create_string_buffer(4096 + 64)
        base = ctypes.addressof(self.raw)
        self.p = (base + 63) // 64 * 64        # 64-byte aligned


def _eval_fwd(lib, p, *, y=True, gamma=True, rm=True, z=True, off=0, B=2, H=1, W=8, C=8, ph=1, pw=2):
    a = lambda on: ctypes.c_void_p(p + off) if on else None   # noqa: E731
    q = ctypes.c_void_p(p)
    return lib.pcgmix_bnrp_eval_fwd_f32(a(y), q if gamma else None, q, q if rm else None, q,
                                        ctypes.c_float(1e-5), None, None, q if z else None,
                                        B, H, W, C, ph, pw, None)


def _eval_bwd(lib, p, *, y=True, dz=True, rv=True, dx=True, off=0, B=2, H=1, W=8, C=8, ph=1, pw=2):
    a = lambda on: ctypes.c_void_p(p + off) if on else None   # noqa: E731
    q = ctypes.c_void_p(p)
    return lib.pcgmix_bnrp_eval_bwd_f32(a(y), q if dz else None, q, q, q, q if rv else None,
                                        ctypes.c_float(1e-5), None, q if dx else None,
                                        B, H, W, C, ph, pw, None)


@pytest.mark.parametrize("kw", [dict(y=False), dict(gamma=False), dict(rm=False), dict(z=False),
                                dict(C=3), dict(C=6), dict(C=MAX_C + 4), dict(B=0), dict(W=0),
                                dict(W=1, pw=2), dict(off=4), dict(off=8), dict(off=4, C=2)])
def test_eval_forward_refuses_before_any_launch(kw):
    buf = _Buffers()
    assert _eval_fwd(_lib.load(), buf.p, **kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [dict(y=False), dict(dz=False), dict(rv=False), dict(dx=False),
                                dict(C=3), dict(C=6), dict(C=MAX_C + 4), dict(B=0), dict(W=0),
                                dict(W=1, pw=2), dict(off=4), dict(off=8), dict(off=4, C=2)])
def test_eval_backward_refuses_before_any_launch(kw):
    buf = _Buffers()
    assert _eval_bwd(_lib.load(), buf.p, **kw) == HIP_ERROR_INVALID_VALUE


def test_supported_is_false_for_cpu_tensors():
    y = torch.zeros(2, 96, 1, 8).contiguous(memory_format=torch.channels_last)
    assert not models.BNReLUPoolFunction.supported(y)


@pytest.mark.parametrize("C,pool,with_skip", [(8, (1, 2), False), (96, None, True), (2, (2, 2), False)])
def test_cpu_eval_keeps_the_torch_composition(C, pool, with_skip):
    torch.manual_seed(C)
    conv = nn.Conv2d(3, C, 3, padding=1)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
    bn.eval()
    x = torch.randn(2, 3, 6, 8)
    with torch.no_grad():
        want = F.relu(F.batch_norm(conv(x), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))
        if pool is not None:
            want = F.max_pool2d(want, pool)
    skip = torch.randn_like(want) if with_skip else None
    if skip is not None:
        want = want + skip
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    with torch.no_grad():
        got = models.conv_bn_relu_pool(x, conv.weight, conv.bias, 1, bn, False, pool, skip)
    assert float((got - want).abs().max()) <= 1e-6
    assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
    assert int(bn.num_batches_tracked) == 0
