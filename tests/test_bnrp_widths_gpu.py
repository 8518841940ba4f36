"""BatchNorm + ReLU + MaxPool kernels (HIP, NHWC) at every ResNet9 ladder width and in eval mode,
against the torch composition in float64.  Tolerances are those of test_bnrp_gpu.py: forward
rtol 1e-4 / atol 2e-5, running statistics rtol 1e-5 / atol 1e-6, gradients beyond
1e-4 * max|ref| + 1e-6 in at most 1e-4 of the elements (ReLU / arg-max decisions within rounding of
a tie; torch's own float32 composition shows none on these shapes).  The check without that
allowance — every element, ties decided by value, guarded buffers, the block edges — is
tests/test_bnrp_edges_gpu.py."""
import argparse
import copy
import warnings

import pytest
import torch
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, models, saliency, train_model as tm

pytestmark = pytest.mark.gpu

# (B, C, H, W, ph, pw, extras): every new vectors-per-row count, more than one block, row counts
# that are no multiple of the rows per block, odd lengths, a ragged 2D window, the generic (1,4)
# window kernels, and the folded bias / skip / counter
TRAIN_SHAPES = [
    (4, 96, 1, 131, 1, 2, False),
    (3, 192, 1, 75, 1, 1, False),
    (2, 384, 1, 37, 1, 2, False),
    (2, 768, 1, 18, 1, 1, False),
    (5, 2, 1, 333, 1, 2, False),
    (8, 2, 1, 501, 1, 1, False),
    (2, 96, 9, 7, 2, 2, False),
    (2, 192, 1, 21, 1, 4, False),
    (3, 384, 1, 40, 1, 1, True),
]
EVAL_SHAPES = TRAIN_SHAPES + [(8, 64, 1, 250, 1, 2, False), (2, 128, 8, 8, 2, 2, True)]


def _inputs(B, C, H, W, ph, pw, extras, device):
    torch.manual_seed(B * C + W)
    y = (torch.randn(B, C, H, W, device=device) * 1.7 + 0.3).contiguous(memory_format=torch.channels_last)
    gamma = torch.rand(C, device=device) + 0.5
    beta = torch.randn(C, device=device) * 0.3
    rm, rv = torch.randn(C, device=device) * 0.1, torch.rand(C, device=device) + 0.5
    skip = bias = None
    if extras:
        skip = torch.randn(B, C, H // ph, W // pw, device=device).contiguous(memory_format=torch.channels_last)
        bias = torch.randn(C, device=device) * 0.2
    dz = torch.randn(B, C, H // ph, W // pw, device=device).contiguous(memory_format=torch.channels_last)
    return y, gamma, beta, rm, rv, skip, bias, dz


def _grad_ok(got, ref, name):
    scale = float(ref.abs().max()) + 1e-12
    diff = (got.double() - ref).abs()
    bad = (diff > 1e-4 * scale + 1e-6).float().mean().item()
    print(f"{name}: max err {float(diff.max()):.3g} of scale {scale:.3g}, fraction beyond the bound {bad:.3g}")
    assert bad <= 1e-4, (name, float(diff.max()), scale, bad)


def _pooled(t, ph, pw):
    return t if (ph, pw) == (1, 1) else F.max_pool2d(t, (ph, pw))


@pytest.mark.parametrize("B,C,H,W,ph,pw,extras", TRAIN_SHAPES)
def test_training_matches_torch_float64(B, C, H, W, ph, pw, extras, device):
    y, gamma, beta, rm, rv, skip, bias, dz = _inputs(B, C, H, W, ph, pw, extras, device)
    assert models.BNReLUPoolFunction.supported(y)
    y.requires_grad_(True); gamma.requires_grad_(True); beta.requires_grad_(True)
    rm2, rv2 = rm.clone().double(), rv.clone().double()
    counter = torch.tensor(7, device=device) if extras else None
    if extras:
        skip.requires_grad_(True); bias.requires_grad_(True)
    z = models.BNReLUPoolFunction.apply(y, gamma, beta, rm, rv, 0.1, 1e-5, ph, pw, skip, bias, counter)
    assert z.shape == (B, C, H // ph, W // pw) and z.is_contiguous(memory_format=torch.channels_last)
    z.backward(dz)

    yd = y.detach().double().requires_grad_(True)
    gd, bd = gamma.detach().double().requires_grad_(True), beta.detach().double().requires_grad_(True)
    pre = yd if bias is None else yd + bias.detach().double().view(1, -1, 1, 1)
    want = _pooled(F.relu(F.batch_norm(pre, rm2, rv2, gd, bd, True, 0.1, 1e-5)), ph, pw)
    if extras:
        want = want + skip.detach().double()
    want.backward(dz.double())
    err = float((z.detach().double() - want.detach()).abs().max())
    print(f"z: max err {err:.3g}")
    assert torch.allclose(z.detach().double(), want.detach(), rtol=1e-4, atol=2e-5), err
    assert torch.allclose(rm.double(), rm2, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rv.double(), rv2, rtol=1e-5, atol=1e-6)
    for got, ref, name in ((y.grad, yd.grad, "dx"), (gamma.grad, gd.grad, "dgamma"), (beta.grad, bd.grad, "dbeta")):
        _grad_ok(got, ref, name)
    if extras:
        assert int(counter) == 8
        assert torch.equal(skip.grad, dz) and not bias.grad.any()


@pytest.mark.parametrize("B,C,H,W,ph,pw,extras", EVAL_SHAPES)
def test_eval_matches_torch_float64(B, C, H, W, ph, pw, extras, device):
    y, gamma, beta, rm, rv, skip, bias, dz = _inputs(B, C, H, W, ph, pw, extras, device)
    assert models.BNReLUPoolFunction.supported(y)
    y.requires_grad_(True)
    if extras:
        skip.requires_grad_(True)
    rm0, rv0 = rm.clone(), rv.clone()
    z = models.BNReLUPoolEvalFunction.apply(y, gamma, beta, rm, rv, 1e-5, ph, pw, skip, bias)
    assert z.shape == (B, C, H // ph, W // pw) and z.is_contiguous(memory_format=torch.channels_last)
    z.backward(dz)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)

    yd = y.detach().double().requires_grad_(True)
    pre = yd if bias is None else yd + bias.double().view(1, -1, 1, 1)
    want = _pooled(F.relu(F.batch_norm(pre, rm.double(), rv.double(), gamma.double(), beta.double(),
                                       False, 0.0, 1e-5)), ph, pw)
    if extras:
        want = want + skip.detach().double()
    want.backward(dz.double())
    err = float((z.detach().double() - want.detach()).abs().max())
    print(f"z: max err {err:.3g}")
    assert torch.allclose(z.detach().double(), want.detach(), rtol=1e-4, atol=2e-5), err
    _grad_ok(y.grad, yd.grad, "dx")
    if extras:
        assert torch.equal(skip.grad, dz)


def _eval_dx(y, gamma, beta, ph, pw):
    C = y.shape[1]
    rm, rv = torch.zeros(C, device=y.device), torch.ones(C, device=y.device)
    if y.is_cuda:
        z = models.BNReLUPoolEvalFunction.apply(y, gamma, beta, rm, rv, 1e-5, ph, pw)
    else:
        z = F.max_pool2d(F.relu(F.batch_norm(y, rm, rv, gamma, beta, False, 0.0, 1e-5)), (ph, pw))
    dz = torch.arange(1, z.numel() + 1, dtype=torch.float32, device=y.device).view(z.shape)
    (dx,) = torch.autograd.grad(z, y, dz)
    return dx


@pytest.mark.parametrize("B,C,H,W,ph,pw", [(2, 64, 1, 32, 1, 2), (1, 8, 4, 4, 2, 2)])
def test_flat_windows_route_to_the_first_maximum(B, C, H, W, ph, pw, device):
    torch.manual_seed(3)
    per_window = torch.rand(B, C, H // ph, W // pw) + 0.5          # positive activation, all ties
    y = per_window.repeat_interleave(ph, 2).repeat_interleave(pw, 3).contiguous(memory_format=torch.channels_last)
    gamma, beta = torch.rand(C) + 0.5, torch.rand(C) * 0.1
    want = _eval_dx(y.clone().requires_grad_(True), gamma, beta, ph, pw)       # torch, CPU, float32
    got = _eval_dx(y.to(device).requires_grad_(True), gamma.to(device), beta.to(device), ph, pw)
    assert int((want != 0).sum()) == B * C * (H // ph) * (W // pw)
    assert torch.equal(got.cpu() != 0, want != 0)
    # activation exactly 0: the ReLU passes nothing
    zero = torch.zeros(B, C, H, W, device=device).contiguous(memory_format=torch.channels_last)
    dx = _eval_dx(zero.requires_grad_(True), gamma.to(device), torch.zeros(C, device=device), ph, pw)
    assert not dx.any()


# float4 with a fixed window; float2 with an uncovered last column; the generic window
@pytest.mark.parametrize("B,C,H,W,ph,pw", [(2, 8, 4, 4, 2, 2), (2, 2, 1, 9, 1, 2), (1, 8, 1, 12, 1, 4)])
def test_eval_dx_zeros_are_exact_for_either_sign_of_gamma(B, C, H, W, ph, pw, device):
    """Off the arg-max, under a closed ReLU and at uncovered positions the eval input gradient is
    +0.0, bit for bit, also in channels with gamma < 0 (a product scale * 0 would give -0.0 there)."""
    y, gamma, beta, rm, rv, _, _, dz = _inputs(B, C, H, W, ph, pw, False, device)
    gamma = gamma * (1 - 2 * (torch.arange(C, device=device) % 2))          # +, -, +, - ...
    y.requires_grad_(True)
    models.BNReLUPoolEvalFunction.apply(y, gamma, beta, rm, rv, 1e-5, ph, pw).backward(dz)
    dx = y.grad
    assert (dx == 0).any()
    assert not dx.view(torch.int32)[dx == 0].any()

    yd = y.detach().double().requires_grad_(True)
    want = _pooled(F.relu(F.batch_norm(yd, rm.double(), rv.double(), gamma.double(), beta.double(),
                                       False, 0.0, 1e-5)), ph, pw)
    want.backward(dz.double())
    _grad_ok(dx, yd.grad, "dx")


def test_new_paths_are_deterministic(device):
    torch.manual_seed(0)
    outs = []
    y = torch.randn(8, 96, 1, 1250, device=device).contiguous(memory_format=torch.channels_last)
    g, b = torch.rand(96, device=device) + 0.5, torch.randn(96, device=device)
    for _ in range(2):
        yy, gg = y.clone().requires_grad_(True), g.clone().requires_grad_(True)
        z = models.BNReLUPoolFunction.apply(yy, gg, b, None, None, 0.1, 1e-5, 1, 2)
        z.square().sum().backward()
        outs.append((z.detach().clone(), yy.grad.clone(), gg.grad.clone()))
    assert all(torch.equal(a, c) for a, c in zip(*outs))
    outs = []
    y = torch.randn(8, 128, 1, 1250, device=device).contiguous(memory_format=torch.channels_last)
    g, b = torch.rand(128, device=device) + 0.5, torch.randn(128, device=device)
    rm, rv = torch.randn(128, device=device) * 0.1, torch.rand(128, device=device) + 0.5
    for _ in range(2):
        yy = y.clone().requires_grad_(True)
        z = models.BNReLUPoolEvalFunction.apply(yy, g, b, rm, rv, 1e-5, 1, 2)
        z.square().sum().backward()
        outs.append((z.detach().clone(), yy.grad.clone()))
    assert all(torch.equal(a, c) for a, c in zip(*outs))


# ------------------------------------------------------------------------------------ models
_EVAL_FUNCTION = models.BNReLUPoolEvalFunction


class _CountingEval(_EVAL_FUNCTION):
    """The eval Function with a call counter: agreement of values alone is what the torch-op
    fallback gives too."""
    calls = 0

    @staticmethod
    def forward(ctx, *args):
        _CountingEval.calls += 1
        return _EVAL_FUNCTION.forward(ctx, *args)


@pytest.fixture
def strict(monkeypatch):
    """No fallback goes unnoticed: the once-only warning set is cleared, warnings are errors, and
    calls of the eval Function are counted."""
    monkeypatch.setattr(models, "_WARNED", set())
    monkeypatch.setattr(models, "FUSED_BN", True)
    _CountingEval.calls = 0
    monkeypatch.setattr(models, "BNReLUPoolEvalFunction", _CountingEval)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        # torch's own notice from torch.backends.cudnn.flags() on ROCm (the deterministic frozen pass)
        warnings.filterwarnings("ignore", message="cuDNN Benchmark limit is not supported in MIOpen")
        yield _CountingEval


def _ladder_model(name, device):
    torch.manual_seed(5)
    args = argparse.Namespace(dataset="PhysioNet", model=name, num_classes=2, num_channels=4, sig_len=64)
    return tm.build_model(args).to(device)


@pytest.mark.parametrize("name", ["resnet9-5k", "resnet9-1.4m", "resnet9-5m"])
def test_ladder_models_run_on_the_kernels(name, device, strict, monkeypatch):
    model = _ladder_model(name, device)
    twin = copy.deepcopy(model)
    torch.manual_seed(9)
    x = torch.randn(4, 4, 64, device=device)
    seed = torch.randn(4, 2, device=device)

    def train_pass(m):
        xx = x.clone().requires_grad_(True)
        out = m.train()(xx)
        (gx,) = torch.autograd.grad(out, xx, seed)
        return out.detach(), gx

    out, gx = train_pass(model)                            # raises on a fallback warning
    assert strict.calls == 0
    monkeypatch.setattr(models, "FUSED_BN", False)
    want, gwant = train_pass(twin)
    monkeypatch.setattr(models, "FUSED_BN", True)
    err = float((out - want).abs().max())
    print(f"{name} train logits: max err {err:.3g}")
    assert err <= 1e-4
    _grad_ok(gx, gwant.double(), f"{name} d logits / d input")

    with torch.no_grad():
        got = model.eval()(x)
        assert strict.calls == 8                           # all eight blocks
        monkeypatch.setattr(models, "FUSED_BN", False)
        want = twin.eval()(x)
    assert strict.calls == 8
    err = float((got - want).abs().max())
    print(f"{name} eval logits: max err {err:.3g}")
    assert err <= 1e-5


def test_frozen_saliency_pass_uses_the_eval_kernels(device, strict, monkeypatch):
    monkeypatch.setattr(saliency, "DETERMINISTIC_FROZEN_PASS", True)
    torch.manual_seed(2)
    model = models.ResNet9(4, 2, linear=models.resnet9_flat_features(64)).to(device).eval()
    with torch.no_grad():
        for m in model.modules():                          # statistics as after some training
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    for p in model.parameters():
        p.requires_grad_(False)
    x = torch.randn(4, 4, 64, device=device)
    tgt = F.one_hot(torch.tensor([0, 1, 1, 0], device=device), 2)
    got = saliency.input_gradient(model, x, tgt)
    assert strict.calls == 8
    monkeypatch.setattr(models, "FUSED_BN", False)
    want = saliency.input_gradient(model, x, tgt)
    monkeypatch.setattr(models, "FUSED_BN", True)
    assert strict.calls == 8
    _grad_ok(got, want.double(), "frozen input gradient")

    # the same pass captured into a graph and replayed on the batch
    xs, seed = torch.zeros_like(x), saliency.class_seed(tgt)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(2):
            saliency.input_gradient_seeded(model, xs, seed)
    torch.cuda.current_stream(device).wait_stream(side)
    calls = strict.calls
    graph = torch.cuda.CUDAGraph()
    with _lib.capture_without_gc(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = saliency.input_gradient_seeded(model, xs, seed)
    assert strict.calls == calls + 8
    xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize(device)
    assert torch.equal(out, got)
