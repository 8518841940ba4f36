"""ResNet9-2D with its frozen Conv2d(3x3) layers on the HIP kernels (models.Conv3x3Function,
csrc/pcgmix_conv3x3.hip): the evaluation forward, the frozen saliency pass (eager and captured), the
routes that must stay on MIOpen, and the reference's recorded '(saloptenv|saloptsum)durratiomixup'
runs on spectrograms with ``models.FUSED_CONV2D = True``.

The network is ``models2d.ResNet9_myrtle(1, 2, 512)`` in eval mode with randomised BatchNorm statistics
at (4, 1, 32, 48): the maps are 32x48, 16x24, 8x12, 4x6 — non-square, and every kernel of the file runs
(1 -> 64, the matrix kernel at 128 / 256 / 512 columns, 64 -> 1 in the backward).  The input is dense
noise.  The float64 baseline is a CPU copy of the same model, computed once.

Decidable samples.  The float32 legs are compared with float64 autograd on the samples that have no
undecidable unit in the float64 CPU model: a ReLU whose pre-activation is below TAU = 1e-6 in
magnitude, or a max-pool window whose two largest entries (the largest > 0) are closer than TAU.  TAU
is the float32 error of the pre-activations as derived in tests/test_conv3_model_gpu.py (max |z32 -
z64| of torch's own float32 CPU pass is 1.5e-7 .. 6.2e-7 there).  A unit of the last blocks sees the
whole 32x48 image, so a sample is kept or left out whole; at most half of the samples may be left out,
which the seed below — picked on the build host from the float64 model alone — satisfies (the fixture
asserts it): about eight of the 1.4 M decisions of a batch are within TAU, so most seeds touch every sample.
Measured on an MI355X, max |err| against float64: logits HIP 1.57e-7, MIOpen 3.97e-8 (scale 0.19: 10 and
2.6 units in the last place of eight numbers); input gradient on the decidable samples HIP 3.3e-9, MIOpen
default and deterministic 3.9e-9 (scale 7.7e-3), and the same figures over all four samples — neither
undecidable unit flipped in any leg.  The recorded runs: maps 3.6e-7 from the reference's in all three files.
"""
import argparse
import copy
import os
import sys

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import augmentations, hostprep, models, models2d, saliency
from conftest import GOLDEN, Args, golden_files, load_golden

pytestmark = pytest.mark.gpu

SEED = 97            # of the seeds 0 .. 119 only 31 and 97 leave two samples whole; 97: two units, in samples 0 and 3
SHAPE, LINEAR = (4, 1, 32, 48), 512
N_CONV = 8
TAU = 1e-6          # float64 margin below which float32 cannot decide a ReLU / max-pool: see the docstring
MAX_LEFT_OUT = 0.5  # share of the samples the comparison may leave out
CASES2D = golden_files("salopt2d_")


def make_model():
    torch.manual_seed(SEED)
    m = models2d.ResNet9_myrtle(1, 2, LINEAR)
    g = torch.Generator().manual_seed(SEED + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            n = mod.num_features
            mod.running_mean.copy_(0.1 * torch.randn(n, generator=g))
            mod.running_var.copy_(0.5 + torch.rand(n, generator=g))
            mod.weight.data.copy_(0.5 + torch.rand(n, generator=g))
            mod.bias.data.copy_(0.1 * torch.randn(n, generator=g))
    return m.eval()


def make_input():
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(SEED + 2))


def make_seed():
    s = torch.zeros(SHAPE[0], 2)
    s[torch.arange(SHAPE[0]), torch.tensor([0, 1, 0, 1])] = 1
    return s


def undecidable_units(m, x):
    """[(kind, layer index, sample, channel, row, column, margin)]: every ReLU whose float64
    pre-activation is below TAU in magnitude and every max-pool window whose two largest entries (the
    largest > 0) are closer than TAU.  ``m`` is the float64 CPU model: its blocks run as plain modules."""
    units, seen = [], {"relu": 0, "pool": 0}

    def add(kind, hit, margin):
        i = seen[kind]
        seen[kind] += 1
        for b, c, r, v in hit.nonzero().tolist():
            units.append((kind, i, b, c, r, v, float(margin[b, c, r, v])))

    def bn_hook(mod, inp, out):
        add("relu", out.abs() < TAU, out)

    def pool_hook(mod, inp, out):
        k, a = mod.kernel_size, inp[0]
        B, C, H, W = a.shape
        nh, nw = H // k, W // k
        win = a[:, :, :nh * k, :nw * k].reshape(B, C, nh, k, nw, k).permute(0, 1, 2, 4, 3, 5).reshape(B, C, nh, nw, k * k)
        top = win.topk(2, dim=-1).values
        gap = top[..., 0] - top[..., 1]
        add("pool", (top[..., 0] > 0) & (gap < TAU), gap)
    hooks = [mod.register_forward_hook(bn_hook if isinstance(mod, torch.nn.BatchNorm2d) else pool_hook)
             for mod in m.modules() if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.MaxPool2d))]
    with torch.no_grad():
        m(x)
    for h in hooks:
        h.remove()
    assert seen == {"relu": N_CONV, "pool": 4}
    return units


@pytest.fixture(scope="module")
def baseline():
    """float64 logits, input gradient, the decidable samples (B,) and the undecidable units of the CPU
    copy; never written to afterwards."""
    m = make_model().double()
    x = make_input().double().requires_grad_(True)
    out = m(x)
    (grad,) = torch.autograd.grad(out, x, make_seed().double())
    units = undecidable_units(m, x.detach())
    keep = torch.ones(SHAPE[0], dtype=torch.bool)
    for u in units:
        keep[u[2]] = False
    assert 1.0 - float(keep.float().mean()) <= MAX_LEFT_OUT, units
    return out.detach(), grad.detach(), keep, units


@pytest.fixture()
def switches():
    """The module switches the legs flip, restored whatever happens."""
    names = [(models, "FUSED_CONV"), (models, "FUSED_CONV2D"), (models, "FUSED_CONV2D_NOGRAD"),
             (saliency, "DETERMINISTIC_FROZEN_PASS"), (saliency, "USE_GRAPHS")]
    saved = [getattr(mod, n) for mod, n in names]
    yield
    for (mod, n), v in zip(names, saved):
        setattr(mod, n, v)
    saliency.set_saliency_model(None)


@pytest.fixture()
def calls(monkeypatch):
    """Counts the convolutions that go through Conv3x3Function."""
    n = [0]
    real = models.Conv3x3Function.apply

    def counting(*a):
        n[0] += 1
        return real(*a)
    monkeypatch.setattr(models.Conv3x3Function, "apply", counting)
    return n


def DETERMINISTIC():
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def frozen(m, device):
    m = copy.deepcopy(m).to(device).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def test_routing(device, switches, calls):
    m, x, seed = frozen(make_model(), device), make_input().to(device), make_seed().to(device)
    models.FUSED_CONV, models.FUSED_CONV2D, models.FUSED_CONV2D_NOGRAD = True, True, True
    with torch.no_grad():
        m(x)
    assert calls[0] == N_CONV
    saliency.DETERMINISTIC_FROZEN_PASS = None
    g_hip = saliency.input_gradient_seeded(m, x, seed)
    assert calls[0] == 2 * N_CONV and g_hip.shape == x.shape
    # the pass with an input gradient has a switch of its own
    models.FUSED_CONV2D = False
    with DETERMINISTIC():
        g_off = saliency.input_gradient_seeded(m, x, seed)
        models.FUSED_CONV, models.FUSED_CONV2D = False, True
        g_mio = saliency.input_gradient_seeded(m, x, seed)
    assert calls[0] == 2 * N_CONV and torch.equal(g_off, g_mio)
    # evaluation: the second switch off, or FUSED_CONV off, is MIOpen — the same bits under its
    # deterministic selection
    with torch.no_grad(), DETERMINISTIC():
        same = m(x)
        models.FUSED_CONV, models.FUSED_CONV2D, models.FUSED_CONV2D_NOGRAD = True, True, False
        off = m(x)
    assert calls[0] == 2 * N_CONV and torch.equal(off, same)
    models.FUSED_CONV2D_NOGRAD = True
    # trainable weights, in train and in eval mode
    out = {}
    for fused in (True, False):
        models.FUSED_CONV = fused
        for training in (False, True):
            t = copy.deepcopy(make_model()).to(device).train(training)
            xin = x.clone().requires_grad_(True)
            with DETERMINISTIC():                  # MIOpen's default selection differs from call to call
                y = t(xin)
                (gx,) = torch.autograd.grad(y.sum(), xin)
            out[fused, training] = (y.detach(), gx)
    assert calls[0] == 2 * N_CONV
    for training in (False, True):
        for a, b in zip(out[True, training], out[False, training]):
            assert torch.isfinite(a).all() and torch.equal(a, b)
    # frozen weights, gradients recorded, but nothing to differentiate: MIOpen as well
    models.FUSED_CONV = True
    y = m(x)
    assert calls[0] == 2 * N_CONV and not y.requires_grad
    # a CPU tensor never reaches the function
    with torch.no_grad():
        frozen(make_model(), "cpu")(make_input())
    assert calls[0] == 2 * N_CONV


def test_logits_under_no_grad(device, baseline, switches, calls, record_property):
    m, x = frozen(make_model(), device), make_input().to(device)
    want = baseline[0]
    models.FUSED_CONV, models.FUSED_CONV2D_NOGRAD = True, True
    with torch.no_grad():
        hip = m(x)
        hip2 = m(x)
    assert calls[0] == 2 * N_CONV and torch.equal(hip, hip2)
    models.FUSED_CONV = False
    with torch.no_grad():
        mio = m(x)
    assert calls[0] == 2 * N_CONV
    e_hip = float((hip.double().cpu() - want).abs().max())
    e_mio = float((mio.double().cpu() - want).abs().max())
    record_property("logits_err_hip", e_hip)
    record_property("logits_err_miopen", e_mio)
    print(f"2D logits: max |err| HIP {e_hip:.3e}, MIOpen {e_mio:.3e}, scale {float(want.abs().max()):.3e}")
    assert e_hip <= 4 * e_mio


def test_input_gradient_of_a_frozen_copy(device, baseline, switches, calls, record_property):
    m, x, seed = frozen(make_model(), device), make_input().to(device), make_seed().to(device)
    want, keep, units = baseline[1], baseline[2], baseline[3]

    def leg(fused, det):
        models.FUSED_CONV, models.FUSED_CONV2D, saliency.DETERMINISTIC_FROZEN_PASS = fused, True, det
        return saliency.input_gradient_seeded(m, x, seed)
    hip = leg(True, None)
    assert calls[0] == N_CONV
    hip2 = leg(True, None)
    mio = leg(False, False)
    det = leg(False, True)
    assert calls[0] == 2 * N_CONV
    assert hip.shape == x.shape and torch.equal(hip, hip2)
    legs = (("hip", hip), ("miopen_default", mio), ("miopen_deterministic", det))
    per_sample = {k: (v.double().cpu() - want).abs().flatten(1).max(1).values for k, v in legs}
    err = {k: float(v[keep].max()) for k, v in per_sample.items()}
    everywhere = {k: float(v.max()) for k, v in per_sample.items()}
    for k, v in err.items():
        record_property("grad_err_" + k, v)
    for k, v in everywhere.items():
        record_property("grad_err_everywhere_" + k, v)
    print("2D input gradient: max |err| on decidable samples " + ", ".join(f"{k} {v:.3e}" for k, v in err.items())
          + "; everywhere " + ", ".join(f"{k} {v:.3e}" for k, v in everywhere.items())
          + f"; scale {float(want.abs().max()):.3e}, samples kept {keep.tolist()}")
    # a sample that leaves the float64 gradient by more than 100x the decidable error: which unit?
    for k, v in per_sample.items():
        for b in (v > 100 * max(err.values())).nonzero().flatten().tolist():
            print(f"  {k}: sample {b} differs by {float(v[b]):.3e}: its undecidable units "
                  f"{[u for u in units if u[2] == b]}")
    print("  undecidable units: " + "; ".join(str(u) for u in units))
    assert err["hip"] <= 4 * err["miopen_deterministic"]


def _frames(B, W):
    fr = np.zeros((B, 5), dtype=np.int64)
    for b in range(B):
        fr[b] = [0, 6 + b, 14 + b, 25 + b, W - 2 * b]
    return fr


def test_captured_pass_equals_eager(device, switches, calls):
    saliency.set_saliency_model(make_model().to(device))
    models.FUSED_CONV, models.FUSED_CONV2D = True, True
    B, W = SHAPE[0], SHAPE[3]
    frames = _frames(B, W)
    tgt = torch.nn.functional.one_hot(torch.tensor([0, 1, 0, 1]), 2).to(device)
    args = Args("x", model="resnet9")

    def maps(data):
        return saliency.get_saliency_maps(args, device, data, tgt, frames, dim=2).clone()
    outs = {}
    for use in (False, True):
        saliency.USE_GRAPHS = use
        outs[use] = [maps(torch.randn(SHAPE, generator=torch.Generator().manual_seed(s)).to(device)) for s in (1, 2)]
    assert calls[0] >= 2 * N_CONV                        # eager passes; the capture's warm-ups add more
    assert len(saliency._GRAPHS) == 1
    for a, b in zip(outs[False], outs[True]):
        assert a.shape == (B, W) and float(a.max()) == 1.0 and torch.equal(a, b)
    assert not torch.equal(outs[True][0], outs[True][1])
    # weights written in place after the capture: the replay builds w' from the weights as they are
    # now, as the eager pass does
    data = torch.randn(SHAPE, generator=torch.Generator().manual_seed(2)).to(device)
    with torch.no_grad():
        for mod in saliency._INJECTED.modules():
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.mul_(1.25)
    saliency.USE_GRAPHS = True
    replayed = maps(data)
    saliency.USE_GRAPHS = False
    eager = maps(data)
    assert len(saliency._GRAPHS) == 1
    assert torch.equal(replayed, eager) and not torch.equal(replayed, outs[True][1])
    # with the route off a 2D pass is MIOpen's and is not captured
    models.FUSED_CONV2D = False
    saliency.USE_GRAPHS = True
    n = calls[0]
    maps(data)
    assert calls[0] == n and len(saliency._GRAPHS) == 1


# ---- the reference's recorded runs (tests/golden/make_golden_salopt2d.py) ----
def _golden_args2d(method, experiments):
    return argparse.Namespace(
        dataset="PhysioNet(spec128)", model="resnet9", method=method, num_epochs=50, batch_size=6,
        n_fraction=1.0, op="adam", use_sched=True, lr_max=0.01, train_balance=True, num_channels=1,
        grad_clip=0.1, seed_data=1100001, valid=False, seed=4, EXPERIMENTS=experiments,
        num_classes=2, sample_rate=1000)


@pytest.mark.parametrize("path", CASES2D, ids=lambda p: p.split("/")[-1][:-4])
def test_reference_parity_resnet9_2d(path, device, switches, calls, tmp_path, record_property):
    """'(saloptenv|saloptsum)durratiomixup' on spectrograms with the ResNet9-2D 'base' checkpoint on the
    HIP kernels and MIOpen's DEFAULT selection for whatever is left to it: the maps are within 1e-5 of
    the reference's recorded ones and the same bits in two passes and eager against captured; fed the
    recorded maps, displacements and output are the reference's exactly."""
    sys.path.insert(0, GOLDEN)
    from make_golden_salopt2d import SEED2D
    g = load_golden(path)
    base = _golden_args2d("base", str(tmp_path))
    exp = saliency.experiment_dir(base)
    os.makedirs(exp, exist_ok=True)
    torch.manual_seed(SEED2D)
    net = models2d.ResNet9(num_classes=2)
    torch.save({"module." + k: v for k, v in net.state_dict().items()}, os.path.join(exp, "model.pth"))
    saliency.set_saliency_model(None)
    saliency._LOADED.clear()
    models.FUSED_CONV, models.FUSED_CONV2D = True, True
    saliency.DETERMINISTIC_FROZEN_PASS = None
    args = _golden_args2d(g["method"], str(tmp_path))
    data = torch.from_numpy(g["x"]).to(device)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(g["labels"]), 2).to(device)
    B, _, F, W = data.shape
    try:
        saliency.USE_GRAPHS = True
        sal = saliency.get_saliency_maps(args, device, data, tgt, g["frames"], dim=2).clone()
        assert calls[0] >= N_CONV
        sal2 = saliency.get_saliency_maps(args, device, data, tgt, g["frames"], dim=2).clone()
        saliency.USE_GRAPHS = False
        sal3 = saliency.get_saliency_maps(args, device, data, tgt, g["frames"], dim=2).clone()
    finally:
        saliency._LOADED.clear()
    eps = float(np.abs(sal.cpu().numpy() - g["sal"]).max())
    record_property("map_err", eps)
    print(f"resnet9-2d saliency maps ({os.path.basename(path)}): max |own - reference| = {eps:.3e}")
    assert sal.shape == (B, W) and torch.equal(sal, sal2) and torch.equal(sal, sal3)
    assert eps <= 1e-5
    # the recorded maps fed in: search and splice alone
    ref_sal = torch.from_numpy(g["sal"]).to(device)
    fr = torch.from_numpy(np.ascontiguousarray(g["frames"], dtype=np.int32)).to(device)
    mx = torch.from_numpy(np.ascontiguousarray(g["mix"], dtype=np.int32)).to(device)
    mode = 0 if "(saloptenv" in g["method"] else 1
    disp = saliency.optimal_displacements(ref_sal, fr.data_ptr(), mx.data_ptr(), float(np.float32(g["lam"])),
                                          mode, B, W)
    assert np.array_equal(disp.cpu().numpy().astype(np.int64), g["disp"])
    plan = hostprep.make_plan(g["method"], g["labels"], g["frames"], g["wav"], g["step"], B, F, is2d=True, n_cols=W)
    assert plan.fired and plan.salopt_mode == mode and np.array_equal(plan.mix, g["mix"])
    assert plan.lam64 == float(g["lam"])
    y = augmentations.apply_plan(plan, data.view(B, F, W), g["frames"], ref_sal).view(B, 1, F, W)
    assert np.array_equal(y.cpu().numpy(), g["y"])
