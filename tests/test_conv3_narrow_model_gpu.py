"""The three smallest ResNet9-1D models with EVERY Conv1d(k=3) layer on the project's kernels: the 2- and
8-channel layers on csrc/pcgmix_conv3_narrow.hip (``models.FUSED_CONV_NARROW``, which follows
``models.FUSED_CONV_TRAIN`` / PCGMIX_TRAIN_DETERMINISTIC where it is None), the others on the matrix
kernels as before.  The route, the frozen copy, bit-identical repeats, the weight gradients against
float64, and a three-step training trajectory, eager and captured.

The pattern is that of tests/test_conv3_train_gpu.py, with ``resnet9-5k``'s network
``ResNet9_myrtle(4, 2, [2, 4, 8, 16], 1248)`` at (3, 4, 2500) on dense noise in train() mode; the widths of
``resnet9-15k`` and ``resnet9-50k`` run the route, the repeats and the weight gradients as well.
"""
import copy
import random
import sys

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, models, train_model as tm
from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import train_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 7
SHAPE = (3, 4, 2500)
NETS = {"resnet9-5k": ([2, 4, 8, 16], 1248), "resnet9-15k": ([4, 8, 16, 32], 2496),
        "resnet9-50k": ([8, 16, 32, 64], 4992)}
N_CONV = 8
ENV = "PCGMIX_TRAIN_DETERMINISTIC"
nets = pytest.mark.parametrize("name", list(NETS))


def make_model(name="resnet9-5k"):
    filters, linear = NETS[name]
    assert tuple(filters) == tm.RESNET9_LADDER[name] and linear == models.resnet9_flat_features(2500, filters[-1])
    torch.manual_seed(SEED)
    m = models.ResNet9_myrtle(4, 2, filters, linear)
    g = torch.Generator().manual_seed(SEED + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            n = mod.num_features
            mod.running_mean.copy_(0.1 * torch.randn(n, generator=g))
            mod.running_var.copy_(0.5 + torch.rand(n, generator=g))
            mod.weight.data.copy_(0.5 + torch.rand(n, generator=g))
            mod.bias.data.copy_(0.1 * torch.randn(n, generator=g))
    return m.train()


def make_input():
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(SEED + 2))


def make_seed():
    s = torch.zeros(SHAPE[0], 2)
    s[torch.arange(SHAPE[0]), torch.tensor([0, 1, 0])] = 1
    return s


def conv_weights(m):
    return [(k, p) for k, p in m.named_parameters() if p.dim() == 3]


def parent_route(m):
    """(layers, input gradients) that the matrix kernels alone take in a training pass whose input wants
    no gradient: what the route was before the narrow kernels, and is with FUSED_CONV_NARROW = False."""
    lib = _lib.load()
    layers = dx = 0
    for n, (_, p) in enumerate(conv_weights(m)):
        cout, cin = int(p.shape[0]), int(p.shape[1])
        need_dx = n > 0
        if lib.pcgmix_conv3_supported(cin, cout) and lib.pcgmix_conv3_wgrad_supported(cin, cout) and (
                not need_dx or lib.pcgmix_conv3_supported(cout, cin)):
            layers += 1
            dx += int(need_dx)
    return layers, dx


def DETERMINISTIC():
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


@pytest.fixture()
def switch(monkeypatch):
    """``models.FUSED_CONV_TRAIN`` and ``models.FUSED_CONV_NARROW``, restored whatever happens; the
    environment variable starts unset."""
    monkeypatch.delenv(ENV, raising=False)
    saved = models.FUSED_CONV_TRAIN, models.FUSED_CONV_NARROW
    assert saved == (None, None)                          # the defaults
    yield
    models.FUSED_CONV_TRAIN, models.FUSED_CONV_NARROW = saved


@pytest.fixture()
def calls(monkeypatch):
    """Counts the convolutions through Conv3TrainFunction ('train') and Conv3Function ('frozen'), and
    the trainable route's input-gradient launches (every one builds the transposed weights: 'dx')."""
    n = {"train": 0, "frozen": 0, "dx": 0}

    def counting(key, real):
        def f(*a):
            n[key] += 1
            return real(*a)
        return f
    monkeypatch.setattr(models.Conv3TrainFunction, "apply", counting("train", models.Conv3TrainFunction.apply))
    monkeypatch.setattr(models.Conv3Function, "apply", counting("frozen", models.Conv3Function.apply))
    monkeypatch.setattr(models.Conv3TrainFunction, "_flipped",
                        staticmethod(counting("dx", models.Conv3TrainFunction._flipped)))
    return n


def fwd_bwd(m, x, seed):
    """One forward + backward on a copy of ``m``: (loss, {name: grad}, {name: buffer}, x.grad)."""
    m = copy.deepcopy(m)
    out = m(x)
    loss = (torch.log_softmax(out, 1) * seed).sum().neg()
    loss.backward()
    return (loss.detach(), {k: p.grad for k, p in m.named_parameters()},
            {k: b.detach().clone() for k, b in m.named_buffers()}, x.grad)


@nets
def test_route(device, switch, calls, monkeypatch, name):
    m, x, seed = make_model(name).to(device), make_input().to(device), make_seed().to(device)
    assert len(conv_weights(m)) == N_CONV
    p_layers, p_dx = parent_route(m)
    assert p_layers < N_CONV                              # the matrix kernels alone leave layers to MIOpen
    # the training switch alone: every convolution, and every input gradient but the first layer's
    models.FUSED_CONV_TRAIN = True
    on = fwd_bwd(m, x, seed)
    assert calls == {"train": N_CONV, "frozen": 0, "dx": N_CONV - 1}
    assert all(torch.isfinite(g).all() for g in on[1].values())
    # the narrow switch off beside it: the matrix kernels' layers only
    models.FUSED_CONV_NARROW = False
    with DETERMINISTIC():
        part = fwd_bwd(m, x, seed)
    assert calls == {"train": N_CONV + p_layers, "frozen": 0, "dx": N_CONV - 1 + p_dx}
    assert torch.allclose(on[0], part[0], rtol=1e-4)
    calls.update(train=0, dx=0)
    # everything unset, and the training switch off: MIOpen everywhere, the same bits either way (its
    # deterministic selection: the default one differs from call to call)
    res = []
    for train, narrow in ((None, None), (False, None), (False, False)):
        models.FUSED_CONV_TRAIN, models.FUSED_CONV_NARROW = train, narrow
        with DETERMINISTIC():
            res.append(fwd_bwd(m, x, seed))
    assert calls == {"train": 0, "frozen": 0, "dx": 0}
    for other in res[1:]:
        assert torch.equal(res[0][0], other[0])
        for k, g in res[0][1].items():
            assert torch.equal(g, other[1][k]), k
    assert torch.allclose(on[0], res[0][0], rtol=1e-4)
    # the narrow switch alone decides no route: it widens the routes that are taken
    models.FUSED_CONV_TRAIN, models.FUSED_CONV_NARROW = None, True
    with DETERMINISTIC():
        fwd_bwd(m, x, seed)
    assert calls == {"train": 0, "frozen": 0, "dx": 0}
    # the environment variable alone turns all of them on
    models.FUSED_CONV_TRAIN = models.FUSED_CONV_NARROW = None
    monkeypatch.setenv(ENV, "1")
    env_on = fwd_bwd(m, x, seed)
    assert calls == {"train": N_CONV, "frozen": 0, "dx": N_CONV - 1} and torch.equal(env_on[0], on[0])
    for k, g in on[1].items():
        assert torch.equal(g, env_on[1][k]), k
    monkeypatch.setenv(ENV, "0")
    with DETERMINISTIC():
        fwd_bwd(m, x, seed)
    assert calls["train"] == N_CONV


@nets
def test_frozen_copy_runs_every_convolution_and_matches_the_trainable_model(device, switch, calls, name):
    m, seed = make_model(name).to(device), make_seed().to(device)
    frozen = copy.deepcopy(m)
    for p in frozen.parameters():
        p.requires_grad_(False)
    lib = _lib.load()
    matrix = sum(int(lib.pcgmix_conv3_supported(int(p.shape[1]), int(p.shape[0]))) for _, p in conv_weights(m))
    # the defaults: the frozen routes keep MIOpen at the narrow widths, as before
    with torch.no_grad():
        copy.deepcopy(frozen)(make_input().to(device))
    assert calls == {"train": 0, "frozen": matrix, "dx": 0} and matrix < N_CONV
    for train, narrow in ((True, None), (None, True)):
        models.FUSED_CONV_TRAIN, models.FUSED_CONV_NARROW = train, narrow
        calls.update(train=0, frozen=0, dx=0)
        with torch.no_grad():
            copy.deepcopy(frozen)(make_input().to(device))
        assert calls == {"train": 0, "frozen": N_CONV, "dx": 0}
        xf = make_input().to(device).requires_grad_(True)
        ref = fwd_bwd(frozen, xf, seed)
        assert calls == {"train": 0, "frozen": 2 * N_CONV, "dx": 0}
        assert ref[3] is not None and torch.isfinite(ref[3]).all()
    # the trainable model with an input that wants a gradient: the same kernels, the same bits
    models.FUSED_CONV_TRAIN, models.FUSED_CONV_NARROW = True, None
    calls.update(train=0, frozen=0, dx=0)
    x = make_input().to(device).requires_grad_(True)
    live = fwd_bwd(m, x, seed)
    assert calls == {"train": N_CONV, "frozen": 0, "dx": N_CONV}
    assert live[3] is not None and live[3].shape == x.shape
    assert torch.equal(live[0], ref[0]) and torch.equal(live[3], ref[3])


@nets
def test_two_passes_from_the_same_state_are_bit_identical(device, switch, calls, name):
    m, x, seed = make_model(name).to(device), make_input().to(device), make_seed().to(device)
    models.FUSED_CONV_TRAIN = True
    a, b = fwd_bwd(m, x, seed), fwd_bwd(m, x, seed)
    assert calls["train"] == 2 * N_CONV
    assert torch.equal(a[0], b[0])
    assert len(a[1]) == len(list(m.parameters())) and all(g is not None for g in a[1].values())
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    moved = 0
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
        moved += int(not torch.equal(a[2][k], dict(m.named_buffers())[k]))
    assert moved == len(a[2])                             # the BatchNorm buffers did take a step


@nets
def test_weight_gradients_against_float64(device, switch, calls, record_property, name):
    m64 = make_model(name).double()
    want = fwd_bwd(m64, make_input().double(), make_seed().double())[1]
    m, x, seed = make_model(name).to(device), make_input().to(device), make_seed().to(device)
    models.FUSED_CONV_TRAIN = True
    hip = fwd_bwd(m, x, seed)[1]
    assert calls["train"] == N_CONV
    models.FUSED_CONV_TRAIN = False
    with DETERMINISTIC():
        mio = fwd_bwd(m, x, seed)[1]
    assert calls["train"] == N_CONV

    def err(got, k):
        return float((got[k].double().cpu() - want[k]).norm() / want[k].norm())
    names = [k for k, _ in conv_weights(m)]
    assert len(names) == N_CONV
    errs = {k: (err(hip, k), err(mio, k)) for k in names}
    for k, (e_hip, e_mio) in errs.items():
        record_property("wgrad_err_hip_" + k, e_hip)
        record_property("wgrad_err_miopen_deterministic_" + k, e_mio)
        print(f"{name} {k}: relative L2 error of the weight gradient HIP {e_hip:.3e}, "
              f"MIOpen deterministic {e_mio:.3e}")
    for k, (e_hip, e_mio) in errs.items():
        assert e_hip <= 4 * e_mio, k


def _trajectory(device, mode):
    """Three steps of train_step (or of the captured step) with ClipAdam on the ResNet9 replay's
    batches, from fixed seeds: (losses, parameters, buffers)."""
    args, batches = TC.resnet1d_args(), TC.resnet1d_batches()
    args.model = "resnet9-5k"
    torch.manual_seed(7)
    random.seed(7)
    np.random.seed(7)
    net = tm.build_model(args).to(device).train()
    opt, sched = tm.make_optimizer(args, net)
    assert isinstance(opt, tm.ClipAdam)
    labels_all = np.concatenate([b[1].numpy() for b in batches])
    crit = tm.SELCLoss(labels_all, 2, es=args.num_epochs + 1, device=device)
    sc = tm.step_counter_class()
    torch.cuda.manual_seed(4)
    B, C, T = batches[0][0].shape
    if mode == "graph":
        gstep = tm.GraphedTrainStep(args, net, opt, sched, crit, device, B, C, T)
        step = lambda b: gstep.step(b, 1, sc)                                  # noqa: E731
    else:
        step = lambda b: tm.train_step(args, net, b, device, opt, sched, crit, 1, sc)   # noqa: E731
    losses = [step((b[0].to(device),) + tuple(b[1:])).clone() for b in batches]
    torch.cuda.synchronize()
    return (torch.stack(losses).cpu(), {k: p.detach().cpu().clone() for k, p in net.named_parameters()},
            {k: b.detach().cpu().clone() for k, b in net.named_buffers()})


def test_training_trajectory_is_reproducible_eager_and_captured(device, switch, calls):
    models.FUSED_CONV_TRAIN = True
    a = _trajectory(device, "eager")
    assert calls["train"] == 3 * N_CONV and calls["dx"] == 3 * (N_CONV - 1)
    b = _trajectory(device, "eager")
    g = _trajectory(device, "graph")
    assert calls["train"] > 6 * N_CONV                    # the capture and its warm-ups went the same way
    assert torch.isfinite(a[0]).all()
    for other, what in ((b, "second eager run"), (g, "captured step")):
        assert torch.equal(a[0], other[0]), (what, a[0], other[0])
        for part in (1, 2):
            for k in a[part]:
                assert torch.equal(a[part][k], other[part][k]), (what, k)
    args = TC.resnet1d_args()
    args.model = "resnet9-5k"
    torch.manual_seed(7)
    first = dict(tm.build_model(args).named_parameters())
    assert any(not torch.equal(a[1][k], first[k].detach()) for k in a[1])      # the weights did move
