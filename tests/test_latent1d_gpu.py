"""1D latentmixup on the GPU.  First part: the latent tail+loss kernel
(``pcgmix_potes_head_loss_latent_fwd_f32``: manifold mixup of the 20
hidden features inside the fused Potes head) against the same maths in torch on the same inputs
and the same dropout bytes.  Second part (further down): ``augment()`` against the reference's
recordings, the drop-in path's gradients, fused step == drop-in step, the reference's train_epoch
trajectories, the drivers and the launch list.  The restatement runs in float64 on the device: it is the value both
float32 computations approximate.  Tolerances are those of
``test_head_gpu.test_fused_head_loss_equals_head_then_celoss``: loss and logits rtol 1e-5 /
atol 1e-6, gradients rtol 1e-4 / atol 1e-7 + 1e-4 * max|g|."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

pytestmark = pytest.mark.gpu


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _permutations(labels: np.ndarray, rng: np.random.Generator):
    """identity / a random same-label permutation / one with fixed points (every second row of a
    same-label permutation sent back to itself where that keeps it a permutation: 2-cycles and
    fixed points only)."""
    B = labels.shape[0]
    ident = np.arange(B)
    same = ident.copy()
    for c in np.unique(labels):
        idx = np.nonzero(labels == c)[0]
        same[idx] = rng.permutation(idx)
    fixed = ident.copy()
    for c in np.unique(labels):
        idx = np.nonzero(labels == c)[0]
        for a, b in zip(idx[0::3], idx[1::3]):           # pairs swap, every third row stays
            fixed[a], fixed[b] = b, a
    return {"identity": ident, "same-label": same, "fixed-points": fixed}


class _Head:
    """Inputs of one case on the device, the C ABI calls, and the float64 restatement."""

    def __init__(self, B, K, C, drop, soft, device):
        g = torch.Generator(device="cpu").manual_seed(1000 * B + K + C + 7 * drop + 13 * soft)
        r = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
        self.B, self.K, self.C, self.dev = B, K, C, device
        self.feat = r(B, K).relu_().to(device)
        self.w1 = (r(20, K) / K ** 0.5).to(device)
        self.b1 = r(20).to(device)
        self.w2 = (r(C, 20) / 4).to(device)
        self.b2 = r(C).to(device)
        self.labels = torch.randint(0, C, (B,), generator=g)
        if soft:
            t = torch.rand(B, C, generator=g)
            self.target = (t / t.sum(1, keepdim=True) * 1.3).to(device)   # need not sum to 1
        else:
            self.target = self.labels.to(torch.uint8).to(device)
        self.soft = soft
        if drop:
            self.m1 = (torch.rand(B, K, generator=g) > 0.25).to(torch.uint8).to(device)
            self.m2 = (torch.rand(B, 20, generator=g) > 0.5).to(torch.uint8).to(device)
            self.s1, self.s2, self.thr = 1 / 0.75, 2.0, 1
        else:
            self.m1 = self.m2 = None
            self.s1 = self.s2 = 1.0
            self.thr = 0

    def run(self, mix, lam, plain=False):
        """(loss, logits, z, dz, dW2, db2, db1, dW1, dx) of the latent entry point (``plain``: of
        pcgmix_potes_head_loss_fwd_f32) followed by pcgmix_potes_head_loss_bwd_f32."""
        lib = _lib.load()
        B, K, C, dev = self.B, self.K, self.C, self.dev
        f32 = dict(dtype=torch.float32, device=dev)
        partial = torch.empty(lib.pcgmix_skinny_linear_splits(B, K), B, 20, **f32)
        z, logits, dz = torch.empty(B, 20, **f32), torch.empty(B, C, **f32), torch.empty(B, 20, **f32)
        loss, small = torch.empty((), **f32), torch.empty(C * 20 + C + 20, **f32)
        out = torch.empty_like(small)
        ws = torch.empty(lib.pcgmix_potes_head_loss_workspace_floats(B), **f32)
        dw1, dx = torch.empty(20, K, **f32), torch.empty(B, K, **f32)
        inv = np.empty_like(mix)
        inv[mix] = np.arange(B)
        both = torch.from_numpy(np.concatenate([mix, inv]).astype(np.int32)).to(dev)
        opt = lambda t: t.data_ptr() if t is not None else None            # noqa: E731
        head = (self.feat.data_ptr(), opt(self.m1), ctypes.c_float(self.s1), self.thr, 8,
                self.w1.data_ptr(), self.b1.data_ptr(), opt(self.m2), ctypes.c_float(self.s2), self.thr,
                self.w2.data_ptr(), self.b2.data_ptr(), self.target.data_ptr(), partial.data_ptr(),
                z.data_ptr(), logits.data_ptr(), dz.data_ptr(), loss.data_ptr(), small.data_ptr(),
                ws.data_ptr(), dw1.data_ptr())
        kind = 0 if self.soft else 1
        if plain:
            _lib.check(lib.pcgmix_potes_head_loss_fwd_f32(*head, 0, kind, B, K, C, _stream(dev)), "fwd")
        else:
            _lib.check(lib.pcgmix_potes_head_loss_latent_fwd_f32(
                *head, kind, B, K, C, both[:B].data_ptr(), both[B:].data_ptr(), ctypes.c_float(lam),
                _stream(dev)), "latent fwd")
        _lib.check(lib.pcgmix_potes_head_loss_bwd_f32(
            dz.data_ptr(), None, self.feat.data_ptr(), opt(self.m1), ctypes.c_float(self.s1), self.thr, 8,
            self.w1.data_ptr(), small.data_ptr(), out.data_ptr(), dw1.data_ptr(), dx.data_ptr(), None,
            None, B, K, C, _stream(dev)), "bwd")
        torch.cuda.synchronize()
        small = out
        return (loss, logits, z, dz, small[:C * 20].view(C, 20).clone(), small[C * 20:C * 20 + C].clone(),
                small[C * 20 + C:].clone(), dw1, dx)

    def restate(self, mix, lam):
        """The same composition in float64 torch with autograd."""
        d = lambda t: t.double().requires_grad_(True)                       # noqa: E731
        feat, w1, b1, w2, b2 = d(self.feat), d(self.w1), d(self.b1), d(self.w2), d(self.b2)
        x = feat * (self.m1.double() * self.s1) if self.m1 is not None else feat
        z = F.linear(x, w1, b1)
        z.retain_grad()
        h = z.relu() * (self.m2.double() * self.s2 if self.m2 is not None else 1.0)
        hm = lam * h + (1 - lam) * h[torch.from_numpy(mix).to(self.dev)]
        logits = F.linear(hm, w2, b2)
        tgt = self.target.double() if self.soft else F.one_hot(self.labels, self.C).double().to(self.dev)
        loss = -(F.log_softmax(logits, dim=1) * tgt).sum(dim=1).mean()
        loss.backward()
        return (loss.detach(), logits.detach(), z.detach(), z.grad, w2.grad, b2.grad, b1.grad, w1.grad,
                feat.grad)


NAMES = ("loss", "logits", "z", "dz", "dW2", "db2", "db1", "dW1", "dx")


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("K", [9968, 19968])
@pytest.mark.parametrize("B", [1, 5, 16, 256])
def test_latent_tail_kernel_matches_torch(B, K, C, drop, device):
    lam = float(np.float32(0.3716))
    for soft in (False, True):
        case = _Head(B, K, C, drop, soft, device)
        perms = _permutations(case.labels.numpy(), np.random.default_rng(B * 31 + C))
        for kind, mix in perms.items():
            got = case.run(mix, lam)
            again = case.run(mix, lam)
            want = case.restate(mix, lam)
            for name, a, b, w in zip(NAMES, got, again, want):
                assert torch.equal(a, b), (name, kind, soft, "two runs differ")
                w = w.float()
                err = float((a - w).abs().max())
                print(f"B={B} K={K} C={C} drop={drop} soft={soft} {kind:12s} {name:6s} "
                      f"max|err|={err:.3e} max|ref|={float(w.abs().max()):.3e}")
                if name in ("loss", "logits", "z"):
                    ok = torch.allclose(a, w, rtol=1e-5, atol=1e-6)
                else:
                    ok = torch.allclose(a, w, rtol=1e-4, atol=1e-7 + 1e-4 * float(w.abs().max()))
                assert ok, (name, kind, soft, err)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("B,K,C", [(1, 9968, 2), (5, 19968, 5), (16, 9968, 5), (256, 19968, 2)])
def test_latent_tail_kernel_lam_one_is_the_plain_kernel(B, K, C, drop, device):
    """lam = 1: every output of the latent entry point equals the plain one's bit for bit, whatever
    the partners — a guard on the summation order of the recomputed partner rows and on the fmaf
    chains the two kernels share."""
    for soft in (False, True):
        case = _Head(B, K, C, drop, soft, device)
        perms = _permutations(case.labels.numpy(), np.random.default_rng(B + 5))
        plain = case.run(perms["identity"], 1.0, plain=True)
        for kind, mix in perms.items():
            got = case.run(mix, 1.0)
            for name, a, b in zip(NAMES, got, plain):
                assert torch.equal(a, b), (name, kind, soft)


def test_latent_entry_point_refuses_bad_arguments(device):
    case = _Head(4, 1028, 2, False, False, device)
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=device)
    bufs = [torch.empty(max(4096, lib.pcgmix_skinny_linear_splits(4, 1028) * 80), **f32) for _ in range(8)]
    both = torch.arange(8, dtype=torch.int32, device=device) % 4
    args = lambda mix, lam: (case.feat.data_ptr(), None, ctypes.c_float(1.0), 0, 8, case.w1.data_ptr(),  # noqa: E731
                             case.b1.data_ptr(), None, ctypes.c_float(1.0), 0, case.w2.data_ptr(),
                             case.b2.data_ptr(), case.target.data_ptr(), *[b.data_ptr() for b in bufs[:7]],
                             None, 1, 4, 1028, 2, mix, both[4:].data_ptr(), ctypes.c_float(lam),
                             _stream(device))
    assert lib.pcgmix_potes_head_loss_latent_fwd_f32(*args(None, 0.5)) != 0
    assert lib.pcgmix_potes_head_loss_latent_fwd_f32(*args(both.data_ptr(), 1.5)) != 0
    assert lib.pcgmix_potes_head_loss_latent_fwd_f32(*args(both.data_ptr(), 0.5)) == 0
    torch.cuda.synchronize()


# ====================================================================================================
# augment() in 1D, the training step and the drivers
# ====================================================================================================
import argparse  # noqa: E402
import copy  # noqa: E402
import glob  # noqa: E402
import os  # noqa: E402
import sys  # noqa: E402

from conftest import GOLDEN, Args, StepCounter, learnable_dataset  # noqa: E402

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import latent_cases as LC  # noqa: E402
import train_cases as TC  # noqa: E402

from pcgmix_amd import augmentations, augmentations2d, hostprep, models, train_model as tm  # noqa: E402

FILES = sorted(glob.glob(os.path.join(GOLDEN, "latent1d_*.npz")))


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _set_np_state(g, which):
    tail = g[which + "_tail"]
    np.random.set_state(("MT19937", g[which].astype(np.uint32), int(tail[0]), int(tail[1]), float(tail[2])))


def _assert_np_state(g, which="np_after"):
    _, key, pos, has_gauss, cached = np.random.get_state()
    tail = g[which + "_tail"]
    assert np.array_equal(key, g[which]) and pos == int(tail[0])
    assert has_gauss == int(tail[1]) and (not has_gauss or cached == tail[2])


def _potes(device, state="potes_state_seed1234.npz"):
    sd = np.load(os.path.join(GOLDEN, state))
    m = models.CNN_potes_TS(4, 2, "PhysioNet")
    m.load_state_dict({k: torch.from_numpy(sd[k]) for k in sd.files})
    return m.to(device)


def _narrow_resnet(device, g=None):
    m = LC.narrow_resnet(models.ResNet9)
    if g is not None:
        m.load_state_dict({k[len("state."):]: torch.from_numpy(g[k]) for k in g if k.startswith("state.")})
    return m.to(device)


def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _inputs(device, x, labels):
    return torch.from_numpy(x).to(device), F.one_hot(torch.from_numpy(labels), 2).to(device)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
@pytest.mark.parametrize("host_labels", [False, True])
def test_augment_against_the_reference(path, host_labels, device):
    """augment() with a 1D latentmixup method == the reference's own call (tests/golden/
    make_golden_latent1d.py): features within 1e-4 * max(1, max|y_ref|) (the bound this project's
    models are held to against the reference's logits), partners, args.depth and numpy's global
    stream exact, the input object returned when the gate rejects."""
    g = _load(path)
    method, step, name = str(g["method"]), int(g["step"]), str(g["model"])
    net = (_potes(device) if name == "Potes" else _narrow_resnet(device, g)).eval()
    data, tgt = _inputs(device, g["x"], g["labels"])
    args = Args(method, model=name, depth=0)
    _set_np_state(g, "np_before")
    with torch.no_grad():
        y, t_out, mix, cut = augmentations.augment(
            args, data, tgt, torch.from_numpy(g["frames"]), tuple(str(w) for w in g["wav"]),
            StepCounter(step), net, device, "", host_labels=g["labels"] if host_labels else None)
    _assert_np_state(g)
    assert cut is None and t_out is tgt
    assert (y is data) == bool(g["same_object"]) and args.depth == int(g["depth"])
    assert np.array_equal(np.asarray(mix, np.int64).reshape(-1), g["mix"])
    if not int(g["fired"]):
        assert isinstance(mix, list) and mix == []
        return
    want = g["y"]
    assert tuple(y.shape) == want.shape and y.dtype == torch.float32
    err = float(np.abs(y.cpu().numpy() - want).max())
    bound = 1e-4 * max(1.0, float(np.abs(want).max()))
    print(f"{os.path.basename(path)} depth {args.depth} max|err| {err:.3e} bound {bound:.3e}")
    assert err <= bound


def test_augment_needs_the_model_and_a_known_model_name(device):
    x, frames, labels, wav = LC.augment_batch()
    data, tgt = _inputs(device, x, labels)
    with pytest.raises(ValueError, match="model"):
        augmentations.augment(Args("latentmixup"), data, tgt, torch.from_numpy(frames), wav, StepCounter(0),
                              None, device, "")
    with pytest.raises(NotImplementedError, match="Potes"):
        augmentations.augment(Args("latentmixup", model="FCN"), data, tgt, torch.from_numpy(frames), wav,
                              StepCounter(0), _potes(device), device, "")
    # strings that select another method (or are refused for another reason) behave as before
    y, _, mix, _ = augmentations.augment(Args("latentmixup timemask(0.2)"), data.clone(), tgt,
                                         torch.from_numpy(frames), wav, StepCounter(0), None, device, "")
    assert y.shape == data.shape and mix == []
    with pytest.raises(NotImplementedError):
        augmentations.augment(Args("latentmixup gaussiannoise"), data, tgt, torch.from_numpy(frames), wav,
                              StepCounter(0), None, device, "")
    assert augmentations2d.latent_blend is augmentations.latent_blend


@pytest.mark.parametrize("name,step", [("Potes", 3), ("resnet9", 1), ("resnet9", 0), ("resnet9", 5)])
def test_augment_in_train_mode_is_the_blend_of_the_first_half(name, step, device):
    """Train mode, dropout on (Potes: Dropout(.25) and Dropout(.5) live; ResNet9-1D: batch
    statistics): with the same torch seed, augment()'s output is lam*h + (1-lam)*h[mix] of
    h = model(x, depth, 'first') to 1e-6 * max(1, max|h|) — the blend and the layout."""
    x, frames, labels, wav = LC.augment_batch()
    data, tgt = _inputs(device, x, labels)
    net = (_potes(device) if name == "Potes" else _narrow_resnet(device)).train()
    args = Args("latentmixup", model=name, depth=0)
    plan = hostprep.latent_plan("latentmixup", name, labels, step, 8)
    torch.manual_seed(50 + step)
    with torch.no_grad():
        h = net(data, depth=plan.depth, pass_part="first")
    torch.manual_seed(50 + step)
    with torch.no_grad():
        y, _, mix, _ = augmentations.augment(args, data, tgt, torch.from_numpy(frames), wav,
                                             StepCounter(step), net, device, "", host_labels=labels)
    assert args.depth == plan.depth and np.array_equal(mix, plan.mix)
    if name == "Potes":
        assert tuple(y.shape) == (8, 20)
    lam = float(plan.lam32)
    want = h * lam + h[torch.from_numpy(plan.mix).to(device)] * (1 - lam)
    assert y.shape == want.shape
    err = float((y - want).abs().max())
    assert err <= 1e-6 * max(1.0, float(h.abs().max())), err


@pytest.mark.parametrize("name,step", [("Potes", 3), ("resnet9", 1), ("resnet9", 0), ("resnet9", 5)])
def test_gradients_through_the_drop_in_path(name, step, device):
    """first half -> HIP blend -> second half -> CELoss on the HIP path against a float64 CPU copy
    of the same model doing the same: loss 1e-4 relative, every parameter gradient
    |dg| <= 1e-2 |g| + 1e-4 (the bound of test_resnet9_channels_last_path_matches_float64)."""
    x, frames, labels, wav = LC.augment_batch()
    data, tgt = _inputs(device, x, labels)
    torch.manual_seed(21)
    net = _no_dropout(_potes(device) if name == "Potes" else _narrow_resnet(device)).train()
    ref = copy.deepcopy(net).cpu().double()
    args = Args("latentmixup", model=name, depth=0)
    y, _, mix, _ = augmentations.augment(args, data, tgt, torch.from_numpy(frames), wav, StepCounter(step),
                                         net, device, "", host_labels=labels)
    assert y.requires_grad
    loss = tm.CELoss(2)(net(y, depth=args.depth, pass_part="second"), tgt)
    loss.backward()
    plan = hostprep.latent_plan("latentmixup", name, labels, step, 8)
    lam = float(plan.lam32)
    h = ref(torch.from_numpy(x).double(), depth=plan.depth, pass_part="first")
    h = h * lam + h[torch.from_numpy(plan.mix)] * (1 - lam)
    out = ref(h, depth=plan.depth, pass_part="second")
    loss_r = -(torch.log_softmax(out, 1) * F.one_hot(torch.from_numpy(labels), 2).double()).sum(1).mean()
    loss_r.backward()
    assert abs(float(loss.detach()) - float(loss_r.detach())) <= 1e-4 * abs(float(loss_r.detach())), (loss, loss_r)
    checked = 0
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if q.grad is None:
            continue
        d = float((p.grad.cpu().double() - q.grad).norm())
        assert d <= 1e-2 * float(q.grad.norm()) + 1e-4, (k, d, float(q.grad.norm()))
        checked += 1
    assert checked >= 4


class _KeepGrads(torch.optim.SGD):
    """An optimiser that moves nothing and keeps the gradients it was handed."""

    def __init__(self, params):
        super().__init__(params, lr=0.0)
        self.seen = None

    def step(self, closure=None):
        self.seen = [p.grad.detach().clone() for g in self.param_groups for p in g["params"]
                     if p.grad is not None]


def _one_batch(B, T, seed):
    x, frames, labels, wav = synthetic_batch(B, T, seed)
    return (torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(frames), wav,
            torch.ones(B, dtype=torch.long), torch.arange(B))


def synthetic_batch(B, T, seed):
    from pcgmix_amd import synthetic
    return synthetic.make_batch(B, 4, T, sample_rate=1000 if T == 2500 else 2000, seed=seed)


@pytest.mark.parametrize("B,T,method,step", [(16, 2500, "latentmixup", 3), (256, 5000, "latentmixup", 11),
                                             (37, 2500, "latentmixup+0.5", 1)])
def test_fused_step_equals_drop_in_step(B, T, method, step, device):
    """One train_step on two copies of a Potes model (dropout 0): the fused path (blend inside the
    head's tail kernel) and the drop-in path forced by ``args.latent_fused = False`` (augment() +
    model(h, 1, 'second') + CELoss).  Loss rtol 1e-5, every gradient rtol 1e-4 / atol 1e-7 +
    1e-4 max|g| (the bounds of test_fused_head_loss_equals_head_then_celoss); the fused one launches
    the latent tail kernel and no blend kernel, the other the reverse."""
    from torch.profiler import profile, ProfilerActivity
    batch = _one_batch(B, T, 70 + B)
    res = []
    for fused in (True, False):
        args = argparse.Namespace(dataset="PhysioNet", model="Potes", method=method, num_epochs=2, batch_size=B,
                                  op="adam", use_sched=False, lr_max=0.01, weight_decay=0.0, grad_clip=0.0,
                                  seed=4, num_classes=2, num_channels=4, sig_len=T, depth=0, num_steps=8,
                                  sample_rate=1000, latent_fused=fused)
        torch.manual_seed(3)
        net = _no_dropout(tm.build_model(args)).to(device).train()
        opt = _KeepGrads([p for p in net.parameters() if p.requires_grad])
        crit = tm.SELCLoss(batch[1].numpy(), 2, es=args.num_epochs + 1, device=device)
        sc = tm.step_counter_class()
        sc.count = step
        np.random.seed(9)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            loss = tm.train_step(args, net, batch, device, opt, None, crit, 1, sc)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()]
        state = np.random.get_state()
        assert args.depth == 0 and sc.count == step + 1
        assert any("potes_tail_loss_latent_kernel" in n for n in names) == fused, names
        assert any("blend_rows" in n for n in names) == (not fused), names
        res.append((float(loss), opt.seen, state))
    assert res[0][2][1].tobytes() == res[1][2][1].tobytes() and res[0][2][2:] == res[1][2][2:]   # numpy's stream
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[1][0]) + 1e-6, (res[0][0], res[1][0])
    assert len(res[0][1]) == len(res[1][1]) >= 8
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-7 + 1e-4 * float(b.abs().max())), \
            (tuple(a.shape), float((a - b).abs().max()), float(b.abs().max()))


def test_fused_step_when_the_gate_rejects_is_the_plain_step(device):
    """latentmixup+0.5 at a step whose gate rejects: the plain fused step, args.depth and numpy's
    stream untouched."""
    B, T = 16, 2500
    batch = _one_batch(B, T, 5)
    res = []
    for method in ("latentmixup+0.5", "base"):
        args = argparse.Namespace(dataset="PhysioNet", model="Potes", method=method, num_epochs=2, batch_size=B,
                                  op="adam", use_sched=False, lr_max=0.01, weight_decay=0.0, grad_clip=0.0,
                                  seed=4, num_classes=2, num_channels=4, sig_len=T, depth=0, num_steps=8,
                                  sample_rate=1000)
        torch.manual_seed(3)
        net = _no_dropout(tm.build_model(args)).to(device).train()
        opt = _KeepGrads([p for p in net.parameters() if p.requires_grad])
        crit = tm.SELCLoss(batch[1].numpy(), 2, es=3, device=device)
        sc = tm.step_counter_class()
        sc.count = 2                                         # Random(2).uniform(0, 1) >= 0.5
        np.random.seed(9)
        before = np.random.get_state()[1].copy()
        loss = tm.train_step(args, net, batch, device, opt, None, crit, 1, sc)
        assert np.array_equal(np.random.get_state()[1], before) and args.depth == 0
        res.append((loss, opt.seen))
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


def test_fused_step_with_dropout_on_trains(device):
    """Train mode with both dropouts live on the fused path: finite loss, every trained parameter
    gets a finite gradient, the same torch seed gives the same loss."""
    B, T = 32, 2500
    batch = _one_batch(B, T, 6)
    losses = []
    for _ in range(2):
        args = argparse.Namespace(dataset="PhysioNet", model="Potes", method="latentmixup", num_epochs=2,
                                  batch_size=B, op="adam", use_sched=False, lr_max=0.01, weight_decay=0.0,
                                  grad_clip=0.0, seed=4, num_classes=2, num_channels=4, sig_len=T, depth=0,
                                  num_steps=8, sample_rate=1000)
        torch.manual_seed(3)
        net = tm.build_model(args).to(device).train()
        opt = _KeepGrads([p for p in net.parameters() if p.requires_grad])
        crit = tm.SELCLoss(batch[1].numpy(), 2, es=3, device=device)
        torch.manual_seed(17)
        losses.append(float(tm.train_step(args, net, batch, device, opt, None, crit, 1, tm.step_counter_class())))
        assert len(opt.seen) == 8 and all(bool(torch.isfinite(g).all()) for g in opt.seen)
    assert np.isfinite(losses[0]) and losses[0] == losses[1]


# ------------------------------------------------------------------ trajectories
def _traj_golden():
    return np.load(os.path.join(GOLDEN, "train_latent1d_ref.npz"))


@pytest.mark.parametrize("mode", ["step", "step_dropin", "epoch"])
def test_potes_trajectory_reproduces_the_reference(mode, device):
    """The reference's train_epoch with method 'latentmixup' (Potes seed 7, dropout 0, 10 steps)
    through eager train_step — fused and with the drop-in path forced — and through train_epoch,
    which must pick the eager step: losses 1e-4, learning rates exact, parameters 1e-3,
    args.depth == 0 after every step."""
    g = _traj_golden()
    args = LC.potes_traj_args()
    if mode == "step_dropin":
        args.latent_fused = False
    torch.manual_seed(7)
    net = _no_dropout(tm.build_model(args)).to(device).train()
    opt, sched = tm.make_optimizer(args, net)
    batches = TC.traj_batches()
    crit = tm.SELCLoss(np.concatenate([b[1].numpy() for b in batches]), 2, es=args.num_epochs + 1, device=device)
    sc = tm.step_counter_class()
    losses, lrs = [], []
    orig = tm.train_step

    def step(*a, **k):
        v = orig(*a, **k)
        losses.append(float(v))
        assert args.depth == 0
        return v
    if mode == "epoch":
        tm.train_step = step
        try:
            mean_loss, acc, lrs = tm.train_epoch(args, net, batches, device, opt, sched, crit, 1, sc)
        finally:
            tm.train_step = orig
        assert "_pcgmix_epoch_step" not in net.__dict__               # never captured
        assert abs(mean_loss - float(g["potes_mean_loss"])) <= 1e-4
        assert abs(100.0 * acc - float(g["potes_acc"])) <= 1e-9
    else:
        for b in batches:
            lrs.append(opt.param_groups[0]["lr"])
            step(args, net, b, device, opt, sched, crit, 1, sc)
    assert sc.count == TC.TRAJ_STEPS and len(losses) == TC.TRAJ_STEPS
    assert np.allclose(lrs, g["potes_lrs"], rtol=1e-12, atol=1e-15)
    err = float(np.abs(np.asarray(losses) - g["potes_losses"]).max())
    state = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    worst = max(float(np.abs(state[k[len("potes_final."):]] - g[k]).max())
                for k in g.files if k.startswith("potes_final."))
    print(f"[latent potes traj {mode}] max loss err {err:.2e}, max param err {worst:.2e}")
    assert err <= 1e-4, (losses, g["potes_losses"])
    assert worst <= 1e-3


def _digest_check(name, got, want, atol, frac_loose=0.0, loose=0.0):
    d = np.abs(TC.tensor_digest(got)[2:] - want[2:])
    n_bad = int((d > atol).sum())
    assert n_bad <= max(1.0 if frac_loose else 0.0, frac_loose * d.size) and (d.max() <= loose if n_bad else True), \
        (name, float(d.max()), n_bad, d.size)
    return float(d.max())


def test_resnet9_trajectory_reproduces_the_reference(device):
    """ResNet9-1D full width, the reference's train_epoch with 'latentmixup' from step count 8
    (depths 1, 2, 3), through eager train_step at the bounds of
    test_train_r3_gpu.test_resnet9_train_mode_reproduces_reference: losses 1e-4 relative, BN
    buffers 1e-4, parameters on the recorded digest (98 % within 2e-6, the rest within 5e-5;
    convolution biases in front of a BatchNorm within 4.6e-5 — see that test for the reasons)."""
    g = _traj_golden()
    args, batches = LC.resnet_traj_args(), LC.resnet_traj_batches()
    torch.manual_seed(7)
    net = tm.build_model(args)
    for k, v in net.state_dict().items():
        if f"r1d_ini.{k}" in g.files:
            assert np.allclose(TC.tensor_digest(v.numpy())[:2], g[f"r1d_ini.{k}"], rtol=1e-6), k
    net = net.to(device).train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(np.concatenate([b[1].numpy() for b in batches]), 2, es=args.num_epochs + 1, device=device)
    sc = tm.step_counter_class()
    sc.count = LC.RESNET_FIRST_COUNT
    losses, lrs, depths = [], [], []
    for b in batches:
        lrs.append(opt.param_groups[0]["lr"])
        depths.append(hostprep.latent_depth("resnet9", sc.count))
        losses.append(float(tm.train_step(args, net, (b[0].to(device),) + tuple(b[1:]), device, opt, sched,
                                          crit, 1, sc)))
        assert args.depth == 0
    assert depths == list(g["r1d_depths"]) == [1, 2, 3]
    assert np.allclose(lrs, g["r1d_lrs"], rtol=1e-12)
    rel = np.abs(np.asarray(losses) - g["r1d_losses"]) / np.abs(g["r1d_losses"])
    print(f"[latent r1d traj] losses {losses} rel err {rel}")
    assert rel.max() <= 1e-4, (losses, g["r1d_losses"])
    state = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    worst_b = worst_p = 0.0
    for k in g.files:
        if k.startswith("r1d_buf."):
            name = k[len("r1d_buf."):]
            if "num_batches" in name:
                assert int(state[name]) == int(g[k]), name
                continue
            d = float(np.abs(state[name] - g[k]).max() / max(1.0, float(np.abs(g[k]).max())))
            worst_b = max(worst_b, d)
            assert d <= 1e-4, (name, d)
        elif k.startswith("r1d_par."):
            name = k[len("r1d_par."):]
            if name.endswith(".0.bias"):
                _digest_check(name, state[name], g[k], 4.6e-5)
                continue
            worst_p = max(worst_p, _digest_check(name, state[name], g[k], 2e-6, 0.02, 5e-5))
    print(f"[latent r1d traj] buffers {worst_b:.2e}, params {worst_p:.2e}")


# ------------------------------------------------------------------ drivers
def _driver_args(out_dir, model):
    return argparse.Namespace(dataset="PhysioNet", model=model, method="latentmixup+0.8", num_epochs=2,
                              batch_size=32, op="adam", use_sched=True, lr_max=0.003, weight_decay=1e-4,
                              grad_clip=0.1, seed=4, seed_data=1100001, n_fraction=1.0, train_balance=True,
                              num_classes=2, sample_rate=1000, num_channels=4, valid=False, depth=0,
                              EXPERIMENTS=out_dir)


@pytest.mark.parametrize("model", ["Potes", "resnet9"])
def test_latentmixup_through_train_model(model, device, tmp_path, monkeypatch):
    """train_model -> train_step with 1D latentmixup+0.8 on a small synthetic dataset: finite
    losses, the expected step count, and the captured step is never built."""
    built = []
    orig_init = tm.GraphedTrainStep.__init__
    monkeypatch.setattr(tm.GraphedTrainStep, "__init__",
                        lambda self, *a, **k: (built.append(1), orig_init(self, *a, **k))[1])
    args = _driver_args(str(tmp_path), model)
    perf = tm.train_model(args, learnable_dataset(n_rec=24), device, log=None)
    assert perf["steps"][-1] == args.num_steps == 2 * (96 // 32)
    assert all(np.isfinite(v) for v in perf["train_loss"]) and len(perf["train_loss"]) >= 1
    assert args.depth == 0 and not built


def test_graphed_step_refuses_latentmixup(device):
    args = _driver_args("", "Potes")
    args.num_steps, args.sig_len = 8, 2500
    net = tm.build_model(args).to(device)
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(np.zeros(32, int), 2, es=3, device=device)
    with pytest.raises(NotImplementedError, match="captured step"):
        tm.GraphedTrainStep(args, net, opt, sched, crit, device, 32, 4, 2500)
    batch = _one_batch(32, 2500, 1)
    assert tm._epoch_graphed_step(args, net, opt, sched, crit, device, 1, batch) is None
    args.method = "durratiomixup"
    assert tm._epoch_graphed_step(args, net, opt, sched, crit, device, 1, batch) is not None


def _ddp_rank(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tm.train_model(_driver_args(out_dir, "Potes"), learnable_dataset(n_rec=24), dev, log=None)
        verdict = "ran"
    except NotImplementedError as exc:
        verdict = "refused: " + str(exc)
    with open(os.path.join(out_dir, f"rank{rank}.txt"), "w") as f:
        f.write(verdict)
    dist.barrier()
    dist.destroy_process_group()


def test_latentmixup_is_refused_under_torch_distributed(tmp_path):
    """Two gloo ranks sharing this GPU: train_model() refuses 1D latentmixup at its start with the
    message of the 2D case."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_ddp_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        verdict = (tmp_path / f"rank{r}.txt").read_text()
        assert verdict == "refused: " + tm.LATENT_DDP_MESSAGE
        assert "latentmixup" in verdict and "distributed" in verdict


def test_fused_latent_step_launches_the_kernels_of_a_plain_step(device):
    """One fused latentmixup Potes step at (256, 4, 5000) launches exactly the kernels of a plain
    fused step with the latent tail kernel in place of potes_tail_loss_kernel — no torch
    elementwise, GEMM or reduction kernel between conv stack and update — plus the one upload of
    the partners."""
    from torch.autograd import DeviceType
    from torch.profiler import profile, ProfilerActivity
    B, T = 256, 5000
    batch = _one_batch(B, T, 8)
    batch = (batch[0].to(device),) + batch[1:]
    seen = {}
    for method in ("base", "latentmixup"):
        args = argparse.Namespace(dataset="PhysioNet", model="Potes", method=method, num_epochs=2, batch_size=B,
                                  op="adam", use_sched=True, lr_max=0.01, weight_decay=1e-4, grad_clip=0.1,
                                  seed=4, num_classes=2, num_channels=4, sig_len=T, depth=0, num_steps=8,
                                  sample_rate=2000)
        torch.manual_seed(3)
        net = tm.build_model(args).to(device).train()
        opt, sched = tm.make_optimizer(args, net)
        crit = tm.SELCLoss(batch[1].numpy(), 2, es=3, device=device)
        sc = tm.step_counter_class()
        for _ in range(2):                                    # warm-up: allocations, first-use setup
            tm.train_step(args, net, batch, device, opt, sched, crit, 1, sc)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            tm.train_step(args, net, batch, device, opt, sched, crit, 1, sc)
            torch.cuda.synchronize()
        ev = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]     # device side only
        # (kernel names without their argument lists)
        seen[method] = (sorted(n.split("(")[0] for n in ev if "memcpy" not in n.lower() and "memset" not in n.lower()),
                        sum("memcpy" in n.lower() for n in ev))
    plain, latent = seen["base"], seen["latentmixup"]
    swapped = sorted(n.replace("potes_tail_loss_kernel", "potes_tail_loss_latent_kernel") for n in plain[0])
    assert any("potes_tail_loss_latent_kernel" in n for n in latent[0])
    assert latent[0] == swapped, (latent[0], plain[0])
    assert latent[1] == plain[1] + 1, (latent[1], plain[1])
    assert len(latent[0]) >= 5, latent[0]
