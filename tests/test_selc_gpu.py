"""SELC phase on the GPU: the generic loss kernels against a float64 evaluation of the reference
formula (train_model.py:56-80), the fused Potes head + SELC node against the unfused chain, the
reference-recorded trajectory (tests/golden/train_selc_ref.npz) through the eager step, the captured
step and the eager epoch, and the captured step's phase handling."""
import argparse
import copy
import os
import sys

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import models, saliency, synthetic, train_model as tm
from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import selc_cases as SC  # noqa: E402
import train_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

M = 0.9


def golden():
    return np.load(os.path.join(GOLDEN, "train_selc_ref.npz"))


# ---- generic kernels -------------------------------------------------------------------------------
def _selc_f64(logits32, soft64, index):
    """One step of the reference formula in float64 on float32 logits: (updated rows, loss, B * dlogits)."""
    z = logits32.astype(np.float64)
    z = z - z.max(1, keepdims=True)
    pred = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    rows = M * soft64[index] + (1 - M) * pred
    loss = float((-(np.log(pred) * rows).sum(1)).mean())
    return rows, loss, pred * rows.sum(1, keepdims=True) - rows


def _kernel_steps(device, logits, index, soft0):
    """Two consecutive SELCFunction steps on the same indices: per step (loss, B * dlogits), final soft."""
    soft = torch.from_numpy(soft0).to(device)
    idx = torch.from_numpy(index).to(device)
    out = []
    for lg in logits:
        x = torch.from_numpy(lg).to(device).requires_grad_(True)
        loss = tm.SELCFunction.apply(x, idx, soft, M)
        loss.backward()
        out.append((loss.detach().cpu().numpy().copy(), (x.grad * x.shape[0]).cpu().numpy()))
    return out, soft.cpu().numpy()


@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("B", [1, 5, 256, 257])
def test_selc_kernels_match_float64_reference(B, C, device):
    """pcgmix_selc_{fwd,bwd}_f32, two steps on the same injective indices into N = B + 7 rows, logits
    N(0,3) (no underflow): updated rows, loss and B * dlogits within 1e-5 (same-input
    model values) of the float64 formula; untouched rows keep their bits; a second run gives the same
    bits."""
    rs = np.random.RandomState(1000 * B + C)
    N = B + 7
    index = rs.permutation(N)[:B].astype(np.int64)
    soft0 = rs.dirichlet(np.ones(C), N).astype(np.float32)
    logits = [(rs.standard_normal((B, C)) * 3).astype(np.float32) for _ in range(2)]
    got, soft = _kernel_steps(device, logits, index, soft0)
    again, soft_again = _kernel_steps(device, logits, index, soft0)
    want = soft0.astype(np.float64)
    for (loss, grad), lg in zip(got, logits):
        rows, wloss, wgrad = _selc_f64(lg, want, index)
        want[index] = rows
        print(f"[selc B={B} C={C}] loss err {abs(float(loss) - wloss):.2e} grad err {np.abs(grad - wgrad).max():.2e}")
        assert abs(float(loss) - wloss) <= 1e-5
        assert np.abs(grad - wgrad).max() <= 1e-5
    print(f"[selc B={B} C={C}] rows err {np.abs(soft[index] - want[index]).max():.2e}")
    assert np.abs(soft[index] - want[index]).max() <= 1e-5
    untouched = np.setdiff1d(np.arange(N), index)
    assert len(untouched) == 7 and np.array_equal(soft[untouched].view(np.uint32), soft0[untouched].view(np.uint32))
    assert np.array_equal(soft.view(np.uint32), soft_again.view(np.uint32))
    for (l0, g0), (l1, g1) in zip(got, again):
        assert l0.tobytes() == l1.tobytes() and g0.tobytes() == g1.tobytes()


def test_selc_row_with_index_out_of_range_is_left_out(device):
    """One index equal to N: nothing is written for it, its row gives zero loss and zero gradient, the
    other rows are as without it (the mean still divides by B)."""
    rs = np.random.RandomState(5)
    B, C, N = 6, 3, 9
    index = np.array([4, 0, N, 7, 2, 8], dtype=np.int64)
    soft0 = rs.dirichlet(np.ones(C), N).astype(np.float32)
    lg = (rs.standard_normal((B, C)) * 3).astype(np.float32)
    # N + 1 rows on the device, the kernel is told N: the guard row behind the table must keep its bits
    guard = np.concatenate([soft0, np.full((1, C), 7.0, np.float32)])
    soft = torch.from_numpy(guard).to(device)
    x = torch.from_numpy(lg).to(device).requires_grad_(True)
    loss = tm.SELCFunction.apply(x, torch.from_numpy(index).to(device), soft[:N], M)
    loss.backward()
    torch.cuda.synchronize()
    ok = index < N
    rows, _, wgrad = _selc_f64(lg[ok], soft0.astype(np.float64), index[ok])
    z = lg[ok].astype(np.float64)
    z = z - z.max(1, keepdims=True)
    wloss = float(-((z - np.log(np.exp(z).sum(1, keepdims=True))) * rows).sum() / B)
    assert abs(float(loss.detach()) - wloss) <= 1e-5
    g = (x.grad * B).cpu().numpy()
    assert np.array_equal(g[2], np.zeros(C, np.float32))
    assert np.abs(g[ok] - wgrad).max() <= 1e-5
    got = soft.cpu().numpy()
    assert np.array_equal(got[N], guard[N])
    untouched = np.setdiff1d(np.arange(N), index[ok])
    assert np.array_equal(got[untouched], soft0[untouched])
    assert np.abs(got[index[ok]] - rows).max() <= 1e-5


# ---- fused head ------------------------------------------------------------------------------------
def _potes(device, dropout, seed=5):
    torch.manual_seed(seed)
    m = models.CNN_potes_TS(4, 2, "PhysioNet").to(device).train()
    if not dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    return m


@pytest.mark.parametrize("B", [3, 4, 33])
def test_fused_selc_head_equals_unfused_chain(B, device):
    """``loss_and_logits(..., selc=...)`` == the model's logits through ``SELCLoss`` with
    ``use_kernel = False`` (torch ops), dropout off, C = 2, a partial last block of four rows for
    B = 3 and 33: loss, logits, all eight parameter gradients and the soft rows, to the tolerances
    tests/test_head_gpu.py holds the CE form to."""
    m = _potes(device, dropout=False)
    rs = np.random.RandomState(B)
    N = B + 5
    x = torch.randn(B, 4, 2500, device=device)
    labels = rs.randint(0, 2, N)
    index = torch.from_numpy(rs.permutation(N)[:B].astype(np.int64))
    res = []
    for fused in (True, False):
        crit = tm.SELCLoss(labels, 2, es=0, device=device)
        crit.soft_labels.mul_(0.8).add_(0.1)                    # rows that are not one-hot
        m.zero_grad(set_to_none=True)
        if fused:
            assert tm.selc_fused_model(m, crit, x, torch.zeros(B, 2, device=device), 1) is m
            loss, logits = m.loss_and_logits(x, torch.zeros(B, 2, device=device),
                                             selc=(index.to(device), crit.soft_labels, crit.momentum))
        else:
            logits = m(x, depth=0, pass_part="second")
            tm.SELCLoss.use_kernel = False
            try:
                loss = crit(logits, None, index, 1, "train")
            finally:
                tm.SELCLoss.use_kernel = True
        loss.backward()
        res.append((loss.detach(), logits.detach(), crit.soft_labels.clone(),
                    {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert torch.allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6), (res[0][0], res[1][0])
    assert torch.allclose(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)
    assert torch.allclose(res[0][2], res[1][2], rtol=1e-5, atol=1e-6)
    assert not torch.equal(res[0][2][index.to(device)], (torch.nn.functional.one_hot(
        torch.from_numpy(labels), 2).float() * 0.8 + 0.1)[index].to(device))
    assert res[0][3].keys() == res[1][3].keys() and len(res[0][3]) == 8
    for k in res[0][3]:
        a, b = res[0][3][k], res[1][3][k]
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-7 + 1e-4 * float(b.abs().max())), k


def test_fused_selc_head_with_dropout_is_seeded(device):
    """Dropout on: the same torch seed gives the same loss twice, every gradient is finite."""
    m = _potes(device, dropout=True)
    B = 9
    x = torch.randn(B, 4, 2500, device=device)
    index = torch.arange(B, device=device)
    losses = []
    for _ in range(2):
        crit = tm.SELCLoss(np.arange(B) % 2, 2, es=0, device=device)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(77)
        loss, _ = m.loss_and_logits(x, torch.zeros(B, 2, device=device),
                                    selc=(index, crit.soft_labels, crit.momentum))
        loss.backward()
        losses.append(float(loss))
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    assert losses[0] == losses[1] and np.isfinite(losses[0])


# ---- reference trajectory --------------------------------------------------------------------------
def _traj_setup(device):
    args, batches = SC.selc_args(), SC.selc_batches()
    torch.manual_seed(7)
    net = tm.build_model(args)
    for mod in net.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    net = net.to(device).train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(SC.selc_labels(batches), 2, es=SC.SELC_ES, device=device)
    return args, batches, net, opt, sched, crit, tm.step_counter_class()


def _check_traj(g, lrs, net, crit, losses=None, means=None):
    assert np.allclose(lrs, g["selc_lrs"], rtol=1e-12, atol=1e-15)
    if losses is not None:
        err = np.abs(np.asarray(losses) - g["selc_losses"]).max()
        print(f"[selc traj] max loss err {err:.2e}")
        assert err <= 1e-4, (losses, g["selc_losses"])
    if means is not None:
        err = np.abs(np.asarray(means) - g["selc_epoch_mean_loss"]).max()
        print(f"[selc traj] max epoch mean err {err:.2e}")
        assert err <= 1e-4, (means, g["selc_epoch_mean_loss"])
    state = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    worst = max(float(np.abs(state[k[len("selc_final."):]] - g[k]).max())
                for k in g.files if k.startswith("selc_final."))
    soft_err = float(np.abs(crit.soft_labels.cpu().numpy() - g["selc_soft"]).max())
    print(f"[selc traj] max param err {worst:.2e}, soft err {soft_err:.2e}")
    assert worst <= 1e-3
    assert soft_err <= 1e-4


def test_selc_trajectory_eager_train_step(device):
    """The reference's 12 recorded steps (epoch 1 plain CE, epochs 2..4 SELC) through ``train_step``:
    losses 1e-4, learning rates exact, parameters 1e-3, final soft labels 1e-4."""
    args, batches, net, opt, sched, crit, sc = _traj_setup(device)
    losses, lrs = [], []
    for epoch in range(1, SC.SELC_EPOCHS + 1):
        for b in batches:
            lrs.append(opt.param_groups[0]["lr"])
            losses.append(float(tm.train_step(args, net, b, device, opt, sched, crit, epoch, sc)))
    assert sc.count == SC.SELC_STEPS
    _check_traj(golden(), lrs, net, crit, losses=losses)


def test_selc_trajectory_train_epoch_captured(device):
    """The same through ``train_epoch`` as it runs by default on a GPU: a captured plain-CE step for
    epoch 1, dropped at the turning point for a captured SELC-phase step.  ``train_epoch`` returns
    the epoch mean only: the four means are held to the loss bound."""
    args, batches, net, opt, sched, crit, sc = _traj_setup(device)
    lrs, means, keys, steps = [], [], [], []
    for epoch in range(1, SC.SELC_EPOCHS + 1):
        mean, _acc, lr = tm.train_epoch(args, net, batches, device, opt, sched, crit, epoch, sc)
        means.append(mean)
        lrs += lr
        hit = net.__dict__["_pcgmix_epoch_step"]
        assert isinstance(hit.step, tm.GraphedTrainStep) and hit.step.selc == (epoch > SC.SELC_ES)
        keys.append(hit.key)
        steps.append(hit.step)
        got = tm._epoch_graphed_step(args, net, opt, sched, crit, device, epoch, batches[0])
        assert got is not None and got is hit.step              # also past the turning point
    assert sc.count == SC.SELC_STEPS
    assert keys[0] != keys[1] and keys[1] == keys[2] == keys[3]  # one re-capture, at the turning point
    assert steps[1] is steps[2] is steps[3] and steps[0] is not steps[1]
    with pytest.raises(NotImplementedError, match="phase"):
        steps[0].prepare(batches[0], 2, sc)                     # the CE-phase step refuses a SELC epoch
    with pytest.raises(NotImplementedError, match="phase"):
        steps[1].prepare(batches[0], 1, sc)
    _check_traj(golden(), lrs, net, crit, means=means)


def test_selc_trajectory_train_epoch_eager(device):
    """The same through ``train_epoch`` with ``args.hipgraph = False`` (``train_step`` per batch)."""
    args, batches, net, opt, sched, crit, sc = _traj_setup(device)
    args.hipgraph = False
    losses, lrs, means = [], [], []
    orig = tm.train_step

    def recording_step(*a, **k):
        v = orig(*a, **k)
        losses.append(v)
        return v
    tm.train_step = recording_step
    try:
        for epoch in range(1, SC.SELC_EPOCHS + 1):
            mean, _acc, lr = tm.train_epoch(args, net, batches, device, opt, sched, crit, epoch, sc)
            means.append(mean)
            lrs += lr
    finally:
        tm.train_step = orig
    assert "_pcgmix_epoch_step" not in net.__dict__
    _check_traj(golden(), lrs, net, crit, losses=[float(v) for v in losses], means=means)


# ---- other models, pipelined slots, warm-up, the CE-only step --------------------------------------
def _batches(B, n, seed, T=2500):
    out = []
    for i in range(n):
        x, frames, labels, wav = synthetic.make_batch(B, 4, T, sample_rate=1000, seed=seed + i)
        out.append((torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(frames), wav,
                    torch.ones(B, dtype=torch.long), torch.arange(B) + B * i))
    return out


def _close(a, b):
    """Captured against eager, as tests/test_train_r3_gpu.py compares them."""
    assert np.allclose(a["losses"], b["losses"], rtol=1e-4, atol=1e-5), (a["losses"], b["losses"])
    for k, v in a["state"].items():
        assert np.allclose(v, b["state"][k], rtol=1e-3, atol=1e-4), k
    assert np.allclose(a["soft"], b["soft"], rtol=1e-4, atol=1e-5)


def test_selc_base_resnet9_captured_equals_eager(device):
    """``SELC_base`` on resnet9-5k at (8,4,2500), two SELC epochs of two batches: the captured step
    (``SELCFunction`` behind the model) == the eager ``train_step``.  Learning rates as the ResNet9
    goldens' (train_cases.RESNET_LR_MAX: the net is chaotic at 0.01)."""
    B = 8
    batches = _batches(B, 2, 810)
    res = {}
    for mode in ("step", "graph"):
        args = SC.selc_args()
        args.__dict__.update(model="resnet9-5k", method="SELC_base", batch_size=B, num_epochs=2,
                             num_steps=TC.SCHED_STEPS, lr_max=TC.RESNET_LR_MAX)
        assert tm.selc_turning_point(args) == 0
        torch.manual_seed(11)
        net = tm.build_model(args).to(device).train()
        opt, sched = tm.make_optimizer(args, net)
        crit = tm.SELCLoss(np.concatenate([b[1].numpy() for b in batches]), 2, es=0, device=device)
        sc = tm.step_counter_class()
        if mode == "graph":
            g = tm.GraphedTrainStep(args, net, opt, sched, crit, device, B, 4, 2500, selc=True)
            assert tm.fused_loss_model(net, crit.CEloss, g.x, g.t, None) is None
        losses = []
        for epoch in (1, 2):
            for b in batches:
                losses.append(float(g.step(b, epoch, sc) if mode == "graph" else
                                    tm.train_step(args, net, b, device, opt, sched, crit, epoch, sc)))
        res[mode] = dict(losses=np.asarray(losses), soft=crit.soft_labels.cpu().numpy(),
                         state={k: v.detach().cpu().numpy() for k, v in net.state_dict().items()})
    _close(res["step"], res["graph"])
    assert np.isfinite(res["graph"]["losses"]).all()
    assert not np.array_equal(res["graph"]["soft"], np.round(res["graph"]["soft"]))


def _write_base_checkpoint(args):
    """The 'base' run's model.pth where saliency.py:26-51 looks for it (reference key layout)."""
    sd = np.load(os.path.join(GOLDEN, "potes_state_seed1234.npz"))
    base = copy.copy(args)
    base.method = "base"
    exp = saliency.experiment_dir(base)
    os.makedirs(exp, exist_ok=True)
    torch.save({"module." + k: torch.from_numpy(sd[k]) for k in sd.files}, os.path.join(exp, "model.pth"))


def test_selc_saloptenv_pipelined_equals_one_slot(device, tmp_path):
    """A saliency-guided SELC name, two SELC-phase steps: ``PipelinedTrainStep`` (``selc=True``
    reaches both slots) gives finite losses and what the one-slot ``GraphedTrainStep`` gives."""
    B = 8
    batches = _batches(B, 2, 830)
    res = {}
    for mode, cls in (("one", tm.GraphedTrainStep), ("pipe", tm.PipelinedTrainStep)):
        args = TC.salopt_traj_args(str(tmp_path / mode))
        args.__dict__.update(method="(saloptenv)SELCdurratiomixup", batch_size=B, num_epochs=2)
        assert tm.selc_turning_point(args) == 0
        assert tm.captured_step_class(args) is tm.PipelinedTrainStep
        _write_base_checkpoint(args)
        torch.manual_seed(7)
        net = tm.build_model(args)
        for mod in net.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        net = net.to(device).train()
        opt, sched = tm.make_optimizer(args, net)
        crit = tm.SELCLoss(np.concatenate([b[1].numpy() for b in batches]), 2, es=0, device=device)
        sc = tm.step_counter_class()
        step = cls(args, net, opt, sched, crit, device, B, 4, 2500, selc=True)
        if mode == "pipe":
            assert all(s.selc for s in step.slots)
        losses = [float(step.step(batches[0], 1, sc, None, next_batch=batches[1])),
                  float(step.step(batches[1], 1, sc, None, next_batch=None))]
        torch.cuda.synchronize()
        res[mode] = dict(losses=np.asarray(losses), soft=crit.soft_labels.cpu().numpy(),
                         state={k: v.detach().cpu().numpy() for k, v in net.state_dict().items()})
    assert np.isfinite(res["pipe"]["losses"]).all()
    _close(res["one"], res["pipe"])


def test_building_a_selc_step_leaves_the_soft_labels_alone(device):
    """The warm-up's three passes run the SELC kernels on placeholder indices: the soft labels (and
    the model's buffers, as always) are put back bit for bit."""
    args, batches, net, opt, sched, crit, _sc = _traj_setup(device)
    crit.soft_labels.mul_(0.7).add_(0.15)
    before = crit.soft_labels.clone()
    step = tm.GraphedTrainStep(args, net, opt, sched, crit, device, SC.SELC_B, 4, 2500, selc=True)
    torch.cuda.synchronize()
    assert step.selc and step.index.dtype == torch.int64 and step.index.shape == (SC.SELC_B,)
    assert torch.equal(crit.soft_labels, before)
    with pytest.raises(IndexError):                             # the host check, before any launch
        step.prepare(batches[0][:5] + (torch.arange(SC.SELC_B) + 40,), 2, _sc)
    assert torch.equal(crit.soft_labels, before)


def test_ce_only_step_is_as_before(device):
    """A criterion that never reaches its SELC phase: the static block has the documented size, the
    hard targets travel as label bytes, there is no index buffer."""
    args, batches, net, opt, sched, _crit, _sc = _traj_setup(device)
    crit = tm.SELCLoss(SC.selc_labels(batches), 2, es=args.num_epochs + 1, device=device)
    B, C = SC.SELC_B, 2
    step = tm.GraphedTrainStep(args, net, opt, sched, crit, device, B, 4, 2500)
    assert not step.selc and step.index is None
    assert step.labels_mode is True
    assert step.block.dev.numel() == 12 + (B + 15) // 16 * 4 + (B * C + 3) // 4 * 4
    assert step._pay_bytes == (12 + (B + 15) // 16 * 4) * 4
    with pytest.raises(ValueError, match="soft_labels"):
        tm.GraphedTrainStep(args, net, opt, sched, tm.CELoss(2), device, B, 4, 2500, selc=True)


def _driver_args(**kw):
    """'Potes(noDropout)' drops the conv branch's dropout only: the head's Dropout(.5) stays on, so the
    run also checks that both drivers draw the same masks across the re-capture."""
    a = argparse.Namespace(dataset="PhysioNet", model="Potes(noDropout)", method="SELCdurratiomixup",
                           num_epochs=5, batch_size=32, op="adam", use_sched=True, lr_max=0.003,
                           weight_decay=1e-4, grad_clip=0.1, seed=4, seed_data=1100001, n_fraction=1.0,
                           train_balance=True, num_classes=2, sample_rate=1000, num_channels=4,
                           valid=False, depth=0)
    a.__dict__.update(kw)
    return a


def test_train_model_driver_captures_both_phases(device, tmp_path):
    """``train_model()`` in one process for a SELC run (5 epochs, turning point 2): graphable regardless
    of ``es`` — a captured plain-CE step, then at the first epoch past ``es`` a captured SELC-phase one
    — and the run ends where the eager driver ends, within the captured-against-eager tolerance."""
    from conftest import learnable_dataset
    ds = learnable_dataset(n_rec=24)
    built, res = [], {}
    orig = tm.GraphedTrainStep.__init__

    def recording_init(self, *a, **k):
        built.append(bool(k.get("selc", False)))
        orig(self, *a, **k)
    for use_graph in (True, False):
        args = _driver_args(EXPERIMENTS=str(tmp_path / str(use_graph)))
        assert tm.selc_turning_point(args) == 2
        tm.GraphedTrainStep.__init__ = recording_init
        try:
            perf = tm.train_model(args, ds, device, use_graph=use_graph, log=None)
        finally:
            tm.GraphedTrainStep.__init__ = orig
        res[use_graph] = (perf["train_loss"], {k: v.detach().cpu().numpy()
                                               for k, v in perf["model"].state_dict().items()})
    assert built == [False, True]                               # one capture per phase, none when eager
    assert np.isfinite(res[True][0]).all()
    assert np.allclose(res[True][0], res[False][0], rtol=1e-4, atol=1e-5), (res[True][0], res[False][0])
    for k, v in res[True][1].items():
        assert np.allclose(v, res[False][1][k], rtol=1e-3, atol=1e-4), k

