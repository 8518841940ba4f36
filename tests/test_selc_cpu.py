"""SELC phase, host side: the reference-recorded golden (tests/golden/train_selc_ref.npz <- the
reference's own SELCLoss and train_epoch), the torch formulation ``SELCLoss.use_kernel = False``
keeps, the keep/take rule, the host index check and the phase logic that needs no device."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import selc_cases as SC  # noqa: E402

import pcgmix_amd  # noqa: E402,F401
from pcgmix_amd import models, train_model as tm  # noqa: E402

CPU = torch.device("cpu")


def golden():
    return np.load(os.path.join(GOLDEN, "train_selc_ref.npz"))


def test_golden_loads():
    g = golden()
    assert g["selc_losses"].shape == (SC.SELC_STEPS,) and g["selc_lrs"].shape == (SC.SELC_STEPS,)
    assert g["selc_soft"].shape == (SC.SELC_B * SC.SELC_BATCHES, 2) and g["selc_soft"].dtype == np.float32
    assert np.isfinite(g["selc_losses"]).all()
    # every soft row has left its one-hot start, and stayed a distribution
    assert (np.abs(g["selc_soft"] - np.round(g["selc_soft"])) > 0).all()
    assert np.allclose(g["selc_soft"].sum(1), 1.0, atol=1e-6)
    assert any(k.startswith("selc_final.") for k in g.files)
    assert tm.selc_turning_point(SC.selc_args()) == SC.SELC_ES


def test_selcloss_on_cpu_reproduces_reference_trajectory():
    """The torch formulation, on the host logic of the step (loss, clip, Adam, OneCycleLR), over the 12
    recorded steps: losses 1e-4, learning rates exact, parameters 1e-3, soft labels 1e-4.  The product
    has no CPU augmentation: the batches are augmented by the oracle, as test_train_cpu does."""
    from oracle import pcgmix_oracle as O
    g = golden()
    args, batches = SC.selc_args(), SC.selc_batches()
    method, args.method = args.method, "base"
    torch.manual_seed(7)
    net = tm.build_model(args)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net.train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(SC.selc_labels(batches), 2, es=SC.SELC_ES)
    sc = tm.step_counter_class()
    losses, lrs = [], []
    for epoch in range(1, SC.SELC_EPOCHS + 1):
        for b in batches:
            y = O.augment(method, b[0].numpy(), b[1].numpy(), b[2].numpy(), b[3], sc.count)["y"]
            lrs.append(opt.param_groups[0]["lr"])
            losses.append(float(tm.train_step(args, net, (torch.from_numpy(y),) + b[1:], CPU, opt, sched,
                                              crit, epoch, sc)))
    assert np.allclose(lrs, g["selc_lrs"], rtol=1e-12, atol=1e-15)
    assert np.abs(np.asarray(losses) - g["selc_losses"]).max() <= 1e-4
    assert np.abs(crit.soft_labels.numpy() - g["selc_soft"]).max() <= 1e-4
    state = net.state_dict()
    for k in g.files:
        if k.startswith("selc_final."):
            assert float(np.abs(state[k[len("selc_final."):]].numpy() - g[k]).max()) <= 1e-3, k


def test_take_is_cast_from_the_double_difference():
    keep, take = tm.selc_keep_take(0.9)
    assert keep.dtype == np.float32 and take.dtype == np.float32
    assert keep == np.float32(0.9)
    assert take == np.float32(1.0 - 0.9)
    assert take != np.float32(1) - np.float32(0.9)
    assert take.view(np.uint32) == 0x3DCCCCCD
    assert (np.float32(1) - np.float32(0.9)).view(np.uint32) == 0x3DCCCCD0
    # what torch itself does with the Python scalar
    assert float(torch.ones(1) * (1 - 0.9)) == float(take)


def test_host_index_check_raises():
    crit = tm.SELCLoss(np.zeros(10, dtype=np.int64), 2, es=0)
    logits = torch.zeros(3, 2)
    before = crit.soft_labels.clone()
    for bad in (torch.tensor([0, 1, 10]), torch.tensor([-1, 1, 2]), np.array([0, 11, 2]), [3, 4, 10]):
        with pytest.raises(IndexError):
            crit(logits, None, bad, 1, "train")
    assert torch.equal(crit.soft_labels, before)
    assert np.isfinite(float(crit(logits, None, torch.tensor([0, 1, 9]), 1, "train")))
    # not looked at before the turning point or in test mode (the reference never reads it there)
    ohe = torch.nn.functional.one_hot(torch.tensor([0, 1, 0]), 2)
    crit.es = 5
    assert np.isfinite(float(crit(logits, ohe, torch.tensor([0, 1, 99]), 1, "train")))
    assert np.isfinite(float(crit(logits, ohe, torch.tensor([0, 1, 99]), 9, "test")))


def test_kernel_switch_exists_and_cpu_takes_torch_ops():
    assert tm.SELCLoss.use_kernel is True
    crit = tm.SELCLoss(np.array([0, 1, 1, 0]), 2, es=0, momentum=0.9)
    logits = torch.tensor([[0.3, -1.2], [2.0, 0.5]], requires_grad=True)
    loss = crit(logits, None, torch.tensor([2, 0]), 1, "train")
    pred = torch.softmax(logits.detach().double(), 1)
    soft = torch.tensor([[0.0, 1.0], [1.0, 0.0]], dtype=torch.float64) * 0.9 + 0.1 * pred
    want = -(torch.log(pred) * soft).sum(1).mean()
    assert abs(float(loss.detach()) - float(want)) <= 1e-6
    assert np.abs(crit.soft_labels[[2, 0]].double().numpy() - soft.numpy()).max() <= 1e-6
    assert torch.equal(crit.soft_labels[[1, 3]], torch.tensor([[0.0, 1.0], [1.0, 0.0]]))
    loss.backward()
    want_grad = (pred * soft.sum(1, keepdim=True) - soft) / 2
    assert np.abs(logits.grad.double().numpy() - want_grad.numpy()).max() <= 1e-6


def test_phase_logic_without_a_device():
    args = SC.selc_args()
    crit = tm.SELCLoss(np.zeros(48, dtype=np.int64), 2, es=SC.SELC_ES)
    assert not tm.selc_phase(crit, 1) and tm.selc_phase(crit, 2) and not tm.selc_phase(crit, None)
    assert not tm.selc_phase(tm.CELoss(2), 5)
    torch.manual_seed(0)
    net = tm.build_model(args)
    x, t = torch.zeros(4, 4, 2500), torch.zeros(4, 2)
    # host tensors never take the fused node, in either phase
    assert tm.fused_loss_model(net, crit, x, t, 1) is None
    assert tm.selc_fused_model(net, crit, x, t, 2) is None
    opt, sched = tm.make_optimizer(args, net)
    batch = SC.selc_batches()[0]
    for epoch in (1, 2):
        assert tm._epoch_graphed_step(args, net, opt, sched, crit, CPU, epoch, batch) is None
    # selc=True is keyword-only and needs soft labels; both are decided before anything is allocated
    with pytest.raises(ValueError, match="soft_labels"):
        tm.GraphedTrainStep(args, net, opt, sched, tm.CELoss(2), CPU, 4, 4, 2500, selc=True)
    with pytest.raises(TypeError):
        tm.GraphedTrainStep(args, net, opt, sched, crit, CPU, 4, 4, 2500, None, True)


def test_head_function_refuses_selc_with_latent():
    f = models.PotesHeadLossFunction
    feat, w1, w2 = torch.zeros(2, 8), torch.zeros(20, 8), torch.zeros(2, 20)
    with pytest.raises(ValueError, match="exclude"):
        f.apply(feat, w1, None, w2, None, torch.zeros(2, 2), 0.0, 0.0, False, None, False,
                (None, None, 1.0), (None, None, 0.9))
