"""ClipSGD on the GPU: the multi-tensor clip + SGD kernel against torch on exact-arithmetic inputs
(bit for bit) and on random ones (against float64), checkpoints, the captured update node, and the
captured Potes / ResNet9 steps with op='SGD'."""
import argparse
import copy

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import synthetic, train_model as tm
from test_sgd_cpu import EXACT_STEPS, exact_case, sgd_f64

pytestmark = pytest.mark.gpu

REDUCE = "pcgmix_sgd_clip_multi_reduce_dev_f32"


def _clip_sgd(case, device):
    hp = case["hp"]
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(device)) for a in case["p0"]]
    return params, tm.ClipSGD(params, lr=hp["lr"], momentum=hp["mom"], weight_decay=hp["wd"],
                              clip_value=hp["clip"])


def _assert_equals_case(params, opt, case):
    for i, (q, want) in enumerate(zip(params, case["p"])):
        assert torch.equal(q.detach().cpu(), torch.from_numpy(want)), (i, case["sizes"][i])
        buf = opt.state.get(q, {}).get("momentum_buffer")
        if case["buf"][i] is None:
            assert buf is None
        else:
            assert torch.equal(buf.cpu(), torch.from_numpy(case["buf"][i])), (i, case["sizes"][i])


@pytest.mark.parametrize("count,variant", [(1, "all"), (32, "all"), (33, "all"), (65, "all"),
                                           (33, "clip0"), (33, "wd0"), (33, "mom0")])
def test_exact_arithmetic_eager_equals_torch_cpu(count, variant, device):
    """Dyadic inputs, power-of-two scalars (tests/test_sgd_cpu.py shows every intermediate is a
    float32 number): parameters and momentum buffers after 4 eager steps == clip_grad_value_ +
    torch.optim.SGD on the CPU, bit for bit, across the 32-tensor table boundary and the
    1024-element block boundary, with a zero-sized tensor in the middle."""
    case = exact_case(count, variant)
    params, opt = _clip_sgd(case, device)
    for step in case["grads"]:
        for q, g in zip(params, step):
            q.grad = torch.from_numpy(g).to(device)
        kept = [q.grad.clone() for q in params]
        opt.step()
        assert all(torch.equal(q.grad, k) for q, k in zip(params, kept))     # gradients are not modified
    _assert_equals_case(params, opt, case)
    if variant == "mom0":
        assert len(opt.state) == 0 and opt.state_dict() == case["state_dict"]


def test_exact_arithmetic_channels_last_weight(device):
    """A channels_last 4-D weight whose gradient arrives contiguous (the ``_dense_grads`` copy) or
    in the weight's own layout: the same bits as torch on the CPU."""
    rs = np.random.RandomState(5)
    shape = (16, 8, 3, 3)
    dy = lambda: torch.from_numpy((rs.randint(-128, 129, size=shape) / 16.0).astype(np.float32))   # noqa: E731
    w = dy()
    grads = [s * dy() for s in range(1, EXACT_STEPS + 1)]
    pa = [torch.nn.Parameter(w.clone().to(device).contiguous(memory_format=torch.channels_last))]
    pb = [torch.nn.Parameter(w.clone())]
    oa = tm.ClipSGD(pa, lr=0.25, momentum=0.5, weight_decay=0.5, clip_value=2.0)
    ob = torch.optim.SGD(pb, lr=0.25, momentum=0.5, weight_decay=0.5)
    for it, g in enumerate(grads):
        ga = g.clone().to(device)
        pa[0].grad = ga.contiguous(memory_format=torch.channels_last) if it % 2 else ga
        pb[0].grad = g.clone()
        torch.nn.utils.clip_grad_value_(pb, 2.0)
        oa.step(); ob.step()
    assert pa[0].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(pa[0].detach().cpu(), pb[0].detach())
    assert torch.equal(oa.state[pa[0]]["momentum_buffer"].cpu(), ob.state[pb[0]]["momentum_buffer"])


def test_random_inputs_under_onecycle_against_float64(device):
    """10 steps under OneCycleLR (lr and momentum move every step), tensors of 5, 1030 and 40000
    elements: ClipSGD and torch.optim.SGD on the same device are two float32 roundings of one
    recurrence, which may differ in contraction.  With E = max |. - float64 restatement|:
    E_new <= 2 E_ref + 2^-23 max|p| (the floor covers E_ref = 0)."""
    torch.manual_seed(0)
    sizes = [5, 1030, 40000]
    pa = [torch.nn.Parameter(torch.randn(n, device=device)) for n in sizes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    p64 = [p.detach().cpu().numpy().astype(np.float64) for p in pa]
    b64 = [None] * len(sizes)
    oa = tm.ClipSGD(pa, lr=0.01, weight_decay=1e-4, clip_value=0.1)
    ob = torch.optim.SGD(pb, lr=0.01, weight_decay=1e-4)
    sa = torch.optim.lr_scheduler.OneCycleLR(oa, max_lr=0.01, total_steps=12)
    sb = torch.optim.lr_scheduler.OneCycleLR(ob, max_lr=0.01, total_steps=12)
    moms = []
    for it in range(10):
        ga, gb = oa.param_groups[0], ob.param_groups[0]
        assert ga["lr"] == gb["lr"] and ga["momentum"] == gb["momentum"] != 0
        moms.append(ga["momentum"])
        for i, (x, y) in enumerate(zip(pa, pb)):
            g = torch.randn_like(x) * (0.3 if it % 2 else 0.05)
            x.grad, y.grad = g.clone(), g.clone()
            p64[i], b64[i] = sgd_f64(p64[i], g.cpu().numpy(), b64[i], 0.1, ga["lr"], ga["momentum"], 1e-4)
        torch.nn.utils.clip_grad_value_(pb, 0.1)
        oa.step(); ob.step(); sa.step(); sb.step()
    assert len(set(moms)) == 10                                   # the scheduler cycled it
    for x, y, want in zip(pa, pb, p64):
        e_new = float(np.abs(x.detach().cpu().numpy().astype(np.float64) - want).max())
        e_ref = float(np.abs(y.detach().cpu().numpy().astype(np.float64) - want).max())
        bound = 2 * e_ref + 2.0 ** -23 * float(np.abs(want).max())
        print(f"n={x.numel()}: E_new={e_new:.3e} E_ref={e_ref:.3e} bound={bound:.3e}")
        assert e_new <= bound, f"n={x.numel()}: E_new={e_new:.3e} E_ref={e_ref:.3e} bound={bound:.3e}"
    for x, y, want in zip(pa, pb, b64):
        e_new = float(np.abs(oa.state[x]["momentum_buffer"].cpu().numpy().astype(np.float64) - want).max())
        e_ref = float(np.abs(ob.state[y]["momentum_buffer"].cpu().numpy().astype(np.float64) - want).max())
        bound = 2 * e_ref + 2.0 ** -23 * float(np.abs(want).max())
        print(f"n={x.numel()} buffer: E_new={e_new:.3e} E_ref={e_ref:.3e} bound={bound:.3e}")
        assert e_new <= bound, f"n={x.numel()} buffer: E_new={e_new:.3e} E_ref={e_ref:.3e} bound={bound:.3e}"


def test_checkpoints_interchange_with_torch_sgd(device):
    """State dicts of ClipSGD and torch.optim.SGD load into each other in the middle of a run and
    both runs end on the exact-arithmetic reference; loading after prepare_capture raises."""
    case = exact_case(33, "all")
    hp = case["hp"]
    pa, oa = _clip_sgd(case, device)
    pb = [torch.nn.Parameter(q.detach().clone()) for q in pa]
    ob = torch.optim.SGD(pb, lr=hp["lr"], momentum=hp["mom"], weight_decay=hp["wd"])
    for it, step in enumerate(case["grads"]):
        if it == 2:
            sa, sb = copy.deepcopy(oa.state_dict()), copy.deepcopy(ob.state_dict())
            assert sa["param_groups"] == sb["param_groups"]
            oa.load_state_dict(sb)                              # torch -> ClipSGD
            ob.load_state_dict(sa)                              # ClipSGD -> torch
        for x, y, g in zip(pa, pb, step):
            x.grad = torch.from_numpy(g).to(device)
            y.grad = x.grad.clone()
        torch.nn.utils.clip_grad_value_(pb, hp["clip"])
        oa.step(); ob.step()
    _assert_equals_case(pa, oa, case)
    _assert_equals_case(pb, ob, case)
    sd = copy.deepcopy(oa.state_dict())
    oa.prepare_capture(pa)
    with pytest.raises(RuntimeError):
        oa.load_state_dict(sd)                                  # a graph would hold the old buffers


def test_captured_update_matches_eager(device):
    """ClipSGD as a hipGraph node (scalars read from device memory, written by next_hyper before
    every replay) == the eager ClipSGD.step, bit for bit, under OneCycleLR (lr and momentum change
    every step); the state dicts agree afterwards."""
    torch.manual_seed(0)
    shapes = [(20, 19968), (8, 1, 5), (20,), (2, 20)]
    pa = [torch.nn.Parameter(torch.randn(s, device=device)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = tm.ClipSGD(pa, lr=0.01, weight_decay=1e-4, clip_value=0.1)
    ob = tm.ClipSGD(pb, lr=0.01, weight_decay=1e-4, clip_value=0.1)
    sa = torch.optim.lr_scheduler.OneCycleLR(oa, max_lr=0.01, total_steps=8)
    sb = torch.optim.lr_scheduler.OneCycleLR(ob, max_lr=0.01, total_steps=8)
    grads = [torch.zeros_like(p) for p in pa]
    for p, g in zip(pa, grads):
        p.grad = g
    hyper = torch.zeros(8, device=device)
    host = np.zeros(8, dtype=np.float32)
    assert oa.can_capture()
    oa.prepare_capture(pa)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.capture_update(hyper)
    for it in range(6):
        for g, y in zip(grads, pb):
            g.copy_(torch.randn_like(g) * (0.3 if it % 2 else 0.05))
            y.grad = g.clone()
        oa.next_hyper(host)
        assert host[2] == np.float32(oa.param_groups[0]["momentum"]) and host[3] == np.float32(oa.param_groups[0]["lr"])
        hyper.copy_(torch.from_numpy(host))
        graph.replay()
        ob.step(); sa.step(); sb.step()
        assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"]
        assert oa.param_groups[0]["momentum"] == ob.param_groups[0]["momentum"]
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
        assert torch.equal(oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"])
    sda, sdb = oa.state_dict(), ob.state_dict()
    assert sda["param_groups"] == sdb["param_groups"] and sda["state"].keys() == sdb["state"].keys()
    for k, v in sda["state"].items():
        assert v.keys() == sdb["state"][k].keys() == {"momentum_buffer"}
        assert torch.equal(v["momentum_buffer"], sdb["state"][k]["momentum_buffer"])


def test_captured_without_buffers_refuses_momentum(device):
    """Momentum 0 at capture: no buffers, the state stays empty over replays and equals the eager
    step; momentum turned on afterwards is refused by next_hyper instead of being dropped."""
    torch.manual_seed(1)
    pa = [torch.nn.Parameter(torch.randn(1500, device=device))]
    pb = [torch.nn.Parameter(pa[0].detach().clone())]
    oa = tm.ClipSGD(pa, lr=0.01, weight_decay=1e-4, clip_value=0.1)
    ob = tm.ClipSGD(pb, lr=0.01, weight_decay=1e-4, clip_value=0.1)
    pa[0].grad = torch.randn_like(pa[0]) * 0.2
    pb[0].grad = pa[0].grad.clone()
    hyper, host = torch.zeros(8, device=device), np.zeros(8, dtype=np.float32)
    oa.prepare_capture(pa)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.capture_update(hyper)
    for _ in range(2):
        oa.next_hyper(host)
        hyper.copy_(torch.from_numpy(host))
        graph.replay()
        ob.step()
    assert torch.equal(pa[0], pb[0]) and len(oa.state) == 0 and oa.state_dict()["state"] == {}
    oa.param_groups[0]["momentum"] = 0.9
    with pytest.raises(RuntimeError):
        oa.next_hyper(host)


# ------------------------------------------------------------------ the captured training steps
def _args(**kw):
    a = argparse.Namespace(dataset="PhysioNet", model="Potes", method="durratiomixup", num_epochs=2,
                           batch_size=8, op="SGD", use_sched=True, lr_max=0.01, weight_decay=1e-4,
                           grad_clip=0.1, seed=4, num_classes=2, num_channels=4, sig_len=2500, depth=0,
                           num_steps=8, sample_rate=1000)
    a.__dict__.update(kw)
    return a


def _batches(B, n, device):
    out = []
    for i in range(n):
        x, frames, labels, wav = synthetic.make_batch(B, 4, 2500, sample_rate=1000, seed=930 + i)
        out.append((torch.from_numpy(x).to(device), torch.from_numpy(labels), torch.from_numpy(frames), wav,
                    torch.ones(B, dtype=torch.long), torch.arange(B)))
    return out


def _run(args, device, batches, captured):
    """Fresh model from one seed, dropout 0; returns (losses, parameters, step object or None, opt)."""
    torch.manual_seed(3)
    net = tm.build_model(args).to(device)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net.train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(np.zeros(len(batches) * batches[0][0].shape[0], int), 2, es=args.num_epochs + 1,
                       device=device)
    sc = tm.step_counter_class()
    g = None
    if captured:
        B, C, T = batches[0][0].shape
        g = tm.GraphedTrainStep(args, net, opt, sched, crit, device, B, C, T)
        losses = [float(g.step(b, 0, sc)) for b in batches]
    else:
        losses = [float(tm.train_step(args, net, b, device, opt, sched, crit, 0, sc)) for b in batches]
    assert sc.count == len(batches)
    return losses, [p.detach().clone() for p in net.parameters() if p.requires_grad], g, opt


def test_captured_potes_step_with_sgd(device, monkeypatch):
    """op='SGD' on the captured Potes step: (a) the five direct launches, the fifth being the SGD
    reduce + update, (b) PCGMIX_NO_TAPE (the hipGraph replay), (c) PCGMIX_NO_REDUCE_FOLD (reduction
    launched on its own) give bit-identical parameters after 4 steps; (d) the eager train_step with
    the same ClipSGD agrees within test_graphed_step_matches_eager's tolerances."""
    batches = _batches(8, 4, device)
    monkeypatch.delenv("PCGMIX_NO_TAPE", raising=False)
    monkeypatch.delenv("PCGMIX_NO_REDUCE_FOLD", raising=False)
    la, pa, g, opt = _run(_args(), device, batches, True)
    assert isinstance(opt, tm.ClipSGD) and g.adam_in_graph
    assert opt.param_groups[0]["momentum"] != 0                 # OneCycleLR: momentum SGD
    assert all("momentum_buffer" in opt.state[p] for p in g.params)
    assert g.tape is not None and len(g.tape) == 5 and g.tape[-1][0] == REDUCE
    monkeypatch.setenv("PCGMIX_NO_TAPE", "1")
    lb, pb, g, opt = _run(_args(), device, batches, True)
    assert isinstance(opt, tm.ClipSGD) and g.tape is None
    monkeypatch.delenv("PCGMIX_NO_TAPE")
    monkeypatch.setenv("PCGMIX_NO_REDUCE_FOLD", "1")
    lc, pc, g, opt = _run(_args(), device, batches, True)
    assert isinstance(opt, tm.ClipSGD) and g.tape is None
    monkeypatch.delenv("PCGMIX_NO_REDUCE_FOLD")
    for other in (pb, pc):
        for x, y in zip(pa, other):
            assert torch.equal(x, y)
    assert la == lb == lc
    ld, pd, _, opt = _run(_args(), device, batches, False)
    assert isinstance(opt, tm.ClipSGD)
    assert np.allclose(la, ld, rtol=1e-4, atol=1e-5), (la, ld)
    for x, y in zip(pa, pd):
        assert torch.allclose(x, y, rtol=1e-3, atol=1e-4), float((x - y).abs().max())


def test_fused_sgd_switch_restores_torch_sgd(device, monkeypatch):
    """``train_model.FUSED_SGD = False``: make_optimizer hands out torch.optim.SGD as before, the
    clip stays a pass of its own and the update stays outside the capture."""
    net = tm.build_model(_args()).to(device)
    monkeypatch.setattr(tm, "FUSED_SGD", False)
    opt, _ = tm.make_optimizer(_args(), net)
    assert type(opt) is torch.optim.SGD and tm.clips_outside_optimizer(_args(), opt)
    monkeypatch.setattr(tm, "FUSED_SGD", True)
    opt, _ = tm.make_optimizer(_args(), net)
    assert type(opt) is tm.ClipSGD and not tm.clips_outside_optimizer(_args(), opt)


def test_captured_resnet9_step_with_sgd(device):
    """'resnet9-5k' has more than 32 parameter tensors (two tables, two launches): one captured
    step and one eager step agree within the same tolerances."""
    batches = _batches(4, 1, device)
    args = _args(model="resnet9-5k", batch_size=4)
    la, pa, g, opt = _run(args, device, batches, True)
    assert isinstance(opt, tm.ClipSGD) and g.adam_in_graph and g.tape is None and len(pa) > 32
    lb, pb, _, opt = _run(_args(model="resnet9-5k", batch_size=4), device, batches, False)
    assert isinstance(opt, tm.ClipSGD)
    assert np.allclose(la, lb, rtol=1e-4, atol=1e-5), (la, lb)
    for x, y in zip(pa, pb):
        assert torch.allclose(x, y, rtol=1e-3, atol=1e-4), float((x - y).abs().max())
