"""The paper's 1D comparison baselines on the GPU: augment() against the reference's recordings
(tests/golden/base1d_*), full-size batches against CPU restatements, B = 0, a time warp above the
LDS threshold, and train_epoch graphed and eager."""
import argparse
import glob
import os
import random

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import augmentations, hostprep, synthetic
from test_baselines_cpu import (BASE_FILES, assert_np_state, check_warped, load, scipy_row,
                                set_np_state)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class Args:
    def __init__(self, method, sample_rate=1000):
        self.method = method
        self.num_classes = 2
        self.sample_rate = sample_rate


class Step:
    def __init__(self, count):
        self.count = count


def run(method, x, labels, frames, wav, step, host_labels=None, sample_rate=1000):
    data = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(np.asarray(labels, dtype=np.int64)), 2).to(DEV)
    out = augmentations.augment(Args(method, sample_rate), data, tgt, torch.from_numpy(frames), wav,
                                Step(step), None, DEV, "", host_labels=host_labels)
    torch.cuda.synchronize()
    return data, tgt, out


@pytest.mark.parametrize("host", [False, True], ids=["ohe", "host_labels"])
@pytest.mark.parametrize("path", BASE_FILES, ids=os.path.basename)
def test_augment_matches_the_reference(path, host):
    g = load(path)
    method, step = str(g["method"]), int(g["step"])
    set_np_state(g, "np_before")
    py = random.getstate()
    data, tgt, (y, t_out, mix, cut) = run(method, g["x"], g["labels"], g["frames"], list(g["wav"]), step,
                                          g["labels"] if host else None, int(g["sample_rate"]))
    assert cut is None and random.getstate() == py
    assert_np_state(g)
    if not int(g["fired"]):
        assert y is data and t_out is tgt and list(mix) == []
        return
    if "timemask" in method:
        assert y is data                                        # zeroed in place
    else:
        assert y is not data and y.data_ptr() != data.data_ptr()
        assert np.array_equal(data.cpu().numpy(), g["x"])      # the input is untouched
    assert np.array_equal(np.asarray(mix, dtype=np.int64), g["mix"])
    assert np.array_equal(t_out.cpu().numpy(), g["target_out"])
    got = y.cpu().numpy()
    if "magnitudewarp" in method:
        from test_baselines_cpu import ulp_diff
        d = ulp_diff(got, g["y"])
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
    elif "timewarp" in method:
        check_warped(got, g["y"], g["x"])
    else:
        assert np.array_equal(got, g["y"])                      # bit-exact


def test_timemask_writes_into_out_when_given():
    x, frames, labels, wav = synthetic.make_batch(6, 3, 501, seed=3, rate_scale=0.35)
    plan = hostprep.make_plan("timemask(0.3)", labels, frames, wav, 4, 6, 3, sig_len=501)
    data = torch.from_numpy(x).to(DEV)
    out = torch.full_like(data, 7.0)
    y = augmentations.apply_plan(plan, data, frames, out=out)
    torch.cuda.synchronize()
    assert y is out and np.array_equal(data.cpu().numpy(), x)
    ref = x.copy()
    for b, (s0, s1) in enumerate(plan.spans):
        ref[b, :, s0:s1] = 0
    assert np.array_equal(out.cpu().numpy(), ref) and (plan.spans[:, 1] > plan.spans[:, 0]).any()


@pytest.mark.parametrize("method", ["mixup(same)", "mixup(mix)", "magnitudewarp(0.2,4)",
                                    "timewarp(0.05,4)", "timemask(0.2)", "respiratoryscale(12,20)"])
def test_empty_batch(method):
    x = np.zeros((0, 4, 5000), np.float32)
    frames = np.zeros((0, 5), np.int64)
    np.random.seed(1)
    data, tgt, (y, t_out, mix, _) = run(method, x, np.zeros(0, np.int64), frames, [], 3)
    assert tuple(y.shape) == (0, 4, 5000) and len(mix) == 0
    assert (y is data) == ("timemask" in method)


def full_batch():
    return synthetic.make_batch(256, 4, 5000, seed=31)


@pytest.mark.parametrize("method", ["mixup(same)", "mixup(mix)", "magnitudewarp(0.2,4)",
                                    "timewarp(0.05,4)", "timemask(0.2)", "respiratoryscale(12,20)"])
def test_full_size_against_cpu(method):
    """(256, 4, 5000) once per method against restatements on the CPU: the oracle's
    magnitude_warp, scipy/numpy for the time warp, numpy for the rest."""
    from oracle import pcgmix_oracle as O
    x, frames, labels, wav = full_batch()
    step = 7
    np.random.seed(11)
    plan = hostprep.make_plan(method, labels, frames, wav, step, *x.shape[:2], sample_rate=1000,
                              sig_len=x.shape[2])
    np.random.seed(11)
    data, tgt, (y, t_out, mix, _) = run(method, x, labels, frames, wav, step)
    got = y.cpu().numpy()
    if plan.kind == "mixup":
        lam = np.float32(plan.lam32)
        assert np.array_equal(got, x * lam + x[plan.mix] * (np.float32(1) - lam))
        assert np.array_equal(mix, plan.mix)
    elif plan.kind == "magnitudewarp":
        np.random.seed(11)                      # the oracle draws the same knots from numpy's stream
        ref = np.transpose(O.magnitude_warp(np.transpose(x, (0, 2, 1)), 0.2, 4), (0, 2, 1))
        from test_baselines_cpu import ulp_diff
        d = ulp_diff(got, ref)
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
    elif plan.kind == "timewarp":
        rows = [(b, c) for b in range(0, 256, 9) for c in range(4)]
        want = np.stack([scipy_row(plan.knots[b, :, c], x[b, c])[0] for b, c in rows])
        check_warped(np.stack([got[b, c] for b, c in rows]), want, np.stack([x[b, c] for b, c in rows]))
    elif plan.kind == "timemask":
        ref = x.copy()
        for b, (s0, s1) in enumerate(plan.spans):
            ref[b, :, s0:s1] = 0
        assert np.array_equal(got, ref)
    else:
        assert np.array_equal(got, (x.astype(np.float64) * plan.scale_row).astype(np.float32))


def test_time_warp_above_the_lds_threshold():
    """T = 6001 (odd, above the 5120 samples whose xp fits in LDS): the global workspace path,
    with non-monotone rows at sigma 0.2."""
    x, frames, labels, wav = synthetic.make_batch(6, 3, 6001, seed=5)
    np.random.seed(2)
    plan = hostprep.make_plan("timewarp(0.2,4)", labels, frames, wav, 3, 6, 3, sig_len=6001)
    assert augmentations._lib.load().pcgmix_time_warp_workspace_bytes(6, 3, 6001) > 0
    np.random.seed(2)
    _, _, (y, *_rest) = run("timewarp(0.2,4)", x, labels, frames, wav, 3)
    got = y.cpu().numpy().reshape(18, 6001)
    want, nonmono = [], 0
    for b in range(6):
        for c in range(3):
            yr, xp = scipy_row(plan.knots[b, :, c], x[b, c])
            want.append(yr)
            nonmono += bool((np.diff(xp) < 0).any())
    check_warped(got, np.stack(want), x.reshape(18, 6001))
    assert nonmono > 0


# ------------------------------------------------------------------ training
def epoch_result(method, hipgraph, device, steps=6):
    from pcgmix_amd import train_model as tm
    B, C, T = 16, 4, 2500
    batches = []
    for i in range(steps):
        x, frames, labels, wav = synthetic.make_batch(B, C, T, sample_rate=1000, seed=900 + i)
        batches.append((torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(frames), wav,
                        torch.ones(B, dtype=torch.long), torch.arange(B)))
    args = argparse.Namespace(dataset="PhysioNet", model="Potes", method=method, num_epochs=2,
                              batch_size=B, op="adam", use_sched=True, lr_max=0.01, weight_decay=1e-4,
                              grad_clip=0.1, seed=4, num_classes=2, num_channels=C, sig_len=T, depth=0,
                              num_steps=steps, sample_rate=1000, hipgraph=hipgraph)
    torch.manual_seed(0)
    net = tm.build_model(args).to(device)
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(np.concatenate([b[1].numpy() for b in batches]), 2, es=args.num_epochs + 1,
                       device=device)
    sc = tm.step_counter_class()
    np.random.seed(0)
    loss, acc, lrs = tm.train_epoch(args, net, batches, device, opt, sched, crit, 1, sc)
    step = net.__dict__.get("_pcgmix_epoch_step")
    assert (step is not None and isinstance(step.step, tm.GraphedTrainStep)) == hipgraph
    assert sc.count == steps and np.isfinite(loss)
    return loss, acc, lrs, [p.detach().cpu().clone() for p in net.parameters() if p.requires_grad]


@pytest.mark.parametrize("method", ["mixup(same)", "mixup(mix)", "magnitudewarp(0.2,4)",
                                    "timewarp(0.05,4)", "timemask(0.2)", "respiratoryscale(12,20)+0.5"])
def test_train_epoch_graphed_and_eager_agree(method):
    """train_epoch on its default captured path and with ``args.hipgraph = False``: the same
    augmentation either way, so the same epoch up to the captured step's own rounding (the bound
    tests/test_train_r3_gpu.py uses: mean loss 1e-4, accuracy and learning rates exact,
    parameters 1e-3)."""
    g = epoch_result(method, True, DEV)
    e = epoch_result(method, False, DEV)
    assert abs(g[0] - e[0]) <= 1e-4 * max(1.0, abs(e[0])), (g[0], e[0])
    assert g[1] == e[1] and g[2] == e[2]
    for a, b in zip(g[3], e[3]):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-3)
