"""The cut-and-paste family, durmixrespscale and bare cutout on the GPU: ``augment()`` against the
reference's recordings (tests/golden/cutpaste_*, cutout2d_*) bit for bit, the two kernels of
csrc/pcgmix_cutpaste.hip against their numpy restatements (tests/cutpaste_ref.py) on random tables,
``out=``, the entry points' argument checks, and the training steps.

Bit-exactness is derived, not measured: every output element is a copy, a zero, one fp32 mul, mul,
add, or one float64 product / two-term sum rounded once, and every transcendental value (the
sinusoid, the sigmoid tables) is computed on the host by numpy as the reference computes it."""
import argparse
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, augmentations, augmentations2d, hostprep, models, synthetic
from pcgmix_amd import train_model as tm
from cutpaste_ref import (CUTOUT2D_FILES, CUTPASTE_FILES, assert_np_state, load, replay_cutpaste,
                          replay_mixscale, replay_pieces, replay_plan, set_np_state)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INVALID = 1                  # hipErrorInvalidValue


class Args:
    def __init__(self, method, batch_size=64, sample_rate=1000):
        self.method = method
        self.num_classes = 2
        self.batch_size = batch_size
        self.sample_rate = sample_rate
        self.model = "Potes"


class Step:
    def __init__(self, count):
        self.count = count


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ augment() against the reference
@pytest.mark.parametrize("host", [False, True], ids=["ohe", "host_labels"])
@pytest.mark.parametrize("path", CUTPASTE_FILES, ids=os.path.basename)
def test_augment_matches_the_reference(path, host):
    g = load(path)
    method, step = g["method"], g["step"]
    name = hostprep.cutpaste_recipe(method, False)
    data = dev(g["x"])
    tgt = torch.nn.functional.one_hot(torch.from_numpy(g["labels"]), 2).to(DEV)
    set_np_state(g)
    py = random.getstate()
    res = augmentations.augment(Args(method, g["batch_size"], g["sample_rate"]), data, tgt,
                                torch.from_numpy(g["frames"]), g["wav"], Step(step), None, DEV, "",
                                host_labels=g["labels"] if host else None)
    torch.cuda.synchronize()
    assert isinstance(res, tuple) and len(res) == 4
    y, t_out, mix, cut = res
    assert random.getstate() == py
    assert_np_state(g)
    assert (y is data) == bool(g["same_object"])
    assert t_out is tgt and np.array_equal(t_out.cpu().numpy(), g["target_out"])
    assert (cut if cut is not None else -1) == g["cut"]
    if not g["fired"]:
        assert list(mix) == [] and cut is None
        assert np.array_equal(data.cpu().numpy(), g["x"])
        return
    if name == "cutout":
        assert y is data and list(mix) == []                     # zeroed in place
    else:
        assert y.data_ptr() != data.data_ptr()
        assert np.array_equal(data.cpu().numpy(), g["x"])        # the input is untouched
        if name == "durmixrespscale":
            assert isinstance(mix, list) and mix == []           # the reference returns no partners here
        else:
            assert np.array_equal(np.asarray(mix, dtype=np.int64), g["mix"])
    assert y.dtype == torch.float32 and tuple(y.shape) == g["y"].shape
    assert np.array_equal(y.cpu().numpy(), g["y"])               # bit-exact


@pytest.mark.parametrize("path", CUTOUT2D_FILES, ids=os.path.basename)
def test_augment2d_cutout_matches_the_reference(path):
    g = load(path)
    data = dev(g["x"])
    tgt = torch.nn.functional.one_hot(torch.from_numpy(g["labels"]), 2).to(DEV)
    set_np_state(g)
    py = random.getstate()
    y, t_out, mix, cut = augmentations2d.augment(Args(g["method"]), data, tgt, torch.from_numpy(g["frames"]),
                                                 None, Step(g["step"]), None, DEV, "")
    torch.cuda.synchronize()
    assert random.getstate() == py
    assert_np_state(g)                                          # numpy's global stream is not touched
    assert y is data and t_out is tgt and list(mix) == [] and cut is None
    assert np.array_equal(y.cpu().numpy(), g["y"])
    if not g["fired"]:
        assert np.array_equal(g["y"], g["x"])


def test_empty_batch():
    for method in ("labelcutmix(smooth)", "durratiocutmix", "durmixrespscale", "cutout", "cutout(ch)"):
        data = torch.zeros((0, 4, 5000), device=DEV)
        tgt = torch.zeros((0, 2), dtype=torch.int64, device=DEV)
        np.random.seed(1)
        y, _, mix, _ = augmentations.augment(Args(method), data, tgt, torch.zeros((0, 5), dtype=torch.int64), (),
                                             Step(3), None, DEV, "")
        assert tuple(y.shape) == (0, 4, 5000) and len(mix) == 0 and (y is data) == ("cutout" in method)


# ------------------------------------------------------------------ the kernels on random tables
SHAPES = [(1, 1, 37), (2, 3, 101), (33, 4, 250), (2, 1, 64), (33, 3, 1023), (1, 4, 4), (2, 4, 5000),
          (33, 1, 998), (1, 3, 2048), (2, 4, 12), (256, 4, 5000)]


def random_table(rs, B, T, wild):
    """Ordered, contiguous segments with random kinds; ``wild``: shifts that point outside the row."""
    segs = np.zeros((B, 5, 4), dtype=np.int32)
    cuts = np.sort(rs.randint(0, T + 1, size=(B, 4)), axis=1)
    bounds = np.concatenate([np.zeros((B, 1), int), cuts, np.full((B, 1), T)], axis=1)
    if wild:
        bounds[:, 5] = rs.randint(T // 2, T + 1, size=B)        # the table may end before the row does
        bounds = np.minimum(bounds, bounds[:, 5:6])
    segs[:, :, 0] = bounds[:, :5]
    segs[:, :, 1] = bounds[:, 1:]
    segs[:, :, 2] = rs.randint(0, 3, size=(B, 5))
    span = T if wild else 0
    for b in range(B):
        for k in range(5):
            lo, hi = segs[b, k, 0], segs[b, k, 1]
            if wild:
                segs[b, k, 3] = rs.randint(-span, span + 1)
            elif hi > lo:
                segs[b, k, 3] = rs.randint(-lo, T - hi + 1)      # the whole source inside the row
    return segs


def random_junctions(rs, B, T, wild):
    j = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        ov = int(rs.randint(0, 11))
        if wild:
            j[b] = (rs.randint(-5, T + 6), rs.randint(-T, 2 * T), rs.randint(-2, 14), rs.randint(0, 9))
        elif 2 * ov <= T and ov > 0:
            j[b] = (rs.randint(ov, T - ov + 1), rs.randint(ov, T - ov + 1), ov, 0)
    return j


def run_cutpaste(x, segs, mix, junc, out=None):
    lib = _lib.load()
    xd, sd, md = dev(x), dev(segs), dev(mix.astype(np.int32))
    jd = dev(junc) if junc is not None else None
    tab = dev(hostprep.sigmoid_table().copy())
    yd = torch.full_like(xd, 7.0) if out is None else out
    B, C, T = x.shape
    err = lib.pcgmix_cutpaste_rows_f32(xd.data_ptr(), yd.data_ptr(), sd.data_ptr(), md.data_ptr(),
                                       jd.data_ptr() if jd is not None else None,
                                       tab.data_ptr() if jd is not None else None, B, C, T, stream())
    assert err == 0
    torch.cuda.synchronize()
    return yd.cpu().numpy()


@pytest.mark.parametrize("wild", [False, True], ids=["valid", "sources_outside_the_row"])
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cutpaste_kernel_on_random_tables(shape, seed, wild):
    """44 random cases: odd T, T % 4 != 0, C in {1, 3, 4}, B in {1, 2, 33}.  ``wild`` tables point
    outside the row (and past the coefficient table): zeros there — the kernel's range checks; all
    memory the test hands over is valid."""
    B, C, T = shape
    rs = np.random.RandomState(1000 * seed + B * 7 + C * 3 + T)
    x = rs.standard_normal(shape).astype(np.float32)
    segs = random_table(rs, B, T, wild)
    mix = rs.randint(0, B, size=B)
    junc = random_junctions(rs, B, T, wild) if seed or wild else None
    got = run_cutpaste(x, segs, mix, junc)
    want = replay_cutpaste(x, segs, mix, junc, hostprep.sigmoid_table())
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ one kernel behind both entry points
@pytest.mark.parametrize("wild", [False, True], ids=["valid", "sources_outside_the_row"])
@pytest.mark.parametrize("T", [37, 64], ids=["by_element", "by_quad"])
def test_same_table_through_both_entry_points(T, wild):
    """pcgmix_cutpaste_rows_f32 without junctions and pcgmix_piecewise_rows_f32 along the columns of a
    one-row image (F = 1, W = Wo = T) are the same copy: identical bytes, equal to the restatement."""
    B, C = 3, 2
    rs = np.random.RandomState(10 * T + wild)
    x = rs.standard_normal((B, C, T)).astype(np.float32)
    segs = random_table(rs, B, T, wild)
    mix = rs.randint(0, B, size=B)
    one = run_cutpaste(x, segs, mix, None)
    two = augmentations2d.piecewise_rows(dev(x).view(B, C, 1, T), segs, mix, 0, T)
    torch.cuda.synchronize()
    two = two.cpu().numpy()[:, :, 0, :]
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))
    assert np.array_equal(one, replay_pieces(x[:, :, None, :], segs, mix, 0, T)[:, :, 0, :])


BIG_B = 32768 + 2            # the batch runs along gridDim.y up to 32768, then along gridDim.z


@pytest.mark.parametrize("wild", [False, True], ids=["valid", "sources_outside_the_row"])
def test_cutpaste_batch_across_the_grid_z_boundary(wild):
    B, C, T = BIG_B, 1, 8
    rs = np.random.RandomState(5 + wild)
    x = rs.standard_normal((B, C, T)).astype(np.float32)
    segs = random_table(rs, B, T, wild)
    mix = rs.randint(0, B, size=B)                               # partners on either side of the boundary
    junc = random_junctions(rs, B, T, wild)
    got = run_cutpaste(x, segs, mix, junc)
    assert np.array_equal(got, replay_cutpaste(x, segs, mix, junc, hostprep.sigmoid_table()))


@pytest.mark.parametrize("axis", [0, 1], ids=["columns", "freq_rows"])
def test_piecewise_batch_across_the_grid_z_boundary(axis):
    B, C, F, W = BIG_B, 1, 2, 4
    rs = np.random.RandomState(7 + axis)
    x = rs.standard_normal((B, C, F, W)).astype(np.float32)
    segs = random_table(rs, B, W if axis == 0 else F, True)
    mix = rs.randint(0, B, size=B)
    y = augmentations2d.piecewise_rows(dev(x), segs, mix, axis, W)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), replay_pieces(x, segs, mix, axis, W))


def random_splice(rs, B, C, T):
    lens = rs.randint(0, max(2, T // 5), size=(B, 4))
    frames = np.zeros((B, 5), dtype=np.int64)
    frames[:, 1:] = np.cumsum(lens, axis=1)
    assert frames.max() <= T
    mix = rs.randint(0, B, size=B)
    gap = np.abs(np.diff(frames[mix], axis=1) - np.diff(frames, axis=1))
    off = (rs.random_sample((B, 4)) * (gap + 1)).astype(np.int32)
    row = np.sin(rs.uniform(0, 7) + np.linspace(0, 9, T))
    return frames, mix, off, row


def run_mixscale(x, frames, mix, off, lam, row):
    lib = _lib.load()
    xd, fd, md = dev(x), dev(frames.astype(np.int32)), dev(mix.astype(np.int32))
    od = dev(off) if off is not None else None
    rd = dev(row)
    yd = torch.full_like(xd, 7.0)
    B, C, T = x.shape
    err = lib.pcgmix_mix_scale_f32(xd.data_ptr(), yd.data_ptr(), fd.data_ptr(), md.data_ptr(),
                                   od.data_ptr() if od is not None else None, ctypes.c_float(lam),
                                   rd.data_ptr(), B, C, T, stream())
    assert err == 0
    torch.cuda.synchronize()
    return yd.cpu().numpy()


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_scale_kernel_on_random_plans(shape, seed):
    B, C, T = shape
    rs = np.random.RandomState(2000 * seed + B * 7 + C * 3 + T)
    x = rs.standard_normal(shape).astype(np.float32)
    frames, mix, off, row = random_splice(rs, B, C, T)
    lam = float(np.float32(rs.uniform(0, 1)))
    got = run_mixscale(x, frames, mix, off if seed else None, lam, row)
    want = replay_mixscale(x, frames, mix, off if seed else None, lam, row)
    assert np.array_equal(got, want)


FULL = ["durratiocutmix", "(rand)durratiocutmix", "(rand)labelcutmix", "labelcutmix(smooth)(cutout)",
        "lengthcutmix(5bins)", "wavcutmix", "datasetcutmix(smooth)", "durmixrespscale", "(rand)durmixrespscale",
        "cutout", "cutout(ch)"]


@pytest.mark.parametrize("method", FULL)
def test_full_size_against_the_replay(method):
    """(256, 4, 5000) through augment() against the plan replayed in numpy."""
    x, frames, labels, wav = synthetic.make_batch(256, 4, 5000, seed=31)
    wav = tuple(f"{'abcd'[i % 4]}{i // 8:04d}" for i in range(256))
    step = 7
    np.random.seed(11)
    plan = hostprep.cutpaste_plan(method, labels, frames, wav, step, 256, 4, 5000, batch_size=256,
                                  sample_rate=1000)
    assert plan.fired
    want = replay_plan(plan, x, frames, hostprep.sigmoid_table())
    data = dev(x)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(DEV)
    np.random.seed(11)
    y, _, mix, cut = augmentations.augment(Args(method, 256), data, tgt, torch.from_numpy(frames), wav, Step(step),
                                           None, DEV, "")
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), want) and not np.array_equal(want, x)
    if plan.kind == "cutpaste":
        assert np.array_equal(mix, plan.mix) and cut == plan.cut and not np.array_equal(mix, np.arange(256))


# ------------------------------------------------------------------ out=, argument checks
@pytest.mark.parametrize("method", ["labelcutmix(smooth)(cutout)", "(rand)wav-durratiocutmix", "durmixrespscale",
                                    "cutout", "cutout(ch)"])
def test_apply_plan_writes_into_out(method):
    x, frames, labels, wav = synthetic.make_batch(9, 3, 501, seed=3, rate_scale=0.3)
    wav = tuple("ab"[i % 2] for i in range(9))
    np.random.seed(5)
    plan = hostprep.cutpaste_plan(method, labels, frames, wav, 4, 9, 3, 501, batch_size=9, sample_rate=1000)
    data = dev(x)
    out = torch.full_like(data, 7.0)
    y = augmentations.apply_plan(plan, data, frames, out=out)
    torch.cuda.synchronize()
    assert y is out and np.array_equal(data.cpu().numpy(), x)     # cutout with out=: data untouched
    assert np.array_equal(out.cpu().numpy(), replay_plan(plan, x, frames, hostprep.sigmoid_table()))
    with pytest.raises(ValueError, match="out must be"):
        augmentations.apply_plan(plan, data, frames, out=data)
    with pytest.raises(ValueError, match="out must be"):
        augmentations.apply_plan(plan, data, frames, out=torch.empty((9, 3, 500), device=DEV))


def test_apply_plan_refuses_partners_outside_the_batch():
    x, frames, labels, wav = synthetic.make_batch(6, 2, 320, seed=3, rate_scale=0.2)
    plan = hostprep.cutpaste_plan("labelcutmix", labels, frames, wav, 3, 6, 2, 320)
    plan.mix = plan.mix.copy()
    plan.mix[2] = 6
    with pytest.raises(ValueError, match="partner index"):
        augmentations.apply_plan(plan, dev(x), frames)


def test_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    B, C, T = 4, 2, 64
    x = torch.zeros((B, C, T), device=DEV)
    y = torch.zeros_like(x)
    both = torch.zeros((2 * B, C, T), device=DEV)
    segs = torch.zeros((B, 5, 4), dtype=torch.int32, device=DEV)
    idx = torch.zeros((B, 5), dtype=torch.int32, device=DEV)
    mix = torch.zeros(B, dtype=torch.int32, device=DEV)
    junc = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    tab = dev(hostprep.sigmoid_table().copy())
    row = torch.zeros(T, dtype=torch.float64, device=DEV)
    s = stream()
    X, Y, S, M, J, Tb, R, Fr = (t.data_ptr() for t in (x, y, segs, mix, junc, tab, row, idx))
    cp = lib.pcgmix_cutpaste_rows_f32
    assert cp(X, Y, S, M, None, None, B, C, T, s) == 0
    assert cp(X, Y, S, M, J, Tb, B, C, T, s) == 0
    assert cp(None, None, None, None, None, None, 0, C, T, s) == 0          # B == 0: nothing to do
    for bad in [(None, Y, S, M, None, None, B, C, T), (X, None, S, M, None, None, B, C, T),
                (X, Y, None, M, None, None, B, C, T), (X, Y, S, None, None, None, B, C, T),
                (X, Y, S, M, J, None, B, C, T),                               # junctions without the table
                (X, X, S, M, None, None, B, C, T),                            # aliasing
                (both.data_ptr(), both.data_ptr() + 4 * C * T * 2, S, M, None, None, B, C, T),   # overlap
                (X, Y, S, M, None, None, -1, C, T), (X, Y, S, M, None, None, B, 0, T),
                (X, Y, S, M, None, None, B, C, 0), (X, Y, S, M, None, None, B, 1 << 16, 1 << 16)]:
        assert cp(*bad, s) == INVALID, bad
    ms = lib.pcgmix_mix_scale_f32
    lam = ctypes.c_float(0.5)
    assert ms(X, Y, Fr, M, None, lam, R, B, C, T, s) == 0
    assert ms(None, None, None, None, None, lam, None, 0, C, T, s) == 0
    for bad in [(None, Y, Fr, M, None, lam, R, B, C, T), (X, None, Fr, M, None, lam, R, B, C, T),
                (X, Y, None, M, None, lam, R, B, C, T), (X, Y, Fr, None, None, lam, R, B, C, T),
                (X, Y, Fr, M, None, lam, None, B, C, T), (X, X, Fr, M, None, lam, R, B, C, T),
                (both.data_ptr(), both.data_ptr() + 4 * C * T * 2, Fr, M, None, lam, R, B, C, T),
                (X, Y, Fr, M, None, lam, R, -1, C, T), (X, Y, Fr, M, None, lam, R, B, 0, T),
                (X, Y, Fr, M, None, lam, R, B, C, 0), (X, Y, Fr, M, None, lam, R, B, 1 << 16, 1 << 16)]:
        assert ms(*bad, s) == INVALID, bad
    torch.cuda.synchronize()


def test_one_launch_per_call():
    from torch.profiler import profile, ProfilerActivity
    x, frames, labels, wav = synthetic.make_batch(32, 4, 2000, seed=9)
    data = dev(x)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(DEV)
    for method, kernel in (("labelcutmix(smooth)(cutout)", "cutpaste_rows_kernel"),
                           ("(rand)durratiocutmix", "cutpaste_rows_kernel"),
                           ("durmixrespscale", "splice_scale_kernel"), ("cutout(ch)", "zero_spans_kernel")):
        augmentations.augment(Args(method), data.clone(), tgt, torch.from_numpy(frames), wav, Step(3), None,
                              DEV, "", host_labels=labels)                  # warm-up: tables, staging
        torch.cuda.synchronize()
        d = data.clone()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            augmentations.augment(Args(method), d, tgt, torch.from_numpy(frames), wav, Step(3), None, DEV, "",
                                  host_labels=labels)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if "Memcpy" not in e.name and "Memset" not in e.name]
        ours = sorted({n for n in names if "pcgmix" in n})
        assert len(ours) == 1 and kernel in ours[0], names


# ------------------------------------------------------------------ training
def _batch(B, T, seed):
    x, frames, labels, wav = synthetic.make_batch(B, 4, T, sample_rate=1000, seed=seed)
    wav = tuple(f"{'ab'[i % 2]}{i // 4:04d}" for i in range(B))
    return (torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(frames), wav,
            torch.ones(B, dtype=torch.long), torch.arange(B))


def _train_args(method, B, T):
    return argparse.Namespace(dataset="PhysioNet", model="Potes", method=method, num_epochs=2, batch_size=B,
                              op="adam", use_sched=False, lr_max=0.003, weight_decay=0.0, grad_clip=0.1,
                              seed=4, num_classes=2, num_channels=4, sig_len=T, depth=0, num_steps=8,
                              sample_rate=1000)


@pytest.mark.parametrize("method", ["labelcutmix", "durmixrespscale", "(rand)labelcutmix(smooth)(cutout)+0.7",
                                    "cutout(ch)"])
def test_five_eager_train_steps(method, monkeypatch):
    """Five train_step()s on Potes: finite losses, hard int64 targets, and the batch the model saw
    is augment()'s output for that step."""
    B, T = 32, 2500
    args = _train_args(method, B, T)
    assert not hostprep.soft_targets(method)
    torch.manual_seed(3)
    net = tm.build_model(args).to(DEV).train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(np.zeros(B, int), 2, es=3, device=DEV)
    seen = []
    orig = models.CNN_potes.loss_and_logits

    def spy(self, x, target, latent=None):
        seen.append((x.detach().clone(), target.detach().clone()))
        return orig(self, x, target, latent=latent)

    monkeypatch.setattr(models.CNN_potes, "loss_and_logits", spy)
    sc = tm.step_counter_class()
    for i in range(5):
        batch = _batch(B, T, 40 + i)
        step = sc.count
        loss = tm.train_step(args, net, batch, DEV, opt, sched, crit, 1, sc)
        assert np.isfinite(float(loss)) and sc.count == step + 1 and len(seen) == i + 1
        tgt = torch.nn.functional.one_hot(batch[1], 2).to(DEV)
        state = np.random.get_state()
        want, t_out, _, _ = augmentations.augment(args, batch[0].to(DEV), tgt, batch[2], batch[3], Step(step),
                                                  net, DEV, None)
        np.random.set_state(state)
        assert torch.equal(seen[i][0], want)
        assert seen[i][1].dtype == torch.int64 and torch.equal(seen[i][1], tgt)
        if hostprep.gate_fires(method, step):
            assert not torch.equal(want, batch[0].to(DEV))


@pytest.mark.parametrize("method", ["labelcutmix", "durmixrespscale(12,20)", "cutout"])
def test_graphed_and_pipelined_steps_refuse_with_the_methods_name(method):
    B, T = 32, 2500
    args = _train_args(method, B, T)
    net = tm.build_model(args).to(DEV)
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(np.zeros(B, int), 2, es=3, device=DEV)
    for cls in (tm.GraphedTrainStep, tm.PipelinedTrainStep):
        with pytest.raises(NotImplementedError) as e:
            cls(args, net, opt, sched, crit, DEV, B, 4, T)
        assert method in str(e.value) and "train_step" in str(e.value)
    assert tm._epoch_graphed_step(args, net, opt, sched, crit, DEV, 1, _batch(B, T, 1)) is None
    args.method = "durratiomixup"
    assert tm._epoch_graphed_step(args, net, opt, sched, crit, DEV, 1, _batch(B, T, 1)) is not None
