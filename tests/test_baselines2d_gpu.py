"""The paper's spectrogram comparison baselines on the GPU: augment() against the reference's
recordings (tests/golden/base2d_*), latentmixup's differentiable blend against torch's autograd,
full-size batches against torch restatements, B = 0, one ResNet9-2D train_step against a float64
CPU copy, train_model end to end, and the refusal under torch.distributed."""
import argparse
import copy
import os
import random
import sys

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import augmentations2d, hostprep, models2d, synthetic, train_model as tm
from cutpaste_ref import replay_pieces
from test_baselines2d_cpu import BASE2D_FILES, ProbeNet, load, np_state_is, set_np_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import train_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
METHODS = ["timemask(0.1)", "freqmask(0.1)", "mixup(same)", "mixup(mix)", "cutmix", "(rand)cutmix",
           "durratiocutmix", "(rand)durratiocutmix", "latentmixup"]


class Args:
    def __init__(self, method):
        self.method = method
        self.num_classes = 2
        self.model = "resnet9"
        self.depth = 0


class Step:
    def __init__(self, count):
        self.count = count


def run(method, x, labels, frames, step, host_labels=None, model=None):
    data = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(np.asarray(labels, dtype=np.int64)), 2).to(DEV)
    args = Args(method)
    out = augmentations2d.augment(args, data, tgt, torch.from_numpy(np.asarray(frames)), None, Step(step),
                                  model, DEV, "", host_labels=host_labels)
    torch.cuda.synchronize()
    return args, data, tgt, out


@pytest.mark.parametrize("host", [False, True], ids=["ohe", "host_labels"])
@pytest.mark.parametrize("path", BASE2D_FILES, ids=os.path.basename)
def test_augment_matches_the_reference(path, host):
    g = load(path)
    method, step = str(g["method"]), int(g["step"])
    set_np_state(g, "np_before")
    py = random.getstate()
    probe = ProbeNet(bool(int(g["probe_cl"])))
    if int(g["raised"]):
        with pytest.raises(ValueError):
            run(method, g["x"], g["labels"], g["frames"], step, g["labels"] if host else None, probe)
        return
    args, data, tgt, (y, t_out, mix, cut) = run(method, g["x"], g["labels"], g["frames"], step,
                                                g["labels"] if host else None, probe)
    assert random.getstate() == py
    assert np_state_is(g, "np_after")
    assert args.depth == int(g["depth"])
    if not int(g["fired"]):
        assert y is data and t_out is tgt and list(mix) == [] and cut is None
        return
    assert bool(y is data) == bool(int(g["same_object"]))
    if "timemask" in method or "freqmask" in method:
        assert y is data                                        # zeroed in place
    else:
        assert y.data_ptr() != data.data_ptr()
        assert np.array_equal(data.cpu().numpy(), g["x"])      # the input is untouched
    assert np.array_equal(np.asarray(mix, dtype=np.int64), g["mix"])
    assert (-1 if cut is None else cut) == int(g["cut"])
    assert np.array_equal(t_out.cpu().numpy(), g["target_out"])
    got = y.detach().cpu().numpy()
    assert got.shape == g["y"].shape and np.array_equal(got, g["y"])       # bit-exact


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("cl", [False, True], ids=["contiguous", "channels_last"])
def test_latent_blend_forward_and_backward_match_torch(depth, cl):
    torch.manual_seed(depth)
    x = torch.randn(24, 1, 64, 48, device=DEV)
    h0 = ProbeNet(cl)(x, depth=depth, pass_part="first")
    labels = np.arange(24) % 3
    mix = hostprep.shuffle_within_groups(labels, 5 + depth)
    lam32 = np.float32(0.3172)
    h = h0.detach().clone().requires_grad_(True)
    out = augmentations2d.latent_blend(h, mix, lam32)
    assert out.stride() == h.stride()                          # the layout is kept
    href = h0.detach().clone().requires_grad_(True)
    lams = torch.full((24,), float(lam32), device=DEV)
    lo = lams.view((24,) + (1,) * (h0.dim() - 1))
    want = href * lo + href[torch.from_numpy(mix).to(DEV)] * (1 - lo)
    assert torch.equal(out.detach(), want.detach())
    for g in (torch.randn_like(want), torch.randn(want.shape, device=DEV)):   # same / other strides
        h.grad = href.grad = None
        out = augmentations2d.latent_blend(h, mix, lam32)
        out.backward(g)
        want = href * lo + href[torch.from_numpy(mix).to(DEV)] * (1 - lo)
        want.backward(g)
        assert h.grad.shape == href.grad.shape
        assert bool((h.grad == href.grad).all())                # == : signed zeros may differ


def full_batch(B=256, F=128, W=128, seed=41):
    _, frames, labels, _ = synthetic.make_batch(B, 1, 5000, sample_rate=2000, seed=seed)
    fs = synthetic.spec_frames(frames, 148, 5000)
    x = np.random.RandomState(seed).standard_normal((B, 1, F, W)).astype(np.float32)
    x[np.broadcast_to(np.arange(W)[None, None, None, :] >= fs[:, 4][:, None, None, None], x.shape)] = 0
    return x, fs, labels


def torch_restatement(method, plan, x, frames):
    """The reference's formulas (augmentations2d.py:461-617) in torch on the device, from the plan's
    partners / lambda / cut / offsets (those are pinned against the reference on the CPU)."""
    d = torch.from_numpy(x).to(DEV)
    B, C, F, W = d.shape
    if plan.kind in ("timemask2d", "freqmask2d"):
        out = d.clone()
        for b, (r0, r1, c0, c1) in enumerate(plan.zero_rect):
            out[b, :, r0:r1, c0:c1] = 0
        return out
    mix = plan.mix
    if plan.kind == "mixup2d":
        lo = torch.full((B, 1, 1, 1), float(plan.lam32), device=DEV)
        return d * lo + d[torch.from_numpy(mix).to(DEV)] * (1 - lo)
    new = torch.zeros((B, C, F, F), device=DEV)
    off = hostprep.rand_offsets(frames, mix, plan.step) if "(rand)" in method else None
    for i in range(B):
        f1, f2, d1, d2 = frames[i], frames[mix[i]], d[i], d[mix[i]]
        if plan.kind == "cutmix2d":
            c = plan.cut
            last = min(f1[c] + f2[4] - f2[c], F)
            new[i, :, :, 0:f1[c]] = d1[:, :, 0:f1[c]]
            new[i, :, :, f1[c]:last] = d2[:, :, f2[c]:f2[c] + last - f1[c]]
            continue
        dn = d1.clone()
        for k in (1, 3):
            n = min(f1[k + 1] - f1[k], f2[k + 1] - f2[k])
            if off is None:
                dn[:, :, f1[k]:f1[k] + n] = d2[:, :, f2[k]:f2[k] + n]
            elif (f2[k + 1] - f2[k]) - (f1[k + 1] - f1[k]) >= 0:
                dn[:, f1[k]:f1[k + 1]] = d2[:, f2[k] + off[i, k]:f2[k] + off[i, k] + n]
            else:
                dn[:, f1[k] + off[i, k]:f1[k] + off[i, k] + n] = d2[:, f2[k]:f2[k + 1]]
        new[i] = dn
    return new


@pytest.mark.parametrize("method", METHODS)
def test_full_size_against_torch(method):
    x, frames, labels = full_batch()
    step = 9
    np.random.seed(3)
    plan = hostprep.make_plan(method, labels, frames, None, step, 256, 1, is2d=True, n_cols=128, n_freq=128)
    np.random.seed(3)
    probe = ProbeNet(True)
    args, data, tgt, (y, t_out, mix, cut) = run(method, x, labels, frames, step, model=probe)
    assert np.array_equal(np.asarray(mix if len(mix) else [], np.int64).reshape(-1),
                          plan.mix if plan.kind not in ("timemask2d", "freqmask2d") else np.zeros(0, np.int64))
    if plan.kind == "latentmixup2d":
        h = probe(torch.from_numpy(x).to(DEV), depth=plan.depth, pass_part="first")
        lo = torch.full((256,) + (1,) * (h.dim() - 1), float(plan.lam32), device=DEV)
        want = h * lo + h[torch.from_numpy(plan.mix).to(DEV)] * (1 - lo)
        assert args.depth == plan.depth and y.stride() == h.stride()
    else:
        want = torch_restatement(method, plan, x, frames)
    assert y.shape == want.shape and torch.equal(y, want)


@pytest.mark.parametrize("method", METHODS)
def test_empty_batch(method):
    x = np.zeros((0, 1, 32, 32), np.float32)
    np.random.seed(1)
    args, data, tgt, (y, t_out, mix, cut) = run(method, x, np.zeros(0, np.int64), np.zeros((0, 5), np.int64), 3,
                                                model=ProbeNet())
    assert y.shape[0] == 0 and len(mix) == 0
    assert (y is data) == ("mask" in method)


def test_latentmixup_refuses_other_models():
    x, frames, labels = full_batch(8, 32, 32)
    data = torch.from_numpy(x).to(DEV)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(DEV)
    args = Args("latentmixup")
    args.model = "Potes"
    with pytest.raises(NotImplementedError, match="resnet9"):
        augmentations2d.augment(args, data, tgt, torch.from_numpy(frames), None, Step(0), ProbeNet(), DEV, "")


def test_latentmixup_train_step_matches_float64():
    """One train_step of ResNet9-2D with latentmixup (first half -> HIP blend -> second half on the
    HIP path, ClipAdam) against a float64 CPU copy doing first, the blend, second, torch's Adam."""
    B = 8
    x, frames, labels = full_batch(B, seed=43)
    args = TC.resnet2d_args()
    args.method = "latentmixup"
    args.batch_size, args.num_steps = B, 40
    torch.manual_seed(11)
    ref = models2d.ResNet9(2).train()
    net = copy.deepcopy(ref).to(DEV).train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(labels, 2, es=args.num_epochs + 1, device=DEV)
    sc = tm.step_counter_class()
    step = sc.count
    np.random.seed(5)
    plan = hostprep.make_plan("latentmixup", labels, frames, None, step, B, 1, is2d=True, n_cols=128, n_freq=128)
    batch = (torch.from_numpy(x).to(DEV), torch.from_numpy(labels), torch.from_numpy(frames), None, None,
             torch.arange(B))
    np.random.seed(5)
    loss = float(tm.train_step(args, net, batch, DEV, opt, sched, crit, 1, sc))
    assert args.depth == 0                                   # reset behind the second half
    ref = ref.double()
    opt_r = torch.optim.Adam(ref.parameters(), lr=args.lr_max, weight_decay=args.weight_decay)
    sched_r = torch.optim.lr_scheduler.OneCycleLR(opt_r, max_lr=args.lr_max, total_steps=args.num_steps)
    h = ref(torch.from_numpy(x).double(), depth=plan.depth, pass_part="first")
    lam = float(plan.lam32)
    h = h * lam + h[torch.from_numpy(plan.mix)] * (1 - lam)
    out = ref(h, depth=plan.depth, pass_part="second")
    t = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).double()
    loss_r = -(torch.log_softmax(out, 1) * t).sum(1).mean()
    loss_r.backward()
    torch.nn.utils.clip_grad_value_(ref.parameters(), args.grad_clip)
    opt_r.step()
    sched_r.step()
    assert abs(loss - float(loss_r)) <= 1e-4 * max(1.0, abs(float(loss_r))), (loss, float(loss_r))
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        d = (p.detach().cpu().double() - q.detach()).abs()
        assert float((d > 1e-4).double().mean()) <= 0.005 and float(d.max()) <= 1e-3, (k, float(d.max()))
    for (k, v), (_, w) in zip(net.named_buffers(), ref.named_buffers()):
        assert torch.allclose(v.cpu().double(), w.double(), rtol=1e-4, atol=1e-5), k


def _image_dataset(n_rec=8, per=3, seed=0):
    rs = np.random.RandomState(seed)
    ds = {}
    for split, n in (("train", n_rec), ("test", n_rec // 2)):
        d = {"data": [], "label": [], "frames": [], "wav": [], "sig_qual": []}
        for r in range(n):
            wav, label = f"{'abcdef'[r % 6]}{r:04d}", r % 2
            for _ in range(per):
                fr = synthetic.spec_frames(synthetic.make_frames(1, 2.0, rs), 148, 5000)[0]
                img = rs.standard_normal((128, 128)).astype(np.float32) * (1.5 if label else 1.0)
                img[:, fr[4]:] = 0
                d["data"].append(img); d["label"].append(label); d["frames"].append(fr)
                d["wav"].append(wav); d["sig_qual"].append(1)
        ds[split] = d
    return ds


def _spec_args(out_dir, method="latentmixup+0.8"):
    return argparse.Namespace(dataset="PhysioNet(spec128)", model="resnet9", method=method, num_epochs=2,
                              batch_size=8, op="adam", use_sched=True, lr_max=0.002, weight_decay=1e-4,
                              grad_clip=0.1, seed=4, seed_data=1100001, n_fraction=1.0, train_balance=True,
                              num_classes=2, sample_rate=2000, num_channels=1, valid=False, depth=0,
                              EXPERIMENTS=out_dir)


def test_latentmixup_through_train_model(tmp_path):
    """train_model -> train_epoch -> train_step with 2D latentmixup (eager, never graphed)."""
    args = _spec_args(str(tmp_path))
    perf = tm.train_model(args, _image_dataset(), DEV, log=None)
    assert perf["steps"][-1] == args.num_steps == 2 * (24 // 8)
    assert all(np.isfinite(v) for v in perf["train_loss"])
    assert args.depth == 0


def _ddp_rank(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(DEV)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tm.train_model(_spec_args(out_dir), _image_dataset(), DEV, log=None)
        verdict = "ran"
    except NotImplementedError as exc:
        verdict = "refused: " + str(exc)
    with open(os.path.join(out_dir, f"rank{rank}.txt"), "w") as f:
        f.write(verdict)
    dist.barrier()
    dist.destroy_process_group()


def test_latentmixup_is_refused_under_torch_distributed(tmp_path):
    """Two gloo ranks sharing this GPU: train_model() refuses 2D latentmixup at its start (two half
    passes of the DDP-wrapped model per step) with a clear NotImplementedError."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_ddp_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        verdict = (tmp_path / f"rank{r}.txt").read_text()
        assert verdict.startswith("refused") and "latentmixup" in verdict and "distributed" in verdict


def small_batch(B, C, F, W, seed):
    """Random images whose cycles end inside min(F, W) columns (every cut fits)."""
    rs = np.random.RandomState(seed)
    n = min(F, W)
    frames = np.zeros((B, 5), np.int64)
    for b in range(B):
        cuts = np.sort(rs.choice(np.arange(1, n + 1), 4, replace=False))
        frames[b, 1:] = cuts
    x = rs.standard_normal((B, C, F, W)).astype(np.float32)
    labels = rs.randint(0, 2, B).astype(np.int64)
    return x, frames, labels


ODD_SHAPES = [(24, 1, 30, 30), (20, 2, 33, 33), (16, 1, 30, 34), (16, 2, 36, 30)]


@pytest.mark.parametrize("method, shape", [(m, s) for m in METHODS[:-1] for s in ODD_SHAPES
                                           if "durratiocutmix" not in m or s[2] == s[3]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_odd_shapes_against_torch(method, shape):
    """F or W not a multiple of 4: the element-wise kernel instantiations (output width % 4 != 0) and
    the vector ones with an odd input width.  (durratiocutmix needs W == F: the reference refuses
    other shapes, pinned by the goldens.)"""
    B, C, F, W = shape
    x, frames, labels = small_batch(B, C, F, W, seed=F * W)
    step = 4
    np.random.seed(3)
    plan = hostprep.make_plan(method, labels, frames, None, step, B, C, is2d=True, n_cols=W, n_freq=F)
    np.random.seed(3)
    args, data, tgt, (y, t_out, mix, cut) = run(method, x, labels, frames, step)
    want = torch_restatement(method, plan, x, frames)
    assert y.shape == want.shape and torch.equal(y, want)


@pytest.mark.parametrize("axis, F, W, Wo", [(0, 13, 20, 20), (0, 13, 18, 13), (0, 9, 7, 12), (0, 11, 3, 8),
                                            (1, 13, 16, 16), (1, 14, 15, 15)])
def test_piecewise_kernel_on_random_tables(axis, F, W, Wo):
    """Any contiguous table: zero segments between short copies, empty segments, shifts that leave the
    input, an end before the last position — the vector and the element paths."""
    check_random_tables(axis, F, W, Wo, B=12)


def test_piecewise_kernel_output_plane_twice_the_input():
    """Wo = 2 W on the vector path: the output offset of a quad lies outside a sample's input plane,
    and for the last sample outside ``x`` — the load a non-copy quad issues must not use it."""
    check_random_tables(0, 5, 8, 16, B=2)


def check_random_tables(axis, F, W, Wo, B):
    rs = np.random.RandomState(F * 100 + W)
    C = 2
    N = Wo if axis == 0 else F
    x = rs.standard_normal((B, C, F, W)).astype(np.float32)
    mix = rs.permutation(B)
    segs = np.zeros((B, 5, 4), np.int32)
    for b in range(B):
        cuts = np.sort(rs.randint(0, N + 1, 4))
        if b % 3 == 0:                       # short copies between zero segments
            cuts = np.sort(np.array([1, 2, 4, 5]) % (N + 1))
        bounds = np.concatenate([[0], cuts, [N if b % 4 else rs.randint(1, N + 1)]])
        bounds[-1] = max(bounds[-1], bounds[-2])
        segs[b, :, 0], segs[b, :, 1] = bounds[:-1], bounds[1:]
        segs[b, :, 2] = rs.randint(0, 3, 5) if b % 3 else [2, 0, 2, 1, 2]
        segs[b, :, 3] = rs.randint(-N, N + 1, 5) if b % 2 else rs.randint(-2, 3, 5)
    data = torch.from_numpy(x).to(DEV)
    y = augmentations2d.piecewise_rows(data, segs, mix, axis, Wo)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), replay_pieces(x, segs, mix, axis, Wo))
