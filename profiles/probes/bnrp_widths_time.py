#!/usr/bin/env python3
"""BatchNorm + ReLU + MaxPool of the ResNet9 blocks at the ladder widths the kernels did not take
before (C = 2, 96, 192, 384, 768) and in eval mode: the HIP path (``models.FUSED_BN = True``)
against the torch-op path (``models.FUSED_BN = False`` — for these cases exactly the code that ran
before the kernels covered them), in ONE process.

  block       forward + backward of one ``conv_bn_relu_pool`` block (a k=3 convolution from 4
              channels, BatchNorm in training mode, ReLU, the layer's pooling) at (256, C, 1, L), L
              the length that layer sees for T = 2500; the convolution is the same on both paths
  step        the eager ``train_step`` of resnet9-1.4m and resnet9-5m at (256, 4, 2500)
  eval fwd    the eval-mode forward under ``no_grad`` (default ResNet9-1D and resnet9-5m)
  frozen      forward + input gradient of the frozen model, as the saliency pass runs it
              (``saliency.input_gradient_seeded``, MIOpen's default algorithms): the default
              ResNet9-1D at (256, 4, 2500) and ResNet9-2D at (256, 1, 128, 128)

Method: every quantity is warmed up on both paths first (code objects, MIOpen's algorithm search);
then ``--rounds`` rounds, the two paths ALTERNATING inside a round, each timing ``--iters``
back-to-back calls between two HIP events on the current stream; the figure of a round is the event
time over ``--iters``.  Reported: median, min and max over the rounds, in microseconds.  The event
window holds the launches' gaps as well as the kernels: it is a call time, not a kernel time.  The
host is shared with other jobs: read the spread next to every median.

Last, the distance of the default-algorithm ResNet9-2D saliency maps to the reference's recorded
ones (tests/golden/salopt2d_*.npz, the figure test_salopt2d_augment_end_to_end reports) on both
paths.  It is reported, not judged: MIOpen's default selection moves it from box to box.

    python profiles/probes/bnrp_widths_time.py [--out profiles/bnrp_widths_time.txt]
"""
import argparse
import glob
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
B = 256
# C, L, pooling: conv1 of resnet9-5k and -5m, conv2 / conv3 / conv4 of resnet9-5m
BLOCKS = [(2, 2500, None), (96, 2500, None), (192, 2500, (1, 2)), (384, 1250, (1, 2)), (768, 625, (1, 2))]


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def on_path(fn, fused):
    """fn with models.FUSED_BN set for the call."""
    from pcgmix_amd import models

    def run():
        models.FUSED_BN = fused
        try:
            return fn()
        finally:
            models.FUSED_BN = True
    return run


def alternate(fn, opts, iters):
    import torch
    legs = {"hip": on_path(fn, True), "torch": on_path(fn, False)}
    for leg in legs.values():
        for _ in range(opts.warmup):
            leg()
    torch.cuda.synchronize()
    got = {k: [] for k in legs}
    for _ in range(opts.rounds):
        for k, leg in legs.items():
            got[k].append(timed(leg, iters))
    return got


def block_leg(C, L, pool, dev):
    import torch
    from pcgmix_amd import models
    torch.manual_seed(C)
    conv = torch.nn.Conv2d(4, C, (1, 3), padding=(0, 1)).to(dev).to(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    x = torch.randn(B, 4, 1, L, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        shape = models.conv_bn_relu_pool(x, conv.weight, conv.bias, (0, 1), bn, True, pool).shape
    dz = torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last)
    params = [conv.weight, conv.bias, bn.weight, bn.bias]

    def run():
        for p in params:
            p.grad = None
        models.conv_bn_relu_pool(x, conv.weight, conv.bias, (0, 1), bn, True, pool).backward(dz)
    return run


def step_leg(name, dev, n_steps):
    """One eager train step; each path trains its own copy of the model."""
    import numpy as np
    import torch
    from pcgmix_amd import models, synthetic, train_model as tm
    T = 2500
    x, frames, labels, wav = synthetic.make_batch(B, 4, T, seed=3)
    batch = (torch.from_numpy(x).to(dev), torch.from_numpy(labels), torch.from_numpy(frames), wav,
             torch.ones(B, dtype=torch.long), torch.arange(B))
    state = {}
    for fused in (True, False):
        args = argparse.Namespace(dataset="PhysioNet", model=name, method="durmixmagwarp(0.2,4)+0.7",
                                  num_epochs=2, batch_size=B, op="adam", use_sched=True, lr_max=0.01,
                                  weight_decay=1e-4, grad_clip=0.1, seed=4, seed_fix=4, num_classes=2,
                                  num_channels=4, sig_len=T, depth=0, num_steps=n_steps, sample_rate=1000)
        torch.manual_seed(0)
        net = tm.build_model(args).to(dev).train()
        opt, sched = tm.make_optimizer(args, net)
        crit = tm.SELCLoss(labels, 2, es=args.num_epochs + 1, device=dev)
        state[fused] = (args, net, opt, sched, crit, tm.step_counter_class())
    np.random.seed(1)

    def run():
        a, n, o, s, c, k = state[models.FUSED_BN]
        tm.train_step(a, n, batch, dev, o, s, c, 1, k)
    return run


def frozen(model, dev):
    model = model.to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def eval_leg(model, x):
    import torch

    def run():
        with torch.no_grad():
            return model(x)
    return run


def frozen_leg(model, x, classes=2):
    import torch
    from pcgmix_amd import saliency
    seed = torch.zeros(x.shape[0], classes, device=x.device)
    seed[:, 0] = 1
    return lambda: saliency.input_gradient_seeded(model, x, seed)


def golden_distance(dev):
    """max |saliency map - reference's recorded map| over the 2D goldens, MIOpen's default algorithms."""
    import numpy as np
    import torch
    from pcgmix_amd import models, models2d, saliency
    torch.manual_seed(4321)                      # the goldens' frozen model (make_golden_salopt2d.py)
    model = frozen(models2d.ResNet9(num_classes=2), dev)
    out = {}
    for fused in (False, True):
        models.FUSED_BN = fused
        worst = 0.0
        for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "salopt2d_*.npz"))):
            g = np.load(path)
            data = torch.from_numpy(g["x"]).to(dev)
            tgt = torch.nn.functional.one_hot(torch.from_numpy(g["labels"]), 2).to(dev)
            sal = saliency.get_saliency_maps(None, dev, data, tgt, torch.from_numpy(g["frames"]), dim=2,
                                             model_sal=model)
            worst = max(worst, float(np.abs(sal.cpu().numpy() - g["sal"]).max()))
        out[fused] = worst
    models.FUSED_BN = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bnrp_widths_time.txt"))
    opts = ap.parse_args()
    import warnings
    import torch
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import models, models2d, train_model as tm
    if not torch.cuda.is_available():
        raise SystemExit("bnrp_widths_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)         # the torch-op path announces itself
    dev = torch.device("cuda", 0)
    out = [f"# {torch.cuda.get_device_name(0)}; ResNet9 BatchNorm+ReLU+pool at the new ladder widths and in eval mode: HIP kernels",
           "# (FUSED_BN = True) against torch ops (FUSED_BN = False: the path these cases took before), one process, both",
           f"# paths warmed up, then {opts.rounds} rounds with the two paths alternating; a round = {opts.iters} calls ({opts.step_iters} train steps)",
           "# between two HIP events.  us per call: median [min .. max] over the rounds.  The host is shared: compare",
           "# medians with the spread in mind.  Call times (launch gaps included), not kernel times.",
           "# quantity                                  hip us                          torch us                        torch/hip  hip < torch"]
    worse = []

    def report(label, got):
        h, t = got["hip"], got["torch"]
        mh, mt = statistics.median(h), statistics.median(t)
        if not mh < mt:
            worse.append(label)
        line = (f"  {label:40s}  {mh:9.1f} [{min(h):9.1f} .. {max(h):9.1f}]  {mt:9.1f} [{min(t):9.1f} .. {max(t):9.1f}]"
                f"  {mt / mh:7.2f}x   {'yes' if mh < mt else 'NO'}")
        out.append(line)
        print(line, flush=True)

    for C, L, pool in BLOCKS:
        report(f"block fwd+bwd ({B},{C},1,{L}) pool {pool[1] if pool else 1}",
               alternate(block_leg(C, L, pool, dev), opts, opts.iters))
        torch.cuda.empty_cache()
    n_steps = 2 * ((opts.rounds + 1) * opts.step_iters + opts.warmup + 8)
    for name in ("resnet9-1.4m", "resnet9-5m"):
        report(f"train_step {name} ({B},4,2500)", alternate(step_leg(name, dev, n_steps), opts, opts.step_iters))
        torch.cuda.empty_cache()
    x1 = torch.randn(B, 4, 2500, device=dev)
    x2 = torch.randn(B, 1, 128, 128, device=dev)
    torch.manual_seed(0)
    default1d = frozen(models.ResNet9(4, 2), dev)
    big1d = frozen(tm.build_model(argparse.Namespace(dataset="PhysioNet", model="resnet9-5m", num_classes=2,
                                                     num_channels=4, sig_len=2500)), dev)
    net2d = frozen(models2d.ResNet9(num_classes=2), dev)
    report(f"eval fwd resnet9 ({B},4,2500)", alternate(eval_leg(default1d, x1), opts, opts.iters))
    report(f"eval fwd resnet9-5m ({B},4,2500)", alternate(eval_leg(big1d, x1), opts, opts.iters))
    report(f"frozen pass resnet9 ({B},4,2500)", alternate(frozen_leg(default1d, x1), opts, opts.iters))
    report(f"frozen pass resnet9-2D ({B},1,128,128)", alternate(frozen_leg(net2d, x2), opts, opts.iters))
    out.append("# acceptance (hip median below torch median for every quantity): " +
               ("met" if not worse else "NOT met for " + "; ".join(worse)))
    d = golden_distance(dev)
    out.append("# ResNet9-2D saliency maps against the reference's recorded ones (tests/golden/salopt2d_*.npz), MIOpen's default")
    out.append(f"# algorithms, max |map - reference|: torch ops {d[False]:.2e}, HIP kernels {d[True]:.2e}  (reported, not judged)")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
