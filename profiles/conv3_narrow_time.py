#!/usr/bin/env python3
"""The narrow fixed-order Conv1d(k=3, pad=1) kernels (csrc/pcgmix_conv3_narrow.hip,
``models.FUSED_CONV_NARROW``) against MIOpen at the 2- and 8-channel layers of 'resnet9-5k',
'resnet9-15k' and 'resnet9-50k', in ONE process at (256, 4, 2500).

  per launch  every forward, input-gradient and weight-gradient call of the three models that goes to the
              narrow kernels, against MIOpen's default selection on channels_last tensors (``F.conv2d``,
              ``torch.autograd.grad`` through it, ``aten.convolution_backward`` with output_mask
              (False, True, False)).  ``--reps`` calls of one path are captured into a graph and one
              replay is timed, so the figure is device time, not the host's launch rate (a call is a
              few microseconds).  GB/s on the 4 (Cin + Cout) B L bytes the layer needs, and its share of
              8 TB/s;
  step        the eager ``train_step`` (durmixmagwarp(0.2,4), ClipAdam) of the three models with
              ``FUSED_CONV_TRAIN = True`` (every convolution on the project's kernels) against the switch
              off (MIOpen's default selection), and ONE timed step of MIOpen's deterministic selection;
  eval        the evaluation forward (eval mode, ``torch.no_grad()``, frozen route) of the three models
              with ``FUSED_CONV_NARROW`` on and off.

Method: warm-up calls per path (MIOpen's find runs there), then ``--rounds`` rounds with the paths
ALTERNATING inside a round; HIP events around the work of one round.  Reported: median [min .. max].
Nothing is decided here: the defaults stay as they are.

    python profiles/conv3_narrow_time.py [--out profiles/conv3_narrow_time.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from conv3_time import B, C_IN, T, alternate, fmt, timed  # noqa: E402

HBM = 8.0e12                          # bytes/s
MODELS = ("resnet9-5k", "resnet9-15k", "resnet9-50k")


def layers(filters):
    """(name, Cin, Cout, L, wants an input gradient) of the eight convolutions at T = 2500."""
    f0, f1, f2, f3 = filters
    return [("conv1", C_IN, f0, T, False), ("conv2", f0, f1, T, True), ("res1.0", f1, f1, T // 2, True),
            ("res1.1", f1, f1, T // 2, True), ("conv3", f1, f2, T // 2, True), ("conv4", f2, f3, T // 4, True),
            ("res2.0", f3, f3, T // 8, True), ("res2.1", f3, f3, T // 8, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-deterministic", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3_narrow_time.txt"))
    opts = ap.parse_args()
    import warnings
    import numpy as np
    import torch
    import torch.nn.functional as F
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import _lib, models, synthetic, train_model as tm
    if not torch.cuda.is_available():
        raise SystemExit("conv3_narrow_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    out = [f"# {torch.cuda.get_device_name(0)}; narrow HIP conv3 (pcgmix_conv3_narrow_nlc_f32, pcgmix_conv3_narrow_wgrad_nlc_f32)",
           "# against MIOpen (channels_last, default algorithm selection), one process,",
           f"# {opts.warmup} warm-up calls per path, then {opts.rounds} rounds with the paths alternating, HIP events.",
           "# ms: median [min .. max].",
           f"# per launch at B = {B}: {opts.reps} calls of one path captured into a graph, one replay per event pair (device time);",
           "# GB/s of the HIP call on 4*(Cin+Cout)*B*L bytes, % of 8 TB/s.  Cin, Cout: the layer's; dx is the kernel call (Cout, Cin)",
           "# dir    Cin Cout    L  HIP ms                        MIOpen ms                     HIP GB/s  % HBM  HIP/MIOpen  models"]

    def say(line):
        out.append(line)
        print(line, flush=True)

    # every narrow launch of the three models, once per (direction, Cin, Cout, L)
    work = {}
    for name in MODELS:
        for lname, cin, cout, L, want_dx in layers(tm.RESNET9_LADDER[name]):
            calls = [("fwd", cin, cout), ("wgrad", cin, cout)] + ([("dx", cout, cin)] if want_dx else [])
            for d, a, b in calls:
                if lib.pcgmix_conv3_narrow_supported(a, b):
                    work.setdefault((d, cin, cout, L), []).append(f"{name[8:]}:{lname}")

    def graphed(fn):
        """``opts.reps`` calls of fn as one captured graph; returns its replay."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(opts.reps):
                fn()
        return g.replay

    models.FUSED_CONV_NARROW = True
    order = {"fwd": 0, "dx": 1, "wgrad": 2}
    for (d, cin, cout, L), users in sorted(work.items(), key=lambda kv: (order[kv[0][0]],) + kv[0][1:]):
        g = torch.Generator(device="cpu").manual_seed(0)
        conv = torch.nn.Conv1d(cin, cout, 3, padding=1)
        w = conv.weight.data.permute(0, 2, 1).contiguous().permute(0, 2, 1).to(dev)   # as ResNet9_myrtle
        w4 = w.unsqueeze(2).requires_grad_(False)
        x = torch.randn(B, cin, 1, L, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, cout, 1, L, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        if d == "fwd":
            rows = models.Conv3Function._rows(w4)
            with torch.no_grad():
                paths = {"hip": graphed(lambda: models.Conv3Function._launch(x, rows, cout)),
                         "miopen": graphed(lambda: F.conv2d(x, w4, None, padding=(0, 1)))}
        elif d == "dx":
            wt = models.Conv3Function._flip(w4)
            paths = {"hip": graphed(lambda: models.Conv3Function._launch(dy, wt, cin)),
                     "miopen": graphed(lambda: torch.ops.aten.convolution_backward(
                         dy, x, w4, None, [1, 1], [0, 1], [1, 1], False, [0, 0], 1, [True, False, False])[0])}
        else:
            paths = {"hip": graphed(lambda: models.Conv3TrainFunction._wgrad(x, dy)),
                     "miopen": graphed(lambda: torch.ops.aten.convolution_backward(
                         dy, x, w4, None, [1, 1], [0, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1])}
        got = alternate(torch, paths, opts.rounds, opts.warmup)
        got = {k: [t / opts.reps for t in v] for k, v in got.items()}
        mh, mm = statistics.median(got["hip"]), statistics.median(got["miopen"])
        rate = 4.0 * (cin + cout) * B * L / (mh * 1e-3)
        say(f"  {d:5s} {cin:4d} {cout:4d} {L:4d}  {fmt(got['hip'])}  {fmt(got['miopen'])}  {rate / 1e9:8.0f}  {100 * rate / HBM:5.1f}"
            f"  {mh / mm:10.2f}  {' '.join(users)}")
        del paths, x, dy
    models.FUSED_CONV_NARROW = None

    # the eager training step and the evaluation forward of the three models
    for name in MODELS:
        args = argparse.Namespace(
            dataset="PhysioNet", model=name, method="durmixmagwarp(0.2,4)", num_epochs=1, batch_size=B,
            op="adam", use_sched=True, lr_max=1e-4, weight_decay=1e-4, grad_clip=0.1, seed=4, seed_fix=4,
            num_classes=2, num_channels=C_IN, sample_rate=1000, depth=0, sig_len=T, num_steps=1000,
            latent_space=False, classical_space=False)
        torch.manual_seed(0)
        net = tm.build_model(args).to(dev).train()
        opt, sched = tm.make_optimizer(args, net)
        xb, frames, labels, wav = synthetic.make_batch(B, C_IN, T, sample_rate=1000, seed=11)
        crit = tm.SELCLoss(labels, 2, es=args.num_epochs + 1, device=dev)
        sc = tm.step_counter_class()
        batch = (torch.from_numpy(xb).to(dev), torch.from_numpy(labels), torch.from_numpy(frames), wav,
                 torch.ones(B, dtype=torch.long), torch.arange(B))

        def step(switch, deterministic=False):
            def run():
                models.FUSED_CONV_TRAIN = switch
                with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=deterministic):
                    return tm.train_step(args, net, batch, dev, opt, sched, crit, 1, sc)
            return run
        got = alternate(torch, {"hip": step(True), "miopen": step(False)}, opts.rounds, opts.warmup)
        mh, mm = statistics.median(got["hip"]), statistics.median(got["miopen"])
        say(f"# eager train_step, {name} at ({B},{C_IN},{T}), durmixmagwarp(0.2,4), ClipAdam")
        say(f"  FUSED_CONV_TRAIN = True   {fmt(got['hip'])} ms   (all 8 convolutions on the HIP kernels)")
        say(f"  FUSED_CONV_TRAIN = False  {fmt(got['miopen'])} ms   (MIOpen default selection)")
        say(f"  HIP / MIOpen default = {mh / mm:.2f}")
        if not opts.skip_deterministic:
            det = step(False, True)
            det()                                              # its own find
            md = timed(torch, det)
            say(f"  MIOpen deterministic selection, ONE step after one warm-up step: {md:.1f} ms   (HIP / it = {mh / md:.2f})")
        models.FUSED_CONV_TRAIN = None
        assert np.isfinite(float(step(True)()))
        models.FUSED_CONV_TRAIN = None

        net.eval()
        data = torch.from_numpy(xb).to(dev)

        def ev(narrow):
            def run():
                models.FUSED_CONV_NARROW = narrow
                with torch.no_grad():
                    return net(data)
            return run
        got = alternate(torch, {"hip": ev(True), "miopen": ev(False)}, opts.rounds, opts.warmup)
        mh, mm = statistics.median(got["hip"]), statistics.median(got["miopen"])
        say(f"# evaluation forward, {name}, eval mode under no_grad at ({B},{C_IN},{T})")
        say(f"  FUSED_CONV_NARROW = True   {fmt(got['hip'])} ms")
        say(f"  FUSED_CONV_NARROW = False  {fmt(got['miopen'])} ms   (MIOpen at the narrow widths)")
        say(f"  narrow / MIOpen = {mh / mm:.2f}")
        models.FUSED_CONV_NARROW = None
        del net, opt, sched, crit
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
