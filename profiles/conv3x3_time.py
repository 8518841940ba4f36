#!/usr/bin/env python3
"""The deterministic HIP Conv2d(3x3, pad=1) (csrc/pcgmix_conv3x3.hip, ``models.Conv3x3Function``)
against MIOpen (``F.conv2d`` on channels_last tensors), the two routes ALTERNATING in one process.

  layers  forward and input gradient at the eight convolutions of ResNet9-2D at (256, 1, 128, 128):
          ms, TFLOP/s and the share of the 157.3 TFLOP/s f32 matrix peak; for the two narrow kernels
          (1 -> 64 forward, 64 -> 1 input gradient) GB/s and the share of 8 TB/s;
  pass    (a) the frozen pass — forward + input gradient of an eval-mode ResNet9-2D with frozen
          parameters — HIP route (``models.FUSED_CONV2D = True``) against MIOpen's default selection
          (``False``: the path before the kernel existed).  Decision: ``FUSED_CONV2D`` defaults to
          True iff the HIP median is at most 2x the MIOpen-default median;
          (b) the evaluation forward under ``no_grad`` with ``models.FUSED_CONV2D_NOGRAD`` on and off.
          Decision: it defaults to True iff the HIP median is below the MIOpen median;
  det     the frozen pass once on MIOpen's deterministic selection
          (``saliency.DETERMINISTIC_FROZEN_PASS = True``), the parity mode the kernel replaces.

Method: warm-up calls per path (MIOpen's find runs there), then ``--rounds`` rounds with the two
paths alternating inside a round; HIP events around the work of one round (per layer: ``--reps``
launches per event pair).  Reported: median [min .. max] over the rounds.  Without ``--step`` the
script starts one child process per step, each under its own ``timeout``, stops at the first that
fails, and joins their reports.

    python profiles/conv3x3_time.py [--out profiles/conv3x3_time.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SIDE = 256, 128
PEAK, HBM = 157.3, 8000.0             # TFLOP/s f32 matrix; GB/s
# (name, Cin, Cout, H = W) of models2d.ResNet9 at 128 x 128
LAYERS = [("conv1", 1, 64, 128), ("conv2", 64, 128, 128), ("res1.0", 128, 128, 64), ("res1.1", 128, 128, 64),
          ("conv3", 128, 256, 64), ("conv4", 256, 512, 32), ("res2.0", 512, 512, 16), ("res2.1", 512, 512, 16)]
CONV_TFLOP = 2.0 * B * 9 * sum(ci * co * s * s for _, ci, co, s in LAYERS) * 2 / 1e12     # forward + input gradient
STEPS = (("layers", 300), ("pass", 300), ("det", 300))                                      # (step, its time limit in s)


def fmt(v):
    return f"{statistics.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]"


def timed(torch, fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(torch, paths, rounds, warmup, reps=1):
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    got = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            got[k].append(timed(torch, fn, reps))
    return got


def step_layers(opts, torch, models, say):
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    say(f"# per layer of ResNet9-2D at ({B},1,{SIDE},{SIDE}), {opts.reps} launches per event pair; rate of the HIP kernel:")
    say(f"# TF = TFLOP/s (2*B*H*W*9*Cin*Cout flop), % of the {PEAK} TFLOP/s f32 matrix peak; the two narrow kernels (*):")
    say(f"# GB/s over x + y, % of {HBM / 1000:.0f} TB/s")
    say("# layer    Cin Cout  H=W  dir   HIP ms                        MIOpen ms                     HIP rate  % peak")
    tot = {"hip": 0.0, "miopen": 0.0}
    for name, cin, cout, s in LAYERS:
        g = torch.Generator(device="cpu").manual_seed(0)
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(memory_format=torch.channels_last)
        w4 = conv.weight.data.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(False)
        x = torch.randn(B, cin, s, s, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, cout, s, s, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        xg = x.clone(memory_format=torch.channels_last).requires_grad_(True)
        wt = models.Conv3x3Function._transposed(w4)
        rows = models.Conv3x3Function._rows(w4)
        flop = 2.0 * B * s * s * 9 * cin * cout
        nbytes = 4.0 * B * s * s * (cin + cout)
        with torch.no_grad():
            fwd = alternate(torch, {"hip": lambda: models.Conv3x3Function._launch(x, rows, cout),
                                    "miopen": lambda: F.conv2d(x, w4, None, padding=1)},
                            opts.rounds, opts.warmup, opts.reps)
        ym = F.conv2d(xg, w4, None, padding=1)
        bwd = alternate(torch, {"hip": lambda: models.Conv3x3Function._launch(dy, wt, cin),
                                "miopen": lambda: torch.autograd.grad(ym, xg, dy, retain_graph=True)},
                        opts.rounds, opts.warmup, opts.reps)
        for d, got in (("fwd", fwd), ("dx", bwd)):
            mh = statistics.median(got["hip"])
            if cin == 1:                       # memory-bound in both directions
                gbs = nbytes / (mh * 1e-3) / 1e9
                rate = f"{gbs:6.0f}*  {100 * gbs / HBM:5.1f}"
            else:
                tf = flop / (mh * 1e-3) / 1e12
                rate = f"{tf:6.1f}   {100 * tf / PEAK:5.1f}"
            say(f"  {name:7s} {cin:4d} {cout:4d} {s:4d}  {d:3s}  {fmt(got['hip'])}  {fmt(got['miopen'])}  {rate}")
            for k in tot:
                tot[k] += statistics.median(got[k])
        del ym, xg, x, dy
    say(f"# sum of the 16 medians: HIP {tot['hip']:.3f} ms, MIOpen {tot['miopen']:.3f} ms")


def _frozen_model(torch, models2d):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = models2d.ResNet9(num_classes=2).to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    data = torch.randn(B, 1, SIDE, SIDE, device=dev)
    seed = torch.zeros(B, 2, device=dev)
    seed[:, 0] = 1
    return model, data, seed


def step_pass(opts, torch, models, say):
    from pcgmix_amd import models2d, saliency
    model, data, seed = _frozen_model(torch, models2d)
    saliency.DETERMINISTIC_FROZEN_PASS = False

    def frozen(fused):
        def run():
            models.FUSED_CONV2D = fused
            return saliency.input_gradient_seeded(model, data, seed)
        return run
    got = alternate(torch, {"hip": frozen(True), "miopen": frozen(False)}, opts.rounds, opts.warmup)
    g1, g2 = frozen(True)(), frozen(True)()
    same = bool(torch.equal(g1, g2))
    m1, m2 = frozen(False)(), frozen(False)()
    same_m = bool(torch.equal(m1, m2))
    mh, mm = statistics.median(got["hip"]), statistics.median(got["miopen"])
    say(f"# (a) frozen pass, ResNet9-2D at ({B},1,{SIDE},{SIDE}), forward + input gradient, {CONV_TFLOP:.2f} TFLOP of convolutions")
    say(f"  HIP route      {fmt(got['hip'])} ms   ({CONV_TFLOP / (mh * 1e-3):.1f} TFLOP/s over the whole pass)")
    say(f"  MIOpen default {fmt(got['miopen'])} ms")
    say(f"  HIP / MIOpen = {mh / mm:.2f}; two HIP passes bit-identical: {'yes' if same else 'NO'}; two MIOpen-default passes: {'yes' if same_m else 'no'}")
    say(f"# decision (a): HIP median <= 2 x MIOpen-default median: {'MET - FUSED_CONV2D defaults to True' if mh <= 2 * mm else 'NOT met - FUSED_CONV2D defaults to False'}")

    def ev(nograd):
        def run():
            models.FUSED_CONV2D_NOGRAD = nograd
            with torch.no_grad():
                return model(data)
        return run
    got = alternate(torch, {"hip": ev(True), "miopen": ev(False)}, opts.rounds, opts.warmup)
    mh, mm = statistics.median(got["hip"]), statistics.median(got["miopen"])
    say(f"# (b) evaluation forward under no_grad, ResNet9-2D at ({B},1,{SIDE},{SIDE}), HIP BatchNorm kernels on both sides")
    say(f"  FUSED_CONV2D_NOGRAD = True   {fmt(got['hip'])} ms")
    say(f"  FUSED_CONV2D_NOGRAD = False  {fmt(got['miopen'])} ms")
    say(f"# decision (b): HIP median below MIOpen median: {'MET - FUSED_CONV2D_NOGRAD defaults to True' if mh < mm else 'NOT met - FUSED_CONV2D_NOGRAD defaults to False'}")


def step_det(opts, torch, models, say):
    from pcgmix_amd import models2d, saliency
    model, data, seed = _frozen_model(torch, models2d)
    models.FUSED_CONV2D = False
    saliency.DETERMINISTIC_FROZEN_PASS = True
    saliency.input_gradient_seeded(model, data, seed)                     # MIOpen's find
    t = timed(torch, lambda: saliency.input_gradient_seeded(model, data, seed))
    models.FUSED_CONV2D = True
    saliency.DETERMINISTIC_FROZEN_PASS = False
    saliency.input_gradient_seeded(model, data, seed)
    h = timed(torch, lambda: saliency.input_gradient_seeded(model, data, seed))
    say(f"# (c) the same frozen pass once on MIOpen's deterministic selection: {t:.1f} ms; the HIP route right after it: "
        f"{h:.1f} ms ({t / h:.1f}x)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3x3_time.txt"))
    opts = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    if opts.step is None:
        # one fresh process per step, each under its own time limit; nothing after a step that failed
        parts = []
        for step, limit in STEPS:
            part = f"{opts.out}.{step}"
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                                 "--step", step, "--out", part, "--rounds", str(opts.rounds),
                                 "--warmup", str(opts.warmup), "--reps", str(opts.reps)]).returncode
            if rc != 0:
                raise SystemExit(f"conv3x3_time.py: step {step} ended with status {rc}; nothing further was run")
            parts.append(part)
        with open(opts.out, "w") as fh:
            for part in parts:
                with open(part) as src:
                    fh.write(src.read())
                os.remove(part)
        return
    import warnings
    import torch
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import models
    if not torch.cuda.is_available():
        raise SystemExit("conv3x3_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    models.FUSED_CONV = True
    out = []

    def say(line):
        out.append(line)
        print(line, flush=True)
    if opts.step == "layers":
        say(f"# {torch.cuda.get_device_name(0)}; HIP conv3x3 (pcgmix_conv3x3_nhwc_f32) against MIOpen (F.conv2d, channels_last,")
        say(f"# default algorithm selection), {opts.warmup} warm-up calls per path, then {opts.rounds} rounds with the two")
        say("# paths alternating, HIP events.  ms: median [min .. max].")
    {"layers": step_layers, "pass": step_pass, "det": step_det}[opts.step](opts, torch, models, say)
    with open(opts.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
