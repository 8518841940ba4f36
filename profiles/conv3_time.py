#!/usr/bin/env python3
"""The deterministic HIP Conv1d(k=3, pad=1) (csrc/pcgmix_conv3.hip, ``models.Conv3Function``) against
MIOpen (``F.conv2d`` on channels_last tensors, default algorithm selection), in ONE process.

  per layer  forward and input gradient at the eight convolutions of 'resnet9' at (256, 4, 2500):
             ms, TFLOP/s and the share of the 157 TFLOP/s f32 matrix peak;
  (a)        the frozen pass — forward + input gradient of an eval-mode 'resnet9' with frozen
             parameters at (256, 4, 2500) — HIP route (``models.FUSED_CONV = True``) against MIOpen
             default (``False``).  Decision: the HIP route is the default iff its median is at most
             2x the MIOpen-default median;
  (b)        the evaluation call of profiles/eval_time.py ('resnet9', ``test_data_accuracy`` over 8000
             cycles, batch 1000, HIP eval kernels on both sides) with ``models.FUSED_CONV_NOGRAD`` on
             and off.  Decision: ``FUSED_CONV_NOGRAD`` defaults to True iff the HIP median is below
             the MIOpen median of this run.

Method: warm-up calls per path (MIOpen's find runs there), then ``--rounds`` rounds with the two
paths ALTERNATING inside a round; HIP events around the work of one round (per layer: ``--reps``
launches per event pair; (b): one call, which ends in its own device-to-host copy).  Reported: median
[min .. max] over the rounds.

    python profiles/conv3_time.py [--out profiles/conv3_time.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
B, C_IN, T = 256, 4, 2500
PEAK = 157.0                          # TFLOP/s, f32 matrix
# (name, Cin, Cout, L) of resnet9 (filters 64, 128, 256, 512) at T = 2500
LAYERS = [("conv1", 4, 64, 2500), ("conv2", 64, 128, 2500), ("res1.0", 128, 128, 1250),
          ("res1.1", 128, 128, 1250), ("conv3", 128, 256, 1250), ("conv4", 256, 512, 625),
          ("res2.0", 512, 512, 312), ("res2.1", 512, 512, 312)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-eval", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3_time.txt"))
    opts = ap.parse_args()
    import warnings
    import torch
    import torch.nn.functional as F
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import models, train_model as tm
    if not torch.cuda.is_available():
        raise SystemExit("conv3_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda", 0)
    out = [f"# {torch.cuda.get_device_name(0)}; HIP conv3 (pcgmix_conv3_nlc_f32) against MIOpen (F.conv2d, channels_last,",
           f"# default algorithm selection), one process, {opts.warmup} warm-up calls per path, then {opts.rounds} rounds with the two",
           "# paths alternating, HIP events.  ms: median [min .. max].",
           f"# per layer of resnet9 at ({B},{C_IN},{T}), {opts.reps} launches per event pair; TF = TFLOP/s of the HIP kernel",
           f"# (2*B*L*3*Cin*Cout flop), % of the {PEAK:.0f} TFLOP/s f32 matrix peak",
           "# layer    Cin Cout    L  dir   HIP ms                        MIOpen ms                     HIP TF   % peak"]

    def say(line):
        out.append(line)
        print(line, flush=True)

    tot = {"hip": 0.0, "miopen": 0.0}
    for name, cin, cout, L in LAYERS:
        g = torch.Generator(device="cpu").manual_seed(0)
        conv = torch.nn.Conv1d(cin, cout, 3, padding=1)
        w = conv.weight.data.permute(0, 2, 1).contiguous().permute(0, 2, 1).to(dev)   # as ResNet9_myrtle
        w4 = w.unsqueeze(2).requires_grad_(False)
        x = torch.randn(B, cin, 1, L, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, cout, 1, L, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        xg = x.clone(memory_format=torch.channels_last).requires_grad_(True)
        wt = models.Conv3Function._transposed(w4)
        rows = models.Conv3Function._rows(w4)
        flop = 2.0 * B * L * 3 * cin * cout
        with torch.no_grad():
            fwd = alternate(torch, {"hip": lambda: models.Conv3Function._launch(x, rows, cout),
                                    "miopen": lambda: F.conv2d(x, w4, None, padding=(0, 1))},
                            opts.rounds, opts.warmup, opts.reps)
        ym = F.conv2d(xg, w4, None, padding=(0, 1))
        bwd = alternate(torch, {"hip": lambda: models.Conv3Function._launch(dy, wt, cin),
                                "miopen": lambda: torch.autograd.grad(ym, xg, dy, retain_graph=True)},
                        opts.rounds, opts.warmup, opts.reps)
        for d, got in (("fwd", fwd), ("dx", bwd)):
            mh = statistics.median(got["hip"])
            tf = flop / (mh * 1e-3) / 1e12
            say(f"  {name:7s} {cin:4d} {cout:4d} {L:4d}  {d:3s}  {fmt(got['hip'])}  {fmt(got['miopen'])}  {tf:6.1f}   {100 * tf / PEAK:5.1f}")
            for k in tot:
                tot[k] += statistics.median(got[k])
        del ym, xg, x, dy
    say(f"# sum of the 16 medians: HIP {tot['hip']:.3f} ms, MIOpen {tot['miopen']:.3f} ms")

    # (a) the frozen pass
    args = argparse.Namespace(dataset="PhysioNet", model="resnet9", method="base", num_classes=2,
                              num_channels=C_IN, sig_len=T)
    torch.manual_seed(0)
    model = tm.build_model(args).to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    data = torch.randn(B, C_IN, T, device=dev)
    seed = torch.zeros(B, 2, device=dev)
    seed[:, 0] = 1

    def frozen(fused):
        def run():
            models.FUSED_CONV = fused
            xin = data.detach().requires_grad_(True)
            with torch.enable_grad():
                (grad,) = torch.autograd.grad(model(xin), xin, seed)
            return grad
        return run
    got = alternate(torch, {"hip": frozen(True), "miopen": frozen(False)}, opts.rounds, opts.warmup)
    models.FUSED_CONV = True
    g1, g2 = frozen(True)(), frozen(True)()
    same = bool(torch.equal(g1, g2))
    mh, mm = statistics.median(got["hip"]), statistics.median(got["miopen"])
    say(f"# (a) frozen pass, resnet9 at ({B},{C_IN},{T}), forward + input gradient, 1.07 TFLOP of convolutions")
    say(f"  HIP route      {fmt(got['hip'])} ms   ({1.07 / (mh * 1e-3):.1f} TFLOP/s over the whole pass)")
    say(f"  MIOpen default {fmt(got['miopen'])} ms")
    say(f"  HIP / MIOpen = {mh / mm:.2f}; two HIP passes bit-identical: {'yes' if same else 'NO'}")
    say(f"# decision (a): HIP median <= 2 x MIOpen-default median: {'MET - the HIP route is the default' if mh <= 2 * mm else 'NOT met - the HIP route is opt-in'}")

    # (b) the evaluation call
    if not opts.skip_eval:
        import eval_time
        loader = eval_time.make_loader(dev)
        call = eval_time.make_call("resnet9", loader, dev)

        def ev(nograd):
            def run():
                models.FUSED_CONV_NOGRAD = nograd
                return call(True)
            return run
        got = alternate(torch, {"hip": ev(True), "miopen": ev(False)}, opts.rounds, opts.warmup)
        mh, mm = statistics.median(got["hip"]), statistics.median(got["miopen"])
        say(f"# (b) evaluation call, resnet9, {eval_time.N} cycles of ({C_IN},{T}), batch {eval_time.BATCH}, HIP eval kernels on both sides")
        say(f"  FUSED_CONV_NOGRAD = True   {fmt(got['hip'])} ms")
        say(f"  FUSED_CONV_NOGRAD = False  {fmt(got['miopen'])} ms")
        say(f"# decision (b): HIP median below MIOpen median: {'MET - FUSED_CONV_NOGRAD defaults to True' if mh < mm else 'NOT met - FUSED_CONV_NOGRAD defaults to False'}")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
