#!/usr/bin/env python3
"""The fixed-order HIP weight gradient of Conv1d(k=3, pad=1) (csrc/pcgmix_conv3_wgrad.hip) and the
training route built on it (``models.Conv3TrainFunction``, ``models.FUSED_CONV_TRAIN``) against MIOpen,
in ONE process.

  per layer  the weight gradient at the eight convolutions of 'resnet9' at (256, 4, 2500):
             ``pcgmix_conv3_wgrad_nlc_f32`` against ``aten.convolution_backward`` with
             output_mask = (False, True, False) on channels_last tensors, MIOpen's default selection;
             ms, TFLOP/s and the share of the 157 TFLOP/s f32 matrix peak, and the splits of the plan;
  step       the eager ``train_step`` ('resnet9', durmixmagwarp(0.2,4), ClipAdam) at (256, 4, 2500) with
             the switch on against the switch off (MIOpen's default selection), and ONE timed step of
             MIOpen's deterministic selection — the path a user who needs reproducibility has without
             the switch.  Decision: the HIP step's median must be below that step; its ratio to
             MIOpen's default is reported.

Method: warm-up calls per path (MIOpen's find runs there), then ``--rounds`` rounds with the paths
ALTERNATING inside a round; HIP events around the work of one round (per layer: ``--reps`` launches per
event pair).  Reported: median [min .. max] over the rounds.

    python profiles/conv3_train_time.py [--out profiles/conv3_train_time.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from conv3_time import B, C_IN, LAYERS, PEAK, T, alternate, fmt, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-deterministic", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3_train_time.txt"))
    opts = ap.parse_args()
    import warnings
    import numpy as np
    import torch
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import _lib, models, synthetic, train_model as tm
    if not torch.cuda.is_available():
        raise SystemExit("conv3_train_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    out = [f"# {torch.cuda.get_device_name(0)}; HIP conv3 weight gradient (pcgmix_conv3_wgrad_nlc_f32) against MIOpen",
           "# (aten.convolution_backward, output_mask (False, True, False), channels_last, default algorithm selection),",
           f"# one process, {opts.warmup} warm-up calls per path, then {opts.rounds} rounds with the paths alternating, HIP events.",
           "# ms: median [min .. max].",
           f"# per layer of resnet9 at ({B},{C_IN},{T}), {opts.reps} launches per event pair; TF = TFLOP/s of the HIP call",
           f"# (2*B*L*3*Cin*Cout flop; both launches), % of the {PEAK:.0f} TFLOP/s f32 matrix peak",
           "# layer    Cin Cout    L splits  HIP ms                        MIOpen ms                     HIP TF   % peak"]

    def say(line):
        out.append(line)
        print(line, flush=True)

    tot = {"hip": 0.0, "miopen": 0.0}
    for name, cin, cout, L in LAYERS:
        g = torch.Generator(device="cpu").manual_seed(0)
        w4 = torch.empty(cout, cin, 1, 3, device=dev).contiguous(memory_format=torch.channels_last)
        x = torch.randn(B, cin, 1, L, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, cout, 1, L, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        splits, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
        _lib.check(lib.pcgmix_conv3_wgrad_plan(B, L, cin, cout, ctypes.byref(splits), ctypes.byref(nbytes)), "plan")

        def miopen():
            return torch.ops.aten.convolution_backward(dy, x, w4, None, [1, 1], [0, 1], [1, 1], False, [0, 0], 1,
                                                       [False, True, False])[1]
        got = alternate(torch, {"hip": lambda: models.Conv3TrainFunction._wgrad(x, dy), "miopen": miopen},
                        opts.rounds, opts.warmup, opts.reps)
        a, b = models.Conv3TrainFunction._wgrad(x, dy), miopen()
        rel = float((a - b).norm() / b.norm())
        flop = 2.0 * B * L * 3 * cin * cout
        tf = flop / (statistics.median(got["hip"]) * 1e-3) / 1e12
        say(f"  {name:7s} {cin:4d} {cout:4d} {L:4d} {splits.value:6d}  {fmt(got['hip'])}  {fmt(got['miopen'])}  {tf:6.1f}   {100 * tf / PEAK:5.1f}"
            f"   (HIP against MIOpen, relative L2: {rel:.1e})")
        for k in tot:
            tot[k] += statistics.median(got[k])
        del x, dy, a, b
    say(f"# sum of the 8 medians: HIP {tot['hip']:.3f} ms, MIOpen {tot['miopen']:.3f} ms")

    # the eager training step
    args = argparse.Namespace(
        dataset="PhysioNet", model="resnet9", method="durmixmagwarp(0.2,4)", num_epochs=1, batch_size=B,
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
    say(f"# eager train_step, resnet9 at ({B},{C_IN},{T}), durmixmagwarp(0.2,4), ClipAdam; 1.60 TFLOP of convolutions")
    say(f"  FUSED_CONV_TRAIN = True   {fmt(got['hip'])} ms")
    say(f"  FUSED_CONV_TRAIN = False  {fmt(got['miopen'])} ms   (MIOpen default selection)")
    say(f"  HIP / MIOpen default = {mh / mm:.2f}")
    if not opts.skip_deterministic:
        det = step(False, True)
        det()                                              # its own find
        md = timed(torch, det)
        say(f"  MIOpen deterministic selection, ONE step after one warm-up step: {md:.1f} ms")
        say(f"# decision: HIP median below the MIOpen-deterministic step: {'MET' if mh < md else 'NOT met'}"
            f" ({md / mh:.0f}x)")
    models.FUSED_CONV_TRAIN = None
    assert np.isfinite(float(step(True)()))
    models.FUSED_CONV_TRAIN = None
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
