#!/usr/bin/env python3
"""A/B of two builds of libpcgmix_hip.so on the BatchNorm + ReLU + MaxPool forward: this tree's library
against another build (the parent commit's), ALTERNATING in fresh processes — one library per process,
``--runs`` processes per library, A B A B ...

A process measures, after a warm-up, ``--rounds`` rounds of ``--iters`` back-to-back calls between two
HIP events, and reports its median round:
  eval fwd    pcgmix_bnrp_eval_fwd_f32 at (256, 64, 1, 2500) window (1, 2) and (256, 128, 1, 1250) window
              (1, 1) — one launch of bnrp_fwd_kernel and nothing else, so this is that kernel's time plus
              one launch gap
  train fwd   pcgmix_bnrp_fwd_f32 at the same shapes: bn_stats_kernel, bn_finalize_kernel, bnrp_fwd_kernel
  step        one eager train_step of ResNet9-1D at (256, 4, 2500)
Reported per library: the median over its processes and [min .. max], and for every quantity whether the
difference of the medians lies inside the parent's own run-to-run spread (max - min).

    python profiles/probes/bnrp_ab.py --parent /path/to/parent/libpcgmix_hip.so [--out profiles/bnrp_nan_ab.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
SHAPES = [(256, 64, 1, 2500, 1, 2), (256, 128, 1, 1250, 1, 1)]


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def leg(opts):
    """One process, one library: a JSON line of median microseconds per quantity."""
    import ctypes
    import numpy as np
    import torch
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import _lib, synthetic, train_model as tm
    if opts.leg != "tree":
        _lib.LIB_PATH = os.path.abspath(opts.leg)
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    legs = {}
    for B, C, H, W, ph, pw in SHAPES:
        torch.manual_seed(C)
        y = torch.randn(B, H, W, C, device=dev) * 1.7 + 0.3
        z = torch.empty(B, H // ph, W // pw, C, device=dev)
        g, b, rm = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.3, torch.randn(C, device=dev) * 0.1
        rv, mean, istd = torch.rand(C, device=dev) + 0.5, torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = torch.empty(lib.pcgmix_bnrp_workspace_floats(B, H, W, C), device=dev)
        keep = (y, z, g, b, rm, rv, mean, istd, ws)

        def eval_fwd(k=keep, s=(B, H, W, C, ph, pw)):
            y, z, g, b, rm, rv = k[:6]
            lib.pcgmix_bnrp_eval_fwd_f32(y.data_ptr(), g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                         ctypes.c_float(1e-5), None, None, z.data_ptr(), *s, stream)

        def train_fwd(k=keep, s=(B, H, W, C, ph, pw)):
            y, z, g, b, rm, rv, mean, istd, ws = k
            lib.pcgmix_bnrp_fwd_f32(y.data_ptr(), g.data_ptr(), b.data_ptr(), None, None, ctypes.c_float(0.1),
                                    ctypes.c_float(1e-5), None, None, None, z.data_ptr(), mean.data_ptr(), istd.data_ptr(),
                                    ws.data_ptr(), *s, stream)
        legs[f"eval fwd  ({B},{C},{H},{W}) window ({ph},{pw})"] = (eval_fwd, opts.iters)
        legs[f"train fwd ({B},{C},{H},{W}) window ({ph},{pw})"] = (train_fwd, opts.iters)
    Bt, T = 256, 2500
    x, frames, labels, wav = synthetic.make_batch(Bt, 4, T, seed=3)
    batch = (torch.from_numpy(x).to(dev), torch.from_numpy(labels), torch.from_numpy(frames), wav,
             torch.ones(Bt, dtype=torch.long), torch.arange(Bt))
    args = argparse.Namespace(dataset="PhysioNet", model="resnet9", method="durmixmagwarp(0.2,4)+0.7", num_epochs=2,
                              batch_size=Bt, op="adam", use_sched=True, lr_max=0.01, weight_decay=1e-4, grad_clip=0.1,
                              seed=4, seed_fix=4, num_classes=2, num_channels=4, sig_len=T, depth=0,
                              num_steps=2 * ((opts.rounds + 1) * opts.step_iters + opts.warmup + 8), sample_rate=1000)
    torch.manual_seed(0)
    np.random.seed(1)
    net = tm.build_model(args).to(dev).train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(labels, 2, es=args.num_epochs + 1, device=dev)
    counter = tm.step_counter_class()
    legs[f"train_step resnet9 ({Bt},4,{T})"] = (lambda: tm.train_step(args, net, batch, dev, opt, sched, crit, 1, counter),
                                                opts.step_iters)
    out = {}
    for name, (fn, iters) in legs.items():
        for _ in range(opts.warmup):
            fn()
        torch.cuda.synchronize()
        out[name] = statistics.median(timed(fn, iters) for _ in range(opts.rounds))
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the other build of libpcgmix_hip.so")
    ap.add_argument("--leg", help="(internal) measure this library in this process: a path, or 'tree'")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--what", default="the ReLU and the window maximum keep a NaN")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bnrp_nan_ab.txt"))
    opts = ap.parse_args()
    if opts.leg:
        return leg(opts)
    if not opts.parent:
        raise SystemExit("--parent: the library to compare with")
    got = {"tree": [], "parent": []}
    for _ in range(opts.runs):
        for who, lib in (("parent", opts.parent), ("tree", "tree")):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", lib, "--rounds", str(opts.rounds), "--iters",
                   str(opts.iters), "--step-iters", str(opts.step_iters), "--warmup", str(opts.warmup)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("LEG ")]
            if res.returncode or not line:
                raise SystemExit(f"{who} leg failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            got[who].append(json.loads(line[0][4:]))
            print(who, line[0], flush=True)
    out = [f"# BatchNorm+ReLU+pool forward, this tree ({opts.what}) against its parent commit: {opts.runs} fresh processes per",
           f"# library, alternating parent, tree, parent, ...; a process reports the median of {opts.rounds} rounds of {opts.iters} calls",
           f"# ({opts.step_iters} train steps) between two HIP events.  us per call: median over the processes [min .. max].  'inside':",
           "# |median(tree) - median(parent)| <= max(parent) - min(parent), the parent's own run-to-run spread.",
           "# quantity                                      parent us                         tree us                           tree/parent  inside"]
    for name in got["tree"][0]:
        p, t = [g[name] for g in got["parent"]], [g[name] for g in got["tree"]]
        mp, mt = statistics.median(p), statistics.median(t)
        inside = abs(mt - mp) <= max(p) - min(p)
        out.append(f"  {name:44s}  {mp:9.1f} [{min(p):9.1f} .. {max(p):9.1f}]  {mt:9.1f} [{min(t):9.1f} .. {max(t):9.1f}]"
                   f"  {mt / mp:9.4f}    {'yes' if inside else 'NO'}")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
