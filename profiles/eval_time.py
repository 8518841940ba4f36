#!/usr/bin/env python3
"""Evaluation pass at the size of the PhysioNet test split: ``test_data_accuracy`` through the HIP
eval kernels (``train_model.FUSED_EVAL = True``: ``predict_recordings``) against the torch
formulation (``False``), in ONE process.

Workload: 8000 synthetic heart cycles of (4, 2500) in 320 recordings (25 cycles each, interleaved),
resident on the device, ``ResidentLoader(batch 1000, shuffle=False)`` — the loader
``physionet_dataloader.run('test')`` builds; models 'Potes' and 'resnet9'; criterion ``SELCLoss`` (what
the run driver evaluates with); method 'base'.

Method: 2 warm-up calls per path, then ``--rounds`` rounds with the two paths ALTERNATING inside a
round; the clock is the host clock around one call (the call ends in its own device-to-host copy;
the device is idle when it starts).  Reported: median [min .. max] over the rounds, in ms.  The
host is shared with other jobs: read the spread next to every median.

Acceptance: for 'Potes' the fused median is below the torch median in the same run; 'resnet9' is
reported only (its convolutions dominate the call).

The share of evaluation in a short run (``--step-us``: the captured Potes train step, default the
121.9 us of profiles/r4_soak.txt): 11 evaluations against 150 train steps (50 epochs of 3 steps,
11 plot epochs).

    python profiles/eval_time.py [--out profiles/eval_time.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/eval_time.py --trace Potes

``--trace MODEL`` makes ``--calls`` fused calls and as many torch calls after one warm-up each and
times nothing: the launch counts and kernel times come from the profiler's statistics.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, R, T, C_IN, BATCH = 8000, 320, 2500, 4, 1000


def make_loader(dev):
    import numpy as np
    from pcgmix_amd import dataloader_physionet as dlp
    rs = np.random.RandomState(0)
    x = rs.standard_normal((N, C_IN, T)).astype(np.float32)
    rec = rs.permutation(np.repeat(np.arange(R), N // R))
    labels = (rec % 2).astype(np.int64)
    x[labels == 1, 2] *= 3.0
    frames = np.tile(np.asarray([0, 300, 500, 800, 1000], dtype=np.int64), (N, 1))
    wav = [f"{'abcdef'[r % 6]}{r:04d}" for r in rec]
    return dlp.ResidentLoader(x, labels, frames, wav, np.ones(N), batch_size=BATCH, shuffle=False,
                              drop_last=False, device=dev)


def make_call(name, loader, dev):
    import numpy as np
    import torch
    from pcgmix_amd import train_model as tm
    args = argparse.Namespace(dataset="PhysioNet", model=name, method="base", num_classes=2,
                              num_channels=C_IN, sig_len=T)
    torch.manual_seed(0)
    model = tm.build_model(args).to(dev)
    crit = tm.SELCLoss(np.zeros(N, int), 2, es=99, device=dev)

    def call(fused):
        tm.FUSED_EVAL = fused
        return tm.test_data_accuracy(args, model, loader, dev, crit)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-us", type=float, default=121.9)
    ap.add_argument("--trace", default=None, metavar="MODEL")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_time.txt"))
    opts = ap.parse_args()
    import warnings
    import torch
    import pcgmix_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("eval_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda", 0)
    loader = make_loader(dev)
    if opts.trace:
        call = make_call(opts.trace, loader, dev)
        for fused in (True, False):
            for _ in range(1 + opts.calls):
                call(fused)
        torch.cuda.synchronize()
        print(f"traced {opts.trace}: 1 + {opts.calls} calls per path")
        return
    out = [f"# {torch.cuda.get_device_name(0)}; test_data_accuracy over {N} cycles of ({C_IN},{T}) in {R} recordings,",
           f"# ResidentLoader(batch {BATCH}, shuffle=False), SELCLoss, method 'base'; HIP eval kernels (FUSED_EVAL = True)",
           f"# against the torch formulation (False), one process, {opts.warmup} warm-up calls per path, then {opts.rounds} rounds with the",
           "# two paths alternating; host clock around one call (it ends in its own device-to-host copy).",
           "# ms per call: median [min .. max].  The host is shared: compare medians with the spread in mind.",
           "# model     fused ms                      torch ms                      torch/fused  fused < torch   same metrics"]
    verdict = None
    potes_ms = None
    for name in ("Potes", "resnet9"):
        call = make_call(name, loader, dev)
        res = {}
        for fused in (True, False):
            for _ in range(opts.warmup):
                res[fused] = call(fused)
        same = all(abs(res[True][k] - res[False][k]) <= 1e-9 for k in
                   ("accuracy", "specificity", "sensitivity", "precision", "recall", "f1")) \
            and abs(res[True]["loss"] - res[False]["loss"]) <= 1e-5
        got = {True: [], False: []}
        for _ in range(opts.rounds):
            for fused in (True, False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(fused)
                got[fused].append((time.perf_counter() - t0) * 1e3)
        f, u = got[True], got[False]
        mf, mu = statistics.median(f), statistics.median(u)
        line = (f"  {name:8s}  {mf:8.3f} [{min(f):8.3f} .. {max(f):8.3f}]  {mu:8.3f} [{min(u):8.3f} .. {max(u):8.3f}]  "
                f"{mu / mf:8.2f}x     {'yes' if mf < mu else 'NO':3s}             {'yes' if same else 'NO'}")
        out.append(line)
        print(line, flush=True)
        if name == "Potes":
            verdict, potes_ms = mf < mu, (mf, mu)
    out.append("# acceptance (Potes: fused median below torch median in this run; resnet9 reported only): " +
               ("met" if verdict else "NOT met"))
    train_ms = 150 * opts.step_us * 1e-3
    for label, ms in (("fused", potes_ms[0]), ("torch", potes_ms[1])):
        out.append(f"# Potes run of 50 epochs x 3 steps: 150 captured steps x {opts.step_us:.1f} us = {train_ms:.1f} ms of training, "
                   f"11 evaluations ({label}) = {11 * ms:.1f} ms: evaluation is {100 * 11 * ms / (11 * ms + train_ms):.1f} % of the two")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
