#!/usr/bin/env python3
"""Narrow Potes models ('Potes0.02' layers [1,1], 'Potes0.1' layers [2,1]): the HIP conv stack
(csrc/pcgmix_potes_narrow.hip, ``m.fused = True``) against the same stack through torch/MIOpen ops
(``m.fused = False`` — what these models ran before the narrow kernels existed), in ONE process.

For each model at (256, 4, 2500) and (256, 4, 5000):

  fwd        the conv stack's forward on the 1024 band rows, no autograd
  fwd+wgrad  forward with autograd + backward of a fixed dL/dh2 to the four weight tensors
  step       the eager ``train_step`` (durmixmagwarp(0.2,4)+0.7, ClipAdam + OneCycleLR, dropout on)

Method: every quantity is warmed up on both paths first (code objects, MIOpen's algorithm search);
then ``--rounds`` rounds, the two paths ALTERNATING inside a round, each timing ``--iters``
back-to-back calls between two HIP events on the current stream; the figure of a round is the
event time over ``--iters``.  Reported: median, min and max over the rounds, in microseconds.  The
event window holds the launches' gaps as well as the kernels: it is a call time, not a kernel time.
The host is shared with other jobs: read the spread next to every median.

Bytes: what the narrow kernels must move per call, from the shapes alone (x in, h2 out, the
routing bytes; for the backward x, dL/dh2 and m2 in) over the fused median, as a share of the
8 TB/s HBM peak of an MI355X — a lower bound on the kernels' own share, since the window also
holds launch gaps.

    python profiles/probes/potes_widths_time.py [--out profiles/potes_widths_time.txt]
"""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
B, C = 256, 4
HBM_PEAK = 8.0e12


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(fns, opts, iters):
    """fns: {label: callable}.  Warm-up, then rounds with the labels alternating."""
    import torch
    for fn in fns.values():
        for _ in range(opts.warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(opts.rounds):
        for k, fn in fns.items():
            got[k].append(timed(fn, iters))
    return got


def stack_legs(name, T, dev):
    import torch
    from pcgmix_amd import models, train_model as tm
    args = argparse.Namespace(dataset="PhysioNet", model=name, num_classes=2, num_channels=C, sig_len=T)
    torch.manual_seed(0)
    m = tm.build_model(args).to(dev).eval()
    c1, c2 = m.cnn1[0][0], m.cnn1[1][0]
    params = [c1.weight, c1.bias, c2.weight, c2.bias]
    rows = torch.randn(B * C, T, device=dev)
    assert m._fused(rows.view(B, C, T)), "the HIP stack does not apply"
    with torch.no_grad():
        ref = m.cnn1(rows.unsqueeze(1))
        got = models.PotesStackFunction.apply(rows, *params)
    assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5), "paths disagree"
    r = torch.randn_like(ref)

    def fwd(fused):
        def run():
            with torch.no_grad():
                return models.PotesStackFunction.apply(rows, *params) if fused else m.cnn1(rows.unsqueeze(1))
        return run

    def fwd_bwd(fused):
        def run():
            for p in params:
                p.grad = None
            h = models.PotesStackFunction.apply(rows, *params) if fused else m.cnn1(rows.unsqueeze(1))
            h.backward(r)
        return run

    C1, C2, P2 = c1.out_channels, c2.out_channels, ref.shape[-1]
    N = B * C
    m2 = N * C2 * ((P2 + 3) // 4)
    b_fwd = N * T * 4 + N * C2 * P2 * 4
    b_bwd = b_fwd + m2 + N * T * 4 + N * C2 * P2 * 4 + m2          # saving forward + weight gradient
    return {"fwd": ({"fused": fwd(True), "unfused": fwd(False)}, b_fwd),
            "fwd+wgrad": ({"fused": fwd_bwd(True), "unfused": fwd_bwd(False)}, b_bwd)}


def step_legs(name, T, dev, n_steps):
    import numpy as np
    import torch
    from pcgmix_amd import synthetic, train_model as tm
    sr = 2000 if T == 5000 else 1000
    x, frames, labels, wav = synthetic.make_batch(B, C, T, sample_rate=sr, seed=3)
    batch = (torch.from_numpy(x).to(dev), torch.from_numpy(labels), torch.from_numpy(frames), wav,
             torch.ones(B, dtype=torch.long), torch.arange(B))
    legs = {}
    for label, fused in (("fused", True), ("unfused", False)):
        args = argparse.Namespace(dataset="PhysioNet", model=name, method="durmixmagwarp(0.2,4)+0.7",
                                  num_epochs=2, batch_size=B, op="adam", use_sched=True, lr_max=0.01,
                                  weight_decay=1e-4, grad_clip=0.1, seed=4, seed_fix=4, num_classes=2,
                                  num_channels=C, sig_len=T, depth=0, num_steps=n_steps, sample_rate=sr)
        torch.manual_seed(0)
        net = tm.build_model(args).to(dev).train()
        net.fused = fused
        opt, sched = tm.make_optimizer(args, net)
        crit = tm.SELCLoss(labels, 2, es=args.num_epochs + 1, device=dev)
        sc = tm.step_counter_class()
        np.random.seed(1)
        legs[label] = (lambda a=args, n=net, o=opt, s=sched, c=crit, k=sc:
                       tm.train_step(a, n, batch, dev, o, s, c, 1, k))
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "potes_widths_time.txt"))
    opts = ap.parse_args()
    import warnings
    import torch
    import pcgmix_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("potes_widths_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda", 0)
    out = [f"# {torch.cuda.get_device_name(0)}; narrow Potes models, HIP conv stack (fused) against torch/MIOpen ops (unfused:",
           "# the path these models took before the narrow kernels), one process, both paths warmed up, then",
           f"# {opts.rounds} rounds with the two paths alternating; a round = {opts.iters} calls ({opts.step_iters} train steps) between two HIP events.",
           "# us per call: median [min .. max] over the rounds.  The host is shared: compare medians with the spread in mind.",
           "# HBM share: bytes the narrow kernels must move (from the shapes) / fused median / 8 TB/s; the event window",
           "# includes launch gaps, so the kernels' own share is higher.",
           "# model      shape            quantity    fused us                    unfused us                  unfused/fused  HBM share  fused < unfused"]
    worse = []
    n_steps = (opts.rounds + 1) * opts.step_iters + opts.warmup + 8
    for name in ("Potes0.02", "Potes0.1"):
        for T in (2500, 5000):
            rows = []
            for q, (fns, nbytes) in stack_legs(name, T, dev).items():
                rows.append((q, alternate(fns, opts, opts.iters), nbytes))
            rows.append(("step", alternate(step_legs(name, T, dev, n_steps), opts, opts.step_iters), None))
            for q, got, nbytes in rows:
                f, u = got["fused"], got["unfused"]
                mf, mu = statistics.median(f), statistics.median(u)
                share = f"{nbytes / (mf * 1e-6) / HBM_PEAK * 100:5.1f} %" if nbytes else "    -  "
                ok = mf < mu
                if not ok:
                    worse.append(f"{name} ({B},{C},{T}) {q}")
                line = (f"  {name:10s} ({B},{C},{T:4d})  {q:10s}  {mf:8.1f} [{min(f):8.1f} .. {max(f):8.1f}]  "
                        f"{mu:8.1f} [{min(u):8.1f} .. {max(u):8.1f}]  {mu / mf:8.2f}x      {share}    {'yes' if ok else 'NO'}")
                out.append(line)
                print(line, flush=True)
    out.append("# acceptance (fused median below unfused median for every quantity): " +
               ("met" if not worse else "NOT met for " + "; ".join(worse)))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
