#!/usr/bin/env python3
"""Big Potes models ('PotesBig64and32' layers [64,32], 'PotesBig128and64' layers [128,64]): the HIP
conv stack (csrc/pcgmix_potes_big.hip, ``m.fused = True``) against the same stack through
torch/MIOpen ops (``m.fused = False`` — what these models ran before the big kernels existed), in
ONE process, after profiles/probes/potes_widths_time.py.

For each model at (256, 4, 2500):

  fwd        the conv stack's forward on the 1024 band rows, no autograd
  fwd+wgrad  forward with autograd + backward of a fixed dL/dh2 to the four weight tensors
  step       the eager ``train_step`` (durmixmagwarp(0.2,4)+0.7, ClipAdam + OneCycleLR, dropout on)
  fwd+dx     ('PotesBig64and32' only) the frozen stack: forward + backward to the input rows

Method: every quantity is warmed up on both paths first (code objects, MIOpen's algorithm search);
then ``--rounds`` rounds, the two paths ALTERNATING inside a round, each timing ``--iters``
back-to-back calls between two HIP events on the current stream; the figure of a round is the
event time over ``--iters``.  Reported: median, min and max over the rounds, in microseconds.  The
event window holds the launches' gaps as well as the kernels: it is a call time, not a kernel time.
The host is shared with other jobs: read the spread next to every median.

Then the four C entry points alone (inference forward, saving forward with m2 + s1, weight gradient
= its three launches, input gradient), the same way, with the matrix work and the bytes each MUST do
(from the shapes alone) over its median as shares of 157 TFLOP/s (f32 matrix peak) and 8 TB/s.

    python profiles/probes/potes_big_time.py [--out profiles/potes_big_time.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
B, C, T = 256, 4, 2500
HBM_PEAK, MATRIX_PEAK = 8.0e12, 157.0e12
MODELS = ("PotesBig64and32", "PotesBig128and64")


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


def build(name, dev):
    import torch
    from pcgmix_amd import train_model as tm
    args = argparse.Namespace(dataset="PhysioNet", model=name, num_classes=2, num_channels=C, sig_len=T)
    torch.manual_seed(0)
    m = tm.build_model(args).to(dev).eval()
    c1, c2 = m.cnn1[0][0], m.cnn1[1][0]
    return m, [c1.weight, c1.bias, c2.weight, c2.bias]


def stack_legs(name, dev):
    import torch
    from pcgmix_amd import models
    m, params = build(name, dev)
    rows = torch.randn(B * C, T, device=dev)
    assert m._fused(rows.view(B, C, T)), "the HIP stack does not apply"
    with torch.no_grad():
        ref = m.cnn1(rows.unsqueeze(1))
        got = models.PotesStackFunction.apply(rows, *params)
    assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5), "paths disagree"
    r = torch.randn_like(ref)
    del ref, got

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

    frozen = [p.detach() for p in params]
    xg = rows.clone().requires_grad_(True)

    def fwd_dx(fused):
        def run():
            xg.grad = None
            if fused:
                h = models.PotesStackFunction.apply(xg, *frozen)
            else:
                a = torch.nn.functional.max_pool1d(torch.relu(
                    torch.nn.functional.conv1d(xg.unsqueeze(1), frozen[0], frozen[1], padding=1)), 2)
                h = torch.nn.functional.max_pool1d(torch.relu(
                    torch.nn.functional.conv1d(a, frozen[2], frozen[3], padding=1)), 2)
            h.backward(r)
        return run

    legs = {"fwd": {"fused": fwd(True), "unfused": fwd(False)},
            "fwd+wgrad": {"fused": fwd_bwd(True), "unfused": fwd_bwd(False)}}
    if name == MODELS[0]:
        legs["fwd+dx"] = {"fused": fwd_dx(True), "unfused": fwd_dx(False)}
    return legs


def step_legs(name, dev, n_steps):
    import numpy as np
    import torch
    from pcgmix_amd import synthetic, train_model as tm
    x, frames, labels, wav = synthetic.make_batch(B, C, T, sample_rate=1000, seed=3)
    batch = (torch.from_numpy(x).to(dev), torch.from_numpy(labels), torch.from_numpy(frames), wav,
             torch.ones(B, dtype=torch.long), torch.arange(B))
    legs = {}
    for label, fused in (("fused", True), ("unfused", False)):
        args = argparse.Namespace(dataset="PhysioNet", model=name, method="durmixmagwarp(0.2,4)+0.7",
                                  num_epochs=2, batch_size=B, op="adam", use_sched=True, lr_max=0.01,
                                  weight_decay=1e-4, grad_clip=0.1, seed=4, seed_fix=4, num_classes=2,
                                  num_channels=C, sig_len=T, depth=0, num_steps=n_steps, sample_rate=1000)
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


def kernel_legs(name, dev):
    """The C entry points alone: {label: (callable, matrix flop, bytes)}."""
    import torch
    from pcgmix_amd import _lib
    lib = _lib.load()
    m, params = build(name, dev)
    w = [p.detach().contiguous() for p in params]
    C1, C2 = w[0].shape[0], w[2].shape[0]
    N = B * C
    P1 = (T - 2) // 2
    P2 = (P1 - 2) // 2
    x = torch.randn(N, T, device=dev)
    g = torch.randn(N, C2, P2, device=dev)
    h2 = torch.empty(N, C2, P2, device=dev)
    nm2, ns1 = lib.pcgmix_potes_big_mask_bytes(N, T, C1, C2, 2), lib.pcgmix_potes_big_mask_bytes(N, T, C1, C2, 1)
    m2 = torch.empty(nm2, dtype=torch.uint8, device=dev)
    s1 = torch.empty(ns1, dtype=torch.uint8, device=dev)
    G, L = lib.pcgmix_potes_big_bwd_blocks(N, T, C1, C2), lib.pcgmix_potes_big_grad_len(C1, C2)
    partial = torch.empty(G, L, device=dev)
    grads = torch.empty(L, device=dev)
    gx = torch.empty(N, T, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    wp = [t.data_ptr() for t in w]
    conv2 = 2.0 * N * 2 * P2 * C2 * 5 * C1            # the second layer as a GEMM
    da1 = 2.0 * N * P1 * C1 * 5 * C2                  # the transposed second layer
    io = N * T * 4 + N * C2 * P2 * 4

    def call(fn, *a):
        def run():
            _lib.check(fn(*a), "probe")
        return run

    return {
        "forward (inference)": (call(lib.pcgmix_potes_big_fwd_f32, x.data_ptr(), *wp, h2.data_ptr(), None, None,
                                     N, T, C1, C2, None, 0, None, 0, st), conv2, io),
        "forward (+ m2, s1)": (call(lib.pcgmix_potes_big_fwd_f32, x.data_ptr(), *wp, h2.data_ptr(), m2.data_ptr(),
                                    s1.data_ptr(), N, T, C1, C2, None, 0, None, 0, st), conv2, io + nm2 + ns1),
        "weight gradient (3 launches)": (call(lib.pcgmix_potes_big_bwd_mask_f32, x.data_ptr(), g.data_ptr(),
                                              m2.data_ptr(), *wp, partial.data_ptr(), grads.data_ptr(), N, T,
                                              C1, C2, st), conv2 + da1, 2 * (io + nm2) + 2 * G * L * 4),
        "input gradient": (call(lib.pcgmix_potes_big_input_grad_mask_f32, g.data_ptr(), m2.data_ptr(),
                                s1.data_ptr(), wp[0], wp[2], gx.data_ptr(), N, T, C1, C2, st), da1,
                           io + nm2 + ns1),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "potes_big_time.txt"))
    opts = ap.parse_args()
    assert opts.rounds >= 7
    import warnings
    import torch
    import pcgmix_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("potes_big_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda", 0)
    out = [f"# {torch.cuda.get_device_name(0)}; big Potes models, HIP conv stack (fused) against torch/MIOpen ops (unfused:",
           "# the path these models took before the big kernels), one process, both paths warmed up, then",
           f"# {opts.rounds} rounds with the two paths alternating; a round = {opts.iters} calls ({opts.step_iters} train steps) between two HIP events.",
           "# us per call: median [min .. max] over the rounds.  The host is shared: compare medians with the spread in mind.",
           "# model             shape           quantity    fused us                      unfused us                    unfused/fused  fused < unfused"]
    worse = []
    n_steps = (opts.rounds + 1) * opts.step_iters + opts.warmup + 8

    def emit(line):
        out.append(line)
        print(line, flush=True)

    for name in MODELS:
        rows = [(q, alternate(fns, opts, opts.iters)) for q, fns in stack_legs(name, dev).items()]
        torch.cuda.empty_cache()
        rows.append(("step", alternate(step_legs(name, dev, n_steps), opts, opts.step_iters)))
        torch.cuda.empty_cache()
        for q, got in rows:
            f, u = got["fused"], got["unfused"]
            mf, mu = statistics.median(f), statistics.median(u)
            ok = mf < mu
            if not ok:
                worse.append(f"{name} {q}")
            emit(f"  {name:16s} ({B},{C},{T:4d})  {q:10s}  {mf:9.1f} [{min(f):9.1f} .. {max(f):9.1f}]  "
                 f"{mu:9.1f} [{min(u):9.1f} .. {max(u):9.1f}]  {mu / mf:8.2f}x      {'yes' if ok else 'NO'}")
    emit("# acceptance (fused median below unfused median for every quantity): " +
         ("met" if not worse else "NOT met for " + "; ".join(worse)))
    emit("# the C entry points alone, 1024 rows of 2500: us per call, median [min .. max]; matrix work and bytes from the")
    emit("# shapes over the median, as shares of 157 TFLOP/s (f32 matrix peak) and of 8 TB/s")
    emit("# model             entry point                     us                            TFLOP/s  of peak   GB/s   of peak")
    for name in MODELS:
        for label, (fn, flop, nbytes) in kernel_legs(name, dev).items():
            t = alternate({"k": fn}, opts, opts.iters)["k"]
            med = statistics.median(t)
            tf, bw = flop / (med * 1e-6), nbytes / (med * 1e-6)
            emit(f"  {name:16s}  {label:30s}  {med:9.1f} [{min(t):9.1f} .. {max(t):9.1f}]  {tf / 1e12:6.1f}  "
                 f"{tf / MATRIX_PEAK * 100:5.1f} %  {bw / 1e9:6.0f}  {bw / HBM_PEAK * 100:5.1f} %")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
