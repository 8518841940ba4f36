#!/usr/bin/env python3
"""The paper's 1D comparison baselines (csrc/pcgmix_baselines.hip) at (256, 4, 5000).

  augment   steady-state time of one augment() call: 20 warm-up calls, then 200 calls back to
            back (a fresh step each, every gate firing), one synchronisation at the end
  kernel    the method's kernel alone, launched back to back on pre-uploaded arguments
            (hipEvent pairs around 50-200 launches), and the fraction of 8 TB/s on the bytes the
            method needs: 12 B per element for mixup (own row, partner row, output), 8 for the
            warps and respiratoryscale, 4 per ZEROED element for timemask (in place) — at
            (256, 4, 5000) and at the saturating 16384 x 4 x 5000
  --trace   only a few augment() calls per method, for
            rocprofv3 --kernel-trace --stats -- python profiles/probes/baselines_time.py --trace

    python profiles/probes/baselines_time.py
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import pcgmix_amd  # noqa: E402,F401
from pcgmix_amd import _lib, augmentations as A, hostprep as H, synthetic  # noqa: E402

METHODS = ("mixup(same)", "mixup(mix)", "magnitudewarp(0.2,4)", "timewarp(0.05,4)",
           "timewarp(0.2,4)", "timemask(0.2)", "respiratoryscale(12,20)")
DEV = torch.device("cuda", 0)
PEAK = 8.0e12


class Args:
    def __init__(self, method):
        self.method, self.num_classes, self.sample_rate = method, 2, 1000


class Step:
    def __init__(self, count):
        self.count = count


def augment_us(method, data, tgt, frames, wav, labels, n=200, warm=20):
    args = Args(method)
    for s in range(warm):
        A.augment(args, data, tgt, frames, wav, Step(s), None, DEV, "", host_labels=labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(warm, warm + n):
        A.augment(args, data, tgt, frames, wav, Step(s), None, DEV, "", host_labels=labels)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def kernel_us(method, x, frames, labels, wav, iters):
    """(us per launch, bytes needed) of the method's kernel on pre-uploaded arguments."""
    B, C, T = x.shape
    lib = _lib.load()
    np.random.seed(1)
    plan = H.make_plan(method, labels, frames, wav, 3, B, C, sample_rate=1000, sig_len=T)
    assert plan.fired
    y = torch.empty_like(x)
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    kind = plan.kind
    if kind == "mixup":
        mix = torch.from_numpy(plan.mix.astype(np.int32)).to(DEV)
        call = lambda: lib.pcgmix_blend_rows_f32(x.data_ptr(), y.data_ptr(), mix.data_ptr(),  # noqa: E731
                                                 ctypes.c_float(float(plan.lam32)), B, C, T, st)
        nbytes = 12 * x.numel()
    elif kind in ("magnitudewarp", "timewarp"):
        kn = torch.from_numpy(plan.knots).to(DEV)
        op = A.spline_operator(DEV, T, plan.n_knots)
        if kind == "magnitudewarp":
            call = lambda: lib.pcgmix_warp_rows_f32(x.data_ptr(), y.data_ptr(), kn.data_ptr(),  # noqa: E731
                                                    op.data_ptr(), plan.n_knots, B, C, T, st)
        else:
            nws = lib.pcgmix_time_warp_workspace_bytes(B, C, T)
            ws = torch.empty(max(1, nws // 8), dtype=torch.float64, device=DEV)
            call = lambda: lib.pcgmix_time_warp_f32(x.data_ptr(), y.data_ptr(), kn.data_ptr(),  # noqa: E731
                                                    op.data_ptr(), plan.n_knots, ws.data_ptr(), B, C, T, st)
        nbytes = 8 * x.numel()
    elif kind == "respiratoryscale":
        row = torch.from_numpy(plan.scale_row).to(DEV)
        call = lambda: lib.pcgmix_scale_rows_f32(x.data_ptr(), y.data_ptr(), row.data_ptr(), B, C, T, st)  # noqa: E731
        nbytes = 8 * x.numel()
    else:
        sp = torch.from_numpy(plan.spans).to(DEV)
        call = lambda: lib.pcgmix_zero_spans_f32(y.data_ptr(), sp.data_ptr(), B, C, T, st)  # noqa: E731
        nbytes = 4 * C * int((plan.spans[:, 1] - plan.spans[:, 0]).sum())
    for _ in range(3):
        _lib.check(call(), method)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, nbytes


def main():
    trace = "--trace" in sys.argv
    x, frames, labels, wav = synthetic.make_batch(256, 4, 5000, sample_rate=2000, seed=1)
    data = torch.from_numpy(x).to(DEV)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(DEV)
    fr = torch.from_numpy(frames)
    if trace:
        for m in METHODS:
            for s in range(5):
                A.augment(Args(m), data, tgt, fr, wav, Step(s), None, DEV, "", host_labels=labels)
        torch.cuda.synchronize()
        print("trace run done")
        return
    print(f"{torch.cuda.get_device_name(0)}; augment() at (256, 4, 5000), host labels, 200 steps")
    for m in METHODS:
        print(f"  {m:26s} {augment_us(m, data, tgt, fr, wav, labels):9.1f} us per call", flush=True)
    big = synthetic.make_batch(16384, 4, 5000, sample_rate=2000, seed=2)
    xb = torch.from_numpy(big[0]).to(DEV)
    for tag, (xx, ff, ll, ww), iters in (("256x4x5000", (data, frames, labels, wav), 200),
                                         ("16384x4x5000", (xb, big[1], big[2], big[3]), 10)):
        print(f"kernel alone, back to back, {tag}")
        for m in METHODS:
            us, nbytes = kernel_us(m, xx, ff, ll, ww, iters)
            print(f"  {m:26s} {us:10.1f} us  {nbytes / us / 1e3:8.1f} GB/s  {nbytes / us * 1e6 / PEAK:5.2f} "
                  f"of 8 TB/s", flush=True)


if __name__ == "__main__":
    main()
