#!/usr/bin/env python3
"""The paper's spectrogram comparison baselines (csrc/pcgmix_baselines.hip, pcgmix_cutpaste.hip) at
(256, 1, 128, 128).

  augment   steady-state time of one augment() call: 20 warm-up calls, then 200 calls back to
            back (a fresh step each, every gate firing), one synchronisation at the end; beside it
            the host plan alone (make_plan over the same steps); latentmixup with ResNet9-2D
            (train mode), and the share of the model's first half
  kernel    the method's kernel alone, launched back to back on pre-uploaded arguments (hipEvent
            pairs), and the fraction of 8 TB/s on the bytes the method needs: 12 B per element for
            the blend (own, partner, output), 4 B per written element plus 4 B per copied one for
            the piecewise copy, 4 B per ZEROED element for the masks (in place) — at 4096 x 1 x
            128 x 128; latentmixup's blend forward and backward at depth 1 (256 x 128 x 64 x 64)
  --trace   only a few augment() calls per method, for
            rocprofv3 --kernel-trace --stats -- python profiles/probes/baselines2d_time.py --trace
  --trace-kernels  the kernel-alone legs only (4096 x 1 x 128 x 128, the latent blend), for the same

    python profiles/probes/baselines2d_time.py
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
from pcgmix_amd import _lib, augmentations2d as A2, hostprep as H, models2d, synthetic  # noqa: E402

METHODS = ("timemask(0.1)", "freqmask(0.1)", "mixup(same)", "mixup(mix)", "cutmix", "(rand)cutmix",
           "durratiocutmix", "(rand)durratiocutmix")
DEV = torch.device("cuda", 0)
PEAK = 8.0e12


class Args:
    def __init__(self, method):
        self.method, self.num_classes, self.model, self.depth = method, 2, "resnet9", 0


class Step:
    def __init__(self, count):
        self.count = count


def batch(B, seed=1):
    _, frames, labels, _ = synthetic.make_batch(B, 1, 5000, sample_rate=2000, seed=seed)
    fs = synthetic.spec_frames(frames, 148, 5000)
    x = np.random.RandomState(seed).standard_normal((B, 1, 128, 128)).astype(np.float32)
    x[np.broadcast_to(np.arange(128)[None, None, None, :] >= fs[:, 4][:, None, None, None], x.shape)] = 0
    return x, fs, labels


def augment_us(method, data, tgt, frames, labels, model=None, n=200, warm=20):
    args = Args(method)
    for s in range(warm):
        A2.augment(args, data, tgt, frames, None, Step(s), model, DEV, "", host_labels=labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(warm, warm + n):
        A2.augment(args, data, tgt, frames, None, Step(s), model, DEV, "", host_labels=labels)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def plan_us(method, frames, labels, n=200):
    """The host part alone: make_plan (gate, partners, draws, tables) with host labels."""
    B = frames.shape[0]
    t0 = time.perf_counter()
    for st in range(n):
        H.make_plan(method, labels, frames, None, st, B, 1, is2d=True, n_cols=128, n_freq=128)
    return (time.perf_counter() - t0) / n * 1e6


def timed(call, iters):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def kernel_us(method, x, frames, labels, iters):
    """(us per launch, bytes needed) of the method's kernel on pre-uploaded arguments."""
    B, C, F, W = x.shape
    lib = _lib.load()
    np.random.seed(1)
    plan = H.make_plan(method, labels, frames, None, 3, B, C, is2d=True, n_cols=W, n_freq=F)
    assert plan.fired
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    kind = plan.kind
    if kind == "mixup2d":
        y = torch.empty_like(x)
        mix = torch.from_numpy(plan.mix.astype(np.int32)).to(DEV)
        call = lambda: lib.pcgmix_blend_rows_f32(x.data_ptr(), y.data_ptr(), mix.data_ptr(),  # noqa: E731
                                                 ctypes.c_float(float(plan.lam32)), B, 1, C * F * W, st)
        nbytes = 12 * x.numel()
    elif kind in ("timemask2d", "freqmask2d"):
        y = x.clone()
        r = plan.zero_rect
        area = (r[:, 1] - r[:, 0]).clip(0) * (r[:, 3] - r[:, 2]).clip(0)
        rect = torch.from_numpy(r).to(DEV)
        call = lambda: lib.pcgmix_zero_rects_f32(y.data_ptr(), rect.data_ptr(), B, C, F, W,  # noqa: E731
                                                 int(area.max()), st)
        nbytes = 4 * C * int(area.sum())
    else:
        y = torch.empty((B, C, F, plan.out_cols), device=DEV)
        segs = torch.from_numpy(plan.segs).to(DEV)
        mix = torch.from_numpy(plan.mix.astype(np.int32)).to(DEV)
        call = lambda: lib.pcgmix_piecewise_rows_f32(x.data_ptr(), y.data_ptr(), segs.data_ptr(),  # noqa: E731
                                                     mix.data_ptr(), plan.seg_axis, B, C, F, W, plan.out_cols, st)
        s = plan.segs.astype(np.int64)
        copied = ((s[:, :, 1] - s[:, :, 0]).clip(0) * (s[:, :, 2] != 2)).sum()
        other = W if plan.seg_axis == 1 else F
        nbytes = 4 * y.numel() + 4 * C * other * int(copied)
    _lib.check(call(), method)
    return timed(call, iters), nbytes


def latent_blend_us(iters=50):
    """latentmixup's blend at depth 1 (256 x 128 x 64 x 64 channels-last): forward, backward."""
    h = torch.randn(256, 128, 64, 64, device=DEV).contiguous(memory_format=torch.channels_last)
    h.requires_grad_(True)
    mix = H.shuffle_within_groups(np.arange(256) % 2, 3)
    g = torch.randn_like(h)
    fwd = timed(lambda: A2.latent_blend(h, mix, np.float32(0.4)), iters)
    out = A2.latent_blend(h, mix, np.float32(0.4))

    def bwd():
        h.grad = None
        out.backward(g, retain_graph=True)
    return fwd, timed(bwd, iters), 12 * h.numel()


def main():
    trace = "--trace" in sys.argv
    x, frames, labels = batch(256)
    data = torch.from_numpy(x).to(DEV)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(DEV)
    fr = torch.from_numpy(frames)
    torch.manual_seed(0)
    net = models2d.ResNet9(2).to(DEV).train()
    if "--trace-kernels" in sys.argv:
        xb, fb, lb = batch(4096, seed=2)
        xb = torch.from_numpy(xb).to(DEV)
        for m in METHODS:
            kernel_us(m, xb, fb, lb, 10)
        latent_blend_us(10)
        torch.cuda.synchronize()
        print("kernel trace run done")
        return
    if trace:
        for m in METHODS + ("latentmixup",):
            for s in range(5):
                A2.augment(Args(m), data.clone(), tgt, fr, None, Step(s), net, DEV, "", host_labels=labels)
        torch.cuda.synchronize()
        print("trace run done")
        return
    print(f"{torch.cuda.get_device_name(0)}; augment() at (256, 1, 128, 128), host labels, 200 steps")
    for m in METHODS:
        print(f"  {m:26s} {augment_us(m, data, tgt, fr, labels):9.1f} us per call, of which "
              f"{plan_us(m, frames, labels):6.1f} us host plan (make_plan alone)", flush=True)
    lat = augment_us("latentmixup", data, tgt, fr, labels, model=net, n=30, warm=5)
    firsts = []
    for depth in (1, 2, 3):
        firsts.append(timed(lambda: net(data, depth=depth, pass_part="first"), 10))
    depths = [H.make_plan("latentmixup", labels, frames, None, s, 256, 1, is2d=True, n_cols=128,
                          n_freq=128).depth for s in range(5, 35)]
    mean_first = float(np.mean([firsts[d - 1] for d in depths]))
    print(f"  {'latentmixup (ResNet9-2D)':26s} {lat:9.1f} us per call; first half alone at depth 1/2/3: "
          f"{firsts[0]:.0f} / {firsts[1]:.0f} / {firsts[2]:.0f} us -> {mean_first / lat:5.1%} of the call "
          f"over the timed steps' depths", flush=True)
    xb, fb, lb = batch(4096, seed=2)
    xb = torch.from_numpy(xb).to(DEV)
    print("kernel alone, back to back, 4096x1x128x128")
    for m in METHODS:
        us, nbytes = kernel_us(m, xb, fb, lb, 20)
        print(f"  {m:26s} {us:10.1f} us  {nbytes / us / 1e3:8.1f} GB/s  {nbytes / us * 1e6 / PEAK:5.2f} "
              f"of 8 TB/s", flush=True)
    fwd, bwd, nbytes = latent_blend_us()
    for tag, us in (("forward", fwd), ("backward", bwd)):
        print(f"  latentmixup blend {tag:9s} {us:10.1f} us  {nbytes / us / 1e3:8.1f} GB/s  "
              f"{nbytes / us * 1e6 / PEAK:5.2f} of 8 TB/s  (256x128x64x64, channels-last)", flush=True)


if __name__ == "__main__":
    main()
