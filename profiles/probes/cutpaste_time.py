#!/usr/bin/env python3
"""The cut-and-paste family and durmixrespscale (csrc/pcgmix_cutpaste.hip): times on one MI355X.

  augment   one augment() call at (256, 4, 5000): 20 warm-up calls, then REPS windows of CALLS
            calls back to back (a fresh step each, every gate firing) between two device events,
            one synchronisation per window; median and min..max of the per-call time
  kernel    the kernel alone on pre-uploaded tables, device events around LAUNCHES launches,
            REPS windows, at (256, 4, 5000) and at the saturating 16384 x 4 x 5000, with the share
            of 8 TB/s on the bytes the method needs: 8 B per element for cut-and-paste (one source
            read, one write), 12 B per element for the splice of durmixrespscale (own row, partner
            row, output — the splice's contract in profiles/r3_mix_roofline.json; the float64 row
            of T values stays in cache)
  fused     durmixrespscale as ONE launch (pcgmix_mix_scale_f32) against the two launches the
            parent commit can do it with (pcgmix_mix_warp_f32 into a scratch tensor, then
            pcgmix_scale_rows_f32), the two forms alternating window by window in the same process;
            outputs compared bit for bit first
  --trace   a few launches of each kernel at the saturating batch only, for
            rocprofv3 --kernel-trace --stats -- python profiles/probes/cutpaste_time.py --trace

    python profiles/probes/cutpaste_time.py > profiles/r7_cutpaste_time.txt
"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import pcgmix_amd  # noqa: E402,F401
from pcgmix_amd import _lib, augmentations as A, hostprep as H, synthetic  # noqa: E402

METHODS = ("durratiocutmix", "(rand)labelcutmix", "labelcutmix(smooth)(cutout)", "durmixrespscale", "cutout")
DEV = torch.device("cuda", 0)
PEAK = 8.0e12
REPS, CALLS, LAUNCHES = 9, 100, 50


class Args:
    def __init__(self, method):
        self.method, self.num_classes, self.sample_rate, self.batch_size = method, 2, 1000, 256


class Step:
    def __init__(self, count):
        self.count = count


def window_us(fn, n):
    """Per-call device time of n back-to-back calls of fn(i) between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def stats(v):
    return f"median {statistics.median(v):9.2f} us   min {min(v):9.2f}   max {max(v):9.2f}"


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def augment_times(out):
    x, frames, labels, wav = synthetic.make_batch(256, 4, 5000, seed=31)
    data = up(x)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(DEV)
    fr = torch.from_numpy(frames)
    out.append("augment() per call at (256, 4, 5000), host labels passed, %d windows of %d calls" % (REPS, CALLS))
    for method in METHODS:
        args = Args(method)
        for s in range(20):
            A.augment(args, data, tgt, fr, wav, Step(s), None, DEV, "", host_labels=labels)
        torch.cuda.synchronize()
        v = [window_us(lambda i, r=r: A.augment(args, data, tgt, fr, wav, Step(20 + r * CALLS + i), None, DEV, "",
                                                  host_labels=labels), CALLS) for r in range(REPS)]
        out.append(f"  {method:30s} {stats(v)}")


class Problem:
    """Device-resident arguments of the kernels for one batch size."""

    def __init__(self, B, C=4, T=5000):
        self.B, self.C, self.T = B, C, T
        frames, labels, wav = synthetic.make_index_data(B, T, seed=5)
        self.x = torch.randn((B, C, T), device=DEV)
        self.y = torch.empty_like(self.x)
        self.tables = {}
        for method in ("durratiocutmix", "(rand)labelcutmix", "labelcutmix(smooth)(cutout)"):
            plan = H.cutpaste_plan(method, labels, frames, wav, 7, B, C, T, batch_size=256)
            self.tables[method] = (up(plan.segs), up(plan.mix.astype(np.int32)),
                                   up(plan.junctions) if plan.junctions is not None else None)
        np.random.seed(3)
        plan = H.cutpaste_plan("durmixrespscale", labels, frames, wav, 7, B, C, T, sample_rate=1000)
        self.frames = up(frames.astype(np.int32))
        self.mix = up(plan.mix.astype(np.int32))
        self.lam = ctypes.c_float(float(plan.lam32))
        self.row = up(plan.scale_row)
        self.sig = up(H.sigmoid_table().copy())
        self.tmp = None

    def cutpaste(self, method):
        segs, mix, junc = self.tables[method]
        lib, s = _lib.load(), stream()
        args = (self.x.data_ptr(), self.y.data_ptr(), segs.data_ptr(), mix.data_ptr(),
                junc.data_ptr() if junc is not None else None, self.sig.data_ptr() if junc is not None else None,
                self.B, self.C, self.T, s)
        return lambda i=0: _lib.check(lib.pcgmix_cutpaste_rows_f32(*args), "pcgmix_cutpaste_rows_f32")

    def fused(self):
        lib, s = _lib.load(), stream()
        args = (self.x.data_ptr(), self.y.data_ptr(), self.frames.data_ptr(), self.mix.data_ptr(), None, self.lam,
                self.row.data_ptr(), self.B, self.C, self.T, s)
        return lambda i=0: _lib.check(lib.pcgmix_mix_scale_f32(*args), "pcgmix_mix_scale_f32")

    def two_launches(self, dst=None):
        if self.tmp is None:
            self.tmp = torch.empty_like(self.x)
        dst = self.y if dst is None else dst
        lib, s = _lib.load(), stream()
        a1 = (self.x.data_ptr(), self.tmp.data_ptr(), self.frames.data_ptr(), self.mix.data_ptr(), None, self.lam,
              None, None, 0, None, self.B, self.C, self.T, s)
        a2 = (self.tmp.data_ptr(), dst.data_ptr(), self.row.data_ptr(), self.B, self.C, self.T, s)

        def run(i=0):
            _lib.check(lib.pcgmix_mix_warp_f32(*a1), "pcgmix_mix_warp_f32")
            _lib.check(lib.pcgmix_scale_rows_f32(*a2), "pcgmix_scale_rows_f32")
        return run


def kernel_times(out, B, launches):
    p = Problem(B)
    elems = B * p.C * p.T
    out.append(f"kernel alone at ({B}, {p.C}, {p.T}), {REPS} windows of {launches} launches")
    for method in p.tables:
        fn = p.cutpaste(method)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        v = [window_us(fn, launches) for _ in range(REPS)]
        med = statistics.median(v)
        out.append(f"  cutpaste_rows  {method:28s} {stats(v)}   {8 * elems / med / 1e6:7.3f} TB/s "
                   f"= {8 * elems / med / 1e6 / PEAK * 1e12 * 100:5.1f} % of 8 TB/s (8 B/element)")
    fused, two = p.fused(), p.two_launches()
    check = torch.empty_like(p.x)
    fused()
    p.two_launches(check)()
    torch.cuda.synchronize()
    same = torch.equal(p.y, check)
    for _ in range(5):
        fused()
        two()
    torch.cuda.synchronize()
    vf, vt = [], []
    for _ in range(REPS):                                   # alternating, window by window
        vf.append(window_us(fused, launches))
        vt.append(window_us(two, launches))
    mf, mt = statistics.median(vf), statistics.median(vt)
    out.append(f"  durmixrespscale, fused launch  (pcgmix_mix_scale_f32)          {stats(vf)}   "
               f"{12 * elems / mf / 1e6:7.3f} TB/s = {12 * elems / mf / 1e6 / PEAK * 1e12 * 100:5.1f} % of 8 TB/s "
               f"(12 B/element)")
    out.append(f"  durmixrespscale, two launches  (mix_warp -> scratch -> scale)   {stats(vt)}")
    out.append(f"    outputs bit-identical: {same};  fused / two launches = {mf / mt:.3f} (medians); spread of this "
               f"run: fused {min(vf):.2f}..{max(vf):.2f}, two {min(vt):.2f}..{max(vt):.2f} us")


def trace_only():
    p = Problem(16384)
    for method in p.tables:
        fn = p.cutpaste(method)
        for _ in range(10):
            fn()
    fused, two = p.fused(), p.two_launches()
    for _ in range(10):
        fused()
        two()
    torch.cuda.synchronize()


def main():
    if "--trace" in sys.argv:
        return trace_only()
    out = ["cut-and-paste family and durmixrespscale on one MI355X (profiles/probes/cutpaste_time.py)",
           f"device: {torch.cuda.get_device_name(0)}", ""]
    augment_times(out)
    out.append("")
    kernel_times(out, 256, 200)
    out.append("")
    kernel_times(out, 16384, LAUNCHES // 2)
    print("\n".join(out))


if __name__ == "__main__":
    main()
