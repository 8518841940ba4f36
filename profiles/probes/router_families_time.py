#!/usr/bin/env python3
"""augment() per call for the host-bound families on one MI355X, for A/B runs of two checkouts: the
package is imported from the WORKING DIRECTORY, so the same file times either tree.

The methods of cutpaste_time.py's augment section, one 1D and one 2D baseline, a general-path and a
2D plain splice at (256, 4, 5000) / (256, 1, 128, 128): 20 warm-up calls, then 9 windows of 100
calls between two device events (median, min..max per call); and the dispatch alone — a passthrough
call is the method lookup and the branch, nothing else — on the host clock.

    (cd CHECKOUT && python <this file>) >> profiles/r8_router_ab.txt
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pcgmix_amd  # noqa: E402,F401
from pcgmix_amd import augmentations as A, augmentations2d as A2, synthetic  # noqa: E402

DEV = torch.device("cuda", 0)
REPS, CALLS = 9, 100


class Args:
    def __init__(self, method, dataset="PhysioNet"):
        self.method, self.num_classes, self.sample_rate, self.batch_size = method, 2, 1000, 256
        self.dataset, self.model = dataset, "resnet9"


class Step:
    def __init__(self, count):
        self.count = count


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def report(name, v):
    print(f"  {name:34s} median {statistics.median(v):9.2f} us   min {min(v):9.2f}   max {max(v):9.2f}", flush=True)


print("tree:", os.getcwd())
x, frames, labels, wav = synthetic.make_batch(256, 4, 5000, seed=31)
data = torch.from_numpy(x).to(DEV)
tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(DEV)
fr = torch.from_numpy(frames)
for method in ("durratiocutmix", "(rand)labelcutmix", "labelcutmix(smooth)(cutout)", "durmixrespscale", "cutout",
               "mixup(same)", "(rand)durratiomixup"):
    args = Args(method)
    for s in range(20):
        A.augment(args, data.clone() if method == "cutout" else data, tgt, fr, wav, Step(s), None, DEV, "", host_labels=labels)
    torch.cuda.synchronize()
    v = [window_us(lambda i, r=r: A.augment(args, data, tgt, fr, wav, Step(20 + r * CALLS + i), None, DEV, "",
                                              host_labels=labels), CALLS) for r in range(REPS)]
    report("1D " + method, v)
# 2D: (256, 1, 128, 128) spectrograms, boundaries in columns
rng = np.random.default_rng(3)
img = torch.randn(256, 1, 128, 128, device=DEV)
cuts = np.sort(rng.integers(1, 128, size=(256, 4)), axis=1)
fr2 = torch.from_numpy(np.concatenate([np.zeros((256, 1), np.int64), cuts], axis=1))
for method in ("mixup(same)", "cutout(0.2,0.2)", "durratiomixup"):
    args = Args(method, "PhysioNet(spec128)")
    for s in range(20):
        A2.augment(args, img, tgt, fr2, wav, Step(s), None, DEV, "", host_labels=labels)
    torch.cuda.synchronize()
    v = [window_us(lambda i, r=r: A2.augment(args, img, tgt, fr2, wav, Step(20 + r * CALLS + i), None, DEV, "",
                                               host_labels=labels), CALLS) for r in range(REPS)]
    report("2D " + method, v)
# the dispatch alone: a passthrough call is the route lookup and the branch, nothing else (host clock)
args, st = Args("none"), Step(1)
for name, mod, d in (("1D", A, data), ("2D", A2, img)):
    v = []
    for r in range(REPS):
        t0 = time.perf_counter()
        for i in range(20000):
            mod.augment(args, d, tgt, fr, wav, st, None, DEV, "")
        v.append((time.perf_counter() - t0) / 20000 * 1e6)
    report(name + " dispatch alone (passthrough)", v)
