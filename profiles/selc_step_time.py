#!/usr/bin/env python3
"""SELC-phase train step, Potes at (256,4,5000), method SELCdurratiomixup: microseconds per step of

  (a) train_epoch's captured SELC-phase step (fused head + SELC tail kernel inside the hipGraph),
  (b) the path such a run took before: args.hipgraph = False with SELCLoss.use_kernel = False
      (eager train_step, the loss as torch ops),
  (c) beside them, the captured plain-CE step of the same run (an epoch before the turning point).

The three alternate in ONE process: two warm-up rounds, then ROUNDS timed rounds; a round is one
train_epoch call over STEPS device-resident batches per path and ends in that call's host read of
the epoch statistics (a synchronise).  Median and [min .. max] over the rounds.

    python profiles/selc_step_time.py [--out profiles/selc_step_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pcgmix_amd  # noqa: E402,F401
from pcgmix_amd import synthetic, train_model as tm  # noqa: E402

B, T, STEPS, ROUNDS, WARM = 256, 5000, 40, 9, 2


def setup(device, batches, es, hipgraph, use_kernel):
    args = argparse.Namespace(
        dataset="PhysioNet", model="Potes", method="SELCdurratiomixup", num_epochs=10, batch_size=B,
        op="adam", use_sched=True, lr_max=0.01, weight_decay=1e-4, grad_clip=0.1, seed=4, seed_fix=4,
        num_classes=2, num_channels=4, sample_rate=2000, depth=0, sig_len=T, num_steps=10 ** 6,
        hipgraph=hipgraph)
    torch.manual_seed(7)
    net = tm.build_model(args).to(device).train()
    opt, sched = tm.make_optimizer(args, net)
    labels = np.concatenate([b[1].numpy() for b in batches])
    crit = tm.SELCLoss(labels, 2, es=es, device=device)
    return dict(args=args, net=net, opt=opt, sched=sched, crit=crit, sc=tm.step_counter_class(),
                use_kernel=use_kernel, times=[])


def run_round(p, batches, device, epoch):
    tm.SELCLoss.use_kernel = p["use_kernel"]
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tm.train_epoch(p["args"], p["net"], batches, device, p["opt"], p["sched"], p["crit"], epoch, p["sc"])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(batches) * 1e6
    finally:
        tm.SELCLoss.use_kernel = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selc_step_time.txt"))
    out_path = ap.parse_args().out
    device = torch.device("cuda:0")
    batches = []
    for i in range(STEPS):
        x, frames, labels, wav = synthetic.make_batch(B, 4, T, sample_rate=2000, seed=900 + i)
        batches.append((torch.from_numpy(x).to(device), torch.from_numpy(labels), torch.from_numpy(frames),
                        wav, torch.ones(B, dtype=torch.long), torch.arange(B) + B * i))
    paths = {
        "a": (setup(device, batches, 1, True, True), 2),      # captured SELC-phase step
        "b": (setup(device, batches, 1, False, False), 2),    # eager step, torch-op loss
        "c": (setup(device, batches, 99, True, True), 1),     # captured plain-CE step
    }
    for r in range(WARM + ROUNDS):
        for name in ("a", "b", "c"):
            p, epoch = paths[name]
            us = run_round(p, batches, device, epoch)
            if r >= WARM:
                p["times"].append(us)
    step_a = paths["a"][0]["net"].__dict__["_pcgmix_epoch_step"].step
    step_c = paths["c"][0]["net"].__dict__["_pcgmix_epoch_step"].step
    assert step_a.selc and not step_c.selc and "_pcgmix_epoch_step" not in paths["b"][0]["net"].__dict__

    def line(tag, t):
        return f"{tag:58s} {statistics.median(t):8.1f} us  [{min(t):.1f} .. {max(t):.1f}]"
    ta, tb, tc = (paths[k][0]["times"] for k in "abc")
    lines = [
        f"SELC-phase train step, Potes ({B},4,{T}), SELCdurratiomixup, {torch.cuda.get_device_name(0)}",
        f"per step over {STEPS}-step train_epoch calls, {ROUNDS} rounds after {WARM} warm-up rounds, paths alternating",
        line("(a) captured SELC-phase step (train_epoch)", ta),
        line("(b) hipgraph=False, SELCLoss.use_kernel=False (before)", tb),
        line("(c) captured plain-CE step (train_epoch)", tc),
        f"median (a) - median (c): {statistics.median(ta) - statistics.median(tc):+.1f} us",
        f"median (b) / median (a): {statistics.median(tb) / statistics.median(ta):.2f}x",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    if not statistics.median(ta) < statistics.median(tb):
        raise SystemExit("acceptance: the captured SELC step is not faster than the eager path")


if __name__ == "__main__":
    main()
