#!/usr/bin/env python3
"""The captured Potes train step with ``op='SGD'``: ClipSGD as the step's last launch
(``train_model.FUSED_SGD = True``) against what the code did before ClipSGD existed (``False``:
``torch.optim.SGD`` — ``clip_grad_value_`` inside the capture, torch's Python optimiser after every
replay), in ONE process, with the ClipAdam step of the same run for scale.

Workload: 'Potes' at batch (256, 4, 2500), method 'durratiomixup', ``use_sched=True`` (OneCycleLR
moves lr and momentum on every step), ``grad_clip=0.1``, through ``train_epoch`` — the captured step
as a user of the reference's loop gets it.  The batches are resident on the device (eight distinct
ones, cycled), so a step is the splice, the step's launches, the scheduler and the counters.

Method: every path has its own model, optimiser and captured step.  ``--warmup`` epochs per path,
then ``--rounds`` rounds with the three paths ALTERNATING inside a round; one timed unit is one
``train_epoch`` of ``--steps`` steps, host clock around the call (it ends in its own device-to-host
copy of the loss sum; the device is idle when it starts).  Reported: us per step, median
[min .. max] over the rounds.  The host is shared with other jobs: read the spread next to every
median.  No ratio is fixed in advance; the file says which median is lower.

Launch counts per step come from a kernel trace, in runs of their own (tracing slows the host):

    rocprofv3 -f csv --kernel-trace -d DIR/new  -- python profiles/sgd_step_time.py --trace new
    rocprofv3 -f csv --kernel-trace -d DIR/old  -- python profiles/sgd_step_time.py --trace old
    rocprofv3 -f csv --kernel-trace -d DIR/adam -- python profiles/sgd_step_time.py --trace adam
    python profiles/sgd_step_time.py --launches DIR [--out profiles/sgd_step_time.txt]

``--trace PATH`` runs one epoch of ``--steps`` steps on one path and times nothing; ``--launches DIR``
counts, in each trace, the dispatches from one forward kernel of the conv stack to the next (the
median over the steady steps) and writes them next to the timings.
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, C, T, POOL = 256, 4, 2500, 8
PATHS = ("new", "old", "adam")
LABEL = {"new": "SGD, ClipSGD in the step (FUSED_SGD = True)",
         "old": "SGD, torch.optim.SGD (FUSED_SGD = False)",
         "adam": "adam, ClipAdam in the step (for scale)"}
FORWARD = "potes_fwd_mfma_kernel"


def make_path(path, dev, pool, steps):
    """(epoch function, captured-step getter) of one path."""
    import numpy as np
    import torch
    from pcgmix_amd import train_model as tm
    args = argparse.Namespace(dataset="PhysioNet", model="Potes", method="durratiomixup", num_epochs=10 ** 6,
                              batch_size=B, op="adam" if path == "adam" else "SGD", use_sched=True,
                              lr_max=0.01, weight_decay=1e-4, grad_clip=0.1, seed=4, seed_fix=4, num_classes=2,
                              num_channels=C, sig_len=T, depth=0, num_steps=10 ** 7, sample_rate=1000)
    torch.manual_seed(0)
    net = tm.build_model(args).to(dev).train()
    tm.FUSED_SGD = path != "old"
    try:
        opt, sched = tm.make_optimizer(args, net)
    finally:
        tm.FUSED_SGD = True
    want = {"new": tm.ClipSGD, "old": torch.optim.SGD, "adam": tm.ClipAdam}[path]
    if type(opt) is not want:
        raise SystemExit(f"path {path!r}: make_optimizer gave {type(opt).__name__}")
    crit = tm.SELCLoss(np.zeros(B * POOL, int), 2, es=args.num_epochs + 1, device=dev)
    sc = tm.step_counter_class()
    loader = [pool[i % POOL] for i in range(steps)]

    def epoch():
        return tm.train_epoch(args, net, loader, dev, opt, sched, crit, 0, sc)

    def captured():
        hit = net.__dict__.get("_pcgmix_epoch_step")
        return None if hit is None else hit.step
    return epoch, captured


def make_pool(dev):
    import torch
    from pcgmix_amd import synthetic
    pool = []
    for i in range(POOL):
        x, frames, labels, wav = synthetic.make_batch(B, C, T, sample_rate=1000, seed=40 + i)
        pool.append((torch.from_numpy(x).to(dev), torch.from_numpy(labels), torch.from_numpy(frames), wav,
                     torch.ones(B, dtype=torch.long), torch.arange(i * B, (i + 1) * B)))
    return pool


def launches_per_step(trace_dir):
    """Median number of kernel dispatches from one conv-stack forward to the next, or None."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    at = [i for i, (_t, name) in enumerate(rows) if FORWARD in name]
    gaps = [b - a for a, b in zip(at, at[1:])]
    gaps = gaps[len(gaps) // 2:]                        # the steady half: past warm-up and capture
    if not gaps:
        return None
    names = []                                          # one steady step, repeats folded: "name x2"
    for _t, n in rows[at[-2]:at[-1]]:
        n = n.replace("void ", "").replace("(anonymous namespace)::", "").split("<")[0].split("(")[0]
        if names and names[-1][0] == n:
            names[-1][1] += 1
        else:
            names.append([n, 1])
    return statistics.median(gaps), min(gaps), max(gaps), [n if k == 1 else f"{n} x{k}" for n, k in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--trace", default=None, choices=PATHS)
    ap.add_argument("--launches", default=None, metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd_step_time.txt"))
    opts = ap.parse_args()
    if opts.rounds < 7:
        raise SystemExit("at least 7 rounds")
    import warnings
    import torch
    import pcgmix_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("sgd_step_time.py needs the GPU: nothing is measured without one")
    warnings.simplefilter("ignore", RuntimeWarning)
    dev = torch.device("cuda", 0)
    pool = make_pool(dev)
    if opts.trace:
        epoch, _ = make_path(opts.trace, dev, pool, opts.steps)
        epoch()
        torch.cuda.synchronize()
        print(f"traced {opts.trace}: one epoch of {opts.steps} steps")
        return
    run, cap = {}, {}
    for p in PATHS:
        run[p], cap[p] = make_path(p, dev, pool, opts.steps)
        for _ in range(opts.warmup):
            run[p]()
    tapes = {p: (None if cap[p]() is None or cap[p]().tape is None else [t[0] for t in cap[p]().tape])
             for p in PATHS}
    in_graph = {p: bool(cap[p]() is not None and cap[p]().adam_in_graph) for p in PATHS}
    got = {p: [] for p in PATHS}
    for r in range(opts.rounds):
        for p in (PATHS if r % 2 == 0 else PATHS[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run[p]()
            got[p].append((time.perf_counter() - t0) / opts.steps * 1e6)
    med = {p: statistics.median(got[p]) for p in PATHS}
    out = [f"# {torch.cuda.get_device_name(0)}; captured Potes train step through train_epoch, batch ({B},{C},{T}),",
           "# method 'durratiomixup', use_sched=True (OneCycleLR), grad_clip=0.1, resident batches; one process,",
           f"# {opts.warmup} warm-up epochs per path, then {opts.rounds} rounds with the paths alternating; one unit = one train_epoch of",
           f"# {opts.steps} steps, host clock around the call (it ends in a device-to-host copy).",
           "# us per step: median [min .. max].  The host is shared: compare medians with the spread in mind.",
           "# path  us per step                      update in the step  direct launches  what"]
    for p in PATHS:
        v = got[p]
        out.append(f"  {p:5s} {med[p]:8.1f} [{min(v):8.1f} .. {max(v):8.1f}]   {'yes' if in_graph[p] else 'no ':3s}"
                   f"                 {'yes' if tapes[p] else 'no ':3s}              {LABEL[p]}")
    out.append(f"# the step's fifth direct launch with SGD: {tapes['new'][-1] if tapes['new'] else 'none (graph replay)'}")
    if med["new"] < med["old"]:
        out.append(f"# SGD: the new median is BELOW the old one: {med['old']:.1f} -> {med['new']:.1f} us per step "
                   f"({med['old'] / med['new']:.2f}x); ClipAdam step in this run: {med['adam']:.1f} us")
    else:
        out.append(f"# SGD: the new median is NOT below the old one: {med['old']:.1f} -> {med['new']:.1f} us per step; "
                   f"ClipAdam step in this run: {med['adam']:.1f} us")
    if opts.launches:
        out.append("# kernel dispatches per step (kernel trace of a run of its own per path; from one conv-stack forward")
        out.append("# to the next, median [min .. max] over the steady half of the epoch), and the kernels of one step:")
        for p in PATHS:
            res = launches_per_step(os.path.join(opts.launches, p))
            if res is None:
                out.append(f"  {p:5s} not measured (no trace under {os.path.join(opts.launches, p)})")
                continue
            m, lo, hi, names = res
            out.append(f"  {p:5s} {m:5.1f} [{lo} .. {hi}]")
            out.extend(f"          {n}" for n in names)
    else:
        out.append("# kernel dispatches per step: not measured (no --launches DIR)")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
