#!/usr/bin/env python3
"""Eager Potes ``train_step`` with 1D latentmixup at (256, 4, 5000): fused path, drop-in path, and
the closest thing a tree without the feature can run (``mixup(same)``: a same-label blend of the
whole waveform followed by the fused head).

One leg = one fresh process: model in train mode (both dropouts live), ClipAdam + OneCycleLR, the
batch resident on the device, ``--warmup`` steps, then ``--steps`` steps between two device
synchronisations; prints ``RESULT <label> <us per step>``.

    python profiles/probes/latent1d_time.py --method latentmixup                  # fused
    python profiles/probes/latent1d_time.py --method latentmixup --dropin         # augment() + 'second'
    python profiles/probes/latent1d_time.py --method "mixup(same)" --root OTHER_TREE

``--all`` runs the three legs alternately, ``--repeat`` times each, as child processes (each under
its own time limit; the first failure ends the run) and writes their figures with the spread to
``--out`` (default profiles/r6_latent1d_time.txt).  ``--parent DIR`` is a checkout of the commit
before the feature, built, for leg (a); without it leg (a) runs on this tree (``mixup(same)`` is
unchanged by the feature).

    python profiles/probes/latent1d_time.py --all --parent DIR

Under rocprofv3 (kernel times, launch counts), a run of its own, program after ``--``:

    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/probes/latent1d_time.py \\
        --method latentmixup --steps 20 --warmup 0
"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
B, C, T = 256, 4, 5000


def leg(opts):
    root = os.path.abspath(opts.root) if opts.root else ROOT
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import synthetic, train_model as tm
    dev = torch.device("cuda", 0)
    args = argparse.Namespace(dataset="PhysioNet", model="Potes", method=opts.method, num_epochs=2,
                              batch_size=B, op="adam", use_sched=True, lr_max=0.01, weight_decay=1e-4,
                              grad_clip=0.1, seed=4, seed_fix=4, num_classes=2, num_channels=C, sig_len=T,
                              depth=0, num_steps=opts.steps + opts.warmup + 1, sample_rate=2000)
    if opts.dropin:
        args.latent_fused = False
    x, frames, labels, wav = synthetic.make_batch(B, C, T, sample_rate=2000, seed=3)
    batch = (torch.from_numpy(x).to(dev), torch.from_numpy(labels), torch.from_numpy(frames), wav,
             torch.ones(B, dtype=torch.long), torch.arange(B))
    torch.manual_seed(0)
    net = tm.build_model(args).to(dev).train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(labels, 2, es=args.num_epochs + 1, device=dev)
    sc = tm.step_counter_class()
    np.random.seed(1)
    for _ in range(opts.warmup):
        tm.train_step(args, net, batch, dev, opt, sched, crit, 1, sc)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(opts.steps):
        loss = tm.train_step(args, net, batch, dev, opt, sched, crit, 1, sc)
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / opts.steps * 1e6
    assert bool(torch.isfinite(loss)), "loss is not finite"
    print(f"RESULT {opts.label or opts.method} {us:.2f}", flush=True)


def run_all(opts):
    me = os.path.abspath(__file__)
    legs = (("a", "parent tree, mixup(same) + fused head" if opts.parent else "this tree, mixup(same) + fused head",
             ["--method", "mixup(same)"] + (["--root", opts.parent] if opts.parent else [])),
            ("b", "this tree, latentmixup fused (blend inside the tail kernel)", ["--method", "latentmixup"]),
            ("c", "this tree, latentmixup drop-in (augment() + model(h, 1, 'second'))",
             ["--method", "latentmixup", "--dropin"]))
    got = {k: [] for k, _, _ in legs}
    for r in range(opts.repeat):
        for key, _what, extra in legs:
            cmd = [sys.executable, me, "--steps", str(opts.steps), "--warmup", str(opts.warmup),
                   "--label", key] + extra
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if res.returncode != 0:
                sys.stderr.write(res.stdout + res.stderr)
                raise SystemExit(f"leg {key} (round {r}) failed with {res.returncode}: stopping")
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            got[key].append(float(line.split()[-1]))
            print(f"round {r} {line}", flush=True)
    import statistics
    import torch
    out = [f"# {torch.cuda.get_device_name(0)}; eager train_step, Potes (train mode, dropout on), ClipAdam + OneCycleLR,",
           f"# ({B}, {C}, {T}) batch resident on the device; {opts.warmup} warm-up steps, then {opts.steps} steps between two",
           f"# device synchronisations; legs alternated, {opts.repeat} fresh processes each.  us per step.",
           "# leg  median     min     max   spread(max-min)  runs"]
    for key, what, _ in legs:
        v = got[key]
        out.append(f"  ({key})  {statistics.median(v):7.1f} {min(v):7.1f} {max(v):7.1f}   {max(v) - min(v):7.1f}          "
                   f"{' '.join(f'{t:.1f}' for t in v)}   {what}")
    a, b, c = (statistics.median(got[k]) for k in "abc")
    spread_a = max(got["a"]) - min(got["a"])
    out.append(f"# (b) - (a) = {b - a:+.1f} us; (a)'s own run-to-run spread {spread_a:.1f} us -> "
               f"(b) <= (a) + spread: {'yes' if b <= a + spread_a else 'NO'}")
    out.append(f"# (c) - (b) = {c - b:+.1f} us per step saved by blending inside the tail kernel")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="latentmixup")
    ap.add_argument("--dropin", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--label", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r6_latent1d_time.txt"))
    opts = ap.parse_args()
    if opts.all:
        run_all(opts)
    else:
        leg(opts)


if __name__ == "__main__":
    main()
