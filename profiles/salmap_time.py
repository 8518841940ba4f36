#!/usr/bin/env python3
"""``saliency.saliency_map`` (one kernel and one device-to-host copy behind the input gradient)
against the reference's formulation of the same call written with torch ops on the same device:
autograd backward of the gathered scores, ``conv1d``, and the per-sample Python loop with four
``interpolate`` + ``repeat_interleave`` calls and the copies it implies (``torch_saliency_map``
below; ``saliency.bin_tensor`` is that loop's body).  That is what a user runs today.

Two quantities, both in ONE process with the two paths ALTERNATING inside a round:

  saliency_map        (256, 4, 2500), model 'Potes' (random weights, eval mode): the whole call
  saliency_map_post   (256, 4, 5000): everything behind the backward pass, from a given gradient
                      (the HIP side ends in ``torch.cuda.synchronize()``; the torch side ends in its
                      own copies)

Method: ``--warmup`` calls per path, then ``--rounds`` rounds; host clock around one call, the device
idle when it starts.  Reported: median [min .. max] in ms.  The host is shared with other jobs: read
the spread next to every median.  Acceptance: the HIP median is below the torch median for both.

    python profiles/salmap_time.py [--out profiles/salmap_time.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/salmap_time.py --trace

``--trace`` makes 21 ``saliency_map_post`` calls (and, for scale, 21 ``saliency_post`` calls with 101
taps) at (256, 4, 5000) and at (256, 4, 2500) and times nothing: the kernel times come from the profiler (profiles/salmap_kernel_trace.txt).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BINS = (1, 4, 1, 8)


def torch_post(grad, frames, dev):
    """saliency.py:147-201 with torch ops from a given ``data.grad``."""
    import numpy as np
    import torch
    from pcgmix_amd import saliency
    B, _, T = grad.shape
    sal = grad.abs()
    for s, f in zip(sal, frames):
        s[:, f[4]:] = 0
    sal = sal.sum(1)[:, None, :]
    kernel = torch.tensor([[saliency.gaussian_kernel(*saliency.SALMAP_GAUSS)]], dtype=torch.float32, device=dev)
    sal = torch.nn.functional.conv1d(sal, kernel, padding="same")
    flat = sal.view(B, -1)
    flat -= flat.min(1, keepdim=True)[0]
    flat /= flat.max(1, keepdim=True)[0]
    sal = torch.nan_to_num(sal, nan=0.0)
    sal_bins = torch.zeros((B, 1, T))                       # on the CPU, as the reference keeps it
    values, bounds = [], []
    for i, (d, f) in enumerate(zip(sal, frames)):
        v_d, b_d = [], []
        for k, n in enumerate(BINS):
            new, v, fr = saliency.bin_tensor(d[:, f[k]:f[k + 1]], n, dev)
            sal_bins[i, :, f[k]:f[k + 1]] = new
            v_d += v
            b_d += [int(x) + int(f[k]) for x in fr]
        values.append(np.array(v_d))
        bounds.append(np.array(b_d + [int(f[4])]))
    return sal, sal_bins, values, bounds


def torch_saliency_map(data, tgt, frames, model, dev):
    import torch
    x = data.clone().requires_grad_()
    model.eval()
    out = model(x)
    scores = out.gather(1, tgt.max(1, keepdim=True)[1].view(-1, 1)).squeeze()
    scores.backward(torch.ones_like(scores))
    return torch_post(x.grad, frames, dev) + (out.detach(),)


def timed(fn, rounds, warmup):
    import torch
    res = {}
    for name, f in fn.items():
        for _ in range(warmup):
            res[name] = f()
    got = {name: [] for name in fn}
    for _ in range(rounds):
        for name, f in fn.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            got[name].append((time.perf_counter() - t0) * 1e3)
    return res, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "salmap_time.txt"))
    opts = ap.parse_args()
    import numpy as np
    import torch
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import saliency, synthetic, train_model as tm
    if not torch.cuda.is_available():
        raise SystemExit("salmap_time.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    B = opts.batch
    if opts.trace:
        for T, rate in ((5000, 2000), (2500, 1000)):
            frames = synthetic.make_index_data(B, T, sample_rate=rate, seed=9)[0]
            grad = torch.from_numpy(np.random.RandomState(1).standard_normal((B, 4, T)).astype(np.float32)).to(dev)
            fr32 = torch.from_numpy(frames.astype(np.int32)).to(dev)
            for _ in range(21):
                saliency.saliency_map_post(grad, frames)
                saliency.saliency_post(grad, fr32.data_ptr(), 101)      # get_saliency_maps' kernel, for scale
            torch.cuda.synchronize()
        print(f"traced saliency_map_post: 21 calls at ({B},4,5000) and at ({B},4,2500)")
        return
    out = [f"# {torch.cuda.get_device_name(0)}; saliency.saliency_map (HIP: pcgmix_saliency_map_f32 + one device-to-host copy)",
           "# against the reference's formulation with torch ops on the same device (per-sample loop, interpolate +",
           f"# repeat_interleave, its copies); one process, {opts.warmup} warm-up calls per path, then {opts.rounds} rounds with the two paths",
           "# alternating; host clock around one call.  ms per call: median [min .. max].  The host is shared.",
           "# quantity                          HIP ms                        torch ms                      torch/HIP  HIP < torch  max |diff| map/bins"]
    ok = True

    def report(label, res, got):
        nonlocal ok
        h, t = got["hip"], got["torch"]
        mh, mt = statistics.median(h), statistics.median(t)
        d_map = float((res["hip"][0].reshape(-1) - res["torch"][0].reshape(-1)).abs().max())
        d_bins = float((res["hip"][1].reshape(-1).cpu() - res["torch"][1].reshape(-1)).abs().max())
        line = (f"  {label:32s}  {mh:8.3f} [{min(h):8.3f} .. {max(h):8.3f}]  {mt:8.3f} [{min(t):8.3f} .. {max(t):8.3f}]  "
                f"{mt / mh:8.1f}x  {'yes' if mh < mt else 'NO':3s}          {d_map:.1e} / {d_bins:.1e}")
        ok = ok and mh < mt
        out.append(line)
        print(line, flush=True)

    # the whole call, (B, 4, 2500), Potes
    T = 2500
    x, frames, labels, _ = synthetic.make_batch(B, 4, T, sample_rate=1000, seed=7)
    torch.manual_seed(0)
    model = tm.build_model(argparse.Namespace(dataset="PhysioNet", model="Potes", num_channels=4, num_classes=2,
                                              sig_len=T)).to(dev).eval()
    data = torch.from_numpy(x).to(dev)
    tgt = torch.nn.functional.one_hot(torch.from_numpy(labels), 2).to(dev)
    fr = torch.from_numpy(frames)
    report(f"saliency_map ({B},4,{T}) Potes", *timed(
        {"hip": lambda: saliency.saliency_map(data, tgt, fr, model, dev),
         "torch": lambda: torch_saliency_map(data, tgt, frames, model, dev)}, opts.rounds, opts.warmup))

    # behind the backward pass, (B, 4, 5000)
    T = 5000
    frames = synthetic.make_index_data(B, T, sample_rate=2000, seed=9)[0]
    grad = torch.from_numpy(np.random.RandomState(1).standard_normal((B, 4, T)).astype(np.float32)).to(dev)
    report(f"saliency_map_post ({B},4,{T})", *timed(
        {"hip": lambda: saliency.saliency_map_post(grad, frames),
         "torch": lambda: torch_post(grad, frames, dev)}, opts.rounds, opts.warmup))
    nbytes = B * (4 * 4 * T + 2 * 4 * T + 4 * 29)
    out.append(f"# saliency_map_post moves {nbytes / 1e6:.2f} MB at ({B},4,{T}): 4 C T read, 2 x 4 T written per row, 116 B of bins")
    out.append("# acceptance (HIP median below the torch median for both quantities): " + ("met" if ok else "NOT met"))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
