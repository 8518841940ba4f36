#!/usr/bin/env python3
"""Conditioning of the batch statistics of the fused BatchNorm + ReLU + MaxPool kernels
(csrc/pcgmix_bnrp.hip): a small block, (8, 64, 1, 250) with a (1, 2) window, fed y ~ N(r sigma, sigma)
for r in {0, 10, 100, 1000} — a batch mean r standard deviations away from zero.  For every r the
maximum error of z (absolute, and as a multiple of the forward tolerance 1e-4 |z| + 2e-5), of invstd
(relative) and of dx (relative to max |dx|) against the float64 restatement of tests/bnrp_ref.py, for the
kernels and for torch's own float32 composition (batch_norm -> relu -> max_pool2d and its autograd) on
the same device.  tests/test_bnrp_edges_gpu.py::test_batch_statistics_far_from_zero asserts the r = 10
and r = 100 rows; r = 1000 is recorded only.

    python profiles/bnrp_conditioning.py [--out profiles/bnrp_conditioning.txt]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "bnrp_conditioning.txt"))
    opts = ap.parse_args()
    import ctypes
    import numpy as np
    import torch
    import torch.nn.functional as F
    import pcgmix_amd  # noqa: F401
    from pcgmix_amd import _lib, models
    import bnrp_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bnrp_conditioning.py needs the GPU")
    dev = torch.device("cuda", 0)
    out = [f"# {torch.cuda.get_device_name(0)}; BatchNorm+ReLU+pool, training mode, (8, 64, 1, 250) window (1, 2), y ~ N(r sigma, sigma),",
           "# sigma = 1.7, against float64.  z: max |diff| and max of |diff| / (1e-4 |z| + 2e-5) (<= 1: inside the forward",
           "# tolerance); invstd: max relative; dx: max |diff| / max |dx|.  hip = the kernels, torch = torch's float32 ops.",
           "#    r   path    z max|diff|   z / tolerance   invstd rel    dx rel      inside the forward tolerance"]
    for r in (0, 10, 100, 1000):
        c = R.conditioning_case(r)
        B, C, H, W, ph, pw = c.shape
        f = R.train_fwd(c.y, c.gamma, c.beta, None, None, c.momentum, c.eps, None, None, None, ph, pw)
        b = R.train_bwd(c.y, c.dz, c.gamma, c.beta, f.mean, f.invstd, ph, pw)
        cl = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).permute(0, 3, 1, 2)   # noqa: E731
        flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1).double().cpu().numpy()                  # noqa: E731
        g, bt = (torch.from_numpy(v.astype(np.float32)).to(dev) for v in (c.gamma, c.beta))
        for path in ("hip", "torch"):
            y = cl(c.y).requires_grad_(True)
            if path == "hip":
                z = models.BNReLUPoolFunction.apply(y, g, bt, None, None, 0.1, c.eps, ph, pw)
            else:
                z = F.max_pool2d(F.relu(F.batch_norm(y, None, None, g, bt, True, 0.1, c.eps)), (ph, pw))
            z.backward(cl(c.dz))
            zerr = np.abs(flat(z) - f.z.reshape(-1))
            ztol = float((zerr / (1e-4 * np.abs(f.z.reshape(-1)) + 2e-5)).max())
            dxe = float(np.abs(flat(y.grad) - b.dx.reshape(-1)).max() / np.abs(b.dx).max())
            if path == "hip":
                mean = torch.empty(C, device=dev)
                istd = torch.empty(C, device=dev)
                lib = _lib.load()
                ws = torch.empty(lib.pcgmix_bnrp_workspace_floats(B, H, W, C), device=dev)
                zz = torch.empty(B * (H // ph) * (W // pw) * C, device=dev)
                yy = y.detach().permute(0, 2, 3, 1).contiguous()
                _lib.check(lib.pcgmix_bnrp_fwd_f32(yy.data_ptr(), g.data_ptr(), bt.data_ptr(), None, None, ctypes.c_float(0.1),
                                                   ctypes.c_float(c.eps), None, None, None, zz.data_ptr(), mean.data_ptr(),
                                                   istd.data_ptr(), ws.data_ptr(), B, H, W, C, ph, pw,
                                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "pcgmix_bnrp_fwd_f32")
                ie = float(np.abs(istd.double().cpu().numpy() / f.invstd - 1).max())
            else:                                          # torch keeps its invstd to itself: its own float32 variance
                v32, _ = torch.var_mean(y.detach(), (0, 2, 3), unbiased=False)
                ie = float(np.abs(torch.rsqrt(v32 + c.eps).double().cpu().numpy() / f.invstd - 1).max())
            line = f"  {r:5d}   {path:5s}   {float(zerr.max()):11.3e}   {ztol:13.3f}   {ie:10.3e}   {dxe:10.3e}   {'yes' if ztol <= 1 else 'NO'}"
            out.append(line)
            print(line, flush=True)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
