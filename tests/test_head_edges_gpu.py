"""The Potes classifier head (csrc/pcgmix_head.hip, csrc/pcgmix_skinny.hip) at its tile edges, every
entry point through the C ABI, against the float64 restatement of tests/head_ref.py.

  * integer data (head_ref.int_case): every sum a kernel forms is exact in float32 in any order, so
    the split-K planes, z, logits, dz, dW2, db2, db1, dW1, dx and the saliency pair must equal float64
    BIT FOR BIT — with packed dropout masks of 1, 2, 4 and 8 bits, rows that start inside a mask byte,
    exact zeros in z, and every optional pointer NULL in turn;
  * exact inputs, transcendental outputs (head_ref.dyadic_case): z and logits still bit for bit; the
    losses and what follows from them within the limits the project already uses for these kernels
        loss       rtol 1e-5, atol 1e-6                    tests/test_head_gpu.py::test_soft_ce_matches_torch
        gradients  rtol 1e-4, atol 1e-7 + 1e-4 max|ref|    tests/test_head_gpu.py::test_fused_head_loss_equals_head_then_celoss
                                                           (and tests/test_latent1d_gpu.py, tests/test_selc_gpu.py)
        SELC rows and soft labels  1e-5 absolute           tests/test_selc_gpu.py
    taken over unchanged.  The logits of a latent blend with a non-dyadic lam are one rounding of every
    blended feature away from exact: they are held to the gradient limit (lam = 0 and 1: bit for bit);
  * the bit-equalities the code promises: the deferred finalize, latent with lam = 1, uint8 labels
    against the one-hot matrix, a second run, and z / logits of the three fused entry points against
    pcgmix_potes_head_fwd_f32;
  * every output buffer is sentinel-filled and over-allocated: every owned element is written (dx under
    dropped bits and in the last partial column tile, all of dW1, columns 0..188 of every workspace row
    block), no guard element is (the guard behind dW1 is not cleared by the spare blocks);
  * refusals return hipErrorInvalidValue and write nothing.
The shape table is head_ref.HEAD_EDGE (tests/test_head_ref_cpu.py::test_shapes_cover_tile_edges says
what it covers).  Only arguments the ABI documents or refuses are passed."""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import head_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -12345.5                      # no output can hold it: integer data gives integers, the rest is small
SENT_BYTE = 0xA5
GUARD = 64
O = R.HEAD_O
FLOATS = ("scale1", "scale2", "keep", "take", "lam")
_HEAD = "x mask1 scale1 thr1 bits1 w1 b1 mask2 scale2 thr2 w2 b2 "
SPEC = {    # entry point -> its arguments in order (the stream follows)
    "pcgmix_skinny_linear_fwd_f32": "x w1 b1 partial z B K O",
    "pcgmix_potes_head_fwd_f32": _HEAD + "partial z logits B K C",
    "pcgmix_potes_head_bwd_f32": "dlogits zin mask2 scale2 thr2 w2 x mask1 scale1 thr1 bits1 w1 dz dw2 db2 db1 dw1 dx B K C",
    "pcgmix_potes_head_saliency_f32": "x w1 b1 w2 seed partial dz dx B K C",
    "pcgmix_potes_head_loss_fwd_f32": _HEAD + "target partial z logits dz loss small ws dw1 defer kind B K C",
    "pcgmix_potes_head_loss_latent_fwd_f32": _HEAD + "target partial z logits dz loss small ws dw1 kind B K C mix inv lam",
    "pcgmix_potes_head_loss_selc_fwd_f32": _HEAD + "index soft N keep take partial z logits dz loss small ws dw1 defer B K C",
    "pcgmix_potes_head_loss_bwd_f32": "dzin gscale x mask1 scale1 thr1 bits1 w1 small_in small_out dw1 dx dws dloss B K C",
    "pcgmix_soft_ce_fwd_f32": "logits_in target loss B C",
    "pcgmix_soft_ce_bwd_f32": "logits_in target gout dlogits_out B C",
    "pcgmix_selc_fwd_f32": "logits_in index soft N keep take rows loss B C",
    "pcgmix_selc_bwd_f32": "logits_in rows_in gout dlogits_out B C",
}
KEEP, TAKE = float(np.float32(0.9)), float(np.float32(1.0 - 0.9))       # train_model.selc_keep_take(0.9)
NO_MASK1 = dict(mask1=None, scale1=1.0, thr1=0, bits1=8)
NO_MASK2 = dict(mask2=None, scale2=1.0, thr2=0)


def invoke(lib, name, env, **over):
    vals = {**env, **over}
    args = []
    for k in SPEC[name].split():
        v = vals[k]
        if k in FLOATS:
            v = ctypes.c_float(v)
        elif isinstance(v, torch.Tensor):
            v = v.data_ptr()
        args.append(v)
    return getattr(lib, name)(*args, vals["stream"])


def _same(name, got, want, problems):
    """Bit equality (float32 outputs widened to float64 first); a mismatch says where."""
    got, want = got.reshape(-1), want.reshape(-1)
    if got.dtype != torch.uint8:
        got, want = got.double(), want.double()
    if got.shape == want.shape and torch.equal(got, want):
        return
    if got.shape != want.shape:
        problems.append(f"{name}: {got.numel()} elements, want {want.numel()}")
        return
    bad = (got != want).nonzero().flatten()
    i = int(bad[0])
    problems.append(f"{name}: {bad.numel()} of {want.numel()} differ, first at {i} (got {got[i].item()}, "
                    f"want {want[i].item()}), last at {int(bad[-1])}")


def _near_loss(name, got, want, problems):
    """rtol 1e-5, atol 1e-6 (tests/test_head_gpu.py::test_soft_ce_matches_torch)."""
    g, w = float(got.reshape(-1)[0]), float(want)
    print(f"{name}: {g!r} against {w!r}, |diff| {abs(g - w):.3g}")
    if not abs(g - w) <= 1e-6 + 1e-5 * abs(w):
        problems.append(f"{name}: {g!r} against {w!r} outside rtol 1e-5, atol 1e-6")


def _near_grad(name, got, want, problems):
    """rtol 1e-4, atol 1e-7 + 1e-4 max|ref| (tests/test_head_gpu.py::test_fused_head_loss_equals_head_then_celoss)."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    top = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"{name}: max |diff| {err:.3g} of {top:.3g}")
    if not torch.allclose(got, want, rtol=1e-4, atol=1e-7 + 1e-4 * top):
        problems.append(f"{name}: max |diff| {err:.3g} of {top:.3g} outside rtol 1e-4, atol 1e-7 + 1e-4 max|ref|")


def _near_selc(name, got, want, problems):
    """1e-5 absolute (tests/test_selc_gpu.py)."""
    err = float((got.double().reshape(-1) - want.double().reshape(-1)).abs().max())
    print(f"{name}: max |diff| {err:.3g}")
    if not err <= 1e-5:
        problems.append(f"{name}: max |diff| {err:.3g} > 1e-5")


class Run:
    """The inputs of one case on the device, and the sentinel-filled, guarded output buffers of the call
    in preparation.  ``take`` checks ownership and hands the owned parts back on the host."""

    def __init__(self, c, device):
        self.c, self.device, self.lib = c, device, _lib.load()
        up = lambda t: None if t is None else t.to(device).contiguous()   # noqa: E731
        self.env = dict(x=up(c.x), w1=up(c.w1), b1=up(c.b1), w2=up(c.w2), b2=up(c.b2), mask1=up(c.mask1),
                        mask2=up(c.mask2), scale1=c.scale1, thr1=c.thr1, bits1=c.bits1, scale2=c.scale2,
                        thr2=c.thr2, dlogits=up(c.dlogits), seed=up(c.seed), target=up(c.target), B=c.B, K=c.K,
                        C=c.C, O=O, N=c.N, keep=KEEP, take=TAKE, defer=0, kind=0, dws=None, dloss=None,
                        stream=ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        if c.mask1 is None:
            self.env.update(NO_MASK1)
            self.env.update(NO_MASK2)
        self.pending = {}                # key -> (buffer, owned elements, how)

    def out(self, key, n, how="all", fill=None, dtype=torch.float32):
        """A guarded output.  how: 'all' = every owned element must be written; 'ws' = columns 0..188 of
        every 192-float row block and nothing else; 'pre' = pre-filled with ``fill`` (an accumulator or an
        in-place table: only the guard is checked); 'none' = the call must not write it at all."""
        sent = SENT_BYTE if dtype == torch.uint8 else SENT
        buf = torch.full((n + GUARD,), sent, dtype=dtype, device=self.device)
        if fill is not None:
            buf[:n] = fill.reshape(-1).to(self.device) if isinstance(fill, torch.Tensor) else fill
        self.env[key] = buf
        self.pending[key] = (buf, n, how)
        return buf

    def keep_as_output(self, key, buf, n, how):
        self.env[key] = buf
        self.pending[key] = (buf, n, how)

    def outs(self, spec):
        for key, n in spec.items():
            self.out(key, n, "ws" if key == "ws" else "all")

    def call(self, name, **over):
        _lib.check(invoke(self.lib, name, self.env, **over), name)

    def take(self, tag, problems):
        """name -> owned part on the host; self.dev keeps the device buffers (guard included)."""
        torch.cuda.synchronize()
        got, self.dev = {}, {}
        for key, (buf, n, how) in self.pending.items():
            host = buf.cpu()
            sent = SENT_BYTE if host.dtype == torch.uint8 else SENT
            own, guard = host[:n], host[n:]
            if not bool((guard == sent).all()):
                problems.append(f"{tag}: {key}: guard elements behind the buffer were written")
            if how == "all":
                left = int((own == sent).sum())
                if left:
                    problems.append(f"{tag}: {key}: {left} of {n} owned elements were not written")
            elif how == "ws":
                blocks = own.view(-1, R.TL_STRIDE)
                left = int((blocks[:, :R.TL_USED] == sent).sum())
                if left:
                    problems.append(f"{tag}: ws: {left} of the columns 0..188 were not written")
                if not bool((blocks[:, R.TL_USED:] == sent).all()):
                    problems.append(f"{tag}: ws: columns behind 188 were written")
            elif how == "none":
                if not bool((own == sent).all()):
                    problems.append(f"{tag}: {key} was written")
            got[key], self.dev[key] = own, buf
        self.pending = {}
        return got


def _ref_args(c, **over):
    v = dict(x=c.x, mask1=c.mask1, scale1=c.scale1, thr1=c.thr1, bits1=c.bits1, w1=c.w1, b1=c.b1, mask2=c.mask2,
             scale2=c.scale2, thr2=c.thr2, w2=c.w2, b2=c.b2)
    v.update(over)
    return tuple(v[k] for k in _HEAD.split())


def _fwd_sizes(c):
    return dict(partial=c.KS * c.B * O, z=c.B * O, logits=c.B * c.C)


def _n_small(c):
    return c.C * O + c.C + O


# ---- exact: integer data ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.HEAD_EDGE, ids=R.EDGE_IDS)
def test_integer_exact(shape, device):
    """torch.equal against float64 for the split-K product (O = 8, 16, 20; 12, 32, 33 refused), the head
    forward (all masks, b1 / b2 NULL, either mask alone, none), the head backward (all outputs; db1 / db2
    NULL; dx NULL; dw1 NULL with a poisoned x, which is documented as not read then), the saliency form
    (its dz also against (z > 0) * (seed W2) formed from pcgmix_potes_head_fwd_f32's own z) and
    pcgmix_potes_head_loss_bwd_f32 fed an integer dz and gscale = 2."""
    c = R.int_case(*shape)
    r = Run(c, device)
    B, K, C, KS = c.B, c.K, c.C, c.KS
    assert r.lib.pcgmix_skinny_linear_splits(B, K) == KS
    assert r.lib.pcgmix_potes_head_loss_workspace_floats(B) == c.nrb * R.TL_STRIDE
    P = []
    # the split-K product on its own
    for width in (8, 16, 20):
        r.outs(dict(partial=KS * B * width, z=B * width))
        r.call("pcgmix_skinny_linear_fwd_f32", w1=r.env["w1"][:width], b1=r.env["b1"][:width], O=width)
        got = r.take(f"skinny O={width}", P)
        partial, z = R.skinny_fwd(c.x, c.w1[:width], c.b1[:width])
        _same(f"skinny O={width}: partial", got["partial"], partial, P)
        _same(f"skinny O={width}: z", got["z"], z, P)
    plain_partial = partial
    for width in (12, 32, 33):
        r.out("partial", KS * B * 33, "none")
        r.out("z", B * 33, "none")
        assert invoke(r.lib, "pcgmix_skinny_linear_fwd_f32", r.env, O=width) == INVALID, width
        r.take(f"skinny O={width} (refused)", P)
    # forward
    variants = [("all", {}), ("b1, b2 NULL", dict(b1=None, b2=None)), ("no masks", {**NO_MASK1, **NO_MASK2})]
    if c.mask1 is not None:
        variants += [("mask1 only", dict(NO_MASK2)), ("mask2 only", dict(NO_MASK1))]
    for tag, over in variants:
        r.outs(_fwd_sizes(c))
        r.call("pcgmix_potes_head_fwd_f32", **over)
        got = r.take(f"fwd, {tag}", P)
        ref = c.ref if tag == "all" else R.head_fwd(*_ref_args(c, **over))
        for k in ("partial", "z", "logits"):
            _same(f"fwd, {tag}: {k}", got[k], getattr(ref, k), P)
        if tag == "no masks":
            z_eval = got["z"]
    # backward: the same values whichever optional output is left out
    zin = c.ref.z.float().to(device)
    sizes = dict(dz=B * O, dw2=C * O, db2=C, db1=O, dw1=O * K, dx=B * K)
    poisoned = torch.full((B, K), float("nan"), device=device)
    for tag, over in (("all", {}), ("db1, db2 NULL", dict(db1=None, db2=None)), ("dx NULL", dict(dx=None)),
                      ("dw1 NULL, x poisoned", dict(dw1=None, x=poisoned))):
        r.outs({k: n for k, n in sizes.items() if k not in over})
        r.call("pcgmix_potes_head_bwd_f32", zin=zin, **over)
        got = r.take(f"bwd, {tag}", P)
        for k in got:
            _same(f"bwd, {tag}: {k}", got[k], getattr(c.bwd, k), P)
    # saliency
    r.outs(dict(partial=KS * B * O, dz=B * O, dx=B * K))
    r.call("pcgmix_potes_head_saliency_f32")
    got = r.take("saliency", P)
    _same("saliency: partial", got["partial"], plain_partial, P)
    _same("saliency: dz", got["dz"], c.sal.dz, P)
    _same("saliency: dx", got["dx"], c.sal.dx, P)
    _same("saliency: dz against (z > 0) * (seed W2) from the forward's z", got["dz"],
          (z_eval.double().view(B, O) > 0).double() * (c.seed.double() @ c.w2.double()), P)
    # the feature pass of the fused form: integer dz, power-of-two gscale
    small_in = R.small_of(c.bwd.dw2, c.bwd.db2, c.bwd.db1).float().to(device)
    dzin = c.bwd.dz.float().to(device)
    gscale = torch.tensor([R.GSCALE], device=device)
    ref = R.head_loss_bwd(c.bwd.dz, R.GSCALE, *_ref_args(c)[:6], small_in)
    ref1 = R.head_loss_bwd(c.bwd.dz, None, *_ref_args(c)[:6], None)
    for tag, over, want in (("gscale 2", {}, ref), ("gscale, small NULL", dict(gscale=None, small_in=None, small_out=None), ref1),
                            ("dx NULL", dict(dx=None), ref), ("dw1 NULL, x poisoned", dict(dw1=None, x=poisoned), ref)):
        for k, n, how in (("small_out", _n_small(c), "all"), ("dw1", O * K, "pre"), ("dx", B * K, "all")):
            if k not in over:
                r.out(k, n, how, fill=0.0 if how == "pre" else None)
        r.call("pcgmix_potes_head_loss_bwd_f32", **{**dict(dzin=dzin, gscale=gscale, small_in=small_in), **over})
        got = r.take(f"loss_bwd, {tag}", P)
        for k in got:
            _same(f"loss_bwd, {tag}: {k}", got[k], getattr(want, "small" if k == "small_out" else k), P)
    assert not P, "\n".join(P)


# ---- exact inputs, transcendental outputs -------------------------------------------------------
_LOSS_OUT = ("partial", "z", "logits", "dz", "loss", "small", "ws", "dw1")


def _loss_sizes(c):
    return dict(partial=c.KS * c.B * O, z=c.B * O, logits=c.B * c.C, dz=c.B * O, loss=1, small=_n_small(c),
                ws=c.nrb * R.TL_STRIDE, dw1=O * c.K)


def _fused_forward(r, name, tag, P, defer=False, **over):
    """One fused forward into fresh guarded buffers: (host outputs, device buffers)."""
    c = r.c
    r.outs(_loss_sizes(c))
    if defer:                            # the forward then writes neither the loss nor the small gradients
        for k in ("loss", "small"):
            r.pending[k] = (r.pending[k][0], r.pending[k][1], "none")
        over = {**over, "defer": 1}
    r.call(name, **over)
    got = r.take(tag, P)
    if bool(got["dw1"].any()):
        P.append(f"{tag}: the dW1 buffer is not cleared")
    return got, r.dev


def _fused_backward(r, tag, P, dev, gscale, deferred=False, **over):
    """pcgmix_potes_head_loss_bwd_f32 behind a fused forward (dW1 accumulates into the buffer it cleared)."""
    c = r.c
    r.out("small_out", _n_small(c))
    r.out("dx", c.B * c.K)
    r.keep_as_output("dw1", dev["dw1"], O * c.K, "all")
    extra = {}
    if deferred:
        r.out("dloss", 1)
        extra = dict(dws=dev["ws"], small_in=None)
    else:
        extra = dict(small_in=dev["small"], dloss=None)
    r.call("pcgmix_potes_head_loss_bwd_f32", dzin=dev["dz"], gscale=gscale, **extra, **over)
    return r.take(tag, P)


def _check_fused(tag, c, got, back, ref, gs, P):
    for k in ("partial", "z", "logits"):
        _same(f"{tag}: {k}", got[k], getattr(ref, k), P)
    _near_loss(f"{tag}: loss", got["loss"], ref.loss, P)
    _near_grad(f"{tag}: dz", got["dz"], ref.dz, P)
    nw = c.C * O
    for part, lo, hi in (("dW2", 0, nw), ("db2", nw, nw + c.C), ("db1", nw + c.C, nw + c.C + O)):
        _near_grad(f"{tag}: small {part}", got["small"][lo:hi], ref.small[lo:hi], P)
    fb = R.head_loss_bwd(ref.dz, gs, *_ref_args(c)[:6], ref.small)
    _near_grad(f"{tag}: dW1", back["dw1"], fb.dw1, P)
    _near_grad(f"{tag}: dx", back["dx"], fb.dx, P)
    for part, lo, hi in (("dW2", 0, nw), ("db2", nw, nw + c.C), ("db1", nw + c.C, nw + c.C + O)):
        _near_grad(f"{tag}: small_out {part}", back["small_out"][lo:hi], fb.small[lo:hi], P)
    if c.mask1 is not None:              # dx is exactly 0 under a dropped bit, whatever the rounding elsewhere
        gone = ~R.keep_vec(c.mask1, c.B * c.K, c.bits1, c.thr1)
        wrong = int((back["dx"][gone] != 0).sum())
        if wrong:
            P.append(f"{tag}: dx is not 0 at {wrong} of {int(gone.sum())} dropped elements")


def _same_bits(tag, a, b, keys, P):
    for k in keys:
        _same(f"{tag}: {k}", a[k], b[k], P)


@pytest.mark.parametrize("shape", R.HEAD_EDGE, ids=R.EDGE_IDS)
def test_losses(shape, device):
    """dyadic_case: the loss kernels on their own (soft and hard targets, SELC with one index outside
    [0,N)), the fused head + CE with both target kinds and the fused head + SELC, each followed by the
    feature pass with a loss gradient of 0.37 — z and logits bit for bit, the rest within the project's
    limits — and the promised bit-equalities: deferred finalize, uint8 labels against one-hot rows, a
    second run, z / logits against pcgmix_potes_head_fwd_f32."""
    c = R.dyadic_case(*shape)
    r = Run(c, device)
    B, K, C = c.B, c.K, c.C
    P = []
    gout = torch.tensor([0.37], device=device)
    logits_in = c.ref.logits.float().to(device)
    assert torch.equal(logits_in.cpu().double(), c.ref.logits)              # exact in float32
    onehot = torch.nn.functional.one_hot(c.labels.long(), C).float().to(device)
    labels = c.labels.to(device)
    index = c.index.to(device)
    # --- soft-target CE alone
    for tag, tgt in (("soft", r.env["target"]), ("hard", onehot)):
        r.outs(dict(loss=1))
        r.call("pcgmix_soft_ce_fwd_f32", logits_in=logits_in, target=tgt)
        r.out("dlogits_out", B * C)
        r.call("pcgmix_soft_ce_bwd_f32", logits_in=logits_in, target=tgt, gout=gout)
        got = r.take(f"soft_ce, {tag}", P)
        _near_loss(f"soft_ce, {tag}: loss", got["loss"], R.soft_ce(c.ref.logits, tgt), P)
        _near_grad(f"soft_ce, {tag}: dlogits", got["dlogits_out"], R.soft_ce_bwd(c.ref.logits, tgt, 0.37), P)
    # --- SELC alone
    want_loss, want_rows, want_soft = R.selc(c.ref.logits, c.index, c.soft, KEEP, TAKE)
    runs = []
    for _ in range(2):
        r.out("soft", c.N * C, "pre", fill=c.soft)
        r.outs(dict(rows=B * C, loss=1))
        r.call("pcgmix_selc_fwd_f32", logits_in=logits_in, index=index)
        got = r.take("selc", P)
        r.out("dlogits_out", B * C)
        r.call("pcgmix_selc_bwd_f32", logits_in=logits_in, rows_in=r.dev["rows"], gout=gout)
        got.update(r.take("selc backward", P))
        runs.append(got)
    got = runs[0]
    _same_bits("selc, second run", runs[1], got, got.keys(), P)
    _near_loss("selc: loss", got["loss"], want_loss, P)
    _near_selc("selc: rows", got["rows"], want_rows, P)
    _near_selc("selc: soft labels", got["soft"], want_soft, P)
    skipped = sorted(set(range(c.N)) - {int(i) for i in c.index.tolist()})
    _same("selc: soft rows no batch row names", got["soft"].view(c.N, C)[skipped], c.soft[skipped], P)
    _same("selc: the row of the index outside [0,N)", got["rows"].view(B, C)[B // 2], torch.zeros(C), P)
    _near_grad("selc: dlogits", got["dlogits_out"], R.soft_ce_bwd(c.ref.logits, want_rows, 0.37), P)
    # --- the plain forward, for the z / logits equalities
    r.outs(_fwd_sizes(c))
    r.call("pcgmix_potes_head_fwd_f32")
    plain = r.take("fwd", P)
    # --- fused head + CE: soft targets, uint8 labels, the one-hot rows of the same labels
    keys_f, keys_b = _LOSS_OUT, ("small_out", "dw1", "dx")
    res = {}
    for tag, over, tgt, kind in (("soft targets", {}, c.target, 0), ("uint8 labels", dict(target=labels, kind=1), c.labels, 1),
                                 ("one-hot rows", dict(target=onehot), onehot.cpu(), 0)):
        name = "pcgmix_potes_head_loss_fwd_f32"
        got, dev = _fused_forward(r, name, f"loss_fwd, {tag}", P, **over)
        back = _fused_backward(r, f"loss_bwd, {tag}", P, dev, gout)
        ref = R.head_loss(*_ref_args(c), tgt, kind)
        _check_fused(f"head + CE, {tag}", c, got, back, ref, 0.37, P)
        _same_bits(f"head + CE, {tag}: against pcgmix_potes_head_fwd_f32", got, plain, ("partial", "z", "logits"), P)
        res[tag] = (got, back)
        # a second run, and the finalize left to the backward: the same bits everywhere
        got2, dev2 = _fused_forward(r, name, f"loss_fwd, {tag}, second run", P, **over)
        back2 = _fused_backward(r, f"loss_bwd, {tag}, second run", P, dev2, gout)
        _same_bits(f"head + CE, {tag}: second run", got2, got, keys_f, P)
        _same_bits(f"head + CE, {tag}: second run", back2, back, keys_b, P)
        got3, dev3 = _fused_forward(r, name, f"loss_fwd, {tag}, deferred", P, defer=True, **over)
        back3 = _fused_backward(r, f"loss_bwd, {tag}, deferred", P, dev3, gout, deferred=True)
        _same_bits(f"head + CE, {tag}: deferred finalize", got3, got, [k for k in keys_f if k not in ("loss", "small")], P)
        _same_bits(f"head + CE, {tag}: deferred finalize", back3, back, keys_b, P)
        _same(f"head + CE, {tag}: deferred finalize: loss", back3["dloss"], got["loss"], P)
    for a, b in zip(res["uint8 labels"], res["one-hot rows"]):
        _same_bits("uint8 labels against one-hot rows", a, b, a.keys(), P)
    # --- fused head + SELC
    name = "pcgmix_potes_head_loss_selc_fwd_f32"
    ref = R.head_loss(*_ref_args(c), None, 0, selc_args=(c.index, c.soft, KEEP, TAKE))
    first = None
    for tag, defer in (("", False), (", second run", False), (", deferred", True)):
        r.out("soft", c.N * C, "pre", fill=c.soft)
        got, dev = _fused_forward(r, name, f"selc_fwd{tag}", P, defer=defer, index=index)
        back = _fused_backward(r, f"selc loss_bwd{tag}", P, dev, gout, deferred=defer)
        if first is None:
            first = (got, back)
            _check_fused("head + SELC", c, got, back, ref, 0.37, P)
            _near_selc("head + SELC: soft labels", got["soft"], ref.soft, P)
            _same("head + SELC: soft rows no batch row names", got["soft"].view(c.N, C)[skipped], c.soft[skipped], P)
            _same_bits("head + SELC: against pcgmix_potes_head_fwd_f32", got, plain, ("partial", "z", "logits"), P)
        else:
            skip = ("loss", "small") if defer else ()
            _same_bits(f"head + SELC{tag}", got, first[0], [k for k in got if k not in skip], P)
            _same_bits(f"head + SELC{tag}", back, first[1], keys_b, P)
            if defer:
                _same(f"head + SELC{tag}: loss", back["dloss"], first[0]["loss"], P)
    assert not P, "\n".join(P)


@pytest.mark.parametrize("shape", R.HEAD_EDGE, ids=R.EDGE_IDS)
def test_latent(shape, device):
    """pcgmix_potes_head_loss_latent_fwd_f32 and the feature pass behind it for lam = 0, a non-dyadic lam
    and lam = 1, with the identity, a same-label shuffle and a permutation with fixed points (partners in
    later and in earlier row blocks wherever B > 4).  z bit for bit; logits bit for bit at lam = 0 and 1;
    lam = 1 gives every bit of the plain entry point."""
    c = R.dyadic_case(*shape)
    r = Run(c, device)
    P = []
    gout = torch.tensor([0.37], device=device)
    labels = c.labels.to(device)
    plain = {}
    for kind, over in ((0, {}), (1, dict(target=labels, kind=1))):
        got, dev = _fused_forward(r, "pcgmix_potes_head_loss_fwd_f32", f"loss_fwd, kind {kind}", P, **over)
        plain[kind] = (got, _fused_backward(r, f"loss_bwd, kind {kind}", P, dev, gout))
    for name, mix in c.perms.items():
        kind = 1 if name == "same-label shuffle" else 0
        over = dict(target=labels, kind=1) if kind else {}
        inv = R.inverse(mix)
        for lam in (0.0, 0.3, 1.0):
            tag = f"latent, {name}, lam {lam}"
            got, dev = _fused_forward(r, "pcgmix_potes_head_loss_latent_fwd_f32", tag, P, mix=mix.to(device),
                                      inv=inv.to(device), lam=lam, **over)
            back = _fused_backward(r, tag + ", backward", P, dev, gout)
            ref = R.head_loss(*_ref_args(c), c.labels if kind else c.target, kind, mix, inv, lam)
            if lam == 0.3:               # blended features are rounded once: not exact any more, so the
                _near_grad(f"{tag}: logits", got["logits"], ref.logits, P)      # bit comparison below is
                ref.logits = got["logits"].double().view(c.B, c.C)              # given the kernel's own
            _check_fused(tag, c, got, back, ref, 0.37, P)
            if lam == 0.3:               # a second run: the same bits
                got2, dev2 = _fused_forward(r, "pcgmix_potes_head_loss_latent_fwd_f32", tag + ", second run", P,
                                            mix=mix.to(device), inv=inv.to(device), lam=lam, **over)
                back2 = _fused_backward(r, tag + ", second run, backward", P, dev2, gout)
                _same_bits(f"{tag}: second run", got2, got, _LOSS_OUT, P)
                _same_bits(f"{tag}: second run", back2, back, ("small_out", "dw1", "dx"), P)
            if lam == 1.0:
                _same_bits(f"{tag}: against the plain entry point", got, plain[kind][0], _LOSS_OUT, P)
                _same_bits(f"{tag}: against the plain entry point", back, plain[kind][1], ("small_out", "dw1", "dx"), P)
    assert not P, "\n".join(P)


# ---- refusals -----------------------------------------------------------------------------------
_REQUIRED = {
    "pcgmix_skinny_linear_fwd_f32": "x w1 partial z",
    "pcgmix_potes_head_fwd_f32": "x w1 w2 partial z logits",
    "pcgmix_potes_head_bwd_f32": "dlogits zin w2 x w1 dz dw2",
    "pcgmix_potes_head_saliency_f32": "x w1 w2 seed partial dz dx",
    "pcgmix_potes_head_loss_fwd_f32": "x w1 w2 target partial z logits dz loss small ws",
    "pcgmix_potes_head_loss_latent_fwd_f32": "x w1 w2 target partial z logits dz loss small ws mix inv",
    "pcgmix_potes_head_loss_selc_fwd_f32": "x w1 w2 index soft partial z logits dz loss small ws",
    "pcgmix_potes_head_loss_bwd_f32": "dzin x w1",
    "pcgmix_soft_ce_fwd_f32": "logits_in target loss",
    "pcgmix_soft_ce_bwd_f32": "logits_in target gout dlogits_out",
    "pcgmix_selc_fwd_f32": "logits_in index soft rows loss",
    "pcgmix_selc_bwd_f32": "logits_in rows_in gout dlogits_out",
}
_FORWARDS = ("pcgmix_potes_head_fwd_f32", "pcgmix_potes_head_loss_fwd_f32", "pcgmix_potes_head_loss_latent_fwd_f32",
             "pcgmix_potes_head_loss_selc_fwd_f32")
_PRODUCT = _FORWARDS + ("pcgmix_skinny_linear_fwd_f32", "pcgmix_potes_head_saliency_f32")      # x, w1: 16-byte aligned
_FEATURE = ("pcgmix_potes_head_bwd_f32", "pcgmix_potes_head_loss_bwd_f32")
_HEADS = _PRODUCT[:4] + ("pcgmix_potes_head_saliency_f32",) + _FEATURE
_TAKES_DZ = _FORWARDS[1:] + ("pcgmix_potes_head_saliency_f32",) + _FEATURE                     # dz: 16-byte aligned


def test_refusals_leave_outputs_untouched(device):
    """hipErrorInvalidValue and not one sentinel touched for: K % 4 != 0, B = 0, C in {0, 9}, bits in
    {0, 3, 16} with a mask, x / w1 / dz off by one float, mask1 off by one byte, target_kind = 2, lam
    outside [0, 1] (NaN included), O not in {8, 16, 20}, every required pointer NULL in turn, and both
    of dw1 / dx NULL.  (A mask with O != 20 cannot be expressed through the C ABI: the only entry point
    that takes O takes no mask.)  The unchanged arguments are then accepted."""
    c = R.int_case(5, 68, 2, 1, 1)
    r = Run(c, device)
    B, K, C = c.B, c.K, c.C
    lib = r.lib
    n = max(c.KS * B * 33, B * K, O * K, c.nrb * R.TL_STRIDE) + 8
    outs = ("partial", "z", "logits", "dz", "dw2", "db2", "db1", "dw1", "dx", "loss", "small", "ws", "small_out",
            "dloss", "dlogits_out", "rows")
    bufs = {k: torch.full((n,), SENT, device=device) for k in outs}
    bufs["soft"] = torch.full((c.N * C + 8,), SENT, device=device)         # read and written in place
    spare = torch.zeros(n, device=device)                                   # inputs some entry points need
    env = {**r.env, **bufs, "zin": spare, "dzin": spare, "small_in": spare, "gscale": None, "logits_in": spare,
           "rows_in": spare, "gout": spare, "index": c.index.to(device), "mix": c.perms["identity"].to(device),
           "inv": c.perms["identity"].to(device), "lam": 0.5, "dws": None, "dloss": None}

    def refused(name, why, **over):
        assert invoke(lib, name, env, **over) == INVALID, (name, why)

    off1 = lambda t: t.reshape(-1)[1:]   # noqa: E731   (never read: the call is refused)
    for name in SPEC:
        refused(name, "B = 0", B=0)
        for arg in _REQUIRED[name].split():
            refused(name, f"{arg} NULL", **{arg: None})
    for name in _HEADS:
        refused(name, "K = 66", K=66)
        refused(name, "K = 0", K=0)
        for bad in (0, 9):
            refused(name, f"C = {bad}", C=bad)
    for name in ("pcgmix_soft_ce_fwd_f32", "pcgmix_soft_ce_bwd_f32", "pcgmix_selc_fwd_f32", "pcgmix_selc_bwd_f32"):
        refused(name, "C = 0", C=0)
    refused("pcgmix_skinny_linear_fwd_f32", "K = 66", K=66)
    for width in (0, 12, 32, 33):
        refused("pcgmix_skinny_linear_fwd_f32", f"O = {width}", O=width)
    for name in _FORWARDS + _FEATURE:
        for bad in (0, 3, 16):
            refused(name, f"bits1 = {bad}", bits1=bad)
    for name in _PRODUCT:
        refused(name, "x off by one float", x=off1(env["x"]))
        refused(name, "w1 off by one float", w1=off1(env["w1"]))
    for name in _FORWARDS:
        refused(name, "mask1 off by one byte", mask1=off1(env["mask1"]))
    for name in _TAKES_DZ:
        key = "dzin" if name == "pcgmix_potes_head_loss_bwd_f32" else "dz"
        refused(name, "dz off by one float", **{key: off1(env[key])})
    for name in _FEATURE:
        refused(name, "dw1 and dx NULL", dw1=None, dx=None)
    refused("pcgmix_potes_head_loss_bwd_f32", "small_out without small_in", small_in=None)
    refused("pcgmix_potes_head_loss_bwd_f32", "deferred_ws without deferred_loss", dws=spare, dloss=None)
    refused("pcgmix_potes_head_loss_bwd_f32", "deferred_ws without small_out", dws=spare, dloss=bufs["loss"], small_out=None)
    for name in ("pcgmix_potes_head_loss_fwd_f32", "pcgmix_potes_head_loss_latent_fwd_f32"):
        refused(name, "target_kind = 2", kind=2)
        refused(name, "target_kind = -1", kind=-1)
    for lam in (-0.25, 1.5, float("nan")):
        refused("pcgmix_potes_head_loss_latent_fwd_f32", f"lam = {lam}", lam=lam)
    for name in ("pcgmix_selc_fwd_f32", "pcgmix_potes_head_loss_selc_fwd_f32"):
        refused(name, "N = 0", N=0)
    assert lib.pcgmix_skinny_linear_splits(0, K) == 0 and lib.pcgmix_skinny_linear_splits(B, 0) == 0
    assert lib.pcgmix_potes_head_loss_workspace_floats(0) == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == SENT).all()), k
    # the same arguments, unchanged, are accepted (and what they compute is the reference)
    bufs["soft"][:c.N * C] = c.soft.reshape(-1).to(device)
    for name in _FORWARDS + ("pcgmix_skinny_linear_fwd_f32", "pcgmix_potes_head_saliency_f32"):
        assert invoke(lib, name, env) == 0, name
    torch.cuda.synchronize()
    assert torch.equal(bufs["z"][:B * O].cpu().double(), c.sal.z.reshape(-1))      # the split-K product's, no masks
