"""The fused BatchNorm + ReLU + MaxPool kernels (csrc/pcgmix_bnrp.hip) at their block edges, all four
entry points through the C ABI, against the float64 restatement of tests/bnrp_ref.py.

  * eval_int_case and train_int_case: every product and sum is exact in float32, so z, mean, invstd,
    both running statistics, dbeta, dgamma, coef and (eval, and training with n a power of two) dx must
    equal float64 BIT FOR BIT, planted ties included; dx with any other n is held, element by element,
    to 2^-21 |scale| (|dy| + |c1| + |xhat c2|) (derivation: bnrp_ref.train_int_case);
  * margin_case: Gaussian data with no ReLU / arg-max decision within 2e-3 of a tie, so EVERY element is
    held to the limits of tests/test_bnrp_gpu.py — forward rtol 1e-4 / atol 2e-5, statistics rtol 1e-5 /
    atol 1e-6, gradients 1e-4 max|ref| + 1e-6 — and none is excused;
  * every output is over-allocated and sentinel-filled: every owned element is written, no guard element
    is; the workspace is exactly pcgmix_bnrp_workspace_floats long with a guard behind it;
  * every optional pointer NULL in turn (one omission: the Gaussian eval case without conv_bias on the two
    capped shapes, which the exact eval case covers there); eval dx zeros are +0.0 by bit pattern; a second run gives the
    same bits; refusals return hipErrorInvalidValue and write nothing; the autograd Functions give the
    bits of the raw calls;
  * a NaN or +inf in y reaches z as torch's float32 composition lets it (forward only), and the
    batch statistics stay within the forward tolerance for a batch mean of 10 and 100 standard
    deviations wherever torch's float32 composition does.
The shapes are bnrp_ref.BNRP_EDGE (tests/test_bnrp_ref_cpu.py::test_shapes_cover_the_block_edges says what
they cover).  Activations of 2^31 elements and more, which take the AnyWindow kernels through the
`fits` test of with_window, are not allocated: those loops run here through the generic windows (1,4),
(2,1), (3,2), (1,3), (2,3).  Only arguments the header documents or refuses are passed."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, models

import bnrp_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -12345.5                      # no output can hold it
SENT_INT = -777
GUARD = 64                           # floats behind every per-channel output (the finalize blocks have 16 channel lanes)
WS_GUARD = 4096                      # two more blocks' partials of the widest row
MAX_SLACK = 1 << 20
SIG = {    # entry point -> its arguments in order (the stream follows)
    "pcgmix_bnrp_fwd_f32": "y gamma beta running_mean running_var momentum eps mean_shift batches_tracked skip z mean "
                           "invstd ws B H W C ph pw",
    "pcgmix_bnrp_bwd_f32": "y dz gamma beta mean invstd dx dgamma dbeta dzero ws B H W C ph pw",
    "pcgmix_bnrp_eval_fwd_f32": "y gamma beta running_mean running_var eps conv_bias skip z B H W C ph pw",
    "pcgmix_bnrp_eval_bwd_f32": "y dz gamma beta running_mean running_var eps conv_bias dx B H W C ph pw",
}
REQUIRED = {
    "pcgmix_bnrp_fwd_f32": "y gamma beta z mean invstd ws",
    "pcgmix_bnrp_bwd_f32": "y dz gamma beta mean invstd dx dgamma dbeta ws",
    "pcgmix_bnrp_eval_fwd_f32": "y gamma beta running_mean running_var z",
    "pcgmix_bnrp_eval_bwd_f32": "y dz gamma beta running_mean running_var dx",
}
VECTOR = {  # read or written as float4 / float2
    "pcgmix_bnrp_fwd_f32": "y gamma beta skip z mean invstd ws",
    "pcgmix_bnrp_bwd_f32": "y dz gamma beta mean invstd dx ws",
    "pcgmix_bnrp_eval_fwd_f32": "y gamma beta running_mean running_var conv_bias skip z",
    "pcgmix_bnrp_eval_bwd_f32": "y dz gamma beta running_mean running_var conv_bias dx",
}


def invoke(lib, name, env, **over):
    vals = {**env, **over}
    args = []
    for k in SIG[name].split():
        v = vals[k]
        if k in ("momentum", "eps"):
            v = ctypes.c_float(v)
        elif isinstance(v, torch.Tensor):
            v = v.data_ptr()
        args.append(v)
    return getattr(lib, name)(*args, vals["stream"])


def _guards(shape):
    """Guard lengths behind (y-shaped, z-shaped) buffers: what bnrp_ref.slack asks for where that is at
    most 2^20 floats, 64 otherwise."""
    g = R.geometry(*shape)
    big, small = R.slack(*shape), g.stride * shape[1]
    return (max(GUARD, big) if big <= MAX_SLACK else GUARD), (max(GUARD, small) if small <= MAX_SLACK else GUARD)


class Run:
    """The inputs of one case on the device (each with zeros behind it) and the sentinel-filled, guarded
    outputs of the call in preparation.  ``take`` checks ownership and hands the owned parts back."""

    def __init__(self, c, device):
        self.c, self.device, self.lib = c, device, _lib.load()
        B, C, H, W, ph, pw = c.shape[:6]
        self.gy, self.gz = _guards(c.shape)
        self.n_y, self.n_z = B * H * W * C, B * (H // ph) * (W // pw) * C
        self.ws_floats = int(self.lib.pcgmix_bnrp_workspace_floats(B, H, W, C))
        self.env = dict(B=B, C=C, H=H, W=W, ph=ph, pw=pw, eps=float(c.eps), momentum=float(getattr(c, "momentum", 0.0)),
                        stream=ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        for k in ("y", "dz", "skip", "gamma", "beta", "mean_shift", "conv_bias"):
            if getattr(c, k, None) is not None:
                self.env[k] = self.inp(getattr(c, k), self.gy if k == "y" else self.gz if k in ("dz", "skip") else GUARD)
        self.pending = {}

    def inp(self, a, guard=GUARD):
        flat = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1))
        assert np.array_equal(flat.numpy().astype(np.float64), np.asarray(a, np.float64).reshape(-1), equal_nan=True)   # float32 data
        buf = torch.zeros(flat.numel() + guard, device=self.device)
        buf[:flat.numel()] = flat.to(self.device)
        return buf

    def out(self, key, n, guard=GUARD, how="all", fill=None, dtype=torch.float32):
        """how: 'all' every owned element must be written; 'pre' pre-filled (updated in place: only the
        guard is checked); 'ws' scratch (only the guard is checked); 'none' must stay untouched."""
        sent = SENT_INT if dtype == torch.int64 else SENT
        buf = torch.full((n + guard,), sent, dtype=dtype, device=self.device)
        if fill is not None:
            buf[:n] = torch.as_tensor(np.asarray(fill), dtype=dtype).reshape(-1).to(self.device)
        self.env[key] = buf
        self.pending[key] = (buf, n, how)
        return buf

    def call(self, name, **over):
        _lib.check(invoke(self.lib, name, self.env, **over), name)

    def take(self, tag, P):
        torch.cuda.synchronize()
        got = {}
        for key, (buf, n, how) in self.pending.items():
            host = buf.cpu()
            sent = SENT_INT if host.dtype == torch.int64 else SENT
            own, guard = host[:n], host[n:]
            if not bool((guard == sent).all()):
                P.append(f"{tag}: {key}: {int((guard != sent).sum())} guard elements behind the buffer were written")
            if how == "all" and bool((own == sent).any()):
                P.append(f"{tag}: {key}: {int((own == sent).sum())} of {n} owned elements were not written")
            if how == "none" and not bool((own == sent).all()):
                P.append(f"{tag}: {key} was written")
            got[key] = own.numpy()
        self.pending = {}
        return got

    # ---- the four calls into fresh guarded outputs; drop: optional pointers passed NULL
    def train_fwd(self, tag, P, drop=()):
        c, C = self.c, self.c.shape[1]
        over = {k: None for k in drop}
        self.out("z", self.n_z, self.gz)
        self.out("mean", C)
        self.out("invstd", C)
        self.out("ws", self.ws_floats, WS_GUARD, "ws")
        for k in ("running_mean", "running_var"):
            if k in drop:
                self.env[k] = None
            else:
                self.out(k, C, how="pre", fill=getattr(c, k))
        if "batches_tracked" in drop:
            self.env["batches_tracked"] = None
        else:
            self.out("batches_tracked", 1, 8, "pre", fill=[c.batches_tracked], dtype=torch.int64)
        self.call("pcgmix_bnrp_fwd_f32", **over)
        return self.take(tag, P)

    def train_bwd(self, tag, P, mean, invstd, drop=()):
        C = self.c.shape[1]
        self.out("dx", self.n_y, self.gy)
        for k in ("dgamma", "dbeta", "dzero"):
            if k in drop:
                self.env[k] = None
            else:
                self.out(k, C)
        self.out("ws", self.ws_floats, WS_GUARD, "ws")
        self.call("pcgmix_bnrp_bwd_f32", mean=self.inp(mean), invstd=self.inp(invstd))
        got = self.take(tag, P)
        got["coef"] = got["ws"][R.BN_MAX_BLOCKS * 2 * C:]
        return got

    def eval_stats(self):
        c = self.c
        self.env["running_mean"], self.env["running_var"] = self.inp(c.running_mean), self.inp(c.running_var)

    def eval_fwd(self, tag, P, drop=()):
        self.eval_stats()
        self.out("z", self.n_z, self.gz)
        self.call("pcgmix_bnrp_eval_fwd_f32", **{k: None for k in drop})
        return self.take(tag, P)

    def eval_bwd(self, tag, P, drop=()):
        self.eval_stats()
        self.out("dx", self.n_y, self.gy)
        self.call("pcgmix_bnrp_eval_bwd_f32", **{k: None for k in drop})
        return self.take(tag, P)


# ---- comparisons -----------------------------------------------------------------------------------
def _same(name, got, want, P):
    """Bit equality of float32 output and float64 reference (which must be a float32 value)."""
    got, want = np.asarray(got).reshape(-1).astype(np.float64), np.asarray(want, np.float64).reshape(-1)
    if got.shape != want.shape:
        P.append(f"{name}: {got.size} elements, want {want.size}")
    elif not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        P.append(f"{name}: {bad.size} of {want.size} differ, first at {i} (got {got[i]!r}, want {want[i]!r}), "
                 f"last at {int(bad[-1])}")


def _plus_zero(name, got, where, P):
    """+0.0 by bit pattern at ``where``."""
    bits = np.asarray(got).reshape(-1).view(np.int32)[np.asarray(where).reshape(-1)]
    if bits.any():
        P.append(f"{name}: {int((bits != 0).sum())} of {bits.size} zeros are not +0.0")


def _near(name, got, want, rtol, atol, P):
    got, want = np.asarray(got).reshape(-1).astype(np.float64), np.asarray(want, np.float64).reshape(-1)
    over = np.abs(got - want) - (atol + rtol * np.abs(want))
    print(f"{name}: max |diff| {float(np.abs(got - want).max()):.3g}, worst margin to the bound {float(over.max()):.3g}")
    if not (over <= 0).all():                          # NaN fails
        P.append(f"{name}: {int((~(over <= 0)).sum())} of {want.size} outside rtol {rtol}, atol {atol}; "
                 f"max |diff| {float(np.abs(got - want).max()):.3g}")


def _near_grad(name, got, want, P):
    """EVERY element within 1e-4 max|ref| + 1e-6."""
    _near(name, got, want, 0.0, 1e-4 * float(np.abs(want).max()) + 1e-6, P)


def _small(shape):
    return shape[0] * shape[1] * shape[2] * shape[3] <= R.BIG


# ---- eval mode, exact ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.BNRP_EDGE, ids=R.EDGE_IDS)
def test_eval_integer_exact(shape, device):
    """eval_int_case: z and dx bit for bit against float64 with and without skip and conv_bias (planted
    ties: whole windows equal, the maximum last, nothing positive, a pre-activation exactly 0); every dx
    off the arg-max is +0.0 by bit pattern in channels of either sign of gamma."""
    c = R.eval_int_case(*shape)
    ph, pw = shape[4:6]
    r = Run(c, device)
    P = []
    args = (c.gamma, c.beta, c.running_mean, c.running_var, c.eps)
    for tag, drop, bias in (("all", (), c.conv_bias), ("conv_bias NULL", ("conv_bias",), None)):
        scale, shift = R.eval_affine(*args, bias)
        z, arg, best = R.pool_fwd(c.y, scale, shift, ph, pw, c.skip)
        got = r.eval_fwd(f"eval fwd, {tag}", P, drop)
        _same(f"eval fwd, {tag}: z", got["z"], z, P)
        got = r.eval_fwd(f"eval fwd, {tag}, skip NULL", P, drop + ("skip",))
        _same(f"eval fwd, {tag}, skip NULL: z", got["z"], best, P)
        dy, hit = R.pool_bwd(c.dz, arg, best, c.y.shape, ph, pw)
        got = r.eval_bwd(f"eval bwd, {tag}", P, drop)
        _same(f"eval bwd, {tag}: dx", got["dx"], np.where(hit, scale * dy, 0.0), P)
        _plus_zero(f"eval bwd, {tag}: dx", got["dx"], ~hit, P)
    assert not P, "\n".join(P)


# ---- training mode, exact --------------------------------------------------------------------------
_FWD_KEYS = ("z", "mean", "invstd", "running_mean", "running_var", "batches_tracked")
_BWD_KEYS = ("dx", "dgamma", "dbeta", "dzero", "coef")


def _check_train_fwd(tag, got, f, drop, same, P):
    same(f"{tag}: z", got["z"], f.best if "skip" in drop else f.z, P)
    if "running_mean" not in drop:
        want = f.running_mean_unshifted if "mean_shift" in drop else f.running_mean
        (same if same is _same else _near_stat)(f"{tag}: running_mean", got["running_mean"], want, P)
    if "batches_tracked" not in drop and int(got["batches_tracked"][0]) != f.batches_tracked:
        P.append(f"{tag}: batches_tracked {int(got['batches_tracked'][0])}, want {f.batches_tracked}")


def _near_stat(name, got, want, P):
    _near(name, got, want, 1e-5, 1e-6, P)


def _near_fwd(name, got, want, P):
    _near(name, got, want, 1e-4, 2e-5, P)


_FWD_DROPS = [(), ("skip",), ("running_mean",), ("running_var",), ("mean_shift",), ("batches_tracked",),
              ("running_mean", "running_var", "mean_shift", "batches_tracked", "skip")]


@pytest.mark.parametrize("shape", R.BNRP_EDGE, ids=R.EDGE_IDS)
def test_train_integer_exact(shape, device):
    """train_int_case: mean, invstd, the running statistics (mean_shift in the running mean only, the
    unbiased variance, the counter + 1), z, dbeta, dgamma, dzero (+0), coef bit for bit; dx bit for bit
    where n is a power of two and within 2^-21 |scale| (|dy| + |c1| + |xhat c2|) per element elsewhere;
    every optional pointer NULL in turn leaves everything else as it was; a second run gives the same
    bits.  Ties are everywhere (y takes two values per channel)."""
    c = R.train_int_case(*shape)
    B, C, H, W, ph, pw = shape[:6]
    r = Run(c, device)
    P = []
    assert r.ws_floats == R.BN_MAX_BLOCKS * 2 * C + 2 * C
    f = R.train_fwd(c.y, c.gamma, c.beta, c.running_mean, c.running_var, c.momentum, c.eps, c.mean_shift,
                    c.batches_tracked, c.skip, ph, pw)
    first = None
    for drop in _FWD_DROPS + [()]:
        tag = "fwd, " + (", ".join(drop) + " NULL" if drop else "all")
        got = r.train_fwd(tag, P, drop)
        _check_train_fwd(tag, got, f, drop, _same, P)
        _same(f"{tag}: mean", got["mean"], f.mean, P)
        _same(f"{tag}: invstd", got["invstd"], f.invstd, P)
        if "running_var" not in drop:
            _same(f"{tag}: running_var", got["running_var"], f.running_var.astype(np.float32), P)
        if first is None:
            first = got
        elif not drop:
            for k in _FWD_KEYS:
                _same(f"fwd, second run: {k}", got[k], first[k].astype(np.float64), P)
    b = R.train_bwd(c.y, c.dz, c.gamma, c.beta, f.mean, f.invstd, ph, pw)
    first = None
    for drop in ((), ("dzero",), ()):
        tag = "bwd, " + (", ".join(drop) + " NULL" if drop else "all")
        got = r.train_bwd(tag, P, f.mean, f.invstd, drop)
        for k in ("dgamma", "dbeta", "coef"):
            _same(f"{tag}: {k}", got[k], getattr(b, k), P)
        if "dzero" not in drop:
            _same(f"{tag}: dzero", got["dzero"], b.dzero, P)
            _plus_zero(f"{tag}: dzero", got["dzero"], np.ones(C, bool), P)
        if c.pow2:
            _same(f"{tag}: dx", got["dx"], b.dx, P)
        else:
            err = np.abs(got["dx"].astype(np.float64) - b.dx.reshape(-1))
            over = err - 2.0 ** -21 * b.dx_terms.reshape(-1)
            print(f"{tag}: dx: max |diff| {float(err.max()):.3g}, worst margin to the bound {float(over.max()):.3g}")
            if not (over <= 0).all():
                P.append(f"{tag}: dx: {int((~(over <= 0)).sum())} of {err.size} outside 2^-21 |scale| (|dy| + |c1| + |xhat c2|), "
                         f"first at {int(np.flatnonzero(~(over <= 0))[0])}")
        if first is None:
            first = got
        elif not drop:
            for k in _BWD_KEYS:
                _same(f"bwd, second run: {k}", got[k], first[k].astype(np.float64), P)
    assert not P, "\n".join(P)


# ---- Gaussian data without near-ties ---------------------------------------------------------------
@pytest.mark.parametrize("shape", R.BNRP_EDGE, ids=R.EDGE_IDS)
def test_margin_data_every_element(shape, device):
    """margin_case, training and eval: every element of z, the statistics, dx, dgamma and dbeta inside the
    limits of tests/test_bnrp_gpu.py — no share of the elements is left out — with the optional pointers
    NULL in turn, a second training run bit-equal, and eval dx +0.0 by bit pattern off the arg-max.
    Without conv_bias the eval decisions move, so that variant is a second generated case; on the two
    capped entries (above bnrp_ref.BIG, 8.4 M floats each) it is left to test_eval_integer_exact, which
    runs it there on exact data."""
    B, C, H, W, ph, pw = shape[:6]
    P = []
    c = R.margin_case(*shape, mode="train")
    r = Run(c, device)
    f = R.train_fwd(c.y, c.gamma, c.beta, c.running_mean, c.running_var, c.momentum, c.eps, c.mean_shift,
                    c.batches_tracked, c.skip, ph, pw)
    for drop in _FWD_DROPS:
        tag = "fwd, " + (", ".join(drop) + " NULL" if drop else "all")
        got = r.train_fwd(tag, P, drop)
        _check_train_fwd(tag, got, f, drop, _near_fwd, P)
        _near_stat(f"{tag}: mean", got["mean"], f.mean, P)
        _near_stat(f"{tag}: invstd", got["invstd"], f.invstd, P)
        if "running_var" not in drop:
            _near_stat(f"{tag}: running_var", got["running_var"], f.running_var, P)
        if not drop:
            mean, invstd, first = got["mean"], got["invstd"], got
    again = r.train_fwd("fwd, second run", P)
    for k in _FWD_KEYS:
        _same(f"fwd, second run: {k}", again[k], first[k].astype(np.float64), P)
    b = R.train_bwd(c.y, c.dz, c.gamma, c.beta, mean, invstd, ph, pw)     # from the statistics the forward left
    for drop in ((), ("dzero",)):
        tag = "bwd, " + (", ".join(drop) + " NULL" if drop else "all")
        got = r.train_bwd(tag, P, mean, invstd, drop)
        for k in ("dx", "dgamma", "dbeta"):
            _near_grad(f"{tag}: {k}", got[k], getattr(b, k), P)
        if not drop:
            _plus_zero(f"{tag}: dzero", got["dzero"], np.ones(C, bool), P)
            first = got
    again = r.train_bwd("bwd, second run", P, mean, invstd)
    for k in _BWD_KEYS:
        _same(f"bwd, second run: {k}", again[k], first[k].astype(np.float64), P)
    c = R.margin_case(*shape, mode="eval")
    r = Run(c, device)
    args = (c.gamma, c.beta, c.running_mean, c.running_var, c.eps)
    variants = [("all", (), c.conv_bias)] + ([("conv_bias NULL", ("conv_bias",), None)] if _small(shape) else [])
    for tag, drop, bias in variants:
        if drop:                                       # without the bias the decisions move: a case of its own
            c2 = R.margin_case(*shape, mode="eval", bias=False)
            r2 = Run(c2, device)
        else:
            c2, r2 = c, r
        scale, shift = R.eval_affine(*args, bias)
        z, arg, best = R.pool_fwd(c2.y, scale, shift, ph, pw, c2.skip)
        _near_fwd(f"eval fwd, {tag}: z", r2.eval_fwd(f"eval fwd, {tag}", P, drop)["z"], z, P)
        _near_fwd(f"eval fwd, {tag}, skip NULL: z", r2.eval_fwd(f"eval fwd, {tag}, skip NULL", P, drop + ("skip",))["z"], best, P)
        dy, hit = R.pool_bwd(c2.dz, arg, best, c2.y.shape, ph, pw)
        got = r2.eval_bwd(f"eval bwd, {tag}", P, drop)
        _near_grad(f"eval bwd, {tag}: dx", got["dx"], np.where(hit, scale * dy, 0.0), P)
        _plus_zero(f"eval bwd, {tag}: dx", got["dx"], ~hit, P)
    assert not P, "\n".join(P)


# ---- refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 4])
def test_refusals_leave_outputs_untouched(C, device):
    """hipErrorInvalidValue and not one sentinel touched for: C in {0, 1, 3, 6, 1028} (and
    pcgmix_bnrp_supported says 0 for exactly those), ph > H, pw > W, a zero or negative dimension, every
    required pointer NULL in turn, and every pointer the kernels access as float4 (C = 4) or float2
    (C = 2) moved by one float.  The unchanged arguments are then accepted."""
    shape = (2, C, 2, 6, 2, 2)
    c = R.train_int_case(*shape)
    c.conv_bias = c.mean_shift
    r = Run(c, device)
    lib = r.lib
    n = r.n_y + 64
    outs = ("z", "mean", "invstd", "dx", "dgamma", "dbeta", "dzero")
    bufs = {k: torch.full((n,), SENT, device=device) for k in outs}
    bufs["ws"] = torch.full((r.ws_floats + 64,), SENT, device=device)
    bufs["batches_tracked"] = torch.full((4,), SENT_INT, dtype=torch.int64, device=device)
    rm, rv = r.inp(c.running_mean), r.inp(c.running_var)
    env = {**r.env, **bufs, "running_mean": rm, "running_var": rv}
    rm0, rv0 = rm.clone(), rv.clone()

    def refused(name, why, **over):
        assert invoke(lib, name, env, **over) == INVALID, (name, why)

    for bad in (0, 1, 3, 6, 1028, -4):
        assert lib.pcgmix_bnrp_supported(bad) == 0, bad
    for ok in (2, 4, 8, 12, 516, 1020, 1024):
        assert lib.pcgmix_bnrp_supported(ok) == 1, ok
    for name in SIG:
        for bad in (0, 1, 3, 6, 1028):
            refused(name, f"C = {bad}", C=bad)
        refused(name, "ph > H", ph=3)
        refused(name, "pw > W", pw=7)
        for dim in ("B", "H", "W", "ph", "pw"):
            refused(name, f"{dim} = 0", **{dim: 0})
            refused(name, f"{dim} = -1", **{dim: -1})
        for arg in REQUIRED[name].split():
            refused(name, f"{arg} NULL", **{arg: None})
        for arg in VECTOR[name].split():
            refused(name, f"{arg} off by one float", **{arg: env[arg][1:]})       # never accessed: the call is refused
    assert lib.pcgmix_bnrp_workspace_floats(0, 2, 6, C) == 0 and lib.pcgmix_bnrp_workspace_floats(2, 2, 6, 0) == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == (SENT_INT if k == "batches_tracked" else SENT)).all()), k
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    # the same arguments, unchanged, are accepted
    bufs["batches_tracked"][0] = c.batches_tracked
    assert invoke(lib, "pcgmix_bnrp_fwd_f32", env) == 0
    torch.cuda.synchronize()
    f = R.train_fwd(c.y, c.gamma, c.beta, c.running_mean, c.running_var, c.momentum, c.eps, c.mean_shift,
                    c.batches_tracked, c.skip, 2, 2)
    assert np.array_equal(bufs["z"][:r.n_z].cpu().numpy().astype(np.float64), f.z.reshape(-1))
    assert int(bufs["batches_tracked"][0]) == c.batches_tracked + 1


# ---- the autograd Functions ----------------------------------------------------------------------------
def _cl(a, device):
    """(B, H, W, C) array -> (B, C, H, W) channels_last float32 tensor."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device).permute(0, 3, 1, 2)


def _flat(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().reshape(-1).cpu().numpy()


@pytest.mark.parametrize("shape", [t for t in R.BNRP_EDGE if t[6] in ("ragged-2x2", "generic-3x2", "Q24-nblk17")],
                         ids=lambda t: t[6])
def test_functions_give_the_bits_of_the_raw_calls(shape, device):
    B, C, H, W, ph, pw = shape[:6]
    P = []
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(device)   # noqa: E731
    c = R.margin_case(*shape, mode="train")
    r = Run(c, device)
    raw = r.train_fwd("fwd", P)
    raw.update(r.train_bwd("bwd", P, raw["mean"], raw["invstd"]))
    y, skip = _cl(c.y, device).requires_grad_(True), _cl(c.skip, device).requires_grad_(True)
    assert y.is_contiguous(memory_format=torch.channels_last) and models.BNReLUPoolFunction.supported(y)
    g, b, bias = t(c.gamma).requires_grad_(True), t(c.beta).requires_grad_(True), t(c.mean_shift).requires_grad_(True)
    rm, rv, bt = t(c.running_mean), t(c.running_var), torch.tensor(c.batches_tracked, device=device)
    z = models.BNReLUPoolFunction.apply(y, g, b, rm, rv, c.momentum, c.eps, ph, pw, skip, bias, bt)
    z.backward(_cl(c.dz, device))
    for name, got in (("z", _flat(z)), ("dx", _flat(y.grad)), ("dgamma", g.grad.cpu().numpy()), ("dbeta", b.grad.cpu().numpy()),
                      ("dzero", bias.grad.cpu().numpy()), ("running_mean", rm.cpu().numpy()), ("running_var", rv.cpu().numpy())):
        _same(f"BNReLUPoolFunction: {name}", got, raw[name].astype(np.float64), P)
    _same("BNReLUPoolFunction: d skip", _flat(skip.grad), c.dz, P)
    assert int(bt) == c.batches_tracked + 1
    c = R.margin_case(*shape, mode="eval")
    r = Run(c, device)
    raw = r.eval_fwd("eval fwd", P)
    raw.update(r.eval_bwd("eval bwd", P))
    y, skip = _cl(c.y, device).requires_grad_(True), _cl(c.skip, device).requires_grad_(True)
    z = models.BNReLUPoolEvalFunction.apply(y, t(c.gamma), t(c.beta), t(c.running_mean), t(c.running_var), c.eps, ph, pw,
                                            skip, t(c.conv_bias))
    z.backward(_cl(c.dz, device))
    _same("BNReLUPoolEvalFunction: z", _flat(z), raw["z"].astype(np.float64), P)
    _same("BNReLUPoolEvalFunction: dx", _flat(y.grad), raw["dx"].astype(np.float64), P)
    _same("BNReLUPoolEvalFunction: d skip", _flat(skip.grad), c.dz, P)
    assert not P, "\n".join(P)


# ---- non-finite activations -------------------------------------------------------------------------------
@pytest.mark.parametrize("pw", [2, 4], ids=["fixed-1x2", "generic-1x4"])
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_activation_reaches_z(value, mode, pw, device):
    """One NaN or +inf in y, in one channel: wherever torch's float32 composition (batch_norm -> relu ->
    max_pool2d) gives NaN in z the kernels do (a ReLU written as a > 0 ? a : 0 would give 0, and a
    diverged run would go on training on zeros); in training mode the channel's mean, invstd and running
    statistics are non-finite where torch's are; every other channel keeps its bits.  Forward only: the
    backward of a non-finite y is outside the contract."""
    shape = (2, 8, 1, 24, 1, pw)
    B, C, H, W, ph, _ = shape
    ch = 5
    c = R.margin_case(*shape, mode=mode)
    c.gamma[ch] = abs(c.gamma[ch])                     # +inf stays +inf in front of the ReLU
    P = []
    clean = Run(c, device)
    fwd = (lambda r, tag: r.train_fwd(tag, P, ("mean_shift",))) if mode == "train" else (lambda r, tag: r.eval_fwd(tag, P, ("conv_bias",)))
    base = fwd(clean, "clean")
    c.y = c.y.copy()
    c.y[1, 0, 7, ch] = value
    got = fwd(Run(c, device), "planted")
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(device)   # noqa: E731
    y = _cl(c.y, device)
    rm, rv = t(c.running_mean), t(c.running_var)
    want = F.max_pool2d(F.relu(F.batch_norm(y, rm, rv, t(c.gamma), t(c.beta), mode == "train", c.momentum, c.eps)), (ph, pw))
    want = _flat(want + _cl(c.skip, device)).reshape(-1, C)
    z = got["z"].reshape(-1, C)
    assert not np.isfinite(want[:, ch]).all() and np.isfinite(np.delete(want, ch, 1)).all()
    assert np.isnan(want[:, ch]).any() or (mode == "eval" and value == float("inf"))
    miss = np.isnan(want) & ~np.isnan(z)
    if miss.any():
        P.append(f"z is not NaN at {int(miss.sum())} of the {int(np.isnan(want).sum())} positions where torch's is "
                 f"(values there: {np.unique(z[miss])[:4]})")
    if not np.array_equal(z[np.isinf(want)], want[np.isinf(want)]):
        P.append("z is not torch's infinity where torch's is infinite")
    others = np.arange(C) != ch
    keys = ("z", "mean", "invstd", "running_mean", "running_var") if mode == "train" else ("z",)
    if mode == "eval":                                 # the NaN stays in its window: the rest of the channel keeps its bits
        fin = np.isfinite(want[:, ch])
        _same("z of the planted channel outside the planted window", z[fin, ch], base["z"].reshape(-1, C)[fin, ch].astype(np.float64), P)
    for k in keys:
        _same(f"{k} of the other channels", got[k].reshape(-1, C)[:, others], base[k].reshape(-1, C)[:, others].astype(np.float64), P)
    if mode == "train":
        var, mean = torch.var_mean(y, (0, 2, 3), unbiased=False)
        torch_stats = dict(mean=mean, invstd=torch.rsqrt(var + c.eps), running_mean=rm, running_var=rv)
        assert not bool(torch.isfinite(torch_stats["invstd"][ch]))
        for k, v in torch_stats.items():
            print(f"{k}[{ch}]: {got[k][ch]!r}, torch {float(v[ch])!r}")
            if not bool(torch.isfinite(v[ch])) and np.isfinite(got[k][ch]):
                P.append(f"{k}[{ch}] is {got[k][ch]!r} where torch's is {float(v[ch])!r}")
    assert not P, "\n".join(P)


# ---- conditioning of the batch statistics ---------------------------------------------------------------------
@pytest.mark.parametrize("r", [10, 100])
def test_batch_statistics_far_from_zero(r, device):
    """y ~ N(r sigma, sigma): the forward tolerance (rtol 1e-4, atol 2e-5 against float64) holds for the
    kernels whenever it holds for torch's own float32 composition on the same device — torch's result is
    the yardstick.  Likewise mean and invstd against the statistics tolerance whenever torch.var_mean
    in float32 meets it.  (profiles/bnrp_conditioning.txt has the sweep, r = 1000 included.)"""
    c = R.conditioning_case(r)
    B, C, H, W, ph, pw = c.shape
    f = R.train_fwd(c.y, c.gamma, c.beta, None, None, c.momentum, c.eps, None, None, None, ph, pw)
    P = []
    got = Run(c, device).train_fwd("fwd", P, ("running_mean", "running_var", "mean_shift", "batches_tracked", "skip"))
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(device)   # noqa: E731
    ref = _flat(F.max_pool2d(F.relu(F.batch_norm(_cl(c.y, device), None, None, t(c.gamma), t(c.beta), True, 0.1, c.eps)), (ph, pw)))
    bound = 2e-5 + 1e-4 * np.abs(f.z.reshape(-1))
    err_torch = np.abs(ref.astype(np.float64) - f.z.reshape(-1))
    err = np.abs(got["z"].astype(np.float64) - f.z.reshape(-1))
    print(f"r = {r}: z max |diff| kernel {float(err.max()):.3g}, torch float32 {float(err_torch.max()):.3g}; "
          f"worst margin to the bound: kernel {float((err - bound).max()):.3g}, torch {float((err_torch - bound).max()):.3g}")
    if (err_torch <= bound).all():
        assert (err <= bound).all(), (float(err.max()), float((err - bound).max()))
    # mean and invstd: the statistics tolerance (rtol 1e-5, atol 1e-6) whenever torch.var_mean in float32 meets it
    var32, mean32 = torch.var_mean(_cl(c.y, device), (0, 2, 3), unbiased=False)
    for k, theirs in (("mean", mean32), ("invstd", torch.rsqrt(var32 + c.eps))):
        want = getattr(f, k)
        lim = 1e-6 + 1e-5 * np.abs(want)
        e_t, e_k = np.abs(theirs.double().cpu().numpy() - want), np.abs(got[k].astype(np.float64) - want)
        print(f"r = {r}: {k} max |diff| kernel {float(e_k.max()):.3g}, torch.var_mean {float(e_t.max()):.3g}")
        if (e_t <= lim).all():
            assert (e_k <= lim).all(), (k, float(e_k.max()))
    assert not P, "\n".join(P)
