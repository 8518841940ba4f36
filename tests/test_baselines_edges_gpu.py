"""The comparison-baseline kernels (csrc/pcgmix_baselines.hip) at their block edges, all seven entry points
through the C ABI with raw pointers, against the plain numpy restatements of tests/baselines_ref.py.

  * pcgmix_blend_rows_f32, pcgmix_scale_rows_f32, pcgmix_warp_rows_f32: BIT FOR BIT (NaN equal to NaN, the
    sign of every zero included) at every (3, C, T) of baselines_ref.STREAM_T, on Gaussian rows with +-0.0,
    float32 subnormals, +-the largest finite value, +inf and NaN planted at the rows' ends and at both sides
    of the block seams; lam in {0, 1, float32(0.2718)}, mix a permutation, the identity and all zeros,
    n_knots in {2, 3, 6, 64}.  y is over-allocated and sentinel-filled: every owned element is written, no
    guard element is; x keeps its bits; a second call gives the same bits.  At T % 4 == 0 the call runs
    once on the tensors as allocated (float4 kernels) and once on views 4 bytes into larger buffers (the
    scalar kernels chosen by alignment alone): the same bits.
  * pcgmix_warp_rows_f32 is also held to oracle.pcgmix_oracle.magnitude_warp (scipy) under the project's
    bound for that pair: at most 1 ulp, fewer than 1e-3 of the elements differing.
  * pcgmix_zero_spans_f32, pcgmix_zero_rects_f32: in place on random bit patterns with guards on both sides;
    the WHOLE buffer equals the numpy reference by bit pattern, so nothing outside a span or rectangle is
    rewritten and no sample takes another's span.  Spans empty, whole, one element, sticking out below and
    above, starting a little above T, starting at and as long as 255, 256, 257; rectangles with clipped
    areas 0, 1, 1023, 1024, 1025, 2048, 2050 and F * W, max_area the exact maximum and F * W.
  * pcgmix_time_warp_f32: y BIT FOR BIT numpy's interp on the host twin's xp (hence the twin's y) at every
    (T, n_knots, sigma) of baselines_ref.tw_cases(), rows of both search paths in one launch; at T = 5121
    the workspace is exactly pcgmix_time_warp_workspace_bytes long with a guard behind it, its doubles are
    the twin's xp bit for bit and its ints, on rows whose xp decreases somewhere, numpy's search results;
    +-inf and NaN samples on rows with flat ends go through numpy's NaN retry.
  * refusals return hipErrorInvalidValue and write nothing; B == 0 and max_area == 0 return 0 and write
    nothing; the unchanged arguments are then accepted.
The only tolerances are the two the project already has: the 1 ulp / 1e-3 bound against the oracle and
check_warped against scipy.  Counts seen against them:
  CPU (tests/test_baselines_ref_cpu.py): warp_rows against the oracle 0 differing elements at every one of
  the 40 (T, n) combinations; time_warp_row against scipy_row at most 1 excused element per (T, n, sigma).
  MI355X (this file): pcgmix_warp_rows_f32 against the oracle 0 of 1 376 319 finite elements differing over
  the 80 (C, T, n) cases; pcgmix_time_warp_f32 against scipy_row 0 excused elements in 45 of the 48
  (T, n, sigma) cases and 1 in each of (5119, 2, 0.3), (5121, 2, 0.05), (5121, 6, 0.05) — the CPU counts,
  as the bit equality with the twin implies.
Only arguments include/pcgmix_hip.h documents or refuses are passed; the grid-size limits are not probed."""
import ctypes

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import baselines_ref as R
from test_baselines_cpu import check_warped, scipy_row, ulp_diff
from test_baselines_ref_cpu import oracle_warp

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -12345.5                      # no output holds it
GUARD = 64                           # floats behind (and, for a view, in front of) every output
SIG = {    # entry point -> its arguments in order (the stream follows)
    "pcgmix_blend_rows_f32": "x y mix lam B C T",
    "pcgmix_warp_rows_f32": "x y knots op n B C T",
    "pcgmix_scale_rows_f32": "x y s B C T",
    "pcgmix_zero_spans_f32": "x spans B C T",
    "pcgmix_time_warp_f32": "x y knots op n ws B C T",
    "pcgmix_zero_rects_f32": "x rect B C F W max_area",
}


def invoke(name, env, **over):
    vals = {**env, **over}
    args = []
    for k in SIG[name].split():
        v = vals[k]
        if k == "lam":
            v = ctypes.c_float(v)
        elif isinstance(v, torch.Tensor):
            v = v.data_ptr()
        args.append(v)
    return getattr(_lib.load(), name)(*args, vals["stream"])


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def to_dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class Inp:
    """A float32 input on the device, ``offset`` floats into a zero-filled buffer with GUARD floats behind."""

    def __init__(self, a, device, offset=0):
        self.host = np.ascontiguousarray(a, np.float32).reshape(-1)
        self.buf = torch.zeros(offset + self.host.size + GUARD, device=device)
        self.t = self.buf[offset:offset + self.host.size]
        self.t.copy_(torch.from_numpy(self.host))
        self.before = self.buf.cpu().numpy().view(np.int32).copy()
        assert self.t.data_ptr() % 16 == (4 * offset) % 16

    def unchanged(self, tag, P):
        if not np.array_equal(self.buf.cpu().numpy().view(np.int32), self.before):
            P.append(f"{tag}: the input was written")


class Out:
    """A sentinel-filled float32 output of n elements, ``offset`` floats into its buffer, GUARD behind."""

    def __init__(self, n, device, offset=0):
        self.n, self.offset = n, offset
        self.buf = torch.full((offset + n + GUARD,), SENT, device=device)
        self.t = self.buf[offset:offset + n]

    def take(self, tag, P, written=True):
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        own = host[self.offset:self.offset + self.n]
        guard = np.concatenate([host[:self.offset], host[self.offset + self.n:]])
        if (guard != SENT).any():
            P.append(f"{tag}: {int((guard != SENT).sum())} guard elements around the output were written")
        if written and (own == SENT).any():
            miss = np.flatnonzero(own == SENT)
            P.append(f"{tag}: {miss.size} of {self.n} owned elements were not written, first {int(miss[0])}, last {int(miss[-1])}")
        if not written and (own != SENT).any():
            P.append(f"{tag}: {int((own != SENT).sum())} elements were written")
        return own.copy()


def _same(tag, got, want, P):
    bad = R.same_bits(got, want)
    if bad.size:
        g, w = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
        i = int(bad[0])
        P.append(f"{tag}: {bad.size} of {w.size} differ by bit pattern, first at {i} (got {g[i]!r}, want {w[i]!r}), "
                 f"last at {int(bad[-1])}")


def _call(name, env, out, tag, P):
    err = invoke(name, env, y=out.t)
    assert err == 0, (name, tag, err)
    return out.take(tag, P)


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ---- the streaming kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.stream_shapes(), ids=_ids(R.stream_shapes()))
def test_blend_rows_exact(shape, device):
    B, C, T = shape
    x = R.samples(shape)
    xin = Inp(x, device)
    P = []
    env = dict(x=xin.t, B=B, C=C, T=T, stream=_stream(device))
    first = None
    for mname, mix in R.mixes(B):
        mix_dev = to_dev(mix, device)
        for lam in R.BLEND_LAM:
            tag = f"mix {mname}, lam {lam}"
            got = _call("pcgmix_blend_rows_f32", dict(env, mix=mix_dev, lam=lam), Out(B * C * T, device), tag, P)
            _same(tag, got, R.blend(x, mix, lam), P)
            if first is None:
                first = got
                again = _call("pcgmix_blend_rows_f32", dict(env, mix=mix_dev, lam=lam), Out(B * C * T, device), tag + ", second call", P)
                _same(tag + ", second call", again, first, P)
    xin.unchanged("blend", P)
    assert not P, "\n".join(P)


@pytest.mark.parametrize("shape", R.stream_shapes(), ids=_ids(R.stream_shapes()))
def test_scale_rows_exact(shape, device):
    B, C, T = shape
    x = R.samples(shape)
    s = R.scale_row(T)
    xin = Inp(x, device)
    P = []
    env = dict(x=xin.t, s=to_dev(s, device), B=B, C=C, T=T, stream=_stream(device))
    got = _call("pcgmix_scale_rows_f32", env, Out(B * C * T, device), "scale", P)
    want = R.scale(x, s)
    _same("scale", got, want, P)
    assert (want.view(np.int32) == np.int32(-2 ** 31)).any() or T < 8        # a -0.0 is among the results
    _same("scale, second call", _call("pcgmix_scale_rows_f32", env, Out(B * C * T, device), "scale, second call", P), got, P)
    xin.unchanged("scale", P)
    assert not P, "\n".join(P)


def _oracle_bound(tag, got, want, P):
    """At most 1 ulp, fewer than 1e-3 of the elements differing, on the finite elements of the oracle's
    result; the others (inf, NaN) must be the same.  Returns (differing, compared)."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    fin = np.isfinite(want)
    _same(tag + ": non-finite elements of the oracle", got[~fin], want[~fin], P)
    d = ulp_diff(got[fin], want[fin])
    n_diff = int((d > 0).sum())
    if d.size and not (d.max() <= 1 and (d > 0).mean() < 1e-3):
        P.append(f"{tag}: against the oracle {n_diff} of {d.size} differ, max {int(d.max())} ulp")
    return n_diff, int(d.size)


@pytest.mark.parametrize("shape", R.warp_shapes(), ids=_ids(R.warp_shapes()))
def test_warp_rows_exact(shape, device):
    """Against baselines_ref.warp_rows bit for bit, and against the oracle's magnitude_warp (which draws the
    knots) under at most 1 ulp with fewer than 1e-3 differing.
    Seen on an MI355X against the oracle: 0 elements differing in every case."""
    B, C, T, n = shape
    x = R.samples((B, C, T))
    want_oracle, knots = oracle_warp(x, n, 0.2, 7 * T + n + C)
    op = R.spline_op(T, n)
    xin = Inp(x, device)
    P = []
    env = dict(x=xin.t, knots=to_dev(knots, device), op=to_dev(op, device), n=n, B=B, C=C, T=T, stream=_stream(device))
    got = _call("pcgmix_warp_rows_f32", env, Out(B * C * T, device), "warp", P)
    _same("warp", got, R.warp_rows(x, knots, op), P)
    n_diff, n_cmp = _oracle_bound("warp", got, want_oracle, P)
    print(f"warp {shape}: against the oracle {n_diff} of {n_cmp} differ")
    _same("warp, second call", _call("pcgmix_warp_rows_f32", env, Out(B * C * T, device), "warp, second call", P), got, P)
    xin.unchanged("warp", P)
    assert not P, "\n".join(P)


@pytest.mark.parametrize("shape", R.integer_break_shapes(), ids=_ids(R.integer_break_shapes()))
def test_warp_rows_piece_search_on_integer_breaks(shape, device):
    """baselines_ref.zero_knots: samples ON a break whose knot is exactly 0.0 take the cubic that starts
    there (S = +0.0, y = +-0.0 by bit pattern), not the one that ends there (y around x * 1e-17)."""
    B, C, T, n = shape
    x = R.samples((B, C, T))
    knots = R.zero_knots(R.knots_for(B, n, C))
    op = R.spline_op(T, n)
    P = []
    env = dict(x=to_dev(x, device), knots=to_dev(knots, device), op=to_dev(op, device), n=n, B=B, C=C, T=T, stream=_stream(device))
    got = _call("pcgmix_warp_rows_f32", env, Out(B * C * T, device), "warp", P)
    _same("warp", got, R.warp_rows(x, knots, op), P)
    at = np.arange(1, n - 1) * ((T - 1) // (n - 1))
    on = got.reshape(B, C, T)[:, 0, at]
    assert not on[np.isfinite(x[:, 0, at])].any()
    assert not P, "\n".join(P)


@pytest.mark.parametrize("T", R.ALIGN_T)
@pytest.mark.parametrize("kernel", ["blend", "scale", "warp"])
def test_scalar_path_by_alignment_gives_the_same_bits(kernel, T, device):
    """C = 1, T % 4 == 0: the tensors as allocated (16-byte aligned: the float4 kernels) and x and y as views
    4 bytes into larger buffers (the scalar kernels), the float64 arrays 8-byte aligned either way."""
    B, C, n = R.B, 1, 6
    x = R.samples((B, C, T), "align")
    P = []
    env = dict(B=B, C=C, T=T, n=n, lam=R.BLEND_LAM[2], stream=_stream(device))
    if kernel == "blend":
        mix = R.mixes(B)[0][1]
        env["mix"], want, name = to_dev(mix, device), R.blend(x, mix, env["lam"]), "pcgmix_blend_rows_f32"
    elif kernel == "scale":
        s = R.scale_row(T)
        env["s"], want, name = to_dev(s, device), R.scale(x, s), "pcgmix_scale_rows_f32"
    else:
        knots, op = R.knots_for(B, n, C), R.spline_op(T, n)
        env["knots"], env["op"], want, name = to_dev(knots, device), to_dev(op, device), R.warp_rows(x, knots, op), "pcgmix_warp_rows_f32"
    for key in ("knots", "op", "s"):
        assert key not in env or env[key].data_ptr() % 8 == 0
    got = {}
    for offset in (0, 1):
        xin, out = Inp(x, device, offset), Out(B * C * T, device, offset)
        assert xin.t.data_ptr() % 16 == 4 * offset and out.t.data_ptr() % 16 == 4 * offset
        got[offset] = _call(name, dict(env, x=xin.t), out, f"{kernel}, offset {offset}", P)
        _same(f"{kernel}, offset {offset}", got[offset], want, P)
        xin.unchanged(f"{kernel}, offset {offset}", P)
    _same(f"{kernel}: aligned against offset", got[0], got[1], P)
    assert not P, "\n".join(P)


# ---- the in-place kernels ----------------------------------------------------------------------------------
class Bits:
    """Random bit patterns (every float32 class among them) of n elements with GUARD elements on both sides."""

    def __init__(self, n, device, seed):
        self.n = n
        rs = np.random.RandomState(seed)
        self.host = rs.randint(-2 ** 31, 2 ** 31, size=n + 2 * GUARD, dtype=np.int64).astype(np.int32)
        self.buf = torch.from_numpy(self.host.copy()).to(device)
        self.t = self.buf[GUARD:GUARD + n].view(torch.float32)

    def expect(self, tag, fn, P):
        """fn: the owned part as float32 -> its reference.  The whole buffer is compared by bit pattern."""
        torch.cuda.synchronize()
        want = self.host.copy()
        own = want[GUARD:GUARD + self.n].view(np.float32)
        want[GUARD:GUARD + self.n] = np.ascontiguousarray(fn(own), np.float32).reshape(-1).view(np.int32)
        got = self.buf.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want) - GUARD
            P.append(f"{tag}: {bad.size} elements differ by bit pattern, first at {int(bad[0])}, last at {int(bad[-1])} "
                     f"(owned: 0..{self.n - 1})")
        return int((want[GUARD:GUARD + self.n] != self.host[GUARD:GUARD + self.n]).sum())


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("T", R.SPAN_T)
def test_zero_spans_writes_only_its_spans(T, C, device):
    sp = R.span_list(T)
    B = len(sp)
    spans = np.array([(a, b) for a, b, _ in sp], np.int32)
    P = []
    x = Bits(B * C * T, device, T + C)
    env = dict(x=x.t, spans=to_dev(spans, device), B=B, C=C, T=T, stream=_stream(device))
    assert invoke("pcgmix_zero_spans_f32", env) == 0
    changed = x.expect("zero_spans", lambda own: R.zero_spans(own.reshape(B, C, T), spans), P)
    assert changed > 0
    assert invoke("pcgmix_zero_spans_f32", env) == 0                 # a second call changes nothing
    x.expect("zero_spans, second call", lambda own: R.zero_spans(own.reshape(B, C, T), spans), P)
    assert not P, "\n".join(P)


@pytest.mark.parametrize("T", R.SPAN_T)
def test_zero_spans_in_the_cutout_convention(T, device):
    """cutout(ch) passes one span per (sample, channel): the batch as (B * C, 1, T), spans (B * C, 2)."""
    sp = R.span_list(T)
    C = 3
    Bc = len(sp) // C
    spans = np.array([(a, b) for a, b, _ in sp[:Bc * C]], np.int32)
    P = []
    x = Bits(Bc * C * T, device, T)
    env = dict(x=x.t, spans=to_dev(spans, device), B=Bc * C, C=1, T=T, stream=_stream(device))
    assert invoke("pcgmix_zero_spans_f32", env) == 0
    assert x.expect("cutout", lambda own: R.zero_spans(own.reshape(Bc * C, 1, T), spans), P) > 0
    assert not P, "\n".join(P)


@pytest.mark.parametrize("plane", R.PLANES, ids=_ids(R.PLANES))
def test_zero_rects_writes_only_its_rectangles(plane, device):
    F, W = plane
    P = []
    for C in R.CHANNELS:
        for rect, why in R.rect_batches(F, W):
            exact = max(R.rect_area(r, F, W) for r in rect)
            for max_area in sorted({exact, F * W}):
                tag = f"C {C}, {why}, max_area {max_area}"
                x = Bits(R.B * C * F * W, device, F * W + C + max_area)
                env = dict(x=x.t, rect=to_dev(rect, device), B=R.B, C=C, F=F, W=W, max_area=max_area, stream=_stream(device))
                assert invoke("pcgmix_zero_rects_f32", env) == 0, tag
                x.expect(tag, lambda own: R.zero_rects(own.reshape(R.B, C, F, W), rect), P)
    assert not P, "\n".join(P)


# ---- the time warp ------------------------------------------------------------------------------------------
WS_GUARD = 4096                      # bytes behind the workspace


def _time_warp(x, kn, n, T, device, P, tag):
    """One launch on (TW_B, TW_C, T): (y, workspace bytes as uint8 or None)."""
    lib = _lib.load()
    Bn, C = x.shape[:2]
    need = int(lib.pcgmix_time_warp_workspace_bytes(Bn, C, T))
    assert need == (0 if T <= R.TW_LDS_MAX_T else Bn * C * T * 12)
    ws = torch.full((need + WS_GUARD,), 0xA5, dtype=torch.uint8, device=device) if need else None
    xin, out = Inp(x, device), Out(Bn * C * T, device)
    env = dict(x=xin.t, knots=to_dev(kn, device), op=to_dev(R.spline_op(T, n), device), n=n, ws=ws, B=Bn, C=C, T=T,
               stream=_stream(device))
    y = _call("pcgmix_time_warp_f32", env, out, tag, P)
    xin.unchanged(tag, P)
    again = _call("pcgmix_time_warp_f32", env, Out(Bn * C * T, device), tag + ", second call", P)
    _same(tag + ", second call", again, y, P)
    if ws is None:
        return y, None
    host = ws.cpu().numpy()
    if (host[need:] != 0xA5).any():
        P.append(f"{tag}: {int((host[need:] != 0xA5).sum())} guard bytes behind the workspace were written")
    return y, host[:need]


@pytest.mark.parametrize("T, n, sigma", R.tw_cases())
def test_time_warp_exact(T, n, sigma, device):
    """y bit for bit numpy's interp on the host twin's xp, and the twin's y; check_warped against scipy.
    Seen on an MI355X against scipy: at most 1 excused element per case (3 cases of 48 have one)."""
    x, kn = R.tw_case(T, n, sigma)
    P = []
    y, ws = _time_warp(x, kn, n, T, device, P, "time warp")
    y = y.reshape(R.TW_B * R.TW_C, T)
    op = R.spline_op(T, n)
    rows = R.tw_rows(T, n, sigma)
    want, xps, twin = zip(*(R.time_warp_row(op, k, xr) for _, _, xr, k in rows))
    _same("y against numpy's interp on the twin's xp", y, np.stack(want), P)
    _same("y against the host twin", y, np.stack(twin), P)
    excused = check_warped(y, np.stack([scipy_row(k, xr)[0] for _, _, xr, k in rows]), np.stack([xr for _, _, xr, _ in rows]))
    nonmono = [bool((np.diff(xp) < 0).any()) for xp in xps]
    print(f"time warp T = {T}, n = {n}, sigma = {sigma}: {excused} of {y.size} excused against scipy, "
          f"{sum(nonmono)} of {len(rows)} rows non-monotone")
    if ws is not None:
        nrow = len(rows)
        got_xp = ws[:nrow * T * 8].view(np.int64).reshape(nrow, T)
        got_j = ws[nrow * T * 8:].view(np.int32).reshape(nrow, T)
        if not np.array_equal(got_xp, np.stack(xps).view(np.int64)):
            P.append(f"workspace: xp differs from the twin's at {int((got_xp != np.stack(xps).view(np.int64)).sum())} elements")
        for r, (xp, dec) in enumerate(zip(xps, nonmono)):
            if dec and not np.array_equal(got_j[r], R.search_walk(xp)):
                P.append(f"workspace: row {r}: {int((got_j[r] != R.search_walk(xp)).sum())} search results are not numpy's")
    assert not P, "\n".join(P)


def test_time_warp_non_finite_samples_on_flat_rows(device):
    """+-inf and NaN samples (finite knots) on rows whose xp has flat steps: numpy's "if we get nan in one
    direction, try the other" branch runs on the device.  Against np.interp with NaN equal to NaN."""
    T, n, sigma = 257, 6, 0.3
    x, kn = R.tw_case(T, n, sigma)
    x = x.copy()
    for i, v in ((0, np.inf), (5, np.inf), (6, -np.inf), (40, -np.inf), (100, np.nan), (T - 40, np.inf), (T - 3, np.inf),
                 (T - 2, np.inf), (T - 1, -np.inf)):
        x[:, :, i] = v
    op = R.spline_op(T, n)
    P = []
    y, _ = _time_warp(x, kn, n, T, device, P, "time warp, non-finite")
    y = y.reshape(-1, T)
    flat = retried = 0
    for r, (b, c) in enumerate((b, c) for b in range(R.TW_B) for c in range(R.TW_C)):
        want, xp, twin = R.time_warp_row(op, np.ascontiguousarray(kn[b, :, c]), x[b, c])
        flat += bool((np.diff(xp) == 0).any())
        j = np.clip(R.search_walk(xp).astype(np.int64), 0, T - 2)
        fp = x[b, c].astype(np.float64)
        with np.errstate(all="ignore"):
            one = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (np.arange(T) - xp[j]) + fp[j]
        retried += int((np.isnan(one) & ~np.isnan(want)).sum())      # the first direction gave NaN, numpy's result is none
        _same(f"row {r} against np.interp", y[r], want, P)
        _same(f"row {r} against the twin", y[r], twin, P)
    assert flat > 0 and retried > 0, (flat, retried)
    assert np.isnan(y).any() and np.isinf(y).any()
    assert not P, "\n".join(P)


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(device):
    """hipErrorInvalidValue and not one element written for: every required pointer NULL in turn, x == y,
    C = 0, T = 0 (T = 1 for the warps), n_knots 1 and 65, a NULL workspace at T = 5121, a negative B or
    max_area, a zero plane side.  B = 0 and max_area = 0 return 0 and write nothing.  Then the unchanged
    arguments are accepted."""
    lib = _lib.load()
    B, C, T, n = 2, 3, 8, 4
    Tw = R.TW_LDS_MAX_T + 1
    F, W = 4, 6
    st = _stream(device)
    x = R._rng("refuse", (B, C, T)).standard_normal((B, C, T)).astype(np.float32)
    xw = R._rng("refuse", (B, C, Tw)).standard_normal((B, C, Tw)).astype(np.float32)
    knots = R.knots_for(B, n, C)
    mix = np.array([1, 0], np.int32)
    spans = np.array([(1, 5), (0, 8)], np.int32)
    rect = np.array([(1, 3, 2, 5), (0, 4, 0, 6)], np.int32)
    xin, xwin = Inp(x, device), Inp(xw, device)
    out, outw = Out(B * C * T, device), Out(B * C * Tw, device)
    inplace = Out(B * C * max(T, F * W), device)                      # the in-place kernels' tensor: sentinels
    ws_bytes = int(lib.pcgmix_time_warp_workspace_bytes(B, C, Tw))
    ws = torch.full((ws_bytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=device)
    common = dict(B=B, C=C, T=T, n=n, stream=st, x=xin.t, y=out.t, knots=to_dev(knots, device),
                  op=to_dev(R.spline_op(T, n), device))
    envs = {
        "pcgmix_blend_rows_f32": dict(common, mix=to_dev(mix, device), lam=0.25),
        "pcgmix_warp_rows_f32": dict(common),
        "pcgmix_scale_rows_f32": dict(common, s=to_dev(R.scale_row(T), device)),
        "pcgmix_zero_spans_f32": dict(common, x=inplace.t, spans=to_dev(spans, device)),
        "pcgmix_time_warp_f32": dict(common, x=xwin.t, y=outw.t, T=Tw, op=to_dev(R.spline_op(Tw, n), device), ws=ws),
        "pcgmix_zero_rects_f32": dict(common, x=inplace.t, rect=to_dev(rect, device), F=F, W=W, max_area=F * W),
    }
    pointers = {
        "pcgmix_blend_rows_f32": "x y mix", "pcgmix_warp_rows_f32": "x y knots op", "pcgmix_scale_rows_f32": "x y s",
        "pcgmix_zero_spans_f32": "x spans", "pcgmix_time_warp_f32": "x y knots op ws", "pcgmix_zero_rects_f32": "x rect",
    }
    warps = ("pcgmix_warp_rows_f32", "pcgmix_time_warp_f32")

    def refused(name, why, **over):
        assert invoke(name, envs[name], **over) == INVALID, (name, why)

    for name, env in envs.items():
        for p in pointers[name].split():
            refused(name, f"{p} NULL", **{p: None})
        if "y" in SIG[name].split():
            refused(name, "x == y", y=env["x"])
        refused(name, "C = 0", C=0)
        refused(name, "C = -1", C=-1)
        refused(name, "B = -1", B=-1)
        if name == "pcgmix_zero_rects_f32":
            refused(name, "F = 0", F=0)
            refused(name, "W = 0", W=0)
            refused(name, "max_area = -1", max_area=-1)
        else:
            refused(name, "T = 0", T=0)
            refused(name, "T = -1", T=-1)
        if name in warps:
            refused(name, "T = 1", T=1)
            refused(name, "n_knots = 1", n=1)
            refused(name, "n_knots = 65", n=R.MAX_KNOTS + 1)
            refused(name, "n_knots = 0", n=0)
        assert invoke(name, env, B=0) == 0, name                    # nothing to do
    assert invoke("pcgmix_zero_rects_f32", envs["pcgmix_zero_rects_f32"], max_area=0) == 0
    assert lib.pcgmix_time_warp_workspace_bytes(B, C, R.TW_LDS_MAX_T) == 0
    assert lib.pcgmix_time_warp_workspace_bytes(B, C, Tw) == B * C * Tw * 12 == ws_bytes
    assert lib.pcgmix_time_warp_workspace_bytes(0, C, Tw) == 0
    P = []
    for tag, o in (("y", out), ("y of the time warp", outw), ("the in-place tensor", inplace)):
        o.take(tag, P, written=False)
    assert bool((ws == 0xA5).all()), "the workspace was written"
    xin.unchanged("x", P)
    xwin.unchanged("x of the time warp", P)
    assert not P, "\n".join(P)
    # the same arguments, unchanged, are accepted
    for name, env in envs.items():
        assert invoke(name, env) == 0, name
        torch.cuda.synchronize()
        if name == "pcgmix_blend_rows_f32":
            _same(name, out.take(name, P), R.blend(x, mix, 0.25), P)
        elif name == "pcgmix_warp_rows_f32":
            _same(name, out.take(name, P), R.warp_rows(x, knots), P)
        elif name == "pcgmix_scale_rows_f32":
            _same(name, out.take(name, P), R.scale(x, R.scale_row(T)), P)
        elif name == "pcgmix_time_warp_f32":
            opw = R.spline_op(Tw, n)
            want = np.stack([R.time_warp_row(opw, np.ascontiguousarray(knots[b, :, c]), xw[b, c])[0] for b in range(B) for c in range(C)])
            _same(name, outw.take(name, P), want, P)
        elif name == "pcgmix_zero_spans_f32":
            got = inplace.buf.cpu().numpy()[:B * C * T]
            want = R.zero_spans(np.full((B, C, T), SENT, np.float32), spans)
            _same(name, got, want, P)
            inplace.buf.fill_(SENT)
        else:
            got = inplace.buf.cpu().numpy()[:B * C * F * W]
            want = R.zero_rects(np.full((B, C, F, W), SENT, np.float32), rect)
            _same(name, got, want, P)
            inplace.buf.fill_(SENT)
    assert not P, "\n".join(P)
