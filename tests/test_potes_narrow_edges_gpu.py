"""The narrow ([1,1] and [2,1]) Potes conv stacks (csrc/pcgmix_potes_narrow.hip) at their tile edges,
through the C ABI (no autograd), against the float64 restatement of tests/potes_narrow_ref.py.

  * integer data (potes_narrow_ref.int_case): float32 in any order is exact, so h2, the routing bytes
    m2 / s1, the weight gradients (the reduced ones, and the per-block partials summed in float64)
    and the input gradient must equal float64 BIT FOR BIT, with exact ties (first maximum wins) and
    exact zeros (dead) in a few per cent of the pairs;
  * float outputs land in SENT-filled, over-allocated buffers; the routing bytes in buffers that hold
    the bitwise COMPLEMENT of the expected bytes (any byte value is a legal quadruple of codes, so
    only the complement proves that every owned byte was written) with a fixed pattern behind them;
  * the forward without s1, and without m2 and s1 (fewer tiles), is bit-identical to the one with;
  * lengths with T % 4 == 0 run again from pointers 4 bytes past a 16-byte boundary: the generic
    staging and the scalar stores see the same tile edges as the 16-byte paths;
  * the weight gradient's persistent loop takes second items, the reduction's stride loop second
    rows, and the row limit is reached and refused one above;
  * random data whose decisions float32 cannot flip: routing bytes exact, every h2 element within its
    own a-priori bound, gradients within the limits of tests/test_potes_widths_gpu.py per element.
The shape table is potes_narrow_ref.EDGE / LOOP / LIMIT
(tests/test_potes_narrow_ref_cpu.py::test_shapes_cover_tile_edges says what it covers)."""
import ctypes
import types

import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import potes_narrow_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -12345.5                      # no output can hold it: integer data give integers, h2 >= 0, and
#                                      the random gradients are orders of magnitude smaller
GUARD = 64
GUARD_BYTE = 0x5A
WIDTH_IDS = [f"{a}-{b}" for a, b in R.WIDTHS]
FLOATS = ("h2", "h2 (no s1)", "h2 (inference)", "partial", "grads", "gx")


def stream_of(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _floats(n, device, lead=0):
    """n owned floats behind ``lead`` floats, all SENT, GUARD more behind them."""
    return torch.full((lead + n + GUARD,), SENT, device=device)


def _complement(want, device):
    buf = torch.full((want.numel() + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device)
    buf[:want.numel()] = torch.bitwise_not(want.reshape(-1)).to(device)
    return buf


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


def _owned(buf, n, name, problems, lead=0):
    """The n owned floats of a SENT-filled buffer: all written, none of the floats around them."""
    own = buf[lead:lead + n]
    left = int((own == SENT).sum())
    if left:
        problems.append(f"{name}: {left} of {n} owned elements were not written")
    if not bool((buf[lead + n:] == SENT).all()):
        problems.append(f"{name}: guard elements behind the buffer were written")
    if lead and not bool((buf[:lead] == SENT).all()):
        problems.append(f"{name}: the element in front of the buffer was written")
    return own.cpu()


def _bytes(buf, want, name, problems):
    """A complement-filled byte buffer after a call that owns it: equal to ``want`` (so every byte
    was written), the pattern behind it intact."""
    n = want.numel()
    got = buf[:n].cpu()
    _same(name, got, want, problems)
    if not bool((buf[n:] == GUARD_BYTE).all()):
        problems.append(f"{name}: guard bytes behind the buffer were written")
    return got


def _untouched(buf, want, name, problems):
    """A complement-filled byte buffer after a call that was not given it."""
    n = want.numel()
    if not (torch.equal(buf[:n].cpu(), torch.bitwise_not(want.reshape(-1))) and bool((buf[n:] == GUARD_BYTE).all())):
        problems.append(f"{name}: written by a call that was not given it")


def _padding_is_zero(c, m2, s1, problems):
    """What byte equality with pack_m2 / pack_s1 implies, said directly on the kernel's bytes: code 0
    behind output P2 - 1, at q = -1 and behind position P1 - 1."""
    m2, s1 = m2.view(c.N * c.C2, -1).int(), s1.view(c.N * c.C1, -1).int()
    if c.P2 & 3 and bool((m2[:, -1] >> (2 * (c.P2 & 3))).any()):
        problems.append("m2: stale bits in the tail slots of the last byte")
    if bool((s1[:, 0] & 3).any()):
        problems.append("s1: slot q = -1 is not code 0")
    if (c.P1 + 1) & 3 and bool((s1[:, -1] >> (2 * ((c.P1 + 1) & 3))).any()):
        problems.append("s1: stale bits behind position P1 - 1")


def _upload(c, device, x_off):
    d = types.SimpleNamespace(**{k: getattr(c, k).to(device).contiguous()
                                 for k in ("w1", "b1", "w2", "b2", "r", "m2", "s1")})
    if x_off:
        hold = torch.zeros(c.N * c.T + 1, device=device)
        d.x = hold[1:]
        d.x.copy_(c.x.reshape(-1))
        assert d.x.data_ptr() % 16 == 4
    else:
        d.x = c.x.to(device).contiguous()
        assert d.x.data_ptr() % 16 == 0
    return d


def run_all(lib, c, device, problems, off=False, tag=""):
    """The three entry points on case c, the forward in its three forms, then everything a second
    time into the same buffers.  off: x (forward, weight gradient) and grad_x (input gradient) sit
    4 bytes past a 16-byte boundary.  Checks what holds for any data — every owned element written,
    guards intact, absent buffers untouched, the forms of the forward and the second run bit-identical
    — and returns name -> flat CPU tensor."""
    N, T, C1, C2, P2 = c.N, c.T, c.C1, c.C2, c.P2
    d = _upload(c, device, off)
    st = stream_of(device)
    w = (d.w1.data_ptr(), d.b1.data_ptr(), d.w2.data_ptr(), d.b2.data_ptr())
    size = (N, T, C1, C2)
    nh, ng = N * C2 * P2, R.grad_len(C1, C2)
    assert lib.pcgmix_potes_narrow_mask_bytes(*size, 2) == c.m2.numel()
    assert lib.pcgmix_potes_narrow_mask_bytes(*size, 1) == c.s1.numel()
    assert lib.pcgmix_potes_narrow_grad_len(C1, C2) == ng
    G = lib.pcgmix_potes_narrow_bwd_blocks(*size)
    assert G == R.bwd_blocks(N, T)
    lead = 1 if off else 0
    out = {}

    def forward(h, m2, s1, what):
        _lib.check(lib.pcgmix_potes_narrow_fwd_f32(
            d.x.data_ptr(), *w, h.data_ptr(), m2.data_ptr() if m2 is not None else None,
            s1.data_ptr() if s1 is not None else None, *size, None, 0, None, 0, st), tag + what)

    def weight_grad(partial, grads):
        _lib.check(lib.pcgmix_potes_narrow_bwd_mask_f32(
            d.x.data_ptr(), d.r.data_ptr(), d.m2.data_ptr(), *w, partial.data_ptr(), grads.data_ptr(),
            *size, st), tag + "bwd_mask")

    def input_grad(gx):
        gx_un = gx[lead:]
        assert gx_un.data_ptr() % 16 == (4 if off else 0)
        _lib.check(lib.pcgmix_potes_narrow_input_grad_mask_f32(
            d.r.data_ptr(), d.m2.data_ptr(), d.s1.data_ptr(), w[0], w[2], gx_un.data_ptr(), *size, st),
            tag + "input_grad_mask")

    # ---- forward with m2 and s1
    h, m2, s1 = _floats(nh, device), _complement(c.m2, device), _complement(c.s1, device)
    forward(h, m2, s1, "fwd")
    out["h2"] = _owned(h, nh, tag + "h2", problems)
    out["m2"] = _bytes(m2, c.m2, tag + "m2", problems)
    out["s1"] = _bytes(s1, c.s1, tag + "s1", problems)
    _padding_is_zero(c, out["m2"], out["s1"], problems)
    # ---- without s1 (fewer tiles), then without both; a complement-filled s1 / m2 stands by
    hb, m2b, s1b = _floats(nh, device), _complement(c.m2, device), _complement(c.s1, device)
    forward(hb, m2b, None, "fwd, s1 = NULL")
    out["h2 (no s1)"] = _owned(hb, nh, tag + "h2 (no s1)", problems)
    out["m2 (no s1)"] = _bytes(m2b, c.m2, tag + "m2 (no s1)", problems)
    _untouched(s1b, c.s1, tag + "s1 (fwd, s1 = NULL)", problems)
    hc, m2c = _floats(nh, device), _complement(c.m2, device)
    forward(hc, None, None, "fwd, m2 = s1 = NULL")
    out["h2 (inference)"] = _owned(hc, nh, tag + "h2 (inference)", problems)
    _untouched(s1b, c.s1, tag + "s1 (fwd, m2 = s1 = NULL)", problems)
    _untouched(m2c, c.m2, tag + "m2 (fwd, m2 = s1 = NULL)", problems)
    for name in ("h2 (no s1)", "h2 (inference)"):
        _same(f"{tag}{name} against h2", out[name], out["h2"], problems)
    _same(f"{tag}m2 (no s1) against m2", out["m2 (no s1)"], out["m2"], problems)
    # ---- weight gradient and input gradient, from the reference's routing bytes
    partial, grads = _floats(G * ng, device), _floats(ng, device)
    weight_grad(partial, grads)
    out["partial"] = _owned(partial, G * ng, tag + "partial", problems)
    out["grads"] = _owned(grads, ng, tag + "grads", problems)
    gx = _floats(N * T, device, lead)
    input_grad(gx)
    out["gx"] = _owned(gx, N * T, tag + "gx", problems, lead)
    if bool((torch.signbit(out["gx"]) & (out["gx"] == 0)).any()):
        problems.append(f"{tag}gx: a zero is -0.0")
    # ---- once more into the same buffers
    forward(h, m2, s1, "fwd, second run")
    weight_grad(partial, grads)
    input_grad(gx)
    again = {"h2": _owned(h, nh, tag + "h2, second run", problems),
             "m2": _bytes(m2, c.m2, tag + "m2, second run", problems),
             "s1": _bytes(s1, c.s1, tag + "s1, second run", problems),
             "partial": _owned(partial, G * ng, tag + "partial, second run", problems),
             "grads": _owned(grads, ng, tag + "grads, second run", problems),
             "gx": _owned(gx, N * T, tag + "gx, second run", problems, lead)}
    for name, got in again.items():
        _same(f"{tag}{name}, second run against the first", got, out[name], problems)
    return out


def check_exact(c, out, problems, tag=""):
    """Integer data: bit equality with float64, nothing excused."""
    ref, ng = c.ref, R.grad_len(c.C1, c.C2)
    for name in ("h2", "h2 (no s1)", "h2 (inference)"):
        _same(tag + name, out[name], ref.h2, problems)
    _same(tag + "grads", out["grads"], ref.grads, problems)
    _same(tag + "column sums of partial (float64)", out["partial"].double().view(-1, ng).sum(0), ref.grads, problems)
    _same(tag + "gx", out["gx"], ref.gx, problems)


def check_close(c, out, problems, tag=""):
    """Random data: every h2 element within its a-priori bound c.e2; every gradient element within
    the limits of tests/test_potes_widths_gpu.py, 1e-4 max|gx| and 2e-4 max|.| per parameter
    tensor, against float64.  Prints the observed maxima."""
    ref = c.ref
    for name in ("h2", "h2 (no s1)", "h2 (inference)"):
        ratio = (out[name].double().view_as(ref.h2) - ref.h2).abs() / c.e2
        print(f"{tag}{name}: max err / e2 {float(ratio.max()):.3g}")
        if not bool((ratio <= 1.0).all()):
            problems.append(f"{tag}{name}: {int((ratio > 1.0).sum())} elements beyond their bound, worst {float(ratio.max()):.3g} e2")
    err, scale = (out["gx"].double() - ref.gx.reshape(-1)).abs(), float(ref.gx.abs().max())
    print(f"{tag}gx: max |diff| {float(err.max()):.3g} of {scale:.3g} ({float(err.max()) / scale:.3g})")
    if not bool((err <= 1e-4 * scale).all()):
        problems.append(f"{tag}gx: {float(err.max()):.3g} > 1e-4 * {scale:.3g}")
    lo = 0
    for part, n in R.grad_parts(c.C1, c.C2):
        a, b = out["grads"][lo:lo + n].double(), ref.grads[lo:lo + n]
        lo += n
        err, scale = (a - b).abs(), float(b.abs().max())
        print(f"{tag}g{part}: max |diff| {float(err.max()):.3g} of {scale:.3g} ({float(err.max()) / scale:.3g})")
        if not bool((err <= 2e-4 * scale).all()):
            problems.append(f"{tag}g{part}: {float(err.max()):.3g} > 2e-4 * {scale:.3g}")


def _int_case(widths, N, T):
    c = R.int_case(widths, N, T)
    for t in (c.ref.h2, c.ref.gx, c.ref.grads):
        assert torch.equal(t, t.round()) and float(t.abs().max()) < -SENT
    return c


def _integer_exact(widths, N, T, device):
    lib = _lib.load()
    c = _int_case(widths, N, T)
    problems = []
    out = run_all(lib, c, device, problems)
    check_exact(c, out, problems)
    if T % 4 == 0:
        un = run_all(lib, c, device, problems, off=True, tag="4 bytes off: ")
        check_exact(c, un, problems, tag="4 bytes off: ")
        for name, got in un.items():
            _same(f"4 bytes off: {name} against the aligned run", got, out[name], problems)
    return lib, c, problems


@pytest.mark.parametrize("N,T", R.EDGE)
@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_integer_exact(widths, N, T, device):
    """Every tile edge of the table: bit equality with float64 on integer data, every owned element
    and byte written, every guard intact, the three forms of the forward and the second run
    identical; where T % 4 == 0 all of it again from pointers 4 bytes off."""
    _, _, problems = _integer_exact(widths, N, T, device)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("N,T", R.LOOP)
@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_persistent_loop_and_reduction_integer_exact(widths, N, T, device):
    """More partial rows than the reduce has threads (300), more items than blocks with one tile per
    row (1030) and with two (520 x 1028: the second item of a block is another tile of another row)."""
    lib = _lib.load()
    assert lib.pcgmix_potes_narrow_bwd_blocks(N, T, *widths) == {300: 300, 1030: 1024, 520: 1024}[N]
    assert N * R.bwd_tiles(T) == {300: 300, 1030: 1030, 520: 1040}[N]
    _, _, problems = _integer_exact(widths, N, T, device)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_row_limit(widths, device):
    """N = 65535 = kMaxN (grid.y) runs and is exact; N = 65536 is refused by all three entry points
    without a launch — so the buffers of 65535 rows serve — and nothing is written."""
    N, T = R.LIMIT
    assert N == R.MAX_N
    lib, c, problems = _integer_exact(widths, N, T, device)
    C1, C2 = widths
    d = _upload(c, device, False)
    st = stream_of(device)
    w = (d.w1.data_ptr(), d.b1.data_ptr(), d.w2.data_ptr(), d.b2.data_ptr())
    ng = R.grad_len(C1, C2)
    h, partial, grads, gx = (_floats(n, device) for n in (N * C2 * c.P2, R.BWD_CAP * ng, ng, N * T))
    m2, s1 = _complement(c.m2, device), _complement(c.s1, device)
    over = (N + 1, T, C1, C2)
    assert lib.pcgmix_potes_narrow_bwd_blocks(*over) == 0
    assert lib.pcgmix_potes_narrow_fwd_f32(d.x.data_ptr(), *w, h.data_ptr(), m2.data_ptr(), s1.data_ptr(), *over,
                                           None, 0, None, 0, st) == INVALID
    assert lib.pcgmix_potes_narrow_bwd_mask_f32(d.x.data_ptr(), d.r.data_ptr(), d.m2.data_ptr(), *w,
                                                partial.data_ptr(), grads.data_ptr(), *over, st) == INVALID
    assert lib.pcgmix_potes_narrow_input_grad_mask_f32(d.r.data_ptr(), d.m2.data_ptr(), d.s1.data_ptr(), w[0], w[2],
                                                       gx.data_ptr(), *over, st) == INVALID
    torch.cuda.synchronize()
    for name, b in (("h2", h), ("partial", partial), ("grads", grads), ("gx", gx)):
        if not bool((b == SENT).all()):
            problems.append(f"{name}: written by a refused call")
    _untouched(m2, c.m2, "m2 (refused call)", problems)
    _untouched(s1, c.s1, "s1 (refused call)", problems)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("N,T", R.EDGE + R.LOOP[1:])
@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_random_parity(widths, N, T, device):
    """randn data with no decision float32 could flip (asserted, seed named): routing bytes equal the
    float64 packing exactly (run_all compares them), h2 within its derived bound element by element,
    gradients within the project's limits element by element."""
    lib = _lib.load()
    c = R.rand_case(widths, N, T)
    assert c.undecidable == 0, f"rand_case({widths}, {N}, {T}, seed={c.seed}): {c.undecidable} undecidable decisions"
    assert max(float(c.ref.gx.abs().max()), float(c.ref.grads.abs().max())) < -SENT
    problems = []
    out = run_all(lib, c, device, problems)
    check_close(c, out, problems, tag=f"{widths} ({N},{T}) ")
    assert not problems, "\n".join(problems)


# ---- refusals ---------------------------------------------------------------------------------
def _fwd(lib, p, size, st):
    return lib.pcgmix_potes_narrow_fwd_f32(p["x"], p["w1"], p["b1"], p["w2"], p["b2"], p["h2"], p["m2"], p["s1"],
                                           *size, None, 0, None, 0, st)


def _bwd(lib, p, size, st):
    return lib.pcgmix_potes_narrow_bwd_mask_f32(p["x"], p["g"], p["m2in"], p["w1"], p["b1"], p["w2"], p["b2"],
                                                p["partial"], p["grads"], *size, st)


def _ingrad(lib, p, size, st):
    return lib.pcgmix_potes_narrow_input_grad_mask_f32(p["g"], p["m2in"], p["s1in"], p["w1"], p["w2"], p["gx"],
                                                       *size, st)


# the NULL pointers tests/test_potes_widths_gpu.py::test_refusals_leave_outputs_untouched leaves out
_REFUSED = ((_fwd, ("b1", "b2")), (_bwd, ("b1", "b2", "partial", "x", "g")), (_ingrad, ("g", "w1", "w2")))


@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_null_pointers_are_refused(widths, device):
    """b1 / b2 (forward, weight gradient), partial, x and grad_h2 (weight gradient), grad_h2, w1 and
    w2 (input gradient) NULL in turn: hipErrorInvalidValue, nothing written; with every pointer given
    the same calls are accepted and exact."""
    lib = _lib.load()
    st = stream_of(device)
    N, T = R.SHORT_N, 23
    C1, C2 = widths
    c = R.int_case(widths, N, T)
    d = _upload(c, device, False)
    ng = R.grad_len(C1, C2)
    G = lib.pcgmix_potes_narrow_bwd_blocks(N, T, C1, C2)
    size = (N, T, C1, C2)
    bufs = {"h2": _floats(N * C2 * c.P2, device), "partial": _floats(G * ng, device), "grads": _floats(ng, device),
            "gx": _floats(N * T, device)}
    m2, s1 = _complement(c.m2, device), _complement(c.s1, device)
    ptr = {"x": d.x.data_ptr(), "g": d.r.data_ptr(), "w1": d.w1.data_ptr(), "b1": d.b1.data_ptr(),
           "w2": d.w2.data_ptr(), "b2": d.b2.data_ptr(), "m2in": d.m2.data_ptr(), "s1in": d.s1.data_ptr(),
           "m2": m2.data_ptr(), "s1": s1.data_ptr(), **{k: v.data_ptr() for k, v in bufs.items()}}
    for call, args in _REFUSED:
        for arg in args:
            assert call(lib, {**ptr, arg: None}, size, st) == INVALID, (call.__name__, arg)
    torch.cuda.synchronize()
    problems = []
    for name, b in bufs.items():
        assert bool((b == SENT).all()), name
    _untouched(m2, c.m2, "m2", problems)
    _untouched(s1, c.s1, "s1", problems)
    assert not problems, "\n".join(problems)
    for call, _ in _REFUSED:
        assert call(lib, ptr, size, st) == 0, call.__name__
    _same("h2", _owned(bufs["h2"], N * C2 * c.P2, "h2", problems), c.ref.h2, problems)
    _same("grads", _owned(bufs["grads"], ng, "grads", problems), c.ref.grads, problems)
    _same("gx", _owned(bufs["gx"], N * T, "gx", problems), c.ref.gx, problems)
    _bytes(m2, c.m2, "m2", problems)
    _bytes(s1, c.s1, "s1", problems)
    assert not problems, "\n".join(problems)
