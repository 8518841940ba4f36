"""The wide ([8,4]) Potes conv stack (csrc/pcgmix_potes.hip) at its tile edges, through the C ABI,
against the float64 restatement of tests/potes_ref.py.

  * integer data (potes_ref.int_case): float32 in any order is exact, so every output — both
    forwards, the routing bytes m2 / s1, the 212 weight gradients of both backward families (reduced
    in the call and by pcgmix_potes_reduce_f32), both input gradients — must equal float64 BIT FOR
    BIT, with exact ties (first maximum wins) and exact zeros (dead) in a few per cent of the pairs;
  * every output buffer is sentinel-filled and over-allocated: each owned element is written (the
    routing bytes' padding bit positions and grad_x's zeros under dead ReLUs included), no guard
    element is;
  * random data whose ReLU/pool decisions float32 rounding cannot flip (potes_ref.undecidable == 0):
    routing bytes exact, values within the limits of tests/test_potes_gpu.py;
  * the persistent loops make second and later trips: PCGMIX_POTES_{FWD,BWD,INGRAD}_BLOCKS in
    {1, 2, 3}, and the default caps crossed at T = 14;
  * refusals launch nothing and write nothing.
The shape table is potes_ref.EDGE_T (tests/test_potes_ref_cpu.py::test_shapes_cover_tile_edges says
what it covers)."""
import ctypes
import types

import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import potes_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                          # hipErrorInvalidValue
SENT = -12345.0                      # no output can hold it: h2 >= 0, integer gradients are far smaller
GUARD = 64
ENV = ("PCGMIX_POTES_FWD_BLOCKS", "PCGMIX_POTES_BWD_BLOCKS", "PCGMIX_POTES_INGRAD_BLOCKS")
FWD_CAP, BWD_CAP, INGRAD_CAP = 1024, 1024, 3072
VALUES = ("h2 (fwd)", "h2 (fwd_save)", "grads (bwd_mask)", "grads (bwd_mask + reduce)", "grads (bwd)",
          "gx (input_grad_mask)", "gx (input_grad)")
GRID_FREE = ("h2 (fwd)", "h2 (fwd_save)", "m2", "s1", "gx (input_grad_mask)", "gx (input_grad)")


@pytest.fixture(autouse=True)
def default_grids(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def stream_of(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _upload(c, device):
    return types.SimpleNamespace(**{k: getattr(c, k).to(device).contiguous()
                                    for k in ("x", "w1", "b1", "w2", "b2", "r")})


def _guarded(n, device, byte=False):
    if byte:
        return torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=device)
    return torch.full((n + GUARD,), SENT, device=device)


def _owned(buf, n, name, problems):
    """The n owned elements of a sentinel-filled buffer: all written, and the guard behind them not."""
    sent = 0xFF if buf.dtype == torch.uint8 else SENT
    left = int((buf[:n] == sent).sum())
    if left:
        problems.append(f"{name}: {left} of {n} owned elements were not written")
    if not bool((buf[n:] == sent).all()):
        problems.append(f"{name}: guard elements behind the buffer were written")
    return buf[:n]


def run_all(lib, c, device, problems):
    """Every entry point once on case c.  Returns name -> flat CPU tensor."""
    d = _upload(c, device)
    N, T, P1, P2 = c.N, c.T, c.P1, c.P2
    st = stream_of(device)
    w = (d.w1.data_ptr(), d.b1.data_ptr(), d.w2.data_ptr(), d.b2.data_ptr())
    nm2, ns1 = lib.pcgmix_potes_mask_bytes(N, T, 2), lib.pcgmix_potes_mask_bytes(N, T, 1)
    assert lib.pcgmix_potes_out_len(T) == P2
    assert nm2 == N * 4 * ((P2 + 3) // 4) and ns1 == N * 8 * ((P1 >> 2) + 1)
    out = {}

    h = _guarded(N * 4 * P2, device)
    _lib.check(lib.pcgmix_potes_stack_fwd_f32(d.x.data_ptr(), *w, h.data_ptr(), N, T, st), "fwd")
    out["h2 (fwd)"] = _owned(h, N * 4 * P2, "h2 (fwd)", problems)

    h, m2, s1 = _guarded(N * 4 * P2, device), _guarded(nm2, device, True), _guarded(ns1, device, True)
    _lib.check(lib.pcgmix_potes_stack_fwd_save_f32(d.x.data_ptr(), *w, h.data_ptr(), m2.data_ptr(),
                                                   s1.data_ptr(), N, T, None, 0, None, 0, st), "fwd_save")
    out["h2 (fwd_save)"] = _owned(h, N * 4 * P2, "h2 (fwd_save)", problems)
    out["m2"] = _owned(m2, nm2, "m2", problems)
    out["s1"] = _owned(s1, ns1, "s1", problems)

    # the backward kernels read the routing the forward just wrote
    G = lib.pcgmix_potes_bwd_blocks(N, T)
    assert 1 <= G <= N * R.bwd_tiles(T)
    partial, grads = _guarded(G * R.NGRAD, device), _guarded(R.NGRAD, device)
    _lib.check(lib.pcgmix_potes_stack_bwd_mask_f32(d.x.data_ptr(), d.r.data_ptr(), m2.data_ptr(), *w,
                                                   partial.data_ptr(), grads.data_ptr(), N, T, st), "bwd_mask")
    _owned(partial, G * R.NGRAD, "partial (bwd_mask)", problems)
    out["grads (bwd_mask)"] = _owned(grads, R.NGRAD, "grads (bwd_mask)", problems)

    partial, grads = _guarded(G * R.NGRAD, device), _guarded(R.NGRAD, device)
    _lib.check(lib.pcgmix_potes_stack_bwd_mask_f32(d.x.data_ptr(), d.r.data_ptr(), m2.data_ptr(), *w,
                                                   partial.data_ptr(), None, N, T, st), "bwd_mask, grads = NULL")
    _lib.check(lib.pcgmix_potes_reduce_f32(partial.data_ptr(), grads.data_ptr(), G, st), "reduce")
    _owned(partial, G * R.NGRAD, "partial (bwd_mask, grads = NULL)", problems)
    out["grads (bwd_mask + reduce)"] = _owned(grads, R.NGRAD, "grads (bwd_mask + reduce)", problems)

    partial, grads = _guarded(G * R.NGRAD, device), _guarded(R.NGRAD, device)
    _lib.check(lib.pcgmix_potes_stack_bwd_f32(d.x.data_ptr(), d.r.data_ptr(), *w, partial.data_ptr(),
                                              grads.data_ptr(), N, T, st), "bwd")
    _owned(partial, G * R.NGRAD, "partial (bwd)", problems)
    out["grads (bwd)"] = _owned(grads, R.NGRAD, "grads (bwd)", problems)

    gx = _guarded(N * T, device)
    _lib.check(lib.pcgmix_potes_stack_input_grad_mask_f32(d.r.data_ptr(), m2.data_ptr(), s1.data_ptr(),
                                                          w[0], w[2], gx.data_ptr(), N, T, st), "input_grad_mask")
    out["gx (input_grad_mask)"] = _owned(gx, N * T, "gx (input_grad_mask)", problems)

    gx = _guarded(N * T, device)
    _lib.check(lib.pcgmix_potes_stack_input_grad_f32(d.x.data_ptr(), d.r.data_ptr(), *w, gx.data_ptr(),
                                                     N, T, st), "input_grad")
    out["gx (input_grad)"] = _owned(gx, N * T, "gx (input_grad)", problems)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _want(c):
    ref = c.ref
    return {"h2 (fwd)": ref.h2, "h2 (fwd_save)": ref.h2, "m2": c.m2, "s1": c.s1,
            "grads (bwd_mask)": ref.grads, "grads (bwd_mask + reduce)": ref.grads, "grads (bwd)": ref.grads,
            "gx (input_grad_mask)": ref.gx, "gx (input_grad)": ref.gx}


def _same(name, got, want, problems):
    """Bit equality (float32 outputs widened to float64 first); a mismatch says where."""
    got, want = got.reshape(-1), want.reshape(-1)
    if got.dtype != torch.uint8:
        got = got.double()
    if got.shape == want.shape and torch.equal(got, want):
        return
    bad = (got != want).nonzero().flatten()
    i = int(bad[0])
    problems.append(f"{name}: {bad.numel()} of {want.numel()} differ, first at {i} (got {got[i].item()}, "
                    f"want {want[i].item()}), last at {int(bad[-1])}")


def check_exact(c, out, problems):
    for name, want in _want(c).items():
        _same(name, out[name], want, problems)


def check_close(c, out, problems, names=VALUES, tag=""):
    """The limits of tests/test_potes_gpu.py against float64: h2 rtol 1e-4 / atol 1e-5; parameter
    gradients <= 2e-4 max|ref| per tensor; grad_x <= 1e-4 max|ref|.  Prints the observed maxima."""
    for name in names:
        got, want = out[name].double().reshape(-1), _want(c)[name].reshape(-1)
        if name.startswith("h2"):
            err = float((got - want).abs().max())
            print(f"{tag}{name}: max |diff| {err:.3g}")
            if not torch.allclose(got, want, rtol=1e-4, atol=1e-5):
                problems.append(f"{name}: max |diff| {err:.3g} outside rtol 1e-4, atol 1e-5")
        elif name.startswith("gx"):
            err, scale = float((got - want).abs().max()), float(want.abs().max())
            print(f"{tag}{name}: max |diff| {err:.3g} of {scale:.3g}")
            if not err <= 1e-4 * scale:
                problems.append(f"{name}: {err:.3g} > 1e-4 * {scale:.3g}")
        else:
            lo = 0
            for part, n in (("w1", 40), ("b1", 8), ("w2", 160), ("b2", 4)):
                a, b = got[lo:lo + n], want[lo:lo + n]
                lo += n
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                print(f"{tag}{name} {part}: max |diff| {err:.3g} of {scale:.3g}")
                if not err <= 2e-4 * scale:
                    problems.append(f"{name} {part}: {err:.3g} > 2e-4 * {scale:.3g}")


def _int_case(N, T):
    c = R.int_case(N, T)
    assert max(float(c.ref.gx.abs().max()), float(c.ref.grads.abs().max())) < -SENT
    return c


def _rand_case(N, T):
    c = R.rand_case(N, T)
    assert c.undecidable == 0, f"rand_case({N}, {T}, seed={c.seed}): {c.undecidable} undecidable positions"
    return c


@pytest.mark.parametrize("T", R.EDGE_T)
def test_integer_exact(T, device):
    """a + b of the suite: bit equality with float64 on integer data, every owned element written,
    every guard intact.  The padding bit positions of m2 and s1 are part of the comparison (the
    forward writes code 0 there).  Where T % 4 == 0 the forward also runs from a base 4 bytes off a
    16-byte boundary, i.e. both staging paths see the same tile edges."""
    lib = _lib.load()
    c = _int_case(R.EDGE_N, T)
    problems = []
    out = run_all(lib, c, device, problems)
    check_exact(c, out, problems)
    if T % 4 == 0:
        N, P2 = c.N, c.P2
        buf = torch.zeros(N * T + 1, device=device)
        x_un = buf[1:]
        x_un.copy_(c.x.reshape(-1))
        assert x_un.data_ptr() % 16 == 4
        w = [t.to(device) for t in (c.w1, c.b1, c.w2, c.b2)]
        h = _guarded(N * 4 * P2, device)
        m2, s1 = _guarded(c.m2.numel(), device, True), _guarded(c.s1.numel(), device, True)
        _lib.check(lib.pcgmix_potes_stack_fwd_save_f32(
            x_un.data_ptr(), *[t.data_ptr() for t in w], h.data_ptr(), m2.data_ptr(), s1.data_ptr(), N, T,
            None, 0, None, 0, stream_of(device)), "fwd_save, unaligned base")
        for name, b, want in (("h2", h, c.ref.h2), ("m2", m2, c.m2), ("s1", s1, c.s1)):
            name += " (fwd_save, unaligned base)"
            _same(name, _owned(b, want.numel(), name, problems).cpu(), want, problems)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("T", R.EDGE_T)
def test_random_parity(T, device):
    """c: randn data with no decision float32 could flip (asserted, seed named): the routing bytes
    equal the float64 packing exactly, values within the project's limits, both backward families."""
    lib = _lib.load()
    c = _rand_case(R.EDGE_N, T)
    problems = []
    out = run_all(lib, c, device, problems)
    _same("m2", out["m2"], c.m2, problems)
    _same("s1", out["s1"], c.s1, problems)
    check_close(c, out, problems, tag=f"T={T} ")
    assert not problems, "\n".join(problems)


def _cap(monkeypatch, blocks):
    for name in ENV:
        monkeypatch.setenv(name, str(blocks))


@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("T", R.PERSIST_T)
def test_persistent_loops_integer_exact(T, blocks, monkeypatch, device):
    """d: 1-3 blocks walk all items of 5 rows (the forward has 5-15 items, the weight gradient 10-25,
    the input gradient 10-25): registers prefetched for the next item, LDS reused, the once-zeroed
    pads.  Integer sums do not depend on the grid, so the weight gradients are exact too."""
    lib = _lib.load()
    c = _int_case(R.PERSIST_N, T)
    work = c.N * R.bwd_tiles(T)
    _cap(monkeypatch, blocks)
    assert lib.pcgmix_potes_bwd_blocks(c.N, T) == min(blocks, work)       # read per call
    problems = []
    out = run_all(lib, c, device, problems)
    check_exact(c, out, problems)
    monkeypatch.delenv(ENV[1])
    assert lib.pcgmix_potes_bwd_blocks(c.N, T) == work < BWD_CAP
    assert not problems, "\n".join(problems)


_DEFAULT_GRID = {}       # T -> outputs of the default-grid run on the random case


@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("T", R.PERSIST_T)
def test_persistent_loops_random(T, blocks, monkeypatch, device):
    """d: on randn data nothing but the weight gradients' summation order depends on the grid: forward
    outputs, routing bytes and both input gradients are bit-equal to the default-grid run; the
    weight gradients stay within the limit against float64."""
    lib = _lib.load()
    c = _rand_case(R.PERSIST_N, T)
    problems = []
    if T not in _DEFAULT_GRID:
        base = run_all(lib, c, device, problems)
        _same("m2", base["m2"], c.m2, problems)
        _same("s1", base["s1"], c.s1, problems)
        check_close(c, base, problems, tag=f"T={T} default grid: ")
        assert not problems, "\n".join(problems)
        _DEFAULT_GRID[T] = base
    base = _DEFAULT_GRID[T]
    _cap(monkeypatch, blocks)
    out = run_all(lib, c, device, problems)
    for name in GRID_FREE:
        _same(f"{name}, {blocks} blocks against the default grid", out[name],
              base[name] if base[name].dtype == torch.uint8 else base[name].double(), problems)
    check_close(c, out, problems, names=[n for n in VALUES if n.startswith("grads")], tag=f"T={T} {blocks} blocks: ")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("N", [1100, 3100])
def test_default_caps_crossed(N, device):
    """d: without any variable set, N one-tile rows of T = 14 exceed the default caps: 1100 items over
    1024 blocks in the forward and both weight gradients, 3100 over 3072 in the input gradient — some
    blocks make a second trip, most do not."""
    lib = _lib.load()
    T = 14
    assert R.fwd_tiles(T) == R.bwd_tiles(T) == R.in_tiles(T) == 1
    assert N > max(FWD_CAP, BWD_CAP) and (N == 1100 or N > INGRAD_CAP)
    assert lib.pcgmix_potes_bwd_blocks(N, T) == BWD_CAP
    c = _int_case(N, T)
    problems = []
    out = run_all(lib, c, device, problems)
    check_exact(c, out, problems)
    assert not problems, "\n".join(problems)


# ---- refusals ---------------------------------------------------------------------------------
# entry point -> (required pointer arguments, call(lib, p, N, T, stream)); p: name -> address or None
_CALLS = {
    "pcgmix_potes_stack_fwd_f32": (
        ("x", "w1", "b1", "w2", "b2", "h2"),
        lambda lib, p, N, T, st: lib.pcgmix_potes_stack_fwd_f32(
            p["x"], p["w1"], p["b1"], p["w2"], p["b2"], p["h2"], N, T, st)),
    "pcgmix_potes_stack_fwd_save_f32": (
        ("x", "w1", "b1", "w2", "b2", "h2", "m2"),
        lambda lib, p, N, T, st: lib.pcgmix_potes_stack_fwd_save_f32(
            p["x"], p["w1"], p["b1"], p["w2"], p["b2"], p["h2"], p["m2"], p["s1"], N, T, None, 0, None, 0, st)),
    "pcgmix_potes_stack_bwd_f32": (
        ("x", "g", "w1", "b1", "w2", "b2", "partial", "grads"),
        lambda lib, p, N, T, st: lib.pcgmix_potes_stack_bwd_f32(
            p["x"], p["g"], p["w1"], p["b1"], p["w2"], p["b2"], p["partial"], p["grads"], N, T, st)),
    "pcgmix_potes_stack_bwd_mask_f32": (
        ("x", "g", "m2", "w1", "b1", "w2", "b2", "partial"),
        lambda lib, p, N, T, st: lib.pcgmix_potes_stack_bwd_mask_f32(
            p["x"], p["g"], p["m2"], p["w1"], p["b1"], p["w2"], p["b2"], p["partial"], p["grads"], N, T, st)),
    "pcgmix_potes_stack_input_grad_f32": (
        ("x", "g", "w1", "b1", "w2", "b2", "gx"),
        lambda lib, p, N, T, st: lib.pcgmix_potes_stack_input_grad_f32(
            p["x"], p["g"], p["w1"], p["b1"], p["w2"], p["b2"], p["gx"], N, T, st)),
    "pcgmix_potes_stack_input_grad_mask_f32": (
        ("g", "m2", "s1", "w1", "w2", "gx"),
        lambda lib, p, N, T, st: lib.pcgmix_potes_stack_input_grad_mask_f32(
            p["g"], p["m2"], p["s1"], p["w1"], p["w2"], p["gx"], N, T, st)),
}
_ACCEPT_N0 = ("pcgmix_potes_stack_fwd_f32", "pcgmix_potes_stack_fwd_save_f32",
              "pcgmix_potes_stack_input_grad_f32", "pcgmix_potes_stack_input_grad_mask_f32")


def test_refusals_leave_outputs_untouched(device):
    """e: T = 13, N = 65536 (and a negative N), NULL for each required pointer in turn — m2 = NULL for
    the saving forward among them — at the six stack entry points, and NULL / G <= 0 at the seventh,
    pcgmix_potes_reduce_f32: hipErrorInvalidValue, no launch, sentinel-filled outputs untouched.
    N = 0 is success without a launch where the entry point accepts it (the forwards and the input
    gradients; the weight gradients refuse it: they would reduce zero partials)."""
    lib = _lib.load()
    st = stream_of(device)
    N, T = 4, 64
    P1, P2 = R.dims(T)
    c = R.int_case(N, T)
    d = _upload(c, device)
    bufs = {"h2": torch.full((N * 4 * P2,), SENT, device=device), "gx": torch.full((N * T,), SENT, device=device),
            "partial": torch.full((N * R.NGRAD,), SENT, device=device),
            "grads": torch.full((R.NGRAD,), SENT, device=device),
            "m2": torch.full((c.m2.numel(),), 0xA5, dtype=torch.uint8, device=device),
            "s1": torch.full((c.s1.numel(),), 0xA5, dtype=torch.uint8, device=device)}
    ptr = {"x": d.x.data_ptr(), "g": d.r.data_ptr(), "w1": d.w1.data_ptr(), "b1": d.b1.data_ptr(),
           "w2": d.w2.data_ptr(), "b2": d.b2.data_ptr(), **{k: v.data_ptr() for k, v in bufs.items()}}
    for name, (required, call) in _CALLS.items():
        assert call(lib, ptr, N, 13, st) == INVALID, (name, "T = 13")
        assert call(lib, ptr, 65536, T, st) == INVALID, (name, "N = 65536")
        assert call(lib, ptr, -1, T, st) == INVALID, (name, "N = -1")
        for arg in required:
            assert call(lib, {**ptr, arg: None}, N, T, st) == INVALID, (name, arg)
        assert call(lib, ptr, 0, T, st) == (0 if name in _ACCEPT_N0 else INVALID), (name, "N = 0")
    for partial, grads, G in ((None, ptr["grads"], 4), (ptr["partial"], None, 4), (ptr["partial"], ptr["grads"], 0),
                              (ptr["partial"], ptr["grads"], -1)):
        assert lib.pcgmix_potes_reduce_f32(partial, grads, G, st) == INVALID
    assert lib.pcgmix_potes_out_len(13) == 0 and lib.pcgmix_potes_bwd_blocks(N, 13) == 0
    assert lib.pcgmix_potes_bwd_blocks(0, T) == 0 and lib.pcgmix_potes_mask_bytes(N, 13, 2) == 0
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert bool((b == (0xA5 if b.dtype == torch.uint8 else SENT)).all()), name
    # the optional pointers really are optional: the same arguments are accepted with them NULL
    assert _CALLS["pcgmix_potes_stack_fwd_save_f32"][1](lib, {**ptr, "s1": None}, N, T, st) == 0
    assert _CALLS["pcgmix_potes_stack_bwd_mask_f32"][1](lib, {**ptr, "grads": None}, N, T, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(bufs["h2"].cpu().double(), c.ref.h2.reshape(-1))
    assert torch.equal(bufs["m2"].cpu(), c.m2.reshape(-1))
    assert bool((bufs["s1"] == 0xA5).all()) and bool((bufs["grads"] == SENT).all())
