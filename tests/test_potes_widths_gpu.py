"""The narrow Potes conv stacks (layers [1,1] and [2,1], csrc/pcgmix_potes_narrow.hip) against the
same stack through torch/MIOpen ops on the same device (``m.fused = False``) in float32 — method and
tolerances of tests/test_potes_gpu.py — plus the ABI's refusals, the dropout bytes, the training
steps of 'Potes0.1' and the reference's recorded logits (tests/golden/model_sizes.npz).
Tile edges, routing bytes and exact arithmetic against float64: tests/test_potes_narrow_edges_gpu.py."""
import argparse
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, models, synthetic, train_model as tm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

INVALID = 1                         # hipErrorInvalidValue
WIDTHS = [(1, 1), (2, 1)]
# kNarTP = 256 (pcgmix_potes_narrow.hip): pooled outputs per tile, one per thread.  P2 = ((T-2)//2 - 2)//2:
#   T = 1027 -> P2 = 255 (one tile minus one output), 1032 -> 256 (exactly one tile), 1034 -> 257
# (one tile plus one).  With the shapes of test_potes_gpu.py all four residues of T mod 4 occur
# (2500, 1032: 0; 1037: 1; 14, 526, 1030, 1034: 2; 23, 1027: 3) — they decide the two pool truncations.
TILE = 256
TILE_T = [1027, 1032, 1034]
# Further lengths at which the kernels change path: 1024 / 1025 — one / two blocks of the input
# gradient (1024 inputs per block) and the last length whose routing bytes fit one forward tile;
# 1028 — the weight gradient's first-layer positions ((P1+1)//2 = 257) need a second tile.
SHAPES = [(2, 14), (1, 23), (3, 526), (2, 1030), (3, 1037), (4, 2500)] + \
    [(2, T) for T in TILE_T] + [(1, 1024), (2, 1025), (1, 1028)]


def _p2(T):
    return ((T - 2) // 2 - 2) // 2


def test_shapes_cover_tile_edges_and_residues():
    assert [_p2(T) for T in TILE_T] == [TILE - 1, TILE, TILE + 1]
    assert {T % 4 for _, T in SHAPES} == {0, 1, 2, 3}


def make(widths, T, device, seed=0):
    torch.manual_seed(seed)
    return models.CNN_potes(4, 2, list(widths), models.potes_flat_features(T, width=widths[1])).to(device)


def stack_params(m):
    c1, c2 = m.cnn1[0][0], m.cnn1[1][0]
    return [c1.weight, c1.bias, c2.weight, c2.bias]


def stream_of(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


@pytest.mark.parametrize("widths", WIDTHS, ids=str)
@pytest.mark.parametrize("B,T", SHAPES)
def test_forward_matches_torch(widths, B, T, device):
    m = make(widths, T, device).eval()
    x = torch.randn(B, 4, T, device=device)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)         # the HIP path: no fall-back warning
        assert m._fused(x) and m._fused_head(x)
        y_f = m(x)
        h_f = models.PotesStackFunction.apply(x.reshape(B * 4, T), *stack_params(m))
    m.fused = False
    y_t = m(x)
    err = float((y_f - y_t).abs().max())
    print(f"logits {widths} ({B},{T}): max |diff| {err:.3g}")
    assert torch.allclose(y_f, y_t, rtol=1e-4, atol=1e-5), err
    h_t = m.cnn1(x.reshape(B * 4, 1, T))
    assert h_f.shape == h_t.shape == (B * 4, widths[1], _p2(T))
    print(f"stack: max |diff| {float((h_f - h_t).abs().max()):.3g}")
    assert torch.allclose(h_f, h_t, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("widths", WIDTHS, ids=str)
@pytest.mark.parametrize("B,T", SHAPES)
def test_weight_gradients_match_torch(widths, B, T, device):
    """dL/d{w1,b1,w2,b2} of a random linear functional of the stack output."""
    m = make(widths, T, device, seed=1).eval()
    x = torch.randn(B, 4, T, device=device)
    params = stack_params(m)
    h_t = m.cnn1(x.reshape(B * 4, 1, T))
    r = torch.randn_like(h_t)
    g_t = torch.autograd.grad((h_t * r).sum(), params)
    h_f = models.PotesStackFunction.apply(x.reshape(B * 4, T), *params)
    g_f = torch.autograd.grad((h_f * r).sum(), params)
    for a, b, name in zip(g_f, g_t, ("w1", "b1", "w2", "b2")):
        assert a.shape == b.shape
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        print(f"{name} {widths} ({B},{T}): max |diff| {err:.3g} of {scale:.3g}")
        assert err <= 2e-4 * scale, (name, err, scale)


@pytest.mark.parametrize("widths", WIDTHS, ids=str)
@pytest.mark.parametrize("B,T", SHAPES)
def test_input_gradient_matches_torch(widths, B, T, device):
    m = make(widths, T, device, seed=3).eval()
    params = stack_params(m)
    x1 = torch.randn(B * 4, T, device=device, requires_grad=True)
    x2 = x1.detach().clone().requires_grad_(True)
    h_t = m.cnn1(x1.unsqueeze(1))
    r = torch.randn_like(h_t)
    (g_t,) = torch.autograd.grad((h_t * r).sum(), x1)
    h_f = models.PotesStackFunction.apply(x2, *params)
    (g_f,) = torch.autograd.grad((h_f * r).sum(), x2)
    scale = float(g_t.abs().max())
    err = float((g_f - g_t).abs().max())
    print(f"dx {widths} ({B},{T}): max |diff| {err:.3g} of {scale:.3g}")
    assert err <= 1e-4 * scale
    # whole model, saliency style: through autograd, not the [8,4]-only one-call chain
    from pcgmix_amd import saliency
    xa = torch.randn(B, 4, T, device=device)
    assert saliency._potes_direct(m, xa) is None
    seed = torch.nn.functional.one_hot(torch.arange(B, device=device) % 2, 2).float()
    m.fused = True
    g_a = saliency.input_gradient_seeded(m, xa, seed)
    m.fused = False
    g_b = saliency.input_gradient_seeded(m, xa, seed)
    assert torch.allclose(g_a, g_b, rtol=1e-3, atol=1e-5 * float(g_b.abs().max()) + 1e-9)


def _call_forward(lib, x, params, N, T, C1, C2, device, s1=True, rnd=None, key=0, key_dev=None):
    h2 = torch.empty(N, C2, _p2(T), device=device)
    m2 = torch.zeros(lib.pcgmix_potes_narrow_mask_bytes(N, T, C1, C2, 2), dtype=torch.uint8, device=device)
    s = torch.zeros(lib.pcgmix_potes_narrow_mask_bytes(N, T, C1, C2, 1), dtype=torch.uint8,
                    device=device) if s1 else None
    _lib.check(lib.pcgmix_potes_narrow_fwd_f32(
        x.data_ptr(), *[p.data_ptr() for p in params], h2.data_ptr(), m2.data_ptr(),
        s.data_ptr() if s1 else None, N, T, C1, C2, rnd.data_ptr() if rnd is not None else None,
        rnd.numel() if rnd is not None else 0, key_dev.data_ptr() if key_dev is not None else None,
        0 if key_dev is not None else key, stream_of(device)), "pcgmix_potes_narrow_fwd_f32")
    return h2, m2, s


@pytest.mark.parametrize("widths", WIDTHS, ids=str)
@pytest.mark.parametrize("N,T", [(3, 23), (2, 1025), (3, 1037), (2, 2500)])
def test_input_gradient_writes_every_element(widths, N, T, device):
    """Every element of grad_x is written, the zeros included (inputs under dead ReLUs, the row's
    end behind the last kept pooled output): a sentinel-filled buffer keeps no sentinel, and the
    guard words behind it keep theirs."""
    C1, C2 = widths
    lib = _lib.load()
    m = make(widths, T, device, seed=5).eval()
    params = [p.detach() for p in stack_params(m)]
    x = torch.randn(N, T, device=device)
    h2, m2, s1 = _call_forward(lib, x, params, N, T, C1, C2, device)
    g = torch.randn_like(h2)
    SENT = -12345.0
    buf = torch.full((N * T + 64,), SENT, device=device)
    _lib.check(lib.pcgmix_potes_narrow_input_grad_mask_f32(
        g.data_ptr(), m2.data_ptr(), s1.data_ptr(), params[0].data_ptr(), params[2].data_ptr(),
        buf.data_ptr(), N, T, C1, C2, stream_of(device)), "input_grad")
    gx = buf[:N * T].view(N, T)
    assert not bool((gx == SENT).any())
    assert bool((buf[N * T:] == SENT).all())
    x1 = x.clone().requires_grad_(True)
    (g_t,) = torch.autograd.grad((m.cnn1(x1.unsqueeze(1)) * g).sum(), x1)
    assert float((gx - g_t).abs().max()) <= 1e-4 * float(g_t.abs().max())


@pytest.mark.parametrize("key_on_device", [False, True], ids=["key_host", "key_device"])
@pytest.mark.parametrize("widths", WIDTHS, ids=str)
def test_dropout_bytes_equal_the_wide_stack(widths, key_on_device, device):
    """For one key and length the narrow forward and pcgmix_potes_stack_fwd_save_f32 fill the same
    bytes (one counter_hash, one fill loop); rnd_out == NULL fills nothing; the forward's own
    outputs do not depend on the fill."""
    C1, C2 = widths
    lib = _lib.load()
    N, T = 8, 526
    m = make(widths, T, device).eval()
    params = [p.detach() for p in stack_params(m)]
    wide = [p.detach() for p in stack_params(make((8, 4), T, device))]
    x = torch.randn(N, T, device=device)
    key = 0x0123456789ABCDEF
    kd = torch.tensor([key & 0xFFFFFFFF, key >> 32], dtype=torch.int64).to(torch.int32).to(device) \
        if key_on_device else None
    h_ref, m_ref, s_ref = _call_forward(lib, x, params, N, T, C1, C2, device)
    for nbytes in (16, 16 * 37, 16 * 70001):            # less than, and far more than, the launch's threads
        a = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=device)
        b = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=device)
        h2, m2, s1 = _call_forward(lib, x, params, N, T, C1, C2, device, rnd=a[:nbytes], key=key, key_dev=kd)
        hw = torch.empty(N, 4, _p2(T), device=device)
        mw = torch.empty(lib.pcgmix_potes_mask_bytes(N, T, 2), dtype=torch.uint8, device=device)
        _lib.check(lib.pcgmix_potes_stack_fwd_save_f32(
            x.data_ptr(), *[p.data_ptr() for p in wide], hw.data_ptr(), mw.data_ptr(), None, N, T,
            b.data_ptr(), nbytes, kd.data_ptr() if kd is not None else None,
            0 if kd is not None else key, stream_of(device)), "wide forward")
        assert torch.equal(a, b)
        assert bool((a[nbytes:] == 0xA5).all()) and not bool((a[:nbytes] == 0xA5).all())
        assert torch.equal(h2, h_ref) and torch.equal(m2, m_ref) and torch.equal(s1, s_ref)
    # rnd_out == NULL: rnd_bytes, key_dev and key are ignored — the call is accepted, the forward's
    # outputs are the same, and the one buffer of the fill's arguments the kernel could still reach
    # (the device key words) keeps its bytes
    keybuf = torch.full((64,), 0xA5, dtype=torch.uint8, device=device)
    h2 = torch.empty(N, C2, _p2(T), device=device)
    m2 = torch.empty_like(m_ref)
    _lib.check(lib.pcgmix_potes_narrow_fwd_f32(
        x.data_ptr(), *[p.data_ptr() for p in params], h2.data_ptr(), m2.data_ptr(), None, N, T, C1, C2,
        None, 64, keybuf.data_ptr(), key, stream_of(device)), "forward without rnd")
    assert bool((keybuf == 0xA5).all()) and torch.equal(h2, h_ref) and torch.equal(m2, m_ref)
    mis = torch.zeros(48, dtype=torch.uint8, device=device)
    for bad_ptr, bad_n in ((mis.data_ptr() + 4, 32), (mis.data_ptr(), 24)):     # misaligned; not 16 k
        assert lib.pcgmix_potes_narrow_fwd_f32(
            x.data_ptr(), *[p.data_ptr() for p in params], h2.data_ptr(), m2.data_ptr(), None, N, T,
            C1, C2, bad_ptr, bad_n, None, key, stream_of(device)) == INVALID
    torch.cuda.synchronize()
    assert not bool(mis.any())


def test_refusals_leave_outputs_untouched(device):
    """Unsupported widths, T < 14, NULL pointers, grads == NULL: hipErrorInvalidValue, no launch."""
    lib = _lib.load()
    st = stream_of(device)
    N, T = 4, 64
    SENT = -777.0
    x = torch.randn(N, T, device=device)
    w = {c: [torch.randn(c[0], 1, 5, device=device), torch.randn(c[0], device=device),
             torch.randn(c[1], c[0], 5, device=device), torch.randn(c[1], device=device)]
         for c in ((2, 1), (3, 2))}
    big = lambda: torch.full((N * 4 * T,), SENT, device=device)      # noqa: E731  (any layout fits)
    mask = lambda: torch.full((N * 4 * T,), 0xA5, dtype=torch.uint8, device=device)      # noqa: E731
    for (C1, C2), Tc, Nc in (((3, 2), T, N), ((2, 1), 13, N), ((2, 1), T, -1), ((8, 4), T, N)):
        p = [t.data_ptr() for t in w[(C1, C2) if (C1, C2) in w else (3, 2)]]
        h2, m2, s1, part, grads, gx = big(), mask(), mask(), big(), big(), big()
        assert lib.pcgmix_potes_narrow_fwd_f32(x.data_ptr(), *p, h2.data_ptr(), m2.data_ptr(),
                                               s1.data_ptr(), Nc, Tc, C1, C2, None, 0, None, 0, st) == INVALID
        assert lib.pcgmix_potes_narrow_bwd_mask_f32(x.data_ptr(), h2.data_ptr(), m2.data_ptr(), *p,
                                                    part.data_ptr(), grads.data_ptr(), Nc, Tc, C1, C2,
                                                    st) == INVALID
        assert lib.pcgmix_potes_narrow_input_grad_mask_f32(h2.data_ptr(), m2.data_ptr(), s1.data_ptr(),
                                                           p[0], p[2], gx.data_ptr(), Nc, Tc, C1, C2,
                                                           st) == INVALID
        torch.cuda.synchronize()
        for t in (h2, part, grads, gx):
            assert bool((t == SENT).all())
        assert bool((m2 == 0xA5).all()) and bool((s1 == 0xA5).all())
    # NULL required pointers, and the deferred reduction (grads == NULL) this stack does not have
    p = [t.data_ptr() for t in w[(2, 1)]]
    h2, m2, s1, part, grads, gx = big(), mask(), mask(), big(), big(), big()
    assert lib.pcgmix_potes_narrow_fwd_f32(None, *p, h2.data_ptr(), m2.data_ptr(), None, N, T, 2, 1,
                                           None, 0, None, 0, st) == INVALID
    assert lib.pcgmix_potes_narrow_fwd_f32(x.data_ptr(), *p, None, m2.data_ptr(), None, N, T, 2, 1,
                                           None, 0, None, 0, st) == INVALID
    assert lib.pcgmix_potes_narrow_bwd_mask_f32(x.data_ptr(), h2.data_ptr(), m2.data_ptr(), *p,
                                                part.data_ptr(), None, N, T, 2, 1, st) == INVALID
    assert lib.pcgmix_potes_narrow_bwd_mask_f32(x.data_ptr(), h2.data_ptr(), None, *p,
                                                part.data_ptr(), grads.data_ptr(), N, T, 2, 1, st) == INVALID
    assert lib.pcgmix_potes_narrow_input_grad_mask_f32(h2.data_ptr(), m2.data_ptr(), None, p[0], p[2],
                                                       gx.data_ptr(), N, T, 2, 1, st) == INVALID
    torch.cuda.synchronize()
    for t in (h2, part, grads, gx):
        assert bool((t == SENT).all())
    # N == 0: success, nothing launched
    assert lib.pcgmix_potes_narrow_fwd_f32(x.data_ptr(), *p, h2.data_ptr(), m2.data_ptr(), None, 0, T,
                                           2, 1, None, 0, None, 0, st) == 0
    assert lib.pcgmix_potes_narrow_input_grad_mask_f32(h2.data_ptr(), m2.data_ptr(), s1.data_ptr(),
                                                       p[0], p[2], gx.data_ptr(), 0, T, 2, 1, st) == 0
    torch.cuda.synchronize()
    assert bool((h2 == SENT).all()) and bool((gx == SENT).all())


def test_unsupported_width_still_runs_through_torch_with_the_warning(device):
    m = make((3, 2), 526, device).eval()
    x = torch.randn(2, 4, 526, device=device)
    models._WARNED.clear()                                     # the warning is a warn-once
    with pytest.warns(RuntimeWarning, match=r"\[1,1\] / \[2,1\]"):
        y = m(x)
    m.fused = False
    assert torch.equal(y, m(x))


def _no_dropout(net):
    for mod in net.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return net


def make_args(**kw):
    a = argparse.Namespace(dataset="PhysioNet", model="Potes0.1", method="durmixmagwarp(0.2,4)+0.7",
                           num_epochs=2, batch_size=32, op="adam", use_sched=True, lr_max=0.01,
                           weight_decay=1e-4, grad_clip=0.1, seed=4, num_classes=2, num_channels=4,
                           sig_len=2500, depth=0, num_steps=12, sample_rate=1000)
    a.__dict__.update(kw)
    return a


def test_training_step_equivalence(device):
    """One Adam step of 'Potes0.1' with the HIP stack == one with the torch stack (dropout off).
    This is the pattern of ``test_training_step_equivalence``, which lives in
    tests/test_potes_gpu.py (not in tests/test_train_gpu.py): one step on random data with that
    test's tolerances, here at B = 32, T = 2500.  The method string and the six steps belong to the
    other pattern, ``test_graphed_step_matches_eager`` below."""
    outs = []
    for fused in (True, False):
        torch.manual_seed(2)
        m = _no_dropout(tm.build_model(make_args()).to(device)).train()
        m.fused = fused
        opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-2)
        torch.manual_seed(5)
        x = torch.randn(32, 4, 2500, device=device)
        t = torch.nn.functional.one_hot(torch.randint(0, 2, (32,), device=device), 2).float()
        assert m._fused(x) == fused
        loss = -(torch.log_softmax(m(x), 1) * t).sum(1).mean()
        loss.backward()
        opt.step()
        outs.append((float(loss), [p.detach().clone() for p in m.cnn1.parameters()] +
                     [m.dimreduc.weight.detach().clone()]))
    print("losses", outs[0][0], outs[1][0])
    assert abs(outs[0][0] - outs[1][0]) < 1e-5
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.allclose(a, b, rtol=1e-3, atol=2e-4)   # Adam normalises: sign/ratio sensitive


def _run_steps(graphed, device, dropout_off, n_steps=6):
    B, C, T = 32, 4, 2500
    pool = synthetic.make_batch(B, C, T, seed=9)
    batch = (torch.from_numpy(pool[0]), torch.from_numpy(pool[2]), torch.from_numpy(pool[1]), pool[3],
             torch.ones(B, dtype=torch.long), torch.arange(B))
    args = make_args()
    torch.manual_seed(0)
    net = tm.build_model(args).to(device)
    if dropout_off:
        _no_dropout(net)
    net.train()
    assert net._fused_head(torch.zeros(B, C, T, device=device))
    before = [p.detach().clone() for p in net.parameters() if p.requires_grad]
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(pool[2], 2, es=args.num_epochs + 1, device=device)
    sc = tm.step_counter_class()
    if graphed:
        g = tm.GraphedTrainStep(args, net, opt, sched, crit, device, B, C, T)
        losses = [float(g.step(batch, 0, sc)) for _ in range(n_steps)]
    else:
        losses = [float(tm.train_step(args, net, batch, device, opt, sched, crit, 0, sc))
                  for _ in range(n_steps)]
    assert sc.count == n_steps
    return losses, before, [p.detach().clone() for p in net.parameters() if p.requires_grad]


def test_graphed_step_matches_eager(device):
    """tests/test_train_gpu.py::test_graphed_step_matches_eager for 'Potes0.1': the captured step
    builds and replays with the narrow kernels (the weight gradient reduces in its own launch, the
    optimiser's fold finds nothing deferred) and follows the eager train_step."""
    eager = _run_steps(False, device, True)
    graph = _run_steps(True, device, True)
    print("eager", eager[0], "graphed", graph[0])
    assert np.allclose(eager[0], graph[0], rtol=1e-4, atol=1e-5), (eager[0], graph[0])
    for a, b in zip(eager[2], graph[2]):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-4)


def test_graphed_step_with_dropout_trains(device):
    losses, before, after = _run_steps(True, device, False)
    assert np.isfinite(losses).all() and len(set(losses)) == len(losses)
    assert all(bool(torch.isfinite(a).all()) for a in after)
    assert any(not torch.equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("name", ["Potes0.02", "Potes0.1"])
def test_hip_path_matches_reference_logits(name, device):
    """Same seed -> same weights -> the HIP path gives the logits the reference's own module gave
    (tolerance of tests/test_train_gpu.py::test_models_match_reference_logits_on_hip_path)."""
    g = np.load(os.path.join(GOLDEN, "model_sizes.npz"))
    i = [str(n) for n in g["names"]].index(name)
    x = torch.from_numpy(np.random.RandomState(3).randn(3, 4, 2500).astype(np.float32)).to(device)
    torch.manual_seed(11)
    m = tm.build_model(make_args(model=name)).to(device).eval()
    assert m._fused_head(x)
    out = m(x, depth=0, pass_part="second").detach().cpu().numpy()
    err = float(np.abs(out - g["logits"][i]).max())
    print(name, "max |diff| to the reference's logits", err)
    assert err <= 1e-4, (name, err)


@pytest.mark.parametrize("name", ["PotesBig64and32", "resnet9-5k"])
def test_fallback_routes_train(name, device):
    """The wide models have no hand-written stack: they train through torch/MIOpen."""
    B, C, T = 8, 4, 2500
    pool = synthetic.make_batch(B, C, T, seed=3)
    batch = (torch.from_numpy(pool[0]), torch.from_numpy(pool[2]), torch.from_numpy(pool[1]), pool[3],
             torch.ones(B, dtype=torch.long), torch.arange(B))
    args = make_args(model=name, method="durmixmagwarp(0.2,4)", batch_size=B, num_steps=4)
    torch.manual_seed(0)
    net = tm.build_model(args).to(device).train()
    opt, sched = tm.make_optimizer(args, net)
    crit = tm.SELCLoss(pool[2], 2, es=args.num_epochs + 1, device=device)
    sc = tm.step_counter_class()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)         # the fall-back announces itself
        losses = [float(tm.train_step(args, net, batch, device, opt, sched, crit, 0, sc)) for _ in range(2)]
    assert np.isfinite(losses).all(), losses
