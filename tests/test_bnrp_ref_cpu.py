"""tests/bnrp_ref.py against torch float64 autograd of batch_norm -> relu -> max_pool2d (+ skip), its
first-maximum rule against torch's CPU float32 max_pool2d backward on planted ties, the exactness the
two integer generators promise, the fixed point of margin_case, and what the shape table covers in
terms of the constants of csrc/pcgmix_bnrp.hip.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bnrp_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(os.path.dirname(HERE), "pcgmix-a-data-augmentation-method-for-heart-sound-classification-extended_amd",
                      "csrc", "pcgmix_bnrp.hip")
SMALL = [t for t in R.BNRP_EDGE if t[0] * t[1] * t[2] * t[3] <= 1 << 16]
SMALL_IDS = [R.EDGE_IDS[R.BNRP_EDGE.index(t)] for t in SMALL]


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def _close(name, got, want, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert got.shape == want.shape and err <= rel * max(scale, 1e-300), (name, err, scale)


def _pool(t, ph, pw):
    return t if (ph, pw) == (1, 1) else F.max_pool2d(t, (ph, pw))


# ---- the rule against torch ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL, ids=SMALL_IDS)
def test_ref_matches_torch_float64_autograd(shape, monkeypatch):
    """Training and eval mode on margin_case data (no decision within 2e-3 of a tie), nothing rounded to
    float32 (R.ROUND = False): z, the statistics, dx, dgamma, dbeta to 1e-12."""
    monkeypatch.setattr(R, "ROUND", False)
    B, C, H, W, ph, pw = shape[:6]
    c = R.margin_case(*shape, mode="train")
    y = _nchw(c.y).requires_grad_(True)
    g, b = torch.from_numpy(c.gamma).requires_grad_(True), torch.from_numpy(c.beta).requires_grad_(True)
    rm, rv = torch.from_numpy(c.running_mean.copy()), torch.from_numpy(c.running_var.copy())
    pre = y + torch.from_numpy(c.mean_shift).view(1, -1, 1, 1)           # the bias left out of y
    want = _pool(F.relu(F.batch_norm(pre, rm, rv, g, b, True, c.momentum, c.eps)), ph, pw) + _nchw(c.skip)
    want.backward(_nchw(c.dz))
    mom = float(np.float32(c.momentum))
    rm = (1 - mom) * torch.from_numpy(c.running_mean) + mom * pre.detach().mean((0, 2, 3))   # momentum as float32
    rv = (1 - mom) * torch.from_numpy(c.running_var) + mom * pre.detach().var((0, 2, 3), unbiased=True)
    f = R.train_fwd(c.y, c.gamma, c.beta, c.running_mean, c.running_var, c.momentum, c.eps, c.mean_shift,
                    c.batches_tracked, c.skip, ph, pw)
    bw = R.train_bwd(c.y, c.dz, c.gamma, c.beta, f.mean, f.invstd, ph, pw)
    _close("z", f.z, _nhwc(want))
    _close("running_mean", f.running_mean, rm.numpy())
    _close("running_var", f.running_var, rv.numpy())
    _close("mean", f.mean, c.y.mean((0, 1, 2)))
    _close("invstd", f.invstd, 1 / np.sqrt(c.y.var((0, 1, 2)) + c.eps))
    assert f.batches_tracked == c.batches_tracked + 1
    _close("dx", bw.dx, _nhwc(y.grad))
    _close("dgamma", bw.dgamma, g.grad.numpy())
    _close("dbeta", bw.dbeta, b.grad.numpy())
    assert not bw.dzero.any() and not np.signbit(bw.dzero).any()
    # optional inputs left out
    f0 = R.train_fwd(c.y, c.gamma, c.beta, None, None, c.momentum, c.eps, None, None, None, ph, pw)
    assert f0.running_mean is None and f0.running_var is None and f0.batches_tracked is None
    _close("z without skip", f0.z, _nhwc(want) - c.skip)
    # eval
    c = R.margin_case(*shape, mode="eval")
    y = _nchw(c.y).requires_grad_(True)
    pre = y + torch.from_numpy(c.conv_bias).view(1, -1, 1, 1)
    want = _pool(F.relu(F.batch_norm(pre, torch.from_numpy(c.running_mean), torch.from_numpy(c.running_var),
                                     torch.from_numpy(c.gamma), torch.from_numpy(c.beta), False, 0.0,
                                     float(np.float32(c.eps)))), ph, pw) + _nchw(c.skip)
    want.backward(_nchw(c.dz))
    args = (c.gamma, c.beta, c.running_mean, c.running_var, c.eps, c.conv_bias)
    _close("eval z", R.eval_fwd(c.y, *args, c.skip, ph, pw), _nhwc(want))
    _close("eval dx", R.eval_bwd(c.y, c.dz, *args, ph, pw), _nhwc(y.grad))


def _torch_dy(a, dz, ph, pw):
    """torch CPU float32: the gradient max_pool2d and relu route back to the pre-activation a."""
    t = _nchw(a.astype(np.float32)).requires_grad_(True)
    _pool(F.relu(t), ph, pw).backward(_nchw(dz.astype(np.float32)))
    return _nhwc(t.grad).astype(np.float64)


@pytest.mark.parametrize("shape", SMALL, ids=SMALL_IDS)
def test_first_maximum_rule_is_torchs_on_planted_ties(shape):
    ph, pw = shape[4:6]
    c = R.eval_int_case(*shape)
    scale, shift = R.eval_affine(c.gamma, c.beta, c.running_mean, c.running_var, c.eps, c.conv_bias)
    a = c.y * scale + shift
    _, arg, best = R.pool_fwd(c.y, scale, shift, ph, pw)
    dy, hit = R.pool_bwd(c.dz, arg, best, c.y.shape, ph, pw)
    assert np.array_equal(dy, _torch_dy(a, c.dz, ph, pw))
    dx = R.eval_bwd(c.y, c.dz, c.gamma, c.beta, c.running_mean, c.running_var, c.eps, c.conv_bias, ph, pw)
    assert np.array_equal(dx, scale * dy) and not np.signbit(dx[~hit]).any()
    c = R.train_int_case(*shape)
    f = R.train_fwd(c.y, c.gamma, c.beta, None, None, c.momentum, c.eps, None, None, None, ph, pw)
    dy, _ = R.pool_bwd(c.dz, f.arg, f.best, c.y.shape, ph, pw)
    assert np.array_equal(dy, _torch_dy(c.y * f.scale + f.shift, c.dz, ph, pw))


# ---- the integer generators ------------------------------------------------------------------------
def _seq32(t):
    """Per-channel float32 sum in index order (the cumulative sum's last row)."""
    return np.cumsum(t.reshape(-1, t.shape[-1]).astype(np.float32), 0, dtype=np.float32)[-1].astype(np.float64)


@pytest.mark.parametrize("shape", R.BNRP_EDGE, ids=R.EDGE_IDS)
def test_eval_int_case_is_exact_and_has_its_ties(shape):
    B, C, H, W, ph, pw = shape[:6]
    c = R.eval_int_case(*shape)
    assert c.eps == 0.0 and set(np.unique(c.running_var)) <= {1.0, 4.0, 16.0, 0.25}
    assert (c.gamma > 0).any() and (c.gamma < 0).any()
    for t in (c.y, c.dz, c.skip, c.gamma, c.beta, c.running_mean, c.conv_bias):
        assert np.array_equal(t, t.astype(np.float32))
    for t in (c.dz, c.skip, c.gamma, c.beta, c.running_mean, c.conv_bias):
        assert np.array_equal(t, np.round(t))
    # the float32 restatement (separate multiply and add: two roundings) gives the float64 values
    scale, shift = R.eval_affine(c.gamma, c.beta, c.running_mean, c.running_var, c.eps, c.conv_bias)
    f = np.float32
    mu32 = c.running_mean.astype(f) - c.conv_bias.astype(f)
    is32 = f(1) / np.sqrt(c.running_var.astype(f))
    scale32 = c.gamma.astype(f) * is32
    shift32 = c.beta.astype(f) - mu32 * scale32
    assert np.array_equal(scale32, scale) and np.array_equal(shift32, shift)
    assert np.array_equal(scale, c.gamma / np.sqrt(c.running_var))              # nothing was rounded at all
    a32 = c.y.astype(f) * scale32 + shift32
    assert a32.dtype == f and np.array_equal(a32, c.y * scale + shift)
    z, arg, best = R.pool_fwd(c.y, scale, shift, ph, pw, c.skip)
    assert np.array_equal(z.astype(f), z)
    dx = R.eval_bwd(c.y, c.dz, c.gamma, c.beta, c.running_mean, c.running_var, c.eps, c.conv_bias, ph, pw)
    assert np.array_equal(dx.astype(f), dx)
    # informative: many levels; the planted windows are what they claim
    levels = min(8, z.size // 2)                          # the smallest entries have 8 outputs in all
    assert len(np.unique(z)) >= levels and len(np.unique(dx)) >= min(levels, 4)
    r = np.maximum(R._windows(c.y * scale + shift, ph, pw), 0.0)
    N = ph * pw
    if c.kind.size >= 5:
        k0, k1, k2 = (r[c.kind == k] for k in (0, 1, 2))
        assert (k0 == k0[..., :1]).all() and (k0 > 0).any()
        assert (k1[..., -1] > 0).all() and (N == 1 or (k1[..., :-1] == 0).all())
        assert (k2 == 0).all()
        a3 = R._windows(c.y * scale + shift, ph, pw)[c.kind == 3]
        assert (a3 <= 0).all() and (a3 == 0).any()
    if N > 1:
        assert (arg == N - 1).any() and (arg == 0).any()


@pytest.mark.parametrize("shape", R.BNRP_EDGE, ids=R.EDGE_IDS)
def test_train_int_case_is_exact(shape):
    B, C, H, W, ph, pw = shape[:6]
    c = R.train_int_case(*shape)                        # asserts the 2^24 bound itself
    n = B * H * W
    f = np.float32
    assert c.eps == 0.0 and c.momentum in (0.5, 0.25)
    assert ((c.y - c.m) > 0).reshape(-1, C).sum(0).tolist() == [n // 2] * C
    assert np.array_equal(np.abs(c.y - c.m).reshape(-1, C).max(0), 2.0 ** c.k)
    fw = R.train_fwd(c.y, c.gamma, c.beta, c.running_mean, c.running_var, c.momentum, c.eps, c.mean_shift,
                     c.batches_tracked, c.skip, ph, pw)
    assert np.array_equal(fw.mean, c.m) and np.array_equal(fw.invstd, 2.0 ** -c.k)
    # float32 sums in index order, plain and about the pivot K_c = y[0, c], give the same statistics
    K = c.y[0, 0, 0]
    for piv in (np.zeros(C), K):
        s, ss = _seq32(c.y - piv), _seq32((c.y - piv) ** 2)
        m = piv + s / n
        assert np.array_equal(m, c.m) and np.array_equal(ss / n - (s / n) ** 2, 4.0 ** c.k)
    # the running statistics in float32 arithmetic
    mom = f(c.momentum)
    rm32 = (f(1) - mom) * c.running_mean.astype(f) + mom * (c.m.astype(f) + c.mean_shift.astype(f))
    unb32 = (4.0 ** c.k * n / (n - 1.0)).astype(f)
    rv32 = (f(1) - mom) * c.running_var.astype(f) + mom * unb32
    assert rm32.dtype == f and np.array_equal(rm32, fw.running_mean) and np.array_equal(rv32, fw.running_var.astype(f))
    assert np.array_equal(fw.z.astype(f), fw.z) and np.array_equal(fw.scale, c.gamma * 2.0 ** -c.k)
    a32 = c.y.astype(f) * fw.scale.astype(f) + fw.shift.astype(f)
    assert np.array_equal(a32, c.y * fw.scale + fw.shift)
    bw = R.train_bwd(c.y, c.dz, c.gamma, c.beta, fw.mean, fw.invstd, ph, pw)
    dy, _ = R.pool_bwd(c.dz, fw.arg, fw.best, c.y.shape, ph, pw)
    xhat = (c.y - c.m) * 2.0 ** -c.k
    assert set(np.unique(xhat)) == {-1.0, 1.0}
    assert np.array_equal(_seq32(dy), bw.dbeta) and np.array_equal(_seq32(dy * xhat), bw.dgamma)
    assert np.array_equal(bw.coef, np.concatenate([bw.dbeta / n, bw.dgamma / n]).astype(f))
    if c.pow2:                                          # dx in float32 arithmetic, unfused, is the float64 value
        c1, c2 = bw.coef[:C].astype(f), bw.coef[C:].astype(f)
        dx32 = fw.scale.astype(f) * (dy.astype(f) - c1 - xhat.astype(f) * c2)
        assert dx32.dtype == f and np.array_equal(dx32, bw.dx)
    # informative: gradient flows, both ReLU outcomes, ties in windows, exact zeros of the pre-activation
    assert bw.dbeta.any() and bw.dgamma.any() and (fw.best == 0).any() and (fw.best > 0).any()
    if C >= 4:
        assert ((c.beta + c.gamma == 0) | (c.beta - c.gamma == 0)).any()


def test_train_int_dx_bound_covers_unfused_float32():
    """The bound of train_int_case's docstring on a non-power-of-two n: the float32 evaluation in the
    kernel's order stays inside 2^-21 |scale| (|dy| + |c1| + |xhat c2|), and so does any fused variant
    (which rounds less)."""
    shape = (2, 12, 7, 5, 3, 2)
    c = R.train_int_case(*shape)
    f = np.float32
    fw = R.train_fwd(c.y, c.gamma, c.beta, None, None, c.momentum, c.eps, None, None, None, 3, 2)
    bw = R.train_bwd(c.y, c.dz, c.gamma, c.beta, fw.mean, fw.invstd, 3, 2)
    assert not c.pow2
    dy, _ = R.pool_bwd(c.dz, fw.arg, fw.best, c.y.shape, 3, 2)
    xhat = ((c.y - c.m) * 2.0 ** -c.k).astype(f)
    c1, c2 = bw.coef[:12].astype(f), bw.coef[12:].astype(f)
    dx32 = fw.scale.astype(f) * (dy.astype(f) - c1 - xhat * c2)
    assert (np.abs(dx32.astype(np.float64) - bw.dx) <= 2.0 ** -21 * bw.dx_terms).all()
    assert (dx32 != bw.dx).any()                         # and the bound is needed: rounding does occur


# ---- margin_case ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.BNRP_EDGE, ids=R.EDGE_IDS)
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_margin_case_reaches_a_fixed_point(shape, mode):
    B, C, H, W, ph, pw = shape[:6]
    c = R.margin_case(*shape, mode=mode)
    assert np.array_equal(c.y, c.y.astype(np.float32))
    if mode == "train":
        f = R.train_fwd(c.y, c.gamma, c.beta, None, None, c.momentum, c.eps, None, None, None, ph, pw)
        scale, shift = f.scale, f.shift
    else:
        scale, shift = R.eval_affine(c.gamma, c.beta, c.running_mean, c.running_var, c.eps, c.conv_bias)
    a = c.y * scale + shift
    assert np.abs(a).min() >= R.MARGIN
    if ph * pw > 1:
        r = np.sort(np.maximum(R._windows(a, ph, pw), 0.0), -1)
        gap = r[..., -1] - r[..., -2]
        assert gap[r[..., -1] > 0].min() >= R.MARGIN
    print(f"{c.rounds} rounds")
    assert (c.gamma < 0).any() or C < 64


# ---- the shape table ------------------------------------------------------------------------------
def _constant(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def test_shapes_cover_the_block_edges():
    """What BNRP_EDGE covers, in terms of the constants read from csrc/pcgmix_bnrp.hip: a retune of any
    of them fails here instead of silently moving the edges away from the table."""
    text = open(SOURCE).read()
    assert _constant(text, r"constexpr int kBnThreads = (\d+);") == R.BN_THREADS
    assert _constant(text, r"constexpr int kBnMaxBlocks = (\d+);") == R.BN_MAX_BLOCKS
    assert _constant(text, r"constexpr int kBnMaxC = (\d+);") == R.BN_MAX_C
    assert _constant(text, r"constexpr int kFinCh = (\d+);") == R.FIN_CH
    assert _constant(text, r"\(n4 \+ \(long long\)kBnThreads \* (\d+) - 1\) / \(\(long long\)kBnThreads \* \1\)") == R.BLOCK_VECS
    assert _constant(text, r"k \+ 7 \* 16 < nblk; k \+= (\d+) \* 16") == R.FIN_UNROLL
    assert _constant(text, r"__launch_bounds__\(kFinCh \* (\d+)\) void bn_finalize_kernel") == R.FIN_LANES
    assert re.search(r"return \(long long\)pcgmix::kBnMaxBlocks \* 2 \* C \+ 2 \* C;", text)
    T = R.BNRP_EDGE
    G = [R.geometry(*t) for t in T]
    assert len(set(t[:6] for t in T)) == len(T) and all(t[6] for t in T) and len(T) <= 32
    assert all(g.n % 2 == 0 for g in G)
    assert any(g.n & (g.n - 1) == 0 for g in G) and any(g.n & (g.n - 1) for g in G)
    Cs = {t[1] for t in T}
    assert {2, 4, 12, 64, 96, 516, 768, 1020, R.BN_MAX_C} <= Cs
    # block widths: full blocks, A < kBnThreads with R > 1, and R = 1 with and without idle lanes
    assert any(g.A == R.BN_THREADS and g.R > 1 for g in G) and any(g.A < R.BN_THREADS and g.R > 1 for g in G)
    assert {g.A for g in G if g.R == 1} >= {R.BN_THREADS // 2 + 1, R.BN_THREADS - 1, R.BN_THREADS}
    assert any(g.Q == 3 for g in G)
    # finalize: a last block with lanes c >= C (C % kFinCh != 0), and full blocks
    assert {t[1] % R.FIN_CH for t in T} >= {0, 2, 4, 12}
    wins = {t[4:6] for t in T}
    assert {(1, 1), (1, 2), (2, 2), (1, 4), (2, 1), (3, 2), (1, 3)} <= wins
    assert all(g.fixed for t, g in zip(T, G) if t[4:6] in ((1, 1), (1, 2), (2, 2)))
    assert any(t[3] % t[5] and not t[2] % t[4] for t in T) and any(t[2] % t[4] and not t[3] % t[5] for t in T)
    assert any(t[3] % t[5] and t[2] % t[4] for t in T)
    for fixed in (True, False):                         # ragged in either kind of loop
        assert any((t[3] % t[5] or t[2] % t[4]) and g.fixed == fixed for t, g in zip(T, G))
    assert any(t[3] // t[5] == 1 for t in T) and any(t[2] == t[4] and t[4] > 1 for t in T)
    # the fixed-window row loops
    F_ = [g for g in G if g.fixed]
    assert any(g.n_rows < g.R for g in F_)
    assert any(g.n_rows == g.R * g.pool_nblk for g in F_) and any(g.n_rows == g.R * g.pool_nblk + 1 for g in F_)
    assert any(g.n_strides % 2 == 1 and g.n_strides >= 3 for g in F_) and any(g.n_strides % 2 == 0 for g in F_)
    assert any(g.edge and g.pool_nblk > 1 for g in F_)
    assert any(g.n_strides > 4 for g in F_)              # more than one trip of the two-row loop
    # partial_sums: both sides of one 8 x 16 trip and of the 16 lanes, in both finalize kernels
    one = R.FIN_UNROLL * R.FIN_LANES
    want = {1, R.FIN_LANES - 1, R.FIN_LANES, R.FIN_LANES + 1, one - R.FIN_LANES, one - R.FIN_LANES + 1, one, one + 1}
    assert want == {1, 15, 16, 17, 112, 113, 128, 129}
    assert want <= {g.stats_nblk for g in G} and want <= {g.pool_nblk for g in G}
    # the grid cap: more blocks wanted than kBnMaxBlocks, by more than one (a cap one too high stays
    # inside the workspace's last 2 C floats), with C = kBnMaxC
    caps = [(t, g) for t, g in zip(T, G) if g.stats_uncapped > R.BN_MAX_BLOCKS]
    assert any(g.stats_uncapped >= R.BN_MAX_BLOCKS + 2 and t[1] == R.BN_MAX_C for t, g in caps)
    assert (4, 1024, 1, 2051, 1, 2) in [t[:6] for t in T]
    g = R.geometry(4, 1024, 1, 2051, 1, 2)
    assert g.n_rows == 4100 and g.pool_uncapped == R.BN_MAX_BLOCKS + 1 and g.pool_nblk == R.BN_MAX_BLOCKS
    assert any(g.pool_uncapped > R.BN_MAX_BLOCKS and g.n_strides > 8 for g in G)
    # the four-deep loop of bn_stats_kernel with a capped grid: at least four grid steps
    assert any(g.stats_uncapped > R.BN_MAX_BLOCKS and g.n * g.Q >= 4 * R.BN_MAX_BLOCKS * g.A for g in G)
    # and with an uncapped one: never more than BLOCK_VECS steps, four-deep at least once
    assert any(g.stats_uncapped <= R.BN_MAX_BLOCKS and g.n * g.Q >= 4 * g.stats_nblk * g.A for g in G)
    assert max(t[0] * t[1] * t[2] * t[3] for t in T) <= 8.5e6
    assert sum(t[0] * t[1] * t[2] * t[3] > R.BIG for t in T) == 2
