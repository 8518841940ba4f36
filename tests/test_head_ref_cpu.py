"""tests/head_ref.py against torch float64 autograd of the composed modules, its bit rule against its
own per-element statement, the exactness claim of its integer inputs, the conditions that keep that
data informative, and what its shape table covers.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_ref as R

F64 = torch.float64


def _close(name, got, want, rel=1e-12):
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    assert got.shape == want.shape and err <= rel * max(scale, 1e-300), (name, err, scale)


# ---- the bit rule -----------------------------------------------------------------------------
def test_bit_rule_by_hand():
    """One byte, least significant bits first: 0b10110100 is the 2-bit values 0, 1, 3, 2, the 4-bit
    values 4, 11 and the bits 0, 0, 1, 0, 1, 1, 0, 1."""
    m = torch.tensor([0b10110100], dtype=torch.uint8)
    for fn in (R.keep_loop, R.keep_vec):
        assert fn(m, 4, 2, 2).tolist() == [False, False, True, True]
        assert fn(m, 4, 2, 1).tolist() == [False, True, True, True]
        assert fn(m, 2, 4, 5).tolist() == [False, True]
        assert fn(m, 8, 1, 1).tolist() == [False, False, True, False, True, True, False, True]
        assert fn(m, 1, 8, 180).tolist() == [True] and fn(m, 1, 8, 181).tolist() == [False]
        assert fn(m, 8, 1, 0).tolist() == [True] * 8


@pytest.mark.parametrize("bits", [1, 2, 4, 8])
def test_bit_rule_loop_equals_vectorised(bits):
    """The per-element loop is the specification; the vectorised form the references use must equal it,
    for every threshold of the table and for rows that start inside a byte (B odd, K % 8 == 4)."""
    g = torch.Generator().manual_seed(bits)
    for B, K in ((5, 12), (3, 68), (2, 64)):
        n = B * K
        mask = torch.randint(0, 256, (R.mask_bytes(n, bits),), generator=g).to(torch.uint8)
        for thr in sorted({0, 1, (1 << bits) // 2, (1 << bits) - 1}):
            want = R.keep_loop(mask, n, bits, thr)
            assert torch.equal(R.keep_vec(mask, n, bits, thr), want), (B, K, thr)
            if thr == 0:
                assert bool(want.all())
    assert R.mask_bytes(12, 1) == 2 and R.mask_bytes(12, 2) == 3 and R.mask_bytes(12, 4) == 6 and R.mask_bytes(12, 8) == 12


def test_one_bit_rows_start_inside_a_byte():
    """What the 1-bit mask of an odd row with K % 8 == 4 looks like: row 1 of K = 4 owns the HIGH nibble
    of byte 0 (a decode that shifts by (k*bits) & 7 instead of ((row*K + k)*bits) & 7 reads the low one)."""
    mask = torch.tensor([0xF0, 0x0F], dtype=torch.uint8)
    keep = R.keep_loop(mask, 16, 1, 1).view(4, 4)
    assert keep.tolist() == [[False] * 4, [True] * 4, [True] * 4, [False] * 4]
    x = torch.ones(4, 4)
    xm, k2 = R.dropped(x, mask, 2.0, 1, 1)
    assert torch.equal(k2, keep) and xm.tolist() == [[0.0] * 4, [2.0] * 4, [2.0] * 4, [0.0] * 4]


# ---- the reference against torch autograd -----------------------------------------------------
def _rand_like(c, seed=0):
    """randn data in the shapes and with the masks of table case c, float64."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)   # noqa: E731
    d = dict(x=rn(c.B, c.K).relu(), w1=rn(R.HEAD_O, c.K) / c.K ** 0.5, b1=rn(R.HEAD_O), w2=rn(c.C, R.HEAD_O) / 4,
             b2=rn(c.C), dl=rn(c.B, c.C), seed=rn(c.B, c.C))
    return {k: v.requires_grad_(k in ("x", "w1", "b1", "w2", "b2")) for k, v in d.items()}


def _torch_head(c, d, mix=None, lam=1.0, masks=True):
    """Linear -> ReLU -> Linear with the masks as tensors: (z, h, logits), autograd on."""
    x = d["x"]
    if masks and c.mask1 is not None:
        x = x * (R.keep_vec(c.mask1, c.B * c.K, c.bits1, c.thr1).view(c.B, c.K).to(F64) * c.scale1)
    z = F.linear(x, d["w1"], d["b1"])
    z.retain_grad()
    h = torch.relu(z)
    if masks and c.mask2 is not None:
        h = h * ((c.mask2.view(c.B, R.HEAD_O).long() >= c.thr2).to(F64) * c.scale2)
    if mix is not None:
        l32 = np.float32(lam)
        h = float(l32) * h + float(np.float32(1) - l32) * h[mix.long()]
    return z, h, F.linear(h, d["w2"], d["b2"])


REF_SHAPES = [(5, 2492, 2, 1, 1), (9, 60, 2, 4, 8), (33, 64, 8, 8, 1), (3, 6144, 2, 2, 1), (49, 128, 2, 0, 0),
              (31, 60, 1, 2, 3)]


def _grads(loss, d, z):
    g = torch.autograd.grad(loss, [d["x"], d["w1"], d["b1"], d["w2"], d["b2"], z], allow_unused=True)
    return dict(zip(("dx", "dw1", "db1", "dw2", "db2", "dz"), g))


def _args(c, d):
    return (d["x"], c.mask1, c.scale1, c.thr1, c.bits1, d["w1"], d["b1"], c.mask2, c.scale2, c.thr2, d["w2"], d["b2"])


@pytest.mark.parametrize("shape", REF_SHAPES, ids=str)
def test_head_ref_matches_torch_autograd(shape):
    """Forward, the explicit backward, the saliency form, the fused loss with both target kinds and the
    latent blend: 1e-12 relative against float64 autograd of Linear -> ReLU -> Linear -> log_softmax."""
    c = R.int_case(*shape)                               # only its shape, masks, labels and permutations
    d = _rand_like(c)
    a = _args(c, d)
    z, h, logits = _torch_head(c, d)
    f = R.head_fwd(*a)
    _close("z", f.z, z.detach())
    _close("logits", f.logits, logits.detach())
    _close("partial", f.partial.sum(0) + d["b1"].detach(), z.detach())
    assert f.partial.shape == (c.KS, c.B, R.HEAD_O)
    want = _grads((logits * d["dl"]).sum(), d, z)
    b = R.head_bwd(d["dl"], f.z, c.mask2, c.scale2, c.thr2, d["w2"], d["x"], c.mask1, c.scale1, c.thr1, c.bits1,
                   d["w1"])
    for k, v in want.items():
        _close(k, getattr(b, k), v)
    # NULL biases
    f0 = R.head_fwd(*a[:6], None, *a[7:11], None)
    z0, _, logits0 = _torch_head(c, {**d, "b1": None, "b2": None})
    _close("z, no biases", f0.z, z0.detach())
    _close("logits, no biases", f0.logits, logits0.detach())
    # saliency: eval mode, no masks
    z, h, logits = _torch_head(c, d, masks=False)
    want = _grads((logits * d["seed"]).sum(), d, z)
    s = R.saliency(d["x"], d["w1"], d["b1"], d["w2"], d["seed"])
    _close("saliency dz", s.dz, want["dz"])
    _close("saliency dx", s.dx, want["dx"])
    # fused loss: soft targets that do not sum to 1, uint8 labels, latent blends
    for kind, tgt in ((0, c.target), (1, c.labels)):
        t = R.targets(tgt, kind, c.C)
        for name, mix in [("plain", None)] + list(c.perms.items()):
            for lam in ((1.0,) if mix is None else (0.0, 0.3, 1.0)):
                z, h, logits = _torch_head(c, d, mix, lam)
                loss = -(F.log_softmax(logits, dim=1) * t).sum(1).mean()
                want = _grads(loss, d, z)
                inv = None if mix is None else R.inverse(mix)
                if mix is not None:
                    assert torch.equal(inv[mix.long()], torch.arange(c.B, dtype=torch.int32))
                o = R.head_loss(*a, tgt, kind, mix, inv, lam)
                _close("loss", o.loss, loss.detach())
                _close("logits", o.logits, logits.detach())
                _close("dz", o.dz, want["dz"])
                _close("small", o.small, R.small_of(want["dw2"], want["db2"], want["db1"]))
                for gs in (None, 0.37):
                    fb = R.head_loss_bwd(o.dz, gs, d["x"], c.mask1, c.scale1, c.thr1, c.bits1, d["w1"], o.small)
                    k = 1.0 if gs is None else gs
                    _close("dw1", fb.dw1, want["dw1"] * k)
                    _close("dx", fb.dx, want["dx"] * k)
                    _close("small_out", fb.small, o.small * k)
        _close("soft_ce", R.soft_ce(f.logits, t), -(F.log_softmax(f.logits, dim=1) * t).sum(1).mean())
        lg = f.logits.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(-(F.log_softmax(lg, dim=1) * t).sum(1).mean() * 0.7, lg)
        _close("soft_ce_bwd", R.soft_ce_bwd(f.logits, t, 0.7), g)


@pytest.mark.parametrize("shape", REF_SHAPES[:4], ids=str)
def test_selc_ref_matches_the_selcloss_formula(shape):
    """A float64 copy of SELCLoss past its turning point as tests/test_selc_cpu.py states it — pred =
    softmax(logits); soft[index] = m soft[index] + (1-m) pred; loss = mean(-sum log(pred) soft[index]) —
    and its autograd gradient, for in-range indices; a row whose index is outside [0,N) updates nothing,
    has a zero row and gives no loss and no gradient."""
    c = R.int_case(*shape)
    d = _rand_like(c, 1)
    a = _args(c, d)
    keep, take = 0.9, 1.0 - 0.9
    index = c.index.clone()
    index[c.B // 2] = (set(range(c.N)) - set(index.tolist())).pop()          # all inside
    z, h, logits = _torch_head(c, d)
    soft = c.soft.double().clone()
    pred = torch.softmax(logits, dim=1)
    soft[index] = keep * soft[index] + take * pred.detach()
    loss = -(torch.log(pred) * soft[index]).sum(1).mean()
    want = _grads(loss, d, z)
    o = R.head_loss(*a, None, 0, selc_args=(index, c.soft, keep, take))
    _close("loss", o.loss, loss.detach())
    _close("soft", o.soft, soft)
    _close("rows", o.rows, soft[index])
    _close("dz", o.dz, want["dz"])
    _close("small", o.small, R.small_of(want["dw2"], want["db2"], want["db1"]))
    l2, rows, s2 = R.selc(logits.detach(), index, c.soft, keep, take)
    _close("selc loss", l2, loss.detach())
    lg = logits.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(-(F.log_softmax(lg, dim=1) * rows).sum(1).mean() * 0.5, lg)
    _close("selc bwd", R.soft_ce_bwd(logits.detach(), rows, 0.5), g)
    # the case's own index has one row outside [0,N)
    out = c.B // 2
    assert not 0 <= int(c.index[out]) < c.N
    l3, rows3, s3 = R.selc(logits.detach(), c.index, c.soft, keep, take)
    assert not bool(rows3[out].any())
    inside = [b for b in range(c.B) if b != out]
    untouched = sorted(set(range(c.N)) - {int(c.index[b]) for b in inside})
    assert torch.equal(s3[untouched], c.soft.double()[untouched])
    if inside:
        _close("rows of the others", rows3[inside], rows[inside])
        _close("loss without the row", l3, -(F.log_softmax(logits.detach(), dim=1)[inside] * rows[inside]).sum() / c.B)
    assert not bool(R.soft_ce_bwd(logits.detach(), rows3)[out].any())


# ---- the exactness claim ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 8196, 2, 1, 1), (257, 516, 2, 1, 1), (129, 2492, 2, 1, 1), (33, 64, 8, 8, 1),
                                   (5, 14848, 2, 2, 1), (127, 60, 2, 0, 0)], ids=str)
def test_integer_case_is_exact_in_float32(shape):
    """The claim the GPU suite rests on: for int_case data torch FLOAT32 on the CPU — its own summation
    order, its own autograd — equals the float64 restatement bit for bit: z, logits, dz, dW2, db2, db1,
    dW1, dx.  All of them are integers."""
    c = R.int_case(*shape)
    d = {k: getattr(c, k).clone().float().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2")}
    x = d["x"]
    if c.mask1 is not None:
        x = x * (R.keep_vec(c.mask1, c.B * c.K, c.bits1, c.thr1).view(c.B, c.K).float() * c.scale1)
    z = F.linear(x, d["w1"], d["b1"])
    z.retain_grad()
    h = torch.relu(z)
    if c.mask2 is not None:
        h = h * ((c.mask2.view(c.B, R.HEAD_O).long() >= c.thr2).float() * c.scale2)
    logits = F.linear(h, d["w2"], d["b2"])
    assert z.dtype == logits.dtype == torch.float32
    got = _grads((logits * c.dlogits).sum(), d, z)
    got.update(z=z.detach(), logits=logits.detach())
    want = dict(z=c.ref.z, logits=c.ref.logits, dz=c.bwd.dz, dw2=c.bwd.dw2, db2=c.bwd.db2, db1=c.bwd.db1,
                dw1=c.bwd.dw1, dx=c.bwd.dx)
    for k, w in want.items():
        assert got[k].dtype == torch.float32 and torch.equal(got[k].double(), w), k
        assert torch.equal(w, w.round()), k
    planes = torch.stack([F.linear(x[:, s:s + R.SK_CHUNK], d["w1"][:, s:s + R.SK_CHUNK])
                          for s in range(0, c.K, R.SK_CHUNK)]).detach()
    assert torch.equal(planes.double(), c.ref.partial)
    assert R.int_case(*shape) is c                       # one shared reference per shape
    # the dyadic form: same z, logits scaled by a power of two, still exact in float32
    y = R.dyadic_case(*shape)
    lg = F.linear(h.detach(), y.w2.float(), y.b2.float())
    assert torch.equal(lg.double(), y.ref.logits) and float(y.ref.logits.abs().max()) <= 8.0
    assert torch.equal(y.ref.z, c.ref.z) and R.dyadic_case(*shape) is y


# ---- informative data -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.HEAD_EDGE, ids=R.EDGE_IDS)
def test_integer_case_is_informative(shape):
    """Conditions, so that a GPU run cannot pass on degenerate data: in every int_case at least 5 % of z
    are <= 0 and at least 1 % exactly 0, every mask keeps between 5 % and 95 % of its elements unless
    thr = 0 keeps all by construction, dW1, dx and the saliency dx are not identically zero, every
    order-independent bound is below 2**24 and all data are integers."""
    B, K, C, bits, thr = shape
    c = R.int_case(*shape)
    assert (c.B, c.K, c.C, c.KS, c.nrb) == (B, K, C, R.splits(K), R.nrb(B))
    assert c.z_nonpos >= 0.05 and c.z_zero >= 0.01, (c.z_nonpos, c.z_zero)
    assert float((c.ref.z > 0).double().mean()) >= 0.05
    if bits == 0:
        assert c.mask1 is None and c.mask2 is None
    else:
        assert c.mask1.numel() == R.mask_bytes(B * K, bits) and c.mask2.numel() == B * R.HEAD_O
        for keep, t in ((c.keep1, c.thr1), (c.keep2, c.thr2)):
            if t == 0:
                assert keep == 1.0
            else:
                assert 0.05 <= keep <= 0.95, (keep, t)
        assert c.scale1 in (2.0, 4.0) and c.scale2 in (2.0, 4.0)
    for name in ("dw1", "dx"):
        assert bool(getattr(c.bwd, name).any()), name
    assert bool(c.sal.dx.any()) and bool(c.sal.dz.any())
    assert float((c.x == 0).float().mean()) >= 0.2 and float(c.x.min()) >= 0.0
    assert set(c.bounds) >= {"partial", "z", "logits", "dz", "dW2", "db2", "db1", "dW1", "dx"}
    for name, bound in c.bounds.items():
        assert float(bound) < 2 ** 24, name
    for t in (c.x, c.w1, c.b1, c.w2, c.b2, c.dlogits, c.seed):
        assert t.dtype == torch.float32 and torch.equal(t, t.round())
    # what the loss tests use
    assert c.index.unique().numel() == B and int(((c.index < 0) | (c.index >= c.N)).sum()) == 1
    assert abs(float(c.target.sum(1).mean()) - 1.3) < 1e-5
    for name, mix in c.perms.items():
        assert sorted(mix.tolist()) == list(range(B)), name
    assert torch.equal(c.labels[c.perms["same-label shuffle"].long()], c.labels)
    fixed = c.perms["with fixed points"]
    assert B == 1 or bool((fixed == torch.arange(B)).any()) or B == 2
    if B > 4:           # partners in a later and in an earlier row block
        blk, pblk = torch.arange(B) // R.TAIL_ROWS, fixed.long() // R.TAIL_ROWS
        assert bool((pblk > blk).any()) and bool((pblk < blk).any())


# ---- the shape table --------------------------------------------------------------------------
def test_shapes_cover_tile_edges():
    """What HEAD_EDGE covers, from the kernels' constants restated in head_ref.py."""
    T = R.HEAD_EDGE
    Bs, Ks = {t[0] for t in T}, {t[1] for t in T}
    assert 35 <= len(T) <= 45 and len(set(T)) == len(T)
    # every value of every axis has at least two partners
    for b in Bs:
        assert len({t[1] for t in T if t[0] == b}) >= 2, b
    for k in Ks:
        assert len({t[0] for t in T if t[1] == k}) >= 2, k
    for m in {t[3:] for t in T}:
        assert len([t for t in T if t[3:] == m]) >= 2, m
    assert {t[3:] for t in T} == {(8, 0), (8, 1), (8, 128), (8, 255), (4, 8), (4, 15), (2, 1), (2, 3), (1, 1), (0, 0)}
    assert {t[2] for t in T} == {1, 2, 3, R.MAX_C}
    for cc in (1, 3, R.MAX_C):
        assert len([t for t in T if t[2] == cc]) >= 2
    assert all(t[0] <= 5 for t in T if t[1] >= 6144) and all(t[1] <= 516 for t in T if t[0] == 257)
    assert max(t[0] * t[1] for t in T) * 4 * 3 < 10e6                    # x, dx and a third of that: < 10 MB
    # B: both sides of every row tile
    for edge in (R.SK_ROWS, R.TAIL_BWD_GROUPS, 2 * R.HB_ROWS):
        assert {edge - 1, edge, edge + 1} <= Bs, edge
    assert {1, R.TAIL_ROWS - 1, R.TAIL_ROWS, R.TAIL_ROWS + 1} <= Bs
    # row halves of ceil(B/2) rows in 64-row chunks: 128 -> 64 + 64, 129 -> (64 + 1) + 64, 130 -> (64 + 1) twice
    assert [(b + 1) // R.HB_SPLIT % R.HB_ROWS for b in (127, 128, 129, 130)] == [0, 0, 1, 1]
    assert R.LOSS_THREADS + 1 in Bs and max(Bs) == R.LOSS_THREADS + 1
    assert {R.nrb(b) for b in Bs} >= {1, 2, 3, 5, 29, 32, 33}
    # nrb = 29: segments of 8, 8, 8, 5 — the eight-deep loop exactly once per full segment; 32: four
    # times 8; 33: per = 9, the last segment 6; 1, 2, 3: empty segments
    per = lambda n: (n + R.TL_SEG - 1) // R.TL_SEG   # noqa: E731
    assert per(29) == R.TL_UNROLL and per(32) == R.TL_UNROLL and per(33) == R.TL_UNROLL + 1
    assert [min(n, R.TL_SEG * per(n)) - (R.TL_SEG - 1) * per(n) for n in (1, 2, 3)] == [-2, -1, 0]
    # K: both sides of the 64-column tile, the 128-column wave span and the 512-element chunk (K % 4 == 0)
    for edge in (R.HB_COLS, R.SK_WAVE, R.SK_CHUNK):
        assert {edge - 4, edge, edge + 4} <= Ks, edge
    assert min(Ks) == 4 and all(k % 4 == 0 for k in Ks)
    assert {R.splits(k) for k in Ks} >= {1, 2, 5, 12, 13, 15, 16, 17, 29}
    # the split sum of potes_tail_*: (four-deep trips, single loads) of lane 0 changes at KS = 13 and 17
    assert [R.tail_sum_shape(n) for n in (12, 13, 15, 16, 17, 29)] == [(0, 3), (1, 0), (1, 0), (1, 0), (1, 1), (2, 0)]
    assert R.splits(2492) == 5 and 2492 % 8 == 4
    # 20*K neither a multiple of the 4096 floats a spare block clears nor above it, and far above it
    assert any(R.HEAD_O * k < R.ZERO_BLOCK for k in Ks) and any(R.HEAD_O * k % R.ZERO_BLOCK for k in Ks if R.HEAD_O * k > R.ZERO_BLOCK)
    # every packed width starts rows inside a byte somewhere (odd B, K % 8 == 4) and byte-aligned elsewhere
    for bits in (1, 2, 4, 8):
        assert any(t[3] == bits and t[0] % 2 == 1 and t[1] % 8 == 4 for t in T), bits
        assert any(t[3] == bits and t[1] % 8 == 0 for t in T), bits
    # the 1-bit, K % 8 == 4 cases that tell the element's bit offset from the column's
    for k in (4, 68, 132, 516, 2492, 6148, 8196):
        assert any(t[1] == k and t[3:] == (1, 1) and t[0] % 2 == 1 for t in T), k
