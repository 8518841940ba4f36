"""Float64 restatement of the Potes classifier head (csrc/pcgmix_head.hip, with the split-K product
of csrc/pcgmix_skinny.hip in front of it) for tests/test_head_ref_cpu.py and
tests/test_head_edges_gpu.py, the inputs both use and the shape table.  Not a test module.

Every function takes the arguments of the entry point it restates, NULL options (None) included,
and computes in torch float64 on the CPU, explicitly: no autograd, no nn module.

  x (B,K) -> dropout 1 -> z = xm W1^T + b1 -> fac = (z > 0) [* dropout 2] -> h = z fac
          -> logits = h W2^T + b2

Dropout 1 is the rule the kernels decode (``keep_vec``; ``keep_loop`` is its specification, one bit at
a time): element e = b*K + k owns ``bits`` consecutive bits of the byte stream at bit offset e*bits
(bit p of the stream is bit p & 7 of byte p >> 3), is kept iff their value >= thr and a kept value is
multiplied by ``scale``.  Dropout 2 is byte-wise: kept iff byte >= thr2.  A NULL mask ignores its scale.

Two kinds of input, cached per shape (the tests share one reference and must not write to it):
  int_case     small integers and power-of-two scales.  For every sum a kernel forms — the split-K
               partial planes, z, logits, dz, dW2, db2, db1, dW1, dx, the saliency pair — the sum of the
               ABSOLUTE values of its addends is computed here and asserted < 2**24: every partial sum,
               in any order and through any fmaf chain, is then an integer float32 holds exactly, so a
               float32 kernel must give the float64 result BIT FOR BIT.
  dyadic_case  the same data with w2, b2 times a power of two that brings max|logits| to <= 8: z and
               logits stay exact (the scaling only moves exponents) and the softmax / log of the loss
               kernels see identical float32 and float64 inputs.
"""
import functools
import types

import numpy as np
import torch

# ---- kernel constants, restated once (file:line of the definition) -------------------------------
HEAD_O = 20            # csrc/pcgmix_head.hip:43     kHeadO, the dimreduc width
MAX_C = 8              # csrc/pcgmix_head.hip:44     kHeadMaxC
TAIL_ROWS = 4          # csrc/pcgmix_head.hip:45     kTailRows: batch rows per block of the tail kernels
TAIL_BWD_GROUPS = 48   # csrc/pcgmix_head.hip:46     kTailBwdGroups: row groups of potes_tail_bwd_kernel
HB_COLS = 64           # csrc/pcgmix_head.hip:47     kHbCols: columns per block of potes_head_bwd_kernel
TAIL_LANES = 4         # csrc/pcgmix_head.hip:60     q = t & 3: lanes that share the split sum of one z
TAIL_DEPTH = 4         # csrc/pcgmix_head.hip:67     ks + 12 < KS: four loads in flight per lane
HB_ROWS = 64           # csrc/pcgmix_head.hip:212    kHbRows: rows per chunk
HB_SPLIT = 2           # csrc/pcgmix_head.hip:212    kHbSplit: row halves (gridDim.y)
TL_STRIDE = 192        # csrc/pcgmix_head.hip:215    kTlStride: workspace floats per row block
TL_USED = 189          # csrc/pcgmix_head.hip:215    columns 0..188 are written (dW2, db2, db1, loss)
TL_SEG = 4             # csrc/pcgmix_head.hip:217    kTlSeg: segments of the finalize sum
TL_UNROLL = 8          # csrc/pcgmix_head.hip:225    g + 8 <= g1: eight loads in flight
LOSS_THREADS = 256     # csrc/pcgmix_head.hip:375    block size of the loss kernels
ZERO_BLOCK = 4096      # csrc/pcgmix_head.hip:1004   dW1 floats cleared per spare block
SK_ROWS = 32           # csrc/pcgmix_skinny.hip:31   kSkinnyRows: batch rows per block
SK_CHUNK = 512         # csrc/pcgmix_skinny.hip:32   kSkinnyChunk: K elements per partial plane
SK_WAVE = 128          # csrc/pcgmix_skinny.hip:35   kSkinnyChunk / kSkinnyWaves: columns per wave

F64 = torch.float64


def splits(K):
    """KS: partial planes of the split-K product (pcgmix_skinny_linear_splits)."""
    return (K + SK_CHUNK - 1) // SK_CHUNK


def nrb(B):
    """Row blocks of the tail kernels."""
    return (B + TAIL_ROWS - 1) // TAIL_ROWS


def tail_sum_shape(KS):
    """(trips of the four-deep loop, single loads behind it) of lane 0 in potes_tail_*'s split sum."""
    ks = deep = 0
    while ks + 3 * TAIL_LANES < KS:
        ks += TAIL_LANES * TAIL_DEPTH
        deep += 1
    return deep, len(range(ks, KS, TAIL_LANES))


def mask_bytes(n, bits):
    return (n * bits + 7) // 8


# ---- the bit rule ---------------------------------------------------------------------------------
def keep_loop(mask, n, bits, thr):
    """THE SPECIFICATION, one bit at a time: element e is kept iff the integer formed by bits
    e*bits .. e*bits + bits - 1 of the byte stream (least significant first) is >= thr."""
    m = mask.tolist()
    out = []
    for e in range(n):
        v = 0
        for j in range(bits):
            p = e * bits + j
            v |= ((m[p >> 3] >> (p & 7)) & 1) << j
        out.append(v >= thr)
    return torch.tensor(out, dtype=torch.bool)


def keep_vec(mask, n, bits, thr):
    """The same rule vectorised (an element never straddles a byte: bits divides 8)."""
    bit = torch.arange(n, dtype=torch.int64) * bits
    val = (mask.reshape(-1)[bit >> 3].to(torch.int64) >> (bit & 7)) & ((1 << bits) - 1)
    return val >= thr


def _d(t):
    return None if t is None else t.detach().to("cpu", F64)


def dropped(x, mask1, scale1, thr1, bits1):
    """(what the forward multiplies, keep) — keep is None without a mask."""
    x = _d(x)
    if mask1 is None:
        return x, None
    keep = keep_vec(mask1.cpu(), x.numel(), bits1, thr1).view_as(x)
    return torch.where(keep, x * scale1, torch.zeros((), dtype=F64)), keep


def tail_fac(z, mask2, scale2, thr2):
    """d h / d z: ReLU (dead at exactly 0) times the byte-wise second dropout."""
    fac = (z > 0).to(F64)
    if mask2 is not None:
        fac = fac * (mask2.cpu().reshape(z.shape).to(torch.int64) >= thr2).to(F64) * scale2
    return fac


# ---- forward --------------------------------------------------------------------------------------
def skinny_fwd(h, W, bias=None, mask=None, scale=1.0, thr=0, bits=8):
    """pcgmix_skinny_linear_fwd_f32 (mask = None) and the masked product of the head:
    (partial (KS,B,O): one plane per 512-column chunk, z (B,O) = their sum + bias)."""
    xm, _ = dropped(h, mask, scale, thr, bits)
    W = _d(W)
    K = xm.shape[1]
    planes = [xm[:, s:s + SK_CHUNK] @ W[:, s:s + SK_CHUNK].T for s in range(0, K, SK_CHUNK)]
    partial = torch.stack(planes)
    z = partial.sum(0)
    if bias is not None:
        z = z + _d(bias)
    return partial, z


def head_fwd(x, mask1, scale1, thr1, bits1, w1, b1, mask2, scale2, thr2, w2, b2):
    """pcgmix_potes_head_fwd_f32: partial, z, logits (and fac, h behind them)."""
    partial, z = skinny_fwd(x, w1, b1, mask1, scale1, thr1, bits1)
    fac = tail_fac(z, mask2, scale2, thr2)
    h = z * fac
    logits = h @ _d(w2).T
    if b2 is not None:
        logits = logits + _d(b2)
    return types.SimpleNamespace(partial=partial, z=z, fac=fac, h=h, logits=logits)


# ---- backward -------------------------------------------------------------------------------------
def tail_bwd(dlogits, z, mask2, scale2, thr2, w2):
    """potes_tail_bwd_kernel: dz (B,20), dW2 (C,20), db2 (C), db1 (20)."""
    dl, z, w2 = _d(dlogits), _d(z), _d(w2)
    fac = tail_fac(z, mask2, scale2, thr2)
    dz = (dl @ w2) * fac
    return types.SimpleNamespace(dz=dz, dw2=dl.T @ (z * fac), db2=dl.sum(0), db1=dz.sum(0))


def feature_bwd(dz, gscale, x, mask1, scale1, thr1, bits1, w1):
    """potes_head_bwd_kernel: dW1 (20,K) = (gs dz)^T xm and dx (B,K) = keep * scale1 * ((gs dz) W1),
    the gradient at the features BEFORE dropout 1.  gscale None = 1."""
    g = _d(dz) * (1.0 if gscale is None else float(gscale))
    xm, keep = dropped(x, mask1, scale1, thr1, bits1)
    dx = g @ _d(w1)
    if keep is not None:
        dx = torch.where(keep, dx * scale1, torch.zeros((), dtype=F64))
    return types.SimpleNamespace(dw1=g.T @ xm, dx=dx)


def head_bwd(dlogits, z, mask2, scale2, thr2, w2, x, mask1, scale1, thr1, bits1, w1):
    """pcgmix_potes_head_bwd_f32: dz, dw2, db2, db1, dw1, dx."""
    t = tail_bwd(dlogits, z, mask2, scale2, thr2, w2)
    f = feature_bwd(t.dz, None, x, mask1, scale1, thr1, bits1, w1)
    t.dw1, t.dx = f.dw1, f.dx
    return t


def saliency(x, w1, b1, w2, seed):
    """pcgmix_potes_head_saliency_f32: dz = (z > 0) * (seed W2), dx = dz W1 (eval mode, no masks)."""
    _, z = skinny_fwd(x, w1, b1)
    dz = (z > 0).to(F64) * (_d(seed) @ _d(w2))
    return types.SimpleNamespace(z=z, dz=dz, dx=dz @ _d(w1))


# ---- losses ---------------------------------------------------------------------------------------
def targets(target, kind, C):
    """target_kind 0: float (B,C), need not sum to 1; 1: uint8 class labels (B) -> one-hot rows."""
    if kind == 0:
        return _d(target)
    return torch.nn.functional.one_hot(target.cpu().long(), C).to(F64)


def _logp(logits):
    x = _d(logits)
    m = x.max(1, keepdim=True).values
    return x - m - torch.log(torch.exp(x - m).sum(1, keepdim=True))


def soft_ce(logits, target):
    """pcgmix_soft_ce_fwd_f32: mean_b(-sum_c log_softmax(logits)[b,c] target[b,c])."""
    return (-(_logp(logits) * _d(target)).sum(1)).mean()


def soft_ce_bwd(logits, target, gout=1.0):
    """pcgmix_soft_ce_bwd_f32 / pcgmix_selc_bwd_f32 (target = the rows the forward stored)."""
    t = _d(target)
    return float(gout) / t.shape[0] * (torch.exp(_logp(logits)) * t.sum(1, keepdim=True) - t)


def selc(logits, index, soft, keep, take):
    """pcgmix_selc_fwd_f32: pred = softmax(logits); soft[index] = keep*soft[index] + take*pred written
    back; loss = mean_b(-sum_c log(pred) soft[index]).  A row whose index is outside [0,N) updates
    nothing, has a zero row and gives zero loss.  Returns (loss, rows (B,C), the new soft (N,C))."""
    logp = _logp(logits)
    p = torch.exp(logp)
    soft = _d(soft).clone()
    rows = torch.zeros_like(p)
    for b, i in enumerate(index.tolist()):
        if 0 <= i < soft.shape[0]:
            soft[i] = float(keep) * soft[i] + float(take) * p[b]
            rows[b] = soft[i]
    return (-(logp * rows).sum(1)).mean(), rows, soft


def small_of(dw2, db2, db1):
    """small = [dW2 (C x 20) | db2 (C) | db1 (20)]."""
    return torch.cat([dw2.reshape(-1), db2.reshape(-1), db1.reshape(-1)])


def head_loss(x, mask1, scale1, thr1, bits1, w1, b1, mask2, scale2, thr2, w2, b2, target, kind,
              mix=None, inv=None, lam=1.0, selc_args=None):
    """pcgmix_potes_head_loss_fwd_f32, ..._latent_fwd_f32 (mix, inv, lam) and ..._selc_fwd_f32
    (selc_args = (index, soft, keep, take) in place of target / kind): z, logits, loss and, for
    d loss = 1, dz and small; for SELC also rows and the updated soft labels.
      latent: hm[b] = lam h[b] + (1-lam) h[mix[b]], logits from hm, dW2 = dl^T hm,
              dz[b] = fac[b] * W2^T (lam dl[b] + (1-lam) dl[inv[b]]); 1-lam is formed in float32."""
    f = head_fwd(x, mask1, scale1, thr1, bits1, w1, b1, None, 1.0, 0, w2, None)
    fac = tail_fac(f.z, mask2, scale2, thr2)
    h = f.z * fac
    w2d = _d(w2)
    C = w2d.shape[0]
    if mix is not None:
        l32 = np.float32(lam)
        la, oml = float(l32), float(np.float32(1) - l32)
        h = la * h + oml * h[mix.cpu().long()]
    logits = h @ w2d.T
    if b2 is not None:
        logits = logits + _d(b2)
    out = types.SimpleNamespace(partial=f.partial, z=f.z, logits=logits)
    if selc_args is not None:
        index, soft, keep, take = selc_args
        out.loss, t, out.soft = selc(logits, index, soft, keep, take)
        out.rows = t
    else:
        t = targets(target, kind, C)
        out.loss = soft_ce(logits, t)
    dl = soft_ce_bwd(logits, t)
    dle = dl if mix is None else la * dl + oml * dl[inv.cpu().long()]
    out.dlogits = dl
    out.dz = (dle @ w2d) * fac
    out.small = small_of(dl.T @ h, dl.sum(0), out.dz.sum(0))
    return out


def head_loss_bwd(dz, gscale, x, mask1, scale1, thr1, bits1, w1, small_in):
    """pcgmix_potes_head_loss_bwd_f32: dW1, dx from gs*dz, small_out = small_in * gs."""
    f = feature_bwd(dz, gscale, x, mask1, scale1, thr1, bits1, w1)
    gs = 1.0 if gscale is None else float(gscale)
    f.small = None if small_in is None else _d(small_in) * gs
    return f


# ---- shapes ---------------------------------------------------------------------------------------
# (B, K, C, bits, thr); bits = 0: no dropout at all (both masks NULL).  Not a full product: every
# value has at least two partners, K >= 6144 only with B <= 5, B = 257 only with K <= 516
# (tests/test_head_ref_cpu.py::test_shapes_cover_tile_edges says what the table covers).
HEAD_EDGE = [
    (3, 6148, 2, 1, 1), (3, 6144, 2, 2, 1), (5, 6144, 3, 8, 128), (1, 6148, 1, 4, 8),       # KS = 13, 12
    (4, 7680, 2, 1, 1), (5, 7680, 8, 0, 0), (1, 8192, 3, 4, 15), (4, 8192, 2, 8, 1),        # KS = 15, 16
    (3, 8196, 2, 1, 1), (5, 8196, 2, 2, 3), (1, 14848, 2, 8, 255), (5, 14848, 2, 2, 1),     # KS = 17, 29
    (5, 2492, 2, 1, 1), (129, 2492, 2, 1, 1), (32, 2492, 2, 2, 1),                          # Potes0.1 / 0.2
    (9, 4, 2, 1, 1), (17, 4, 3, 8, 0), (129, 4, 1, 4, 8),
    (9, 60, 2, 4, 8), (31, 60, 1, 2, 3), (127, 60, 2, 0, 0),
    (17, 64, 2, 1, 1), (33, 64, 8, 8, 1), (257, 64, 3, 8, 128),
    (33, 68, 2, 1, 1), (47, 68, 2, 8, 128), (128, 68, 2, 2, 1),
    (31, 124, 2, 8, 255), (48, 124, 3, 2, 1), (130, 124, 2, 8, 1),
    (32, 128, 2, 4, 15), (49, 128, 2, 0, 0), (113, 128, 2, 8, 0),
    (49, 132, 2, 1, 1), (127, 132, 2, 4, 8),
    (47, 508, 2, 2, 3), (128, 508, 2, 8, 1),
    (48, 512, 8, 1, 1), (130, 512, 2, 2, 1),
    (113, 516, 2, 1, 1), (257, 516, 2, 1, 1),
]
EDGE_IDS = [f"B{B}-K{K}-C{C}-bits{bits}-thr{thr}" for B, K, C, bits, thr in HEAD_EDGE]
SEEDS = 64             # int_case takes the first seed below this whose data is informative


# ---- inputs ---------------------------------------------------------------------------------------
def _below(bound, unit, name):
    assert float(bound) < 2.0 ** 24 * unit, f"{name}: sum of |addends| {float(bound):.4g} is not below 2**24 * {unit}"


def _abs_bounds(c, gs):
    """Order-independent bounds: the sum of the absolute values of the addends of every sum the
    kernels form on case c (all in units of 1: the data and the scales are integers)."""
    ax, _ = dropped(c.x, c.mask1, c.scale1, c.thr1, c.bits1)
    ax, aw1 = ax.abs(), _d(c.w1).abs()
    planes = torch.stack([ax[:, s:s + SK_CHUNK] @ aw1[:, s:s + SK_CHUNK].T for s in range(0, c.K, SK_CHUNK)])
    f, b = c.ref, c.bwd
    adl, aw2 = _d(c.dlogits).abs(), _d(c.w2).abs()
    adz = b.dz.abs() * gs
    asal = c.sal.dz.abs()
    return {
        "partial": planes.max(),
        "z": (planes.sum(0) + _d(c.b1).abs()).max(),
        "logits": (f.h.abs() @ aw2.T + _d(c.b2).abs()).max(),
        "dz": ((adl @ aw2) * f.fac).max(),
        "dW2": (adl.T @ f.h.abs()).max(),
        "db2": adl.sum(0).max(),
        "db1": b.dz.abs().sum(0).max(),
        "dW1": (adz.T @ ax).max(),
        "dx": ((adz @ aw1) * c.scale1).max(),
        "saliency dz": (_d(c.seed).abs() @ aw2).max(),
        "saliency dx": (asal @ aw1).max(),
        "saliency z": (_d(c.x).abs() @ aw1.T + _d(c.b1).abs()).max(),
    }


def _mask8(g, n, thr):
    """Random bytes for an 8-bit rule: uniform where that keeps 5..95 %, otherwise half of them drawn
    below thr and half at or above it, with thr - 1 and thr themselves frequent."""
    if thr == 0 or 13 <= thr <= 243:
        return torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
    lo = torch.randint(0, thr, (n,), generator=g)
    hi = torch.randint(thr, 256, (n,), generator=g)
    near = torch.randint(0, 2, (n,), generator=g).bool()
    lo, hi = torch.where(near, torch.full_like(lo, thr - 1), lo), torch.where(near, torch.full_like(hi, thr), hi)
    return torch.where(torch.randint(0, 2, (n,), generator=g).bool(), hi, lo).to(torch.uint8)


def _same_label_shuffle(labels):
    """Every row's partner is the next row of its class (the last one's is the first): same label,
    partners in the blocks ahead and — through the wrap — behind; a class of one is a fixed point."""
    mix = torch.arange(labels.numel(), dtype=torch.int32)
    for c in labels.unique().tolist():
        rows = (labels == c).nonzero().flatten()
        mix[rows] = rows.roll(-1).to(torch.int32)
    return mix


def _make(B, K, C, bits, thr, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()   # noqa: E731
    c = types.SimpleNamespace(B=B, K=K, C=C, bits1=bits or 8, thr1=thr, seed_used=seed, KS=splits(K), nrb=nrb(B))
    # features as the conv branch leaves them: >= 0, three in ten exactly 0
    c.x = ri(0, 3, B, K) * (torch.rand(B, K, generator=g) < 0.7).float()
    # w1: ten dense rows in {-1, 0, 1}; ten rows with at most eight non-zeros in {-2, -1, 1, 2}, whose z
    # is a short sum (exact zeros and sign changes are then common at every K)
    c.w1 = ri(-1, 1, HEAD_O, K)
    for o in range(HEAD_O // 2, HEAD_O):
        row = torch.zeros(K)
        at = torch.randperm(K, generator=g)[:8]
        row[at] = ri(1, 2, at.numel()) * (ri(0, 1, at.numel()) * 2 - 1)
        c.w1[o] = row
    c.b1, c.w2, c.b2 = ri(-2, 2, HEAD_O), ri(-2, 2, C, HEAD_O), ri(-2, 2, C)
    c.dlogits, c.seed = ri(-2, 2, B, C), ri(-2, 2, B, C)
    if bits:
        n1 = mask_bytes(B * K, bits)
        c.mask1 = _mask8(g, n1, thr) if bits == 8 else torch.randint(0, 256, (n1,), generator=g).to(torch.uint8)
        c.thr2 = (1, 64, 128, 255)[(B + K // 4) % 4]
        c.mask2 = _mask8(g, B * HEAD_O, c.thr2)
        c.scale1, c.scale2 = (2.0 if bits in (1, 8) else 4.0), (4.0 if bits == 8 else 2.0)
    else:
        c.mask1 = c.mask2 = None
        c.thr2, c.scale1, c.scale2 = 0, 1.0, 1.0
    # what the loss tests add: soft targets that do not sum to 1, labels, SELC state, partner permutations
    t = torch.rand(B, C, generator=g) + 0.05
    c.target = (t / t.sum(1, keepdim=True) * 1.3).float()
    c.labels = torch.randint(0, C, (B,), generator=g).to(torch.uint8)
    c.N = B + 7
    s = torch.rand(c.N, C, generator=g) + 0.05
    c.soft = (s / s.sum(1, keepdim=True)).float()
    c.index = torch.randperm(c.N, generator=g)[:B].to(torch.int64)          # distinct
    c.index[B // 2] = c.N + 3                                               # one row outside [0,N)
    ident = torch.arange(B, dtype=torch.int32)
    fixed = ident.clone()
    fixed[0::2] = ident[0::2].roll(-1)                                      # odd rows are fixed points
    c.perms = {"identity": ident, "same-label shuffle": _same_label_shuffle(c.labels.long()),
               "with fixed points": fixed}
    return c


def _args(c):
    return (c.x, c.mask1, c.scale1, c.thr1, c.bits1, c.w1, c.b1, c.mask2, c.scale2, c.thr2, c.w2, c.b2)


def inverse(mix):
    inv = torch.empty_like(mix)
    inv[mix.long()] = torch.arange(mix.numel(), dtype=mix.dtype)
    return inv


def _refs(c):
    c.ref = head_fwd(*_args(c))
    c.bwd = head_bwd(c.dlogits, c.ref.z, c.mask2, c.scale2, c.thr2, c.w2, c.x, c.mask1, c.scale1, c.thr1,
                     c.bits1, c.w1)
    c.sal = saliency(c.x, c.w1, c.b1, c.w2, c.seed)
    c.z_nonpos = float((c.ref.z <= 0).double().mean())
    c.z_zero = float((c.ref.z == 0).double().mean())
    c.keep1 = None if c.mask1 is None else float(keep_vec(c.mask1, c.B * c.K, c.bits1, c.thr1).double().mean())
    c.keep2 = None if c.mask2 is None else float((c.mask2.long() >= c.thr2).double().mean())


def all_keep(thr):
    return thr == 0


def informative(c):
    """The conditions tests/test_head_ref_cpu.py asserts for every table entry."""
    ok = c.z_nonpos >= 0.05 and c.z_zero >= 0.01
    for keep, thr in ((c.keep1, c.thr1), (c.keep2, c.thr2)):
        if keep is not None and not all_keep(thr):
            ok = ok and 0.05 <= keep <= 0.95
    return ok and bool(c.bwd.dw1.any()) and bool(c.bwd.dx.any()) and bool(c.sal.dx.any())


GSCALE = 2.0           # the power-of-two loss gradient of the exact pcgmix_potes_head_loss_bwd_f32 test


@functools.lru_cache(maxsize=None)
def int_case(B, K, C, bits, thr):
    """Integer data for one table entry (see the module docstring): x in {0..3} with exact zeros,
    w1 in {-1, 0, 1} (ten dense rows) and {-2..2} (ten sparse rows), b1, w2, b2, dlogits, seed in
    {-2..2}, masks of random bytes, scale1 and scale2 in {2, 4}.  The first seed whose data is
    ``informative`` is taken (asserted to exist), then every bound of ``_abs_bounds`` is asserted."""
    assert K % 4 == 0 and 1 <= C <= MAX_C and bits in (0, 1, 2, 4, 8) and 0 <= thr < (1 << (bits or 8))
    for seed in range(SEEDS):
        c = _make(B, K, C, bits, thr, seed)
        _refs(c)
        if informative(c):
            break
    else:
        raise AssertionError(f"int_case{(B, K, C, bits, thr)}: no informative data in {SEEDS} seeds")
    c.bounds = _abs_bounds(c, GSCALE)
    for name, bound in c.bounds.items():
        _below(bound, 1.0, name)
    return c


@functools.lru_cache(maxsize=None)
def dyadic_case(B, K, C, bits, thr):
    """int_case with w2 and b2 times 2**-s, s the smallest integer with max|logits| <= 8 (over both the
    masked and the unmasked second dropout the loss tests use): z unchanged, logits scaled exactly."""
    base = int_case(B, K, C, bits, thr)
    c = types.SimpleNamespace(**vars(base))
    top = float((base.ref.h.abs() @ _d(base.w2).abs().T + _d(base.b2).abs()).max())   # bounds any blend too
    c.shift = max(0, int(np.ceil(np.log2(max(top, 1.0) / 8.0))))
    c.w2, c.b2 = base.w2 * 2.0 ** -c.shift, base.b2 * 2.0 ** -c.shift
    c.ref = head_fwd(*_args(c))
    assert float(c.ref.logits.abs().max()) <= 8.0
    assert torch.equal(c.ref.z, base.ref.z) and torch.equal(c.ref.logits, base.ref.logits * 2.0 ** -c.shift)
    _below(base.bounds["logits"] * 2.0 ** -c.shift, 2.0 ** -c.shift, "logits (dyadic)")
    return c
