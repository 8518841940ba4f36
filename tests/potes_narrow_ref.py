"""Float64 restatement of the narrow ([1,1] and [2,1]) Potes conv stacks for
tests/test_potes_narrow_ref_cpu.py and tests/test_potes_narrow_edges_gpu.py, the inputs both use and
the shape table.  Not a test module.

The stacks (csrc/pcgmix_potes_narrow.hip) are Conv1d(1->C1, k5, pad 1) + ReLU + MaxPool1d(2), then
Conv1d(C1->C2, k5, pad 1) + ReLU + MaxPool1d(2), on N rows of T samples, (C1, C2) in WIDTHS.  The
geometry, the ReLU/pool rule (``route``: relu_pool2 of csrc/pcgmix_potes_stack.h written out, first
maximum wins, exactly 0 is dead) and the routing-byte layouts are those of the wide stack and are
imported from tests/potes_ref.py; everything that depends on the widths is here.

Two kinds of input, cached per (widths, N, T): the tests share one reference and must not write to it.
  int_case   x, r, b2 integers in -2..2, w1, w2, b1 in {-1, 0, 1}.  For every sum a kernel forms — the
             two conv chains, dL/da1 and dL/dx of the backward kernels, each weight / bias gradient over
             all rows and positions (any per-block partial and the reduction are sub-sums of it) — the
             sum of the ABSOLUTE values of its addends is computed and asserted < 2**24 (the rule of
             tests/head_ref.py).  Every partial sum, in any order and through any fmaf chain, is then
             an integer float32 holds exactly: a float32 kernel must equal float64 BIT FOR BIT.  Exact
             ties and exact zeros, which random data never produces, are common — asserted.
             No bias is zero either: with b2 = 0 (one draw in five) a kernel that dropped b2 from one
             of its two conv outputs would pass that case.
  rand_case  randn rows and default-initialised Conv1d weights, with ``decisions`` to tell whether
             float32 rounding could flip any ReLU/pool decision, and the a-priori bound on h2.

Finite inputs only (see tests/potes_ref.py).
"""
import functools
import types

import torch
import torch.nn.functional as F

from potes_ref import (U24, _candidates, _fragile, dims, pack_m2, pack_s1, route,  # noqa: F401
                       unpack_m2, unpack_s1)

K = 5
WIDTHS = [(1, 1), (2, 1)]

# ---- kernel constants, stated once (csrc/pcgmix_potes_narrow.hip) ------------------------------
NAR_TP = 256          # kNarTP: pooled outputs per tile of the forward and the weight gradient
THREADS = 256         # kThreads: also the rows one pass of narrow_reduce_kernel takes
IN_TU = 1024          # kInTU = 4 * kThreads: inputs per block of the input gradient
BWD_CAP = 1024        # pcgmix_potes_narrow_bwd_blocks: persistent blocks of the weight gradient
MAX_N = 65535         # kMaxN: rows (grid.y)
MIN_T = 14


def grad_len(C1, C2):
    """[gw1 | gb1 | gw2 | gb2]"""
    return K * C1 + C1 + K * C1 * C2 + C2


def grad_parts(C1, C2):
    return (("w1", K * C1), ("b1", C1), ("w2", K * C1 * C2), ("b2", C2))


def s1row(T):
    return (dims(T)[0] >> 2) + 1


def m2row(T):
    return (dims(T)[1] + 3) // 4


def fwd_tiles(T, with_s1):
    """fwd_tiles of the .hip file: with s1 the even outputs p <= 2 * (s1row - 1) each write one byte."""
    return ((2 * s1row(T) - 1 if with_s1 else dims(T)[1]) + NAR_TP - 1) // NAR_TP


def bwd_tiles(T):
    """bwd_tiles of the .hip file: a thread owns first-layer positions 2p, 2p + 1 < P1."""
    return ((dims(T)[0] + 1) // 2 + NAR_TP - 1) // NAR_TP


def in_blocks(T):
    return (T + IN_TU - 1) // IN_TU


def bwd_blocks(N, T):
    return min(N * bwd_tiles(T), BWD_CAP)


# ---- shapes -----------------------------------------------------------------------------------
SHORT_N, EDGE_N = 16, 3          # 16 rows where a row has only a handful of pairs; 3 rows, so that odd T
#                                  puts rows at odd float offsets
SHORT_T = [14, 15, 16, 17, 23]   # the minimum length and all four residues of T mod 4
EDGE_T = [1024, 1025,            # input gradient 1 -> 2 blocks; P1 = 511: the last s1 row of one forward tile
          1026,                  # P1 = 512: the forward with s1 needs two tiles, without it one (P2 = 255)
          1027, 1028,            # P2 = 255, generic / aligned; at 1028 (P1+1)//2 = 257: weight gradient 1 -> 2
          1032,                  # P2 = 256: exactly one tile
          1034, 1036,            # P2 = 257: one tile plus one output, generic / aligned
          2048, 2049,            # input gradient 2 -> 3 blocks
          2056, 2058, 2060]      # P2 = 512; 513, generic / aligned: three tiles in the forward and the weight gradient
EDGE = [(SHORT_N, T) for T in SHORT_T] + [(EDGE_N, T) for T in EDGE_T]
# the persistent loop of the weight gradient and the stride loop of its reduction
LOOP = [(300, 14),               # G = 300 > 256: threads 0..43 of the reduce take two partial rows
        (1030, 14),              # 1030 items on 1024 blocks: blocks 0..5 take a second item
        (520, 1028)]             # two tiles per row, 1040 items on 1024 blocks: blocks 0..15 go on to a tile of
#                                  another row (item / tiles, item % tiles with tiles = 2)
LIMIT = (MAX_N, 14)              # the row limit; integer data only
# (widths, N, T) -> seed, 0 where absent.  Integer cases: the first seed whose data passes int_case's
# exactness and non-degeneracy assertions.  Random cases: the first seed with no undecidable decision.
INT_SEED = {
    ((1, 1), 16, 14): 1, ((1, 1), 16, 15): 1, ((1, 1), 16, 16): 12, ((1, 1), 16, 23): 1, ((1, 1), 3, 1024): 1,
    ((1, 1), 3, 1025): 2, ((1, 1), 3, 1026): 5, ((1, 1), 3, 1028): 2, ((1, 1), 3, 1032): 13, ((1, 1), 3, 1034): 4,
    ((1, 1), 3, 1036): 2, ((1, 1), 3, 2049): 2, ((1, 1), 3, 2058): 4, ((1, 1), 3, 2060): 6, ((1, 1), 300, 14): 13,
    ((1, 1), 1030, 14): 7, ((1, 1), 520, 1028): 3, ((1, 1), 65535, 14): 5, ((2, 1), 16, 14): 9, ((2, 1), 16, 15): 23,
    ((2, 1), 16, 16): 26, ((2, 1), 16, 17): 32, ((2, 1), 16, 23): 27, ((2, 1), 3, 1025): 2, ((2, 1), 3, 1026): 2,
    ((2, 1), 3, 1027): 3, ((2, 1), 3, 1028): 7, ((2, 1), 3, 1032): 1, ((2, 1), 3, 1034): 5, ((2, 1), 3, 1036): 10,
    ((2, 1), 3, 2048): 1, ((2, 1), 3, 2049): 2, ((2, 1), 3, 2056): 1, ((2, 1), 3, 2058): 10, ((2, 1), 3, 2060): 5,
    ((2, 1), 300, 14): 16, ((2, 1), 1030, 14): 6, ((2, 1), 520, 1028): 2, ((2, 1), 65535, 14): 30}
RAND_SEED = {((2, 1), 3, 2048): 1, ((2, 1), 3, 2049): 1, ((2, 1), 3, 2056): 1, ((2, 1), 3, 2058): 1,
             ((2, 1), 3, 2060): 1, ((2, 1), 520, 1028): 4}


# ---- the stack --------------------------------------------------------------------------------
def stack_ref(x, w1, b1, w2, b2, r):
    """x (N,T), w1 (C1,1,5), b1 (C1), w2 (C2,C1,5), b2 (C2), r (N,C2,P2), any float dtype.  Float64
    on the CPU; the gradients are those of (h2 * r).sum() through ``route``'s routing.  Returns h2
    (N,C2,P2), gx (N,T), grads (grad_len: [gw1 | gb1 | gw2 | gb2]), code1 (N,C1,P1), code2 (N,C2,P2),
    the packed m2 and s1, and the intermediates z1, a1, z2 with dL/dz1 and dL/dz2."""
    P1, P2 = dims(x.shape[1])
    x64 = x.detach().double().cpu().clone().requires_grad_(True)
    p64 = [p.detach().double().cpu().clone().requires_grad_(True) for p in (w1, b1, w2, b2)]
    z1 = F.conv1d(x64[:, None, :], p64[0], p64[1], padding=1)
    a1, code1 = route(z1, P1)
    z2 = F.conv1d(a1, p64[2], p64[3], padding=1)
    h2, code2 = route(z2, P2)
    g = torch.autograd.grad((h2 * r.detach().double().cpu()).sum(), [x64] + p64 + [z1, z2])
    return types.SimpleNamespace(h2=h2.detach(), gx=g[0], grads=torch.cat([t.reshape(-1) for t in g[1:5]]),
                                 code1=code1, code2=code2, m2=pack_m2(code2, P2), s1=pack_s1(code1, P1),
                                 z1=z1.detach(), a1=a1.detach(), z2=z2.detach(), gz1=g[5], gz2=g[6])


def _case(widths, x, w1, b1, w2, b2, r, **kw):
    c = types.SimpleNamespace(widths=widths, C1=widths[0], C2=widths[1], x=x, w1=w1, b1=b1, w2=w2, b2=b2,
                              r=r, N=x.shape[0], T=x.shape[1], **kw)
    c.P1, c.P2 = dims(c.T)
    c.ref = stack_ref(x, w1, b1, w2, b2, r)
    c.m2, c.s1 = c.ref.m2, c.ref.s1
    return c


# ---- integer inputs -----------------------------------------------------------------------------
def abs_bounds(c):
    """For every sum the three kernels form on case c: the largest sum of the absolute values of its
    addends.  The gradients of a conv in |.| data are exactly those sums."""
    ref = c.ref
    x, w1, b1, w2, b2 = (t.detach().double().abs() for t in (c.x, c.w1, c.b1, c.w2, c.b2))
    a1, gz1, gz2 = ref.a1.abs(), ref.gz1.abs(), ref.gz2.abs()

    def conv_sums(inp, w, b, gz):
        inp, w = inp.clone().requires_grad_(True), w.clone().requires_grad_(True)
        z = F.conv1d(inp, w, b, padding=1)
        gi, gw = torch.autograd.grad((z * gz).sum(), [inp, w])
        return z.detach().max(), gi.max(), gw.max()

    z1, dx, gw1 = conv_sums(x[:, None, :], w1, b1, gz1)
    z2, ga1, gw2 = conv_sums(a1, w2, b2, gz2)
    return {"z1": z1, "z2": z2, "ga1": ga1, "dx": dx, "gw1": gw1, "gb1": gz1.sum((0, 2)).max(),
            "gw2": gw2, "gb2": gz2.sum((0, 2)).max()}


def _fractions(z, code, P):
    za, zb = _candidates(z, P)
    tie = float(((za == zb) & (za > 0)).double().mean())
    return tie, [float((code == k).double().mean()) for k in (0, 1, 2)]


def degenerate(c):
    """None, or why the integer case c would not exercise the tie and zero rules or some gradient."""
    for layer, z, code, P in ((1, c.ref.z1, c.ref.code1, c.P1), (2, c.ref.z2, c.ref.code2, c.P2)):
        tie, codes = _fractions(z, code, P)
        if tie < 0.01:
            return f"layer {layer}: exact positive ties in {tie:.4f} of the pairs"
        if min(codes) < 0.05:
            return f"layer {layer}: code fractions {codes}"
    if not bool((c.ref.grads != 0).all()):
        return "a weight or bias gradient is zero"
    if not (bool((c.b1 != 0).all()) and bool((c.b2 != 0).all())):
        return "a bias is zero: a kernel that dropped it would go unnoticed"
    nz = float((c.ref.gx != 0).double().mean())
    if nz < 0.20:
        return f"gx non-zero in {nz:.3f} of the elements"
    return None


def int_data(widths, N, T, seed):
    """(x, w1, b1, w2, b2, r) of one seed."""
    C1, C2 = widths
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()   # noqa: E731
    return (ri(-2, 2, N, T), ri(-1, 1, C1, 1, K), ri(-1, 1, C1), ri(-1, 1, C2, C1, K), ri(-2, 2, C2),
            ri(-2, 2, N, C2, dims(T)[1]))


def make_int(widths, N, T, seed):
    """The integer data of one seed with its reference, unjudged."""
    return _case(widths, *int_data(widths, N, T, seed), seed=seed)


@functools.lru_cache(maxsize=None)
def int_case(widths, N, T, seed=None):
    """Integer-valued float32 data (see the module docstring) with its float64 reference.  Asserts
    exactness (every bound of ``abs_bounds`` < 2**24) and that the case has not degenerated: >= 1 %
    exact positive ties and >= 5 % of each code 0, 1, 2 in both layers, no zero among the weight and
    bias gradients nor among the biases themselves, >= 20 % of gx non-zero."""
    if seed is None:
        seed = INT_SEED.get((widths, N, T), 0)
    c = make_int(widths, N, T, seed)
    c.bounds = abs_bounds(c)
    for name, bound in c.bounds.items():
        assert float(bound) < 2.0 ** 24, f"int_case{(widths, N, T, seed)} {name}: sum of |addends| {float(bound):.4g}"
    why = degenerate(c)
    assert why is None, f"int_case{(widths, N, T, seed)} degenerated: {why}"
    return c


# ---- could float32 rounding flip a decision? ----------------------------------------------------
def chain_factor(n):
    """Bound, in units of 2^-24 times the sum of |terms|, on the float32 error of a sum of n terms
    (products w * a, or the bias) formed in ANY order: a term passes through at most one rounding of
    its product and n - 1 of additions, n in all, and (1 + u)^n - 1 < (n + 1) u for n u << 1.  n = 6
    gives the 7 of potes_ref.undecidable's first layer."""
    return n + 1


def decisions(x, w1, b1, w2, b2):
    """potes_ref.undecidable for any C1: the number of ReLU/pool decisions (both layers) whose float64
    margin lies within the a-priori float32 error bound, and the bounds themselves:
      layer 1: e1 = chain_factor(6) 2^-24 (sum |w1||x| + |b1|)
      layer 2: e2 = chain_factor(5 C1 + 1) 2^-24 (sum |w2||a1| + |b2|) + sum |w2| e(a1), e(a1) the larger
               e1 of the pooled pair (ReLU and max are 1-Lipschitz)
      h2:      the larger e2 of its pair, for the same reason."""
    P1, P2 = dims(x.shape[1])
    x, w1, b1, w2, b2 = (t.detach().double().cpu() for t in (x, w1, b1, w2, b2))
    C1 = w1.shape[0]
    z1 = F.conv1d(x[:, None, :], w1, b1, padding=1)
    e1 = chain_factor(K + 1) * U24 * F.conv1d(x.abs()[:, None, :], w1.abs(), b1.abs(), padding=1)
    za, zb = _candidates(z1, P1)
    ea, eb = _candidates(e1, P1)
    n1 = int(_fragile(za, zb, ea, eb).sum())
    a1, _ = route(z1, P1)
    ea1 = torch.maximum(ea, eb)
    z2 = F.conv1d(a1, w2, b2, padding=1)
    e2 = chain_factor(K * C1 + 1) * U24 * F.conv1d(a1.abs(), w2.abs(), b2.abs(), padding=1) \
        + F.conv1d(ea1, w2.abs(), None, padding=1)
    za, zb = _candidates(z2, P2)
    ea, eb = _candidates(e2, P2)
    return types.SimpleNamespace(undecidable=n1 + int(_fragile(za, zb, ea, eb).sum()), e1=e1, e2=e2,
                                 e_h2=torch.maximum(ea, eb))


@functools.lru_cache(maxsize=None)
def rand_case(widths, N, T, seed=None):
    """randn rows and output weights, Conv1d's default initialisation; the global RNG is left alone.
    c.undecidable counts the decisions float32 could flip, c.e2 (N,C2,P2) bounds |h2 - float64| per
    element.  Cached like int_case."""
    if seed is None:
        seed = RAND_SEED.get((widths, N, T), 0)
    C1, C2 = widths
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        c1, c2 = torch.nn.Conv1d(1, C1, K, padding=1), torch.nn.Conv1d(C1, C2, K, padding=1)
        x = torch.randn(N, T)
        r = torch.randn(N, C2, dims(T)[1])
    p = [t.detach() for t in (c1.weight, c1.bias, c2.weight, c2.bias)]
    c = _case(widths, x, *p, r, seed=seed)
    d = decisions(x, *p)
    c.undecidable, c.e2 = d.undecidable, d.e_h2
    return c
