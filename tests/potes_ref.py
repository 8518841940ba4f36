"""Float64 restatement of the wide ([8,4]) Potes conv stack for tests/test_potes_ref_cpu.py and
tests/test_potes_edges_gpu.py, the inputs both use and the shape table.  Not a test module.

The stack (csrc/pcgmix_potes.hip) is Conv1d(1->8, k5, pad 1) + ReLU + MaxPool1d(2), then
Conv1d(8->4, k5, pad 1) + ReLU + MaxPool1d(2), on N rows of T samples.  Here it is torch float64 on
the CPU, and the ReLU/pool routing is NOT taken from ``max_pool1d`` indices: it is computed from the
float64 pre-activations with the rule of csrc/pcgmix_potes_stack.h (``relu_pool2``) written out —
code 0: both candidates ReLU-dead, 1: the first candidate (conv output 2q) won, 2: the second was
STRICTLY larger (the first maximum wins a tie) — and the gradients flow through exactly that routing.

Two kinds of input:
  int_case   small integers.  Every intermediate, in float32 or float64 and in any summation order
             (fmaf chains, packed multiply-adds, the f32 matrix instruction), is an integer below
             2**24, so a float32 kernel must give the float64 result BIT FOR BIT — and exact ties and
             exact zeros, which random data never produces, are common.
  rand_case  randn rows and default-initialised Conv1d weights, with ``undecidable`` to tell
             whether float32 rounding could flip any ReLU/pool decision of that input.

Finite inputs only: ``relu_max2`` (one v_max3_f32) documents finite operands, and torch would
propagate a NaN where that instruction does not.  Nothing here generates or judges non-finite data.
"""
import functools
import types

import torch
import torch.nn.functional as F

C1, C2, K = 8, 4, 5
NGRAD = C1 * K + C1 + C2 * C1 * K + C2            # 212, [gw1 | gb1 | gw2 | gb2]
U24 = 2.0 ** -24                                  # float32 unit roundoff

# ---- shapes -----------------------------------------------------------------------------------
# Tile constants of csrc/pcgmix_potes.hip: the forward owns kFwdTP = 252 pooled outputs per tile, the
# weight gradient has (P2 + 2 + 124) // 125 tiles per row, the input gradient owns kInNU = 496 inputs
# per tile.  P1 = (T-2)//2, P2 = (P1-2)//2.
FWD_TP, BWD_TP, IN_NU = 252, 125, 496
EDGE_N = 3            # odd T then puts rows at odd float offsets: the input gradient's scalar stores
EDGE_T = [14, 23,             # P2 = 2, 4: the minimum length; one partly filled tile everywhere
          496, 497,           # 122: input-gradient tile 1 -> 2
          498, 502,           # 123, 124: weight-gradient tile 1 -> 2
          506,                # 125
          992, 993,           # 246: input-gradient tile 2 -> 3
          998, 1002,          # 248, 249: weight-gradient tile 2 -> 3
          1013,               # 251: forward tile minus one
          1016, 1017,         # 252: exactly one forward tile, aligned and generic staging
          1018, 1020,         # 253: one whole tile plus a one-output tile, both stagings
          2024, 2026]         # 504, 505: two whole tiles; two plus one
PERSIST_N = 5
PERSIST_T = [1018, 2026, 502]                     # 2-5 tiles per row in every persistent kernel
# (N, T) -> seed.  Integer cases: the first seed at which both layers have >= 1 % exact positive ties
# (int_case asserts it; only the shortest rows, with a few dozen pairs, need more than seed 0).
# Random cases: the first seed with undecidable(...) == 0 (the GPU test asserts it).
INT_SEED = {(3, 998): 2, (3, 1017): 1, (3, 1020): 1, (5, 502): 1, (3100, 14): 1}
RAND_SEED = {}                                    # seed 0 has no undecidable position at any shape used


def dims(T):
    P1 = (T - 2) // 2
    return P1, (P1 - 2) // 2


def fwd_tiles(T):
    return (dims(T)[1] + FWD_TP - 1) // FWD_TP


def bwd_tiles(T):
    return (dims(T)[1] + 2 + BWD_TP - 1) // BWD_TP


def in_tiles(T):
    return (T + IN_NU - 1) // IN_NU


# ---- the stack --------------------------------------------------------------------------------
def _candidates(z, P):
    return z[..., 0:2 * P:2], z[..., 1:2 * P:2]


def route(z, P):
    """ReLU + MaxPool1d(2) of pre-activations z (..., L >= 2P): (pooled values, codes uint8)."""
    za, zb = _candidates(z, P)
    second = (zb > za) & (zb > 0)
    first = ~second & (za > 0)
    zero = torch.zeros((), dtype=z.dtype)
    a = torch.where(second, zb, torch.where(first, za, zero))
    return a, second.to(torch.uint8) * 2 + first.to(torch.uint8)


def stack_ref(x, w1, b1, w2, b2, r):
    """x (N, T), w1 (8,1,5), b1 (8), w2 (4,8,5), b2 (4), r (N, 4, P2), any float dtype.  Returns a
    namespace of float64 CPU tensors: h2 (N,4,P2); gx (N,T) and grads (212, [gw1|gb1|gw2|gb2]) of
    (h2 * r).sum(); code1 (N,8,P1) and code2 (N,4,P2), uint8."""
    P1, P2 = dims(x.shape[1])
    x64 = x.detach().double().cpu().clone().requires_grad_(True)
    p64 = [p.detach().double().cpu().clone().requires_grad_(True) for p in (w1, b1, w2, b2)]
    z1 = F.conv1d(x64[:, None, :], p64[0], p64[1], padding=1)
    a1, code1 = route(z1, P1)
    z2 = F.conv1d(a1, p64[2], p64[3], padding=1)
    h2, code2 = route(z2, P2)
    g = torch.autograd.grad((h2 * r.detach().double().cpu()).sum(), [x64] + p64)
    return types.SimpleNamespace(h2=h2.detach(), gx=g[0], grads=torch.cat([t.reshape(-1) for t in g[1:]]),
                                 code1=code1, code2=code2, z1=z1.detach(), z2=z2.detach(), a1=a1.detach())


# ---- routing bytes (csrc/pcgmix_potes_stack.h) ------------------------------------------------
def _pack4(slots):
    q = slots.reshape(*slots.shape[:-1], -1, 4).to(torch.int32)
    return (q[..., 0] | (q[..., 1] << 2) | (q[..., 2] << 4) | (q[..., 3] << 6)).to(torch.uint8)


def _unpack4(b):
    b = b.to(torch.int32)
    return torch.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], dim=-1).reshape(*b.shape[:-1], -1).to(torch.uint8)


def pack_m2(codes, P2):
    """codes (..., P2) -> (..., (P2+3)//4) bytes: output p in bits 2*(p&3) of byte p>>2, code 0 in the
    tail of the last byte."""
    assert codes.shape[-1] == P2
    slots = torch.zeros(*codes.shape[:-1], 4 * ((P2 + 3) // 4), dtype=torch.uint8)
    slots[..., :P2] = codes
    return _pack4(slots)


def pack_s1(codes, P1):
    """codes (..., P1) -> (..., (P1>>2)+1) bytes: position q in bits 2*((q+1)&3) of byte (q+1)>>2, code
    0 at q = -1 (the low bits of byte 0) and behind q = P1 - 1."""
    assert codes.shape[-1] == P1
    slots = torch.zeros(*codes.shape[:-1], 4 * ((P1 >> 2) + 1), dtype=torch.uint8)
    slots[..., 1:P1 + 1] = codes
    return _pack4(slots)


def unpack_m2(b, P2):
    return _unpack4(b)[..., :P2]


def unpack_s1(b, P1):
    return _unpack4(b)[..., 1:P1 + 1]


# ---- could float32 rounding flip a decision? ----------------------------------------------------
def _fragile(za, zb, ea, eb):
    """Pairs whose code an error of up to ea / eb on the candidates could change: the margin that
    decides the code (|zb - za| and the winner's sign; both signs where both are dead) within bound."""
    second = (zb > za) & (zb > 0)
    first = ~second & (za > 0)
    safe2 = second & (zb - za > ea + eb) & (zb > eb)
    safe1 = first & (za - zb > ea + eb) & (za > ea)
    safe0 = ~second & ~first & (za < -ea) & (zb < -eb)
    return ~(safe2 | safe1 | safe0)


def undecidable(x, w1, b1, w2, b2):
    """Number of ReLU/pool decisions (both layers) whose float64 margin lies within an a-priori bound
    on the float32 accumulation error, for ANY summation order:
      layer 1: e1 = 7 * 2^-24 * (sum |w1||x| + |b1|)          (n + 1 roundings of n = 6 terms, plus one)
      layer 2: e2 = 43 * 2^-24 * (sum |w2||a1| + |b2|) + sum |w2| e(a1)   (n = 41; e(a1) = the larger e1
               of the pooled pair: ReLU and max are 1-Lipschitz)."""
    P1, P2 = dims(x.shape[1])
    x, w1, b1, w2, b2 = (t.detach().double().cpu() for t in (x, w1, b1, w2, b2))
    z1 = F.conv1d(x[:, None, :], w1, b1, padding=1)
    e1 = 7 * U24 * F.conv1d(x.abs()[:, None, :], w1.abs(), b1.abs(), padding=1)
    za, zb = _candidates(z1, P1)
    ea, eb = _candidates(e1, P1)
    n1 = int(_fragile(za, zb, ea, eb).sum())
    a1, _ = route(z1, P1)
    ea1 = torch.maximum(ea, eb)
    z2 = F.conv1d(a1, w2, b2, padding=1)
    e2 = 43 * U24 * F.conv1d(a1.abs(), w2.abs(), b2.abs(), padding=1) + F.conv1d(ea1, w2.abs(), None, padding=1)
    za, zb = _candidates(z2, P2)
    ea, eb = _candidates(e2, P2)
    return n1 + int(_fragile(za, zb, ea, eb).sum())


# ---- inputs -----------------------------------------------------------------------------------
def _case(x, w1, b1, w2, b2, r, **kw):
    c = types.SimpleNamespace(x=x, w1=w1, b1=b1, w2=w2, b2=b2, r=r, N=x.shape[0], T=x.shape[1], **kw)
    c.P1, c.P2 = dims(c.T)
    c.ref = stack_ref(x, w1, b1, w2, b2, r)
    c.m2 = pack_m2(c.ref.code2, c.P2)
    c.s1 = pack_s1(c.ref.code1, c.P1)
    return c


def _tie_fraction(z, P):
    za, zb = _candidates(z, P)
    return float(((za == zb) & (za > 0)).double().mean())


@functools.lru_cache(maxsize=None)
def int_case(N, T, seed=None):
    """Integer-valued float32 data: x, r, b2 in {-2..2}, w1, w2, b1 in {-1, 0, 1}.  Then |z1| <= 11,
    |a1| <= 11, |z2| <= 442, |dL/da1| <= 40 and every partial sum of a weight gradient is an integer
    of magnitude <= 80 N T, so with N T < 2**24 / 80 float32 is exact in any order.  Cached: the
    tests share one reference per shape and must not write to it."""
    if seed is None:
        seed = INT_SEED.get((N, T), 0)
    assert 80 * N * T < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    P1, P2 = dims(T)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()   # noqa: E731
    c = _case(ri(-2, 2, N, T), ri(-1, 1, C1, 1, K), ri(-1, 1, C1), ri(-1, 1, C2, C1, K), ri(-2, 2, C2),
              ri(-2, 2, N, C2, P2), seed=seed)
    for name in ("h2", "gx", "grads", "z1", "z2"):
        assert float(getattr(c.ref, name).abs().max()) < 2 ** 24, name
    c.ties = (_tie_fraction(c.ref.z1, P1), _tie_fraction(c.ref.z2, P2))
    c.zeros1 = float((c.ref.z1 == 0).double().mean())
    assert min(c.ties) >= 0.01, f"int_case({N}, {T}, seed={seed}) degenerated: tie fractions {c.ties}"
    return c


@functools.lru_cache(maxsize=None)
def rand_case(N, T, seed=None):
    """randn rows and output weights, Conv1d's default initialisation; the global RNG is left alone.
    c.undecidable is undecidable() of this input.  Cached like int_case."""
    if seed is None:
        seed = RAND_SEED.get((N, T), 0)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        c1, c2 = torch.nn.Conv1d(1, C1, K, padding=1), torch.nn.Conv1d(C1, C2, K, padding=1)
        x = torch.randn(N, T)
        r = torch.randn(N, C2, dims(T)[1])
    p = [t.detach() for t in (c1.weight, c1.bias, c2.weight, c2.bias)]
    c = _case(x, *p, r, seed=seed)
    c.undecidable = undecidable(x, *p)
    return c
