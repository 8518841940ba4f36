"""Float64 restatement of the Potes conv stack for ANY layer widths (C1, C2) — tests/potes_ref.py is
the [8,4] instance — for tests/test_potes_big_cpu.py and tests/test_potes_big_gpu.py (the big stacks
of csrc/pcgmix_potes_big.hip, layers [64,32] and [128,64]).  Not a test module.

The routing rule, the byte packings and the fragility test are potes_ref's own (imported, not
restated).  New here:
  * ``stack_ref(..., codes=)`` can be GIVEN the routing codes instead of deriving them — the gradient
    of a kernel whose float32 rounding flipped a near-tie is then judged against the float64 gradient
    of the same routing;
  * ``undecidable`` returns the boolean maps of both layers (and, for layer 2, which codes the bound
    allows), with n = 5*C1 + 1 terms in a second-layer chain: the constant 43 = 5*8 + 3 of potes_ref
    becomes 5*C1 + 3;
  * ``int_case`` takes the widths and a density of the second layer's weights.
"""
import functools
import types

import torch
import torch.nn.functional as F

from potes_ref import (K, U24, _candidates, _fragile, dims, pack_m2, pack_s1, route,  # noqa: F401
                       unpack_m2, unpack_s1)

WIDTHS = [(64, 32), (128, 64)]


def grad_len(C1, C2):
    return K * C1 + C1 + K * C1 * C2 + C2          # [gw1 | gb1 | gw2 | gb2]


def _route_by(z, P, code):
    """ReLU + MaxPool1d(2) with the decisions GIVEN: the pooled value is the candidate the code names."""
    za, zb = _candidates(z, P)
    zero = torch.zeros((), dtype=z.dtype)
    return torch.where(code == 2, zb, torch.where(code == 1, za, zero))


def stack_ref(x, w1, b1, w2, b2, r, codes=None):
    """x (N, T), w1 (C1,1,5), b1 (C1), w2 (C2,C1,5), b2 (C2), r (N, C2, P2), any float dtype.  Returns
    float64 CPU tensors: h2 (N,C2,P2); gx (N,T) and grads ([gw1|gb1|gw2|gb2]) of (h2 * r).sum(); code1
    (N,C1,P1) and code2 (N,C2,P2), uint8.  codes = (code1, code2): route by these instead."""
    P1, P2 = dims(x.shape[1])
    x64 = x.detach().double().cpu().clone().requires_grad_(True)
    p64 = [p.detach().double().cpu().clone().requires_grad_(True) for p in (w1, b1, w2, b2)]
    z1 = F.conv1d(x64[:, None, :], p64[0], p64[1], padding=1)
    if codes is None:
        a1, code1 = route(z1, P1)
    else:
        code1 = codes[0]
        a1 = _route_by(z1, P1, code1)
    z2 = F.conv1d(a1, p64[2], p64[3], padding=1)
    if codes is None:
        h2, code2 = route(z2, P2)
    else:
        code2 = codes[1]
        h2 = _route_by(z2, P2, code2)
    g = torch.autograd.grad((h2 * r.detach().double().cpu()).sum(), [x64] + p64)
    return types.SimpleNamespace(h2=h2.detach(), gx=g[0], grads=torch.cat([t.reshape(-1) for t in g[1:]]),
                                 code1=code1, code2=code2, z1=z1.detach(), z2=z2.detach(), a1=a1.detach())


def _allowed(za, zb, ea, eb):
    """(..., 3) bool: code k is reachable with errors of up to ea / eb on the candidates."""
    two = (zb + eb > za - ea) & (zb + eb > 0)
    one = (za + ea >= zb - eb) & (za + ea > 0)
    none = (za - ea <= 0) & (zb - eb <= 0)
    return torch.stack([none, one, two], dim=-1)


def undecidable(x, w1, b1, w2, b2):
    """The ReLU/pool decisions whose float64 margin lies within an a-priori bound on the float32
    accumulation error, for ANY summation order (the matrix instruction's included):
      layer 1: e1 = 7 * 2^-24 * (sum |w1||x| + |b1|)
      layer 2: e2 = (5 C1 + 3) * 2^-24 * (sum |w2||a1| + |b2|) + sum |w2| e(a1)     (n = 5 C1 + 1 terms)
    Returns frag1 (N,C1,P1), frag2 (N,C2,P2) bool, and allowed2 (N,C2,P2,3): the codes the bound allows."""
    C1 = w1.shape[0]
    P1, P2 = dims(x.shape[1])
    x, w1, b1, w2, b2 = (t.detach().double().cpu() for t in (x, w1, b1, w2, b2))
    z1 = F.conv1d(x[:, None, :], w1, b1, padding=1)
    e1 = 7 * U24 * F.conv1d(x.abs()[:, None, :], w1.abs(), b1.abs(), padding=1)
    za, zb = _candidates(z1, P1)
    ea, eb = _candidates(e1, P1)
    frag1 = _fragile(za, zb, ea, eb)
    a1, _ = route(z1, P1)
    ea1 = torch.maximum(ea, eb)
    z2 = F.conv1d(a1, w2, b2, padding=1)
    e2 = (K * C1 + 3) * U24 * F.conv1d(a1.abs(), w2.abs(), b2.abs(), padding=1) + \
        F.conv1d(ea1, w2.abs(), None, padding=1)
    za, zb = _candidates(z2, P2)
    ea, eb = _candidates(e2, P2)
    return types.SimpleNamespace(frag1=frag1, frag2=_fragile(za, zb, ea, eb), allowed2=_allowed(za, zb, ea, eb))


def _case(x, w1, b1, w2, b2, r, **kw):
    c = types.SimpleNamespace(x=x, w1=w1, b1=b1, w2=w2, b2=b2, r=r, N=x.shape[0], T=x.shape[1],
                              C1=w1.shape[0], C2=w2.shape[0], **kw)
    c.P1, c.P2 = dims(c.T)
    c.ref = stack_ref(x, w1, b1, w2, b2, r)
    c.m2 = pack_m2(c.ref.code2, c.P2)
    c.s1 = pack_s1(c.ref.code1, c.P1)
    return c


def _tie_fraction(z, P):
    za, zb = _candidates(z, P)
    return float(((za == zb) & (za > 0)).double().mean())


@functools.lru_cache(maxsize=None)
def int_case(widths, N, T, density, seed=0):
    """Integer-valued float32 data: x, r, b2 in {-2..2}; w1, b1 in {-1,0,1}; w2 in {-1,0,1} times a
    Bernoulli(density) mask.  Then |z1| <= 11, |z2| <= 55 C1 + 2, |dL/da1| <= 10 C2 and every partial
    sum of gw1 is an integer of magnitude <= 20 C2 N T: with that below 2**24 (asserted, with every
    reference tensor) float32 is exact in any order, the matrix instruction included.  density 1.0
    runs the whole K loop on dense operands; 1/32 produces exact ties (>= 1 % per layer, asserted for
    density < 1 only).  Cached: tests share one reference per case and must not write to it."""
    C1, C2 = widths
    assert 20 * C2 * N * T < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    P1, P2 = dims(T)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()   # noqa: E731
    x, w1, b1, w2 = ri(-2, 2, N, T), ri(-1, 1, C1, 1, K), ri(-1, 1, C1), ri(-1, 1, C2, C1, K)
    keep = (torch.rand(C2, C1, K, generator=g) < density).float()
    c = _case(x, w1, b1, w2 * keep, ri(-2, 2, C2), ri(-2, 2, N, C2, P2), seed=seed, density=density)
    for name in ("h2", "gx", "grads", "z1", "z2"):
        assert float(getattr(c.ref, name).abs().max()) < 2 ** 24, name
    c.ties = (_tie_fraction(c.ref.z1, P1), _tie_fraction(c.ref.z2, P2))
    if density < 1:
        assert min(c.ties) >= 0.01, f"int_case({widths}, {N}, {T}, {density}, seed={seed}): ties {c.ties}"
    return c


@functools.lru_cache(maxsize=None)
def rand_case(widths, N, T, seed=0):
    """randn rows and output weights, Conv1d's default initialisation; the global RNG is left alone.
    c.und is undecidable() of this input.  Cached like int_case."""
    C1, C2 = widths
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        c1, c2 = torch.nn.Conv1d(1, C1, K, padding=1), torch.nn.Conv1d(C1, C2, K, padding=1)
        x = torch.randn(N, T)
        r = torch.randn(N, C2, dims(T)[1])
    p = [t.detach() for t in (c1.weight, c1.bias, c2.weight, c2.bias)]
    c = _case(x, *p, r, seed=seed)
    c.und = undecidable(x, *p)
    return c
