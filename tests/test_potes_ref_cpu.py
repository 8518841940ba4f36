"""tests/potes_ref.py against torch's own modules on the CPU, its byte layouts against themselves,
the exactness claim of its integer inputs, and what its shape table covers.  No GPU."""
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import models

import potes_ref as R


def _module_with(c):
    """models.CNN_potes_TS.cnn1 (float32, CPU, eval) carrying the case's weights."""
    m = models.CNN_potes_TS(4, 2, "PhysioNet", sig_len=c.T).eval()
    c1, c2 = m.cnn1[0][0], m.cnn1[1][0]
    with torch.no_grad():
        for p, v in zip((c1.weight, c1.bias, c2.weight, c2.bias), (c.w1, c.b1, c.w2, c.b2)):
            p.copy_(v)
    return m.cnn1, [c1.weight, c1.bias, c2.weight, c2.bias]


def _through_torch(c):
    cnn1, params = _module_with(c)
    x = c.x.clone().requires_grad_(True)
    h = cnn1(x.unsqueeze(1))
    g = torch.autograd.grad((h * c.r).sum(), [x] + params)
    return h.detach(), g[0], torch.cat([t.reshape(-1) for t in g[1:]])


@pytest.mark.parametrize("T", [14, 23, 498, 1017])
def test_stack_ref_matches_torch_modules(T):
    """Random data, the limits of tests/test_potes_gpu.py (torch float32 against the float64
    restatement), and the codes against torch's float64 max-pool indices (no ties in randn data)."""
    c = R.rand_case(3, T)
    assert c.undecidable == 0, f"rand_case(3, {T}, seed={c.seed})"
    h, gx, grads = _through_torch(c)
    assert c.ref.h2.shape == h.shape == (3, 4, c.P2)
    assert c.ref.gx.shape == (3, T) and c.ref.grads.shape == (R.NGRAD,)
    assert torch.allclose(h.double(), c.ref.h2, rtol=1e-4, atol=1e-5)
    assert float((gx.double() - c.ref.gx).abs().max()) <= 1e-4 * float(c.ref.gx.abs().max())
    lo = 0
    for n in (40, 8, 160, 4):
        a, b = grads[lo:lo + n].double(), c.ref.grads[lo:lo + n]
        assert float((a - b).abs().max()) <= 2e-4 * float(b.abs().max())
        lo += n
    for z, code, P in ((c.ref.z1, c.ref.code1, c.P1), (c.ref.z2, c.ref.code2, c.P2)):
        v, idx = torch.nn.functional.max_pool1d(torch.relu(z), 2, return_indices=True)
        want = torch.where(v > 0, idx - 2 * torch.arange(P) + 1, torch.zeros((), dtype=torch.long))
        assert torch.equal(code.long(), want)
        assert 0.05 < float((code == 1).double().mean()) and 0.05 < float((code == 2).double().mean())


@pytest.mark.parametrize("N,T", [(3, 1017), (3, 14), (5, 502)])
def test_integer_case_is_exact_in_float32(N, T):
    """The claim the GPU suite rests on: for int_case data torch float32 (its own summation order,
    its own max-pool and ReLU backward: first maximum wins, dead at exactly 0) equals the float64
    restatement bit for bit — h2 and all five gradients — while ties and exact zeros are common."""
    c = R.int_case(N, T)
    h, gx, grads = _through_torch(c)
    assert torch.equal(h.double(), c.ref.h2)
    assert torch.equal(gx.double(), c.ref.gx)
    assert torch.equal(grads.double(), c.ref.grads)
    for t in (c.x, c.w1, c.b1, c.w2, c.b2, c.r, c.ref.h2, c.ref.gx, c.ref.grads):
        assert torch.equal(t, t.round())
    assert min(c.ties) >= 0.01 and c.zeros1 >= 0.05
    assert bool((c.ref.code1 == 0).any()) and bool((c.ref.code2 == 0).any())
    assert float(c.ref.grads.abs().max()) < 2 ** 24
    assert R.int_case(N, T) is c                       # one shared reference per shape


def test_tie_and_zero_rule():
    """The rule itself on hand-made pairs: the first maximum wins a tie, exactly 0 is dead."""
    z = torch.tensor([[1., 1., 0., 0., -1., 2., 3., 2., 0., 1., 2., 0., -3., -3., 0., -1.]], dtype=torch.float64)
    a, code = R.route(z, 8)
    assert code.tolist() == [[1, 0, 2, 1, 2, 1, 0, 0]]
    assert a.tolist() == [[1., 0., 2., 3., 1., 2., 0., 0.]]


@pytest.mark.parametrize("res", range(4))
def test_pack_round_trip(res):
    """Both layouts for every residue of P1 and P2 mod 4: round trip, row lengths of
    pcgmix_potes_stack.h, zero codes at every bit position outside the valid range, and the
    positions of single codes written out by hand."""
    g = torch.Generator().manual_seed(res)
    for P in (res + 4, res + 252):
        codes = torch.randint(0, 3, (2, 3, P), generator=g).to(torch.uint8)
        m2, s1 = R.pack_m2(codes, P), R.pack_s1(codes, P)
        assert m2.shape == (2, 3, (P + 3) // 4) and s1.shape == (2, 3, (P >> 2) + 1)
        assert m2.dtype == s1.dtype == torch.uint8
        assert torch.equal(R.unpack_m2(m2, P), codes) and torch.equal(R.unpack_s1(s1, P), codes)
        for p in range(P):
            assert torch.equal((m2[..., p >> 2] >> (2 * (p & 3))) & 3, codes[..., p])
            assert torch.equal((s1[..., (p + 1) >> 2] >> (2 * ((p + 1) & 3))) & 3, codes[..., p])
        assert not bool((s1[..., 0] & 3).any())                               # q = -1
        full = torch.full((2, 3, P), 2, dtype=torch.uint8)
        for p in range(P, 4 * ((P + 3) // 4)):
            assert not bool(((R.pack_m2(full, P)[..., -1] >> (2 * (p & 3))) & 3).any())
        for slot in range(P + 1, 4 * ((P >> 2) + 1)):
            assert not bool(((R.pack_s1(full, P)[..., -1] >> (2 * (slot & 3))) & 3).any())
    one = torch.zeros(1, 6, dtype=torch.uint8)
    one[0, 5] = 2
    assert R.pack_m2(one, 6).tolist() == [[0, 2 << 2]]           # p = 5: byte 1, bits 2..3
    assert R.pack_s1(one, 6).tolist() == [[0, 2 << 4]]           # q = 5: slot 6 = byte 1, bits 4..5


def test_undecidable_counts_near_ties():
    """A decision inside the bound is counted, one far outside is not."""
    w1 = torch.zeros(8, 1, 5)
    w1[:, 0, 1] = 1.0                                   # z1[i] = x[i] + 1 (tap 1 of a pad-1 conv)
    b1, w2, b2 = torch.ones(8), torch.zeros(4, 8, 5), torch.full((4,), -1.0)
    x = torch.tensor([[1.0, 2.0] * 7])
    assert R.undecidable(x, w1, b1, w2, b2) == 0
    x[0, 1] = 1.0 + 2.0 ** -23                          # one float32 ulp from a tie, in all 8 channels
    assert R.undecidable(x, w1, b1, w2, b2) == 8
    x[0, 1], x[0, 0] = -3.0, -1.0 + 2.0 ** -23          # a first candidate alive by one ulp of its terms
    assert R.undecidable(x, w1, b1, w2, b2) == 8


def test_shapes_cover_tile_edges():
    """The shape table of tests/test_potes_edges_gpu.py against the kernels' tile constants."""
    p2 = {R.dims(T)[1] for T in R.EDGE_T}
    tp = R.FWD_TP
    assert {tp - 1, tp, tp + 1, 2 * tp, 2 * tp + 1} <= p2                      # 251, 252, 253, 504, 505
    assert {122, 123, 124, 248, 249} <= p2
    # P2 + 2 crosses a multiple of kBwdTP between 123 and 124, and between 248 and 249
    assert [R.bwd_tiles(T) for T in (498, 502, 998, 1002)] == [1, 2, 2, 3]
    assert {R.IN_NU, R.IN_NU + 1, 2 * R.IN_NU, 2 * R.IN_NU + 1} <= set(R.EDGE_T)      # 496, 497, 992, 993
    assert [R.in_tiles(T) for T in (496, 497, 992, 993)] == [1, 2, 2, 3]
    assert {T % 4 for T in R.EDGE_T} == {0, 1, 2, 3}
    # both forward staging paths (16-byte loads need T % 4 == 0) at a forward tile edge
    for edge in (tp, tp + 1):
        at = {T % 4 == 0 for T in R.EDGE_T if R.dims(T)[1] == edge}
        assert at == {True, False}, edge
    assert min(R.EDGE_T) == 14 and R.dims(14) == (6, 2)
    # odd T with N = 3 rows: rows at odd float offsets (the input gradient's scalar-store branch)
    assert R.EDGE_N == 3 and any(T % 2 for T in R.EDGE_T)
    # the persistent shapes: 2-5 tiles per row in each kernel, so a block crosses tiles and rows
    for tiles in (R.fwd_tiles, R.bwd_tiles, R.in_tiles):
        per_row = [tiles(T) for T in R.PERSIST_T]
        assert max(per_row) <= 5 and sorted(per_row)[1] >= 2, per_row
    assert {R.fwd_tiles(14), R.bwd_tiles(14), R.in_tiles(14)} == {1}          # the cap-crossing shape
