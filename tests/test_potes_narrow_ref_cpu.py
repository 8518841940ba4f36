"""tests/potes_narrow_ref.py pinned on the CPU: against torch float64 autograd, its tie rule against a
scalar loop, the routing-byte layouts against a byte-at-a-time statement, what its shape table
covers, that every integer and random case of the table builds at the first seed that can, and the
library's size helpers against the formulas.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib

import potes_narrow_ref as R

WIDTH_IDS = [f"{a}-{b}" for a, b in R.WIDTHS]
ALL_INT = R.EDGE + R.LOOP + [R.LIMIT]
ALL_RAND = R.EDGE + R.LOOP[1:]
TABLE_T = R.SHORT_T + R.EDGE_T


# ---- against torch ------------------------------------------------------------------------------
def _through_torch(c, dtype):
    x = c.x.to(dtype).clone().requires_grad_(True)
    p = [t.to(dtype).clone().requires_grad_(True) for t in (c.w1, c.b1, c.w2, c.b2)]
    a1, i1 = F.max_pool1d(torch.relu(F.conv1d(x[:, None, :], p[0], p[1], padding=1)), 2, return_indices=True)
    h2, i2 = F.max_pool1d(torch.relu(F.conv1d(a1, p[2], p[3], padding=1)), 2, return_indices=True)
    g = torch.autograd.grad((h2 * c.r.to(dtype)).sum(), [x] + p)
    codes = [torch.where(v > 0, i - 2 * torch.arange(v.shape[-1]) + 1, torch.zeros((), dtype=torch.long))
             for v, i in ((a1.detach(), i1), (h2.detach(), i2))]
    return h2.detach(), g[0], torch.cat([t.reshape(-1) for t in g[1:]]), codes


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("N,T", [(16, 14), (16, 23), (3, 1027), (3, 1036)])
@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_stack_ref_matches_float64_autograd(widths, N, T):
    """conv1d -> relu -> max_pool1d, twice, in torch float64 on tie-free random data: values and all
    gradients <= 1e-12 relative, codes those of max_pool1d's indices plus the ReLU sign."""
    c = R.rand_case(widths, N, T)
    C1, C2 = widths
    assert c.undecidable == 0
    h, gx, grads, codes = _through_torch(c, torch.float64)
    assert c.ref.h2.shape == h.shape == (N, C2, c.P2) and c.ref.gx.shape == (N, T)
    assert c.ref.grads.shape == (R.grad_len(C1, C2),) == (5 * C1 + C1 + 5 * C1 * C2 + C2,)
    assert _rel(c.ref.h2, h) <= 1e-12 and _rel(c.ref.gx, gx) <= 1e-12
    lo = 0
    for _, n in R.grad_parts(C1, C2):
        assert _rel(c.ref.grads[lo:lo + n], grads[lo:lo + n]) <= 1e-12
        lo += n
    assert lo == R.grad_len(C1, C2)
    assert c.ref.code1.shape == (N, C1, c.P1) and c.ref.code2.shape == (N, C2, c.P2)
    assert torch.equal(c.ref.code1.long(), codes[0]) and torch.equal(c.ref.code2.long(), codes[1])
    assert torch.equal(c.m2, R.pack_m2(c.ref.code2, c.P2)) and torch.equal(c.s1, R.pack_s1(c.ref.code1, c.P1))
    assert c.e2.shape == c.ref.h2.shape and float(c.e2.min()) > 0


@pytest.mark.parametrize("N,T", [(16, 14), (3, 1028), (300, 14)])
@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_integer_case_is_exact_in_float32(widths, N, T):
    """What the GPU suite rests on: on int_case data torch float32 (its own summation order, its own
    max-pool and ReLU backward: first maximum wins, dead at exactly 0) equals the float64
    restatement bit for bit, and the data are integers."""
    c = R.int_case(widths, N, T)
    h, gx, grads, codes = _through_torch(c, torch.float32)
    assert torch.equal(h.double(), c.ref.h2) and torch.equal(gx.double(), c.ref.gx)
    assert torch.equal(grads.double(), c.ref.grads)
    assert torch.equal(c.ref.code1.long(), codes[0]) and torch.equal(c.ref.code2.long(), codes[1])
    for t in (c.x, c.w1, c.b1, c.w2, c.b2, c.r, c.ref.h2, c.ref.gx, c.ref.grads):
        assert torch.equal(t, t.round())
    assert R.int_case(widths, N, T) is c                 # one shared reference per shape


# ---- the tie rule, without route ----------------------------------------------------------------
def _scalar_stack(c, last_wins=False):
    """The stack and its backward as Python loops over lists, one row at a time.  last_wins flips the
    tie rule (>= for >).  Returns (h2, code1, code2, gx, grads) as nested lists."""
    C1, C2, T, P1, P2 = c.C1, c.C2, c.T, c.P1, c.P2
    w1, b1, w2, b2 = c.w1.tolist(), c.b1.tolist(), c.w2.tolist(), c.b2.tolist()

    def pool(za, zb):
        if zb > 0 and (zb >= za if last_wins else zb > za):
            return zb, 2
        return (za, 1) if za > 0 else (0.0, 0)

    gw1 = [[0.0] * 5 for _ in range(C1)]
    gb1 = [0.0] * C1
    gw2 = [[[0.0] * 5 for _ in range(C1)] for _ in range(C2)]
    gb2 = [0.0] * C2
    H, CODE1, CODE2, GX = [], [], [], []
    for xrow, rrow in zip(c.x.tolist(), c.r.tolist()):
        xp = [0.0] + xrow + [0.0]
        a1p, code1 = [], []
        for ch in range(C1):
            z = [b1[ch] + sum(w1[ch][0][k] * xp[i + k] for k in range(5)) for i in range(T - 2)]
            pairs = [pool(z[2 * q], z[2 * q + 1]) for q in range(P1)]
            a1p.append([0.0] + [v for v, _ in pairs] + [0.0])
            code1.append([s for _, s in pairs])
        h, code2 = [], []
        ga1p = [[0.0] * (P1 + 2) for _ in range(C1)]
        for co in range(C2):
            z = [b2[co] + sum(w2[co][ci][k] * a1p[ci][j + k] for ci in range(C1) for k in range(5))
                 for j in range(P1 - 2)]
            pairs = [pool(z[2 * p], z[2 * p + 1]) for p in range(P2)]
            h.append([v for v, _ in pairs])
            code2.append([s for _, s in pairs])
            for p, (_, s) in enumerate(pairs):
                if s:
                    j, g = 2 * p + s - 1, rrow[co][p]
                    gb2[co] += g
                    for ci in range(C1):
                        for k in range(5):
                            gw2[co][ci][k] += g * a1p[ci][j + k]
                            ga1p[ci][j + k] += w2[co][ci][k] * g
        gxp = [0.0] * (T + 2)
        for ch in range(C1):
            for q, s in enumerate(code1[ch]):
                if s:
                    i, g = 2 * q + s - 1, ga1p[ch][q + 1]
                    gb1[ch] += g
                    for k in range(5):
                        gw1[ch][k] += g * xp[i + k]
                        gxp[i + k] += w1[ch][0][k] * g
        H.append(h); CODE1.append(code1); CODE2.append(code2); GX.append(gxp[1:T + 1])
    flat = [v for row in gw1 for v in row] + gb1 + [v for co in gw2 for row in co for v in row] + gb2
    return H, CODE1, CODE2, GX, flat


@pytest.mark.parametrize("T", [17, 23])
@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_tie_rule_against_a_scalar_loop(widths, T):
    """A statement of the stack that shares nothing with ``route``: same codes, values and gradients
    on short integer rows — and with the rule flipped to 'last maximum wins' the codes of both
    layers, the input gradient and the weight gradients of those rows change (h2 cannot: tied
    candidates are equal), i.e. the integer cases tell the two rules apart."""
    c = R.int_case(widths, R.SHORT_N, T)
    h, code1, code2, gx, grads = _scalar_stack(c)
    assert c.ref.h2.tolist() == h and c.ref.gx.tolist() == gx and c.ref.grads.tolist() == grads
    assert c.ref.code1.tolist() == code1 and c.ref.code2.tolist() == code2
    h_l, code1_l, code2_l, gx_l, grads_l = _scalar_stack(c, last_wins=True)
    assert code1_l != code1 and code2_l != code2
    assert gx_l != gx and grads_l != grads


def test_tie_and_zero_rule_by_hand():
    z = torch.tensor([[1., 1., 0., 0., -1., 2., 3., 2., 0., 1., 2., 0., -3., -3., 0., -1.]], dtype=torch.float64)
    a, code = R.route(z, 8)
    assert code.tolist() == [[1, 0, 2, 1, 2, 1, 0, 0]]
    assert a.tolist() == [[1., 0., 2., 3., 1., 2., 0., 0.]]


# ---- routing bytes ------------------------------------------------------------------------------
def _bytes_one_at_a_time(codes, nbytes, first):
    """The layout comment of csrc/pcgmix_potes_stack.h, one byte and one slot at a time: slot s of
    byte b holds, in bits 2s..2s+1, the code of position 4b + s + first — code 0 where that position
    does not exist.  m2: first = 0 (output p in bits 2*(p&3) of byte p>>2); s1: first = -1 (position q
    in bits 2*((q+1)&3) of byte (q+1)>>2)."""
    out = []
    for b in range(nbytes):
        byte = 0
        for s in range(4):
            pos = 4 * b + s + first
            byte |= (codes[pos] if 0 <= pos < len(codes) else 0) << (2 * s)
        out.append(byte)
    return out


@pytest.mark.parametrize("T", R.SHORT_T + [1027, 1028, 1032, 1034])
def test_pack_against_the_layout_comment(T):
    """pack_m2 / pack_s1 on the codes of an integer case: the bytes of the one-at-a-time statement,
    the row lengths of pcgmix_potes_stack.h, a round trip, code 0 in slot q = -1 and in the unused
    tail slots (with every real code non-zero, so nothing hides them)."""
    widths = (2, 1)
    c = R.int_case(widths, R.SHORT_N if T <= 23 else R.EDGE_N, T)
    P1, P2 = c.P1, c.P2
    assert c.m2.shape == (c.N, 1, (P2 + 3) // 4) == (c.N, 1, R.m2row(T))
    assert c.s1.shape == (c.N, 2, (P1 >> 2) + 1) == (c.N, 2, R.s1row(T))
    assert c.m2.dtype == c.s1.dtype == torch.uint8
    for n in range(c.N):
        assert c.m2[n, 0].tolist() == _bytes_one_at_a_time(c.ref.code2[n, 0].tolist(), R.m2row(T), 0)
        for ch in range(2):
            assert c.s1[n, ch].tolist() == _bytes_one_at_a_time(c.ref.code1[n, ch].tolist(), R.s1row(T), -1)
    assert torch.equal(R.unpack_m2(c.m2, P2), c.ref.code2) and torch.equal(R.unpack_s1(c.s1, P1), c.ref.code1)
    m2 = R.pack_m2(torch.full((1, P2), 2, dtype=torch.uint8), P2)[0].tolist()
    s1 = R.pack_s1(torch.full((1, P1), 2, dtype=torch.uint8), P1)[0].tolist()
    assert m2 == _bytes_one_at_a_time([2] * P2, R.m2row(T), 0)
    assert s1 == _bytes_one_at_a_time([2] * P1, R.s1row(T), -1)
    assert s1[0] & 3 == 0                                                           # q = -1
    assert [(m2[-1] >> (2 * s)) & 3 for s in range(4)] == [2 if 4 * (len(m2) - 1) + s < P2 else 0 for s in range(4)]
    assert [(s1[-1] >> (2 * s)) & 3 for s in range(4)] == \
        [2 if 0 <= 4 * (len(s1) - 1) + s - 1 < P1 else 0 for s in range(4)]


# ---- the shape table ----------------------------------------------------------------------------
def test_shapes_cover_tile_edges():
    """Every count recomputed from the kernel's constants, and the transitions the table names."""
    assert (R.NAR_TP, R.THREADS, R.IN_TU, R.BWD_CAP, R.MAX_N) == (256, 256, 1024, 1024, 65535)
    fs = {T: R.fwd_tiles(T, True) for T in TABLE_T}
    f0 = {T: R.fwd_tiles(T, False) for T in TABLE_T}
    bw = {T: R.bwd_tiles(T) for T in TABLE_T}
    ib = {T: R.in_blocks(T) for T in TABLE_T}
    p1 = {T: R.dims(T)[0] for T in TABLE_T}
    p2 = {T: R.dims(T)[1] for T in TABLE_T}
    for T in TABLE_T:           # the formulas of fwd_tiles / bwd_tiles, written out
        assert fs[T] == -(-(2 * ((p1[T] >> 2) + 1) - 1) // 256) and f0[T] == -(-p2[T] // 256)
        assert bw[T] == -(-((p1[T] + 1) // 2) // 256) and ib[T] == -(-T // 1024)
        assert f0[T] <= fs[T]                        # 2 * (P1 / 4) >= P2: the s1 walk covers every output
    assert min(TABLE_T) == R.MIN_T == 14 and R.dims(14) == (6, 2)
    assert all(fs[T] == f0[T] == bw[T] == ib[T] == 1 for T in R.SHORT_T)
    # input gradient 1 -> 2 -> 3 blocks
    assert [ib[T] for T in (1024, 1025, 2048, 2049)] == [1, 2, 2, 3]
    # forward with s1: P1 = 511 is the last row whose 2 * s1row - 1 = 255 even outputs fit one tile
    assert p1[1024] == p1[1025] == 511 and p1[1026] == 512
    assert [fs[T] for T in (1025, 1026)] == [1, 2] and 2 * R.s1row(1026) - 1 == 257 and f0[1026] == 1 and p2[1026] == 255
    assert [fs[T] for T in (2049, 2056)] == [2, 3]
    # forward without s1: P2 = 255, 256 | 257 and 512 | 513
    assert [p2[T] for T in (1027, 1028, 1032, 1034, 1036)] == [255, 255, 256, 257, 257]
    assert [f0[T] for T in (1027, 1028, 1032, 1034, 1036)] == [1, 1, 1, 2, 2]
    assert [p2[T] for T in (2056, 2058, 2060)] == [512, 513, 513] and [f0[T] for T in (2056, 2058, 2060)] == [2, 3, 3]
    # weight gradient: (P1 + 1) // 2 = 256 | 257, and a third tile
    assert [(p1[T] + 1) // 2 for T in (1027, 1028)] == [256, 257] and [bw[T] for T in (1027, 1028)] == [1, 2]
    assert [bw[T] for T in (2049, 2056)] == [2, 3]
    # residues: all four among the short rows and among the long ones
    assert {T % 4 for T in R.SHORT_T} == {T % 4 for T in R.EDGE_T} == {0, 1, 2, 3}
    # the paths chosen by T % 4 (stage_tile in the forward and the weight gradient, the float4 store of
    # the input gradient): every tile / block count a kernel reaches, it reaches at an aligned length
    # AND at another one
    for name, count in (("forward with s1", fs), ("forward without s1", f0), ("weight gradient", bw),
                        ("input gradient", ib)):
        for n in set(count.values()):
            assert {T % 4 == 0 for T in TABLE_T if count[T] == n} == {True, False}, (name, n)
    # ... and the named edges P2 = 255 and 257, 513 in both
    for edge in (255, 257, 513):
        assert {T % 4 == 0 for T in TABLE_T if p2[T] == edge} == {True, False}, edge
    assert [T for T in TABLE_T if T % 4 == 0] == [16, 1024, 1028, 1032, 1036, 2048, 2056, 2060]
    # rows: 16 up to T = 23, else 3, so that odd T puts rows at odd float offsets
    assert all(N == (R.SHORT_N if T <= 23 else R.EDGE_N) for N, T in R.EDGE) and [T for _, T in R.EDGE] == TABLE_T
    assert R.EDGE_N % 2 == 1 and any(T % 2 for T in R.EDGE_T)
    # the persistent loop, the reduction, the limit
    assert [N * bw.get(T, R.bwd_tiles(T)) for N, T in R.LOOP] == [300, 1030, 1040]
    assert [R.bwd_blocks(N, T) for N, T in R.LOOP] == [300, 1024, 1024]
    assert R.THREADS < 300 < 2 * R.THREADS and 300 - R.THREADS == 44          # threads 0..43 take two rows
    assert R.bwd_tiles(1028) == 2 and 1040 - R.BWD_CAP == 16                     # blocks 0..15: a second item
    # item = row * tiles + tile: block g's second item g + 1024 is a tile of row g / 2 + 512
    assert [divmod(g + R.BWD_CAP, 2) for g in (0, 15)] == [(512, 0), (519, 1)] and 519 == 520 - 1
    assert R.LIMIT == (65535, 14) and R.bwd_blocks(*R.LIMIT) == R.BWD_CAP
    assert max(R.bwd_blocks(N, T) for N, T in R.EDGE) == R.SHORT_N < R.THREADS     # no edge case loops anywhere


# ---- the cases build, at the first seed that can ------------------------------------------------
def _passes(c):
    return max(float(v) for v in R.abs_bounds(c).values()) < 2 ** 24 and R.degenerate(c) is None


@pytest.mark.parametrize("N,T", ALL_INT)
@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_every_integer_case_builds_at_the_first_seed(widths, N, T):
    """int_case's own assertions (every sum of |addends| < 2**24; ties, all three codes, no zero
    gradient, no zero bias, gx alive) hold at the table's seed and at no smaller one."""
    c = R.int_case(widths, N, T)
    assert c.seed == R.INT_SEED.get((widths, N, T), 0)
    assert set(c.bounds) == {"z1", "z2", "ga1", "dx", "gw1", "gb1", "gw2", "gb2"}
    assert max(float(v) for v in c.bounds.values()) < 2 ** 24
    assert float(c.ref.grads.abs().max()) <= max(float(c.bounds[k]) for k in ("gw1", "gb1", "gw2", "gb2"))
    for s in range(c.seed):
        _, _, b1, _, b2, _ = R.int_data(widths, N, T, s)
        if bool((b1 != 0).all()) and bool((b2 != 0).all()):          # else refused before any arithmetic
            assert not _passes(R.make_int(widths, N, T, s)), f"seed {s} passes as well"


def test_seed_tables_name_only_table_cases():
    assert set(R.INT_SEED) <= {(w, N, T) for w in R.WIDTHS for N, T in ALL_INT}
    assert set(R.RAND_SEED) <= {(w, N, T) for w in R.WIDTHS for N, T in ALL_RAND}
    assert all(s > 0 for s in list(R.INT_SEED.values()) + list(R.RAND_SEED.values()))


def test_degenerate_names_each_failure():
    """The judge itself: the conditions fire on data made to miss them."""
    c = R.make_int((2, 1), R.SHORT_N, 23, R.INT_SEED[((2, 1), R.SHORT_N, 23)])
    assert R.degenerate(c) is None
    dead = R._case((2, 1), c.x, c.w1 * 0, c.b1 * 0 - 1, c.w2, c.b2, c.r, seed=None)     # z1 = -1 everywhere
    assert "layer 1" in R.degenerate(dead)
    tie_free = R.rand_case((2, 1), R.SHORT_N, 23)
    assert "ties" in R.degenerate(tie_free)
    big = R._case((2, 1), c.x * 2.0 ** 22, c.w1, c.b1, c.w2, c.b2, c.r, seed=None)
    assert max(float(v) for v in R.abs_bounds(big).values()) >= 2 ** 24


@pytest.mark.parametrize("N,T", ALL_RAND)
@pytest.mark.parametrize("widths", R.WIDTHS, ids=WIDTH_IDS)
def test_every_random_case_is_decidable_at_the_first_seed(widths, N, T):
    c = R.rand_case(widths, N, T)
    assert c.seed == R.RAND_SEED.get((widths, N, T), 0) and c.undecidable == 0
    for s in range(c.seed):
        assert R.rand_case(widths, N, T, s).undecidable > 0, f"seed {s} is decidable as well"


# ---- the error bound ------------------------------------------------------------------------------
def test_chain_factors():
    """n terms in any order: n roundings per term, (1 + u)^n - 1 < (n + 1) u.  Layer 1 has n = 6 for
    every width (the 7 of potes_ref.undecidable); layer 2 has n = 5 C1 + 1: 7 and 12 here.  The wide
    stack's hard-wired 43 for n = 41 is one above the rule, so it stays a bound."""
    assert R.chain_factor(6) == 7
    assert [R.chain_factor(5 * C1 + 1) for C1, _ in R.WIDTHS] == [7, 12]
    assert R.chain_factor(41) == 42 <= 43
    u = 2.0 ** -24
    for n in (6, 11, 41):
        assert (1 + u) ** n - 1 < R.chain_factor(n) * u
    # the formulas on data whose sums are known: x = 1, every weight and bias 1
    for C1 in (1, 2):
        d = R.decisions(torch.ones(1, 40), torch.ones(C1, 1, 5), torch.ones(C1), torch.ones(1, C1, 5), torch.ones(1))
        assert float(d.e1[0, 0, 10]) == 7 * u * 6                              # z1 = 6 inside the row
        z2 = 5 * C1 * 6 + 1
        want = R.chain_factor(5 * C1 + 1) * u * z2 + 5 * C1 * (7 * u * 6)
        assert abs(float(d.e2[0, 0, 5]) - want) <= 1e-12 * want and abs(float(d.e_h2[0, 0, 3]) - want) <= 1e-12 * want
        assert d.undecidable > 0                       # constant rows: every pair is a tie


@pytest.mark.parametrize("C1", [1, 2])
def test_decisions_count_near_ties(C1):
    """A decision inside the bound is counted, one far outside is not."""
    w1 = torch.zeros(C1, 1, 5)
    w1[:, 0, 1] = 1.0                                   # z1[i] = x[i] + 1 (tap 1 of a pad-1 conv)
    b1, w2, b2 = torch.ones(C1), torch.zeros(1, C1, 5), torch.full((1,), -1.0)
    x = torch.tensor([[1.0, 2.0] * 7])
    assert R.decisions(x, w1, b1, w2, b2).undecidable == 0
    x[0, 1] = 1.0 + 2.0 ** -23                          # one float32 ulp from a tie, in every channel
    assert R.decisions(x, w1, b1, w2, b2).undecidable == C1
    x[0, 1], x[0, 0] = -3.0, -1.0 + 2.0 ** -23          # a first candidate alive by one ulp of its terms
    assert R.decisions(x, w1, b1, w2, b2).undecidable == C1


# ---- the library's size helpers, no device needed ---------------------------------------------------
def test_helpers_match_the_formulas():
    lib = _lib.load()
    for C1, C2 in R.WIDTHS:
        assert lib.pcgmix_potes_narrow_supported(C1, C2) == 1
        assert lib.pcgmix_potes_narrow_grad_len(C1, C2) == R.grad_len(C1, C2) == 5 * C1 + C1 + 5 * C1 * C2 + C2
        for N, T in ALL_INT:
            assert lib.pcgmix_potes_narrow_bwd_blocks(N, T, C1, C2) == min(N * R.bwd_tiles(T), 1024)
            assert lib.pcgmix_potes_narrow_mask_bytes(N, T, C1, C2, 2) == N * C2 * R.m2row(T)
            assert lib.pcgmix_potes_narrow_mask_bytes(N, T, C1, C2, 1) == N * C1 * R.s1row(T)
            assert lib.pcgmix_potes_narrow_mask_bytes(N, T, C1, C2, 0) == 0
        for N, T in ((0, 64), (65536, 64), (4, 13)):
            assert lib.pcgmix_potes_narrow_bwd_blocks(N, T, C1, C2) == 0
            assert lib.pcgmix_potes_narrow_mask_bytes(N, T, C1, C2, 1) == 0
            assert lib.pcgmix_potes_narrow_mask_bytes(N, T, C1, C2, 2) == 0
    for C1, C2 in ((3, 2), (8, 4)):
        assert lib.pcgmix_potes_narrow_supported(C1, C2) == 0 and lib.pcgmix_potes_narrow_grad_len(C1, C2) == 0
        assert lib.pcgmix_potes_narrow_bwd_blocks(4, 64, C1, C2) == 0
        assert lib.pcgmix_potes_narrow_mask_bytes(4, 64, C1, C2, 1) == 0
        assert lib.pcgmix_potes_narrow_mask_bytes(4, 64, C1, C2, 2) == 0
