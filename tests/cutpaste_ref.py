"""CPU restatements for the cut-and-paste and 2D cutmix tests (tests/test_cutpaste_cpu.py,
test_cutpaste_gpu.py, test_baselines2d_cpu.py, test_baselines2d_gpu.py): what the kernels of
csrc/pcgmix_cutpaste.hip compute from a plan's tables, in numpy, and the golden files' helpers.
Not a test module."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CUTPASTE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "cutpaste_*.npz")))
CUTOUT2D_FILES = sorted(glob.glob(os.path.join(GOLDEN, "cutout2d_*.npz")))
OWN, PARTNER, ZERO = 0, 1, 2
MAX_OV = 10


def load(path):
    with np.load(path, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g["method"] = str(g["method"])
    g["wav"] = tuple(str(w) for w in g["wav"])
    for k in ("step", "batch_size", "sample_rate", "fired", "same_object", "cut"):
        g[k] = int(g[k])
    return g


def set_np_state(g, which="np_before"):
    tail = g[which + "_tail"]
    np.random.set_state(("MT19937", g[which].astype(np.uint32), int(tail[0]), int(tail[1]), float(tail[2])))


def assert_np_state(g):
    _, key, pos, has_gauss, cached = np.random.get_state()
    tail = g["np_after_tail"]
    assert np.array_equal(key, g["np_after"]) and pos == int(tail[0])
    assert has_gauss == int(tail[1]) and (not has_gauss or cached == tail[2])


def replay_pieces(x, segs, mix, axis, Wo, junctions=None, sig_tab=None):
    """The segment-table contract of pcgmix_piecewise_rows_f32 and pcgmix_cutpaste_rows_f32
    (include/pcgmix_hip.h) in numpy, for all samples at once: y (B, C, F, Wo) from x (B, C, F, W) and
    the (B, 5, 4) table {lo, hi, src, shift} along the columns (axis 0) or along F (axis 1).  A position
    takes the LAST segment whose lo <= p; it is zero before the first lo, at or beyond the last hi, in a
    ZERO segment and where its source position lies outside the input.  junctions (B, 4) with the
    (10, 20) float64 coefficient table: the '(smooth)' window along the columns (W == Wo)."""
    B, C, F, W = x.shape
    n_out, n_in = (Wo, W) if axis == 0 else (F, F)
    rows = np.arange(B)[:, None]
    mix = np.asarray(mix).astype(np.int64)
    m = np.where((mix >= 0) & (mix < B), mix, np.arange(B))
    p = np.arange(n_out)[None, :]
    k = np.zeros((B, n_out), dtype=np.int64)
    for j in range(1, segs.shape[1]):
        k[p >= segs[:, j, 0:1]] = j
    src = np.take_along_axis(segs[:, :, 2], k, 1)
    st = p + np.take_along_axis(segs[:, :, 3], k, 1).astype(np.int64)
    copied = ((src == OWN) | (src == PARTNER)) & (p >= segs[:, 0, 0:1]) & (p < segs[:, -1, 1:2])
    ok = copied & (st >= 0) & (st < n_in)
    who = np.where(src == OWN, rows, m[:, None])
    stc = np.clip(st, 0, n_in - 1)
    if axis == 0:
        y = np.where(ok[:, :, None, None], x[who, :, :, stc], np.float32(0)).transpose(0, 2, 3, 1)
    else:
        y = np.where(ok[:, :, None, None], x[who, :, stc, :], np.float32(0)).transpose(0, 2, 1, 3)
    y = np.ascontiguousarray(y)
    if junctions is not None:
        assert axis == 0 and W == Wo
        c1, c2, ov = (junctions[:, i].astype(np.int64) for i in range(3))
        for j in range(2 * MAX_OV):
            t, sp = c1 - ov + j, c2 - ov + j
            bs = np.nonzero((ov >= 1) & (ov <= MAX_OV) & (j < 2 * ov) & (t >= 0) & (t < W))[0]
            bs = bs[copied[bs, t[bs]]]
            inside = ((sp[bs] >= 0) & (sp[bs] < W))[:, None, None]
            s = sig_tab[ov[bs] - 1, j][:, None, None]
            val = (x[bs, :, :, t[bs]].astype(np.float64) * (1.0 - s)
                   + x[m[bs], :, :, np.clip(sp[bs], 0, W - 1)].astype(np.float64) * s).astype(np.float32)
            y[bs, :, :, t[bs]] = np.where(inside, val, np.float32(0))
    return y


def replay_cutpaste(x, segs, mix, junctions=None, sig_tab=None):
    """pcgmix_cutpaste_rows_f32 in numpy: (B, C, T) float32 from the (B, 5, 4) table, the partners,
    the optional (B, 4) junctions and the (10, 20) float64 coefficient table — the F = 1 case."""
    return replay_pieces(x[:, :, None, :], segs, mix, 0, x.shape[2], junctions, sig_tab)[:, :, 0, :]


def replay_splice(x, frames, mix, off, lam32):
    """The splice of pcgmix_mix_warp_f32 without warp (mixup_keepdur_multidim_tensors): per state
    the shorter length, '(rand)' offset on the longer side; fp32 mul, mul, add."""
    lam = np.float32(lam32)
    oml = np.float32(1) - lam
    y = x.copy()
    T = x.shape[2]
    for b in range(x.shape[0]):
        m = int(mix[b])
        f1, f2 = frames[b], frames[m]
        for k in range(4):
            l1, l2 = int(f1[k + 1] - f1[k]), int(f2[k + 1] - f2[k])
            gap = l2 - l1
            o = int(off[b, k]) if off is not None else 0
            o = min(max(o, 0), abs(gap))
            a = int(f1[k]) + (o if gap < 0 else 0)
            s = int(f2[k]) + (o if gap > 0 else 0)
            n = min(l1, l2, T - a, T - s)
            if a < 0 or s < 0 or n <= 0:
                continue
            y[b, :, a:a + n] = x[b, :, a:a + n] * lam + x[m, :, s:s + n] * oml
    return y


def replay_mixscale(x, frames, mix, off, lam32, row):
    """pcgmix_mix_scale_f32: float(double(splice) * row[t])."""
    return (replay_splice(x, frames, mix, off, lam32).astype(np.float64) * row[None, None, :]).astype(np.float32)


def replay_spans(x, spans, rows):
    """cutout: spans (B*rows, 2) zeroed on the (B*rows, C/rows, T) view."""
    B, C, T = x.shape
    y = x.copy().reshape(B * rows, C // rows, T)
    for r, (s0, s1) in enumerate(spans):
        y[r, :, max(int(s0), 0):min(int(s1), T)] = 0
    return y.reshape(B, C, T)


def replay_rects(x, rect):
    y = x.copy()
    for b, (r0, r1, c0, c1) in enumerate(rect):
        y[b, :, max(r0, 0):r1, max(c0, 0):c1] = 0
    return y


def replay_plan(plan, x, frames, sig_tab):
    """The output a fired ``hostprep.cutpaste_plan`` defines for the input ``x``."""
    kind = plan.kind
    if kind == "cutpaste":
        return replay_cutpaste(x, plan.segs, plan.mix, plan.junctions, sig_tab)
    if kind == "mixscale":
        return replay_mixscale(x, frames, plan.mix, plan.rand_off, plan.lam32, plan.scale_row)
    if kind == "cutout":
        return replay_spans(x, plan.spans, plan.span_rows)
    if kind == "cutout2d":
        return replay_rects(x, plan.zero_rect)
    raise AssertionError(kind)
