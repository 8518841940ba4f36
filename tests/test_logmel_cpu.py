"""Host-side pins of the log-mel front end (no GPU): the high-precision restatement of
tests/logmel_ref.py against oracle.logmel / oracle.logmel_recording on every input class and shape
the GPU tests use, the library's constant tables against oracle.mel_filterbank, and the LDS plan of
one block (pcgmix_logmel_lds_layout) over the same shapes."""
import ctypes

import numpy as np
import pytest

import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib
from oracle import pcgmix_oracle as O

import logmel_ref as R

# The two CPU restatements may differ by a tenth of the 1e-4 the GPU is held to, so that they
# cannot use up that budget between them.
REF_TOL = 1e-5
PADS = ["constant", "reflect"]


def _basis(cfg):
    sr, n_fft, hop, n_mels, fmin, fmax, T, W = cfg
    return O.mel_filterbank(float(sr), n_fft, n_mels, fmin, fmax)


@pytest.mark.parametrize("pad_mode", PADS)
@pytest.mark.parametrize("cls", R.CLASSES)
@pytest.mark.parametrize("sr,T", [(2000, 5000), (1000, 2500)])
def test_reference_agrees_with_oracle_per_class(sr, T, cls, pad_mode):
    n_fft, hop = 4 * int(sr * 2.2 / 128), int(sr * 2.2 / 128)
    x, frames = R.make_batch([cls] * 2, T, sr, seed=3)
    basis = O.mel_filterbank(float(sr), n_fft, 128, 25.0, 1000.0)
    ref, fs, info = R.logmel(x, frames, basis, n_fft=n_fft, hop=hop, pad_mode=pad_mode)
    if sr == 2000:
        R.assert_engages(cls, info, 128)             # the inputs do what the GPU tests rely on
    orc, fs_o = O.logmel(x, frames, n_fft=n_fft, hop=hop, sr=float(sr), pad_mode=pad_mode)
    assert np.array_equal(fs, fs_o)
    err = np.abs(ref - orc).max()
    assert err <= REF_TOL, err


@pytest.mark.parametrize("pad_mode", PADS)
@pytest.mark.parametrize("cfg", R.SWEEP, ids=R.sweep_id)
def test_reference_agrees_with_oracle_over_the_sweep(cfg, pad_mode):
    sr, n_fft, hop, n_mels, fmin, fmax, T, W = cfg
    x, frames = R.make_batch(R.CLASSES, T, sr, seed=1)
    frames[0, 4], frames[1, 4] = 0, T                      # nothing kept / everything kept
    ref, fs, _ = R.logmel(x, frames, _basis(cfg), n_fft=n_fft, hop=hop, W=W, pad_mode=pad_mode)
    orc, fs_o = O.logmel(x, frames, n_fft=n_fft, hop=hop, n_mels=n_mels, fmin=fmin, fmax=fmax,
                         sr=float(sr), W=W, pad_mode=pad_mode)
    assert np.array_equal(fs, fs_o)
    assert (ref[0] == 0).all() and fs[1, 4] == 1 + T // hop
    err = np.abs(ref - orc).max()
    assert err <= REF_TOL, err


@pytest.mark.parametrize("pad_mode", PADS)
@pytest.mark.parametrize("kind,sr,W", [("edges", 2000, 128), ("edges", 2000, 100), ("edges", 1000, 128),
                                       ("many", 2000, 128)])
def test_reference_agrees_with_oracle_per_recording(kind, sr, W, pad_mode):
    hop = int(sr * 2.2 / 128)
    n_fft = 4 * hop
    basis = O.mel_filterbank(float(sr), n_fft, 128, 25.0, 1000.0)
    ys, bs, st = R.make_recordings(kind, sr, hop, 128, W, seed=4)
    worst = 0.0
    for y, b, s in zip(ys[:40], bs, st):
        ref, rel, _ = R.logmel_recording(y, b, s, basis, n_fft=n_fft, hop=hop, W=W, pad_mode=pad_mode)
        orc, rel_o = O.logmel_recording(y, b, s, n_fft=n_fft, hop=hop, sr=float(sr), W=W, pad_mode=pad_mode)
        assert np.array_equal(rel, rel_o)
        if len(s):
            worst = max(worst, float(np.abs(ref - orc).max()))
    assert worst <= REF_TOL, worst


def test_round_half_even_columns():
    """The restatement's integer round-half-even against Python's round() of the float quotient
    (what the notebook evaluates), ties included."""
    for n_frames, T in ((148, 5000), (4, 8), (3, 6), (101, 5000), (148, 4997)):
        for f in list(range(0, T + 1, 7)) + [T // 2, T // 4, 3 * T // 4, T]:
            assert R.round_half_even_ratio(f * n_frames, T) == round(f * n_frames / T)
    assert [R.round_half_even_ratio(k, 2) for k in (1, 3, 5, 7)] == [0, 2, 2, 4]


@pytest.mark.parametrize("cfg", R.SWEEP + [R.TOO_LARGE], ids=R.sweep_id)
def test_tables_match_the_oracle_bank(cfg):
    """wts == oracle.mel_filterbank bit for bit as float32 (the sign of a zero weight aside: numpy's
    maximum(0, -0.0) keeps the -0.0 where the ramp ends exactly on a bin, the library stores +0.0;
    either is a zero tap); krange = first / last non-zero bin;
    bin_lo / n_left_used and the transform the tables encode: the invariants of
    test_host_logic.py::test_logmel_tables_are_the_windowed_transform, at every swept shape."""
    sr, n_fft, hop, n_mels, fmin, fmax, T, W = cfg
    tb = R.check_tables_are_the_windowed_transform(float(sr), n_fft, n_mels, fmin, fmax)
    want = _basis(cfg)
    assert want.dtype == np.float32 and np.array_equal((tb["wts"] + np.float32(0)).view(np.uint32), (want + np.float32(0)).view(np.uint32))
    for m in range(n_mels):
        nz = np.flatnonzero(want[m])
        if nz.size:
            assert tuple(tb["krange"][m]) == (nz[0], nz[-1]), m
        else:
            assert tb["krange"][m, 1] < tb["krange"][m, 0], m


def test_the_sweep_reaches_the_table_layouts_it_is_meant_to():
    """Statements about the sweep itself (from the oracle's bank and the table arithmetic alone), so
    that a change of the sweep cannot silently stop covering a kernel branch."""
    seen = {"span": set(), "n_left": set(), "used": set(), "bin_lo": set(), "ksteps": set()}
    by_cfg = {}
    for cfg in R.SWEEP:
        sr, n_fft, hop, n_mels, fmin, fmax, T, W = cfg
        tb = R.check_tables_are_the_windowed_transform(float(sr), n_fft, n_mels, fmin, fmax)
        kr = tb["krange"]
        spans = set((kr[:, 1] - kr[:, 0])[kr[:, 1] >= kr[:, 0]].tolist())
        by_cfg[cfg] = (spans, tb["lay"]["n_left"], tb["n_left_used"], tb["bin_lo"], tb["lay"]["ksteps"])
        seen["span"] |= spans
        seen["n_left"].add(tb["lay"]["n_left"]); seen["used"].add(tb["n_left_used"])
        seen["bin_lo"].add(tb["bin_lo"]); seen["ksteps"].add(tb["lay"]["ksteps"])
    assert {0, 1, 2, 3} <= seen["span"] and max(seen["span"]) >= 6          # 1-tap, 4-tap, global-weights path
    assert {0, 5} <= seen["n_left"] and {0, 1, 2, 4, 5} <= seen["used"] and {0, 2, 10} <= seen["bin_lo"]
    assert {2, 3, 6, 9, 13} <= seen["ksteps"]
    assert max(by_cfg[R.SWEEP[1]][0]) >= 6                                   # n_mels = 16: spans 6-7
    assert 3 in by_cfg[R.SWEEP[0]][0] and {2, 3} <= by_cfg[R.SWEEP[2]][0]    # n_mels = 32, 40
    assert by_cfg[R.SWEEP[6]][1] > 0 and by_cfg[R.SWEEP[6]][2] == 0          # n_fft = 128: rows present, none read
    assert by_cfg[R.SWEEP[9]][1] > 0 and by_cfg[R.SWEEP[9]][2] == 0          # 300-900 Hz likewise
    assert by_cfg[R.SWEEP[7]][1] == 0 and by_cfg[R.SWEEP[8]][1] == 0         # n_fft = 80, 40: no VALU rows
    assert by_cfg[R.SWEEP[3]][2] == 4 and by_cfg[R.SWEEP[5]][2] == 5         # fmin = 0 / n_fft = 140: 4 and 5 rows
    assert by_cfg[R.SWEEP[4]][4] == 9 and by_cfg[R.SWEEP[5]][4] == 9         # the ring at n_fft = 132, 140
    assert any(1024 % c[7] for c in R.SWEEP) and any(c[7] & 3 for c in R.SWEEP)
    assert any(c[2] * 4 != c[1] for c in R.SWEEP) and any(c[7] > 1 + c[6] // c[2] for c in R.SWEEP)


NAMES = ("xrow", "ps", "img", "melw", "left", "win", "part")
LIMIT = 158 * 1024


def _layout(mode, T, n_fft, hop, n_mels, W, used=-1):
    out = np.zeros(20, dtype=np.int32)
    rc = _lib.load().pcgmix_logmel_lds_layout(mode, T, n_fft, hop, n_mels, W, used, out.ctypes.data)
    assert rc == 0, rc
    reg = {n: (int(out[2 * i]), int(out[2 * i + 1])) for i, n in enumerate(NAMES)}
    return reg, dict(total=int(out[14]), part_need=int(out[15]), nfp=int(out[16]), n_left=int(out[17]),
                     accepted=int(out[18]), limit=int(out[19]))


def _check_layout(mode, T, n_fft, hop, n_mels, W):
    reg, info = _layout(mode, T, n_fft, hop, n_mels, W)
    assert info["limit"] == LIMIT and info["accepted"] == int(info["total"] <= LIMIT)
    if info["total"] == np.iinfo(np.int32).max:
        return reg, info
    lay = R.mel_table_layout(n_fft, n_mels)
    n_frames = 1 + T // hop if mode == 0 else _lib.load().pcgmix_logmel_tile_frames()
    nfp = -(-n_frames // 32) * 32
    assert info["nfp"] == nfp and info["n_left"] == lay["n_left"]
    # what each region has to hold, from the kernel's indexing
    m_tiles = max(2 * lay["tpp"], -(-lay["n_bins"] // 16))
    assert reg["xrow"][1] >= ((nfp - 1) * hop + n_fft + 8) * 4
    assert reg["ps"][1] == m_tiles * 16 * nfp * 4
    assert reg["img"][1] == (n_mels * W * 4 if mode == 0 else 0)
    assert reg["melw"][1] == n_mels * 32
    assert reg["left"][1] == lay["n_left"] * (n_fft // 2 + 8) * 16 and reg["win"][1] == (n_fft // 2 + 1) * 8
    overlay = mode == 0 and reg["part"][0] == reg["img"][0]
    spans = sorted((o, o + s, n) for n, (o, s) in reg.items() if s and not (overlay and n == "part"))
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, (an, bn)                               # disjoint
    assert all(o % 4 == 0 for o, _, _ in spans) and reg["left"][0] % 8 == 0 and reg["win"][0] % 8 == 0
    assert reg["part"][0] % 8 == 0
    assert max(e for _, e, _ in spans) <= info["total"]
    if overlay:
        assert reg["part"][1] == reg["img"][1]
    # the partial sums fit, for every number of rows a table can ask for: n_fg wave jobs per k part,
    # at least one part, each job `used` rows x 64 lanes x (re, im) doubles
    n_fg = -(-nfp // 64)
    for used in range(0, lay["n_left"] + 1):
        need = _layout(mode, T, n_fft, hop, n_mels, W, used)[1]["part_need"]
        assert need >= n_fg * used * 1024 and need % (n_fg * 1024) == 0
        assert need <= reg["part"][1], (used, need, reg["part"])
    return reg, info


@pytest.mark.parametrize("cfg", R.SWEEP, ids=R.sweep_id)
def test_lds_layout_over_the_sweep(cfg):
    sr, n_fft, hop, n_mels, fmin, fmax, T, W = cfg
    reg, info = _check_layout(0, T, n_fft, hop, n_mels, W)
    assert info["accepted"] == 1, info                           # every swept shape is launched
    _check_layout(1, 0, n_fft, hop, n_mels, W)


def test_lds_layout_small_image_gets_its_own_partial_sums():
    """n_fft = 136, T = 5000, 32 x 32: the 4096-byte image cannot hold one k part of the five VALU
    rows of three 64-frame groups (15360 bytes) — they used to be written over it regardless, into
    the filter records and coefficients behind it."""
    reg, info = _check_layout(0, 5000, 136, 34, 32, 32)
    assert reg["img"][1] == 4096 and reg["part"][0] != reg["img"][0] and reg["part"][1] >= 15360
    reg, info = _check_layout(0, 5000, 136, 34, 128, 128)        # the default shape keeps the overlay
    assert reg["part"][0] == reg["img"][0] and info["accepted"] == 1
    for n_mels, W in ((1, 1), (3, 1280), (60, 64), (59, 64), (128, 30), (128, 29)):
        _check_layout(0, 5000, 136, 34, n_mels, W)


def test_lds_layout_refuses_what_does_not_fit():
    sr, n_fft, hop, n_mels, fmin, fmax, T, W = R.TOO_LARGE
    reg, info = _check_layout(0, T, n_fft, hop, n_mels, W)
    assert info["accepted"] == 0 and info["total"] > LIMIT
    for T, n_fft, hop, n_mels, W in ((2 ** 31 - 1, 136, 1, 128, 128), (5000, 136, 34, 2 ** 20, 2 ** 12),
                                     (5000, 2 ** 30, 34, 128, 128), (2 ** 30, 136, 2 ** 30, 2 ** 27, 1)):
        _, info = _check_layout(0, T, n_fft, hop, n_mels, W)     # beyond int arithmetic: still refused
        assert info["accepted"] == 0
    out = np.zeros(20, dtype=np.int32)
    lib = _lib.load()
    for bad in ((2, 5000, 136, 34, 128, 128, -1), (0, 5000, 134, 34, 128, 128, -1), (0, 5000, 0, 34, 128, 128, -1),
                (0, 5000, 136, 0, 128, 128, -1), (0, 5000, 136, 34, 0, 128, -1), (0, 5000, 136, 34, 128, 0, -1),
                (0, 1, 136, 34, 128, 128, -1), (0, 5000, 136, 34, 128, 128, 6)):
        assert lib.pcgmix_logmel_lds_layout(*bad, out.ctypes.data) != 0, bad
    assert lib.pcgmix_logmel_lds_layout(0, 5000, 136, 34, 128, 128, -1, None) != 0


@pytest.mark.parametrize("mode", [0, 1])
def test_lds_layout_random_shapes(mode):
    rs = np.random.RandomState(7 + mode)
    n_acc = 0
    for _ in range(400):
        n_fft = 4 * int(rs.randint(1, 80))
        hop = int(rs.randint(1, n_fft + 1))
        T = int(rs.randint(n_fft // 2 + 1, 9000))
        n_mels, W = int(rs.randint(1, 200)), int(rs.randint(1, 200))
        n_acc += _check_layout(mode, T, n_fft, hop, n_mels, W)[1]["accepted"]
    assert 50 < n_acc
