"""High-precision restatement of the log-mel front end for tests/test_logmel_cpu.py and
tests/test_logmel_gpu.py, and the inputs both use.  Not a test module.

It shares no code with oracle.logmel: the transform is a direct DFT in np.longdouble (no FFT, no
complex64 rounding), the mel projection, dB, reference, clip and normalisation are float64, the
padding and the round-half-even column boundaries are written out here.  Only the filter bank may
come from outside (``basis``): oracle.mel_filterbank, which tests/test_logmel_cpu.py pins against
the library's table on its own.
"""
import numpy as np

MEAN = -59.606563568115234
STD = 15.96771240234375
AMIN = 1e-10
TOP_DB = 80.0

LD = np.longdouble


def round_half_even_ratio(num: int, den: int) -> int:
    """round(num / den) for integers, ties to even, without a floating-point quotient."""
    q, r = divmod(int(num), int(den))
    if 2 * r > den or (2 * r == den and (q & 1)):
        q += 1
    return q


def columns(frames_row, n_frames: int, sig_len: int):
    return [round_half_even_ratio(int(f) * n_frames, sig_len) for f in frames_row]


def padded(y, pad: int, pad_mode: str):
    y = np.asarray(y, dtype=LD)
    n = len(y)
    out = np.zeros(n + 2 * pad, dtype=LD)
    out[pad:pad + n] = y
    if pad_mode == "reflect":                       # the edge sample itself is not repeated
        for i in range(1, pad + 1):
            out[pad - i] = y[i]
            out[pad + n - 1 + i] = y[n - 1 - i]
    elif pad_mode != "constant":
        raise ValueError(pad_mode)
    return out


_DFT = {}


def _dft(n_fft):
    if n_fft not in _DFT:
        k = np.arange(n_fft // 2 + 1)[:, None]
        n = np.arange(n_fft)[None, :]
        ang = (2 * np.arctan2(LD(0), LD(-1))) * ((k * n) % n_fft).astype(LD) / LD(n_fft)   # 2 pi (kn mod N)/N
        win = LD(0.5) - LD(0.5) * np.cos(2 * np.arctan2(LD(0), LD(-1)) * np.arange(n_fft).astype(LD) / LD(n_fft))
        _DFT[n_fft] = (np.cos(ang) * win[None, :], -np.sin(ang) * win[None, :])
    return _DFT[n_fft]


def mel_power(y, n_fft, hop, basis, pad_mode):
    """Centred frames, periodic Hann, |DFT|^2, mel projection: (n_mels, 1 + len(y)//hop) float64."""
    n_frames = 1 + len(y) // hop
    yp = padded(y, n_fft // 2, pad_mode)
    fr = np.stack([yp[t * hop:t * hop + n_fft] for t in range(n_frames)], axis=1)     # (n_fft, n_frames)
    cw, sw = _dft(n_fft)
    re, im = np.matmul(cw, fr), np.matmul(sw, fr)
    power = (re * re + im * im).astype(np.float64)
    return np.asarray(basis, dtype=np.float64) @ power


def normalised_db(mel, mean=MEAN, std=STD):
    """power_to_db(ref=max, amin, top_db) then (x - mean)/std; also the un-clipped relative dB."""
    db = 10.0 * np.log10(np.maximum(AMIN, mel))
    rel = db - 10.0 * np.log10(max(AMIN, float(mel.max())))
    return (np.maximum(rel, rel.max() - TOP_DB) - mean) / std, rel


def logmel(x, frames, basis, n_fft=136, hop=34, mean=MEAN, std=STD, W=128, pad_mode="constant"):
    """Per cycle.  Returns (spec (B, n_mels, W) float64, frames_spec (B, 5) int64, info) where
    info[b] = dict(mel, rel, c4): the item's mel power and un-clipped relative dB over ALL of its
    frames and the number of kept columns, for the tests' statements about their own inputs."""
    B, T = x.shape
    n_frames = 1 + T // hop
    out = np.zeros((B, basis.shape[0], W))
    fspec = np.zeros((B, 5), dtype=np.int64)
    info = []
    for b in range(B):
        mel = mel_power(x[b], n_fft, hop, basis, pad_mode)
        z, rel = normalised_db(mel, mean, std)
        fspec[b] = columns(frames[b], n_frames, T)
        c4 = max(0, min(int(fspec[b, 4]), W, n_frames))
        out[b, :, :c4] = z[:, :c4]
        info.append({"mel": mel, "rel": rel, "c4": c4})
    return out, fspec, info


def logmel_recording(y, boundaries, seg_starts, basis, n_fft=136, hop=34, mean=MEAN, std=STD, W=128,
                     pad_mode="constant"):
    """Per recording: one transform, the recording's maximum as the dB reference, then per cycle the
    columns [col(b[i]), col(b[i+4])) (cut at W and at the recording's last frame), zero-padded.
    Returns (specs (n_cycles, n_mels, W) float64, frames_spec (n_cycles, 5) cycle-relative, mel)."""
    mel = mel_power(y, n_fft, hop, basis, pad_mode)
    z, _ = normalised_db(mel, mean, std)
    n_frames = mel.shape[1]
    cols = columns(boundaries, n_frames, len(y))
    specs = np.zeros((len(seg_starts), basis.shape[0], W))
    rel = np.zeros((len(seg_starts), 5), dtype=np.int64)
    for j, i in enumerate(seg_starts):
        c0, c4 = cols[i], cols[i + 4]
        keep = max(0, min(c4 - c0, W, n_frames - c0))
        specs[j, :, :keep] = z[:, c0:c0 + keep]
        rel[j] = np.asarray(cols[i:i + 5]) - c0
    return specs, rel, mel


# ---- inputs -------------------------------------------------------------------------------------
CLASSES = ("tone", "click", "silence", "loud", "faint", "late")


def make_input(cls, T, sr, seed=0):
    """One float32 cycle of T samples and its five boundaries; frames[4] keeps the part the class is
    about inside the compared columns (or, for 'late', outside them).
      tone     110 Hz sine + 1e-4 noise floor: cells from 0 dB down to below the -80 dB clip
      click    one sample of amplitude 50 in a 1e-3 floor: most columns ~77 dB under the click's
      silence  noise at 1e-3, then exact zeros: mel power under amin in kept columns, and the item
               quiet enough (maximum ~ -40 dB) that those cells stay above the clip: amin shows
      loud     amplitude 1e4
      faint    amplitude 1e-6: every cell under amin
      late     the loudest burst lies behind frames[4] and in the last 6% of the item"""
    rs = np.random.RandomState(1000 * seed + CLASSES.index(cls))
    t = np.arange(T) / float(sr)
    f4 = int(0.93 * T) | 1
    if cls == "tone":
        x = np.sin(2 * np.pi * 110.0 * t) + 1e-4 * rs.standard_normal(T)
    elif cls == "click":
        x = 1e-3 * rs.standard_normal(T)
        x[int(0.41 * T) + 3] = 50.0
    elif cls == "silence":
        x = 1e-3 * rs.standard_normal(T) * (0.3 + np.abs(np.sin(2 * np.pi * 2.0 * t)))
        x[T // 2 + 7:] = 0.0
    elif cls == "loud":
        x = 1e4 * rs.standard_normal(T) * (0.2 + np.abs(np.sin(2 * np.pi * 3.0 * t)))
    elif cls == "faint":
        x = 1e-6 * rs.standard_normal(T)
    elif cls == "late":
        x = 0.05 * rs.standard_normal(T)
        x[int(0.94 * T):int(0.985 * T)] *= 400.0
        f4 = int(0.55 * T) | 1
    else:
        raise ValueError(cls)
    frames = np.array([0, int(0.11 * T), int(0.29 * T) + 1, int(0.43 * T), f4], dtype=np.int64)
    return x.astype(np.float32), frames


def assert_engages(cls, info, W):
    """What an input of class `cls` is meant to engage, asserted on the restatement's own
    intermediate results (info of logmel()) at the reference's 2 kHz shape."""
    for it in info:
        c4 = it["c4"]
        rel, mel = it["rel"][:, :c4], it["mel"][:, :c4]
        assert c4 > 0
        if cls in ("tone", "click"):                  # the -80 dB clip on compared cells, both sides of it
            assert (rel <= -TOP_DB).mean() >= 0.10 and (rel > -TOP_DB).mean() >= 0.10
        elif cls == "silence":                        # amin cells that the clip does not hide
            under = mel < AMIN
            assert under.mean() >= 0.10 and (rel[under] > -TOP_DB + 5.0).all()
        elif cls == "faint":
            assert (it["mel"] < AMIN).all()
        elif cls == "loud":
            assert it["mel"].max() > 1e8
        elif cls == "late":                           # the dB reference lies outside the kept image
            assert np.unravel_index(it["mel"].argmax(), it["mel"].shape)[1] >= W > c4
            assert mel.max() < 1e-3 * it["mel"].max()


def make_batch(classes, T, sr, seed=0):
    xs, fs = zip(*(make_input(c, T, sr, seed + i) for i, c in enumerate(classes)))
    return np.stack(xs), np.stack(fs)


# (sr, n_fft, hop, n_mels, fmin, fmax, T, W): what each one reaches is listed in
# tests/test_logmel_gpu.py's docstring
SWEEP = [
    (2000, 136, 34, 32, 25.0, 1000.0, 5000, 32),
    (2000, 136, 34, 16, 25.0, 1000.0, 5000, 128),
    (2000, 136, 34, 40, 25.0, 1000.0, 5000, 100),
    (2000, 136, 34, 64, 0.0, 1000.0, 5000, 64),
    (2000, 132, 33, 128, 25.0, 1000.0, 5000, 128),
    (2000, 140, 35, 128, 25.0, 1000.0, 5000, 128),
    (2000, 128, 32, 64, 25.0, 1000.0, 5000, 128),
    (2000, 80, 20, 40, 25.0, 1000.0, 3000, 96),
    (2000, 40, 10, 20, 25.0, 1000.0, 1500, 128),
    (2000, 136, 34, 128, 300.0, 900.0, 5000, 128),
    (2000, 136, 50, 128, 25.0, 1000.0, 5000, 101),
    (2000, 200, 50, 48, 25.0, 1000.0, 5000, 64),
    # the reference's own two shapes, T % hop == 0 and == hop - 1, W beyond the item's frames
    (2000, 136, 34, 128, 25.0, 1000.0, 4998, 128),
    (2000, 136, 34, 64, 25.0, 1000.0, 4997, 160),
    (1000, 68, 17, 128, 25.0, 1000.0, 2500, 128),
    (2000, 24, 6, 8, 25.0, 1000.0, 600, 128),
]
TOO_LARGE = (4000, 272, 68, 128, 25.0, 2000.0, 10000, 128)


def sweep_id(cfg):
    return "sr%d-nfft%d-hop%d-mels%d-f%g_%g-T%d-W%d" % cfg


def make_recordings(kind, sr, hop, tile, W, seed=0):
    """Recordings for the per-recording front end: (ys, boundaries, seg_starts).
      'edges'   r0: the loudest burst in the last, partial tile; a cycle across frame `tile`; a cycle
                    wider than W columns; the last cycle ends exactly at the recording's end
                r1: no cycles (empty seg_starts) but the loudest recording of all
                r2: last boundary beyond the recording's end (kept columns cut by its last frame),
                    quiet, exact silence in the middle
      'none'    three recordings, no cycles at all
      'many'    300 short recordings of one cycle each"""
    rs = np.random.RandomState(seed)
    noise = lambda n, a: (a * rs.standard_normal(n) * (0.1 + np.abs(np.sin(np.arange(n) * 2 * np.pi * 1.3 / sr))))
    if kind == "many":
        ys, bs, st = [], [], []
        for r in range(300):
            n = int(rs.randint(12 * hop, 30 * hop))
            ys.append(noise(n, float(rs.uniform(1e-3, 30.0))).astype(np.float32))
            q = np.sort(rs.choice(np.arange(1, n - 1), 3, replace=False))
            bs.append(np.array([int(rs.randint(0, 3)), q[0], q[1], q[2], n - int(rs.randint(0, 3))], dtype=np.int64))
            st.append([0])
        return ys, bs, st
    n0 = (2 * tile + 37) * hop + 5                                  # frames 0 .. 2*tile+37: partial last tile
    y0 = noise(n0, 0.05)
    y0[(2 * tile + 20) * hop:(2 * tile + 30) * hop] *= 300.0        # loudest in the last tile
    wide = (W + 19) * hop
    b0 = [40 * hop + 3]
    for step in (9, 7, 11, 8):                                      # a short cycle
        b0.append(b0[-1] + step * hop + 5)
    e = b0[-1]                                                      # a cycle wider than W, across `tile`
    b0 += [e + wide // 4, e + wide // 2 + 1, e + 3 * (wide // 4) + 3, e + wide + 9]
    assert e // hop < tile < b0[-1] // hop
    rest = n0 - b0[-1]
    assert rest > 8 * hop, "the recording must hold one more cycle"
    b0 += [b0[-1] + rest // 4, b0[-1] + rest // 2, b0[-1] + 3 * (rest // 4), n0]   # ends at the last sample
    y1 = noise(tile * hop + 11, 5.0)
    n2 = (tile + 50) * hop - 1
    y2 = noise(n2, 2e-3)
    y2[n2 // 3:n2 // 2] = 0.0
    b2 = [n2 - 30 * hop, n2 - 22 * hop, n2 - 15 * hop, n2 - 6 * hop, n2 + 4 * hop]
    b2 = [10 * hop + 1, 18 * hop, 25 * hop, 33 * hop, n2 // 2 + 9] + b2
    ys = [y0.astype(np.float32), y1.astype(np.float32), y2.astype(np.float32)]
    bs = [np.asarray(b0, dtype=np.int64), np.asarray([5, 50, 90, 120, 300], dtype=np.int64),
          np.asarray(b2, dtype=np.int64)]
    st = [[0, 4, 8], [], [0, 5]]
    if kind == "none":
        st = [[], [], []]
    elif kind != "edges":
        raise ValueError(kind)
    return ys, bs, st


# ---- the library's constant tables ----------------------------------------------------------------
def mel_table_layout(n_fft, n_mels):
    """The blob layout of pcgmix_logmel_tables (pcgmix_logmel.hip: mel_tables)."""
    n_bins = n_fft // 2 + 1
    tpp = n_bins // 32
    rem = n_bins - 32 * tpp
    if tpp >= 1 and rem <= 8:
        n_left = rem
    else:
        tpp, n_left = (n_bins + 31) // 32, 0
    ksteps = (n_fft // 4 + 1 + 3) // 4
    o = 2 * tpp * ksteps * 2 * 64 * 8
    off_wts = o
    o = (o + n_mels * n_bins * 4 + 7) & ~7
    off_kr = o
    o = (o + n_mels * 8 + 7) & ~7
    off_left = o
    o += n_left * (n_fft // 2 + 8) * 16
    off_win = o
    o += (n_fft // 2 + 1) * 8
    return dict(n_bins=n_bins, tpp=tpp, n_left=n_left, ksteps=ksteps, off_wts=off_wts, off_kr=off_kr,
                off_left=off_left, off_win=off_win, off_meta=o, total=(o + 8 + 15) & ~15)


def check_tables_are_the_windowed_transform(sr, n_fft, n_mels, fmin, fmax):
    """pcgmix_logmel_tables (host): the doubly folded twiddle fragments (window on the data side,
    even / odd bins, columns n = 0 .. n_fft/4 with weights 1/2 at both ends), the single-fold rows of
    the bins beyond the tiles, the window and bin_lo / n_left_used, evaluated in numpy exactly as the
    kernel evaluates them, give rfft(hann * frame) for every bin a mel filter reads.  Returns the
    parsed tables."""
    import ctypes
    from pcgmix_amd import _lib
    lib = _lib.load()
    lay = mel_table_layout(n_fft, n_mels)
    assert lib.pcgmix_logmel_tables_size(n_fft, n_mels) == lay["total"]
    blob = np.zeros(lay["total"], dtype=np.uint8)
    assert lib.pcgmix_logmel_tables(n_fft, n_mels, ctypes.c_float(fmin), ctypes.c_float(fmax),
                                    ctypes.c_float(sr), blob.ctypes.data) == 0
    N, H, Q = n_fft, n_fft // 2, n_fft // 4
    tpp, ks, n_bins = lay["tpp"], lay["ksteps"], lay["n_bins"]
    afrag = blob[:lay["off_wts"]].view(np.float64).reshape(tpp, ks, 4, 64)
    kr = blob[lay["off_kr"]:lay["off_kr"] + n_mels * 8].view(np.int32).reshape(n_mels, 2)
    left = blob[lay["off_left"]:lay["off_win"]].view(np.float64).reshape(lay["n_left"], H + 8, 2)
    win = blob[lay["off_win"]:lay["off_meta"]].view(np.float64)
    used, bin_lo = blob[lay["off_meta"]:lay["off_meta"] + 8].view(np.int32)
    assert np.allclose(win, 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(H + 1) / N), atol=1e-15)
    nonempty = kr[:, 1] >= kr[:, 0]
    lo_bin, hi_bin = int(kr[nonempty, 0].min()), int(kr[nonempty, 1].max())
    assert bin_lo % 2 == 0 and 0 <= bin_lo <= lo_bin and hi_bin < bin_lo + 32 * tpp + lay["n_left"]
    rs = np.random.RandomState(n_fft)
    x = rs.randn(N + 1).astype(np.float32).astype(np.float64)          # x[N] is not part of the frame
    ref = np.fft.rfft(0.5 * (1 - np.cos(2 * np.pi * np.arange(N) / N)) * x[:N])
    # the kernel's B operands, column n = 0 .. Q (column 0 pairs x[0] with itself)
    n = np.arange(Q + 1)
    hi_n = np.where(n == 0, 0, N - n)
    u, v = win[n] * (x[n] + x[hi_n]), win[n] * (x[n] - x[hi_n])
    m = H - n
    u2, v2 = win[m] * (x[m] + x[H + n]), win[m] * (x[m] - x[H + n])
    ops = [u + u2, v - v2, u - u2, v + v2]                              # even re, even im, odd re, odd im
    got = {}
    for tp in range(tpp):
        for row in range(16):
            for par in range(2):
                b = bin_lo + 2 * (16 * tp + row) + par
                lanes = row + 16 * np.arange(4)                       # lane = row + 16 * (n & 3), k-step n >> 2
                coef = lambda q: np.array([afrag[tp, nn >> 2, q, lanes[nn & 3]] for nn in range(4 * ks)])
                cre, cim = coef(2 * par), coef(2 * par + 1)
                assert (cre[Q + 1:] == 0).all() and (cim[Q + 1:] == 0).all()
                if b < n_bins:
                    got[b] = complex(np.dot(cre[:Q + 1], ops[2 * par]), np.dot(cim[:Q + 1], ops[2 * par + 1]))
    k = np.arange(1, H + 1)
    for lb in range(lay["n_left"]):
        b = bin_lo + 32 * tpp + lb
        assert (left[lb, H:] == 0).all()                               # the zero columns behind the row
        if b < n_bins:
            got[b] = complex(np.dot(left[lb, :H, 0], x[k] + x[N - k]), np.dot(left[lb, :H, 1], x[k] - x[N - k]))
    for b in range(lo_bin, hi_bin + 1):
        assert b in got, b
        assert abs(got[b] - ref[b]) <= 1e-12 * max(1.0, np.abs(ref).max()), (b, got[b], ref[b])
    assert used == max(0, min(lay["n_left"], hi_bin - (bin_lo + 32 * tpp) + 1))
    wts = blob[lay["off_wts"]:lay["off_wts"] + n_mels * n_bins * 4].view(np.float32).reshape(n_mels, n_bins)
    return dict(lay=lay, wts=wts, krange=kr, n_left_used=int(used), bin_lo=int(bin_lo))
