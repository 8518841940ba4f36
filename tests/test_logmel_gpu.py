"""HIP log-mel front end against the numpy restatement of librosa 0.9.2 semantics
(oracle.logmel — parity with librosa itself is UNPINNED: it is not installed and the reference
stores no spectrogram) and against the high-precision restatement of
tests/logmel_ref.py (direct long-double DFT, float64 behind it).  Both are held to 1e-4 on every
element; tests/test_logmel_cpu.py holds the two restatements to 1e-5 of each other.

Which test reaches which branch of csrc/pcgmix_logmel.hip (SWEEP index = position in
logmel_ref.SWEEP; what a shape's tables look like is asserted on the host by
test_logmel_cpu.py::test_the_sweep_reaches_the_table_layouts_it_is_meant_to):

  top_db clip on kept cells            test_logmel_input_classes[tone], [click]
  amin on kept cells above the clip    test_logmel_input_classes[silence]; every cell at amin: [faint]
  dB reference outside the kept image  test_logmel_input_classes[late] (behind f4 and behind column W)
  large amplitudes                     test_logmel_input_classes[loud]
  mel span >= 4 (weights from global)  test_logmel_sweep[0] (span 3 of the 4-tap path), [1] (spans 6-7),
                                       [2], [11] (spans 2-3)
  partial sums in their own LDS region test_logmel_sweep[0] (32 x 32 image), [1] (16 x 128)
  n_left == 0                          test_logmel_sweep[7] (n_fft 80), [8] (n_fft 40), [15] (n_fft 24)
  n_left_used == 0 with n_left > 0     test_logmel_sweep[6] (n_fft 128), [9] (300-900 Hz)
  n_left_used 4 / 5 / 1                test_logmel_sweep[3] (fmin 0) / [5] (n_fft 140) / [4] (n_fft 132)
  bin_lo 0 / 10                        test_logmel_sweep[3], [7] / [9]
  the KS = 9 ring off n_fft 136        test_logmel_sweep[4] (132), [5] (140), [6] (128)
  general loop, ksteps 2, 3, 5, 6, 13  test_logmel_sweep[15], [8], [14], [7], [11]
  hop != n_fft / 4                     test_logmel_sweep[10]
  store: kMelThreads % W != 0          test_logmel_sweep[2] (W 100), [7] (96), [10] (101), [13] (160)
  W > n_frames (col_end clamp)         test_logmel_sweep[13]
  T % hop == 0 / hop - 1               test_logmel_sweep[12] / [13]
  f4 == 0 / f4 == T                    every test_logmel_sweep case (items 0 / 1)
  1 kHz, filters empty above Nyquist   test_logmel_sweep[14]
  shape beyond the LDS budget refused  test_logmel_shape_that_does_not_fit_is_refused
  frames in device memory, B > 1024    test_logmel_device_frames_branch_of_the_frontend
  every hipErrorInvalidValue return    test_logmel_entry_points_refuse_bad_arguments
  recordings: maximum in the last partial tile, a cycle across a tile edge, a cycle wider than W,
    a cycle ending at / cut by the recording's last frame, a recording without cycles, exact
    silence above the clip                test_logmel_recordings_edges (W 128; W 100: the scalar slice
                                          path; 1 kHz: the general loop in tile mode)
  recordings: no cycle at all          test_logmel_recordings_without_any_cycle
  recordings: R = 300 (zero_u32_kernel's second block)   test_logmel_recordings_many_short
"""
import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import frontend, synthetic
from oracle import pcgmix_oracle as O

import logmel_ref as R

pytestmark = pytest.mark.gpu


def test_filterbank_structure():
    """125 of the 128 filters have one non-zero FFT bin, 3 have two."""
    w = O.mel_filterbank(2000.0, 136, 128, 25.0, 1000.0)
    nnz = (w > 0).sum(1)
    assert (nnz == 1).sum() == 125 and (nnz == 2).sum() == 3 and (nnz == 0).sum() == 0
    assert (w[:, [0, 1, 68]] == 0).all()


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("B,seed", [(8, 0), (32, 3)])
def test_logmel_matches_restatement(B, seed, pad_mode, device):
    """Per-cycle front end vs the numpy restatement, for both paddings of the centred frames
    (which one librosa 0.9.2 defaults to is the open point of the restatement: a parameter, with
    'constant' the default; tolerance 1e-4 = north_star's bound on spectrograms)."""
    x, frames, _, _ = synthetic.make_batch(B, 1, 5000, sample_rate=2000, seed=seed)
    # heart-sound-like content: band-limited bursts instead of white noise in S1/S2
    t = np.arange(5000) / 2000.0
    x[:, 0] *= (0.2 + np.abs(np.sin(2 * np.pi * 3.0 * t)))[None, :].astype(np.float32)
    ref, fs_ref = O.logmel(x[:, 0], frames, pad_mode=pad_mode)
    spec, fs = frontend.logmel(torch.from_numpy(x).to(device), frames, pad_mode=pad_mode)
    got = spec.cpu().numpy()[:, 0]
    assert np.array_equal(fs, fs_ref)                      # column boundaries: bit-exact
    assert got.shape == (B, 128, 128)
    err = np.abs(got - ref)
    assert err.max() <= 1e-4, err.max()                    # north_star tolerance on spectrograms
    cols = np.arange(128)[None, None, :] >= fs[:, 4][:, None, None]
    assert (got[np.broadcast_to(cols, got.shape)] == 0).all()


@pytest.mark.parametrize("sample_rate,T", [(2000, 5000), (1000, 2500), (1000, 1800)])
def test_logmel_boundaries_in_arguments_equal_boundaries_in_memory(sample_rate, T, device):
    """pcgmix_logmel_hostframes_f32 (cycle ends in the kernel arguments: what frontend.logmel calls)
    == pcgmix_logmel_f32 (boundaries read from device memory, with frames_out), bit for bit, at
    n_fft = 136 (nine k-steps, the register ring) and at 68 (the general loop); and both
    against the restatement."""
    import ctypes
    from pcgmix_amd import _lib
    from pcgmix_amd.augmentations import upload_array
    B = 6
    x, frames, _, _ = synthetic.make_batch(B, 1, T, sample_rate=sample_rate, seed=2)
    xd = torch.from_numpy(x[:, 0].copy()).to(device)
    spec, fs = frontend.logmel(xd, frames, sample_rate=sample_rate)
    n_fft, hop = frontend.stft_params(sample_rate)
    lib = _lib.load()
    tables = frontend.logmel_tables(xd.device, n_fft, 128, sample_rate)
    fr = upload_array(frames.astype(np.int32), xd.device)
    spec2 = torch.empty_like(spec)
    fo = torch.empty((B, 5), dtype=torch.int32, device=device)
    _lib.check(lib.pcgmix_logmel_f32(xd.data_ptr(), fr.data_ptr(), tables.data_ptr(), spec2.data_ptr(),
                                     fo.data_ptr(), B, T, n_fft, hop, 128, ctypes.c_float(frontend.TRAIN_MEAN),
                                     ctypes.c_float(frontend.TRAIN_STD), 128, 0,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "pcgmix_logmel_f32")
    assert torch.equal(spec, spec2)
    assert np.array_equal(fo.cpu().numpy().astype(np.int64), fs)
    ref, fs_ref = O.logmel(x[:, 0], frames, n_fft=n_fft, hop=hop, sr=float(sample_rate))
    assert np.array_equal(fs, fs_ref)
    assert np.abs(spec.cpu().numpy()[:, 0] - ref).max() <= 1e-4


def test_logmel_silence_and_bad_arguments(device):
    x = torch.zeros(2, 5000, device=device)
    frames = np.array([[0, 200, 600, 800, 1800]] * 2)
    spec, fs = frontend.logmel(x, frames)
    # all-zero input: every band sits at amin, ref is amin too -> 0 dB -> (0 - mean)/std inside
    inside = spec[0, 0, :, : int(fs[0, 4])].cpu().numpy()
    assert np.allclose(inside, (0.0 - frontend.TRAIN_MEAN) / frontend.TRAIN_STD, atol=1e-6)
    with pytest.raises(ValueError):
        frontend.logmel(torch.zeros(2, 2, 5000, device=device), frames)
    with pytest.raises(ValueError):
        frontend.logmel(torch.zeros(2, 5000), frames)


def test_pad_modes_differ_only_at_the_edges(device):
    x, frames, _, _ = synthetic.make_batch(4, 1, 5000, sample_rate=2000, seed=1)
    x[:, 0, 2000:2400] *= 6.0                              # the item's maximum is in the interior
    frames[:, 4] = 4990                                    # keep every column
    xd = torch.from_numpy(x).to(device)
    a, _ = frontend.logmel(xd, frames, pad_mode="constant")
    b, _ = frontend.logmel(xd, frames, pad_mode="reflect")
    a, b = a.cpu().numpy()[:, 0], b.cpu().numpy()[:, 0]
    assert frontend.DEFAULT_PAD_MODE == "constant"
    assert np.abs(a[:, :, :2] - b[:, :, :2]).max() > 1e-3  # frames 0, 1 see the padding
    assert np.abs(a[:, :, 2:128] - b[:, :, 2:128]).max() <= 1e-5
    with pytest.raises(ValueError):
        frontend.logmel(xd, frames, pad_mode="edge")


def _recordings(seed, n_rec, sample_rate=2000):
    """Synthetic recordings in the shape databuilder.ipynb cell 6 sees them: a waveform of several
    consecutive heart cycles, the boundaries of ALL heart states in samples, and the indices of
    the boundaries at which a full cycle starts."""
    rs = np.random.RandomState(seed)
    ys, bounds, starts = [], [], []
    for r in range(n_rec):
        n_cyc = int(rs.randint(3, 12))
        fr = synthetic.make_frames(n_cyc, sample_rate / 1000.0, rs)          # (n_cyc, 5) relative
        lead = int(rs.randint(0, 900))
        b = [lead]
        for c in range(n_cyc):
            b += list(b[-1] + np.diff(fr[c]))
        tail = int(rs.randint(70, 1500))
        n = b[-1] + tail
        t = np.arange(n) / sample_rate
        y = (rs.standard_normal(n) * (0.05 + np.abs(np.sin(2 * np.pi * 1.3 * t + r)))).astype(np.float32)
        y *= float(rs.uniform(0.05, 3.0))                                  # recordings differ in level
        ys.append(y)
        bounds.append(np.asarray(b, dtype=np.int64))
        starts.append(list(range(0, 4 * n_cyc, 4)))
    return ys, bounds, starts


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_logmel_recordings_match_restatement(pad_mode, device):
    """The reference's order of operations (databuilder.ipynb cell 6:81-101, 127-142): ONE
    transform per recording, dB relative to the recording's maximum, per-cycle column slices,
    zero-padding after normalisation — against oracle.logmel_recording; column boundaries
    bit-exact, values within 1e-4."""
    ys, bounds, starts = _recordings(11, 9)
    y = torch.from_numpy(np.concatenate(ys)).to(device)
    spec, fs, rec_of = frontend.logmel_recordings(y, [len(v) for v in ys], bounds, starts,
                                                  pad_mode=pad_mode)
    got = spec.cpu().numpy()[:, 0]
    k = 0
    for r, (yy, b, st) in enumerate(zip(ys, bounds, starts)):
        ref, rel = O.logmel_recording(yy, b, st, pad_mode=pad_mode)
        n = len(st)
        assert np.array_equal(fs[k:k + n], rel) and (rec_of[k:k + n] == r).all()
        err = np.abs(got[k:k + n] - ref).max()
        assert err <= 1e-4, (r, err)
        k += n
    assert k == got.shape[0] and got.shape[1:] == (128, 128)


def test_recording_level_differs_from_per_cycle_as_documented(device):
    """Why both granularities exist: the same cycle cut out of a recording-level spectrogram
    differs from the per-cycle transform of its samples at the cycle's edge columns (neighbouring
    samples instead of padding) and by the dB reference (recording maximum vs item maximum); in
    the interior, when the cycle starts on the recording's frame grid, the two differ by that
    constant only."""
    rs = np.random.RandomState(5)
    hop = 34
    fr = synthetic.make_frames(3, 2.0, rs)
    b = [5 * hop]                                           # cycle 0 starts on the frame grid
    for c in range(3):
        b += list(b[-1] + np.diff(fr[c]))
    n = b[-1] + 400
    y = rs.standard_normal(n).astype(np.float32)
    y[b[4]:b[8]] *= 4.0                                     # the loudest part is in cycle 1
    bounds = np.asarray(b, dtype=np.int64)
    spec, fs, _ = frontend.logmel_recordings(torch.from_numpy(y).to(device), [n], [bounds], [[0, 4, 8]])
    item = np.zeros((1, 5000), np.float32)
    seg = y[b[0]:b[4]]
    item[0, :len(seg)] = seg
    per_cycle, fs1 = frontend.logmel(torch.from_numpy(item).to(device), (bounds[:5] - b[0])[None, :])
    a, c = spec[0, 0].cpu().numpy(), per_cycle[0, 0].cpu().numpy()
    m = int(min(fs[0, 4], fs1[0, 4])) - 3
    diff = a[:, 3:m] - c[:, 3:m]
    assert np.abs(diff).max() > 1e-2                        # not the same image ...
    assert np.ptp(diff) <= 2e-3                             # ... but a constant apart inside
    assert np.abs(a[:, :2] - c[:, :2] - diff.mean()).max() > 1e-2   # and not at the edge columns


# ---- parity across the shapes and inputs the ABI accepts -------------------------------------------
TOL = 1e-4                 # the project's bound on spectrograms (README), every element
INVALID = 1                # hipErrorInvalidValue


def _tables(cfg, device):
    import ctypes
    from pcgmix_amd import _lib
    sr, n_fft, hop, n_mels, fmin, fmax, T, W = cfg
    lib = _lib.load()
    host = np.zeros(lib.pcgmix_logmel_tables_size(n_fft, n_mels), dtype=np.uint8)
    _lib.check(lib.pcgmix_logmel_tables(n_fft, n_mels, ctypes.c_float(fmin), ctypes.c_float(fmax),
                                        ctypes.c_float(sr), host.ctypes.data), "pcgmix_logmel_tables")
    return torch.from_numpy(host).to(device)


def _abi(cfg, x, frames, pad_mode, device, entry="hostframes", tables=None, check=True):
    """One call of the C ABI with the shape's own tables.  Returns (rc, spec (B, n_mels, W) numpy,
    frames_out or None)."""
    import ctypes
    from pcgmix_amd import _lib
    from pcgmix_amd.augmentations import upload_array
    sr, n_fft, hop, n_mels, fmin, fmax, T, W = cfg
    lib = _lib.load()
    B = x.shape[0]
    tables = _tables(cfg, device) if tables is None else tables
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    spec = torch.full((B, n_mels, W), 7.0, dtype=torch.float32, device=device)
    fr32 = np.ascontiguousarray(frames, dtype=np.int32)
    mean, std = ctypes.c_float(frontend.TRAIN_MEAN), ctypes.c_float(frontend.TRAIN_STD)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fo = None
    if entry == "hostframes":
        rc = lib.pcgmix_logmel_hostframes_f32(xd.data_ptr(), fr32.ctypes.data, tables.data_ptr(), spec.data_ptr(),
                                              B, T, n_fft, hop, n_mels, mean, std, W, frontend.PAD_MODES[pad_mode],
                                              stream)
    else:
        fr = upload_array(fr32, xd.device)
        fo = torch.full((B, 5), -1, dtype=torch.int32, device=device)
        rc = lib.pcgmix_logmel_f32(xd.data_ptr(), fr.data_ptr(), tables.data_ptr(), spec.data_ptr(), fo.data_ptr(),
                                   B, T, n_fft, hop, n_mels, mean, std, W, frontend.PAD_MODES[pad_mode], stream)
    if check:
        _lib.check(rc, "pcgmix_logmel_*")
    torch.cuda.synchronize()
    return rc, spec.cpu().numpy(), (None if fo is None else fo.cpu().numpy().astype(np.int64))


def _compare(got, ref, orc, fs, fs_ref, fs_orc, W, n_frames):
    """Boundaries exact, every element within TOL of both restatements, columns >= c4 exactly 0."""
    assert np.array_equal(fs, fs_ref) and np.array_equal(fs, fs_orc)
    e_ref, e_orc = float(np.abs(got - ref).max()), float(np.abs(got - orc).max())
    print("max |gpu - ref| = %.3g, max |gpu - oracle| = %.3g" % (e_ref, e_orc))
    assert e_ref <= TOL, e_ref
    assert e_orc <= TOL, e_orc
    c4 = np.minimum(fs[:, 4], min(W, n_frames))
    cols = np.arange(W)[None, None, :] >= c4[:, None, None]
    assert (got[np.broadcast_to(cols, got.shape)] == 0).all()
    return max(e_ref, e_orc)


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("cls", R.CLASSES)
def test_logmel_input_classes(cls, pad_mode, device, record_property):
    """The inputs that engage amin, the top_db clip and the dB reference on cells that are compared
    (frontend.logmel at the reference's 2 kHz shape); what each input engages is first asserted on
    the restatement alone."""
    T, sr = 5000, 2000
    x, frames = R.make_batch([cls] * 3, T, sr, seed=3)
    basis = O.mel_filterbank(2000.0, 136, 128, 25.0, 1000.0)
    ref, fs_ref, info = R.logmel(x, frames, basis, pad_mode=pad_mode)
    R.assert_engages(cls, info, 128)
    orc, fs_orc = O.logmel(x, frames, pad_mode=pad_mode)
    spec, fs = frontend.logmel(torch.from_numpy(x).to(device), frames, pad_mode=pad_mode)
    worst = _compare(spec.cpu().numpy()[:, 0], ref, orc, fs, fs_ref, fs_orc, 128, 148)
    record_property("max_abs_err", worst)


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("idx", range(len(R.SWEEP)), ids=[R.sweep_id(c) for c in R.SWEEP])
def test_logmel_sweep(idx, pad_mode, device, record_property):
    """Every input class as one item of a batch, item 0 with f4 = 0 and item 1 with f4 = T, at each
    swept shape: pcgmix_logmel_hostframes_f32 and pcgmix_logmel_f32 with the shape's own tables, bit
    for bit equal to each other, and frontend.logmel where it can express the shape."""
    from pcgmix_amd import _lib
    cfg = R.SWEEP[idx]
    sr, n_fft, hop, n_mels, fmin, fmax, T, W = cfg
    out = np.zeros(20, dtype=np.int32)
    assert _lib.load().pcgmix_logmel_lds_layout(0, T, n_fft, hop, n_mels, W, -1, out.ctypes.data) == 0
    assert out[18] == 1 and out[15] <= out[13], "never launch a shape whose LDS plan does not hold"
    x, frames = R.make_batch(R.CLASSES, T, sr, seed=1)
    frames[0, 4], frames[1, 4] = 0, T
    basis = O.mel_filterbank(float(sr), n_fft, n_mels, fmin, fmax)
    ref, fs_ref, _ = R.logmel(x, frames, basis, n_fft=n_fft, hop=hop, W=W, pad_mode=pad_mode)
    orc, fs_orc = O.logmel(x, frames, n_fft=n_fft, hop=hop, n_mels=n_mels, fmin=fmin, fmax=fmax,
                           sr=float(sr), W=W, pad_mode=pad_mode)
    tables = _tables(cfg, device)
    _, got, _ = _abi(cfg, x, frames, pad_mode, device, "hostframes", tables)
    _, got2, fo = _abi(cfg, x, frames, pad_mode, device, "device", tables)
    assert np.array_equal(got, got2)
    worst = _compare(got, ref, orc, fo, fs_ref, fs_orc, W, 1 + T // hop)
    assert (got[0] == 0).all()                                             # f4 = 0: nothing kept
    if (n_fft, hop) == frontend.stft_params(sr) and (fmin, fmax) == (frontend.FMIN, frontend.FMAX):
        spec, fs = frontend.logmel(torch.from_numpy(x).to(device), frames, sample_rate=sr, n_mels=n_mels,
                                   width=W, pad_mode=pad_mode)
        assert np.array_equal(spec.cpu().numpy()[:, 0], got) and np.array_equal(fs, fs_ref)
    record_property("max_abs_err", worst)


def test_logmel_shape_that_does_not_fit_is_refused(device):
    """A 4 kHz cycle (n_fft 272, T 10000, 128 x 128) needs more LDS than a block can have: both
    per-cycle entry points return hipErrorInvalidValue and write nothing."""
    cfg = R.TOO_LARGE
    x, frames = R.make_batch(R.CLASSES[:2], cfg[6], cfg[0], seed=1)
    for entry in ("hostframes", "device"):
        rc, spec, _ = _abi(cfg, x, frames, "constant", device, entry, check=False)
        assert rc == INVALID and (spec == 7.0).all()


def test_logmel_device_frames_branch_of_the_frontend(device):
    """B = 1025 takes frontend.logmel's other branch (boundaries uploaded, pcgmix_logmel_f32 with
    frames_out = NULL): bit for bit the host-frames path on the first 1024 items, the last item
    against the restatements."""
    B, T, sr = 1025, 2500, 1000
    x6, f6 = R.make_batch(R.CLASSES, T, sr, seed=2)
    reps = -(-B // 6)
    x, frames = np.tile(x6, (reps, 1))[:B].copy(), np.tile(f6, (reps, 1))[:B].copy()
    x *= (1.0 + 0.001 * (np.arange(B) % 97))[:, None].astype(np.float32)
    frames[:, 4] -= (np.arange(B) % 50) * 7
    xd = torch.from_numpy(x).to(device)
    big, fs_big = frontend.logmel(xd, frames, sample_rate=sr)
    small, fs_small = frontend.logmel(xd[:1024].contiguous(), frames[:1024], sample_rate=sr)
    assert torch.equal(big[:1024], small) and np.array_equal(fs_big[:1024], fs_small)
    basis = O.mel_filterbank(float(sr), 68, 128, 25.0, 1000.0)
    ref, fs_ref, _ = R.logmel(x[1020:], frames[1020:], basis, n_fft=68, hop=17)
    orc, fs_orc = O.logmel(x[1020:], frames[1020:], n_fft=68, hop=17, sr=float(sr))
    _compare(big[1020:, 0].cpu().numpy(), ref, orc, fs_big[1020:], fs_ref, fs_orc, 128, 1 + T // 17)


def test_logmel_entry_points_refuse_bad_arguments(device):
    """Every hipErrorInvalidValue return of pcgmix_logmel_f32, pcgmix_logmel_hostframes_f32 and
    pcgmix_logmel_recordings_f32, one violated condition at a time; nothing is launched (the output
    keeps its fill) and the same call with the condition restored succeeds."""
    import ctypes
    from pcgmix_amd import _lib
    lib = _lib.load()
    T, n_fft, hop, n_mels, W, B = 600, 24, 6, 8, 16, 2
    cfg = (2000, n_fft, hop, n_mels, 25.0, 1000.0, T, W)
    tables = _tables(cfg, device)
    x = torch.randn(B, T, device=device)
    fr_host = np.array([[0, 100, 200, 300, 500]] * B, dtype=np.int32)
    fr_dev = torch.from_numpy(fr_host).to(device)
    spec = torch.full((B, n_mels, W), 7.0, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cf = ctypes.c_float
    good = dict(x=x.data_ptr(), frames=fr_dev.data_ptr(), tables=tables.data_ptr(), spec=spec.data_ptr(),
                frames_out=None, B=B, T=T, n_fft=n_fft, hop=hop, n_mels=n_mels, mean=cf(0.0), std=cf(1.0), W=W,
                pad_mode=0)
    order = ("x", "frames", "tables", "spec", "frames_out", "B", "T", "n_fft", "hop", "n_mels", "mean", "std", "W",
             "pad_mode")
    bad_common = [("x", None), ("frames", None), ("tables", None), ("spec", None), ("B", -1), ("T", 1),
                  ("n_fft", 0), ("n_fft", 22), ("hop", 0), ("n_mels", 0), ("W", 0), ("std", cf(0.0)),
                  ("T", 12), ("pad_mode", 2), ("pad_mode", -1),
                  ("W", 6000)]                                             # 8 x 6000 image: beyond the LDS budget

    def call(entry, **kw):
        a = dict(good, **kw)
        if entry == "device":
            return lib.pcgmix_logmel_f32(*[a[k] for k in order], stream)
        a["frames"] = fr_host.ctypes.data if kw.get("frames", 1) is not None else None
        return lib.pcgmix_logmel_hostframes_f32(*[a[k] for k in order if k != "frames_out"], stream)

    for entry in ("device", "hostframes"):
        for k, v in bad_common + ([("B", 1025), ("T", 32768)] if entry == "hostframes" else []):
            assert call(entry, **{k: v}) == INVALID, (entry, k, v)
        torch.cuda.synchronize()
        assert (spec == 7.0).all()
        assert call(entry, B=0) == 0 and (spec == 7.0).all()               # an empty batch is fine
        assert call(entry) == 0
        torch.cuda.synchronize()
        assert not (spec == 7.0).any()
        spec.fill_(7.0)
    # the table builder and its size
    host = np.zeros(lib.pcgmix_logmel_tables_size(n_fft, n_mels), dtype=np.uint8)
    for a in ((n_fft, n_mels, 25.0, 1000.0, 2000.0, None), (0, n_mels, 25.0, 1000.0, 2000.0, 1),
              (22, n_mels, 25.0, 1000.0, 2000.0, 1), (n_fft, 0, 25.0, 1000.0, 2000.0, 1),
              (n_fft, n_mels, 1000.0, 1000.0, 2000.0, 1), (n_fft, n_mels, 25.0, float("nan"), 2000.0, 1),
              (n_fft, n_mels, 25.0, 1000.0, 0.0, 1)):
        out = host.ctypes.data if a[5] else None
        assert lib.pcgmix_logmel_tables(a[0], a[1], cf(a[2]), cf(a[3]), cf(a[4]), out) == INVALID, a
    assert [lib.pcgmix_logmel_tables_size(*a) for a in ((0, 8), (22, 8), (24, 0))] == [0, 0, 0]
    # the per-recording entry point
    y = torch.randn(900, device=device)
    rec_off = torch.zeros(1, dtype=torch.int64, device=device)
    rec_len = torch.full((1,), 900, dtype=torch.int32, device=device)
    n_frames = 1 + 900 // hop
    tiles_np = np.array([[0, f0, min(128, n_frames - f0), f0] for f0 in range(0, n_frames, 128)], dtype=np.int32)
    tiles = torch.from_numpy(tiles_np).to(device)
    cycles = torch.tensor([[0, 10, 12, 0]], dtype=torch.int32, device=device)
    scratch = torch.empty((n_mels, n_frames), device=device)
    ref_pow = torch.empty(1, dtype=torch.int32, device=device)
    rspec = torch.full((1, n_mels, W), 7.0, device=device)
    rgood = dict(y=y.data_ptr(), rec_off=rec_off.data_ptr(), rec_len=rec_len.data_ptr(), R=1, tiles=tiles.data_ptr(),
                 n_tiles=len(tiles_np), cycles=cycles.data_ptr(), n_cycles=1, tables=tables.data_ptr(),
                 db_scratch=scratch.data_ptr(), scratch_cols=n_frames, ref_pow=ref_pow.data_ptr(),
                 spec=rspec.data_ptr(), n_fft=n_fft, hop=hop, n_mels=n_mels, mean=cf(0.0), std=cf(1.0), W=W, pad_mode=0)
    rorder = tuple(rgood)
    rbad = [(k, None) for k in ("y", "rec_off", "rec_len", "tiles", "cycles", "tables", "db_scratch", "ref_pow", "spec")]
    rbad += [("R", 0), ("n_tiles", 0), ("n_cycles", -1), ("scratch_cols", 0), ("n_fft", 0), ("n_fft", 22), ("hop", 0),
             ("n_mels", 0), ("W", 0), ("std", cf(0.0)), ("pad_mode", 2), ("hop", 400)]   # 128 frames x 400: beyond LDS
    for k, v in rbad:
        a = dict(rgood, **{k: v})
        assert lib.pcgmix_logmel_recordings_f32(*[a[k2] for k2 in rorder], stream) == INVALID, (k, v)
    torch.cuda.synchronize()
    assert (rspec == 7.0).all()
    assert lib.pcgmix_logmel_recordings_f32(*[rgood[k2] for k2 in rorder], stream) == 0
    torch.cuda.synchronize()
    assert not (rspec[:, :, :12] == 7.0).any() and (rspec[:, :, 12:] == 0).all()


def test_logmel_recordings_frontend_checks(device):
    y = torch.zeros(3000, device=device)
    b = [np.array([0, 100, 200, 300, 400])]
    with pytest.raises(ValueError):
        frontend.logmel_recordings(y, [2999], b, [[0]])                     # lengths do not add up
    with pytest.raises(ValueError):
        frontend.logmel_recordings(y, [2932, 68], b + b, [[0], []])         # shorter than half a window
    with pytest.raises(ValueError):
        frontend.logmel_recordings(y.cpu(), [3000], b, [[0]])
    with pytest.raises(ValueError):
        frontend.logmel_recordings(y.view(1, -1), [3000], b, [[0]])
    with pytest.raises(ValueError):
        frontend.logmel_recordings(y, [3000], b, [[0]], pad_mode="edge")
    spec, fs, rec_of = frontend.logmel_recordings(y, [2931, 69], b + b, [[0], []])
    assert spec.shape == (1, 1, 128, 128) and rec_of.tolist() == [0]


def _check_recordings(ys, bounds, starts, sr, W, pad_mode, device):
    hop = int(sr * 2.2 / 128)
    n_fft = 4 * hop
    basis = O.mel_filterbank(float(sr), n_fft, 128, 25.0, 1000.0)
    y = torch.from_numpy(np.concatenate(ys)).to(device)
    spec, fs, rec_of = frontend.logmel_recordings(y, [len(v) for v in ys], bounds, starts, sample_rate=sr,
                                                  width=W, pad_mode=pad_mode)
    got = spec.cpu().numpy()[:, 0]
    k, worst = 0, 0.0
    for r, (yy, b, st) in enumerate(zip(ys, bounds, starts)):
        n = len(st)
        if n:
            ref, rel, _ = R.logmel_recording(yy, b, st, basis, n_fft=n_fft, hop=hop, W=W, pad_mode=pad_mode)
            orc, rel_o = O.logmel_recording(yy, b, st, n_fft=n_fft, hop=hop, sr=float(sr), W=W, pad_mode=pad_mode)
            assert np.array_equal(fs[k:k + n], rel) and np.array_equal(rel, rel_o) and (rec_of[k:k + n] == r).all()
            e_ref, e_orc = np.abs(got[k:k + n] - ref).max(), np.abs(got[k:k + n] - orc).max()
            assert e_ref <= TOL, (r, e_ref)
            assert e_orc <= TOL, (r, e_orc)
            worst = max(worst, float(e_ref), float(e_orc))
        k += n
    assert k == got.shape[0] and got.shape[1:] == (128, W)
    print("max |gpu - restatements| = %.3g" % worst)
    return worst


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("sr,W", [(2000, 128), (2000, 100), (1000, 128), (1000, 100)])
def test_logmel_recordings_edges(sr, W, pad_mode, device, record_property):
    from pcgmix_amd import _lib
    hop, tile = int(sr * 2.2 / 128), _lib.load().pcgmix_logmel_tile_frames()
    ys, bounds, starts = R.make_recordings("edges", sr, hop, tile, W, seed=4)
    # what the generator is meant to produce, on the restatement alone
    basis = O.mel_filterbank(float(sr), 4 * hop, 128, 25.0, 1000.0)
    _, rel, mel = R.logmel_recording(ys[0], bounds[0], starts[0], basis, n_fft=4 * hop, hop=hop, W=W, pad_mode=pad_mode)
    n_frames = mel.shape[1]
    cols = R.columns(bounds[0], n_frames, len(ys[0]))
    assert n_frames % tile and np.unravel_index(mel.argmax(), mel.shape)[1] >= (n_frames // tile) * tile
    assert cols[4] < tile < cols[8] and cols[8] - cols[4] > W and cols[12] == n_frames
    _, _, mel2 = R.logmel_recording(ys[2], bounds[2], starts[2], basis, n_fft=4 * hop, hop=hop, W=W, pad_mode=pad_mode)
    cols2 = R.columns(bounds[2], mel2.shape[1], len(ys[2]))
    assert cols2[9] > mel2.shape[1] > cols2[5]                               # cut by the last frame
    kept = mel2[:, cols2[0]:cols2[4]]
    assert (kept < R.AMIN).mean() >= 0.10 and 10 * np.log10(mel2.max()) < -25.0   # amin cells above the clip
    record_property("max_abs_err", _check_recordings(ys, bounds, starts, sr, W, pad_mode, device))


def test_logmel_recordings_without_any_cycle(device):
    ys, bounds, starts = R.make_recordings("none", 2000, 34, 128, 128, seed=4)
    y = torch.from_numpy(np.concatenate(ys)).to(device)
    spec, fs, rec_of = frontend.logmel_recordings(y, [len(v) for v in ys], bounds, starts)
    torch.cuda.synchronize()
    assert spec.shape == (0, 1, 128, 128) and fs.shape == (0, 5) and rec_of.shape == (0,)


@pytest.mark.parametrize("sr", [2000, 1000])
def test_logmel_recordings_many_short(sr, device, record_property):
    hop = int(sr * 2.2 / 128)
    ys, bounds, starts = R.make_recordings("many", sr, hop, 128, 128, seed=6)
    assert len(ys) == 300
    record_property("max_abs_err", _check_recordings(ys, bounds, starts, sr, 128, "constant", device))
