/*
 * pcgmix_hip.h — C ABI of libpcgmix_hip.so, the MI355X (gfx950) implementation of the
 * PCGmix per-batch hot path.
 *
 * This is the drop-in boundary.  The upstream reference is pure Python and
 * has no FFI of its own; each entry point below replaces the O(B*C*T) part of one reference
 * function and is what a ctypes binding inside the reference's augmentations.py would call
 * (INTEGRATION.md shows that binding).  Conventions:
 *
 *   - every pointer documented "device" is a device pointer owned by the caller;
 *   - no entry point allocates device memory, synchronises, or touches the default stream:
 *     kernels are enqueued on `stream` and the call returns;
 *   - return value: 0 (hipSuccess) or a hipError_t; pcgmix_error_string() names it;
 *   - tensors are dense row-major ("contiguous" in torch terms), float32 unless noted;
 *   - `frames` holds cumulative heart-state boundaries per sample,
 *     [0, S1end, sysEnd, S2end, cycleEnd] (dataloader_physionet.py:151-172), as int32.
 *
 * File:line citations are into the upstream repository
 * (Liisjak/PCGmix-A-Data-Augmentation-Method-for-Heart-Sound-Classification-EXTENDED).
 */
#ifndef PCGMIX_HIP_H
#define PCGMIX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque HIP stream handle (same type as hipStream_t; declared here so that a host
 * language binding does not need the HIP headers). */
typedef struct ihipStream_t* pcgmix_stream_t;

#define PCGMIX_ABI_VERSION 25

/* ABI version of the loaded library (== PCGMIX_ABI_VERSION it was built with). */
int pcgmix_abi_version(void);

/* Human-readable name of an error code returned by any entry point. */
const char* pcgmix_error_string(int err);

/* ------------------------------------------------------------------------------------------
 * Constant operator of the magnitude-warp spline.                                  [host]
 *
 * Replaces the per-(sample, channel) construction
 *     CubicSpline(linspace(0, T-1, n_knots), random_warps[b, :, c])
 * in magnitude_warp(), augmentations.py:674-683 (scipy default bc_type 'not-a-knot').  The
 * break points are the same for every (b, c), so knots -> piecewise-cubic coefficients is
 * one constant linear map; this fills
 *     op[0 .. n_knots-1]                              break points, float64, as numpy's
 *                                                     linspace(0, T-1, n_knots) rounds them
 *     op[n_knots + (p*4 + j)*n_knots + i]             d coef[p][j] / d knot[i],
 *                                                     p = piece 0..n_knots-2,
 *                                                     j = 0..3 multiplies (t - brk[p])^(3-j)
 * Pure host arithmetic; no device is touched.  n_knots >= 2, T >= 2.
 * Size of `op` in doubles: pcgmix_spline_operator_size(n_knots).
 */
int pcgmix_spline_operator_size(int n_knots);
int pcgmix_spline_operator_f64(int T, int n_knots, double* op /* host */);

/* ------------------------------------------------------------------------------------------
 * Partner permutation.                                                              [host]
 *
 * Replaces the per-group shuffle of get_same_label_mix_indices / get_same_wav_mix_indices /
 * get_same_dataset_mix_indices (augmentations.py:500-514, 528-540, 542-556) and the '(mixAll)'
 * draw (augmentations.py:883-884):
 *     mix[group] = random.Random(seed).sample(list(group), len(group))
 * with a FRESH generator per group.  CPython's algorithm is restated exactly: MT19937 seeded by
 * init_by_array over the 32-bit words of |seed|, sample()'s pool branch (always taken when
 * k == n), _randbelow by rejection on getrandbits(n.bit_length()).  Integer results are
 * bit-identical to CPython 3.8-3.12 (checked against `random` in tests/test_host_logic.py).
 *
 *   group_id    host, int32 (B): any labelling of the groups, values in [0, n_groups)
 *   mix         host, int64 (B) out: mix[b] = partner of sample b
 */
int pcgmix_partner_permutation_i64(const int32_t* group_id, int B, int n_groups, uint64_t seed,
                                   int64_t* mix);

/* A partner permutation and its inverse as one int32 block, what a kernel that follows the
 * partners in both directions reads (pcgmix_potes_head_loss_latent_fwd_f32):
 *   out[0..B) = mix, out[B..2B) = inv with inv[mix[b]] = b.                              [host]
 * Returns -3 when an index lies outside [0, B), -4 when mix is not a permutation.              */
int pcgmix_pack_partners_i32(const int64_t* mix, int B, int32_t* out);

/* random.Random(seed).uniform(0, 1) — the probability-gate draw (augmentations.py:869-870). */
double pcgmix_py_uniform01(uint64_t seed);

/* random.Random(seed).randint(0, hi) — the '(rand)' placement offset (augmentations.py:307). */
int64_t pcgmix_py_randint0(uint64_t seed, int64_t hi);

/* ------------------------------------------------------------------------------------------
 * numpy's legacy global random stream, restated (host).  csrc/pcgmix_nprand.hip.
 *
 * Replaces, bit for bit, the draws the reference takes from it in every step:
 *     np.random.seed(seed); lam = np.random.beta(alpha, alpha)        augmentations.py:659-666
 *     np.random.normal(loc=1.0, scale=sigma, size=(B, knot+2, C))     augmentations.py:677
 * `mt_state` is numpy's own generator state — struct { uint32_t key[624]; int pos; }, the address
 * np.random.get_bit_generator().ctypes.state_address — or a private copy of that layout; the
 * functions advance it in place, so the global stream ends where the reference leaves it.
 * numpy's Gaussian cache flag lives outside that struct: counts of normals must be even (the
 * cache is then empty before and after, as it is behind np.random.seed).  All return 0, or 1
 * for arguments outside that contract (the caller then draws with numpy).
 */
/* RandomState.seed(int): mt19937_seed / init_genrand. */
int pcgmix_np_seed(void* mt_state, uint32_t seed);
/* RandomState.beta(a, b) for a <= 1 and b <= 1 (Johnk's algorithm, legacy_beta). */
int pcgmix_np_beta(void* mt_state, double a, double b, double* out);
/* RandomState.normal(loc, scale, n) into out (host, n doubles), n even (legacy_gauss pairs). */
int pcgmix_np_normal_fill(void* mt_state, double loc, double scale, long long n, double* out);

/* One step's (lambda, knots), drawn one step ahead.  pcgmix_npdraw_step returns what
 * seed(seed) -> beta(alpha, alpha) -> normal(1, sigma, n) yield: *lam, and *knots -> n doubles in
 * memory the object owns (valid until the next call on it); `np_state` (numpy's state address, or
 * NULL) receives the generator state behind the draws.  With `lookahead` = L in 1..3 the object
 * owns L + 1 worker threads that draw the blocks of seed + 1 .. seed + L (same alpha, sigma, n)
 * while the caller works on this step; *hit (optional) says whether this call found its block
 * ready.  Contract: 0 < alpha <= 1, n even.  One caller thread per object; a forked child draws
 * inline. */
typedef struct pcgmix_npdraw pcgmix_npdraw;
int pcgmix_npdraw_create(pcgmix_npdraw** out, int lookahead);
void pcgmix_npdraw_destroy(pcgmix_npdraw* d);
int pcgmix_npdraw_step(pcgmix_npdraw* d, uint32_t seed, double alpha, double sigma, long long n,
                       void* np_state, double* lam, const double** knots, int* hit);
/* Blocks found ready / drawn inline so far. */
long long pcgmix_npdraw_stats(pcgmix_npdraw* d, long long* misses);

/* Validate `frames` (int64 (B,5), as the reference's loader yields them) against the signal
 * length and pack the per-step index block read by pcgmix_mix_warp_f32 into `out` (host, e.g.
 * pinned staging): int32 frames[B][5] | mix[B] | rand_off[B][4] (if given) | rect[B][4] (if
 * given).  Returns 0, or 1 = boundaries negative / decreasing, 2 = cycle longer than T (the
 * reference mis-slices silently there, augmentations.py:294-304), 3 = partner index out of
 * range.                                                                            [host] */
int pcgmix_pack_plan_i32(const int64_t* frames, const int64_t* mix, const int32_t* rand_off,
                         const int32_t* rect, int B, int T, int32_t* out);

/* ------------------------------------------------------------------------------------------
 * Fused segment-aware splice (+ optional magnitude warp).                        [device]
 *
 * Replaces, for a whole batch in one launch:
 *   mixup_keepdur_multidim_tensors            augmentations.py:289-337   (plain and '(rand)')
 *   mixup_keepdur_multidim_tensors_salopt     augmentations.py:210-287   (blend part; the
 *                                             displacement comes from pcgmix_salopt_disp_f32)
 *   the per-sample loop around them           augmentations.py:909-917 / 969-977
 *   magnitude_warp + its D2H/H2D round trip   augmentations.py:674-683, 924-928
 *   augmentations2d.mixup_keepdur_multidim_tensors  augmentations2d.py:206-221 (call with
 *                                             C = F rows, T = W columns of the spectrogram)
 *   the 2D mask loops                         augmentations2d.py:320-323, 355-358, 393 (zero_rect)
 *
 * For sample b with partner m = mix_idx[b], heart state k = 0..3:
 *     len1 = frames[b][k+1]-frames[b][k],  len2 = frames[m][k+1]-frames[m][k],  n = min(len1,len2)
 *     o    = off ? min(off[b][k], |len1-len2|) : 0
 *     a    = frames[b][k] + (len1 > len2 ? o : 0)        own-side start
 *     s    = frames[m][k] + (len2 > len1 ? o : 0)        partner-side start
 *     y[b,c,a+i] = x[b,c,a+i]*lam + x[m,c,s+i]*(1-lam)   i = 0..n-1   (fp32 mul, mul, add —
 *                                                        never contracted to an FMA)
 *   everywhere else y = x.  (1-lam) is formed in float32.  Elements whose source index would
 *   fall outside [0,T) are left unblended (the reference would raise on such frames).
 * If `knots` is non-NULL each output is then multiplied by the not-a-knot cubic spline through
 * knots[b,:,c] evaluated at t in float64 (scipy's term order c3 + c2*s + c1*s^2 + c0*s^3 with a
 * running power) and rounded once to float32, as `ret[i] = pat * warper` does.
 *
 *   x, y        device, (B, C, T); y must not alias x
 *   frames      device, int32 (B, 5)
 *   mix_idx     device, int32 (B), values in [0, B)
 *   off         device, int32 (B, 4) >= 0, or NULL
 *   knots       device, float64 (B, n_knots, C) exactly as numpy.random.normal fills it, or NULL
 *   spline_op   device, float64 (pcgmix_spline_operator_size(n_knots)); required iff knots
 *   zero_rect   device, int32 (B, 4) = [row0, row1, col0, col1) per sample, or NULL: outputs with
 *               row0 <= c < row1 and col0 <= t < col1 are written as 0 — the masks that
 *               durmixcutout / durmixtimemask / durmixfreqmask apply after the 2D splice
 *               (augmentations2d.py:309-323, 348-358, 384-394)
 */
int pcgmix_mix_warp_f32(const float* x, float* y,
                        const int32_t* frames, const int32_t* mix_idx, const int32_t* off,
                        float lam,
                        const double* knots, const double* spline_op, int n_knots,
                        const int32_t* zero_rect,
                        int B, int C, int T, pcgmix_stream_t stream);

/* The plain splice (no '(rand)' offsets, no warp, no rectangle) with its index block in the KERNEL
 * ARGUMENTS: frames16 (B,5) and mix16 (B) are HOST arrays of int16 that the launch copies into the
 * kernel's 4 KB argument segment (3 KB used) — the blocks read them with scalar loads, and there is
 * no host-to-device copy in front of the launch.  Needs B <= 256, T <= 32767, T % 4 == 0, x and y
 * 16-byte aligned (BASELINE configs[1]); hipErrorInvalidValue otherwise.  Same arithmetic and
 * results as pcgmix_mix_warp_f32.  pcgmix_augment_plain_f32 takes this path by itself.
 * pcgmix_mix_karg_variant: 1 and the instantiation's unroll if (B, C, T) qualifies, else 0.    */
int pcgmix_mix_karg_f32(const float* x, float* y, const int16_t* frames16, const int16_t* mix16,
                        float lam, int B, int C, int T, pcgmix_stream_t stream);
int pcgmix_mix_karg_variant(int B, int C, int T, int* unroll);

/* ------------------------------------------------------------------------------------------
 * Saliency post-processing.                                                       [device]
 *
 * Replaces saliency.get_saliency_maps(), saliency.py:63-91 (dim == 1), after the model's
 * backward pass: |grad| -> zero t >= frames[b][4] -> sum over channels -> `ksize`-tap Gaussian
 * (weights 1/(sigma*sqrt(2*pi)) * exp(-r^2 / (2 sigma^2)), not renormalised, zero 'same'
 * padding, saliency.py:15-18) -> zero the tail again -> per row (s - min) / max(s - min),
 * NaN -> 0.
 *
 *   grad        device, (B, C, T)
 *   sal         device, (B, T) out
 *   ksize       odd, <= 255 (the reference uses 101); weights are formed on the host in
 *               float64 exactly as gaussian_kernel() does and rounded to float32
 *   sigma       float64, the reference's (12/101)*ksize
 *   T           <= 19000 (the row is staged in LDS)
 */
int pcgmix_saliency_post_f32(const float* grad, const int32_t* frames, float* sal,
                             int ksize, double sigma, int B, int C, int T,
                             pcgmix_stream_t stream);

/* saliency.saliency_map(), saliency.py:147-201, after the model's backward pass, for a batch in
 * one launch (the reference: a Python loop over samples, four interpolate + repeat_interleave
 * calls and a host copy per sample).  As pcgmix_saliency_post_f32 up to the Gaussian, then:
 * the tail is NOT zeroed again (smoothed values up to ksize/2 samples past frames[b][4] stay and
 * take part in the minimum and maximum) -> per row (s - min) / max(s - min), NaN -> 0 -> sal.
 * The four heart states k, [lo, hi) = [f[k], f[k+1]) of length L, are then summarised in
 * n = n_bins[k] values by torch's linear interpolation with align_corners=False (bin_tensor,
 * saliency.py:118-130), all in float32:
 *     scale = float(L) / float(n);  src = max(scale * (i + 0.5f) - 0.5f, 0)
 *     i0 = (int)src;  i1 = min(i0 + 1, L - 1);  l1 = src - i0;  l0 = 1 - l1
 *     value_i = fmaf(l0, s[lo + i0], l1 * s[lo + i1])
 * and every value is held for spb = ceil(L / n) samples:
 *
 *   sal_bins    device, (B, T) out: value_{(t - lo) / spb} for lo <= t < hi, 0 outside [f[0], f[4])
 *               (with L < n only the first L values appear here, all n are reported below)
 *   bin_values  device, (B, N) out, N = n_bins[0] + .. + n_bins[3] (the reference: 1, 4, 1, 8)
 *   bin_frames  device, (B, N + 1) int32 out: lo + i * spb per bin, then f[4]
 *   n_bins      HOST, 4 values >= 1 with N <= 64
 *   ksize       odd, <= 255 (the reference ends up with 57, sigma 7.54, saliency.py:156)
 *
 * grad, frames, sal, T and the refusals as for pcgmix_saliency_post_f32.  frames must be
 * non-decreasing within [0, T] (they are clamped to that for memory safety); a state of length 0
 * reports zeros — the reference's interpolate raises there, and so does the Python layer.
 * The same bits on every call.                                                       [device] */
int pcgmix_saliency_map_f32(const float* grad, const int32_t* frames, float* sal, float* sal_bins,
                            float* bin_values, int32_t* bin_frames, int ksize, double sigma,
                            const int32_t* n_bins, int B, int C, int T, pcgmix_stream_t stream);

/* The spectrogram branch of the same function (saliency.py:93-113, dim = 2).  grad (B, F, W)
 * float32 (the single image channel folded away), frames (B,5) in spectrogram columns, sal (B, W):
 * |grad| -> columns t >= f[4] zeroed -> sum over the F frequency rows -> `ksize`-tap Gaussian along
 * time (the reference: 11 taps, sigma 1) with zero 'same' padding -> tail zeroed -> min/max
 * normalisation over the cycle's own columns [0, f[4]) ONLY -> NaN -> 0.  W <= 1024.  [device] */
int pcgmix_saliency_post2d_f32(const float* grad, const int32_t* frames, float* sal, int ksize,
                               double sigma, int B, int F, int W, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Saliency-optimal displacement search.                                           [device]
 *
 * Replaces optimal_displacement_max_envelope (mode 0, augmentations.py:60-93) and
 * optimal_displacement_max_sum (mode 1, augmentations.py:95-128) for every (sample, state):
 * disp[b][k] = first strict argmax over d in [0, |len1-len2|] of the float32 objective,
 * evaluated in numpy's pairwise-summation order so that the integer result is the
 * reference's; 0 where the two lengths agree.
 *
 *   sal         device, (B, T) saliency maps
 *   disp        device, int32 (B, 4) out — feeds pcgmix_mix_warp_f32's `off`
 *   workspace   device, pcgmix_salopt_workspace_bytes(B) bytes, 8-byte aligned: the candidates of
 *               one (sample, state) are shared out over several blocks; their partial arg-maxima
 *               meet here (greatest value, smallest displacement on ties = first strict maximum)
 *   max_len     the longest heart state of the batch in samples, max_k,b(frames[b][k+1] -
 *               frames[b][k]) — the caller has `frames` on the host — or 0 for "unknown" (= T).
 *               It sizes the blocks' LDS (2 * max_len floats): the smaller, the more blocks a CU
 *               holds.  States longer than max_len are cut to it (memory safety only).
 *   B <= 65535, T <= 19000
 */
long long pcgmix_salopt_workspace_bytes(int B);
int pcgmix_salopt_disp_f32(const float* sal, const int32_t* frames, const int32_t* mix_idx,
                           float lam, int mode, int32_t* disp, void* workspace, int max_len, int B,
                           int T, pcgmix_stream_t stream);
/* The same search for a caller that ALSO holds the boundaries and the partners on the host — the
 * reference's own situation: mixup_keepdur_multidim_tensors_salopt receives `frames` and the partner
 * index as CPU arrays (augmentations.py:210-287).  frames_host (B,5) / mix_host (B): host copies of
 * `frames` / `mix_idx` (same values: the device copies stay the ones the kernel reads).  With them
 * (B <= 256) the launch holds only the blocks that have candidates, ordered by the length of their
 * chain of sums, longest first, in the kernel arguments; either NULL: as pcgmix_salopt_disp_f32.
 * Results are identical.                                                                        */
int pcgmix_salopt_disp_hosted_f32(const float* sal, const int32_t* frames, const int32_t* mix_idx,
                                  float lam, int mode, int32_t* disp, void* workspace, int max_len,
                                  int B, int T, pcgmix_stream_t stream, const int32_t* frames_host,
                                  const int32_t* mix_host);
/* Host only: that launch plan, for inspection and tests.  ids_out receives up to `cap` block ids
 * ((sample << 4) | (state << 2) | slice: slice z of pair (sample, state) holds the displacements
 * 256 z .. 256 z + 255, + 1024, ...) in launch order — longest chain of sums first; a pair without a
 * search (equal lengths) is represented by its slice 0.  Returns the number of blocks, 0 when no plan
 * is made for this shape (B > 256 or more than 1408 blocks: the full grid is launched), < 0 for
 * bad arguments.                                                                        [host]   */
int pcgmix_salopt_plan(const int32_t* frames_host, const int32_t* mix_host, int B, int T, int max_len,
                       uint16_t* ids_out, int cap);
/* The saliency-guided splice — mixup_keepdur_multidim_tensors_salopt for the whole batch
 * (augmentations.py:210-287 with :60-128, the loop at :909-917, magnitude_warp :674-683) — in one
 * call: the search above, then pcgmix_mix_warp_f32's kernel, whose blocks reduce the search's
 * per-block results for their own sample themselves (no launch in between).  knots / spline_op /
 * n_knots as in pcgmix_mix_warp_f32 (NULL, NULL, 0: no warp).  disp_out: NULL, or int32 (B,4) that
 * receives the displacements from a small launch BEHIND the splice.                            */
int pcgmix_salopt_mix_warp_f32(const float* x, float* y, const float* sal, const int32_t* frames,
                               const int32_t* mix_idx, float lam, int mode, const double* knots,
                               const double* spline_op, int n_knots, void* workspace, int max_len,
                               int32_t* disp_out, int B, int C, int T, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Log-mel front end.                                                    [host tables + device]
 *
 * Replaces the offline librosa pipeline of databuilder.ipynb cell 6:19-23, 81-101, 127-142
 * (melspectrogram -> power_to_db(ref=np.max) -> (x-mean)/std -> slice the cycle's columns ->
 * zero-pad to W columns), on device.  librosa 0.9.2 semantics restated (centred frames, periodic
 * Hann of n_fft, float64 transform rounded to complex64, power 2, Slaney mel scale and
 * normalisation, amin 1e-10, top_db 80); parity with librosa itself is UNPINNED (librosa is not
 * available offline and the reference stores no spectrogram).  One point of that restatement is
 * open and therefore a parameter: `pad_mode` of the centred frames, 0 = zeros (numpy 'constant')
 * or 1 = 'reflect'.
 *
 * Two granularities:
 *   pcgmix_logmel_f32             one transform per heart-cycle item of a batch; `ref` is the
 *                                 item's own maximum (what a per-batch transform of cut cycles
 *                                 can see).
 *   pcgmix_logmel_recordings_f32  the reference's order of operations: ONE transform over each
 *                                 whole recording, `ref` = the recording's maximum (cell 6:93),
 *                                 then cycle c keeps the recording's columns
 *                                 [round(f0*n_frames/len(y)), round(f4*n_frames/len(y)))
 *                                 (cell 6:101, 134), zero-padded to W after normalisation.
 *
 * pcgmix_logmel_tables builds, on the host, everything that does not depend on the data: the
 * windowed DFT matrix in matrix-core operand order, the mel filter bank and each filter's
 * non-zero span (pcgmix_logmel_tables_size bytes).  The caller copies that blob to the device
 * once and passes it to every pcgmix_logmel_f32 call with the same (n_fft, n_mels).
 *
 *   x           device, (B, T) one channel per row
 *   frames      device, int32 (B, 5) waveform boundaries; columns >= round(f4 * n_frames / T)
 *               are zero-filled after normalisation
 *   tables      device, the blob above
 *   spec        device, (B, n_mels, W) out
 *   frames_out  device, int32 (B, 5) out or NULL: boundaries in spectrogram columns
 *
 * Supported shapes (everything else: hipErrorInvalidValue, nothing is launched):
 *   n_fft >= 4 and a multiple of 4; hop >= 1 (hop need not be n_fft/4); n_mels >= 1; W >= 1 (W may
 *   exceed the 1 + T/hop frames of an item: the columns beyond them are zero); fmin < fmax, sr > 0;
 *   n_fft/2 < T; std != 0; pad_mode 0 or 1; and one block's LDS plan (pcgmix_logmel_lds_layout:
 *   padded row + power spectrogram of ceil32(1 + T/hop) frames + the n_mels x W image + tables) must
 *   fit 158 KB.  The reference's shapes (n_fft 136 / T 5000 and n_fft 68 / T 2500, any n_mels x W up to
 *   128 x 128) fit; n_fft = 272 at T = 10000 (a 4 kHz cycle) does not and is refused.  The per-recording
 *   entry point transforms tiles of pcgmix_logmel_tile_frames() frames, so its plan does not depend
 *   on the recording's length or on W.  Filters of any width are supported (up to 4 bins from LDS,
 *   wider ones read their weights from the table), as are banks that leave bins unread at either end.
 */
long long pcgmix_logmel_tables_size(int n_fft, int n_mels);
int pcgmix_logmel_tables(int n_fft, int n_mels, float fmin, float fmax, float sr, void* out /* host */);
int pcgmix_logmel_f32(const float* x, const int32_t* frames, const void* tables, float* spec,
                      int32_t* frames_out, int B, int T, int n_fft, int hop, int n_mels,
                      float mean, float std, int W, int pad_mode, pcgmix_stream_t stream);
/* The same for a caller that holds the boundaries on the host (as the reference does: numpy
 * arrays, databuilder.ipynb cell 6:101): frames_host (B,5) int32 HOST memory.  B <= 1024 and
 * T <= 32767: the cycle ends travel in the kernel arguments — no upload, no copy kernel in front
 * of the launch; otherwise hipErrorInvalidValue (upload, then pcgmix_logmel_f32).               */
int pcgmix_logmel_hostframes_f32(const float* x, const int32_t* frames_host, const void* tables,
                                 float* spec, int B, int T, int n_fft, int hop, int n_mels,
                                 float mean, float std, int W, int pad_mode, pcgmix_stream_t stream);

/* Per-recording front end.  All pointers device.  The column bookkeeping (which is integer work
 * on a handful of numbers per cycle: n_frames = 1 + len/hop, Python round()) is the caller's; the
 * kernels take it as descriptor tables:
 *   y            recordings back to back, float32
 *   rec_off      int64 (R): first sample of recording r in y;  rec_len int32 (R): its length
 *   tiles        int32 (n_tiles, 4): {recording, first frame, frames in this tile
 *                (<= pcgmix_logmel_tile_frames()), absolute scratch column of that first frame};
 *                the tiles of a recording cover its frames 0 .. n_frames-1 once
 *   cycles       int32 (n_cycles, 4): {recording, absolute scratch column of the cycle's first
 *                column, number of columns kept (clipped to W), 0}
 *   db_scratch   float32 (n_mels, scratch_cols) workspace: un-referenced dB of every frame
 *   ref_pow      uint32 (R) workspace: bit pattern of the recording's maximum mel power
 *   spec         float32 (n_cycles, n_mels, W) out
 * Three launches: zero ref_pow; transform + mel + dB per tile (f64 matrix cores), maximum folded
 * in with an unsigned atomicMax (non-negative floats order like their bit patterns: the result is
 * order-independent); slice / reference / clip / normalise / pad per cycle.
 */
int pcgmix_logmel_tile_frames(void);
/* Host only: the LDS plan of one block of the per-cycle kernel (mode 0, 1 + T/hop frames, with the
 * n_mels x W dB image) or of the per-recording tile kernel (mode 1, pcgmix_logmel_tile_frames()
 * frames, no image; T is ignored), for inspection and tests.  out receives 20 int32:
 *   [2i], [2i+1]  byte offset and size of region i = 0..6: padded row, power spectrogram, dB image,
 *                 filter records, coefficients of the VALU rows, window, partial sums of the VALU rows.
 *                 The partial sums lie over the dB image (same offset) when the image holds at least
 *                 one k part of every 64-frame group at the table's row count; otherwise, and in
 *                 mode 1, they have a region of their own.  All other regions are disjoint.
 *   [14] total bytes   [15] bytes of partial sums the kernel writes when n_left_used rows are in
 *   use (n_left_used < 0: all the table has; always <= [13])   [16] frames, padded to 32
 *   [17] rows the table holds for the VALU   [18] 1 when the entry points accept the shape
 *   (total <= [19]), else 0   [19] the limit, 158 KB.
 * A shape of which one region alone exceeds the limit reports total = INT32_MAX, [18] = 0 and no
 * regions.  Returns hipErrorInvalidValue for arguments the entry points refuse outright.   [host] */
int pcgmix_logmel_lds_layout(int mode, int T, int n_fft, int hop, int n_mels, int W, int n_left_used,
                             int32_t* out);
int pcgmix_logmel_recordings_f32(const float* y, const int64_t* rec_off, const int32_t* rec_len,
                                 int R, const int32_t* tiles, int n_tiles, const int32_t* cycles,
                                 int n_cycles, const void* tables, float* db_scratch,
                                 long long scratch_cols, uint32_t* ref_pow, float* spec, int n_fft,
                                 int hop, int n_mels, float mean, float std, int W, int pad_mode,
                                 pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Potes 1D-CNN convolutional branch, fused.                                         [device]
 *
 * Replaces, for the N = 4*B band rows of a batch, CNN_potes.cnn1 (models.py:359-381, 444-455):
 *     Conv1d(1->8,k5,pad1) + ReLU + MaxPool1d(2) -> Conv1d(8->4,k5,pad1) + ReLU + MaxPool1d(2)
 * (the Dropout(0.25) that follows is applied by the caller).  Weight layouts are torch's:
 * w1 (8,1,5), b1 (8), w2 (4,8,5), b2 (4).
 *
 *   pcgmix_potes_out_len(T)        pooled output length P2 (1248 for T = 5000, 623 for 2500)
 *   pcgmix_potes_stack_fwd_f32     x (N,T) -> h2 (N,4,P2)
 *   pcgmix_potes_bwd_blocks(N,T)   G = number of partial rows the backward needs
 *   pcgmix_potes_stack_bwd_f32     x, dL/dh2 (N,4,P2) -> grads[212] = [gw1(40) | gb1(8) |
 *                                  gw2(160) | gb2(4)]; `partial` is caller-provided scratch of
 *                                  G*212 floats.  The forward is recomputed tile by tile.
 *   pcgmix_potes_stack_input_grad_f32   x, dL/dh2 -> dL/dx (N,T): what saliency.py:52-61 needs
 *                                  (the class score differentiated w.r.t. the input); also
 *                                  recomputes the forward, keeps nothing from it.
 * All pointers device; float32.  Both forwards run on the f32 matrix cores
 * (v_mfma_f32_4x4x1_16b_f32: every output is an in-order fmaf chain from the bias over (input
 * channel, tap) — exact f32); the recomputing backward kernels and the layer-1 recompute of the
 * mask-based weight gradient use a VALU summation order and agree with it to float rounding.
 */
int pcgmix_potes_out_len(int T);
int pcgmix_potes_bwd_blocks(int N, int T);
int pcgmix_potes_stack_fwd_f32(const float* x, const float* w1, const float* b1, const float* w2,
                               const float* b2, float* h2, int N, int T, pcgmix_stream_t stream);
int pcgmix_potes_stack_input_grad_f32(const float* x, const float* grad_h2, const float* w1,
                                      const float* b1, const float* w2, const float* b2,
                                      float* grad_x, int N, int T, pcgmix_stream_t stream);
int pcgmix_potes_stack_bwd_f32(const float* x, const float* grad_h2, const float* w1,
                               const float* b1, const float* w2, const float* b2, float* partial,
                               float* grads, int N, int T, pcgmix_stream_t stream);
/* The same three passes with the forward's ReLU / max-pool routing SAVED instead of recomputed
 * (what autograd keeps for nn.ReLU / nn.MaxPool1d in models.py:359-365, at 2 bits or a byte per
 * position instead of the activations):
 *   m2   uint8 (N, 4, ceil(P2/4))  second layer: per pooled output 2 bits — 0 ReLU-dead, 1 the
 *        first conv output of the pooled pair won, 2 the second; four outputs per byte
 *   s1   uint8 (N, 8, P1/4 + 1)    first layer: the same selector, four positions per byte
 *        (position q in bits 2*((q+1)&3) of byte (q+1)>>2); only the input gradient needs it
 *        (pass NULL to the forward otherwise)
 *   sizes in bytes: pcgmix_potes_mask_bytes(N, T, layer = 2 or 1)
 *   pcgmix_potes_stack_fwd_save_f32        the forward above + m2 (+ s1)
 *   pcgmix_potes_stack_bwd_mask_f32        weight gradients: recomputes layer 1 only
 *   pcgmix_potes_stack_input_grad_mask_f32 dL/dx from grad_h2, m2, s1 and the weights alone:
 *                                          no forward recompute at all
 * Gradients flow exactly where the forward's maxima were (the recomputing kernels re-derive the
 * routing with a different summation order and can differ at exact near-ties).
 *
 * rnd_out != NULL: the forward launch also fills rnd_out[0 .. rnd_bytes) (16-byte aligned, a
 * multiple of 16) with the uniformly random bytes the head's dropouts read (mask1 / mask2 of
 * pcgmix_potes_head_*): 32-bit word w = a keyed counter hash of w.  The 64-bit key is `key`, or —
 * key_dev != NULL — the two 32-bit words (low, high) at key_dev in DEVICE memory: for training
 * steps captured in a hipGraph, nn.Dropout's mask generation (models.py:364, 380) without an RNG
 * launch per replay — the key changes per step, the graph does not.  rnd_out == NULL: nothing is
 * filled (rnd_bytes, key_dev, key ignored).
 */
long long pcgmix_potes_mask_bytes(int N, int T, int layer);
int pcgmix_potes_stack_fwd_save_f32(const float* x, const float* w1, const float* b1,
                                    const float* w2, const float* b2, float* h2, uint8_t* m2,
                                    uint8_t* s1, int N, int T, uint8_t* rnd_out, long long rnd_bytes,
                                    const uint32_t* key_dev, uint64_t key, pcgmix_stream_t stream);
int pcgmix_potes_stack_bwd_mask_f32(const float* x, const float* grad_h2, const uint8_t* m2,
                                    const float* w1, const float* b1, const float* w2,
                                    const float* b2, float* partial, float* grads, int N, int T,
                                    pcgmix_stream_t stream);
int pcgmix_potes_stack_input_grad_mask_f32(const float* grad_h2, const uint8_t* m2,
                                           const uint8_t* s1, const float* w1, const float* w2,
                                           float* grad_x, int N, int T, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Narrow Potes conv stacks (the reference's model-size ladder).                      [device]
 *
 * The same chain on the N = 4*B band rows x (N,T) for the two small models of models.py:352-356
 * (CNN_potes_tenpercent_TS, layers [2,1]; CNN_potes_twopercent_TS, layers [1,1]) over
 * models.py:359-381:
 *     Conv1d(1->C1,k5,pad1) + ReLU + MaxPool1d(2) -> Conv1d(C1->C2,k5,pad1) + ReLU + MaxPool1d(2)
 * (C1,C2) in {(1,1), (2,1)}; torch weight layouts w1 (C1,1,5), b1 (C1), w2 (C2,C1,5), b2 (C2);
 * float32, T >= 14, P2 = pcgmix_potes_out_len(T).  Plain VALU kernels (csrc/pcgmix_potes_narrow.hip):
 * every conv output is an in-order fmaf chain from the bias over (input channel, tap).
 *
 *   pcgmix_potes_narrow_supported(C1,C2)   1 for (1,1) and (2,1), else 0
 *   pcgmix_potes_narrow_grad_len(C1,C2)    5*C1 + C1 + 5*C1*C2 + C2 (12, 23); 0 if unsupported
 *   pcgmix_potes_narrow_bwd_blocks         G = partial rows the weight gradient needs
 *   pcgmix_potes_narrow_mask_bytes         bytes of m2 (layer = 2) / s1 (layer = 1)
 *                                          (both helpers: 0 for an unsupported (C1,C2), T < 14,
 *                                          N <= 0 or N > 65535 — whatever the launching entry
 *                                          points refuse)
 *   pcgmix_potes_narrow_fwd_f32            ONE launch: h2 (N,C2,P2); m2 != NULL: + the second layer's
 *                                          routing; s1 != NULL: + the first layer's (only the input
 *                                          gradient reads it).  m2 and s1 are the 2-bit encodings
 *                                          defined above with 8 -> C1 and 4 -> C2: m2 uint8
 *                                          (N, C2, ceil(P2/4)), s1 uint8 (N, C1, P1/4 + 1).
 *                                          m2 == s1 == rnd_out == NULL: the inference forward.
 *                                          rnd_out, rnd_bytes, key_dev, key: exactly as in
 *                                          pcgmix_potes_stack_fwd_save_f32 — the same hash, the
 *                                          same checks, the same bytes for a key and a length.
 *   pcgmix_potes_narrow_bwd_mask_f32       weight gradients: recomputes layer 1 from x, routes
 *                                          through m2, writes `partial` (G, grad_len) and reduces
 *                                          it in a fixed order (no float atomics) into grads =
 *                                          [gw1 | gb1 | gw2 | gb2].  grads == NULL (the deferred
 *                                          reduction of the [8,4] kernels) is NOT supported:
 *                                          hipErrorInvalidValue.
 *   pcgmix_potes_narrow_input_grad_mask_f32  dL/dx (N,T) from grad_h2, m2, s1 and the weights
 *                                          alone; every element of grad_x is written.
 * Every entry point returns hipErrorInvalidValue, launching nothing and leaving its outputs
 * untouched, for an unsupported (C1,C2), T < 14, N < 0 (or > 65535), a NULL required pointer or a
 * misaligned rnd_out; N == 0 succeeds without a launch.  All are legal on a capturing stream.
 */
int pcgmix_potes_narrow_supported(int C1, int C2);
int pcgmix_potes_narrow_grad_len(int C1, int C2);
int pcgmix_potes_narrow_bwd_blocks(int N, int T, int C1, int C2);
long long pcgmix_potes_narrow_mask_bytes(int N, int T, int C1, int C2, int layer);
int pcgmix_potes_narrow_fwd_f32(const float* x, const float* w1, const float* b1, const float* w2,
                                const float* b2, float* h2, uint8_t* m2, uint8_t* s1, int N, int T,
                                int C1, int C2, uint8_t* rnd_out, long long rnd_bytes,
                                const uint32_t* key_dev, uint64_t key, pcgmix_stream_t stream);
int pcgmix_potes_narrow_bwd_mask_f32(const float* x, const float* grad_h2, const uint8_t* m2,
                                     const float* w1, const float* b1, const float* w2,
                                     const float* b2, float* partial, float* grads, int N, int T,
                                     int C1, int C2, pcgmix_stream_t stream);
int pcgmix_potes_narrow_input_grad_mask_f32(const float* grad_h2, const uint8_t* m2,
                                            const uint8_t* s1, const float* w1, const float* w2,
                                            float* grad_x, int N, int T, int C1, int C2,
                                            pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Big Potes conv stacks (the wide end of the reference's model-size ladder).         [device]
 *
 * The same chain on the N = 4*B band rows x (N,T) for the two big models of models.py:339-343
 * (CNN_potes_big64and32_TS, layers [64,32]; CNN_potes_big128and64_TS, layers [128,64]) over
 * models.py:359-381:
 *     Conv1d(1->C1,k5,pad1) + ReLU + MaxPool1d(2) -> Conv1d(C1->C2,k5,pad1) + ReLU + MaxPool1d(2)
 * (C1,C2) in {(64,32), (128,64)}; torch weight layouts as above; float32, T >= 14,
 * P2 = pcgmix_potes_out_len(T).  csrc/pcgmix_potes_big.hip: the first layer on the VALU into LDS,
 * the second layer and both transposed products as implicit GEMMs on v_mfma_f32_32x32x2_f32 — exact
 * float32, every second-layer output the chain "b2, then (input channel, tap) in order".
 *
 *   pcgmix_potes_big_supported(C1,C2)      1 for (64,32) and (128,64), else 0
 *   pcgmix_potes_big_grad_len(C1,C2)       5*C1 + C1 + 5*C1*C2 + C2 (10656, 41792); 0 if unsupported
 *   pcgmix_potes_big_bwd_blocks            G = partial rows the weight gradient needs
 *   pcgmix_potes_big_mask_bytes            bytes of m2 (layer = 2) / s1 (layer = 1)
 *                                          (both helpers: 0 for whatever the launching entry points
 *                                          refuse, as in the narrow section)
 *   pcgmix_potes_big_fwd_f32               ONE launch: h2 (N,C2,P2); m2 != NULL: + m2 uint8
 *                                          (N, C2, ceil(P2/4)); s1 != NULL: + s1 uint8
 *                                          (N, C1, P1/4 + 1) (only the input gradient reads it); the
 *                                          encodings defined above with 8 -> C1 and 4 -> C2.
 *                                          rnd_out, rnd_bytes, key_dev, key: exactly as in
 *                                          pcgmix_potes_narrow_fwd_f32 — the same hash, the same
 *                                          checks, the same bytes for a key and a length.
 *   pcgmix_potes_big_bwd_mask_f32          weight gradients: recomputes layer 1 from x, routes
 *                                          through m2; two persistent launches write `partial`
 *                                          (G, grad_len) — gw2 | gb2, then gw1 | gb1 through the
 *                                          transposed second layer — and a third reduces it in a
 *                                          fixed order (no float atomics) into grads =
 *                                          [gw1 | gb1 | gw2 | gb2].  grads == NULL is NOT supported:
 *                                          hipErrorInvalidValue.
 *   pcgmix_potes_big_input_grad_mask_f32   dL/dx (N,T) from grad_h2, m2, s1 and the weights alone;
 *                                          every element of grad_x is written.
 * The refusal contract of the narrow section holds word for word: hipErrorInvalidValue, nothing
 * launched and no output touched, for an unsupported (C1,C2), T < 14, N < 0 (or > 65535), a NULL
 * required pointer or a misaligned rnd_out; N == 0 succeeds without a launch.  All are legal on a
 * capturing stream.  PCGMIX_POTES_BIG_BWD_BLOCKS in the environment caps G (tuning runs, tests).
 */
int pcgmix_potes_big_supported(int C1, int C2);
int pcgmix_potes_big_grad_len(int C1, int C2);
int pcgmix_potes_big_bwd_blocks(int N, int T, int C1, int C2);
long long pcgmix_potes_big_mask_bytes(int N, int T, int C1, int C2, int layer);
int pcgmix_potes_big_fwd_f32(const float* x, const float* w1, const float* b1, const float* w2,
                             const float* b2, float* h2, uint8_t* m2, uint8_t* s1, int N, int T,
                             int C1, int C2, uint8_t* rnd_out, long long rnd_bytes,
                             const uint32_t* key_dev, uint64_t key, pcgmix_stream_t stream);
int pcgmix_potes_big_bwd_mask_f32(const float* x, const float* grad_h2, const uint8_t* m2,
                                  const float* w1, const float* b1, const float* w2, const float* b2,
                                  float* partial, float* grads, int N, int T, int C1, int C2,
                                  pcgmix_stream_t stream);
int pcgmix_potes_big_input_grad_mask_f32(const float* grad_h2, const uint8_t* m2, const uint8_t* s1,
                                         const float* w1, const float* w2, float* grad_x, int N,
                                         int T, int C1, int C2, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Skinny linear layer forward (the Potes head's `dimreduc`, models.py:376, 430).    [device]
 *
 *   z (B,O) = h (B,K) . W (O,K)^T + bias (O)      O in {8, 16, 20}, K % 4 == 0
 * Split-K with a deterministic two-stage reduction; `partial` is caller-provided scratch of
 * pcgmix_skinny_linear_splits(B,K) * B * O floats.  h and W must be 16-byte aligned.
 */
int pcgmix_skinny_linear_splits(int B, int K);
int pcgmix_skinny_linear_fwd_f32(const float* h, const float* W, const float* bias, float* partial,
                                 float* z, int B, int K, int O, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gradient value clipping + Adam update of one parameter tensor.                    [device]
 *
 * Replaces nn.utils.clip_grad_value_(…, grad_clip) followed by torch.optim.Adam.step() with L2
 * weight decay (train_model.py:557-558, 404-407, 566) for one tensor, in one pass:
 *   g = clamp(g, -clip, clip) (clip <= 0: no clipping) + weight_decay * p
 *   m = m + (1-beta1)(g - m);  v = beta2 v + (1-beta2) g^2
 *   p -= lr / (1-beta1^step) * m / (sqrt(v) / sqrt(1-beta2^step) + eps)          step >= 1
 * p, m, v are updated in place; g is read only.
 */
int pcgmix_adam_clip_f32(float* p, const float* g, float* m, float* v, long long n, float clip,
                         float lr, float beta1, float beta2, float eps, float weight_decay,
                         long long step, pcgmix_stream_t stream);

/* The same update for n_tensors parameter tensors in one launch (one per 32 tensors).  p, g, m,
 * v are HOST arrays of n_tensors device pointers, n the HOST array of element counts; all tensors
 * share the hyper-parameters and the step number (one torch param group).                    */
int pcgmix_adam_clip_multi_f32(int n_tensors, float* const* p, const float* const* g,
                               float* const* m, float* const* v, const long long* n, float clip,
                               float lr, float beta1, float beta2, float eps, float weight_decay,
                               long long step, pcgmix_stream_t stream);

/* The multi-tensor update with its eight scalars in DEVICE memory, for a launch captured in a
 * hipGraph (OneCycleLR moves lr and beta1 every step, the bias corrections move with `step`:
 * kernel arguments would be frozen at capture).  pcgmix_adam_hyper computes the eight floats on
 * the host exactly as pcgmix_adam_clip_multi_f32 does internally — {clip, weight_decay, 1-beta1,
 * beta2, 1-beta2, lr/(1-beta1^step), 1/sqrt(1-beta2^step), eps} — and the caller gets them to
 * hyper_dev before the replay (e.g. with pcgmix_ctx_set_payload).                              */
int pcgmix_adam_hyper(float clip, float lr, float beta1, float beta2, float eps, float weight_decay,
                      long long step, float* out8);
int pcgmix_adam_clip_multi_dev_f32(int n_tensors, float* const* p, const float* const* g,
                                   float* const* m, float* const* v, const long long* n,
                                   const float* hyper_dev, pcgmix_stream_t stream);
/* The same update with the Potes conv stack's gradient reduction folded in (one launch less at
 * the end of a captured training step): pcgmix_potes_stack_bwd_mask_f32 called with grads = NULL
 * leaves its G x 212 partial rows un-reduced; this launch carries 212 extra blocks, each of which
 * sums one column in pcgmix_potes_reduce_f32's order (same bits), stores it at grads[e] and updates
 * the element of the tensor whose gradient pointer g[i] lies inside grads[0 .. 212) (such tensors
 * are updated by those blocks only).  n_tensors <= 32.  pcgmix_potes_reduce_f32 is the reduction
 * alone (what pcgmix_potes_stack_bwd_mask_f32 launches when grads != NULL).                      */
int pcgmix_adam_clip_multi_reduce_dev_f32(int n_tensors, float* const* p, const float* const* g,
                                          float* const* m, float* const* v, const long long* n,
                                          const float* hyper_dev, const float* partial, float* grads,
                                          int G, pcgmix_stream_t stream);
int pcgmix_potes_reduce_f32(const float* partial, float* grads, int G, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gradient value clipping + SGD update of all parameter tensors of a model.          [device]
 *
 * Replaces nn.utils.clip_grad_value_(…, grad_clip) followed by torch.optim.SGD.step()
 * (train_model.py:404-405, 557-558, 566; dampening 0, no nesterov, no maximize) in one launch per
 * 32 tensors, with torch's _single_tensor_sgd order of roundings:
 *   g = clamp(g, -clip, clip)              (clip <= 0: no clipping)
 *   g = fma(weight_decay, p, g)            (weight_decay != 0)
 *   b = rn(momentum * b) + g;  g = b       (momentum != 0; two roundings, not an fma)
 *   p = fma(-lr, g, p)
 * A zero buffer b makes the first step torch's clone(grad).  p, g, m are HOST arrays of n_tensors
 * device pointers (m: the momentum buffers), n the HOST array of element counts; p and m are
 * updated in place, g is read only.  With momentum == 0 the buffers are neither read nor written
 * and m (or any m[i]) may be NULL; with momentum != 0 a NULL m[i] of a non-empty tensor is
 * hipErrorInvalidValue.  Negative n[i], NULL tables: hipErrorInvalidValue; empty tensors are skipped.
 */
int pcgmix_sgd_clip_multi_f32(int n_tensors, float* const* p, const float* const* g,
                              float* const* m, const long long* n, float clip, float lr,
                              float momentum, float weight_decay, pcgmix_stream_t stream);

/* The same update with its scalars in DEVICE memory, for a launch captured in a hipGraph: with
 * OneCycleLR the reference's SGD runs move lr AND momentum on every step (train_model.py:404-405,
 * 557-558, 566).  pcgmix_sgd_hyper writes the eight floats {clip, weight_decay, momentum, lr, 0, 0,
 * 0, 0} (the size of pcgmix_adam_hyper's block; the last four are not read).  The table m must be
 * given; a NULL m[i] is legal only while the momentum word stays 0 — the kernel updates such a
 * tensor without momentum whatever the word says.                                              */
int pcgmix_sgd_hyper(float clip, float lr, float momentum, float weight_decay, float* out8);
int pcgmix_sgd_clip_multi_dev_f32(int n_tensors, float* const* p, const float* const* g,
                                  float* const* m, const long long* n, const float* hyper_dev,
                                  pcgmix_stream_t stream);
/* ... and with the Potes conv stack's gradient reduction folded in, exactly as
 * pcgmix_adam_clip_multi_reduce_dev_f32 does it (train_model.py:404-405, 557-558, 566): 212 extra
 * blocks sum the partial columns in pcgmix_potes_reduce_f32's order (same bits), store grads[e] and
 * update the element that owns it.  n_tensors <= 32, G >= 1.                                    */
int pcgmix_sgd_clip_multi_reduce_dev_f32(int n_tensors, float* const* p, const float* const* g,
                                         float* const* m, const long long* n,
                                         const float* hyper_dev, const float* partial, float* grads,
                                         int G, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Potes classifier head, forward and backward.                                       [device]
 *
 * Replaces CNN_potes' Dropout(.25) -> Flatten/concat -> dimreduc Linear(K->20) -> ReLU ->
 * Dropout(.5) -> Linear(20->C) (models.py:364, 376-381, 456-465) and their autograd twins.
 *   x       (B,K) features BEFORE the Dropout(.25) of the conv branch (K % 4 == 0, 16-byte aligned)
 *   mask1   random bits or NULL (no dropout): element e = b*K + k owns bits1 (1, 2, 4 or 8)
 *           consecutive bits at bit offset e*bits1 and is kept iff their value >= thr1, kept
 *           values times scale1.  bits1 = 8, thr1 = 1 reads a 0/1 byte mask; uniformly random bits
 *           with thr1 = 2^bits1 * p drop with probability p exactly (p = 0.25: 2 bits, thr 1;
 *           scale = 1/(1-p)).  4-byte aligned.  Applied where x is read: no separate pass.
 *   w1,b1   dimreduc (20,K), (20) — b1 may be NULL;   w2,b2  linear (C,20), (C), C <= 8
 *   mask2   (B,20) bytes, kept iff byte >= thr2, NULL = no dropout (eval); scale2 as scale1
 *   partial workspace, pcgmix_skinny_linear_splits(B,K) * B * 20 floats
 *   z       (B,20) out: dimreduc output incl. bias, kept for backward;  logits (B,C) out
 * Backward, given dlogits (B,C) and the SAME x, mask1, mask2:
 *   dz (B,20) workspace/out (gradient at z; 16-byte aligned); dw2 (C,20), db2 (C, may be NULL), db1 (20, may be
 *   NULL), dw1 (20,K; may be NULL when dx is given: frozen weights, e.g. the saliency model — x is
 *   then not read at all), dx (B,K, may be NULL) = gradient at the features BEFORE Dropout(.25).
 * x is read once and dx written once (9 bytes per feature element); reductions are fixed-order.
 */
int pcgmix_potes_head_fwd_f32(const float* x, const uint8_t* mask1, float scale1, int thr1,
                              int bits1, const float* w1, const float* b1, const uint8_t* mask2, float scale2,
                              int thr2, const float* w2, const float* b2, float* partial, float* z,
                              float* logits, int B, int K, int C, pcgmix_stream_t stream);
int pcgmix_potes_head_bwd_f32(const float* dlogits, const float* z, const uint8_t* mask2,
                              float scale2, int thr2, const float* w2, const float* x,
                              const uint8_t* mask1, float scale1, int thr1, int bits1,
                              const float* w1, float* dz, float* dw2, float* db2, float* db1,
                              float* dw1, float* dx,
                              int B, int K, int C, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation pass.                                                                    [device]
 *
 * The reference's test_data_accuracy (train_model.py:591-670): per batch of heart cycles the
 * softmax of the logits (:602) and the criterion (:608-609), per recording the mean of its cycles'
 * softmax rows (np.mean(arr, axis=0), :627) or, under '(class_majority)', the bincount of their
 * arg-max votes (:634-647).  No atomics; every sum in a stated order; 1 <= C <= 8.
 *
 * Row rule (one device function behind both forward entry points), for logits l[0..C):
 *   m = max_c l_c;  e_c = expf(l_c - m);  s = sum_c e_c (c ascending);  p_c = e_c / s
 *   loss = -((l_y - m) - logf(s)) for the label byte y (CELoss with a one-hot target, :45-54)
 *   vote = lowest index of the maximum of the float32 p (np.argmax of the softmax OUTPUT, :637)
 *
 * pcgmix_eval_rows_f32: logits (B,C) of any model -> prob (B,C), loss_rows (B) (0 when labels is
 *   NULL), vote (B) bytes.  labels: (B) bytes or NULL; a byte >= C gives loss 0 (the host refuses
 *   such labels).  B == 0 returns 0 and launches nothing; C outside 1..8: hipErrorInvalidValue.
 *
 * pcgmix_potes_head_eval_f32: the Potes head in eval mode (no dropout) — the split-K partial launch
 *   of pcgmix_potes_head_fwd_f32, then ONE tail launch that sums the partials in that entry point's
 *   order, adds the bias, applies ReLU and the fmaf chain over the 20 features, then the row rule.
 *   The logits (optional output, may be NULL) are bit-identical to pcgmix_potes_head_fwd_f32 with
 *   both masks NULL; prob, loss_rows and vote are those of pcgmix_eval_rows_f32 on them.  x, w1, b1,
 *   w2, b2, partial: as for pcgmix_potes_head_fwd_f32 (K % 4 == 0, x and w1 16-byte aligned, partial
 *   pcgmix_skinny_linear_splits(B,K) * B * 20 floats).
 *
 * pcgmix_eval_segments_f32: the per-recording reduction of N rows into R recordings.
 *   order     (N) int32: the cycle rows grouped by recording, within a recording in loader order
 *   rec_start (R+1) int32 CSR offsets into order
 *   mean_p    (R,C): the recording's rows added SEQUENTIALLY in float32, divided by float(n) —
 *             bit for bit np.mean(list_of_rows, axis=0) (:627)
 *   votes     (R,C) int32: how many of the recording's vote bytes equal c (np.bincount, :638)
 *   loss_rec  (R) float64 (8-byte aligned): the recording's row losses added sequentially in double
 *   One thread per (recording, class).  The caller validates order and rec_start; the kernel
 *   additionally clamps every index it reads into range.  R == 0 returns 0 and launches nothing.
 */
int pcgmix_eval_rows_f32(const float* logits, const uint8_t* labels, float* prob, float* loss_rows,
                         uint8_t* vote, int B, int C, pcgmix_stream_t stream);
int pcgmix_potes_head_eval_f32(const float* x, const float* w1, const float* b1, const float* w2,
                               const float* b2, const uint8_t* labels, float* partial, float* logits,
                               float* prob, float* loss_rows, uint8_t* vote, int B, int K, int C,
                               pcgmix_stream_t stream);
int pcgmix_eval_segments_f32(const float* prob, const float* loss_rows, const uint8_t* vote,
                             const int32_t* order, const int32_t* rec_start, float* mean_p,
                             int32_t* votes, double* loss_rec, int N, int R, int C,
                             pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Potes classifier head + soft-target cross entropy, fused.                           [device]
 *
 * The head above followed by CELoss (train_model.py:45-54: mean_b(-sum_c log_softmax(logits)[b,c]
 * * target[b,c])) as ONE autograd node: the row-local part of the four small kernels between the
 * split-K product and the head's backward (tail forward, CE forward, CE backward, tail backward)
 * runs in one launch, their batch reductions in a second.
 *   forward : x, masks, weights, target (B,C float, soft targets) -> z, logits, loss (scalar) and,
 *             for d loss = 1: dz (B,20) and small = [dW2 (C x 20) | db2 (C) | db1 (20)];
 *             ws: pcgmix_potes_head_loss_workspace_floats(B) floats; dw1_zero (20,K) or NULL: the
 *             buffer the backward accumulates dW1 into, cleared here.
 *   backward: gscale = device scalar d L / d loss (NULL = 1): dx and dW1 from dz * gscale in one pass
 *             over x (as pcgmix_potes_head_bwd_f32), small_out = small_in * gscale.
 */
/* The head of a FROZEN model in eval mode, for d score / d input (saliency.py:52-61): features ->
 * split-K product -> dz = (z > 0) * (seed W2) -> dx = dz W1, three launches, no logits, no weight
 * gradients.  seed (B,C) = d score / d logits (the one-hot of the label; pcgmix_ctx_labels_begin
 * can write it); partial as for pcgmix_potes_head_fwd_f32; dz (B,20) scratch, 16-byte aligned;
 * dx (B,K) out.                                                                              */
int pcgmix_potes_head_saliency_f32(const float* x, const float* w1, const float* b1, const float* w2,
                                   const float* seed, float* partial, float* dz, float* dx, int B,
                                   int K, int C, pcgmix_stream_t stream);
/* The whole saliency pass of a frozen CNN_potes (saliency.py:26-91 with models.py:444-465 as the
 * model) in one call: the six launches of pcgmix_potes_stack_fwd_save_f32 ->
 * pcgmix_potes_head_saliency_f32 -> pcgmix_potes_stack_input_grad_mask_f32 ->
 * pcgmix_saliency_post_f32 back to back.  x (B,4,T); c*: conv stack weights; h*: head weights
 * (hb1 may be NULL); h2, m2, s1, partial, dz, gfeat, gx: the intermediate buffers of those entry
 * points (sizes as documented there); frames (B,5) device; sal (B,T) out.            [device]   */
int pcgmix_potes_saliency_pass_f32(const float* x, const float* cw1, const float* cb1, const float* cw2,
                                   const float* cb2, float* h2, uint8_t* m2, uint8_t* s1,
                                   const float* hw1, const float* hb1, const float* hw2,
                                   const float* seed, float* partial, float* dz, float* gfeat, float* gx,
                                   const int32_t* frames, float* sal, int ksize, double sigma, int B,
                                   int T, int K, int n_classes, pcgmix_stream_t stream);
long long pcgmix_potes_head_loss_workspace_floats(int B);
int pcgmix_potes_head_loss_fwd_f32(const float* x, const uint8_t* mask1, float scale1, int thr1,
                                   int bits1, const float* w1, const float* b1, const uint8_t* mask2,
                                   float scale2, int thr2, const float* w2, const float* b2,
                                   const float* target, float* partial, float* z, float* logits,
                                   float* dz, float* loss, float* small, float* ws, float* dw1_zero,
                                   int defer_finalize, int target_kind, int B, int K, int C,
                                   pcgmix_stream_t stream);
int pcgmix_potes_head_loss_bwd_f32(const float* dz, const float* gscale, const float* x,
                                   const uint8_t* mask1, float scale1, int thr1, int bits1,
                                   const float* w1, const float* small_in, float* small_out,
                                   float* dw1, float* dx, const float* deferred_ws,
                                   float* deferred_loss, int B, int K, int C,
                                   pcgmix_stream_t stream);
/* target_kind: 0 = `target` is float (B,C) (soft targets, CELoss' general case); 1 = `target` points
 * to uint8 class labels (B): hard targets as one byte per row.
 * defer_finalize / deferred_ws, deferred_loss: the forward's last launch — the fixed-order sum of
 * the per-row-block contributions in `ws` into `loss` and `small` — can be left to the backward,
 * whose feature pass does it in its first block (same order, same values): one launch less per
 * step when forward and backward always run together (a training step captured in a hipGraph).
 * With defer_finalize != 0 the forward writes neither `loss` nor `small`; the backward then takes
 * deferred_ws = ws, writes the loss to deferred_loss and ignores small_in.                      */

/* The fused forward with manifold mixup at the hidden layer — 1D `latentmixup` with a Potes model
 * (augmentations.py:1472-1506: `data = model(data, depth=1, 'first')`, `data*lam +
 * data[mix_indices]*(1-lam)`, then train_model.py:537 `model(data, depth=1, 'second')` = Linear(20->C),
 * models.py:456-465).  With h[b] = relu(z[b]) * mask2[b] * scale2 (every row under its own dropout
 * bytes, as the first half applies Dropout(.5) before the blend):
 *   hm[b] = lam h[b] + (1-lam) h[mix[b]];   logits[b] = W2 hm[b] + b2;   loss, dl as above;
 *   dW2 = sum_b dl[b] (x) hm[b];  db2 = sum_b dl[b];
 *   dz[b] = fac[b] * W2^T (lam dl[b] + (1-lam) dl[inv[b]]);  db1 = sum_b dz[b].
 * mix (B) = the partner permutation, inv (B) = its inverse (inv[mix[b]] = b), both int32 on the
 * device with values in [0, B); 0 <= lam <= 1.  z and dz are stored per row, z un-blended: the
 * backward is pcgmix_potes_head_loss_bwd_f32, unchanged (deferred_ws = NULL: this entry point always
 * finalizes).  Two launches behind the split-K product, as the plain forward; lam = 1 reproduces
 * the plain forward's outputs bit for bit.  Other arguments as pcgmix_potes_head_loss_fwd_f32.  */
int pcgmix_potes_head_loss_latent_fwd_f32(const float* x, const uint8_t* mask1, float scale1,
                                          int thr1, int bits1, const float* w1, const float* b1,
                                          const uint8_t* mask2, float scale2, int thr2,
                                          const float* w2, const float* b2, const float* target,
                                          float* partial, float* z, float* logits, float* dz,
                                          float* loss, float* small, float* ws, float* dw1_zero,
                                          int target_kind, int B, int K, int C, const int32_t* mix,
                                          const int32_t* inv, float lam, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Soft-target cross entropy (train_model.py:45-54, CELoss).                          [device]
 *   loss[0] = mean_b( -sum_c log_softmax(logits)[b,c] * target[b,c] )
 *   dlogits[b,c] = gout[0] / B * (softmax[b,c] * sum_c' target[b,c'] - target[b,c])
 * logits, target (B,C) float32; gout: device scalar (the incoming gradient of the loss).
 */
int pcgmix_soft_ce_fwd_f32(const float* logits, const float* target, float* loss, int B, int C,
                           pcgmix_stream_t stream);
int pcgmix_soft_ce_bwd_f32(const float* logits, const float* target, const float* gout,
                           float* dlogits, int B, int C, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SELC loss past its turning point (train_model.py:56-80, SELCLoss.forward, 'train', epoch > es):
 *   pred = softmax(logits)
 *   soft_labels[index] = m * soft_labels[index] + (1 - m) * pred.detach()      (side effect)
 *   loss = mean_b( -sum_c log(pred[b,c]) * soft_labels[index[b], c] )           [device]
 *
 * pcgmix_selc_fwd_f32: logits (B,C) float32; index (B) int64 on the device; soft_labels (N,C)
 * float32, read and written; rows (B,C) out = the updated soft rows, kept for the backward; loss
 * = device scalar.  One launch; the batch mean is summed in a fixed order (same inputs, same bits).
 *   keep = (float)m and take = (float)(1.0 - m) with the subtraction done in DOUBLE on the host:
 *   that is how torch casts the Python scalars of `m * a + (1 - m) * b`.  1.f - 0.9f in float is a
 *   different number (0x3DCCCCD0, not 0x3DCCCCCD).  keep*soft + take*pred is evaluated unfused.
 *   The row loss is -sum_c logp_c * s_c with logp = z - max - log(sum exp(z - max)): a deliberate
 *   deviation from the reference's log(softmax(z)) where pred underflows to 0 — there the reference
 *   returns inf and a nan gradient, this stays finite.  Elsewhere the two agree to rounding.
 *   A row whose index is outside [0,N) makes no update, gets a zero row in `rows` and contributes
 *   zero loss and zero gradient (the mean still divides by B); nothing outside soft_labels is ever
 *   written.  Precondition: the indices of one batch are distinct (torch's indexed assignment is
 *   undefined otherwise too; the reference's loaders sample without replacement).
 * pcgmix_selc_bwd_f32: dlogits[b,c] = gout[0] / B * (softmax[b,c] * sum_c' rows[b,c'] - rows[b,c]).
 *   It reads `rows`, not soft_labels: a later step may have moved those already.
 */
int pcgmix_selc_fwd_f32(const float* logits, const long long* index, float* soft_labels, int N,
                        float keep, float take, float* rows, float* loss, int B, int C,
                        pcgmix_stream_t stream);
int pcgmix_selc_bwd_f32(const float* logits, const float* rows, const float* gout, float* dlogits,
                        int B, int C, pcgmix_stream_t stream);
/* pcgmix_potes_head_loss_fwd_f32 with the SELC loss in place of CELoss: index, soft_labels, N, keep,
 * take (as above, same rules for a bad index and for duplicates) take the place of target /
 * target_kind; the tail kernel forms each row's target from the row's own logits and writes the
 * soft row back.  Everything behind it — dz, small, ws, defer_finalize, and the backward
 * pcgmix_potes_head_loss_bwd_f32 — is unchanged.  C <= 8.                                        */
int pcgmix_potes_head_loss_selc_fwd_f32(const float* x, const uint8_t* mask1, float scale1, int thr1,
                                        int bits1, const float* w1, const float* b1,
                                        const uint8_t* mask2, float scale2, int thr2,
                                        const float* w2, const float* b2, const long long* index,
                                        float* soft_labels, int N, float keep, float take,
                                        float* partial, float* z, float* logits, float* dz,
                                        float* loss, float* small, float* ws, float* dw1_zero,
                                        int defer_finalize, int B, int K, int C,
                                        pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One-call step of the plain PCGmix methods (durratiomixup / durmixmagwarp, same-label partners,
 * no '(rand)', no saliency): everything augmentations.py:941, 962-977 (and :874, 906-928) do
 * between the probability gate and the returned tensor.                      [host + device]
 *
 *   labels (B) int64, frames (B,5) int64: HOST.  x, y (B,C,T): device.  lam: float32(lambda).
 *   knots: HOST (B,n_knots,C) float64 as numpy drew them, or NULL (no warp); spline_op: DEVICE
 *   operator of pcgmix_spline_operator_f64 for (T, n_knots).
 *   staging: PINNED host scratch, dev_idx: device scratch, both pcgmix_splice_staging_bytes(B, C,
 *   n_knots) bytes; staging may be reused once the copy enqueued here has completed (record an
 *   event on `stream` after the call).
 *   mix_out (B) int64 HOST: the partner permutation — groups of equal label in order of first
 *   appearance, each permuted by a FRESH Random(step).sample (bit-identical to CPython).
 * Does: permutation, boundary validation, packing, ONE hipMemcpyAsync, the kernel launch.
 * Returns 0; -1 frames not monotone / negative, -2 cycle end beyond T, -3 partner out of range
 * (nothing enqueued); or a hipError_t.
 */
int pcgmix_splice_same_label_f32(const float* x, float* y, const int64_t* labels,
                                 const int64_t* frames, uint64_t step, float lam,
                                 const double* knots, const double* spline_op, int n_knots,
                                 void* staging, void* dev_idx, int64_t* mix_out, int B, int C,
                                 int T, pcgmix_stream_t stream);
/* Same, with the labels still on the device as the reference passes them (one-hot int64
 * (B, num_classes), contiguous): copies them into `ohe_pinned` (PINNED host, B*num_classes
 * int64), synchronises `stream` (the one host sync the reference's signature forces,
 * augmentations.py:501), takes the first-maximum argmax and continues as above. */
int pcgmix_splice_same_label_ohe_f32(const float* x, float* y, const int64_t* target_ohe_dev,
                                     int num_classes, int64_t* ohe_pinned, const int64_t* frames,
                                     uint64_t step, float lam, const double* knots,
                                     const double* spline_op, int n_knots, void* staging,
                                     void* dev_idx, int64_t* mix_out, int B, int C, int T,
                                     pcgmix_stream_t stream);
long long pcgmix_splice_staging_bytes(int B, int C, int n_knots);

/* ------------------------------------------------------------------------------------------
 * Per-device step context + the whole fired step of a plain PCGmix method in ONE call.
 *                                                                            [host + device]
 * What the reference's augment() does between the probability gate and the returned tensor for
 * durratiomixup / durmixmagwarp with same-label partners (augmentations.py:874-928, 941-977):
 * label recovery from the one-hot matrix (:501), the partner permutation (:500-514), boundary
 * packing, the per-sample splice loop (:909-917, 969-977) and magnitude_warp (:674-683).
 *
 * The context owns what the step needs besides the batch: a ring of pinned staging buffers with
 * device twins (a slot is reused only after the kernel that read it has finished), host-mapped
 * memory for the label read-back, the spline operators per (T, n_knots).  It is created on
 * `device`; calls may come with any device current.  One context per device and host thread.
 *
 * pcgmix_augment_plain_f32:
 *   x, y            device (B, C, T); y must not alias x
 *   target_ohe_dev  device int64 (B, num_classes) one-hot as the reference passes it, or NULL when
 *   labels_host     host int64 (B) class labels are given instead (no read-back, no host wait)
 *   frames          HOST int64 (B, 5), as the reference's loader yields them
 *   lam             float32(lambda) drawn by the caller from numpy's global stream (:659-666)
 *   knots           HOST float64 (B, n_knots, C) as numpy.random.normal drew them (:677), or NULL
 *   mix_out         HOST int64 (B) out: the partner permutation (bit-identical to CPython's)
 * Order of work: the label arg-max kernel is enqueued FIRST (it writes int32 labels into
 * host-mapped memory and releases a flag word); boundaries are validated and packed, knots staged
 * and MT19937 seeded while the GPU gets there; then the host spins on the flag (the one wait
 * the reference's signature forces; falls back to hipStreamSynchronize after 2 ms), draws the
 * permutation, issues ONE hipMemcpyAsync and the fused kernel.  Must not be called on a
 * capturing stream when target_ohe_dev is used (hipErrorStreamCaptureUnsupported).
 * Returns 0; -1 frames not monotone / negative, -2 cycle end beyond T (splice not enqueued); or
 * a hipError_t.
 *
 * pcgmix_ctx_gate: random.Random(step).uniform(0, 1) (augmentations.py:869-870, 936-937); the
 * seeded generator is kept, so the step call for the same `step` does not seed a second time.
 */
/* Host-to-device copy as ONE kernel launch: src_pinned = pinned host memory (hipHostMalloc, torch
 * pin_memory: device-readable at the same address), dst_dev = device memory, both 16-byte aligned;
 * nbytes is rounded up to whole 16-byte words, which both buffers must hold.  For per-step index
 * data above 16 KB (e.g. the magnitude-warp knots, augmentations.py:677: 49 KB at bs 256):
 * hipMemcpyAsync switches from a blit kernel to the SDMA engine there, which on MI355X stalls the
 * stream for ~25 us per copy.  The step context does this internally.          */
int pcgmix_fetch_h2d(const void* src_pinned, void* dst_dev, size_t nbytes, pcgmix_stream_t stream);

typedef struct pcgmix_ctx pcgmix_ctx;
int pcgmix_ctx_create(int device, pcgmix_ctx** out);
void pcgmix_ctx_destroy(pcgmix_ctx* ctx);
double pcgmix_ctx_gate(pcgmix_ctx* ctx, uint64_t step);
/* Up to 1 MiB the caller wants on the device together with the NEXT pcgmix_augment_plain_f32 step
 * of this context (the float targets the loss reads — train_model.py:541-549 moves them with
 * their own .to(device) —, optimiser scalars, a dropout key): the bytes are copied now, appended
 * to that step's index block (same pinned slot, same single H2D copy) and written to dst_dev
 * (DEVICE, 16-byte aligned, >= bytes rounded up to 16) by the splice kernel, i.e. they are in
 * place for everything enqueued behind the step on its stream.  One shot; bytes == 0 withdraws. */
int pcgmix_ctx_set_payload(pcgmix_ctx* ctx, const void* host, size_t bytes, void* dst_dev);
/* Sends a pending payload on its own — the step it was meant for ran no plain splice (probability
 * gate): one H2D copy from the context's pinned ring straight to dst_dev on `stream`.  No-op
 * when nothing is pending. */
int pcgmix_ctx_flush_payload(pcgmix_ctx* ctx, pcgmix_stream_t stream);
/* The saliency-guided step ('(saloptenv)…' / '(saloptsum)…' with same-label partners,
 * augmentations.py:874-928) as two calls around the caller's saliency pass:
 *   begin   label arg-max kernel (labels -> host-mapped memory; float one-hot -> seed_out, DEVICE
 *           (B, num_classes), the saliency model's gradient seed, may be NULL); `frames` (HOST
 *           int64 (B,5)) validated, packed to int32 and copied to frames_dst_dev (DEVICE, B*5
 *           int32: what saliency post-processing, search and splice read).  target_ohe_dev may be
 *           NULL when the labels will be handed over to finish.
 *   ...     the caller enqueues the frozen model's forward + input gradient + post-processing
 *           (get_saliency_maps, saliency.py:20-91) and draws lambda and the warp knots
 *   finish  labels picked up (labels_host NULL) or taken from labels_host; partners drawn as
 *           get_same_label_mix_indices does; [partners | knots] in one H2D copy; displacement
 *           search + fused splice(+warp) as in pcgmix_salopt_mix_warp_f32; mix_out (HOST int64
 *           (B)) = the partner indices.
 * Returns 0, -1 / -2 for malformed boundaries (begin; nothing is copied), or a hipError_t.       */
int pcgmix_ctx_salopt_begin(pcgmix_ctx* ctx, const int64_t* target_ohe_dev, int num_classes,
                            float* seed_out, const int64_t* frames, int32_t* frames_dst_dev, int B,
                            int T, pcgmix_stream_t stream);
/* begin for a caller that holds the class labels on the HOST (a training loop with the loader's
 * CPU `target`, train_model.py:498-501): no read-back.  labels_host HOST int64 (B), values in
 * [0, num_classes).  Up to 256 samples (T <= 32767, num_classes <= 256) ONE launch carries the
 * labels, the boundaries and a pending pcgmix_ctx_set_payload of up to 320 bytes in its
 * arguments and writes seed_out, frames_dst_dev and the payload's destination; larger batches
 * stage [frames | labels] through a pinned slot (the payload then stays pending for
 * pcgmix_ctx_flush_payload).  finish is called with the same labels_host.  Returns as begin.
 * All step-context entry points return hipErrorStreamCaptureUnsupported on a capturing stream. */
int pcgmix_ctx_salopt_begin_labels(pcgmix_ctx* ctx, const int64_t* labels_host, int num_classes,
                                   float* seed_out, const int64_t* frames,
                                   int32_t* frames_dst_dev, int B, int T, pcgmix_stream_t stream);
int pcgmix_ctx_salopt_finish(pcgmix_ctx* ctx, const float* x, float* y, const float* sal,
                             const int32_t* frames_dev, const int64_t* labels_host, uint64_t step,
                             float lam, int mode, const double* knots, int n_knots, int64_t* mix_out,
                             int B, int C, int T, pcgmix_stream_t stream);
/* The label read-back alone, in two halves, for steps that have GPU work to enqueue in between
 * (the saliency-guided step, augmentations.py:881-907): begin = the arg-max kernel on `stream`;
 * wait = the spin on the flag word, then int64 class labels in labels_out (HOST, B).
 * seed_out (DEVICE, float (B, num_classes), may be NULL): the same kernel also writes the one-hot
 * of the labels as floats — d score[label] / d logits, the seed of the saliency model's input
 * gradient (saliency.py:52-61) — sparing the max / zeros / scatter launches that build it. */
int pcgmix_ctx_labels_begin(pcgmix_ctx* ctx, const int64_t* target_ohe_dev, int num_classes, int B,
                            float* seed_out, pcgmix_stream_t stream);
int pcgmix_ctx_labels_wait(pcgmix_ctx* ctx, int64_t* labels_out, int B, pcgmix_stream_t stream);
int pcgmix_augment_plain_f32(pcgmix_ctx* ctx, const float* x, float* y,
                             const int64_t* target_ohe_dev, int num_classes,
                             const int64_t* labels_host, const int64_t* frames, uint64_t step,
                             float lam, const double* knots, int n_knots, int64_t* mix_out,
                             int B, int C, int T, pcgmix_stream_t stream);

/* The armed plain step.  With target_ohe_dev given (the reference's signature: labels on the device,
 * augmentations.py:501), no warp, B <= 256, T <= 32767, T % 4 == 0 and 16-byte aligned x, y,
 * pcgmix_augment_plain_f32 enqueues ONE kernel at the start of the call: its first block does the
 * label arg-max, its other blocks wait for the index records the host writes into host-mapped
 * memory once it has drawn the partners (csrc/pcgmix_kernels.h, ArmedArgs).  Same output as the
 * two-launch path (PCGMIX_NO_ARMED=1), bit for bit.  The waiting blocks give up `timeout_ticks`
 * (100 MHz; default 1 s) after the kernel started; the call notices (records written later than
 * 0.4 s after the launch: stream synchronisation, abort word) and launches the splice again.
 * stats: out3 = steps armed | of them checked after a stream synchronisation | kernels given up
 * (relaunched unarmed, or released by pcgmix_augment_plain_abort / the next begin).
 * debug (tests): the relays' timeout and a host stall in front of the record write; 0, 0 = defaults. */
int pcgmix_ctx_armed_stats(pcgmix_ctx* ctx, long long* out3);
/* The armed plain step (no warp) in two calls, for a binding with host work of its own between the
 * launch and the moment lambda is known — PKG/augmentations.py draws lambda from numpy's global stream
 * there (augmentations.py:661-663), 2.7 us that otherwise stand in front of the launch.
 * begin: validates, and if the step is eligible (conditions above) enqueues the armed kernel and returns
 * 0; returns PCGMIX_NOT_ARMED with nothing enqueued when it is not (call pcgmix_augment_plain_f32), a
 * hipError_t on failure.  A pending pcgmix_ctx_set_payload travels with the launch.
 * finish: boundaries (validated: -1 / -2 as pcgmix_augment_plain_f32, the waiting kernel is released),
 * label pick-up, partner draw into mix_out (HOST int64 (B)), records + lambda.  hipErrorNotReady without
 * a begin.  A begin that is never finished is released by pcgmix_augment_plain_abort, by the next begin
 * (or by the blocks' timeout).
 * abort: for the caller whose own work between begin and finish failed (numpy refused the step number, an
 * interrupt): if a begin is open, the waiting kernel is told to give up at once (its output is then
 * undefined), the step is closed and counted in stats' third number; 0.  Nothing open: 0, nothing done.
 * hipErrorInvalidValue for a NULL context. */
#define PCGMIX_NOT_ARMED (-3)
int pcgmix_augment_plain_abort(pcgmix_ctx* ctx);
int pcgmix_augment_plain_begin(pcgmix_ctx* ctx, const float* x, float* y, const int64_t* target_ohe_dev,
                               int num_classes, int B, int C, int T, pcgmix_stream_t stream);
int pcgmix_augment_plain_finish(pcgmix_ctx* ctx, const int64_t* frames, uint64_t step, float lam,
                                int64_t* mix_out);
/* begin with the step's boundaries (HOST int64 (B,5), the array finish will get) at hand: the kernel is
 * told every sample's own cycle [frames[b,0], frames[b,4]) in its arguments and loads its own rows — and
 * stores the elements outside the cycle, which are copies whatever partner is drawn — while it waits for
 * the records.  Nothing is validated here (a sample whose edges are out of range is left to the records);
 * finish reports malformed boundaries as before.  frames == NULL: as pcgmix_augment_plain_begin.  If finish
 * is handed boundaries whose cycles reach outside the ones given here, it gives the kernel up and runs the
 * step unarmed: same result.  pcgmix_augment_plain_f32 passes its boundaries the same way. */
int pcgmix_augment_plain_begin_edges(pcgmix_ctx* ctx, const float* x, float* y, const int64_t* target_ohe_dev,
                                     int num_classes, int B, int C, int T, const int64_t* frames,
                                     pcgmix_stream_t stream);
int pcgmix_ctx_armed_debug(pcgmix_ctx* ctx, unsigned long long timeout_ticks, int stall_ms);

/* Diagnostic: mean host nanoseconds per pcgmix_augment_plain_f32 call since the last query, by
 * phase: label kernel launch | slot reserve | pack + seed | label wait | grouping + permutation |
 * H2D enqueue | kernel launch | event record.  Returns the number of calls averaged; resets. */
long long pcgmix_ctx_phase_times(pcgmix_ctx* ctx, double* out8);

/* Which instantiation of the splice kernel pcgmix_mix_warp_f32 launches for this problem:
 * vec = 4 (16-byte lanes; needs T % 4 == 0 and 16-byte aligned x, y) or 1, unroll = quads per
 * lane (1, 2, 4).  For reporting: the kernel's name is mix_warp_kernel<vec, warp, unroll>. */
int pcgmix_mix_variant(int B, int C, int T, int warp, int aligned16, int* vec, int* unroll);
/* Name of the kernel instantiation pcgmix_mix_warp_f32 launches for this problem, as rocprofv3
 * lists it (e.g. "pcgmix::mix_warp_tq_kernel<2, 1>"), written NUL-terminated into buf.  n_knots = 0:
 * no warp; zero_rect != 0: the call carries 2D mask rectangles.  Asks the same selection routine
 * the launcher uses. */
int pcgmix_mix_kernel_name(int B, int C, int T, int n_knots, int zero_rect, int aligned16, char* buf,
                           int buf_len);

/* ------------------------------------------------------------------------------------------
 * BatchNorm + ReLU + MaxPool of a ResNet9 block, channels innermost.               [device]
 *
 * Replaces nn.BatchNorm1d/2d -> nn.ReLU -> nn.MaxPool1d/2d of conv_block (models.py:468-473,
 * models2d.py:13-19) and their autograd.  y is the convolution output stored NHWC: (B, H, W, C)
 * row-major (H = 1 for the 1D network); C is 2 or a multiple of 4 up to 1024
 * (pcgmix_bnrp_supported), which covers every width of the reference's ResNet9 size ladder.
 *   forward : batch mean / biased variance per channel -> z (B, H/ph, W/pw, C) =
 *             maxpool_{ph x pw}(relu(gamma * (y - mean) / sqrt(var + eps) + beta)) [+ skip];
 *             ph = pw = 1: no pooling.  skip (shape of z, or NULL): the residual connection of
 *             res1 / res2 (models.py:577, 581: `out = self.res1(out) + out`) added in the same
 *             pass; its gradient is dz itself, so the backward below is unchanged.  mean, invstd (C each) are outputs kept for backward; running_mean /
 *             running_var (may be NULL) are updated in place with `momentum` (unbiased variance).
 *   backward: dz (shape of z) -> dx (shape of y), dgamma, dbeta (C each).  The ReLU mask and the
 *             pooling arg-max (first maximum) are recomputed from y.
 * workspace: pcgmix_bnrp_workspace_floats(B, H, W, C) floats.  All pointers 16-byte aligned
 * (8-byte for C = 2), the workspace included; a misaligned one is refused (hipErrorInvalidValue).
 * Non-finite input (forward): the ReLU and the window maximum keep a NaN as torch's relu and
 * max_pool do, so a NaN in y — which in training mode makes the whole channel's statistics NaN —
 * reaches z instead of turning into zeros.  The backward of a non-finite y is not specified.
 * Each direction reads y twice and writes its output once; reductions are fixed-order.
 */
/* 1 for the channel counts the kernels take, else 0.  Host only: no device is touched. */
int pcgmix_bnrp_supported(int C);
long long pcgmix_bnrp_workspace_floats(int B, int H, int W, int C);
/* mean_shift (C, may be NULL): a per-channel constant left out of y — the convolution's bias, which
 * the normalisation cancels — added to the batch mean in the running-mean update only;
 * batches_tracked (may be NULL): nn.BatchNorm's num_batches_tracked, incremented by one;
 * dzero (C, may be NULL): receives zeros, the exact gradient of such a constant (so that the
 * optimiser still sees the parameter and applies weight decay, as in the reference).            */
int pcgmix_bnrp_fwd_f32(const float* y, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, float momentum, float eps, const float* mean_shift,
                        long long* batches_tracked, const float* skip, float* z, float* mean,
                        float* invstd, float* workspace, int B, int H, int W, int C, int ph, int pw,
                        pcgmix_stream_t stream);
int pcgmix_bnrp_bwd_f32(const float* y, const float* dz, const float* gamma, const float* beta,
                        const float* mean, const float* invstd, float* dx, float* dgamma,
                        float* dbeta, float* dzero, float* workspace, int B, int H, int W, int C,
                        int ph, int pw, pcgmix_stream_t stream);
/* Eval mode: the same block with BatchNorm on its running statistics, as the reference's model runs
 * in test_data_accuracy (train_model.py:591-670) and in the frozen saliency pass
 * (saliency.py:26-61) after model.eval(): nn.BatchNorm1d/2d (eval) -> nn.ReLU -> nn.MaxPool1d/2d
 * of conv_block (models.py:468-473, models2d.py:13-19).
 *   z = maxpool_{ph x pw}(relu(gamma * (y - (running_mean - conv_bias)) / sqrt(running_var + eps)
 *       + beta)) [+ skip]
 * conv_bias (C, may be NULL): the convolution's bias when it was left out of y.  One launch, no
 * workspace; the running statistics are read only.  Shapes, channel counts and alignment as above;
 * conv_bias and skip may be NULL.                                                              */
int pcgmix_bnrp_eval_fwd_f32(const float* y, const float* gamma, const float* beta,
                             const float* running_mean, const float* running_var, float eps,
                             const float* conv_bias, const float* skip, float* z, int B, int H,
                             int W, int C, int ph, int pw, pcgmix_stream_t stream);
/* The input gradient of the above (replaces the autograd of the same three modules in the frozen
 * pass, saliency.py:26-61): dx (shape of y) = gamma / sqrt(running_var + eps) * dz at the FIRST
 * maximum of each window where the activation is > 0, exact zeros everywhere else, the positions
 * no window covers included.  One launch, no reduction.  The gradient of skip is dz itself.     */
int pcgmix_bnrp_eval_bwd_f32(const float* y, const float* dz, const float* gamma, const float* beta,
                             const float* running_mean, const float* running_var, float eps,
                             const float* conv_bias, float* dx, int B, int H, int W, int C, int ph,
                             int pw, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The paper's 1D comparison augmentations.                                        [device]
 *
 * One launch each for the O(B*C*T) part of the reference's baseline branches of augment();
 * the RNG, the parsing and the host arrays stay in hostprep.py.  B == 0 returns 0 and
 * launches nothing.
 *
 * pcgmix_blend_rows_f32 — mixup(same) / mixup(mix), augmentations.py:838-861:
 *     y[b] = x[b]*lam + x[mix[b]]*(1-lam)   over the whole (C, T) plane; fp32 mul, mul, add,
 *     (1-lam) formed in float32.  mix: device int32 (B), values in [0, B).
 * pcgmix_warp_rows_f32 — magnitude_warp over whole rows, augmentations.py:674-683, 1026-1048:
 *     y[b,c,t] = float(double(x[b,c,t]) * S_bc(t)), S_bc the not-a-knot spline through
 *     (linspace(0, T-1, n_knots), knots[b,:,c]); knots device float64 (B, n_knots, C) as numpy
 *     drew them, spline_op the device copy of pcgmix_spline_operator_f64(T, n_knots).  Same
 *     coefficients and evaluation as the warp stage of pcgmix_mix_warp_f32.
 * pcgmix_scale_rows_f32 — respiratoryscale, augmentations.py:777-804:
 *     y[b,c,t] = float(double(x[b,c,t]) * s[t]),  s device float64 (T) (the numpy sinusoid).
 * pcgmix_zero_spans_f32 — timemask, augmentations.py:807-827, IN PLACE:
 *     x[b, :, spans[b][0] : spans[b][1]] = 0,  spans device int32 (B, 2), clipped to [0, T).
 * pcgmix_time_warp_f32 — time_warp, augmentations.py:685-696, 1002-1024: per row (b, c)
 *     tw    = CubicSpline(brk, brk * knots[b,:,c])(arange(T))       (products first, fp64)
 *     xp    = clip(((T-1) / tw[T-1]) * tw, 0, T-1)
 *     y     = float(np.interp(arange(T), xp, double(x[b,c,:])))
 *   np.interp restated exactly, including xp that decreases somewhere (numpy's search with the
 *   previous query's result as its guess).  workspace: device, pcgmix_time_warp_workspace_bytes
 *   (B, C, T) bytes (0 = none needed: the row lives in LDS); n_knots 2..64, T >= 2.
 * x and y are distinct (B, C, T) float32 tensors.
 * Refused with hipErrorInvalidValue, nothing launched: a NULL pointer among those named above,
 * x == y, B < 0, C <= 0, T <= 0 (T < 2 for the two warps), n_knots outside 2..64, workspace NULL
 * when pcgmix_time_warp_workspace_bytes is not 0.  Span ends outside [0, T] are clipped, a
 * span with s1 <= s0 zeroes nothing.                                                          */
int pcgmix_blend_rows_f32(const float* x, float* y, const int32_t* mix, float lam, int B, int C,
                          int T, pcgmix_stream_t stream);
int pcgmix_warp_rows_f32(const float* x, float* y, const double* knots, const double* spline_op,
                         int n_knots, int B, int C, int T, pcgmix_stream_t stream);
int pcgmix_scale_rows_f32(const float* x, float* y, const double* s, int B, int C, int T,
                          pcgmix_stream_t stream);
int pcgmix_zero_spans_f32(float* x, const int32_t* spans, int B, int C, int T,
                          pcgmix_stream_t stream);
long long pcgmix_time_warp_workspace_bytes(int B, int C, int T);
int pcgmix_time_warp_f32(const float* x, float* y, const double* knots, const double* spline_op,
                         int n_knots, void* workspace, int B, int C, int T, pcgmix_stream_t stream);

/* Host twins of the time warp, built from the same __host__ __device__ code as the kernel.  [host]
 * pcgmix_np_interp_f64: out = np.interp(x, xp, fp) for any xp (numpy's query-order search with
 *   guess, its NaN-slope retry, left/right = fp[0]/fp[n-1]); n >= 1.
 * pcgmix_time_warp_row_f64: one row of time_warp — spline_op of (T, n_knots), knots (n_knots)
 *   of that row, x (T) float32 -> y (T) float32; xp_out (T, may be NULL) receives xp.          */
int pcgmix_np_interp_f64(const double* x, long long nx, const double* xp, const double* fp,
                         long long n, double* out);
int pcgmix_time_warp_row_f64(const double* spline_op, const double* knots, int n_knots,
                             const float* x, int T, float* y, double* xp_out);

/* ------------------------------------------------------------------------------------------
 * The paper's spectrogram comparison baselines.  csrc/pcgmix_baselines.hip (zero_rects_kernel) and
 * csrc/pcgmix_cutpaste.hip (cutpaste_rows_kernel, the segment-table copy shared with the 1D
 * cut-and-paste family).
 *
 * One launch each for the O(B*C*F*W) part of the reference's 2D baseline branches
 * (augmentations2d.py:461-617); the RNG, the parsing and the per-sample tables stay in
 * hostprep.py.  Batches are float32 (B, C, F, W), contiguous.  B == 0 returns 0 and launches
 * nothing.  (mixup and latentmixup's blend are pcgmix_blend_rows_f32 on the flat sample planes.)
 *
 * pcgmix_zero_rects_f32 — timemask (augmentations2d.py:461-485) and freqmask (:487-508), IN PLACE:
 *     x[b, c, rect[b][0] : rect[b][1], rect[b][2] : rect[b][3]] = 0   for every channel c;
 *   rect device int32 (B, 4), clipped to the plane; max_area an upper bound of the rectangles'
 *   clipped areas (it sizes the grid; F*W is always safe).  Only the zeroed elements are written.
 *   max_area == 0 returns 0 and launches nothing; max_area < 0, F <= 0, W <= 0, C <= 0, B < 0 and a
 *   NULL x or rect are refused with hipErrorInvalidValue.
 * pcgmix_piecewise_rows_f32 — cutmix (:574-597, cutmix_multidim_tensors :34-51) and
 *   durratiocutmix (:599-617, cutmix_keepdur_multidim_tensors :223-249):
 *     y (B, C, F, Wo) from x (B, C, F, W).  segs device int32 (B, PCGMIX_PIECE_SEGS, 4), per
 *     segment {lo, hi, src, shift}: contiguous, ordered, lo of the first = 0, along the columns
 *     (axis 0) or along F (axis 1, Wo == W).  A position p in [lo, hi) reads
 *       PCGMIX_PIECE_OWN      x[b]       at p + shift
 *       PCGMIX_PIECE_PARTNER  x[mix[b]]  at p + shift
 *       PCGMIX_PIECE_ZERO     0
 *     along that axis (the other coordinates unchanged); positions beyond the last hi, and source
 *     positions outside the input, give 0.  mix device int32 (B), values in [0, B).  x != y.
 *     The batch runs along gridDim.y and gridDim.z, as for pcgmix_cutpaste_rows_f32:
 *     B <= 32768 * 1024, hipErrorInvalidValue beyond.                                        */
#define PCGMIX_PIECE_SEGS 5
#define PCGMIX_PIECE_OWN 0
#define PCGMIX_PIECE_PARTNER 1
#define PCGMIX_PIECE_ZERO 2
int pcgmix_zero_rects_f32(float* x, const int32_t* rect, int B, int C, int F, int W, int max_area,
                          pcgmix_stream_t stream);
int pcgmix_piecewise_rows_f32(const float* x, float* y, const int32_t* segs, const int32_t* mix,
                              int axis, int B, int C, int F, int W, int Wo, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The heart-cycle cut-and-paste family (cutpaste_rows_kernel) and durmixrespscale
 * (splice_scale_kernel).  csrc/pcgmix_cutpaste.hip.
 *
 * One launch each, on (B, C, T) float32 contiguous batches; the RNG, the partner selection and the
 * per-sample tables stay in hostprep.py.  B == 0 returns 0 and launches nothing.  The input and
 * the output may not overlap (every sample reads its partner's rows).
 *
 * pcgmix_cutpaste_rows_f32 — replaces the per-sample loops around cutmix_keepdur_multidim_tensors
 *   (augmentations.py:340-366; the branches :983-1000 wav-durratiocutmix, :1101-1119
 *   durratiocutmix) and cutmix_multidim_tensors (:30-58; :1121-1151 lengthcutmix, :1153-1182
 *   datasetcutmix, :1184-1213 wavcutmix, :1285-1316 labelcutmix, with their 'cutout' suffix):
 *     segs device int32 (B, PCGMIX_PIECE_SEGS, 4), {lo, hi, src, shift} along T in the convention
 *     of pcgmix_piecewise_rows_f32, whose kernel this is (contiguous, ordered; positions beyond the
 *     last hi and source positions outside [0, T) give 0); mix device int32 (B), values in [0, B);
 *     B <= 32768 * 1024.
 *     junctions: NULL, or device int32 (B, 4) {c1, c2, ov, unused} — the '(smooth)' cross-fade
 *     (:41-51): for ov in 1..PCGMIX_CUTPASTE_MAX_OVERLAP and t in [c1-ov, c1+ov), j = t-(c1-ov),
 *       y[b,c,t] = float(double(x[b,c,t]) * (1 - s[j]) + double(x[mix[b],c,c2-ov+j]) * s[j])
 *     (float64 multiply, multiply, add, each rounded on its own, then one rounding to float32)
 *     unless t lies in a ZERO segment; ov outside that range: no window.  sigmoid_tab: device
 *     float64 (PCGMIX_CUTPASTE_MAX_OVERLAP, 2*PCGMIX_CUTPASTE_MAX_OVERLAP), row ov-1 = the
 *     reference's sigmoid(ov) (:668-672) in its first 2*ov entries; required with junctions.
 * pcgmix_mix_scale_f32 — durmixrespscale (:734-775): the splice of pcgmix_mix_warp_f32 without
 *   warp (frames, mix_idx, off as there; fp32 mul, mul, add) and then, for EVERY element,
 *     y[b,c,t] = float(double(splice[b,c,t]) * row[t])
 *   with row device float64 (T) — one launch instead of the splice followed by
 *   pcgmix_scale_rows_f32.                                                                   */
#define PCGMIX_CUTPASTE_MAX_OVERLAP 10
int pcgmix_cutpaste_rows_f32(const float* x, float* y, const int32_t* segs, const int32_t* mix,
                             const int32_t* junctions, const double* sigmoid_tab, int B, int C,
                             int T, pcgmix_stream_t stream);
int pcgmix_mix_scale_f32(const float* x, float* y, const int32_t* frames, const int32_t* mix_idx,
                         const int32_t* off, float lam, const double* row, int B, int C, int T,
                         pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conv1d(k = 3, pad = 1, stride 1) of ResNet9-1D, channels innermost.              [device]
 * csrc/pcgmix_conv3.hip (conv3_kernel).
 *
 * Replaces nn.Conv1d(c_in, c_out, kernel_size=3, padding=1) of conv_block (models.py:468-473)
 * where its weights are frozen: the evaluation pass (train_model.py:591-670) and the frozen
 * saliency pass (saliency.py:26-61).  No bias (the BatchNorm kernels above take it).
 *   x (B, L, Cin)     the memory of a (B, Cin, 1, L) channels_last tensor
 *   w (Cout, 3, Cin)  [o][tap][i], the memory ResNet9_myrtle gives its Conv1d weights
 *   y (B, L, Cout)    y[b,l,o] = sum over tap, i of x[b, l+tap-1, i] * w[o,tap,i], zeros beyond
 *                     both ends of every sample
 * The input gradient of the layer is the same call on dy with w'[i][tap][o] = w[o][2-tap][i].
 * One launch.  Every output element is ONE float32 fmaf chain over the 3*Cin products in a fixed
 * order (groups of 16 input channels; in a group tap 0, 1, 2; in a tap the channels ascending) on
 * v_mfma_f32_32x32x2_f32: no split-K, no atomics, so a sample's result is the same bits in every
 * launch, at every B and at every place in the batch.
 * pcgmix_conv3_supported: 1 for Cin % 4 == 0, 4 <= Cin <= 1024 and Cout == 4 or Cout % 16 == 0,
 *   Cout <= 1024, else 0.  Host only: no device is touched.
 * Refused with hipErrorInvalidValue, nothing launched and y untouched: unsupported widths, a NULL
 * pointer, a pointer that is not 16-byte aligned, B < 0, L < 1, L * max(Cin, Cout) > INT_MAX.
 * B == 0 returns 0 and launches nothing.  x and y may not overlap.
 * pcgmix_conv3_tile: the kernel's tile constants, for tests that place shapes at tile edges:
 *   which = 0 the positions of one M tile (128), 1 the input channels of one K group (16), else 0.
 *   Host only.                                                                                  */
int pcgmix_conv3_supported(int Cin, int Cout);
int pcgmix_conv3_tile(int which);
int pcgmix_conv3_nlc_f32(const float* x, const float* w, float* y, int B, int L, int Cin, int Cout,
                         pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Weight gradient of the same Conv1d(k = 3, pad = 1, stride 1), channels innermost.   [device]
 * csrc/pcgmix_conv3_wgrad.hip (wgrad_kernel, reduce_kernel).
 *
 * The weight gradient of nn.Conv1d(c_in, c_out, kernel_size=3, padding=1) of conv_block
 * (models.py:468-473) in the training step; with it models.Conv3TrainFunction runs all three GEMMs
 * of a trainable layer on the project's kernels (opt-in: models.FUSED_CONV_TRAIN).
 *   x  (B, L, Cin)     the layer's input, as pcgmix_conv3_nlc_f32 takes it
 *   dy (B, L, Cout)    the gradient of the layer's output
 *   dw (Cout, 3, Cin)  [o][tap][i], the layout of w above
 *   dw[o][tap][i] = sum over b, l of dy[b][l][o] * x[b][l + tap - 1][i], x zero outside [0, L).
 * The sum over the B * L positions is cut into K tiles of 64 consecutive positions of one sample,
 * numbered sample-major; `splits` blocks per output tile each add a contiguous ascending range of
 * them on v_mfma_f32_32x32x2_f32 and write one partial into the caller's workspace; a second launch
 * adds the partials in ascending order with plain float32 adds.  No atomics, no grid-wide wait, no
 * allocation: dw's bits are a function of x, dy and (B, L, Cin, Cout) alone, the same on every
 * device and in every run.  Unlike y above they DO depend on B (B sets the splits).
 * pcgmix_conv3_wgrad_supported (models.py:468-473): the widths pcgmix_conv3_supported takes.  Host only.
 * pcgmix_conv3_wgrad_tile (models.py:468-473): the kernel's tile constants, for tests that place
 *   shapes at tile edges: which = 0 the positions of one K tile (64), 1 the output channels of a
 *   block tile (128), 2 the input channels of a block tile (64; 32 where Cin <= 32), else 0.  Host only.
 * pcgmix_conv3_wgrad_plan (models.py:468-473): *splits (1 <= splits <= number of K tiles, 1 for an
 *   empty batch) and *workspace_bytes (splits * Cout * 3 * Cin * 4, or 0 when splits == 1) for a call
 *   of these arguments; either pointer may be NULL.  0, or hipErrorInvalidValue for unsupported widths,
 *   B < 0 or L < 1.  Host only.
 * pcgmix_conv3_wgrad_nlc_f32 (models.py:468-473): refused with hipErrorInvalidValue, nothing launched
 *   and dw and the workspace untouched: unsupported widths, a NULL x, dy or dw, a NULL workspace when
 *   the plan needs bytes, a pointer that is not 16-byte aligned, workspace_bytes below the plan's,
 *   B < 0, L < 1, L * max(Cin, Cout) > INT_MAX.  B == 0 writes zeros to dw and returns 0.  The
 *   workspace is never read before the same call has written it, and nothing beyond the planned
 *   bytes is touched.  dw and the workspace may not overlap x, dy or each other.               */
int pcgmix_conv3_wgrad_supported(int Cin, int Cout);
int pcgmix_conv3_wgrad_tile(int which);
int pcgmix_conv3_wgrad_plan(int B, int L, int Cin, int Cout, int* splits, size_t* workspace_bytes);
int pcgmix_conv3_wgrad_nlc_f32(const float* x, const float* dy, float* dw, void* workspace,
                               size_t workspace_bytes, int B, int L, int Cin, int Cout, pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same Conv1d(k = 3, pad = 1, stride 1) and its weight gradient for the narrow layers of
 * resnet9-5k .. resnet9-50k, channels innermost, on the vector ALU.                  [device]
 * csrc/pcgmix_conv3_narrow.hip (fwd_kernel, wgrad_kernel, reduce_kernel).
 *
 * nn.Conv1d(c_in, c_out, kernel_size=3, padding=1) of conv_block (models.py:468-473) at the widths the
 * two blocks above refuse: Cin and Cout both in {2, 4, 8, 16} with Cin == 2 or Cout in {2, 8} — the
 * ten pairs (2,2) (2,4) (2,8) (2,16) (4,2) (8,2) (16,2) (4,8) (8,8) (16,8).  The two sets are
 * disjoint.  x, w, y, dy and dw are laid out as above; models.FUSED_CONV_NARROW routes to them.
 * pcgmix_conv3_narrow_supported (models.py:468-473): 1 on exactly those ten pairs, else 0.  Host only.
 * pcgmix_conv3_narrow_tile (models.py:468-473): which = 0 the positions of one forward tile (256),
 *   1 the positions of one weight-gradient K tile (256), else 0.  Host only.
 * pcgmix_conv3_narrow_nlc_f32 (models.py:468-473; saliency.py:26-61; train_model.py:591-670): one
 *   launch, one position a thread.  Every output element is ONE float32 fmaf chain from +0 over the
 *   3*Cin products: tap 0, 1, 2, in a tap the channels ascending (the rule of pcgmix_conv3_nlc_f32
 *   for a single K group).  No split-K, no atomics: a sample's result is the same bits in every
 *   launch, at every B and at every place in the batch.  A row outside the sample is zeros by a
 *   select on a clamped load.  The input gradient is the same call on dy with
 *   w'[i][tap][o] = w[o][2-tap][i].  Refusals and B == 0 as for pcgmix_conv3_nlc_f32.
 * pcgmix_conv3_narrow_wgrad_plan (models.py:468-473): as pcgmix_conv3_wgrad_plan, with K tiles of
 *   256 positions: *splits = min(1024, K tiles / 2), at least 1 — a function of (B, L) alone.
 * pcgmix_conv3_narrow_wgrad_nlc_f32 (models.py:468-473): the contract of
 *   pcgmix_conv3_wgrad_nlc_f32.  Split s adds the K tiles [s U / S, (s + 1) U / S) in ascending
 *   order; inside a block the thread groups combine through a fixed LDS tree (the file's header
 *   has it); a second launch adds the partials in ascending order with plain float32 adds.  No
 *   atomics, no grid-wide wait, no allocation; the workspace is never read before the same call
 *   has written it and nothing beyond the planned bytes is touched.  Refusals and B == 0 (zeros
 *   to dw) as for pcgmix_conv3_wgrad_nlc_f32.                                                    */
int pcgmix_conv3_narrow_supported(int Cin, int Cout);
int pcgmix_conv3_narrow_tile(int which);
int pcgmix_conv3_narrow_nlc_f32(const float* x, const float* w, float* y, int B, int L, int Cin, int Cout,
                                pcgmix_stream_t stream);
int pcgmix_conv3_narrow_wgrad_plan(int B, int L, int Cin, int Cout, int* splits, size_t* workspace_bytes);
int pcgmix_conv3_narrow_wgrad_nlc_f32(const float* x, const float* dy, float* dw, void* workspace,
                                      size_t workspace_bytes, int B, int L, int Cin, int Cout,
                                      pcgmix_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conv2d(k = 3x3, pad = 1, stride 1) of ResNet9-2D, channels innermost.             [device]
 * csrc/pcgmix_conv3x3.hip (conv3x3_kernel, first_kernel, last_kernel).
 *
 * Replaces nn.Conv2d(c_in, c_out, kernel_size=3, padding=1) of conv_block (models2d.py:6-11)
 * where its weights are frozen: the evaluation pass (train_model.py:591-670) and the frozen
 * saliency pass on spectrograms (saliency.py:26-61, 93-113).  No bias (the BatchNorm kernels
 * above take it).
 *   x (B, H, W, Cin)     the memory of a (B, Cin, H, W) channels_last tensor
 *   w (Cout, 3, 3, Cin)  [o][kh][kw][i], the memory models2d.ResNet9_myrtle gives its Conv2d weights
 *   y (B, H, W, Cout)    y[b][h][v][o] = sum over kh, kw, i of x[b][h+kh-1][v+kw-1][i] * w[o][kh][kw][i],
 *                        x zero outside [0, H) x [0, W) of every sample
 * The layer's input gradient is the same call on dy with w'[i][kh][kw][o] = w[o][2-kh][2-kw][i].
 * One launch.  Every output element is summed in ONE fixed order that is a function of (Cin, Cout)
 * alone — no split-K, no atomics — so a sample's result is the same bits in every launch, at every B
 * and at every place in the batch:
 *   Cin % 16 == 0 and Cout % 16 == 0: one float32 fmaf chain from +0 on v_mfma_f32_32x32x2_f32 over
 *     groups of 16 input channels ascending; in a group kh = 0, 1, 2; in a kh kw = 0, 1, 2; in a tap
 *     the channels ascending.
 *   Cin == 1: one fmaf chain from +0 over the nine taps, (kh, kw) = (0,0), (0,1) .. (2,2).
 *   Cout == 1: per input pixel and tap, sixteen fmaf chains (chain l: channels 4q .. 4q+3 of the quads
 *     q = l, l+16, .. ascending) added in a butterfly (distance 8, 4, 2, 1); then the nine taps' values
 *     are added to +0 in (kh, kw) order with float32 adds, +0 for a tap outside the sample.
 * pcgmix_conv3x3_supported (models2d.py:6-11): 1 for (Cin == 1 or Cin % 16 == 0, Cin <= 1024) and
 *   (Cout == 1 or Cout % 16 == 0, Cout <= 1024), not both 1; else 0.  Host only: no device is touched.
 * pcgmix_conv3x3_tile (models2d.py:6-11): the matrix kernel's tile constants, for tests that place
 *   shapes at tile edges: which = 0 the rows of one tile of output pixels (8), 1 its columns (16),
 *   2 the input channels of one K group (16), else 0.  Host only.
 * pcgmix_conv3x3_nhwc_f32 (models2d.py:6-11; saliency.py:26-61, 93-113; train_model.py:591-670):
 *   refused with hipErrorInvalidValue, nothing launched and y untouched: unsupported widths, a NULL
 *   pointer, a pointer that is not 16-byte aligned, B < 0, H < 1, W < 1, H * W * max(Cin, Cout) >
 *   INT_MAX, more than INT_MAX blocks.  B == 0 returns 0 and launches nothing.  x and y may not overlap. */
int pcgmix_conv3x3_supported(int Cin, int Cout);
int pcgmix_conv3x3_tile(int which);
int pcgmix_conv3x3_nhwc_f32(const float* x, const float* w, float* y, int B, int H, int W, int Cin,
                            int Cout, pcgmix_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCGMIX_HIP_H */
