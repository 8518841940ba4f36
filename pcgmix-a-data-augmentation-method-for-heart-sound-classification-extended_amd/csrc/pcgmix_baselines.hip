// pcgmix_baselines.hip — the paper's comparison augmentations for gfx950 (MI355X).
//
// The reference runs them through the same augment() call as PCGmix (augmentations.py:777-862,
// 1002-1048; the spectrogram ones through augmentations2d.py:461-617); here each is one launch on
// the caller's stream:
//
//   mixup(same|mix)      blend_rows_kernel    y[b] = x[b]*lam + x[mix[b]]*(1-lam)      fp32, unfused
//   magnitudewarp        scale_rows_kernel    y = float(double(x) * S_bc(t))           whole row
//   respiratoryscale     scale_rows_kernel    y = float(double(x) * s[t])              s from numpy
//   timemask             zero_spans_kernel    x[b, :, s0:s1] = 0                       in place
//   timewarp             time_warp_kernel     np.interp(arange(T), xp, x_row), xp from the spline
//   2D timemask/freqmask zero_rects_kernel    x[b, :, f0:f1, t0:t1] = 0                in place
//
// (2D mixup and latentmixup's blend are blend_rows_kernel on the flat sample planes; 2D cutmix and
// durratiocutmix are the segment-table kernel of pcgmix_cutpaste.hip.)
//
// The first four stream (8 algorithmic bytes per element, 12 for the blend: the partner row is
// a second read).  The time warp is one workgroup per (b, c) row: xp in LDS (global workspace
// above kTwLdsMaxT), a block-wide test whether xp is non-decreasing — then every query is an
// independent binary search — and otherwise numpy's own sequential search-with-guess on one lane.
// The numpy restatement (np_bsearch_guess / np_interp_pick) is __host__ __device__ and exported
// for the host as pcgmix_np_interp_f64 / pcgmix_time_warp_row_f64, so the CPU suite fuzzes the
// very code the kernel runs against numpy.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pcgmix_kernels.h"

namespace pcgmix {
namespace {

constexpr int kThreadsB = 256;
constexpr int kUnrollB = 4;                         // quads in flight per lane
constexpr int kEpbB = kThreadsB * 4 * kUnrollB;     // elements per block of the streaming kernels
constexpr int kZeroChunk = kThreadsB * 4;           // rectangle elements per block
constexpr int kMaxKnotsB = 64;
constexpr int kTwLdsMaxT = 5120;                    // 12 B per sample (xp f64 + index i32) <= 60 KB

// ---- numpy's interp (numpy/_core/src/multiarray/compiled_base.c) ------------------------------
// binary_search_with_guess: -1 below xp[0], len above xp[len-1]; linear for len <= 4; otherwise the
// guess (clamped to [1, len-3]) and its neighbours first, then a window of 8, then bisection.
__host__ __device__ inline long long np_bsearch_guess(double key, const double* arr, long long len,
                                                      long long guess) {
  constexpr long long kCache = 8;  // LIKELY_IN_CACHE_SIZE
  long long imin = 0, imax = len;
  if (key > arr[len - 1]) return len;
  if (key < arr[0]) return -1;
  if (len <= 4) {
    long long i = 1;
    while (i < len && key >= arr[i]) ++i;
    return i - 1;
  }
  if (guess > len - 3) guess = len - 3;
  if (guess < 1) guess = 1;
  if (key < arr[guess]) {
    if (key < arr[guess - 1]) {
      imax = guess - 1;
      if (guess > kCache && key >= arr[guess - kCache]) imin = guess - kCache;
    } else {
      return guess - 1;
    }
  } else {
    if (key < arr[guess + 1]) return guess;
    if (key < arr[guess + 2]) return guess + 1;
    imin = guess + 2;
    if (guess < len - kCache - 1 && key < arr[guess + kCache]) imax = guess + kCache;
  }
  while (imin < imax) {
    const long long imid = imin + ((imax - imin) >> 1);
    if (key >= arr[imid]) imin = imid + 1;
    else imax = imid;
  }
  return imin - 1;
}

// The value numpy's interp loop stores for search result j (left = fp[0], right = fp[n-1]).
template <typename FP>
__host__ __device__ inline double np_interp_pick(double key, long long j, const double* xp,
                                                 const FP* fp, long long n) {
  if (j < 0) return (double)fp[0];
  if (j >= n) return (double)fp[n - 1];
  if (j == n - 1) return (double)fp[j];
  if (xp[j] == key) return (double)fp[j];
  const double f0 = (double)fp[j], f1 = (double)fp[j + 1];
  const double slope = (f1 - f0) / (xp[j + 1] - xp[j]);
  double r = slope * (key - xp[j]) + f0;
  if (isnan(r)) {  // "if we get nan in one direction, try the other"
    r = slope * (key - xp[j + 1]) + f1;
    if (isnan(r) && f0 == f1) r = f0;
  }
  return r;
}

// Last j with xp[j] <= key (-1 if none) on a NON-DECREASING xp: there the guess never changes the
// answer of np_bsearch_guess (j == len and j == len-1 give the same value).
__host__ __device__ inline long long last_le(double key, const double* xp, long long n) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (key >= xp[mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// ---- the warp splines (pcgmix_spline_operator_f64 layout) -------------------------------------
// coef[p*4 + j4] = sum_i op[n + (p*4+j4)*n + i] * v[i], accumulated in i order from 0.0 as the
// splice's warp stage does (pcgmix_mix.hip build_records).
__host__ __device__ inline double spline_coef(const double* op, int n, int k, const double* v,
                                              long long v_stride) {
  const double* row = op + n + (size_t)k * n;
  double acc = 0.0;
  for (int i = 0; i < n; ++i) acc = acc + row[i] * v[i * v_stride];
  return acc;
}

// scipy's PPoly evaluation at integer t (piece = searchsorted(brk, t, 'right') - 1, clipped to the
// last piece; c3 + c2*s + c1*s^2 + c0*s^3 with a running power), every operation rounded in fp64.
__host__ __device__ inline double spline_eval(const double* coef, const double* brk, int n, int t) {
  int p = 0;
  for (int i = 1; i <= n - 2; ++i) p += ((double)t >= brk[i]) ? 1 : 0;
  const double* c = coef + p * 4;
  const double s = (double)t - brk[p];
  double r = c[3] + c[2] * s;
  double z = s * s;
  r = r + c[1] * z;
  z = z * s;
  return r + c[0] * z;
}

// time_warp's xp (augmentations.py:692-694): clip(scale * tw, 0, T-1) with scale = (T-1)/tw[T-1]
__host__ __device__ inline double tw_xp(const double* coef, const double* brk, int n, int t,
                                        double scale, double hi) {
  double v = scale * spline_eval(coef, brk, n, t);
  v = v < 0.0 ? 0.0 : v;
  return v > hi ? hi : v;
}

// ---- streaming kernels ------------------------------------------------------------------------
// mixup: sample b's plane blended with its partner's (augmentations.py:846, 856): fp32 mul, mul,
// add, (1-lam) formed in fp32 by the caller.  grid (B, chunks of the plane).
template <bool VEC>
__global__ __launch_bounds__(kThreadsB) void blend_rows_kernel(const float* __restrict__ x,
                                                               float* __restrict__ y,
                                                               const int32_t* __restrict__ mix,
                                                               float lam, float oml, int B,
                                                               long long plane) {
  const int b = blockIdx.x;
  int m = mix[b];
  m = (m < 0 || m >= B) ? b : m;  // memory safety; the host validates as well
  const float* xo = x + (size_t)b * plane;
  const float* xm = x + (size_t)m * plane;
  float* yo = y + (size_t)b * plane;
  const long long base = (long long)blockIdx.y * kEpbB;
  if (VEC) {
    float4_a a[kUnrollB], p[kUnrollB];
#pragma unroll
    for (int u = 0; u < kUnrollB; ++u) {
      const long long i = base + ((long long)u * kThreadsB + threadIdx.x) * 4;
      if (i < plane) {
        a[u] = *reinterpret_cast<const float4_a*>(xo + i);
        p[u] = *reinterpret_cast<const float4_a*>(xm + i);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnrollB; ++u) {
      const long long i = base + ((long long)u * kThreadsB + threadIdx.x) * 4;
      if (i < plane) {
        float4_a r;
        r.x = __fadd_rn(__fmul_rn(a[u].x, lam), __fmul_rn(p[u].x, oml));
        r.y = __fadd_rn(__fmul_rn(a[u].y, lam), __fmul_rn(p[u].y, oml));
        r.z = __fadd_rn(__fmul_rn(a[u].z, lam), __fmul_rn(p[u].z, oml));
        r.w = __fadd_rn(__fmul_rn(a[u].w, lam), __fmul_rn(p[u].w, oml));
        __builtin_nontemporal_store(r, reinterpret_cast<float4_a*>(yo + i));
      }
    }
  } else {
    const long long end = base + kEpbB < plane ? base + kEpbB : plane;
    for (long long i = base + threadIdx.x; i < end; i += kThreadsB)
      yo[i] = __fadd_rn(__fmul_rn(xo[i], lam), __fmul_rn(xm[i], oml));
  }
}

// magnitudewarp (SPLINE) and respiratoryscale (!SPLINE): y = float(double(x) * w[t]) over whole
// rows.  grid (B*C, chunks of a row); the spline's coefficient records of the block's row are built
// in LDS first (knots (B, n, C) as numpy drew them).
template <bool SPLINE, bool VEC>
__global__ __launch_bounds__(kThreadsB) void scale_rows_kernel(const float* __restrict__ x,
                                                               float* __restrict__ y,
                                                               const double* __restrict__ knots,
                                                               const double* __restrict__ op,
                                                               int n, const double* __restrict__ s,
                                                               int C, int T) {
  __shared__ double coef[(kMaxKnotsB - 1) * 4];
  __shared__ double brk[kMaxKnotsB];
  const long long row = blockIdx.x;
  const int b = (int)(row / C), c = (int)(row % C);
  if (SPLINE) {
    for (int i = threadIdx.x; i < n; i += kThreadsB) brk[i] = op[i];
    for (int k = threadIdx.x; k < (n - 1) * 4; k += kThreadsB)
      coef[k] = spline_coef(op, n, k, knots + (size_t)b * n * C + c, C);
    __syncthreads();
  }
  const float* xr = x + (size_t)row * T;
  float* yr = y + (size_t)row * T;
  const int base = blockIdx.y * kEpbB;
  auto w = [&](int t) -> double { return SPLINE ? spline_eval(coef, brk, n, t) : s[t]; };
  if (VEC) {
    float4_a a[kUnrollB];
#pragma unroll
    for (int u = 0; u < kUnrollB; ++u) {
      const int t = base + (u * kThreadsB + (int)threadIdx.x) * 4;
      if (t < T) a[u] = *reinterpret_cast<const float4_a*>(xr + t);
    }
#pragma unroll
    for (int u = 0; u < kUnrollB; ++u) {
      const int t = base + (u * kThreadsB + (int)threadIdx.x) * 4;
      if (t < T) {
        float4_a r;
        r.x = (float)((double)a[u].x * w(t));
        r.y = (float)((double)a[u].y * w(t + 1));
        r.z = (float)((double)a[u].z * w(t + 2));
        r.w = (float)((double)a[u].w * w(t + 3));
        __builtin_nontemporal_store(r, reinterpret_cast<float4_a*>(yr + t));
      }
    }
  } else {
    const int end = base + kEpbB < T ? base + kEpbB : T;
    for (int t = base + threadIdx.x; t < end; t += kThreadsB) yr[t] = (float)((double)xr[t] * w(t));
  }
}

// timemask: x[b, :, s0:s1) = 0 in place (augmentations.py:822-826); spans (B, 2) clipped by the
// host, and again here.  grid (B*C); lanes stride over the span.
__global__ __launch_bounds__(kThreadsB) void zero_spans_kernel(float* __restrict__ x,
                                                               const int32_t* __restrict__ spans,
                                                               int C, int T) {
  const long long row = blockIdx.x;
  const int b = (int)(row / C);
  int s0 = spans[2 * b], s1 = spans[2 * b + 1];
  s0 = s0 < 0 ? 0 : (s0 > T ? T : s0);  // above as well: s0 + threadIdx.x must not wrap
  s1 = s1 > T ? T : s1;
  float* xr = x + (size_t)row * T;
  for (int t = s0 + threadIdx.x; t < s1; t += kThreadsB) xr[t] = 0.f;
}

// 2D timemask / freqmask (and any per-sample rectangle): rect (B, 4) = [f0, f1, t0, t1), applied to
// every channel, clipped to the plane here as well; only the zeroed elements are touched.
// grid (B*C, chunks of the largest rectangle).
__global__ __launch_bounds__(kThreadsB) void zero_rects_kernel(float* __restrict__ x,
                                                               const int32_t* __restrict__ rect,
                                                               int C, int F, int W) {
  const long long plane = blockIdx.x;
  const int b = (int)(plane / C);
  int f0 = rect[4 * b], f1 = rect[4 * b + 1], t0 = rect[4 * b + 2], t1 = rect[4 * b + 3];
  f0 = f0 < 0 ? 0 : f0;
  t0 = t0 < 0 ? 0 : t0;
  f1 = f1 > F ? F : f1;
  t1 = t1 > W ? W : t1;
  const int h = f1 - f0, w = t1 - t0;
  if (h <= 0 || w <= 0) return;
  const int area = h * w;
  const int lo = (int)blockIdx.y * kZeroChunk;
  if (lo >= area) return;
  const int hi = lo + kZeroChunk < area ? lo + kZeroChunk : area;
  float* xp = x + (size_t)plane * F * W + (size_t)f0 * W + t0;
  for (int i = lo + (int)threadIdx.x; i < hi; i += kThreadsB) {
    const int r = i / w, c = i - r * w;
    xp[r * W + c] = 0.f;
  }
}

// timewarp: one workgroup per (b, c) row.  LDS: xp (T doubles) then the search results (T ints)
// when T <= kTwLdsMaxT, otherwise the same two arrays in the caller's workspace.
template <bool LDS>
__global__ __launch_bounds__(kThreadsB) void time_warp_kernel(const float* __restrict__ x,
                                                              float* __restrict__ y,
                                                              const double* __restrict__ knots,
                                                              const double* __restrict__ op, int n,
                                                              int C, int T, double* ws_xp,
                                                              int* ws_j) {
  extern __shared__ __align__(16) double dyn[];
  __shared__ double coef[(kMaxKnotsB - 1) * 4];
  __shared__ double brk[kMaxKnotsB];
  __shared__ double yv[kMaxKnotsB];
  const long long row = blockIdx.x;
  const int b = (int)(row / C), c = (int)(row % C);
  double* xp = LDS ? dyn : ws_xp + (size_t)row * T;
  int* jx = LDS ? reinterpret_cast<int*>(dyn + T) : ws_j + (size_t)row * T;
  // spline through (brk, brk * knots[b, :, c]): the products first (augmentations.py:692)
  for (int i = threadIdx.x; i < n; i += kThreadsB) {
    brk[i] = op[i];
    yv[i] = op[i] * knots[((size_t)b * n + i) * C + c];
  }
  __syncthreads();
  for (int k = threadIdx.x; k < (n - 1) * 4; k += kThreadsB) coef[k] = spline_coef(op, n, k, yv, 1);
  __syncthreads();
  const double hi = (double)(T - 1);
  const double scale = hi / spline_eval(coef, brk, n, T - 1);
  for (int t = threadIdx.x; t < T; t += kThreadsB) xp[t] = tw_xp(coef, brk, n, t, scale, hi);
  __syncthreads();
  int dec = 0;
  for (int t = threadIdx.x + 1; t < T; t += kThreadsB) dec |= xp[t] < xp[t - 1];
  dec = __syncthreads_or(dec);
  const float* fp = x + (size_t)row * T;
  float* yr = y + (size_t)row * T;
  if (!dec) {
    for (int t = threadIdx.x; t < T; t += kThreadsB)
      yr[t] = (float)np_interp_pick((double)t, last_le((double)t, xp, T), xp, fp, T);
    return;
  }
  // a decreasing step: the guess matters, numpy's walk in query order on one lane
  if (threadIdx.x == 0) {
    long long j = 0;
    for (int t = 0; t < T; ++t) {
      j = np_bsearch_guess((double)t, xp, T, j);
      jx[t] = (int)j;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < T; t += kThreadsB)
    yr[t] = (float)np_interp_pick((double)t, (long long)jx[t], xp, fp, T);
}

// rows (or samples) along gridDim.x, whose limit is the 2^32 work-items of a dispatch; chunks of a
// row along gridDim.y (<= 65535)
inline bool grid_ok(long long rows, long long chunks) {
  return rows * kThreadsB < (1LL << 32) && chunks <= 65535;
}

}  // namespace
}  // namespace pcgmix

using namespace pcgmix;

extern "C" int pcgmix_blend_rows_f32(const float* x, float* y, const int32_t* mix, float lam,
                                     int B, int C, int T, pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || T <= 0) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const long long plane = (long long)C * T;
  const long long chunks = (plane + kEpbB - 1) / kEpbB;
  if (!x || !y || !mix || x == y || !grid_ok(B, chunks)) return hipErrorInvalidValue;
  const float oml = 1.0f - lam;  // (1 - lams_out) in float32, augmentations.py:846
  const dim3 grid((unsigned)B, (unsigned)chunks);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (plane % 4 == 0 && aligned16(x) && aligned16(y))
    hipLaunchKernelGGL(blend_rows_kernel<true>, grid, dim3(kThreadsB), 0, s, x, y, mix, lam, oml, B, plane);
  else
    hipLaunchKernelGGL(blend_rows_kernel<false>, grid, dim3(kThreadsB), 0, s, x, y, mix, lam, oml, B, plane);
  return hipGetLastError();
}

static int launch_scale_rows(const float* x, float* y, const double* knots, const double* op, int n,
                             const double* w, int B, int C, int T, hipStream_t s) {
  const long long rows = (long long)B * C, chunks = (T + kEpbB - 1) / kEpbB;
  if (!grid_ok(rows, chunks)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)rows, (unsigned)chunks);
  const bool vec = T % 4 == 0 && aligned16(x) && aligned16(y);
  if (op) {
    if (vec)
      hipLaunchKernelGGL((scale_rows_kernel<true, true>), grid, dim3(kThreadsB), 0, s, x, y, knots, op, n, w, C, T);
    else
      hipLaunchKernelGGL((scale_rows_kernel<true, false>), grid, dim3(kThreadsB), 0, s, x, y, knots, op, n, w, C, T);
  } else {
    if (vec)
      hipLaunchKernelGGL((scale_rows_kernel<false, true>), grid, dim3(kThreadsB), 0, s, x, y, knots, op, n, w, C, T);
    else
      hipLaunchKernelGGL((scale_rows_kernel<false, false>), grid, dim3(kThreadsB), 0, s, x, y, knots, op, n, w, C, T);
  }
  return hipGetLastError();
}

extern "C" int pcgmix_warp_rows_f32(const float* x, float* y, const double* knots,
                                    const double* spline_op, int n_knots, int B, int C, int T,
                                    pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || T < 2 || n_knots < 2 || n_knots > kMaxKnotsB) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!x || !y || !knots || !spline_op || x == y) return hipErrorInvalidValue;
  return launch_scale_rows(x, y, knots, spline_op, n_knots, nullptr, B, C, T,
                           reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcgmix_scale_rows_f32(const float* x, float* y, const double* s, int B, int C, int T,
                                     pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || T <= 0) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!x || !y || !s || x == y) return hipErrorInvalidValue;
  return launch_scale_rows(x, y, nullptr, nullptr, 0, s, B, C, T, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcgmix_zero_spans_f32(float* x, const int32_t* spans, int B, int C, int T,
                                     pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || T <= 0) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!x || !spans) return hipErrorInvalidValue;
  const long long rows = (long long)B * C;
  if (!grid_ok(rows, 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zero_spans_kernel, dim3((unsigned)rows), dim3(kThreadsB), 0, reinterpret_cast<hipStream_t>(stream),
                     x, spans, C, T);
  return hipGetLastError();
}

extern "C" int pcgmix_zero_rects_f32(float* x, const int32_t* rect, int B, int C, int F, int W,
                                     int max_area, pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || F <= 0 || W <= 0 || max_area < 0) return hipErrorInvalidValue;
  if (B == 0 || max_area == 0) return hipSuccess;
  if (!x || !rect) return hipErrorInvalidValue;
  const long long planes = (long long)B * C;
  if ((long long)F * W >= (1LL << 31)) return hipErrorInvalidValue;
  const long long area = (long long)F * W < max_area ? (long long)F * W : max_area;
  const long long chunks = (area + kZeroChunk - 1) / kZeroChunk;
  if (!grid_ok(planes, chunks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zero_rects_kernel, dim3((unsigned)planes, (unsigned)chunks), dim3(kThreadsB), 0,
                     reinterpret_cast<hipStream_t>(stream), x, rect, C, F, W);
  return hipGetLastError();
}

extern "C" long long pcgmix_time_warp_workspace_bytes(int B, int C, int T) {
  if (B < 0 || C <= 0 || T < 2) return -1;
  if (T <= kTwLdsMaxT) return 0;
  return (long long)B * C * T * (long long)(sizeof(double) + sizeof(int));
}

extern "C" int pcgmix_time_warp_f32(const float* x, float* y, const double* knots,
                                    const double* spline_op, int n_knots, void* workspace, int B,
                                    int C, int T, pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || T < 2 || n_knots < 2 || n_knots > kMaxKnotsB) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!x || !y || !knots || !spline_op || x == y) return hipErrorInvalidValue;
  const long long rows = (long long)B * C;
  if (!grid_ok(rows, 1)) return hipErrorInvalidValue;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool lds = T <= kTwLdsMaxT;
  if (!lds && !workspace) return hipErrorInvalidValue;
  double* ws_xp = lds ? nullptr : static_cast<double*>(workspace);
  int* ws_j = lds ? nullptr : reinterpret_cast<int*>(ws_xp + (size_t)rows * T);
  if (lds)
    hipLaunchKernelGGL(time_warp_kernel<true>, dim3((unsigned)rows), dim3(kThreadsB),
                       (size_t)T * (sizeof(double) + sizeof(int)), s, x, y, knots, spline_op, n_knots,
                       C, T, ws_xp, ws_j);
  else
    hipLaunchKernelGGL(time_warp_kernel<false>, dim3((unsigned)rows), dim3(kThreadsB), 0, s, x, y, knots,
                       spline_op, n_knots, C, T, ws_xp, ws_j);
  return hipGetLastError();
}

extern "C" int pcgmix_np_interp_f64(const double* x, long long nx, const double* xp,
                                    const double* fp, long long n, double* out) {
  if (nx < 0 || n < 1 || (nx && (!x || !out)) || !xp || !fp) return hipErrorInvalidValue;
  long long j = 0;
  for (long long i = 0; i < nx; ++i) {
    const double key = x[i];
    if (isnan(key)) {
      out[i] = key;
      continue;
    }
    if (n == 1) {  // numpy's one-point branch (left = right = fp[0])
      out[i] = fp[0];
      continue;
    }
    j = np_bsearch_guess(key, xp, n, j);
    out[i] = np_interp_pick(key, j, xp, fp, n);
  }
  return hipSuccess;
}

extern "C" int pcgmix_time_warp_row_f64(const double* spline_op, const double* knots, int n_knots,
                                        const float* x, int T, float* y, double* xp_out) {
  if (!spline_op || !knots || !x || !y || T < 2 || n_knots < 2 || n_knots > kMaxKnotsB)
    return hipErrorInvalidValue;
  double coef[(kMaxKnotsB - 1) * 4], yv[kMaxKnotsB];
  const double* brk = spline_op;
  for (int i = 0; i < n_knots; ++i) yv[i] = brk[i] * knots[i];
  for (int k = 0; k < (n_knots - 1) * 4; ++k) coef[k] = spline_coef(spline_op, n_knots, k, yv, 1);
  const double hi = (double)(T - 1);
  const double scale = hi / spline_eval(coef, brk, n_knots, T - 1);
  double* xp = new double[(size_t)T];
  for (int t = 0; t < T; ++t) xp[t] = tw_xp(coef, brk, n_knots, t, scale, hi);
  long long j = 0;
  for (int t = 0; t < T; ++t) {
    j = np_bsearch_guess((double)t, xp, T, j);
    y[t] = (float)np_interp_pick((double)t, j, xp, x, T);
  }
  if (xp_out)
    for (int t = 0; t < T; ++t) xp_out[t] = xp[t];
  delete[] xp;
  return hipSuccess;
}
