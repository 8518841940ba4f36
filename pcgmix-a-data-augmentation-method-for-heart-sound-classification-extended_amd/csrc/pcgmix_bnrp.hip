// pcgmix_bnrp.hip — BatchNorm + ReLU + MaxPool of the ResNet9 blocks as fused NHWC kernels
// (gfx950): training mode (forward + backward) and eval mode (forward + input gradient).
//
// Reference: models.py:468-473 / models2d.py:13-19 (conv_block: Conv + BatchNorm + ReLU [+ MaxPool]).
// The convolutions run at ~130 TFLOP/s fp32 through MIOpen's implicit-GEMM kernels (84 % of the
// matrix peak); what is left of a ResNet9 step is memory-bound elementwise work on activations of
// 0.3-0.65 GB each: BatchNorm forward (2 kernels), ReLU, pooling, and their backward twins
// (pool, ReLU, two BatchNorm kernels) — nine to ten passes over the activation per block, each
// through HBM.  Here, with y = conv output (rows x C, channels innermost):
//
//   forward   bn_stats_kernel        one read of y  -> per-block (sum, sum of squares) of y - y[0, c] per channel
//             bn_finalize_kernel     mean, 1/std, running-stat update (float64 combination)
//             bnrp_fwd_kernel        one read of y  -> z = maxpool(relu(gamma * xhat + beta)) [+ skip]
//   backward  bnrp_bwd_reduce_kernel one read of y, dz -> sums of dy and dy * xhat per channel
//             bn_bwd_finalize_kernel dgamma, dbeta, the two means BatchNorm's dx needs
//             bnrp_dx_kernel         one read of y, dz -> dx (one write)
//   eval      bnrp_fwd_kernel        the same kernel, scale and shift from the running statistics
//             bnrp_dx_kernel         the same kernel, dx = scale * dz at the arg-max, 0 elsewhere
//
// bnrp_fwd_kernel and bnrp_dx_kernel are templates over <Window, Stats, V>: Stats (TrainStats or
// EvalStats) says where scale and shift come from and which rule gives dx; Window (FixedWindow<PH,
// PW> or AnyWindow) picks the loop: loads-before-first-use with 32-bit indices for the window
// shapes ResNet9 uses, a runtime window with 64-bit indices for everything else (with_window).
//
// The ReLU mask and the pooling arg-max are recomputed from y (first maximum wins, as in torch's
// max_pool), so nothing but y, mean and 1/std is kept for backward.  Five passes instead of ten.
// All reductions are fixed-order (deterministic).  HBM-bound: 4 bytes per element per pass.
//
// Channel counts: a thread owns one vector of a row's channels (V = float4: Q = C / 4 vectors per
// row; V = float2 for C = 2: Q = 1) and keeps it across the grid stride, so every stride must be a
// multiple of Q.  A block therefore has A = (256 / Q) * Q threads: 256 where Q divides 256, the
// largest multiple of Q below it otherwise (C = 96: 240, C = 768: 192), and all strides and the
// LDS reduction run over A.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <cmath>
#include <initializer_list>

#include "pcgmix_kernels.h"

namespace pcgmix {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int kBnThreads = 256;       // most threads of a block (LDS is sized for it)
constexpr int kBnMaxBlocks = 1024;
constexpr int kBnMaxC = 1024;         // widest row: 256 float4
constexpr int kFinCh = 16;            // channels per finalize block (x 16 partial-row lanes)

struct BnShape {
  int B, H, W, C, ph, pw, Ho, Wo;
  int Q;   // vectors per row (C / 4; 1 for C = 2)
  int A;   // threads per block: (kBnThreads / Q) * Q
};

template <typename V>
constexpr int kLanes = (int)(sizeof(V) / sizeof(float));

template <typename V>
__device__ __forceinline__ V vsplat(float x) {
  V v;
#pragma unroll
  for (int e = 0; e < kLanes<V>; ++e) v[e] = x;
  return v;
}

template <typename V>
__device__ __forceinline__ V vfma(V a, V b, V c) {
  V r;
#pragma unroll
  for (int e = 0; e < kLanes<V>; ++e) r[e] = fmaf(a[e], b[e], c[e]);
  return r;
}

// the vector of channel group q of a per-channel array
template <typename V>
__device__ __forceinline__ V vchan(const float* __restrict__ p, int q) {
  return *reinterpret_cast<const V*>(p + kLanes<V> * q);
}

// Sum the per-thread vectors of the threads that share a channel group (tid % Q) in a fixed
// order and let thread q < Q write the result for group q.
template <typename V>
__device__ __forceinline__ void quad_reduce_store(V a, V b, int Q, int A, V* lds, float* out0,
                                                  float* out1) {
  const int tid = threadIdx.x;
  lds[tid] = a;
  lds[kBnThreads + tid] = b;
  __syncthreads();
  if (tid < Q) {
    V sa = lds[tid], sb = lds[kBnThreads + tid];
    for (int j = tid + Q; j < A; j += Q) {
      sa += lds[j];
      sb += lds[kBnThreads + j];
    }
    *reinterpret_cast<V*>(out0 + kLanes<V> * tid) = sa;
    *reinterpret_cast<V*>(out1 + kLanes<V> * tid) = sb;
  }
}

// ------------------------------------------------------------------------------------ forward
template <typename V>
__global__ __launch_bounds__(kBnThreads) void bn_stats_kernel(const V* __restrict__ y,
                                                              long long n4, int Q, int A,
                                                              float* __restrict__ partial, int C) {
  __shared__ V lds[2 * kBnThreads];
  V s = vsplat<V>(0.f), ss = vsplat<V>(0.f);
  const long long stride = (long long)gridDim.x * A;              // multiple of Q
  long long i = (long long)blockIdx.x * A + threadIdx.x;
  // Sums of y - K and (y - K)^2 about the pivot K_c = y[0, c] (the thread's channel group of row 0):
  // var = E[(y-K)^2] - E[y-K]^2 then cancels digits in proportion to |mean - K| / std, not |mean| / std.
  const V K = y[threadIdx.x % Q];
  for (; i + 3 * stride < n4; i += 4 * stride) {   // four loads in flight per lane (a pure reader
    const V v0 = y[i] - K, v1 = y[i + stride] - K, v2 = y[i + 2 * stride] - K, v3 = y[i + 3 * stride] - K;
    s += v0; ss = vfma(v0, v0, ss);                 // has no store to hide a load-wait-load chain behind)
    s += v1; ss = vfma(v1, v1, ss);
    s += v2; ss = vfma(v2, v2, ss);
    s += v3; ss = vfma(v3, v3, ss);
  }
  for (; i < n4; i += stride) {
    const V v = y[i] - K;
    s += v;
    ss = vfma(v, v, ss);
  }
  float* p = partial + (size_t)blockIdx.x * 2 * C;
  quad_reduce_store(s, ss, Q, A, lds, p, p + C);
}

// Sum of the per-block partials of 16 channels: 16 lanes per channel stride over the blocks in
// float64, then a fixed-order combination through LDS.  (One thread per channel walking 1024+
// partials serially took 0.5 ms per call — more than the pass over the activation itself.)
__device__ __forceinline__ void partial_sums(const float* __restrict__ partial, int nblk, int C,
                                             int c, int lane, double (*lds)[kFinCh][16], double* s0,
                                             double* s1) {
  double a = 0.0, b = 0.0;
  if (c < C) {
    int k = lane;
    for (; k + 7 * 16 < nblk; k += 8 * 16) {       // eight pairs of loads in flight, added in order
      float va[8], vb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        va[u] = partial[(size_t)(k + 16 * u) * 2 * C + c];
        vb[u] = partial[(size_t)(k + 16 * u) * 2 * C + C + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        a += (double)va[u];
        b += (double)vb[u];
      }
    }
    for (; k < nblk; k += 16) {
      a += (double)partial[(size_t)k * 2 * C + c];
      b += (double)partial[(size_t)k * 2 * C + C + c];
    }
  }
  const int cl = threadIdx.x % kFinCh;
  lds[0][cl][lane] = a;
  lds[1][cl][lane] = b;
  __syncthreads();
  a = b = 0.0;
  for (int k = 0; k < 16; ++k) {
    a += lds[0][cl][k];
    b += lds[1][cl][k];
  }
  *s0 = a;
  *s1 = b;
}

// var is the biased batch variance (normalisation); the running variance gets the unbiased one,
// as torch.nn.BatchNorm does.  Block = 16 channels x 16 lanes.
__global__ __launch_bounds__(kFinCh * 16) void bn_finalize_kernel(
    const float* __restrict__ partial, const float* __restrict__ pivot, int nblk, int C, double n_rows,
    float eps, float momentum, float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, const float* __restrict__ mean_shift,
    long long* __restrict__ batches_tracked) {
  // mean_shift: a per-channel constant that was left out of y (the convolution's bias, which the
  // normalisation cancels): it belongs in the running mean.  batches_tracked: nn.BatchNorm's counter.
  if (batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) batches_tracked[0] += 1;
  __shared__ double lds[2][kFinCh][16];
  const int c = blockIdx.x * kFinCh + threadIdx.x % kFinCh, lane = threadIdx.x / kFinCh;
  double s, ss;
  partial_sums(partial, nblk, C, c, lane, lds, &s, &ss);
  if (c >= C || lane != 0) return;
  const double d = s / n_rows;                       // mean of y - K, K = pivot[c] = y[0, c] (bn_stats_kernel)
  const double m = (double)pivot[c] + d;
  double var = ss / n_rows - d * d;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)m;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean)
    running_mean[c] = (1.f - momentum) * running_mean[c] +
                      momentum * ((float)m + (mean_shift ? mean_shift[c] : 0.f));
  if (running_var) {
    const double unbiased = n_rows > 1.0 ? var * n_rows / (n_rows - 1.0) : var;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

// The affine map in front of the ReLU for channel group q.  Training: from the batch statistics
// the finalize kernel left.
template <typename V>
struct BnAffine {
  V scale, shift, mu, is;
};

template <typename V>
__device__ __forceinline__ BnAffine<V> train_affine(const float* __restrict__ gamma,
                                                    const float* __restrict__ beta,
                                                    const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, int q) {
  BnAffine<V> a;
  const V g = vchan<V>(gamma, q), bt = vchan<V>(beta, q);
  a.mu = vchan<V>(mean, q);
  a.is = vchan<V>(invstd, q);
  a.scale = g * a.is;
  a.shift = bt - a.mu * a.scale;
  return a;
}

// Eval: from the running statistics; `bias` (optional) is the convolution's bias that was left out
// of y, i.e. BN(y + bias) with the running mean == BN(y) with (running mean - bias).
template <typename V>
__device__ __forceinline__ BnAffine<V> eval_affine(const float* __restrict__ gamma,
                                                   const float* __restrict__ beta,
                                                   const float* __restrict__ running_mean,
                                                   const float* __restrict__ running_var,
                                                   const float* __restrict__ bias, float eps, int q) {
  BnAffine<V> a;
  const V g = vchan<V>(gamma, q), bt = vchan<V>(beta, q), rv = vchan<V>(running_var, q);
  a.mu = vchan<V>(running_mean, q);
  if (bias) a.mu -= vchan<V>(bias, q);
#pragma unroll
  for (int e = 0; e < kLanes<V>; ++e) a.is[e] = 1.f / sqrtf(rv[e] + eps);
  a.scale = g * a.is;
  a.shift = bt - a.mu * a.scale;
  return a;
}

// The per-channel arrays of a launch, passed to the kernels by value.  kBatch: the statistics are
// the batch's own, so the input gradient carries BatchNorm's two mean terms.
struct TrainStats {
  static constexpr bool kBatch = true;
  const float *__restrict__ gamma, *__restrict__ beta, *__restrict__ mean, *__restrict__ invstd;
  template <typename V>
  __device__ __forceinline__ BnAffine<V> affine(int q) const {
    return train_affine<V>(gamma, beta, mean, invstd, q);
  }
};

struct EvalStats {
  static constexpr bool kBatch = false;
  const float *__restrict__ gamma, *__restrict__ beta, *__restrict__ running_mean,
      *__restrict__ running_var, *__restrict__ bias;
  float eps;
  template <typename V>
  __device__ __forceinline__ BnAffine<V> affine(int q) const {
    return eval_affine<V>(gamma, beta, running_mean, running_var, bias, eps, q);
  }
};

// The pooling window as a kernel template argument: known at compile time (with 32-bit indexing),
// or read from the BnShape (with 64-bit indexing).  with_window() maps a shape to its tag.
template <int PH_, int PW_>
struct FixedWindow {
  static constexpr bool kFixed = true;
  static constexpr int PH = PH_, PW = PW_;
};
struct AnyWindow {
  static constexpr bool kFixed = false;
};

// row of pooled outputs -> (b, ho, wo)
struct PoolPos {
  long long b;
  int ho, wo;
};
__device__ __forceinline__ PoolPos pool_pos(const BnShape& s, long long orow) {
  PoolPos p;
  p.wo = (int)(orow % s.Wo);
  const long long t = orow / s.Wo;
  p.ho = (int)(t % s.Ho);
  p.b = t / s.Ho;
  return p;
}

// ReLU that keeps a NaN (torch.relu does): a diverged activation must reach the loss, not turn
// into zeros.  -0.0 and everything below give +0.0.
__device__ __forceinline__ float relu_nan(float a) { return a <= 0.f ? 0.f : a; }

// relu(scale * y + shift) at the ph x pw window of pooled position (b, ho, wo), channel group q;
// returns the maximum and (through *arg) the index i * pw + j of its FIRST occurrence.
// If `raw` is given it receives y itself at that first maximum (what the backward's xhat needs:
// re-reading it by index is a dependent scalar gather per channel).
template <typename V>
__device__ __forceinline__ V window_max(const V* __restrict__ y, const BnShape& s, long long b,
                                        int ho, int wo, int q, V scale, V shift,
                                        int (&arg)[kLanes<V>], V* raw = nullptr) {
  V best = vsplat<V>(-1.f);                           // relu output is >= 0: any value beats this
  V vb = vsplat<V>(0.f);
  for (int i = 0; i < s.ph; ++i)
    for (int j = 0; j < s.pw; ++j) {
      const long long row = (b * s.H + (ho * s.ph + i)) * s.W + (wo * s.pw + j);
      const V v = y[row * s.Q + q];
      V a = vfma(v, scale, shift);
      const int idx = i * s.pw + j;
#pragma unroll
      for (int e = 0; e < kLanes<V>; ++e) {
        const float r = relu_nan(a[e]);
        if (r > best[e] || r != r) {                  // a NaN wins and stays, as in torch's max_pool
          best[e] = r;
          arg[e] = idx;
          vb[e] = v[e];
        }
      }
    }
  if (raw) *raw = vb;
  return best;
}

// z = maxpool(relu(scale * y + shift)) [+ skip], any window
template <typename V>
__device__ __forceinline__ void apply_rows(const V* __restrict__ y, const V* __restrict__ skip,
                                           V* __restrict__ z, const BnShape& s, int q, V scale,
                                           V shift) {
  const long long n_out = (long long)s.B * s.Ho * s.Wo * s.Q;
  const long long stride = (long long)gridDim.x * s.A;
  for (long long o = (long long)blockIdx.x * s.A + threadIdx.x; o < n_out; o += stride) {
    const PoolPos p = pool_pos(s, o / s.Q);
    int arg[kLanes<V>];
    V v = window_max(y, s, p.b, p.ho, p.wo, q, scale, shift, arg);
    if (skip) v += skip[o];                           // residual connection (models.py:577, 581)
    z[o] = v;
  }
}

// ------------------------------------------------------------------------------------ fixed windows
// The window shapes ResNet9 uses ((1,1), (1,2), (2,2)) with index ranges that fit 32 bits.  The
// generic loops walk the window with runtime bounds: one global load, one s_waitcnt vmcnt(0), the
// next load — and the backward reduction then waits once more for dz.  A forward pass hides that
// behind its store (fire and forget), a pure reader does not: the generic backward reduction ran
// at 2.4-2.8 TB/s where the forward reaches 6.0 (profiles/r2_resnet1d_step_kernels.csv).  With a
// FixedWindow every thread handles TWO pooled rows per iteration and issues all of their loads
// (2 x PH x PW of y, 2 of dz) before the first use; row -> (b, ho, wo) is 32-bit arithmetic (the
// generic 64-bit divisions are ~100 instructions each).  A block covers R = A / Q pooled rows per
// step.
template <int PH, int PW>
__device__ __forceinline__ unsigned window_row(const BnShape& s, unsigned r) {
  const unsigned wo = r % (unsigned)s.Wo, t = r / (unsigned)s.Wo;
  const unsigned ho = t % (unsigned)s.Ho, b = t / (unsigned)s.Ho;
  return (b * (unsigned)s.H + ho * PH) * (unsigned)s.W + wo * PW;      // first input row of the window
}

template <int PH, int PW, typename V>
__device__ __forceinline__ void window_load(const V* __restrict__ y, const BnShape& s, unsigned row0,
                                            int q, V (&v)[PH * PW]) {
#pragma unroll
  for (int i = 0; i < PH; ++i)
#pragma unroll
    for (int j = 0; j < PW; ++j)
      v[i * PW + j] = y[(size_t)(row0 + (unsigned)i * (unsigned)s.W + (unsigned)j) * s.Q + q];
}

// window_max on registers: maximum of relu(scale * y + shift), index of its FIRST occurrence, and
// y itself there.
template <int N, typename V>
__device__ __forceinline__ V window_best(const V (&v)[N], V scale, V shift, int (&arg)[kLanes<V>],
                                         V* raw) {
  V best = vsplat<V>(-1.f), vb = vsplat<V>(0.f);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const V a = vfma(v[k], scale, shift);
#pragma unroll
    for (int e = 0; e < kLanes<V>; ++e) {
      const float r = relu_nan(a[e]);
      if (r > best[e] || r != r) {
        best[e] = r;
        arg[e] = k;
        vb[e] = v[k][e];
      }
    }
  }
  *raw = vb;
  return best;
}

template <int PH, int PW, typename V>
__device__ __forceinline__ void apply_win_rows(const V* __restrict__ y, const V* __restrict__ skip,
                                               V* __restrict__ z, const BnShape& s, int q, V scale,
                                               V shift) {
  const unsigned R = s.A / s.Q, rloc = threadIdx.x / s.Q;
  const unsigned n_rows = (unsigned)s.B * s.Ho * s.Wo, stride = gridDim.x * R;
  for (unsigned r = blockIdx.x * R + rloc; r < n_rows; r += 2 * stride) {
    const bool two = r + stride < n_rows;
    const unsigned r2 = two ? r + stride : r;
    V va[PH * PW], vb[PH * PW];
    window_load<PH, PW>(y, s, window_row<PH, PW>(s, r), q, va);
    window_load<PH, PW>(y, s, window_row<PH, PW>(s, r2), q, vb);
    V ka = vsplat<V>(0.f), kb = ka;
    if (skip) {
      ka = skip[(size_t)r * s.Q + q];
      kb = skip[(size_t)r2 * s.Q + q];
    }
    int arg[kLanes<V>];
    V raw;
    z[(size_t)r * s.Q + q] = window_best<PH * PW>(va, scale, shift, arg, &raw) + ka;
    if (two) z[(size_t)r2 * s.Q + q] = window_best<PH * PW>(vb, scale, shift, arg, &raw) + kb;
  }
}

template <typename Win, typename Stats, typename V>
__global__ __launch_bounds__(kBnThreads) void bnrp_fwd_kernel(const V* __restrict__ y, Stats st,
                                                              const V* __restrict__ skip,
                                                              V* __restrict__ z, BnShape s) {
  const int q = threadIdx.x % s.Q;                    // fixed per thread: strides are multiples of Q
  const BnAffine<V> a = st.template affine<V>(q);
  if constexpr (Win::kFixed)
    apply_win_rows<Win::PH, Win::PW>(y, skip, z, s, q, a.scale, a.shift);
  else
    apply_rows(y, skip, z, s, q, a.scale, a.shift);
}

// ------------------------------------------------------------------------------------ backward
template <typename Win, typename V>
__global__ __launch_bounds__(kBnThreads) void bnrp_bwd_reduce_kernel(
    const V* __restrict__ y, const V* __restrict__ dz, TrainStats st, float* __restrict__ partial,
    BnShape s) {
  __shared__ V lds[2 * kBnThreads];
  const int q = threadIdx.x % s.Q;
  const BnAffine<V> a = st.affine<V>(q);
  const V mu = a.mu, is = a.is, scale = a.scale, shift = a.shift;
  V s1 = vsplat<V>(0.f), s2 = vsplat<V>(0.f);
  if constexpr (Win::kFixed) {
    constexpr int PH = Win::PH, PW = Win::PW;
    const unsigned R = s.A / s.Q, rloc = threadIdx.x / s.Q;
    const unsigned n_rows = (unsigned)s.B * s.Ho * s.Wo, stride = gridDim.x * R;
    for (unsigned r = blockIdx.x * R + rloc; r < n_rows; r += 2 * stride) {
      const bool two = r + stride < n_rows;
      const unsigned r2 = two ? r + stride : r;
      V va[PH * PW], vb[PH * PW];
      window_load<PH, PW>(y, s, window_row<PH, PW>(s, r), q, va);
      window_load<PH, PW>(y, s, window_row<PH, PW>(s, r2), q, vb);
      const V da = dz[(size_t)r * s.Q + q];
      V db = dz[(size_t)r2 * s.Q + q];
      if (!two) db = vsplat<V>(0.f);
      int arg[kLanes<V>];
      V raw;
      V best = window_best<PH * PW>(va, scale, shift, arg, &raw);
#pragma unroll
      for (int e = 0; e < kLanes<V>; ++e) {
        const float d = best[e] > 0.f ? da[e] : 0.f;  // ReLU passes the gradient at the arg-max
        s1[e] += d;
        s2[e] = fmaf(d, (raw[e] - mu[e]) * is[e], s2[e]);
      }
      best = window_best<PH * PW>(vb, scale, shift, arg, &raw);
#pragma unroll
      for (int e = 0; e < kLanes<V>; ++e) {
        const float d = best[e] > 0.f ? db[e] : 0.f;
        s1[e] += d;
        s2[e] = fmaf(d, (raw[e] - mu[e]) * is[e], s2[e]);
      }
    }
  } else {
    const long long n_out = (long long)s.B * s.Ho * s.Wo * s.Q;
    const long long stride = (long long)gridDim.x * s.A;
    for (long long o = (long long)blockIdx.x * s.A + threadIdx.x; o < n_out; o += stride) {
      const PoolPos p = pool_pos(s, o / s.Q);
      int arg[kLanes<V>];
      V vraw;
      const V best = window_max(y, s, p.b, p.ho, p.wo, q, scale, shift, arg, &vraw);
      const V d = dz[o];
#pragma unroll
      for (int e = 0; e < kLanes<V>; ++e) {
        if (best[e] > 0.f) {                          // ReLU passes the gradient at the arg-max
          const float xh = (vraw[e] - mu[e]) * is[e];     // xhat at the arg-max
          s1[e] += d[e];
          s2[e] = fmaf(d[e], xh, s2[e]);
        }
      }
    }
  }
  float* p = partial + (size_t)blockIdx.x * 2 * s.C;
  quad_reduce_store(s1, s2, s.Q, s.A, lds, p, p + s.C);
}

__global__ __launch_bounds__(kFinCh * 16) void bn_bwd_finalize_kernel(
    const float* __restrict__ partial, int nblk, int C, double n_rows, float* __restrict__ dgamma,
    float* __restrict__ dbeta, float* __restrict__ coef, float* __restrict__ dzero) {
  __shared__ double lds[2][kFinCh][16];
  const int c = blockIdx.x * kFinCh + threadIdx.x % kFinCh, lane = threadIdx.x / kFinCh;
  double s1, s2;
  partial_sums(partial, nblk, C, c, lane, lds, &s1, &s2);
  if (c >= C || lane != 0) return;
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  if (dzero) dzero[c] = 0.f;               // the exact zero gradient of a constant the norm cancels
  coef[c] = (float)(s1 / n_rows);          // mean of dy
  coef[C + c] = (float)(s2 / n_rows);      // mean of dy * xhat
}

// Calls f(e) once for the vector index e of every position that no window covers (odd lengths):
// columns w >= Wo*pw of every row, then rows h >= Ho*ph of the covered columns.
template <typename F>
__device__ __forceinline__ void for_uncovered(const BnShape& s, int q, F f) {
  const long long stride = (long long)gridDim.x * s.A;
  const int wc = s.Wo * s.pw, hc = s.Ho * s.ph;
  const long long n_col = (long long)s.B * s.H * (s.W - wc) * s.Q;
  for (long long i = (long long)blockIdx.x * s.A + threadIdx.x; i < n_col; i += stride) {
    const long long r = i / s.Q;
    const int w = wc + (int)(r % (s.W - wc));
    const long long bh = r / (s.W - wc);                           // b * H + h
    f((bh * s.W + w) * s.Q + q);
  }
  const long long n_row = (long long)s.B * (s.H - hc) * wc * s.Q;
  for (long long i = (long long)blockIdx.x * s.A + threadIdx.x; i < n_row; i += stride) {
    const long long r = i / s.Q;
    const int w = (int)(r % wc);
    const long long t = r / wc;
    const int h = hc + (int)(t % (s.H - hc));
    const long long b = t / (s.H - hc);
    f(((b * s.H + h) * s.W + w) * s.Q + q);
  }
}

// The input gradient of one position, given dy = dz at the window's first maximum where the
// activation is positive and 0 everywhere else (positions that no window covers included).
//   kBatch (training): dx = gamma * invstd * (dy - mean(dy) - xhat * mean(dy * xhat)); c1 and c2
//     are the two means (bn_bwd_finalize_kernel).
//   running statistics (eval): they are constants, so dx = scale * dy, written as a select so that
//     every other position gets an exact +0 whatever the sign of gamma.
// dx_at: position idx of a window whose maximum `best` sits at arg; v = y there, d = the window's dz.
template <bool kBatch, typename V>
__device__ __forceinline__ V dx_at(const BnAffine<V>& a, V c1, V c2, V v, V best,
                                   const int (&arg)[kLanes<V>], int idx, V d) {
  V dy = vsplat<V>(0.f);
#pragma unroll
  for (int e = 0; e < kLanes<V>; ++e)
    if (best[e] > 0.f && arg[e] == idx) dy[e] = kBatch ? d[e] : a.scale[e] * d[e];
  if constexpr (kBatch) {
    const V xh = (v - a.mu) * a.is;
    return a.scale * (dy - c1 - xh * c2);
  } else {
    return dy;
  }
}

// a position that no window covers; v = y there
template <bool kBatch, typename V>
__device__ __forceinline__ V dx_uncovered(const BnAffine<V>& a, V c1, V c2, V v) {
  if constexpr (kBatch) {
    const V xh = (v - a.mu) * a.is;
    return a.scale * (-c1 - xh * c2);
  } else {
    return vsplat<V>(0.f);
  }
}

// One thread per (window, channel group): every y of the window is read once and every dx written
// once; the tail loops write the positions that no window covers.  No reduction here: in eval
// mode this kernel is the whole backward.
template <typename Win, typename Stats, typename V>
__global__ __launch_bounds__(kBnThreads) void bnrp_dx_kernel(const V* __restrict__ y,
                                                             const V* __restrict__ dz, Stats st,
                                                             const float* __restrict__ coef,
                                                             V* __restrict__ dx, BnShape s) {
  const int q = threadIdx.x % s.Q;
  constexpr bool kBatch = Stats::kBatch;
  const BnAffine<V> a = st.template affine<V>(q);
  const V scale = a.scale, shift = a.shift;
  V c1 = vsplat<V>(0.f), c2 = c1;
  if constexpr (kBatch) {
    c1 = vchan<V>(coef, q);
    c2 = vchan<V>(coef + s.C, q);
  }
  if constexpr (Win::kFixed) {
    constexpr int PH = Win::PH, PW = Win::PW;
    const unsigned R = s.A / s.Q, rloc = threadIdx.x / s.Q;
    const unsigned n_rows = (unsigned)s.B * s.Ho * s.Wo, stride = gridDim.x * R;
    auto emit = [&](const V (&v)[PH * PW], V d, unsigned row0) {
      int arg[kLanes<V>] = {};
      V raw;
      const V best = window_best<PH * PW>(v, scale, shift, arg, &raw);
#pragma unroll
      for (int i = 0; i < PH; ++i)
#pragma unroll
        for (int j = 0; j < PW; ++j)
          dx[(size_t)(row0 + (unsigned)i * (unsigned)s.W + (unsigned)j) * s.Q + q] =
              dx_at<kBatch>(a, c1, c2, v[i * PW + j], best, arg, i * PW + j, d);
    };
    for (unsigned r = blockIdx.x * R + rloc; r < n_rows; r += 2 * stride) {
      const bool two = r + stride < n_rows;
      const unsigned r2 = two ? r + stride : r;
      const unsigned rowa = window_row<PH, PW>(s, r), rowb = window_row<PH, PW>(s, r2);
      V va[PH * PW], vb[PH * PW];
      window_load<PH, PW>(y, s, rowa, q, va);
      window_load<PH, PW>(y, s, rowb, q, vb);
      const V da = dz[(size_t)r * s.Q + q], db = dz[(size_t)r2 * s.Q + q];
      emit(va, da, rowa);
      if (two) emit(vb, db, rowb);
    }
  } else {
    const long long stride = (long long)gridDim.x * s.A;
    const long long n_out = (long long)s.B * s.Ho * s.Wo * s.Q;
    for (long long o = (long long)blockIdx.x * s.A + threadIdx.x; o < n_out; o += stride) {
      const PoolPos p = pool_pos(s, o / s.Q);
      // pass 1 over the window: arg-max of relu(a) (first maximum)
      int arg[kLanes<V>] = {};
      const V best = window_max(y, s, p.b, p.ho, p.wo, q, scale, shift, arg);
      const V d = dz[o];
      // pass 2 (the window is in cache): dx for every position
      for (int i = 0; i < s.ph; ++i)
        for (int j = 0; j < s.pw; ++j) {
          const long long row = (p.b * s.H + (p.ho * s.ph + i)) * s.W + (p.wo * s.pw + j);
          dx[row * s.Q + q] = dx_at<kBatch>(a, c1, c2, y[row * s.Q + q], best, arg, i * s.pw + j, d);
        }
    }
  }
  for_uncovered(s, q, [&](long long e) { dx[e] = dx_uncovered<kBatch>(a, c1, c2, y[e]); });
}

// ------------------------------------------------------------------------------------ host
// Calls f with the window tag of the shape: the windows ResNet9 uses where every index fits 32
// bits, AnyWindow for every other shape.
template <typename F>
void with_window(const BnShape& s, F f) {
  const bool fits = (long long)s.B * s.H * s.W * s.Q < (1ll << 31);
  if (fits && s.ph == 1 && s.pw == 1) return f(FixedWindow<1, 1>{});
  if (fits && s.ph == 1 && s.pw == 2) return f(FixedWindow<1, 2>{});
  if (fits && s.ph == 2 && s.pw == 2) return f(FixedWindow<2, 2>{});
  f(AnyWindow{});
}

// Calls f with a value of the vector type a thread owns: float2 for C = 2, float4 otherwise.
template <typename F>
void with_vector(int C, F f) {
  if (C == 2) return f(f2{});
  f(f4{});
}

// Both: f(window tag, vector value), the two template arguments a launch needs.
template <typename F>
void with_window_and_vector(const BnShape& s, F f) {
  with_vector(s.C, [&](auto vec) { with_window(s, [&](auto win) { f(win, vec); }); });
}

inline int bn_blocks(long long n4) {
  long long b = (n4 + (long long)kBnThreads * 8 - 1) / ((long long)kBnThreads * 8);
  if (b < 1) b = 1;
  return (int)(b > kBnMaxBlocks ? kBnMaxBlocks : b);
}

// Vectors per row of a supported channel count, 0 for every other: C = 2 (one float2), or a
// multiple of 4 up to kBnMaxC (C / 4 float4).
inline int bn_width(int C) {
  if (C == 2) return 1;
  if (C <= 0 || (C & 3) || C > kBnMaxC) return 0;
  return C / 4;
}

inline bool bn_shape(BnShape* s, int B, int H, int W, int C, int ph, int pw) {
  const int Q = bn_width(C);
  if (B <= 0 || H <= 0 || W <= 0 || ph <= 0 || pw <= 0 || Q == 0) return false;
  *s = BnShape{B, H, W, C, ph, pw, H / ph, W / pw, Q, (kBnThreads / Q) * Q};
  return s->Ho > 0 && s->Wo > 0;
}

inline bool bn_aligned(int C, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & (C == 2 ? sizeof(f2) - 1 : sizeof(f4) - 1)) == 0;
}

// grid of the passes over the pooled rows (two per thread and iteration)
inline int pooled_blocks(const BnShape& s) {
  return bn_blocks((long long)s.B * s.Ho * s.Wo * s.Q * 2);
}

template <typename Stats>
void launch_fwd(const float* y, const Stats& stats, const float* skip, float* z, const BnShape& s,
                hipStream_t st) {
  with_window_and_vector(s, [&](auto win, auto vec) {
    using V = decltype(vec);
    hipLaunchKernelGGL((bnrp_fwd_kernel<decltype(win), Stats, V>), dim3(pooled_blocks(s)), dim3(s.A), 0, st,
                       reinterpret_cast<const V*>(y), stats, reinterpret_cast<const V*>(skip),
                       reinterpret_cast<V*>(z), s);
  });
}

template <typename Stats>
void launch_dx(const float* y, const float* dz, const Stats& stats, const float* coef, float* dx,
               const BnShape& s, hipStream_t st) {
  with_window_and_vector(s, [&](auto win, auto vec) {
    using V = decltype(vec);
    hipLaunchKernelGGL((bnrp_dx_kernel<decltype(win), Stats, V>), dim3(pooled_blocks(s)), dim3(s.A), 0, st,
                       reinterpret_cast<const V*>(y), reinterpret_cast<const V*>(dz), stats, coef,
                       reinterpret_cast<V*>(dx), s);
  });
}

}  // namespace pcgmix

extern "C" int pcgmix_bnrp_supported(int C) { return pcgmix::bn_width(C) != 0; }

extern "C" long long pcgmix_bnrp_workspace_floats(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return (long long)pcgmix::kBnMaxBlocks * 2 * C + 2 * C;
}

extern "C" int pcgmix_bnrp_fwd_f32(const float* y, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, float momentum,
                                   float eps, const float* mean_shift, long long* batches_tracked,
                                   const float* skip, float* z, float* mean, float* invstd,
                                   float* workspace, int B, int H, int W, int C, int ph, int pw,
                                   pcgmix_stream_t stream) {
  using namespace pcgmix;
  BnShape s;
  if (!y || !gamma || !beta || !z || !mean || !invstd || !workspace || !bn_shape(&s, B, H, W, C, ph, pw))
    return hipErrorInvalidValue;
  if (!bn_aligned(C, {y, z, skip, gamma, beta, mean, invstd, workspace})) return hipErrorInvalidValue;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long long rows = (long long)B * H * W, n4 = rows * s.Q;
  const int nblk = bn_blocks(n4);
  with_vector(C, [&](auto vec) {
    using V = decltype(vec);
    hipLaunchKernelGGL(bn_stats_kernel<V>, dim3(nblk), dim3(s.A), 0, st, reinterpret_cast<const V*>(y), n4, s.Q, s.A,
                       workspace, C);
  });
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(kFinCh * 16), 0, st, workspace, y, nblk, C,
                     (double)rows, eps, momentum, mean, invstd, running_mean, running_var, mean_shift,
                     batches_tracked);
  launch_fwd(y, TrainStats{gamma, beta, mean, invstd}, skip, z, s, st);
  return (int)hipGetLastError();
}

extern "C" int pcgmix_bnrp_bwd_f32(const float* y, const float* dz, const float* gamma,
                                   const float* beta, const float* mean, const float* invstd,
                                   float* dx, float* dgamma, float* dbeta, float* dzero,
                                   float* workspace, int B, int H, int W, int C, int ph, int pw,
                                   pcgmix_stream_t stream) {
  using namespace pcgmix;
  BnShape s;
  if (!y || !dz || !gamma || !beta || !mean || !invstd || !dx || !dgamma || !dbeta || !workspace ||
      !bn_shape(&s, B, H, W, C, ph, pw))
    return hipErrorInvalidValue;
  if (!bn_aligned(C, {y, dz, dx, workspace, gamma, beta, mean, invstd})) return hipErrorInvalidValue;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const TrainStats stats{gamma, beta, mean, invstd};
  const int nblk = pooled_blocks(s);
  float* coef = workspace + (size_t)kBnMaxBlocks * 2 * C;
  with_window_and_vector(s, [&](auto win, auto vec) {
    using V = decltype(vec);
    hipLaunchKernelGGL((bnrp_bwd_reduce_kernel<decltype(win), V>), dim3(nblk), dim3(s.A), 0, st,
                       reinterpret_cast<const V*>(y), reinterpret_cast<const V*>(dz), stats, workspace, s);
  });
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + kFinCh - 1) / kFinCh), dim3(kFinCh * 16), 0, st, workspace, nblk,
                     C, (double)((long long)B * H * W), dgamma, dbeta, coef, dzero);
  launch_dx(y, dz, stats, coef, dx, s, st);
  return (int)hipGetLastError();
}

extern "C" int pcgmix_bnrp_eval_fwd_f32(const float* y, const float* gamma, const float* beta,
                                        const float* running_mean, const float* running_var,
                                        float eps, const float* conv_bias, const float* skip,
                                        float* z, int B, int H, int W, int C, int ph, int pw,
                                        pcgmix_stream_t stream) {
  using namespace pcgmix;
  BnShape s;
  if (!y || !gamma || !beta || !running_mean || !running_var || !z || !bn_shape(&s, B, H, W, C, ph, pw))
    return hipErrorInvalidValue;
  if (!bn_aligned(C, {y, z, skip, gamma, beta, running_mean, running_var, conv_bias}))
    return hipErrorInvalidValue;
  launch_fwd(y, EvalStats{gamma, beta, running_mean, running_var, conv_bias, eps}, skip, z, s,
             reinterpret_cast<hipStream_t>(stream));
  return (int)hipGetLastError();
}

extern "C" int pcgmix_bnrp_eval_bwd_f32(const float* y, const float* dz, const float* gamma,
                                        const float* beta, const float* running_mean,
                                        const float* running_var, float eps, const float* conv_bias,
                                        float* dx, int B, int H, int W, int C, int ph, int pw,
                                        pcgmix_stream_t stream) {
  using namespace pcgmix;
  BnShape s;
  if (!y || !dz || !gamma || !beta || !running_mean || !running_var || !dx ||
      !bn_shape(&s, B, H, W, C, ph, pw))
    return hipErrorInvalidValue;
  if (!bn_aligned(C, {y, dz, dx, gamma, beta, running_mean, running_var, conv_bias}))
    return hipErrorInvalidValue;
  launch_dx(y, dz, EvalStats{gamma, beta, running_mean, running_var, conv_bias, eps}, nullptr, dx, s,
            reinterpret_cast<hipStream_t>(stream));
  return (int)hipGetLastError();
}
