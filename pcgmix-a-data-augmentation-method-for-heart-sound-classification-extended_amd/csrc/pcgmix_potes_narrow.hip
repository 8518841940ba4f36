// pcgmix_potes_narrow.hip — the conv branch of the NARROW Potes models as fused kernels (gfx950).
//
// Reference: models.py:352-356 (CNN_potes_tenpercent_TS layers [2,1], CNN_potes_twopercent_TS
// layers [1,1]) over models.py:359-381 (conv_block_1d, CNN_potes.cnn1): per band row
//     Conv1d(1->C1, k5, pad1) + ReLU + MaxPool(2)  ->  Conv1d(C1->C2, k5, pad1) + ReLU + MaxPool(2)
// with (C1,C2) in {(1,1), (2,1)}.  pcgmix_potes.hip is built around 8 and 4 channels (MFMA 4x4x1
// tiling, 212 gradient columns); at one or two channels there is nothing for a matrix core to do
// and the stack is a pure bandwidth / latency problem: at N = 1024 rows of T = 2500 about 10 MB in
// and 2.5 MB out, a few hundred multiply-adds per output.  Plain VALU code, one thread per pooled
// output:
//
//   narrow_fwd_kernel         a block stages 4*kNarTP + 16 inputs of one row in LDS with coalesced
//                             (16-byte where the row allows) loads; every thread reads its
//                             20-float window from there (five ds_read_b128, consecutive lanes
//                             16 bytes apart: no bank conflict), computes the six first-layer
//                             values its pooled output needs in registers — neighbouring threads
//                             recompute each other's, cheaper than a second LDS round trip and a
//                             second barrier — and writes h2, and on request the routing m2 / s1.
//   narrow_bwd_kernel         weight gradients: the same window and recompute; a thread owns
//                             pooled output p for the second layer's gradients and first-layer
//                             positions 2p, 2p+1 for the first layer's; persistent blocks keep the
//                             grad_len sums in registers and write one partial row each;
//                             narrow_reduce_kernel sums the rows in a fixed order (no atomics).
//   narrow_input_grad_kernel  dL/dx from dL/dh2, m2, s1 and the weights alone; a thread owns four
//                             consecutive inputs.
// Arithmetic: float32, every conv output an in-order fmaf chain from the bias over (input channel,
// tap); ReLU / max-pool routing by relu_pool2 (pcgmix_potes_stack.h: first maximum wins).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcgmix_kernels.h"
#include "pcgmix_potes_stack.h"

namespace pcgmix {
namespace narrow {

constexpr int kK = 5;
constexpr int kThreads = 256;
constexpr int kNarTP = 256;                 // pooled outputs per tile: one per thread
constexpr int kNarXN = 4 * kNarTP + 16;     // staged inputs x[4 p0 - 4 .. 4 p0 + 4 kNarTP + 12)
constexpr int kInTU = 4 * kThreads;         // inputs per block of the input gradient
constexpr int kMaxN = 65535;                // rows: grid.y

// without s1 (inference, weight gradient only) only the outputs p < P2 matter
// with it the forward walks further: even p up to 2*(P1/4) each write one byte of s1 (byte p/2 holds
// first-layer positions 2p-1 .. 2p+2), and 2*(P1/4) >= P2
__host__ __device__ inline int fwd_tiles(const PotesDims& d, bool with_s1) {
  return ((with_s1 ? 2 * d.s1row() - 1 : d.P2) + kNarTP - 1) / kNarTP;
}
// the weight gradient owns first-layer positions q = 2p, 2p+1 < P1 and outputs p < P2 <= P1/2
__host__ __device__ inline int bwd_tiles(const PotesDims& d) {
  return ((d.P1 + 1) / 2 + kNarTP - 1) / kNarTP;
}

template <int C1, int C2>
struct Weights {
  float w1[C1 * kK], b1[C1], w2[C2 * C1 * kK], b2[C2];
};
// wave-uniform addresses: the compiler keeps these in scalar registers
template <int C1, int C2>
__device__ __forceinline__ void load_weights(Weights<C1, C2>& W, const float* __restrict__ w1,
                                             const float* __restrict__ b1,
                                             const float* __restrict__ w2,
                                             const float* __restrict__ b2) {
#pragma unroll
  for (int i = 0; i < C1 * kK; ++i) W.w1[i] = w1[i];
#pragma unroll
  for (int i = 0; i < C1; ++i) W.b1[i] = b1 ? b1[i] : 0.f;
#pragma unroll
  for (int i = 0; i < C2 * C1 * kK; ++i) W.w2[i] = w2[i];
#pragma unroll
  for (int i = 0; i < C2; ++i) W.b2[i] = b2 ? b2[i] : 0.f;
}

// xs[u] = x[4 p0 - 4 + u], u < kNarXN, zero outside [0, T).  fast: T % 4 == 0 and x 16-byte aligned,
// so every aligned group of four is wholly inside or wholly outside the row.
__device__ __forceinline__ void stage_tile(float* xs, const float* __restrict__ xrow, int p0, int T,
                                           bool fast) {
  const int g0 = 4 * p0 - 4;
  if (fast) {
    for (int v = threadIdx.x; v < kNarXN / 4; v += kThreads) {
      const int g = g0 + 4 * v;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g >= 0 && g < T) val = *reinterpret_cast<const float4*>(xrow + g);
      *reinterpret_cast<float4*>(xs + 4 * v) = val;
    }
  } else {
    for (int u = threadIdx.x; u < kNarXN; u += kThreads) {
      const int g = g0 + u;
      xs[u] = (g >= 0 && g < T) ? xrow[g] : 0.f;
    }
  }
}

__device__ __forceinline__ void load_window(const float* xs, float (&xw)[20]) {
  const float4* p = reinterpret_cast<const float4*>(xs + 4 * threadIdx.x);
#pragma unroll
  for (int v = 0; v < 5; ++v) {
    const float4 a = p[v];
    xw[4 * v] = a.x; xw[4 * v + 1] = a.y; xw[4 * v + 2] = a.z; xw[4 * v + 3] = a.w;
  }
}

// First layer around pooled output p from the window xw[e] = x[4p - 4 + e]: a1[c][r] and its
// selector for positions q = 2p - 1 + r, r < 6 (zero outside [0, P1): conv2's padding).  Conv output
// i = 2q + h = 4p - 2 + m (m = 2r + h) reads x[i - 1 + k] = xw[1 + m + k].
template <int C1>
__device__ __forceinline__ void layer1(const float* w1, const float* b1, const float (&xw)[20], int p,
                                       int P1, float (&a1)[C1][6], uint32_t (&sel)[C1][6]) {
#pragma unroll
  for (int c = 0; c < C1; ++c)
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      float z[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float acc = b1[c];
#pragma unroll
        for (int k = 0; k < kK; ++k) acc = fmaf(w1[c * kK + k], xw[1 + 2 * r + h + k], acc);
        z[h] = acc;
      }
      const int q = 2 * p - 1 + r;
      relu_pool2(z[0], z[1], q >= 0 && q < P1, a1[c][r], sel[c][r]);
    }
}

// Second-layer conv output j = 2p + e of channel co: a1 position j - 1 + k = 2p - 1 + (e + k).
template <int C1>
__device__ __forceinline__ float conv2_at(const float* w2co, float bias, const float (&a1)[C1][6],
                                          int e) {
  float acc = bias;
#pragma unroll
  for (int ci = 0; ci < C1; ++ci)
#pragma unroll
    for (int k = 0; k < kK; ++k) acc = fmaf(w2co[ci * kK + k], a1[ci][e + k], acc);
  return acc;
}

// ---------------------------------------------------------------------------------- forward
// grid (tiles, N).  m2, s1, rnd: each written where non-null (all null: the inference forward).
template <int C1, int C2>
__global__ __launch_bounds__(kThreads) void narrow_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ h2,
    uint8_t* __restrict__ m2, uint8_t* __restrict__ s1, int T, uint4* __restrict__ rnd,
    long long rnd_n16, const uint32_t* __restrict__ key, uint32_t key_lo, uint32_t key_hi) {
  if (rnd)
    counter_hash_fill(rnd, rnd_n16, key, key_lo, key_hi,
                      ((long long)blockIdx.y * gridDim.x + blockIdx.x) * kThreads + threadIdx.x,
                      (long long)gridDim.x * gridDim.y * kThreads);
  __shared__ __align__(16) float xs[kNarXN];
  const PotesDims d = potes_dims(T);
  const int s1row = d.s1row(), m2row = d.m2row();
  const int n = blockIdx.y, p0 = blockIdx.x * kNarTP, p = p0 + (int)threadIdx.x;
  const float* xrow = x + (size_t)n * T;
  const bool fast = !(T & 3) && !(reinterpret_cast<uintptr_t>(x) & 15);
  Weights<C1, C2> W;
  load_weights(W, w1, b1, w2, b2);
  stage_tile(xs, xrow, p0, T, fast);
  __syncthreads();
  float xw[20];
  load_window(xs, xw);
  float a1[C1][6];
  uint32_t sel[C1][6];
  layer1<C1>(W.w1, W.b1, xw, p, d.P1, a1, sel);
  if (s1 && !(p & 1) && (p >> 1) < s1row) {
    // position q in bits 2*((q+1)&3) of byte (q+1)>>2: q + 1 = 2p + r, p even: r < 4 is byte p/2
#pragma unroll
    for (int c = 0; c < C1; ++c)
      s1[((size_t)n * C1 + c) * s1row + (p >> 1)] =
          (uint8_t)(sel[c][0] | (sel[c][1] << 2) | (sel[c][2] << 4) | (sel[c][3] << 6));
  }
  const bool own = p < d.P2;
#pragma unroll
  for (int co = 0; co < C2; ++co) {
    const float za = conv2_at<C1>(W.w2 + co * C1 * kK, W.b2[co], a1, 0);
    const float zb = conv2_at<C1>(W.w2 + co * C1 * kK, W.b2[co], a1, 1);
    float o;
    uint32_t code;
    relu_pool2(za, zb, own, o, code);
    if (own) h2[((size_t)n * C2 + co) * d.P2 + p] = o;
    if (m2) {
      // four outputs per byte, output p in bits 2*(p&3): p0 % 4 == 0, so a quad of lanes is a byte
      uint32_t b = code << (2 * (threadIdx.x & 3));
      b |= __shfl_xor(b, 1);
      b |= __shfl_xor(b, 2);
      if (own && !(threadIdx.x & 3)) m2[((size_t)n * C2 + co) * m2row + (p >> 2)] = (uint8_t)b;
    }
  }
}

// ---------------------------------------------------------------------------------- routing reads
// dL/d(conv2 output j) of channel co of row n: the pooled output j>>1 hands its gradient to the
// conv output its m2 code names.
template <int C2>
struct Routed {
  const float* g;       // grad_h2 + n*C2*P2
  const uint8_t* m;     // m2 + n*C2*m2row
  int P2, m2row;
  __device__ __forceinline__ void at(int co, int p, float& gv, uint32_t& code) const {
    gv = 0.f;
    code = 0u;
    if (p >= 0 && p < P2) {
      gv = g[(size_t)co * P2 + p];
      code = route2(m + (size_t)co * m2row, p);
    }
  }
};

// ---------------------------------------------------------------------------------- weight gradient
template <int C1, int C2>
constexpr int grad_len() { return kK * C1 + C1 + kK * C1 * C2 + C2; }

// Sum over the block in a fixed order: lanes by xor-shuffles, the four waves in order.
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if (!(threadIdx.x & 63)) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (G): block g takes items g, g + G, ... of the N * bwd_tiles (row, tile) pairs and writes
// partial[g][0 .. grad_len) = [gw1 | gb1 | gw2 | gb2] of its items.
template <int C1, int C2>
__global__ __launch_bounds__(kThreads) void narrow_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ grad_h2, const uint8_t* __restrict__ m2,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, float* __restrict__ partial, int N, int T) {
  constexpr int kGW1 = 0, kGB1 = kK * C1, kGW2 = kGB1 + C1, kGB2 = kGW2 + kK * C1 * C2;
  constexpr int kLen = grad_len<C1, C2>();
  __shared__ __align__(16) float xs[kNarXN];
  __shared__ float red[4];
  const PotesDims d = potes_dims(T);
  const int m2row = d.m2row();
  const int tiles = bwd_tiles(d), items = N * tiles;
  const bool fast = !(T & 3) && !(reinterpret_cast<uintptr_t>(x) & 15);
  Weights<C1, C2> W;
  load_weights(W, w1, b1, w2, b2);
  float acc[kLen];
#pragma unroll
  for (int e = 0; e < kLen; ++e) acc[e] = 0.f;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int n = item / tiles, p0 = (item - n * tiles) * kNarTP, p = p0 + (int)threadIdx.x;
    __syncthreads();                               // the previous item's window reads are done
    stage_tile(xs, x + (size_t)n * T, p0, T, fast);
    __syncthreads();
    float xw[20];
    load_window(xs, xw);
    float a1[C1][6];
    uint32_t sel[C1][6];
    layer1<C1>(W.w1, W.b1, xw, p, d.P1, a1, sel);
    const Routed<C2> R = {grad_h2 + (size_t)n * C2 * d.P2, m2 + (size_t)n * C2 * m2row, d.P2, m2row};
    // gradients of the conv2 outputs j = 2p - 4 + jj, jj < 8 (pooled outputs p-2 .. p+1)
    float gz2[C2][8];
#pragma unroll
    for (int co = 0; co < C2; ++co)
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) {
        float gv;
        uint32_t code;
        R.at(co, p - 2 + pp, gv, code);
        gz2[co][2 * pp] = code == 1u ? gv : 0.f;
        gz2[co][2 * pp + 1] = code == 2u ? gv : 0.f;
      }
    // second layer, owned output p: conv output j = 2p + e reads a1 position 2p - 1 + (e + k)
#pragma unroll
    for (int co = 0; co < C2; ++co)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float gv = gz2[co][4 + e];
        acc[kGB2 + co] += gv;
#pragma unroll
        for (int ci = 0; ci < C1; ++ci)
#pragma unroll
          for (int k = 0; k < kK; ++k) acc[kGW2 + (co * C1 + ci) * kK + k] += gv * a1[ci][e + k];
      }
    // first layer, owned positions q = 2p + t (r = 1 + t): dL/da1[c][q] = sum over (co, k) of
    // w2[co][c][k] * gz2[co][j = q + 1 - k], j - (2p - 4) = t + 5 - k; routed by the selector to conv
    // output i = 2q + (sel - 1) = 4p - 2 + m, m = 2r + sel - 1, which read x[i - 1 + k] = xw[1 + m + k]
#pragma unroll
    for (int c = 0; c < C1; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float ga = 0.f;
#pragma unroll
        for (int co = 0; co < C2; ++co)
#pragma unroll
          for (int k = 0; k < kK; ++k) ga = fmaf(W.w2[(co * C1 + c) * kK + k], gz2[co][t + 5 - k], ga);
        const uint32_t s = sel[c][1 + t];            // 0 outside [0, P1) as well
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float gz = s == (uint32_t)(1 + h) ? ga : 0.f;
          acc[kGB1 + c] += gz;
#pragma unroll
          for (int k = 0; k < kK; ++k) acc[kGW1 + c * kK + k] += gz * xw[1 + 2 * (1 + t) + h + k];
        }
      }
  }
#pragma unroll
  for (int e = 0; e < kLen; ++e) {
    const float v = block_sum(acc[e], red);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.x * kLen + e] = v;
  }
}

// grid (grad_len): column e of partial (G, len), rows in a fixed order.
__global__ __launch_bounds__(kThreads) void narrow_reduce_kernel(const float* __restrict__ partial,
                                                                 float* __restrict__ grads, int G,
                                                                 int len) {
  __shared__ float red[4];
  float v = 0.f;
  for (int g = threadIdx.x; g < G; g += kThreads) v += partial[(size_t)g * len + blockIdx.x];
  v = block_sum(v, red);
  if (threadIdx.x == 0) grads[blockIdx.x] = v;
}

// ---------------------------------------------------------------------------------- input gradient
// grid (ceil(T / kInTU), N).  Thread u of the row owns inputs t = 4u + tt, tt < 4:
//   dx[t]      = sum over (c, k) of w1[c][k] * gz1[c][i = t + 1 - k]            i - (4u - 4) = tt + 5 - k
//   gz1[c][i]  = ga1[c][q = i >> 1] where s1 names conv output i, else 0         q - (2u - 2) = ii >> 1
//   ga1[c][q]  = sum over (co, k) of w2[co][c][k] * gz2[co][j = q + 1 - k]        j - (2u - 6) = qq + 5 - k
// so five first-layer positions q = 2u-2 .. 2u+2 and five pooled outputs p = u-3 .. u+1.
template <int C1, int C2>
__global__ __launch_bounds__(kThreads) void narrow_input_grad_kernel(
    const float* __restrict__ grad_h2, const uint8_t* __restrict__ m2, const uint8_t* __restrict__ s1,
    const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ grad_x, int T) {
  const PotesDims d = potes_dims(T);
  const int s1row = d.s1row(), m2row = d.m2row();
  const int n = blockIdx.y, u = blockIdx.x * kThreads + (int)threadIdx.x;
  if (4 * u >= T) return;
  Weights<C1, C2> W;
  load_weights<C1, C2>(W, w1, nullptr, w2, nullptr);
  const Routed<C2> R = {grad_h2 + (size_t)n * C2 * d.P2, m2 + (size_t)n * C2 * m2row, d.P2, m2row};
  float gz2[C2][10];
#pragma unroll
  for (int co = 0; co < C2; ++co)
#pragma unroll
    for (int pp = 0; pp < 5; ++pp) {
      float gv;
      uint32_t code;
      R.at(co, u - 3 + pp, gv, code);
      gz2[co][2 * pp] = code == 1u ? gv : 0.f;
      gz2[co][2 * pp + 1] = code == 2u ? gv : 0.f;
    }
  float dx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < C1; ++c) {
    const uint8_t* srow = s1 + ((size_t)n * C1 + c) * s1row;
    float gz1[10];
#pragma unroll
    for (int qq = 0; qq < 5; ++qq) {
      const int q = 2 * u - 2 + qq;
      uint32_t s = 0u;
      if (q >= 0 && q < d.P1) s = route2(srow, q + 1);
      float ga = 0.f;
#pragma unroll
      for (int co = 0; co < C2; ++co)
#pragma unroll
        for (int k = 0; k < kK; ++k) ga = fmaf(W.w2[(co * C1 + c) * kK + k], gz2[co][qq + 5 - k], ga);
      gz1[2 * qq] = s == 1u ? ga : 0.f;
      gz1[2 * qq + 1] = s == 2u ? ga : 0.f;
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int k = 0; k < kK; ++k) dx[tt] = fmaf(W.w1[c * kK + k], gz1[tt + 5 - k], dx[tt]);
  }
  float* out = grad_x + (size_t)n * T + 4 * u;
  if (!(T & 3) && !(reinterpret_cast<uintptr_t>(grad_x) & 15)) {
    *reinterpret_cast<float4*>(out) = make_float4(dx[0], dx[1], dx[2], dx[3]);
  } else {
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
      if (4 * u + tt < T) out[tt] = dx[tt];
  }
}

inline bool supported(int C1, int C2) { return C2 == 1 && (C1 == 1 || C1 == 2); }
inline int grad_len_of(int C1, int C2) { return kK * C1 + C1 + kK * C1 * C2 + C2; }

}  // namespace narrow
}  // namespace pcgmix

using namespace pcgmix;
using namespace pcgmix::narrow;

extern "C" int pcgmix_potes_narrow_supported(int C1, int C2) { return supported(C1, C2) ? 1 : 0; }

extern "C" int pcgmix_potes_narrow_grad_len(int C1, int C2) {
  return supported(C1, C2) ? grad_len_of(C1, C2) : 0;
}

extern "C" int pcgmix_potes_narrow_bwd_blocks(int N, int T, int C1, int C2) {
  if (!supported(C1, C2) || N <= 0 || N > kMaxN || T < 14) return 0;
  // persistent blocks, four per CU: each ends with grad_len block-wide sums, so few and long
  const long long work = (long long)N * bwd_tiles(potes_dims(T));
  return (int)(work < 1024 ? work : 1024);
}

extern "C" long long pcgmix_potes_narrow_mask_bytes(int N, int T, int C1, int C2, int layer) {
  if (!supported(C1, C2) || N <= 0 || N > kMaxN || T < 14) return 0;
  const PotesDims d = potes_dims(T);
  return layer == 2 ? (long long)N * C2 * d.m2row() : (layer == 1 ? (long long)N * C1 * d.s1row() : 0);
}

extern "C" int pcgmix_potes_narrow_fwd_f32(const float* x, const float* w1, const float* b1,
                                           const float* w2, const float* b2, float* h2, uint8_t* m2,
                                           uint8_t* s1, int N, int T, int C1, int C2,
                                           uint8_t* rnd_out, long long rnd_bytes,
                                           const uint32_t* key_dev, uint64_t key,
                                           pcgmix_stream_t stream) {
  if (!supported(C1, C2) || !x || !w1 || !b1 || !w2 || !b2 || !h2 || N < 0 || N > kMaxN || T < 14)
    return hipErrorInvalidValue;
  if (!pcgmix::dropout_fill_args_ok(rnd_out, rnd_bytes, N)) return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  const dim3 grid((unsigned)fwd_tiles(potes_dims(T), s1 != nullptr), (unsigned)N), block(kThreads);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint4* rnd = reinterpret_cast<uint4*>(rnd_out);
  const long long n16 = rnd_out ? rnd_bytes / 16 : 0ll;
  const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
  if (C1 == 1)
    hipLaunchKernelGGL((narrow_fwd_kernel<1, 1>), grid, block, 0, s, x, w1, b1, w2, b2, h2, m2, s1, T,
                       rnd, n16, key_dev, klo, khi);
  else
    hipLaunchKernelGGL((narrow_fwd_kernel<2, 1>), grid, block, 0, s, x, w1, b1, w2, b2, h2, m2, s1, T,
                       rnd, n16, key_dev, klo, khi);
  return (int)hipGetLastError();
}

extern "C" int pcgmix_potes_narrow_bwd_mask_f32(const float* x, const float* grad_h2,
                                                const uint8_t* m2, const float* w1, const float* b1,
                                                const float* w2, const float* b2, float* partial,
                                                float* grads, int N, int T, int C1, int C2,
                                                pcgmix_stream_t stream) {
  if (!supported(C1, C2) || !x || !grad_h2 || !m2 || !w1 || !b1 || !w2 || !b2 || !partial || !grads ||
      N < 0 || N > kMaxN || T < 14)
    return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  const int G = pcgmix_potes_narrow_bwd_blocks(N, T, C1, C2), len = grad_len_of(C1, C2);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (C1 == 1)
    hipLaunchKernelGGL((narrow_bwd_kernel<1, 1>), dim3((unsigned)G), dim3(kThreads), 0, s, x, grad_h2,
                       m2, w1, b1, w2, b2, partial, N, T);
  else
    hipLaunchKernelGGL((narrow_bwd_kernel<2, 1>), dim3((unsigned)G), dim3(kThreads), 0, s, x, grad_h2,
                       m2, w1, b1, w2, b2, partial, N, T);
  hipLaunchKernelGGL(narrow_reduce_kernel, dim3((unsigned)len), dim3(kThreads), 0, s, partial, grads,
                     G, len);
  return (int)hipGetLastError();
}

extern "C" int pcgmix_potes_narrow_input_grad_mask_f32(const float* grad_h2, const uint8_t* m2,
                                                       const uint8_t* s1, const float* w1,
                                                       const float* w2, float* grad_x, int N, int T,
                                                       int C1, int C2, pcgmix_stream_t stream) {
  if (!supported(C1, C2) || !grad_h2 || !m2 || !s1 || !w1 || !w2 || !grad_x || N < 0 || N > kMaxN ||
      T < 14)
    return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  const dim3 grid((unsigned)((T + kInTU - 1) / kInTU), (unsigned)N), block(kThreads);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (C1 == 1)
    hipLaunchKernelGGL((narrow_input_grad_kernel<1, 1>), grid, block, 0, s, grad_h2, m2, s1, w1, w2,
                       grad_x, T);
  else
    hipLaunchKernelGGL((narrow_input_grad_kernel<2, 1>), grid, block, 0, s, grad_h2, m2, s1, w1, w2,
                       grad_x, T);
  return (int)hipGetLastError();
}
