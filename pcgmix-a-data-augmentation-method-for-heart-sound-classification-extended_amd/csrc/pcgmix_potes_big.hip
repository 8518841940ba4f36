// pcgmix_potes_big.hip — the conv branch of the BIG Potes models on the f32 matrix instruction
// (gfx950).
//
// Reference: models.py:339-343 (CNN_potes_big64and32_TS layers [64,32], CNN_potes_big128and64_TS
// layers [128,64]) over models.py:359-381 (conv_block_1d, CNN_potes.cnn1): per band row
//     Conv1d(1->C1, k5, pad1) + ReLU + MaxPool(2)  ->  Conv1d(C1->C2, k5, pad1) + ReLU + MaxPool(2)
// with (C1,C2) in {(64,32), (128,64)}.  At these widths the second layer is a real GEMM per row
// (K = 5*C1 = 320 / 640) and runs on v_mfma_f32_32x32x2_f32, whose result is bit for bit a k-ordered
// fmaf chain; the first layer (5 multiply-adds per output) stays on the VALU and never leaves LDS.
// Geometry, relu_pool2 and the m2 / s1 byte encodings are pcgmix_potes_stack.h's.
//
//   big_fwd_kernel     grid (tiles, N).  A tile is kTM = 128 second-layer conv positions of one row
//                      (64 pooled outputs).  Layer 1 writes a1[c][q], q = m0-1 .. m0+130, into LDS
//                      (and the s1 bytes 32*tile .. 32*tile+31 on request); layer 2 is the implicit
//                      GEMM A[m][(c,tap)] = a1[c][m+tap-1], B[(c,tap)][n] = w2[n][c][tap], positions
//                      on the M axis: wave w owns positions 32w .. 32w+31 and all C2 channels, its
//                      accumulators seeded with b2.  A lane of the 32x32 accumulator holds four
//                      consecutive positions of one channel, i.e. both candidates of two pooled
//                      pairs: relu_pool2 in registers.  w2 streams through LDS in groups of kCG = 8
//                      input channels (register prefetch of the next group).  h2 and m2 leave through
//                      an LDS image of the tile, whole rows at a time.
//   big_gw2_kernel     persistent.  a1 recomputed as above, dz2[n][m] routed from grad_h2 by m2 into
//                      LDS; gw2[n][(c,tap)] += sum_m dz2[n][m] a1[c][m+tap-1] is the GEMM M = C2,
//                      N = 5*C1, K = the tile's 128 positions, its accumulators live in registers for
//                      the whole launch (wave w owns column tiles w, w+4, ..).  gb2 on the side.
//   big_da1_kernel     ONE template for the transposed second layer, dA1[q][c] = sum over (n,tap) of
//                      dz2[n][q+1-tap] w2[n][c][tap]: GEMM M = 128 positions, N = C1, K = 5*C2, w2
//                      streamed in groups of 8 output channels.  kGw1: persistent, routes dA1 by the
//                      first layer's decisions recomputed from x (relu_pool2) into gw1 / gb1
//                      registers.  kDx: grid (tiles, N), routes by s1, reduces over the channels in
//                      LDS and applies the transposed 5-tap conv with w1: 250 inputs per tile.
//   big_reduce_kernel  partial (G, grad_len) -> grads, rows in a fixed order.  No atomics anywhere.
//
// LDS per block ([64,32] / [128,64]): forward 39 / 77 KB, gw2 50 / 99 KB, dA1 28 / 55 KB (kGw1),
// 34 / 69 KB (kDx).  DESIGN.md 3.5c has the register budget, the rooflines and the measured rates.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "pcgmix_kernels.h"
#include "pcgmix_potes_stack.h"

namespace pcgmix {
namespace big {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kK = 5;
constexpr int kThreads = 256;
constexpr int kTM = 128;                  // positions per tile (M of the forward / dA1 GEMMs)
constexpr int kLD = kTM + 4;              // a1 tile row: local i <-> q = m0 - 1 + i  (132 = 4 mod 32)
constexpr int kXN = 272;                  // staged inputs (268 / 261 used)
constexpr int kCG = 8;                    // channels per streamed group of w2
constexpr int kLDZ = kTM + 1;             // dz2 tile row of the gw2 GEMM
constexpr int kLDQ = kTM + 7;             // dz2 tile row of the dA1 GEMM: 134 used, odd
constexpr int kLDR = kTM + 1;             // dA1 tile row of the input gradient
constexpr int kInTT = 250;                // inputs per tile of the input gradient
constexpr int kMaxN = 65535;              // rows: grid.y

__host__ __device__ inline int fwd_tiles(const PotesDims& d, bool with_s1) {
  const int a = (d.P2 + 63) / 64, b = with_s1 ? (d.s1row() + 31) / 32 : 0;
  return a > b ? a : b;
}
__host__ __device__ inline int gw2_tiles(const PotesDims& d) { return (d.P2 + 63) / 64; }
__host__ __device__ inline int gw1_tiles(const PotesDims& d) { return (d.P1 + kTM - 1) / kTM; }
__host__ __device__ inline int in_tiles(int T) { return (T + kInTT - 1) / kInTT; }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// accumulator register r of lane (j, h): row (r&3) + 8*(r>>2) + 4*h, column j
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// xs[u] = x[g0 + u], u < n, zero outside [0, T)
__device__ __forceinline__ void stage_x(float* xs, const float* __restrict__ xrow, int g0, int n, int T) {
  for (int u = threadIdx.x; u < n; u += kThreads) {
    const int g = g0 + u;
    xs[u] = (g >= 0 && g < T) ? xrow[g] : 0.f;
  }
}

// First-layer pre-activations of position q (conv outputs 2q, 2q+1) from xw[k] = x[2q - 1 + k]
__device__ __forceinline__ void conv1_pair(const float (&w)[kK], float b, const float* xw, float& z0,
                                           float& z1) {
  z0 = b;
  z1 = b;
#pragma unroll
  for (int k = 0; k < kK; ++k) {
    z0 = fmaf(w[k], xw[k], z0);
    z1 = fmaf(w[k], xw[k + 1], z1);
  }
}

// a1s[c][i] = a1[c][q = m0 - 1 + i], i < 132, from xs[u] = x[2 m0 - 3 + u]; zero outside [0, P1)
// (conv2's padding).  A thread keeps its channel (256 % C1 == 0) and walks quads of positions; quad
// g < 32 is byte m0/4 + g of the s1 row (srow: this row's, nullptr: not wanted).
template <int C1>
__device__ __forceinline__ void layer1_tile(const float* xs, float* a1s, const float* __restrict__ w1,
                                            const float* __restrict__ b1, int m0, int P1, uint8_t* srow,
                                            int s1row) {
  const int c = threadIdx.x % C1;
  float w[kK];
#pragma unroll
  for (int k = 0; k < kK; ++k) w[k] = w1[c * kK + k];
  const float b = b1[c];
  for (int g = threadIdx.x / C1; g < kLD / 4; g += kThreads / C1) {
    float a[4];
    uint32_t byte = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * g + r, q = m0 - 1 + i;
      float z0, z1;
      conv1_pair(w, b, xs + 2 * i, z0, z1);
      uint32_t code;
      relu_pool2(z0, z1, q >= 0 && q < P1, a[r], code);
      byte |= code << (2 * r);
    }
    *reinterpret_cast<float4*>(a1s + c * kLD + 4 * g) = make_float4(a[0], a[1], a[2], a[3]);
    if (srow && g < kTM / 4 && (m0 >> 2) + g < s1row) srow[(size_t)c * s1row + (m0 >> 2) + g] = (uint8_t)byte;
  }
}

// dL/d(conv2 output m) of channel co: the pooled output m>>1 hands its gradient to the conv output
// its m2 code names.  g / mrow: this row's grad_h2 (C2, P2) and m2 (C2, m2row).
__device__ __forceinline__ float routed_dz2(const float* __restrict__ g, const uint8_t* __restrict__ mrow,
                                            int co, int m, int P2, int m2row) {
  if (m < 0 || m >= 2 * P2) return 0.f;
  const int p = m >> 1;
  const uint32_t code = route2(mrow + (size_t)co * m2row, p);
  return code == (uint32_t)(m & 1) + 1u ? g[(size_t)co * P2 + p] : 0.f;
}

// Ten consecutive k of a GEMM whose A operand is a 5-tap window over two LDS rows: the two k of step
// s (lane half h takes k = 2s + h) sit at p[off] for every step but the one that straddles the rows.
#define PCGMIX_BIG_K10(av, p, p2, o0, o1, o3, o4) \
  const float av[5] = {(p)[o0], (p)[o1], (p2)[0], (p)[o3], (p)[o4]}

// ---------------------------------------------------------------------------------- forward
// acc[nt] += A B for this wave's 32 positions: A[m][(c,tap)] = a1s[c][m + tap], B = w2 streamed.
template <int C1, int C2>
__device__ __forceinline__ void conv2_gemm(const float* a1s, float* w2s, const float* __restrict__ w2,
                                           f32x16 (&acc)[C2 / 32]) {
  constexpr int NT = C2 / 32, LDB = C2 + 1, NG = C1 / kCG, KG = kK * kCG, PF = KG * C2 / kThreads;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  float pf[PF];
#pragma unroll
  for (int e = 0; e < PF; ++e) {
    const int idx = threadIdx.x + kThreads * e;
    pf[e] = w2[(size_t)(idx / KG) * C1 * kK + idx % KG];
  }
  for (int g = 0; g < NG; ++g) {
    __syncthreads();                       // a1s complete / the previous group's reads done
#pragma unroll
    for (int e = 0; e < PF; ++e) {
      const int idx = threadIdx.x + kThreads * e;
      w2s[(idx % KG) * LDB + idx / KG] = pf[e];
    }
    __syncthreads();
    if (g + 1 < NG) {
#pragma unroll
      for (int e = 0; e < PF; ++e) {
        const int idx = threadIdx.x + kThreads * e;
        pf[e] = w2[(size_t)(idx / KG) * C1 * kK + (g + 1) * KG + idx % KG];
      }
    }
    const float* base = a1s + g * kCG * kLD + 32 * w + j;
    const float* pa = base + h;
    const float* pa2 = base + (h ? kLD : 4);
    const float* pb = w2s + h * LDB + j;
#pragma unroll
    for (int cp = 0; cp < kCG / 2; ++cp) {
      PCGMIX_BIG_K10(av, pa + 2 * cp * kLD, pa2 + 2 * cp * kLD, 0, 2, kLD + 1, kLD + 3);
#pragma unroll
      for (int s = 0; s < 5; ++s)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[nt] = mfma(av[s], pb[(10 * cp + 2 * s) * LDB + 32 * nt], acc[nt]);
    }
  }
}

template <int C1, int C2>
constexpr int fwd_lds_floats() { return C1 * kLD + kK * kCG * (C2 + 1) + kXN; }

// grid (tiles, N).  m2, s1, rnd: each written where non-null.
template <int C1, int C2>
__global__ __launch_bounds__(kThreads) void big_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ h2,
    uint8_t* __restrict__ m2, uint8_t* __restrict__ s1, int T, uint4* __restrict__ rnd,
    long long rnd_n16, const uint32_t* __restrict__ key, uint32_t key_lo, uint32_t key_hi) {
  if (rnd)
    counter_hash_fill(rnd, rnd_n16, key, key_lo, key_hi,
                      ((long long)blockIdx.y * gridDim.x + blockIdx.x) * kThreads + threadIdx.x,
                      (long long)gridDim.x * gridDim.y * kThreads);
  constexpr int NT = C2 / 32, kLDO = 65;
  extern __shared__ __align__(16) float smem[];
  float* a1s = smem;
  float* w2s = a1s + C1 * kLD;
  float* xs = w2s + kK * kCG * (C2 + 1);
  const PotesDims d = potes_dims(T);
  const int s1row = d.s1row(), m2row = d.m2row();
  const int n = blockIdx.y, tile = blockIdx.x, m0 = tile * kTM;
  stage_x(xs, x + (size_t)n * T, 2 * m0 - 3, 2 * kLD + 4, T);
  __syncthreads();
  layer1_tile<C1>(xs, a1s, w1, b1, m0, d.P1, s1 ? s1 + (size_t)n * C1 * s1row : nullptr, s1row);
  if (64 * tile >= d.P2) return;            // a tile that only had routing bytes of layer 1 to write
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const float b = b2[32 * nt + j];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = b;
  }
  conv2_gemm<C1, C2>(a1s, w2s, w2, acc);
  __syncthreads();                          // a1s is dead: the tile's outputs take its place
  float* outs = smem;                       // [C2][65] pooled values, [C2][16] routing bytes
  uint8_t* mbs = reinterpret_cast<uint8_t*>(outs + C2 * kLDO);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      uint32_t byte = 0u;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int pl = 16 * w + 4 * rr + 2 * h + e;
        float o;
        uint32_t code;
        relu_pool2(acc[nt][4 * rr + 2 * e], acc[nt][4 * rr + 2 * e + 1], 64 * tile + pl < d.P2, o, code);
        outs[(32 * nt + j) * kLDO + pl] = o;
        byte |= code << (2 * (2 * h + e));
      }
      byte |= __shfl_xor(byte, 32);
      if (!h) mbs[(32 * nt + j) * 16 + 4 * w + rr] = (uint8_t)byte;
    }
  __syncthreads();
  for (int idx = threadIdx.x; idx < C2 * 64; idx += kThreads) {
    const int col = idx >> 6, pl = idx & 63, p = 64 * tile + pl;
    if (p < d.P2) h2[((size_t)n * C2 + col) * d.P2 + p] = outs[col * kLDO + pl];
  }
  if (m2)
    for (int idx = threadIdx.x; idx < C2 * 16; idx += kThreads) {
      const int col = idx >> 4, bi = 16 * tile + (idx & 15);
      if (bi < m2row) m2[((size_t)n * C2 + col) * m2row + bi] = mbs[idx];
    }
}

// ---------------------------------------------------------------------------------- gw2, gb2
template <int C1, int C2>
constexpr int grad_len() { return kK * C1 + C1 + kK * C1 * C2 + C2; }
template <int C1, int C2>
constexpr int gw2_lds_floats() { return C1 * kLD + C2 * kLDZ + kXN; }

// grid (G): block g takes items g, g + G, .. of the N * gw2_tiles (row, tile) pairs and writes the
// gw2 | gb2 columns of partial[g].
template <int C1, int C2>
__global__ __launch_bounds__(kThreads) void big_gw2_kernel(
    const float* __restrict__ x, const float* __restrict__ grad_h2, const uint8_t* __restrict__ m2,
    const float* __restrict__ w1, const float* __restrict__ b1, float* __restrict__ partial, int N,
    int T) {
  constexpr int kGW2 = kK * C1 + C1, kGB2 = kGW2 + kK * C1 * C2, kLen = grad_len<C1, C2>();
  constexpr int NCT = kK * C1 / 32, NI = (NCT + 3) / 4, NRT = C2 / 32, NB = C2 / 2;
  extern __shared__ __align__(16) float smem[];
  float* a1s = smem;
  float* dzs = a1s + C1 * kLD;
  float* xs = dzs + C2 * kLDZ;
  const PotesDims d = potes_dims(T);
  const int m2row = d.m2row(), tiles = gw2_tiles(d), items = N * tiles;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  f32x16 acc[NI][NRT];
  int boff[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int col = 32 * (w + 4 * i) + j;
    boff[i] = (col / kK) * kLD + col % kK + h;
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][rt][r] = 0.f;
  }
  float gb2[NB];                            // thread (ml = tid & 127) sums channels (tid >> 7) + 2e
#pragma unroll
  for (int e = 0; e < NB; ++e) gb2[e] = 0.f;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int n = item / tiles, m0 = (item - n * tiles) * kTM;
    __syncthreads();                        // the previous item's GEMM reads are done
    stage_x(xs, x + (size_t)n * T, 2 * m0 - 3, 2 * kLD + 4, T);
    const float* g = grad_h2 + (size_t)n * C2 * d.P2;
    const uint8_t* mrow = m2 + (size_t)n * C2 * m2row;
#pragma unroll
    for (int e = 0; e < NB; ++e) {
      const int co = (threadIdx.x >> 7) + 2 * e, ml = threadIdx.x & 127;
      const float v = routed_dz2(g, mrow, co, m0 + ml, d.P2, m2row);
      dzs[co * kLDZ + ml] = v;
      gb2[e] += v;
    }
    __syncthreads();
    layer1_tile<C1>(xs, a1s, w1, b1, m0, d.P1, nullptr, 0);
    __syncthreads();
    const float* pa = dzs + j * kLDZ + h;
#pragma unroll 2
    for (int s = 0; s < kTM / 2; ++s) {
      float av[NRT];
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) av[rt] = pa[32 * rt * kLDZ + 2 * s];
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (w + 4 * i < NCT) {
          const float bv = a1s[boff[i] + 2 * s];
#pragma unroll
          for (int rt = 0; rt < NRT; ++rt) acc[i][rt] = mfma(av[rt], bv, acc[i][rt]);
        }
    }
  }
  float* out = partial + (size_t)blockIdx.x * kLen;
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (w + 4 * i < NCT)
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          out[kGW2 + (32 * rt + acc_row(r, h)) * (kK * C1) + 32 * (w + 4 * i) + j] = acc[i][rt][r];
  __syncthreads();
  float* red = xs;                          // [NB][4]: lanes by xor-shuffles, then the waves in order
#pragma unroll
  for (int e = 0; e < NB; ++e) {
    float v = gb2[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (!lane) red[4 * e + w] = v;
  }
  __syncthreads();
  if (threadIdx.x < C2) {
    const int e = threadIdx.x >> 1, par = threadIdx.x & 1;
    out[kGB2 + threadIdx.x] = red[4 * e + 2 * par] + red[4 * e + 2 * par + 1];
  }
}

// ---------------------------------------------------------------------------------- dA1
// acc[ct][r] = dA1[q = qb + 32w + acc_row(r,h)][c = 32 ct + j] for the 128 positions from qb, from
// dzs[co][ml] = dz2[co][m = qb - 4 + ml], ml < 134: A[q][(co,tap)] = dzs[co][q - qb + 5 - tap],
// B[(co,tap)][c] = w2[co][c][tap], streamed through w2b in groups of kCG output channels.
template <int C1, int C2>
__device__ __forceinline__ void da1_gemm(const float* dzs, float* w2b, const float* __restrict__ w2,
                                         f32x16 (&acc)[C1 / 32]) {
  constexpr int NCT = C1 / 32, LDB = C1 + 1, NG = C2 / kCG, KG = kK * kCG, PF = KG * C1 / kThreads;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  float pf[PF];
#pragma unroll
  for (int e = 0; e < PF; ++e) pf[e] = w2[threadIdx.x + kThreads * e];
  for (int g = 0; g < NG; ++g) {
    __syncthreads();                       // dzs complete / the previous group's reads done
#pragma unroll
    for (int e = 0; e < PF; ++e) {
      const int idx = threadIdx.x + kThreads * e;      // (co_l, c, tap) of the group, as in w2
      w2b[((idx / (kK * C1)) * kK + idx % kK) * LDB + (idx / kK) % C1] = pf[e];
    }
    __syncthreads();
    if (g + 1 < NG) {
#pragma unroll
      for (int e = 0; e < PF; ++e) pf[e] = w2[(size_t)(g + 1) * kCG * C1 * kK + threadIdx.x + kThreads * e];
    }
    const float* base = dzs + g * kCG * kLDQ + 32 * w + j;
    const float* pa = base - h;
    const float* pa2 = base + (h ? kLDQ + 5 : 1);
    const float* pb = w2b + h * LDB + j;
#pragma unroll
    for (int cp = 0; cp < kCG / 2; ++cp) {
      PCGMIX_BIG_K10(av, pa + 2 * cp * kLDQ, pa2 + 2 * cp * kLDQ, 5, 3, kLDQ + 4, kLDQ + 2);
#pragma unroll
      for (int s = 0; s < 5; ++s)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          acc[ct] = mfma(av[s], pb[(10 * cp + 2 * s) * LDB + 32 * ct], acc[ct]);
    }
  }
}

template <int C2>
__device__ __forceinline__ void fill_dzs(float* dzs, const float* __restrict__ g,
                                         const uint8_t* __restrict__ mrow, int mbase, int P2, int m2row) {
  for (int idx = threadIdx.x; idx < C2 * 134; idx += kThreads) {
    const int co = idx / 134, ml = idx - co * 134;
    dzs[co * kLDQ + ml] = routed_dz2(g, mrow, co, mbase + ml, P2, m2row);
  }
}

enum { kGw1 = 0, kDx = 1 };
template <int C1, int C2, int MODE>
constexpr int da1_lds_floats() {
  constexpr int gemm = C2 * kLDQ + kK * kCG * (C1 + 1);
  constexpr int route = C1 * kLDR + C1 * (kTM / 16);
  return MODE == kGw1 ? gemm + kXN : (gemm > route ? gemm : route);
}

// kGw1: grid (G), persistent over the N * gw1_tiles (row, tile) pairs, writes the gw1 | gb1 columns of
//       partial[g] (x, w1, b1, partial used).
// kDx:  grid (in_tiles, N), writes grad_x (s1, w1, grad_x used).
template <int C1, int C2, int MODE>
__global__ __launch_bounds__(kThreads) void big_da1_kernel(
    const float* __restrict__ x, const float* __restrict__ grad_h2, const uint8_t* __restrict__ m2,
    const uint8_t* __restrict__ s1, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, float* __restrict__ partial, float* __restrict__ grad_x, int N, int T) {
  constexpr int NCT = C1 / 32;
  extern __shared__ __align__(16) float smem[];
  float* dzs = smem;
  float* w2b = dzs + C2 * kLDQ;
  const PotesDims d = potes_dims(T);
  const int m2row = d.m2row();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  f32x16 acc[NCT];
  if constexpr (MODE == kGw1) {
    float* xs = w2b + kK * kCG * (C1 + 1);
    const int tiles = gw1_tiles(d), items = N * tiles;
    float wr[NCT][kK], br[NCT], gw[NCT][kK], gb[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      br[ct] = b1[32 * ct + j];
      gb[ct] = 0.f;
#pragma unroll
      for (int k = 0; k < kK; ++k) {
        wr[ct][k] = w1[(32 * ct + j) * kK + k];
        gw[ct][k] = 0.f;
      }
    }
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
      const int n = item / tiles, q0 = (item - n * tiles) * kTM;
      __syncthreads();                      // the previous item's reads of xs and dzs are done
      stage_x(xs, x + (size_t)n * T, 2 * q0 - 1, 2 * kTM + 5, T);      // xs[u] = x[2 q0 - 1 + u]
      fill_dzs<C2>(dzs, grad_h2 + (size_t)n * C2 * d.P2, m2 + (size_t)n * C2 * m2row, q0 - 4, d.P2, m2row);
      da1_gemm<C1, C2>(dzs, w2b, w2, acc);
      // route by the first layer's own decisions: conv output 2q + (code - 1) read x[2q + code - 2 + k]
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = 32 * w + acc_row(r, h);
          float z0, z1, a;
          uint32_t code;
          conv1_pair(wr[ct], br[ct], xs + 2 * ql, z0, z1);
          relu_pool2(z0, z1, q0 + ql < d.P1, a, code);
          const float gz = code ? acc[ct][r] : 0.f;
          const float* xw = xs + 2 * ql + (code == 2u ? 1 : 0);
          gb[ct] += gz;
#pragma unroll
          for (int k = 0; k < kK; ++k) gw[ct][k] = fmaf(gz, xw[k], gw[ct][k]);
        }
    }
    // the eight holders of a channel (four waves, two lane halves), in a fixed order
    __syncthreads();
    float* red = smem;                      // [8][6 C1]
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      float* r8 = red + (2 * w + h) * 6 * C1;
#pragma unroll
      for (int k = 0; k < kK; ++k) r8[(32 * ct + j) * kK + k] = gw[ct][k];
      r8[kK * C1 + 32 * ct + j] = gb[ct];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 6 * C1; e += kThreads) {
      float v = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) v += red[u * 6 * C1 + e];
      partial[(size_t)blockIdx.x * grad_len<C1, C2>() + e] = v;
    }
  } else {
    const int n = blockIdx.y, t0 = blockIdx.x * kInTT, qb = (t0 >> 1) - 2;
    const int s1row = d.s1row();
    fill_dzs<C2>(dzs, grad_h2 + (size_t)n * C2 * d.P2, m2 + (size_t)n * C2 * m2row, qb - 4, d.P2, m2row);
    da1_gemm<C1, C2>(dzs, w2b, w2, acc);
    __syncthreads();                        // the GEMM's operands are dead: dA1 and its codes take over
    float* rs = smem;                       // [C1][129] dA1, then [C1][32] bytes: four codes each
    uint8_t* cds = reinterpret_cast<uint8_t*>(rs + C1 * kLDR);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int c = 32 * ct + j;
      const uint8_t* srow = s1 + ((size_t)n * C1 + c) * s1row;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        uint32_t byte = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ql = 32 * w + 8 * rr + 4 * h + e, q = qb + ql;
          rs[c * kLDR + ql] = acc[ct][4 * rr + e];
          if (q >= 0 && q < d.P1) byte |= route2(srow, q + 1) << (2 * e);
        }
        cds[c * (kTM / 4) + 8 * w + 2 * rr + h] = (uint8_t)byte;
      }
    }
    __syncthreads();
    // u[e][k] = sum over c of w1[c][k] dz1[c][o = 2q + e]: thread (ql, half of the channels)
    const int ql = threadIdx.x & (kTM - 1), half = threadIdx.x >> 7;
    float u[2][kK];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int k = 0; k < kK; ++k) u[e][k] = 0.f;
    for (int c = half * (C1 / 2); c < (half + 1) * (C1 / 2); ++c) {
      const float v = rs[c * kLDR + ql];
      const uint32_t code = route2_of(cds[c * (kTM / 4) + (ql >> 2)], ql);
      const float v0 = code == 1u ? v : 0.f, v1 = code == 2u ? v : 0.f;
#pragma unroll
      for (int k = 0; k < kK; ++k) {
        const float wk = w1[c * kK + k];
        u[0][k] = fmaf(wk, v0, u[0][k]);
        u[1][k] = fmaf(wk, v1, u[1][k]);
      }
    }
    __syncthreads();
    float* us = smem;                       // [half][k][o_l = 2 ql + e], o = t0 - 4 + o_l
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int k = 0; k < kK; ++k) us[(half * kK + k) * (2 * kTM) + 2 * ql + e] = u[e][k];
    __syncthreads();
    // dx[t] = sum over k of u_k[o = t + 1 - k], o_l = t - t0 + 5 - k
    const int tt = threadIdx.x;
    if (tt < kInTT && t0 + tt < T) {
      float dx = 0.f;
#pragma unroll
      for (int k = 0; k < kK; ++k)
        dx += us[k * (2 * kTM) + tt + 5 - k] + us[(kK + k) * (2 * kTM) + tt + 5 - k];
      grad_x[(size_t)n * T + t0 + tt] = dx;
    }
  }
}

// grid (ceil(len / 64)): 64 columns of partial (G, len) per block, four row groups in a fixed order.
__global__ __launch_bounds__(kThreads) void big_reduce_kernel(const float* __restrict__ partial,
                                                              float* __restrict__ grads, int G, int len) {
  __shared__ float red[4][64];
  const int cx = threadIdx.x & 63, rg = threadIdx.x >> 6, e = blockIdx.x * 64 + cx;
  float v = 0.f;
  if (e < len)
    for (int g = rg; g < G; g += 4) v += partial[(size_t)g * len + e];
  red[rg][cx] = v;
  __syncthreads();
  if (!rg && e < len) grads[e] = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
}

inline bool supported(int C1, int C2) { return (C1 == 64 && C2 == 32) || (C1 == 128 && C2 == 64); }
inline int grad_len_of(int C1, int C2) { return kK * C1 + C1 + kK * C1 * C2 + C2; }

static long long env_blocks(const char* name, long long dflt, long long max) {
  if (const char* env = getenv(name)) {
    const long long v = atoll(env);
    if (v >= 1 && v <= max) return v;
  }
  return dflt;
}

template <int C1, int C2>
static int launch_fwd(dim3 grid, hipStream_t s, const float* x, const float* w1, const float* b1,
                      const float* w2, const float* b2, float* h2, uint8_t* m2, uint8_t* s1, int T,
                      uint4* rnd, long long n16, const uint32_t* key_dev, uint32_t klo, uint32_t khi) {
  static unsigned long long lds_ok = 0;
  constexpr int lds = fwd_lds_floats<C1, C2>() * 4;
  auto kern = big_fwd_kernel<C1, C2>;
  if (hipError_t e = allow_large_lds(reinterpret_cast<const void*>(kern), &lds_ok, lds)) return (int)e;
  hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, s, x, w1, b1, w2, b2, h2, m2, s1, T, rnd, n16,
                     key_dev, klo, khi);
  return (int)hipGetLastError();
}

template <int C1, int C2>
static int launch_bwd(int G, hipStream_t s, const float* x, const float* grad_h2, const uint8_t* m2,
                      const float* w1, const float* b1, const float* w2, float* partial, float* grads,
                      int N, int T) {
  static unsigned long long ok_a = 0, ok_b = 0;
  constexpr int lds_a = gw2_lds_floats<C1, C2>() * 4, lds_b = da1_lds_floats<C1, C2, kGw1>() * 4;
  constexpr int len = grad_len<C1, C2>();
  auto ka = big_gw2_kernel<C1, C2>;
  auto kb = big_da1_kernel<C1, C2, kGw1>;
  if (hipError_t e = allow_large_lds(reinterpret_cast<const void*>(ka), &ok_a, lds_a)) return (int)e;
  if (hipError_t e = allow_large_lds(reinterpret_cast<const void*>(kb), &ok_b, lds_b)) return (int)e;
  hipLaunchKernelGGL(ka, dim3((unsigned)G), dim3(kThreads), lds_a, s, x, grad_h2, m2, w1, b1, partial, N, T);
  hipLaunchKernelGGL(kb, dim3((unsigned)G), dim3(kThreads), lds_b, s, x, grad_h2, m2,
                     (const uint8_t*)nullptr, w1, b1, w2, partial, (float*)nullptr, N, T);
  hipLaunchKernelGGL(big_reduce_kernel, dim3((unsigned)((len + 63) / 64)), dim3(kThreads), 0, s, partial,
                     grads, G, len);
  return (int)hipGetLastError();
}

template <int C1, int C2>
static int launch_dx(dim3 grid, hipStream_t s, const float* grad_h2, const uint8_t* m2, const uint8_t* s1,
                     const float* w1, const float* w2, float* grad_x, int N, int T) {
  static unsigned long long lds_ok = 0;
  constexpr int lds = da1_lds_floats<C1, C2, kDx>() * 4;
  auto kern = big_da1_kernel<C1, C2, kDx>;
  if (hipError_t e = allow_large_lds(reinterpret_cast<const void*>(kern), &lds_ok, lds)) return (int)e;
  hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, s, (const float*)nullptr, grad_h2, m2, s1, w1,
                     (const float*)nullptr, w2, (float*)nullptr, grad_x, N, T);
  return (int)hipGetLastError();
}

}  // namespace big
}  // namespace pcgmix

using namespace pcgmix;
using namespace pcgmix::big;

extern "C" int pcgmix_potes_big_supported(int C1, int C2) { return supported(C1, C2) ? 1 : 0; }

extern "C" int pcgmix_potes_big_grad_len(int C1, int C2) {
  return supported(C1, C2) ? grad_len_of(C1, C2) : 0;
}

extern "C" int pcgmix_potes_big_bwd_blocks(int N, int T, int C1, int C2) {
  if (!supported(C1, C2) || N <= 0 || N > kMaxN || T < 14) return 0;
  // persistent blocks that keep the gw2 accumulators in registers for the whole launch: one per CU at
  // [128,64] (160 accumulator registers a lane), two at [64,32]
  const PotesDims d = potes_dims(T);
  const long long ta = gw2_tiles(d), tb = gw1_tiles(d), work = (long long)N * (ta < tb ? ta : tb);
  const long long cap = env_blocks("PCGMIX_POTES_BIG_BWD_BLOCKS", C1 == 64 ? 512 : 256, 65535);
  return (int)(work < cap ? work : cap);
}

extern "C" long long pcgmix_potes_big_mask_bytes(int N, int T, int C1, int C2, int layer) {
  if (!supported(C1, C2) || N <= 0 || N > kMaxN || T < 14) return 0;
  const PotesDims d = potes_dims(T);
  return layer == 2 ? (long long)N * C2 * d.m2row() : (layer == 1 ? (long long)N * C1 * d.s1row() : 0);
}

extern "C" int pcgmix_potes_big_fwd_f32(const float* x, const float* w1, const float* b1,
                                        const float* w2, const float* b2, float* h2, uint8_t* m2,
                                        uint8_t* s1, int N, int T, int C1, int C2, uint8_t* rnd_out,
                                        long long rnd_bytes, const uint32_t* key_dev, uint64_t key,
                                        pcgmix_stream_t stream) {
  if (!supported(C1, C2) || !x || !w1 || !b1 || !w2 || !b2 || !h2 || N < 0 || N > kMaxN || T < 14)
    return hipErrorInvalidValue;
  if (!pcgmix::dropout_fill_args_ok(rnd_out, rnd_bytes, N)) return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  const dim3 grid((unsigned)fwd_tiles(potes_dims(T), s1 != nullptr), (unsigned)N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint4* rnd = reinterpret_cast<uint4*>(rnd_out);
  const long long n16 = rnd_out ? rnd_bytes / 16 : 0ll;
  const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
  return C1 == 64 ? launch_fwd<64, 32>(grid, s, x, w1, b1, w2, b2, h2, m2, s1, T, rnd, n16, key_dev, klo, khi)
                  : launch_fwd<128, 64>(grid, s, x, w1, b1, w2, b2, h2, m2, s1, T, rnd, n16, key_dev, klo, khi);
}

extern "C" int pcgmix_potes_big_bwd_mask_f32(const float* x, const float* grad_h2, const uint8_t* m2,
                                             const float* w1, const float* b1, const float* w2,
                                             const float* b2, float* partial, float* grads, int N,
                                             int T, int C1, int C2, pcgmix_stream_t stream) {
  if (!supported(C1, C2) || !x || !grad_h2 || !m2 || !w1 || !b1 || !w2 || !b2 || !partial || !grads ||
      N < 0 || N > kMaxN || T < 14)
    return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  const int G = pcgmix_potes_big_bwd_blocks(N, T, C1, C2);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return C1 == 64 ? launch_bwd<64, 32>(G, s, x, grad_h2, m2, w1, b1, w2, partial, grads, N, T)
                  : launch_bwd<128, 64>(G, s, x, grad_h2, m2, w1, b1, w2, partial, grads, N, T);
}

extern "C" int pcgmix_potes_big_input_grad_mask_f32(const float* grad_h2, const uint8_t* m2,
                                                    const uint8_t* s1, const float* w1,
                                                    const float* w2, float* grad_x, int N, int T,
                                                    int C1, int C2, pcgmix_stream_t stream) {
  if (!supported(C1, C2) || !grad_h2 || !m2 || !s1 || !w1 || !w2 || !grad_x || N < 0 || N > kMaxN ||
      T < 14)
    return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  const dim3 grid((unsigned)in_tiles(T), (unsigned)N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return C1 == 64 ? launch_dx<64, 32>(grid, s, grad_h2, m2, s1, w1, w2, grad_x, N, T)
                  : launch_dx<128, 64>(grid, s, grad_h2, m2, s1, w1, w2, grad_x, N, T);
}
