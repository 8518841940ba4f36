// pcgmix_conv3x3.hip — Conv2d(k = 3x3, pad = 1, stride 1) of ResNet9-2D on the f32 matrix
// instruction (gfx950), channels innermost.
//
// Reference: models2d.py:6-11 (conv_block's nn.Conv2d(c_in, c_out, kernel_size=3, padding=1)) as the
// frozen saliency pass (saliency.py:26-61, 93-113) and test_data_accuracy (train_model.py:591-670)
// run it.  No bias: it is folded into the BatchNorm kernels behind this one (pcgmix_bnrp.hip).
//
//     y[b][h][v][o] = sum over kh, kw, i of  x[b][h + kh - 1][v + kw - 1][i] * w[o][kh][kw][i]
//                     (zero outside [0, H) x [0, W) of every sample)
//
// The input gradient of the same layer is this convolution again with
// w'[i][kh][kw][o] = w[o][2-kh][2-kw][i], so one entry point serves the forward and the frozen backward.
//
// ORDER OF SUMMATION (a function of (Cin, Cout) alone; no split-K, no atomics, the whole of K in one
// thread or one block, so an element's bits depend on its sample's x and on w alone):
//   Cin % 16 == 0, Cout % 16 == 0   conv3x3_kernel<NT>: ONE float32 fmaf chain per output element,
//                      starting from +0: groups of kKC = 16 input channels ascending; in a group
//                      kh = 0, 1, 2; in a kh kw = 0, 1, 2; in a tap the channels ascending.
//   Cin == 1           first_kernel: one fmaf chain from +0 over the taps (kh, kw) = (0,0), (0,1) .. (2,2).
//   Cout == 1          last_kernel: per input pixel and tap a partial p[kh][kw]: lane l of 16 runs one fmaf
//                      chain from +0 over its channels 4 q .. 4 q + 3 of the quads q = l, l + 16, ..
//                      ascending, then the 16 lanes are added in a butterfly (lane distance 8, 4, 2, 1);
//                      y = ((0 + p[0][0](h-1, v-1)) + p[0][1](h-1, v)) + .. + p[2][2](h+1, v+1) with
//                      plain float32 adds, a partial outside the sample being +0.
//
//   conv3x3_kernel<NT> 1-D grid, block = (sample b, tile row, tile column, N tile), the N tile fastest
//                      so that the blocks which share an x tile run together.  The implicit GEMM:
//                      M = output pixels (a tile is kTH x kTW = 8 x 16 pixels of ONE sample, wave w owns
//                      tile rows 2 w and 2 w + 1), N = Cout (32 NT columns per block, columns >= Cout
//                      are zero weights and never stored), K = 9 Cin.
//                      Per group: xs[p][c] = x[h0 - 1 + p / 18][w0 - 1 + p % 18][i0 + c], p < 180 (the tile
//                      and its one-pixel halo; pixels outside the sample are zeros by a select on a
//                      clamped load), staged once per group; per (group, kh):
//                      ws[kw * 16 + c][n] = w[n0 + n][kh][kw][i0 + c] — the nine taps of a group at
//                      NT = 4 would be 92 KB, three of them are 30 KB.  Both go through registers,
//                      loaded for the next step while the matrix unit works on this one.
//                      v_mfma_f32_32x32x2_f32: lane (j, h) supplies A[row j][k = h], B[k = h][col j]
//                      and owns D[(r & 3) + 8 (r >> 2) + 4 h][j] in register r; the result is bit for
//                      bit the k-ordered fmaf chain.
//                      Epilogue: 32 columns at a time through an LDS image [128][40], rows leave as
//                      16-byte stores.
//   first_kernel       Cin == 1 (conv1, 1 -> 64): item = (pixel, quad of output channels), the flat
//                      index over the whole of y, so consecutive threads write consecutive 16 bytes;
//                      the 9 Cout weights sit in LDS as [tap][o].  Bound by the store of y.
//   last_kernel        Cout == 1 (the last hop of the input gradient, 64 -> 1): a block owns 16 x 32
//                      output pixels of one sample, reads every pixel of the tile and its halo ONCE
//                      (16 lanes per pixel, 16 bytes a lane), leaves its nine partials in LDS and adds
//                      them per output pixel.  Bound by the read of x.
//
// LDS: xs 180 x 18 floats (18 p + h: the 64 lanes of an A read hit 62 banks), ws 48 x LDB floats
// (LDB = 32 mod 64: the two k rows of a B read fall in opposite halves of the banks); 19 / 31 / 43 KB
// for NT = 1 / 2 / 4; the output image (20 KB) is aliased on top.  NT = 4 holds 214 registers a lane
// (64 of them the accumulators): two blocks a CU.
// DESIGN.md 3.5f has the roofline and the rates.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "pcgmix_kernels.h"

namespace pcgmix {
namespace conv3x3 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kTH = 8, kTW = 16;          // output pixels per tile: rows x columns
constexpr int kTM = kTH * kTW;            // 128
constexpr int kHW = kTW + 2;              // staged columns: w0 - 1 .. w0 + kTW
constexpr int kPix = (kTH + 2) * kHW;     // staged pixels (180)
constexpr int kKC = 16;                   // input channels per K group
constexpr int kLDX = kKC + 2;             // xs pixel (floats)
constexpr int kLDO = 40;                  // output image row (floats): 4 rows apart = 32 banks apart
constexpr int kPFX = (kPix * 4 + kThreads - 1) / kThreads;       // float4 of x a thread stages per group
constexpr int kMaxC = 1024;

__host__ __device__ constexpr int ldb(int NT) { return NT == 1 ? 32 : 32 * NT + 32; }
__host__ __device__ constexpr int lds_floats(int NT) {
  return kPix * kLDX + 3 * kKC * ldb(NT) > kTM * kLDO ? kPix * kLDX + 3 * kKC * ldb(NT) : kTM * kLDO;
}

inline bool width_ok(int C) { return C == 1 || (C >= 16 && C <= kMaxC && C % 16 == 0); }
inline bool supported(int Cin, int Cout) { return width_ok(Cin) && width_ok(Cout) && !(Cin == 1 && Cout == 1); }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// accumulator register r of lane (j, h): row (r&3) + 8*(r>>2) + 4*h, column j
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int NT>
struct Staged {
  static constexpr int kPFW = (3 * 32 * NT * 4 + kThreads - 1) / kThreads;
  float4 x[kPFX], w[kPFW];
};

// Channels [i0, i0 + 16) of the tile and its halo into registers.  xb: the sample's x; item idx is
// (pixel p = idx >> 2, quad q = idx & 3).
template <int NT>
__device__ __forceinline__ void load_x(Staged<NT>& st, const float* __restrict__ xb, int h0, int w0, int i0,
                                       int H, int W, int Cin) {
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int e = 0; e < kPFX; ++e) {
    const int idx = threadIdx.x + kThreads * e, p = idx >> 2, q = idx & 3;
    st.x[e] = zero;
    if (p < kPix) {
      const int hh = h0 - 1 + p / kHW, vv = w0 - 1 + p % kHW;
      const bool in = hh >= 0 && hh < H && vv >= 0 && vv < W;
      const int hc = hh < 0 ? 0 : (hh >= H ? H - 1 : hh), vc = vv < 0 ? 0 : (vv >= W ? W - 1 : vv);
      const float4 v = *reinterpret_cast<const float4*>(xb + ((size_t)hc * W + vc) * Cin + i0 + 4 * q);
      st.x[e] = in ? v : zero;
    }
  }
}

// The weights of (group i0, kernel row kh): item idx is (kw, column n, quad q) = (idx >> 2) / TN,
// (idx >> 2) % TN, idx & 3.
template <int NT>
__device__ __forceinline__ void load_w(Staged<NT>& st, const float* __restrict__ w, int n0, int i0, int kh,
                                       int Cin, int Cout) {
  constexpr int TN = 32 * NT;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int e = 0; e < Staged<NT>::kPFW; ++e) {
    const int idx = threadIdx.x + kThreads * e, q = idx & 3, n = (idx >> 2) % TN, kw = (idx >> 2) / TN;
    st.w[e] = zero;
    if (kw < 3) {
      const int o = n0 + n, oc = o < Cout ? o : Cout - 1;
      const float4 v = *reinterpret_cast<const float4*>(w + (((size_t)oc * 3 + kh) * 3 + kw) * Cin + i0 + 4 * q);
      st.w[e] = (o == oc) ? v : zero;
    }
  }
}

template <int NT>
__device__ __forceinline__ void store_x(const Staged<NT>& st, float* xs) {
#pragma unroll
  for (int e = 0; e < kPFX; ++e) {
    const int idx = threadIdx.x + kThreads * e, p = idx >> 2, q = idx & 3;
    if (p < kPix) {
      float2* d = reinterpret_cast<float2*>(xs + p * kLDX + 4 * q);
      d[0] = make_float2(st.x[e].x, st.x[e].y);
      d[1] = make_float2(st.x[e].z, st.x[e].w);
    }
  }
}

template <int NT>
__device__ __forceinline__ void store_w(const Staged<NT>& st, float* ws) {
  constexpr int TN = 32 * NT, LDB = ldb(NT);
#pragma unroll
  for (int e = 0; e < Staged<NT>::kPFW; ++e) {
    const int idx = threadIdx.x + kThreads * e, q = idx & 3, n = (idx >> 2) % TN, kw = (idx >> 2) / TN;
    if (kw < 3) {
      float* d = ws + (kw * kKC + 4 * q) * LDB + n;
      d[0] = st.w[e].x;
      d[LDB] = st.w[e].y;
      d[2 * LDB] = st.w[e].z;
      d[3 * LDB] = st.w[e].w;
    }
  }
}

// grid (B * tiles_h * tiles_w * tiles_n).  x (B, H, W, Cin), w (Cout, 3, 3, Cin), y (B, H, W, Cout);
// Cin % 16 == 0.
template <int NT>
__global__ __launch_bounds__(kThreads) void conv3x3_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ w,
                                                           float* __restrict__ y, int H, int W, int Cin,
                                                           int Cout, int tiles_h, int tiles_w, int tiles_n) {
  constexpr int LDB = ldb(NT);
  extern __shared__ __align__(16) float smem[];
  float* xs = smem;
  float* ws = smem + kPix * kLDX;
  const int tn = blockIdx.x % tiles_n, bm = blockIdx.x / tiles_n;
  const int tw = bm % tiles_w, bh = bm / tiles_w, th = bh % tiles_h, b = bh / tiles_h;
  const int h0 = th * kTH, w0 = tw * kTW, n0 = tn * 32 * NT;
  const float* xb = x + (size_t)b * H * W * Cin;
  float* yb = y + (size_t)b * H * W * Cout;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
  Staged<NT> st;
  load_x<NT>(st, xb, h0, w0, 0, H, W, Cin);
  load_w<NT>(st, w, n0, 0, 0, Cin, Cout);
  // row j of the wave's A operand: tile pixel (2 wv + j / 16, j % 16); tap (kh, kw) reads the staged
  // pixel (row + kh, column + kw)
  const float* pa = xs + ((2 * wv + (j >> 4)) * kHW + (j & 15)) * kLDX + h;
  const float* pb = ws + h * LDB + j;
  for (int i0 = 0; i0 < Cin; i0 += kKC) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      __syncthreads();                       // the previous step's reads are done
      if (kh == 0) store_x<NT>(st, xs);
      store_w<NT>(st, ws);
      __syncthreads();
      if (kh < 2) {
        load_w<NT>(st, w, n0, i0, kh + 1, Cin, Cout);
      } else if (i0 + kKC < Cin) {
        load_x<NT>(st, xb, h0, w0, i0 + kKC, H, W, Cin);
        load_w<NT>(st, w, n0, i0 + kKC, 0, Cin, Cout);
      }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int c = 0; c < kKC; c += 2) {
          const float a = pa[(kh * kHW + kw) * kLDX + c];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[nt] = mfma(a, pb[(kw * kKC + c) * LDB + 32 * nt], acc[nt]);
        }
    }
  }
  // the tile leaves 32 columns at a time: registers -> outs[pixel][column] -> 16-byte stores
  float* outs = smem;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    __syncthreads();                         // the GEMM's operands / the previous image are dead
#pragma unroll
    for (int r = 0; r < 16; ++r) outs[(32 * wv + acc_row(r, h)) * kLDO + j] = acc[nt][r];
    __syncthreads();
    const int col = n0 + 32 * nt + 4 * (threadIdx.x & 7);
#pragma unroll
    for (int e = 0; e < kTM / 32; ++e) {
      const int row = (threadIdx.x >> 3) + 32 * e, hh = h0 + row / kTW, vv = w0 + row % kTW;
      if (hh < H && vv < W && col < Cout)
        *reinterpret_cast<float4*>(yb + ((size_t)hh * W + vv) * Cout + col) =
            *reinterpret_cast<const float4*>(outs + row * kLDO + 4 * (threadIdx.x & 7));
    }
  }
}

template <int NT>
static int launch(hipStream_t s, const float* x, const float* w, float* y, int B, int H, int W, int Cin,
                  int Cout) {
  static unsigned long long lds_ok = 0;
  constexpr int lds = lds_floats(NT) * 4;
  const long long tiles_h = (H + kTH - 1) / kTH, tiles_w = (W + kTW - 1) / kTW;
  const long long tiles_n = (Cout + 32 * NT - 1) / (32 * NT);
  const long long blocks = (long long)B * tiles_h * tiles_w * tiles_n;      // < 2**31 * 2**28 / 128 * 32
  if (blocks > INT_MAX) return (int)hipErrorInvalidValue;
  auto kern = conv3x3_kernel<NT>;
  if (hipError_t e = allow_large_lds(reinterpret_cast<const void*>(kern), &lds_ok, lds)) return (int)e;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kThreads), lds, s, x, w, y, H, W, Cin, Cout,
                     (int)tiles_h, (int)tiles_w, (int)tiles_n);
  return (int)hipGetLastError();
}

// ---- Cin == 1 --------------------------------------------------------------------------------
constexpr int kFirstItems = 4;            // (pixel, quad) items per thread

// grid (ceil(B H W Q / (256 * 4))), Q = Cout / 4.  x (B, H, W), w (Cout, 9), y (B, H, W, Cout).
__global__ __launch_bounds__(kThreads) void first_kernel(const float* __restrict__ x,
                                                         const float* __restrict__ w, float* __restrict__ y,
                                                         long long items, int H, int W, int Cout) {
  extern __shared__ __align__(16) float smem[];                  // ws[tap][o]
  for (int idx = threadIdx.x; idx < 9 * Cout; idx += kThreads) smem[(idx % 9) * Cout + idx / 9] = w[idx];
  __syncthreads();
  const int Q = Cout >> 2;
  const long long first = (long long)blockIdx.x * (kThreads * kFirstItems) + threadIdx.x;
#pragma unroll
  for (int e = 0; e < kFirstItems; ++e) {
    const long long item = first + (long long)kThreads * e;
    if (item >= items) break;
    const long long pix = item / Q;
    const int q = (int)(item - pix * Q);
    const long long row = pix / W;                                // b * H + h
    const int v = (int)(pix - row * W), hh = (int)(row % H);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int h2 = hh + kh - 1, v2 = v + kw - 1;
        const bool in = h2 >= 0 && h2 < H && v2 >= 0 && v2 < W;
        // (row + kh - 1) * W + v2 stays inside the sample when `in`
        const float xv = in ? x[(size_t)((row + kh - 1) * W + v2)] : 0.f;
        const float4 wq = *reinterpret_cast<const float4*>(smem + (kh * 3 + kw) * Cout + 4 * q);
        acc.x = fmaf(xv, wq.x, acc.x);
        acc.y = fmaf(xv, wq.y, acc.y);
        acc.z = fmaf(xv, wq.z, acc.z);
        acc.w = fmaf(xv, wq.w, acc.w);
      }
    *reinterpret_cast<float4*>(y + (size_t)item * 4) = acc;
  }
}

static int launch_first(hipStream_t s, const float* x, const float* w, float* y, int B, int H, int W, int Cout) {
  const long long items = (long long)B * H * W * (Cout / 4);
  const long long per = kThreads * kFirstItems, blocks = (items + per - 1) / per;
  if (blocks > INT_MAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(first_kernel, dim3((unsigned)blocks), dim3(kThreads), 9 * Cout * sizeof(float), s, x, w, y,
                     items, H, W, Cout);
  return (int)hipGetLastError();
}

// ---- Cout == 1 -------------------------------------------------------------------------------
constexpr int kLH = 16, kLW = 32;         // output pixels per block: rows x columns
constexpr int kLHW = kLW + 2;
constexpr int kLPix = (kLH + 2) * kLHW;   // 612 pixels with the halo
constexpr int kLLanes = 16;               // lanes per input pixel

// grid (B * tiles_h * tiles_w).  x (B, H, W, Cin), w (9, Cin), y (B, H, W).  LDS: ws[9][Cin], ps[612][9].
__global__ __launch_bounds__(kThreads) void last_kernel(const float* __restrict__ x,
                                                        const float* __restrict__ w, float* __restrict__ y,
                                                        int H, int W, int Cin, int tiles_h, int tiles_w) {
  extern __shared__ __align__(16) float smem[];
  float* ws = smem;
  float* ps = smem + 9 * Cin;
  const int tw = blockIdx.x % tiles_w, bh = blockIdx.x / tiles_w, th = bh % tiles_h, b = bh / tiles_h;
  const int h0 = th * kLH, w0 = tw * kLW;
  const float* xb = x + (size_t)b * H * W * Cin;
  for (int idx = threadIdx.x; idx < 9 * Cin; idx += kThreads) ws[idx] = w[idx];
  __syncthreads();
  const int l = threadIdx.x % kLLanes, quads = Cin >> 2;
  for (int p = threadIdx.x / kLLanes; p < kLPix; p += kThreads / kLLanes) {    // (uniform over the 16 lanes)
    const int hh = h0 - 1 + p / kLHW, vv = w0 - 1 + p % kLHW;
    float part[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) part[t] = 0.f;
    if (hh >= 0 && hh < H && vv >= 0 && vv < W) {
      const float* xp = xb + ((size_t)hh * W + vv) * Cin;
      for (int q = l; q < quads; q += kLLanes) {
        const float4 xv = *reinterpret_cast<const float4*>(xp + 4 * q);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const float4 wq = *reinterpret_cast<const float4*>(ws + t * Cin + 4 * q);
          part[t] = fmaf(xv.w, wq.w, fmaf(xv.z, wq.z, fmaf(xv.y, wq.y, fmaf(xv.x, wq.x, part[t]))));
        }
      }
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int d = kLLanes / 2; d >= 1; d >>= 1) part[t] += __shfl_xor(part[t], d, kLLanes);
    }
    if (l < 9) {
      float mine = part[0];
#pragma unroll
      for (int t = 1; t < 9; ++t) mine = l == t ? part[t] : mine;
      ps[p * 9 + l] = mine;
    }
  }
  __syncthreads();
  float* yb = y + (size_t)b * H * W;
  for (int o = threadIdx.x; o < kLH * kLW; o += kThreads) {
    const int r = o / kLW, c = o % kLW, hh = h0 + r, vv = w0 + c;
    if (hh < H && vv < W) {
      float sum = 0.f;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) sum += ps[((r + kh) * kLHW + c + kw) * 9 + kh * 3 + kw];
      yb[(size_t)hh * W + vv] = sum;
    }
  }
}

static int launch_last(hipStream_t s, const float* x, const float* w, float* y, int B, int H, int W, int Cin) {
  static unsigned long long lds_ok = 0;
  const long long tiles_h = (H + kLH - 1) / kLH, tiles_w = (W + kLW - 1) / kLW;
  const long long blocks = (long long)B * tiles_h * tiles_w;
  if (blocks > INT_MAX) return (int)hipErrorInvalidValue;
  const int lds = (9 * Cin + kLPix * 9) * (int)sizeof(float);                  // at most 58 KB
  if (hipError_t e = allow_large_lds(reinterpret_cast<const void*>(last_kernel), &lds_ok, 64 * 1024))
    return (int)e;
  hipLaunchKernelGGL(last_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, s, x, w, y, H, W, Cin,
                     (int)tiles_h, (int)tiles_w);
  return (int)hipGetLastError();
}

}  // namespace conv3x3
}  // namespace pcgmix

using namespace pcgmix;

extern "C" int pcgmix_conv3x3_tile(int which) {
  return which == 0 ? conv3x3::kTH : (which == 1 ? conv3x3::kTW : (which == 2 ? conv3x3::kKC : 0));
}

extern "C" int pcgmix_conv3x3_supported(int Cin, int Cout) { return conv3x3::supported(Cin, Cout) ? 1 : 0; }

extern "C" int pcgmix_conv3x3_nhwc_f32(const float* x, const float* w, float* y, int B, int H, int W,
                                       int Cin, int Cout, pcgmix_stream_t stream) {
  if (!conv3x3::supported(Cin, Cout) || !x || !w || !y || B < 0 || H < 1 || W < 1) return hipErrorInvalidValue;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y)) & 15u))
    return hipErrorInvalidValue;
  // pixels and channels of one sample are indexed in 32 bits, samples in 64
  if ((long long)H * W * (Cin > Cout ? Cin : Cout) > INT_MAX) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (Cin == 1) return conv3x3::launch_first(s, x, w, y, B, H, W, Cout);
  if (Cout == 1) return conv3x3::launch_last(s, x, w, y, B, H, W, Cin);
  // the widest N tile that Cout fills: 128, 64 or 32 columns per block
  if (Cout % 128 == 0) return conv3x3::launch<4>(s, x, w, y, B, H, W, Cin, Cout);
  if (Cout % 64 == 0) return conv3x3::launch<2>(s, x, w, y, B, H, W, Cin, Cout);
  return conv3x3::launch<1>(s, x, w, y, B, H, W, Cin, Cout);
}
