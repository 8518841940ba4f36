// pcgmix_conv3_narrow.hip — Conv1d(k = 3, pad = 1, stride 1) of ResNet9-1D and its weight gradient for
// the 2- and 8-channel layers of resnet9-5k .. resnet9-50k, on the vector ALU (gfx950), channels innermost.
//
// Reference: models.py:468-473 (conv_block's nn.Conv1d(c_in, c_out, kernel_size=3, padding=1)).  The
// matrix kernels (pcgmix_conv3.hip, pcgmix_conv3_wgrad.hip) take Cin % 4 == 0 and Cout == 4 or
// Cout % 16 == 0; this file takes the pairs with Cin, Cout in {2, 4, 8, 16} that they refuse — Cin == 2
// or Cout in {2, 8}, ten pairs — under the same memory contract:
//
//     y[b][l][o]      = sum over tap, i of  x[b][l + tap - 1][i] * w[o][tap][i]    (x zero outside [0, L))
//     dw[o][tap][i]   = sum over b, l of    dy[b][l][o] * x[b][l + tap - 1][i]
//
// A layer moves 4 (Cin + Cout) bytes per position for at most 3 * 16 * 8 FMAs: the bound is HBM and the
// launch, not arithmetic, so there is no matrix instruction and no LDS staging here.  A row of 2 channels
// is one float2, any other row float4s; a row outside the sample is zeros by a select on a clamped
// load — a neighbouring sample is never read.
//
//   fwd_kernel<CI, CO>    1-D grid, block = (sample b, tile of kTM = 256 positions), one position a thread.
//                         The thread loads the rows l - 1, l, l + 1 (neighbouring lanes share them through
//                         the cache) and, per output channel, runs ONE fmaf chain from +0: tap 0, 1, 2, in
//                         a tap the channels ascending — the matrix kernel's rule for a single K group.
//                         The weights are read at block-uniform addresses.  No split-K, no atomics: an
//                         element's bits depend on its sample's x and on w alone.
//                         The input gradient is this kernel on dy with w'[i][tap][o] = w[o][2-tap][i].
//   wgrad_kernel<CI, CO>  1-D grid of S blocks.  A unit of reduction is a K tile: kTK = 256 consecutive
//                         positions of ONE sample, numbered u = b * ceil(L / kTK) + t; split s of S takes
//                         the units [s U / S, (s + 1) U / S) in ascending order.  The outputs are cut
//                         into NT register tiles of TO x 3 x TI (TO = min(CO, 4), TI = min(CI, 4)); thread
//                         tid is (group g = tid / NT, tile tid % NT), G = 256 / NT groups.  In a unit,
//                         group g takes the NT consecutive positions p0 + g NT .. p0 + g NT + NT - 1 in
//                         ascending order, one fmaf per accumulator and position (acc = fmaf(dy, x, acc));
//                         the x row of one position is the next one's row l - 1.  Rows beyond the sample
//                         add fmaf(0, 0, acc).
//                         Then the G groups of a tile combine through an LDS tree, written out:
//                             for h = G / 2, G / 4, .., 1:   v[g] = v[g] + v[g + h]   for every g < h
//                         (plain float32 adds, a barrier before each level), and group 0 stores ONE
//                         partial part[s][CO][3][CI]; with S == 1 that store is dw itself.
//   reduce_kernel         one block per float4 of dw: the S partials are fetched side by side into LDS,
//                         then one thread adds them, dw = ((0 + part[0]) + part[1]) + .. + part[S - 1]:
//                         plain float32 adds, ascending s.  It reads exactly the words the first launch of
//                         the same call wrote.  With S == 0 it writes zeros (the empty batch).
//
// S is a pure function of (B, L) — see plan() — never of the device or the environment, and there are
// no atomics, no grid-wide wait and no allocation in the call: dw's bits are a function of the arguments
// alone.  Unlike y they DO depend on B (B sets the number of units, hence S and each split's range).
//
// Registers (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), scratch 0 everywhere:
//   (CI, CO)        2,2  2,4  2,8  2,16  4,2  8,2  16,2  4,8  8,8  16,8
//   fwd VGPRs        17   18   22    24   24   46   100   36   58   104
//   wgrad VGPRs      36   48   70    83   54   70    82  102  131   170
//   reduce_kernel   36 VGPRs
// LDS: wgrad 256 x TO x 3 x TI floats (12 .. 48 KB), reduce 16 KB.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "pcgmix_kernels.h"

namespace pcgmix {
namespace conv3n {

constexpr int kThreads = 256;
constexpr int kTM = 256;                  // forward: positions per block, one a thread
constexpr int kTK = 256;                  // weight gradient: positions per K tile
constexpr int kMaxS = 1024;               // splits at most: four blocks on each of 256 CUs — a constant, not a query

// every pair of widths this file compiles
#define PCGMIX_CONV3_NARROW_PAIRS(X) X(2, 2) X(2, 4) X(2, 8) X(2, 16) X(4, 2) X(8, 2) X(16, 2) X(4, 8) X(8, 8) X(16, 8)

inline bool width(int c) { return c == 2 || c == 4 || c == 8 || c == 16; }
inline bool supported(int Cin, int Cout) {
  return width(Cin) && width(Cout) && (Cin == 2 || Cout == 2 || Cout == 8);
}

// W = 2 or 4 consecutive floats as one load / store; keep == false gives zeros (a select, not a branch)
template <int W>
__device__ __forceinline__ void load_row(float* d, const float* __restrict__ p, bool keep) {
  if constexpr (W == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    d[0] = keep ? v.x : 0.f;
    d[1] = keep ? v.y : 0.f;
  } else {
    const float4 v = *reinterpret_cast<const float4*>(p);
    d[0] = keep ? v.x : 0.f;
    d[1] = keep ? v.y : 0.f;
    d[2] = keep ? v.z : 0.f;
    d[3] = keep ? v.w : 0.f;
  }
}
template <int W>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float* s) {
  if constexpr (W == 2)
    *reinterpret_cast<float2*>(p) = make_float2(s[0], s[1]);
  else
    *reinterpret_cast<float4*>(p) = make_float4(s[0], s[1], s[2], s[3]);
}
// W channels from c0 of row l of a sample (xb: its first row, C channels a row); zeros outside [0, L)
template <int W>
__device__ __forceinline__ void load_pos(float* d, const float* __restrict__ xb, int l, int L, int C, int c0) {
  const int lc = l < 0 ? 0 : (l >= L ? L - 1 : l);
  load_row<W>(d, xb + (size_t)lc * C + c0, l == lc);
}

// grid (B * tilesL).  x (B, L, CI), w (CO, 3, CI), y (B, L, CO).
template <int CI, int CO>
__global__ __launch_bounds__(kThreads) void fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       float* __restrict__ y, int L, int tilesL) {
  constexpr int WI = CI == 2 ? 2 : 4, WO = CO == 2 ? 2 : 4;
  const int b = blockIdx.x / tilesL, l = (blockIdx.x - b * tilesL) * kTM + threadIdx.x;
  if (l >= L) return;
  const float* xb = x + (size_t)b * L * CI;
  float xr[3][CI];
#pragma unroll
  for (int tap = 0; tap < 3; ++tap)
#pragma unroll
    for (int c = 0; c < CI; c += WI) load_pos<WI>(&xr[tap][c], xb, l + tap - 1, L, CI, c);
  float acc[CO];
#pragma unroll
  for (int o = 0; o < CO; ++o) {
    float a = 0.f;
#pragma unroll
    for (int tap = 0; tap < 3; ++tap)
#pragma unroll
      for (int i = 0; i < CI; ++i) a = fmaf(xr[tap][i], w[(o * 3 + tap) * CI + i], a);
    acc[o] = a;
  }
  float* yr = y + ((size_t)b * L + l) * CO;
#pragma unroll
  for (int o = 0; o < CO; o += WO) store_row<WO>(yr + o, &acc[o]);
}

// grid (S).  x (B, L, CI), dy (B, L, CO), out (S, CO, 3, CI).
template <int CI, int CO>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ out, int L, int tilesL,
                                                         long long units, int S) {
  constexpr int TI = CI < 4 ? CI : 4, TO = CO < 4 ? CO : 4, NTI = CI / TI, NT = NTI * (CO / TO);
  constexpr int G = kThreads / NT, R = kTK / G, A = TO * 3 * TI;
  __shared__ float red[A * kThreads];     // red[a][tid]: a level's reads and writes run along the banks
  const int s = blockIdx.x, tid = threadIdx.x;
  const int tile = tid % NT, g = tid / NT, o0 = (tile / NTI) * TO, i0 = (tile % NTI) * TI;
  const long long u0 = (long long)s * units / S, u1 = (long long)(s + 1) * units / S;
  float acc[TO][3][TI];
#pragma unroll
  for (int oo = 0; oo < TO; ++oo)
#pragma unroll
    for (int tap = 0; tap < 3; ++tap)
#pragma unroll
      for (int ii = 0; ii < TI; ++ii) acc[oo][tap][ii] = 0.f;
  int b = (int)(u0 / tilesL), t = (int)(u0 - (long long)b * tilesL);
  for (long long u = u0; u < u1; ++u) {
    const float* xb = x + (size_t)b * L * CI;
    const float* dyb = dy + (size_t)b * L * CO;
    const int q0 = t * kTK + g * R;
    float xw[3][TI], d[TO];               // the rows q - 1, q, q + 1
    load_pos<TI>(xw[0], xb, q0 - 1, L, CI, i0);
    load_pos<TI>(xw[1], xb, q0, L, CI, i0);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      load_pos<TI>(xw[2], xb, q0 + k + 1, L, CI, i0);
      load_pos<TO>(d, dyb, q0 + k, L, CO, o0);
#pragma unroll
      for (int oo = 0; oo < TO; ++oo)
#pragma unroll
        for (int tap = 0; tap < 3; ++tap)
#pragma unroll
          for (int ii = 0; ii < TI; ++ii) acc[oo][tap][ii] = fmaf(d[oo], xw[tap][ii], acc[oo][tap][ii]);
#pragma unroll
      for (int ii = 0; ii < TI; ++ii) {
        xw[0][ii] = xw[1][ii];
        xw[1][ii] = xw[2][ii];
      }
    }
    if (++t == tilesL) {
      t = 0;
      ++b;
    }
  }
  // the tree over the groups of a tile: v[g] += v[g + h], h = G / 2 .. 1
  float* mine = red + tid;
#pragma unroll
  for (int h = G / 2; h >= 1; h >>= 1) {
    if (g < 2 * h) {
#pragma unroll
      for (int a = 0; a < A; ++a) mine[a * kThreads] = acc[a / (3 * TI)][(a / TI) % 3][a % TI];
    }
    __syncthreads();
    if (g < h) {
#pragma unroll
      for (int a = 0; a < A; ++a) acc[a / (3 * TI)][(a / TI) % 3][a % TI] += mine[a * kThreads + h * NT];
    }
    __syncthreads();                      // the level's reads are done before the next level's writes
  }
  if (g == 0) {
    float* outb = out + (size_t)s * CO * 3 * CI;
#pragma unroll
    for (int oo = 0; oo < TO; ++oo)
#pragma unroll
      for (int tap = 0; tap < 3; ++tap) store_row<TI>(outb + ((o0 + oo) * 3 + tap) * CI + i0, acc[oo][tap]);
  }
}

// grid (n4).  dw[e] = part[0][e] + part[1][e] + ... in ascending s; n4 float4 per partial, S <= kMaxS.
__global__ __launch_bounds__(kThreads) void reduce_kernel(const float4* __restrict__ part, float4* __restrict__ dw,
                                                          int n4, int S) {
  __shared__ float4 v[kMaxS];
  const int e = blockIdx.x;
  for (int s = threadIdx.x; s < S; s += kThreads) v[s] = part[(size_t)s * n4 + e];
  __syncthreads();
  if (threadIdx.x != 0) return;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < S; ++s) {
    const float4 p = v[s];
    a.x += p.x;
    a.y += p.y;
    a.z += p.z;
    a.w += p.w;
  }
  dw[e] = a;
}

// The split count: at most kMaxS blocks, at least two units per split, at least one split.  Nothing but
// the arguments enters.
static int plan(int B, int L, int Cin, int Cout, int* splits, size_t* bytes) {
  if (!supported(Cin, Cout) || B < 0 || L < 1) return (int)hipErrorInvalidValue;
  const long long units = (long long)B * ((L + kTK - 1) / kTK);
  long long S = units / 2 < kMaxS ? units / 2 : kMaxS;
  if (S < 1) S = 1;
  *splits = (int)S;
  *bytes = S > 1 ? (size_t)S * Cout * 3 * Cin * sizeof(float) : 0;
  return 0;
}

static int launch_fwd(hipStream_t st, const float* x, const float* w, float* y, int B, int L, int Cin, int Cout) {
  const int tilesL = (L + kTM - 1) / kTM;
  const long long blocks = (long long)B * tilesL;
  if (blocks > INT_MAX) return (int)hipErrorInvalidValue;
#define PCGMIX_CASE(CI, CO)                                                                                  \
  if (Cin == CI && Cout == CO)                                                                               \
    hipLaunchKernelGGL((fwd_kernel<CI, CO>), dim3((unsigned)blocks), dim3(kThreads), 0, st, x, w, y, L, tilesL);
  PCGMIX_CONV3_NARROW_PAIRS(PCGMIX_CASE)
#undef PCGMIX_CASE
  return (int)hipGetLastError();
}

static int launch_wgrad(hipStream_t st, const float* x, const float* dy, float* out, int B, int L, int Cin,
                        int Cout, int S) {
  const int tilesL = (L + kTK - 1) / kTK;
  const long long units = (long long)B * tilesL;
#define PCGMIX_CASE(CI, CO)                                                                                  \
  if (Cin == CI && Cout == CO)                                                                               \
    hipLaunchKernelGGL((wgrad_kernel<CI, CO>), dim3((unsigned)S), dim3(kThreads), 0, st, x, dy, out, L, tilesL, \
                       units, S);
  PCGMIX_CONV3_NARROW_PAIRS(PCGMIX_CASE)
#undef PCGMIX_CASE
  return (int)hipGetLastError();
}

}  // namespace conv3n
}  // namespace pcgmix

using namespace pcgmix;

extern "C" int pcgmix_conv3_narrow_supported(int Cin, int Cout) { return conv3n::supported(Cin, Cout) ? 1 : 0; }

extern "C" int pcgmix_conv3_narrow_tile(int which) {
  return which == 0 ? conv3n::kTM : (which == 1 ? conv3n::kTK : 0);
}

extern "C" int pcgmix_conv3_narrow_nlc_f32(const float* x, const float* w, float* y, int B, int L, int Cin,
                                           int Cout, pcgmix_stream_t stream) {
  if (!conv3n::supported(Cin, Cout) || !x || !w || !y || B < 0 || L < 1) return hipErrorInvalidValue;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y)) & 15u))
    return hipErrorInvalidValue;
  // positions and channels of one sample are indexed in 32 bits, samples in 64
  if ((long long)L * (Cin > Cout ? Cin : Cout) > INT_MAX) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  return conv3n::launch_fwd(reinterpret_cast<hipStream_t>(stream), x, w, y, B, L, Cin, Cout);
}

extern "C" int pcgmix_conv3_narrow_wgrad_plan(int B, int L, int Cin, int Cout, int* splits,
                                              size_t* workspace_bytes) {
  int S = 0;
  size_t bytes = 0;
  if (int e = conv3n::plan(B, L, Cin, Cout, &S, &bytes)) return e;
  if (splits) *splits = S;
  if (workspace_bytes) *workspace_bytes = bytes;
  return 0;
}

extern "C" int pcgmix_conv3_narrow_wgrad_nlc_f32(const float* x, const float* dy, float* dw, void* workspace,
                                                 size_t workspace_bytes, int B, int L, int Cin, int Cout,
                                                 pcgmix_stream_t stream) {
  int S = 0;
  size_t need = 0;
  if (conv3n::plan(B, L, Cin, Cout, &S, &need) || !x || !dy || !dw) return hipErrorInvalidValue;
  if ((need && !workspace) || workspace_bytes < need) return hipErrorInvalidValue;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dw) |
        reinterpret_cast<uintptr_t>(workspace)) & 15u))
    return hipErrorInvalidValue;
  // positions and channels of one sample are indexed in 32 bits, samples and partials in 64
  if ((long long)L * (Cin > Cout ? Cin : Cout) > INT_MAX) return hipErrorInvalidValue;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int n4 = Cout * 3 * Cin / 4;
  if (B > 0) {
    float* out = S > 1 ? static_cast<float*>(workspace) : dw;
    const int e = conv3n::launch_wgrad(st, x, dy, out, B, L, Cin, Cout, S);
    if (e || S == 1) return e;
  }
  // the partials in ascending order; an empty batch: no partial, zeros
  hipLaunchKernelGGL(conv3n::reduce_kernel, dim3((unsigned)n4), dim3(conv3n::kThreads), 0, st,
                     static_cast<const float4*>(workspace), reinterpret_cast<float4*>(dw), n4, B > 0 ? S : 0);
  return (int)hipGetLastError();
}
