// pcgmix_conv3.hip — Conv1d(k = 3, pad = 1, stride 1) of ResNet9-1D on the f32 matrix instruction
// (gfx950), channels innermost.
//
// Reference: models.py:468-473 (conv_block's nn.Conv1d(c_in, c_out, kernel_size=3, padding=1)) as
// the frozen saliency pass (saliency.py:26-61) and test_data_accuracy (train_model.py:591-670) run
// it.  No bias: it is folded into the BatchNorm kernels behind this one (pcgmix_bnrp.hip).
//
//     y[b][l][o] = sum over tap, i of  x[b][l + tap - 1][i] * w[o][tap][i]      (zero outside [0, L))
//
// The input gradient of the same layer is this convolution again with w'[i][tap][o] = w[o][2-tap][i],
// so one kernel body serves the forward and the frozen backward.
//
//   conv3_kernel<NT>   1-D grid, block = (sample b, M tile, N tile), the N tile fastest so that the
//                      blocks which share an x tile run together.  The implicit GEMM: M = positions
//                      (a tile is kTM = 128 positions of ONE sample, wave w owns 32 w .. 32 w + 31),
//                      N = Cout (32 NT columns per block, columns >= Cout are zero weights and never
//                      stored), K = 3 Cin.  K is walked in groups of kKC = 16 input channels, in a
//                      group tap 0, 1, 2, in a tap the channels in ascending order: one fixed order
//                      per output element, the whole of K in one block — no split-K, no atomics, so
//                      an element's bits depend on its sample's x and on w alone.
//                      Per group: xs[r][c] = x[m0 - 1 + r][i0 + c], r < 130 (the tile and its two halo
//                      rows; rows outside the sample are zeros by a select on a clamped load), and
//                      ws[tap * 16 + c][n] = w[n0 + n][tap][i0 + c]; both through registers, loaded
//                      for group g + 1 while the matrix unit works on group g.
//                      v_mfma_f32_32x32x2_f32: lane (j, h) supplies A[row j][k = h], B[k = h][col j]
//                      and owns D[(r & 3) + 8 (r >> 2) + 4 h][j] in register r; the result is bit for
//                      bit the k-ordered fmaf chain.
//                      Epilogue: 32 columns at a time through an LDS image [128][40], rows leave as
//                      16-byte stores.
//
// LDS: xs 130 x 18 floats (18 j + h: the 64 lanes of an A read hit 64 banks), ws 48 x LDB floats
// (LDB = 32 mod 64: the two k rows of a B read fall in opposite halves of the banks); 17 / 28 / 40 KB
// for NT = 1 / 2 / 4; the output image (20 KB) is aliased on top, so NT = 1 allocates 20 KB.  DESIGN.md 3.5d has the roofline and the rates.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "pcgmix_kernels.h"

namespace pcgmix {
namespace conv3 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kTM = 128;                  // positions per tile
constexpr int kRows = kTM + 2;            // staged rows: m0 - 1 .. m0 + kTM
constexpr int kKC = 16;                   // input channels per K group
constexpr int kLDX = kKC + 2;             // xs row (floats)
constexpr int kLDO = 40;                  // output image row (floats): 4 rows apart = 32 banks apart
constexpr int kPFX = (kRows * 4 + kThreads - 1) / kThreads;      // float4 of x a thread stages per group
constexpr int kMaxC = 1024;

__host__ __device__ constexpr int ldb(int NT) { return NT == 1 ? 32 : 32 * NT + 32; }
__host__ __device__ constexpr int lds_floats(int NT) {
  return kRows * kLDX + 3 * kKC * ldb(NT) > kTM * kLDO ? kRows * kLDX + 3 * kKC * ldb(NT) : kTM * kLDO;
}

inline bool supported(int Cin, int Cout) {
  return Cin >= 4 && Cin <= kMaxC && Cin % 4 == 0 && Cout >= 4 && Cout <= kMaxC &&
         (Cout % 16 == 0 || Cout == 4);
}

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

// Group [i0, i0 + kc) of the input channels into registers.  xb: the sample's x; item idx of x is
// (row r = idx >> 2, quad q = idx & 3), of w (tap, column n, quad q) = (idx >> 2) / TN, (idx >> 2) % TN,
// idx & 3.  A quad beyond kc is never read back by the GEMM and is not loaded.
template <int NT>
__device__ __forceinline__ void load_group(Staged<NT>& st, const float* __restrict__ xb,
                                           const float* __restrict__ w, int m0, int n0, int i0, int kc,
                                           int L, int Cin, int Cout) {
  constexpr int TN = 32 * NT;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int e = 0; e < kPFX; ++e) {
    const int idx = threadIdx.x + kThreads * e, r = idx >> 2, q = idx & 3;
    st.x[e] = zero;
    if (r < kRows && 4 * q < kc) {
      const int l = m0 - 1 + r, lc = l < 0 ? 0 : (l >= L ? L - 1 : l);
      const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)lc * Cin + i0 + 4 * q);
      st.x[e] = (l == lc) ? v : zero;
    }
  }
#pragma unroll
  for (int e = 0; e < Staged<NT>::kPFW; ++e) {
    const int idx = threadIdx.x + kThreads * e, q = idx & 3, n = (idx >> 2) % TN, tap = (idx >> 2) / TN;
    st.w[e] = zero;
    if (tap < 3 && 4 * q < kc) {
      const int o = n0 + n, oc = o < Cout ? o : Cout - 1;
      const float4 v = *reinterpret_cast<const float4*>(w + ((size_t)oc * 3 + tap) * Cin + i0 + 4 * q);
      st.w[e] = (o == oc) ? v : zero;
    }
  }
}

template <int NT>
__device__ __forceinline__ void store_group(const Staged<NT>& st, float* xs, float* ws, int kc) {
  constexpr int TN = 32 * NT, LDB = ldb(NT);
#pragma unroll
  for (int e = 0; e < kPFX; ++e) {
    const int idx = threadIdx.x + kThreads * e, r = idx >> 2, q = idx & 3;
    if (r < kRows && 4 * q < kc) {
      float2* p = reinterpret_cast<float2*>(xs + r * kLDX + 4 * q);
      p[0] = make_float2(st.x[e].x, st.x[e].y);
      p[1] = make_float2(st.x[e].z, st.x[e].w);
    }
  }
#pragma unroll
  for (int e = 0; e < Staged<NT>::kPFW; ++e) {
    const int idx = threadIdx.x + kThreads * e, q = idx & 3, n = (idx >> 2) % TN, tap = (idx >> 2) / TN;
    if (tap < 3 && 4 * q < kc) {
      float* p = ws + (tap * kKC + 4 * q) * LDB + n;
      p[0] = st.w[e].x;
      p[LDB] = st.w[e].y;
      p[2 * LDB] = st.w[e].z;
      p[3 * LDB] = st.w[e].w;
    }
  }
}

// grid (B * tiles_m * tiles_n).  x (B, L, Cin), w (Cout, 3, Cin), y (B, L, Cout).
template <int NT>
__global__ __launch_bounds__(kThreads) void conv3_kernel(const float* __restrict__ x,
                                                         const float* __restrict__ w,
                                                         float* __restrict__ y, int L, int Cin, int Cout,
                                                         int tiles_m, int tiles_n) {
  constexpr int LDB = ldb(NT);
  extern __shared__ __align__(16) float smem[];
  float* xs = smem;
  float* ws = smem + kRows * kLDX;
  const int tn = blockIdx.x % tiles_n, bm = blockIdx.x / tiles_n;
  const int b = bm / tiles_m, m0 = (bm - b * tiles_m) * kTM, n0 = tn * 32 * NT;
  const float* xb = x + (size_t)b * L * Cin;
  float* yb = y + (size_t)b * L * Cout;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
  Staged<NT> st;
  int kc = Cin < kKC ? Cin : kKC;
  load_group<NT>(st, xb, w, m0, n0, 0, kc, L, Cin, Cout);
  for (int i0 = 0; i0 < Cin; i0 += kKC) {
    __syncthreads();                         // the previous group's reads are done
    store_group<NT>(st, xs, ws, kc);
    __syncthreads();
    const int kc_now = kc;
    if (i0 + kKC < Cin) {
      kc = Cin - i0 - kKC < kKC ? Cin - i0 - kKC : kKC;
      load_group<NT>(st, xb, w, m0, n0, i0 + kKC, kc, L, Cin, Cout);
    }
    const float* pa = xs + (32 * wv + j) * kLDX + h;
    const float* pb = ws + h * LDB + j;
#pragma unroll
    for (int tap = 0; tap < 3; ++tap)
#pragma unroll
      for (int c4 = 0; c4 < kKC; c4 += 4)
        if (c4 < kc_now) {                   // (wave-uniform: only a last group is short)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const float a = pa[tap * kLDX + c4 + 2 * s];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[nt] = mfma(a, pb[(tap * kKC + c4 + 2 * s) * LDB + 32 * nt], acc[nt]);
          }
        }
  }
  // the tile leaves 32 columns at a time: registers -> outs[position][column] -> 16-byte stores
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
      const int row = (threadIdx.x >> 3) + 32 * e, l = m0 + row;
      if (l < L && col < Cout)
        *reinterpret_cast<float4*>(yb + (size_t)l * Cout + col) =
            *reinterpret_cast<const float4*>(outs + row * kLDO + 4 * (threadIdx.x & 7));
    }
  }
}

template <int NT>
static int launch(hipStream_t s, const float* x, const float* w, float* y, int B, int L, int Cin,
                  int Cout) {
  static unsigned long long lds_ok = 0;
  constexpr int lds = lds_floats(NT) * 4;
  const long long tiles_m = (L + kTM - 1) / kTM, tiles_n = (Cout + 32 * NT - 1) / (32 * NT);
  const long long blocks = (long long)B * tiles_m * tiles_n;
  if (blocks > INT_MAX) return (int)hipErrorInvalidValue;
  auto kern = conv3_kernel<NT>;
  if (hipError_t e = allow_large_lds(reinterpret_cast<const void*>(kern), &lds_ok, lds)) return (int)e;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kThreads), lds, s, x, w, y, L, Cin, Cout,
                     (int)tiles_m, (int)tiles_n);
  return (int)hipGetLastError();
}

}  // namespace conv3
}  // namespace pcgmix

using namespace pcgmix;

extern "C" int pcgmix_conv3_tile(int which) {
  return which == 0 ? conv3::kTM : (which == 1 ? conv3::kKC : 0);
}

extern "C" int pcgmix_conv3_supported(int Cin, int Cout) { return conv3::supported(Cin, Cout) ? 1 : 0; }

extern "C" int pcgmix_conv3_nlc_f32(const float* x, const float* w, float* y, int B, int L, int Cin,
                                    int Cout, pcgmix_stream_t stream) {
  if (!conv3::supported(Cin, Cout) || !x || !w || !y || B < 0 || L < 1) return hipErrorInvalidValue;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y)) & 15u))
    return hipErrorInvalidValue;
  // positions and channels of one sample are indexed in 32 bits, samples in 64
  if ((long long)L * (Cin > Cout ? Cin : Cout) > INT_MAX) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the widest N tile that Cout fills: 128, 64 or 32 columns per block
  if (Cout % 128 == 0) return conv3::launch<4>(s, x, w, y, B, L, Cin, Cout);
  if (Cout % 64 == 0) return conv3::launch<2>(s, x, w, y, B, L, Cin, Cout);
  return conv3::launch<1>(s, x, w, y, B, L, Cin, Cout);
}
