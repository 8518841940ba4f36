// pcgmix_conv3_wgrad.hip — weight gradient of Conv1d(k = 3, pad = 1, stride 1) of ResNet9-1D on the
// f32 matrix instruction (gfx950), channels innermost, in one fixed order of summation.
//
// Reference: models.py:468-473 (conv_block's nn.Conv1d(c_in, c_out, kernel_size=3, padding=1)) as the
// training step differentiates it.  The forward and the input gradient are pcgmix_conv3.hip.
//
//     dw[o][tap][i] = sum over b, l of  dy[b][l][o] * x[b][l + tap - 1][i]       (x zero outside [0, L))
//
// As a GEMM: M = Cout, N = 3 Cin, K = B L.  Both operands have the reduction index (the position) as
// the outer memory dimension and the channel innermost, so one LDS image [position][channel] of each
// serves the matrix instruction as it stands: lane (j, h) of v_mfma_f32_32x32x2_f32 supplies
// A[row j][k = h] = dy[pos 2s + h][o0 + j] and B[k = h][col j] = x[pos 2s + h + tap - 1][i0 + j].
//
//   wgrad_kernel<NI32>  1-D grid, block = (split s, M tile, N tile), the N tile fastest.  A block owns
//                       kMO = 128 output channels (wave w the rows 32 w .. 32 w + 31) by 3 taps x 32 NI32
//                       input channels: 3 NI32 independent 32x32 accumulators per wave (3 or 6).
//                       A unit of reduction is a K tile: kTK = 64 consecutive positions of ONE sample,
//                       numbered u = b * ceil(L / kTK) + t.  Per unit: dys[r][c] = dy[p0 + r][o0 + c]
//                       (r < 64) and xs[r][c] = x[p0 - 1 + r][i0 + c] (r < 66: one staged x tile serves
//                       the three taps); rows outside [0, L) and channels beyond the layer's are zeros
//                       by a select on a clamped load — a neighbouring sample is never read.  Both go
//                       through registers, loaded for unit u + 1 while the matrix unit works on unit u.
//                       Split s of S takes the units [s U / S, (s + 1) U / S) in ascending order into
//                       its accumulators and stores ONE partial part[s][Cout][3][Cin] straight from
//                       the accumulator registers (register r of a wave is two 128-byte runs); with
//                       S == 1 that store is dw itself.
//   reduce_kernel       dw = ((part[0] + part[1]) + ...) + part[S - 1]: plain float32 adds, ascending s.
//                       It reads exactly the words the first launch of the same call wrote.
//                       With S == 0 it writes zeros (the empty batch).
//
// S is a pure function of (B, L, Cin, Cout) — see plan() — never of the device, its CU count or the
// environment, and there are no atomics, no grid-wide wait and no allocation in the call: dw's bits
// are a function of the arguments alone.  UNLIKE the forward kernel's, they DO depend on B: B sets
// the number of units, hence S and where each split's range ends.
// Non-finite x or dy give a non-finite dw, as in any GEMM (a zero-filled row times inf is NaN).
//
// LDS: dys 64 x 160 floats, xs 66 x 96 (NI32 = 2) or 66 x 32 (NI32 = 1): 66.3 / 49.4 KB.  Both row
// pitches are 32 mod 64 floats, so the two k rows of a fragment read fall in opposite halves of the
// banks; each half-wave reads 32 consecutive floats.  DESIGN.md 3.5e has the tile's derivation.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "pcgmix_kernels.h"

namespace pcgmix {
namespace conv3w {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kTK = 64;                   // positions per K tile
constexpr int kMO = 128;                  // output channels per block
constexpr int kNI = 64;                   // input channels per block (32 where Cin <= 32)
constexpr int kRowsX = kTK + 2;           // staged x rows: p0 - 1 .. p0 + kTK
constexpr int kLDA = kMO + 32;            // dys row (floats)
constexpr int kPFA = kTK * (kMO / 4) / kThreads;                 // float4 of dy a thread stages per unit
constexpr int kMaxC = 1024;
constexpr int kRB = 16;                   // partials a thread of the second launch has in flight
constexpr int kTargetBlocks = 512;       // two resident blocks on each of 256 CUs — a constant, not a query

__host__ __device__ constexpr int ldx(int NI32) { return NI32 == 2 ? 96 : 32; }
__host__ __device__ constexpr int lds_floats(int NI32) { return kTK * kLDA + kRowsX * ldx(NI32); }

inline bool supported(int Cin, int Cout) {
  return Cin >= 4 && Cin <= kMaxC && Cin % 4 == 0 && Cout >= 4 && Cout <= kMaxC &&
         (Cout % 16 == 0 || Cout == 4);
}

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// accumulator register r of lane (j, h): row (r&3) + 8*(r>>2) + 4*h, column j
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// v, or zeros: component by component, so that the choice is four v_cndmask and not a choice of address
__device__ __forceinline__ float4 keep(float4 v, bool k) {
  return make_float4(k ? v.x : 0.f, k ? v.y : 0.f, k ? v.z : 0.f, k ? v.w : 0.f);
}

template <int NI32>
struct Staged {
  static constexpr int kPFX = (kRowsX * 8 * NI32 + kThreads - 1) / kThreads;
  float4 a[kPFA], x[kPFX];
};

// Unit (sample b, tile t) into registers.  Item idx of dy is (row idx >> 5, quad idx & 31), of x
// (row idx / NQ, quad idx % NQ).  A quad beyond the layer's channels is zero and is not loaded.
template <int NI32>
__device__ __forceinline__ void load_unit(Staged<NI32>& st, const float* __restrict__ x,
                                          const float* __restrict__ dy, int b, int t, int o0, int i0,
                                          int L, int Cin, int Cout) {
  constexpr int NQ = 8 * NI32;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const int p0 = t * kTK;
  const float* xb = x + (size_t)b * L * Cin;
  const float* dyb = dy + (size_t)b * L * Cout;
#pragma unroll
  for (int e = 0; e < kPFA; ++e) {
    const int idx = threadIdx.x + kThreads * e, r = idx >> 5, c = o0 + 4 * (idx & 31);
    st.a[e] = zero;
    if (c < Cout) {
      const int p = p0 + r, pc = p >= L ? L - 1 : p;
      const float4 v = *reinterpret_cast<const float4*>(dyb + (size_t)pc * Cout + c);
      st.a[e] = keep(v, p == pc);
    }
  }
#pragma unroll
  for (int e = 0; e < Staged<NI32>::kPFX; ++e) {
    const int idx = threadIdx.x + kThreads * e, r = idx / NQ, c = i0 + 4 * (idx % NQ);
    st.x[e] = zero;
    if (r < kRowsX && c < Cin) {
      const int p = p0 - 1 + r, pc = p < 0 ? 0 : (p >= L ? L - 1 : p);
      const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)pc * Cin + c);
      st.x[e] = keep(v, p == pc);
    }
  }
}

template <int NI32>
__device__ __forceinline__ void store_unit(const Staged<NI32>& st, float* dys, float* xs) {
  constexpr int NQ = 8 * NI32, LDX = ldx(NI32);
#pragma unroll
  for (int e = 0; e < kPFA; ++e) {
    const int idx = threadIdx.x + kThreads * e;
    *reinterpret_cast<float4*>(dys + (idx >> 5) * kLDA + 4 * (idx & 31)) = st.a[e];
  }
#pragma unroll
  for (int e = 0; e < Staged<NI32>::kPFX; ++e) {
    const int idx = threadIdx.x + kThreads * e, r = idx / NQ;
    if (r < kRowsX) *reinterpret_cast<float4*>(xs + r * LDX + 4 * (idx % NQ)) = st.x[e];
  }
}

// grid (S * tiles_o * tiles_i).  x (B, L, Cin), dy (B, L, Cout), out (S, Cout, 3, Cin).
template <int NI32>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(const float* __restrict__ x,
                                                         const float* __restrict__ dy,
                                                         float* __restrict__ out, int L, int Cin, int Cout,
                                                         int tilesL, long long units, int S, int tiles_o,
                                                         int tiles_i) {
  constexpr int LDX = ldx(NI32), NA = 3 * NI32;
  extern __shared__ __align__(16) float smem[];
  float* dys = smem;
  float* xs = smem + kTK * kLDA;
  const int ti = blockIdx.x % tiles_i, so = blockIdx.x / tiles_i;
  const int s = so / tiles_o, o0 = (so - s * tiles_o) * kMO, i0 = ti * 32 * NI32;
  const long long u0 = (long long)s * units / S, u1 = (long long)(s + 1) * units / S;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const bool live = o0 + 32 * wv < Cout;     // (wave-uniform) a wave whose 32 rows are all beyond Cout only stages
  f32x16 acc[NA];
#pragma unroll
  for (int t = 0; t < NA; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  Staged<NI32> st;
  int b = (int)(u0 / tilesL), t = (int)(u0 - (long long)b * tilesL);          // the unit in registers
  if (u0 < u1) load_unit<NI32>(st, x, dy, b, t, o0, i0, L, Cin, Cout);
  for (long long u = u0; u < u1; ++u) {
    __syncthreads();                         // the previous unit's reads are done
    store_unit<NI32>(st, dys, xs);
    __syncthreads();
    const int rows = L - t * kTK;            // of the unit now in LDS
    if (++t == tilesL) {
      t = 0;
      ++b;
    }
    if (u + 1 < u1) load_unit<NI32>(st, x, dy, b, t, o0, i0, L, Cin, Cout);
    if (live) {
      // the k steps that hold a row of the sample, rounded up to the unroll: the rest of the image is zeros
      const int steps = rows >= kTK ? kTK / 2 : (((rows + 1) / 2 + 3) & ~3);
      const float* pa = dys + h * kLDA + 32 * wv + j;
      const float* pb = xs + h * LDX + j;
      for (int s4 = 0; s4 < steps; s4 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int row = 2 * (s4 + k);
          const float a = pa[row * kLDA];
#pragma unroll
          for (int tap = 0; tap < 3; ++tap)
#pragma unroll
            for (int ih = 0; ih < NI32; ++ih)
              acc[tap * NI32 + ih] = mfma(a, pb[(row + tap) * LDX + 32 * ih], acc[tap * NI32 + ih]);
        }
      }
    }
  }
  // register r of an accumulator is 32 consecutive input channels of two output rows: stored as it stands
  float* outb = out + (size_t)s * Cout * 3 * Cin;
  if (live) {
#pragma unroll
    for (int tap = 0; tap < 3; ++tap)
#pragma unroll
      for (int ih = 0; ih < NI32; ++ih) {
        const int i = i0 + 32 * ih + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = o0 + 32 * wv + acc_row(r, h);
          if (o < Cout && i < Cin) outb[((size_t)o * 3 + tap) * Cin + i] = acc[tap * NI32 + ih][r];
        }
      }
  }
}

// dw[e] = part[0][e] + part[1][e] + ... in ascending s; n4 float4 per partial.
__global__ __launch_bounds__(kThreads) void reduce_kernel(const float4* __restrict__ part,
                                                          float4* __restrict__ dw, int n4, int S) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= n4) return;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  // kRB loads in flight, then their adds in ascending s: a thread's chain of S dependent round trips
  // to memory (512 of them for the first layers) becomes S / kRB; the order of the adds is unchanged
  for (int s0 = 0; s0 < S; s0 += kRB) {
    float4 v[kRB];
#pragma unroll
    for (int k = 0; k < kRB; ++k) {
      const int s = s0 + k < S ? s0 + k : S - 1;
      v[k] = part[(size_t)s * n4 + e];
    }
#pragma unroll
    for (int k = 0; k < kRB; ++k)
      if (s0 + k < S) {
        a.x += v[k].x;
        a.y += v[k].y;
        a.z += v[k].z;
        a.w += v[k].w;
      }
  }
  dw[e] = a;
}

// The split count: enough blocks to fill the device twice over (a constant 512, whatever the device),
// at least two units per split, at least one split.  Nothing but the four arguments enters.
static int plan(int B, int L, int Cin, int Cout, int* splits, size_t* bytes) {
  if (!supported(Cin, Cout) || B < 0 || L < 1) return (int)hipErrorInvalidValue;
  const long long units = (long long)B * ((L + kTK - 1) / kTK);
  const int ni = Cin > 32 ? kNI : 32;
  const long long tiles = (long long)((Cout + kMO - 1) / kMO) * ((Cin + ni - 1) / ni);
  long long S = (kTargetBlocks + tiles - 1) / tiles;
  if (S > units / 2) S = units / 2;
  if (S < 1) S = 1;
  *splits = (int)S;
  *bytes = S > 1 ? (size_t)S * Cout * 3 * Cin * sizeof(float) : 0;
  return 0;
}

template <int NI32>
static int launch(hipStream_t st, const float* x, const float* dy, float* out, int B, int L, int Cin,
                  int Cout, int S) {
  static unsigned long long lds_ok = 0;
  constexpr int lds = lds_floats(NI32) * 4;
  const int tilesL = (L + kTK - 1) / kTK, tiles_o = (Cout + kMO - 1) / kMO;
  const int tiles_i = (Cin + 32 * NI32 - 1) / (32 * NI32);
  auto kern = wgrad_kernel<NI32>;
  if (hipError_t e = allow_large_lds(reinterpret_cast<const void*>(kern), &lds_ok, lds)) return (int)e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(S * tiles_o * tiles_i)), dim3(kThreads), lds, st, x, dy, out, L,
                     Cin, Cout, tilesL, (long long)B * tilesL, S, tiles_o, tiles_i);
  return (int)hipGetLastError();
}

}  // namespace conv3w
}  // namespace pcgmix

using namespace pcgmix;

extern "C" int pcgmix_conv3_wgrad_supported(int Cin, int Cout) { return conv3w::supported(Cin, Cout) ? 1 : 0; }

extern "C" int pcgmix_conv3_wgrad_tile(int which) {
  return which == 0 ? conv3w::kTK : (which == 1 ? conv3w::kMO : (which == 2 ? conv3w::kNI : 0));
}

extern "C" int pcgmix_conv3_wgrad_plan(int B, int L, int Cin, int Cout, int* splits, size_t* workspace_bytes) {
  int S = 0;
  size_t bytes = 0;
  if (int e = conv3w::plan(B, L, Cin, Cout, &S, &bytes)) return e;
  if (splits) *splits = S;
  if (workspace_bytes) *workspace_bytes = bytes;
  return 0;
}

extern "C" int pcgmix_conv3_wgrad_nlc_f32(const float* x, const float* dy, float* dw, void* workspace,
                                          size_t workspace_bytes, int B, int L, int Cin, int Cout,
                                          pcgmix_stream_t stream) {
  int S = 0;
  size_t need = 0;
  if (conv3w::plan(B, L, Cin, Cout, &S, &need) || !x || !dy || !dw) return hipErrorInvalidValue;
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
    const int e = Cin > 32 ? conv3w::launch<2>(st, x, dy, out, B, L, Cin, Cout, S)
                           : conv3w::launch<1>(st, x, dy, out, B, L, Cin, Cout, S);
    if (e || S == 1) return e;
  }
  // the partials in ascending order; an empty batch: no partial, zeros
  hipLaunchKernelGGL(conv3w::reduce_kernel, dim3((unsigned)((n4 + conv3w::kThreads - 1) / conv3w::kThreads)),
                     dim3(conv3w::kThreads), 0, st, static_cast<const float4*>(workspace),
                     reinterpret_cast<float4*>(dw), n4, B > 0 ? S : 0);
  return (int)hipGetLastError();
}
