// pcgmix_skinny.hip — split-K linear layer with a skinny output (the Potes `dimreduc`, gfx950).
//
//   skinny_linear_partial_kernel  per-K-chunk partial products on the f32 matrix cores, with the
//                                 head's first dropout applied on the way in on request
//   skinny_linear_reduce_kernel   fixed-order sum of the partials plus bias
// launch_skinny_partial is shared with the fused classifier head (pcgmix_head.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcgmix_kernels.h"

namespace pcgmix {

typedef float f4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------- dimreduc
// z[B][O] = h[B][K] . W[O][K]^T + bias for a SKINNY output (O <= 32; the Potes head is 19968 -> 20,
// models.py:376).  hipBLASLt runs this shape as 32 workgroups with no split-K: 53 us at bs=256
// for a 20 MB read.  The first version here (VALU dot products against an LDS copy of W, 16 rows x
// 1024 columns per block) ran 18 us, bound by ds_read_b128 of W and instruction issue.  This one
// uses the f32-input matrix instruction, v_mfma_f32_32x32x2_f32 (exact f32, same peak as the f32
// VALU but none of its issue slots and no LDS in the inner loop):
//   D[o][b] += W[o][k] * h[b][k]      A = W (rows o >= O are zero lanes), B = h^T, 32 x 32 x 2
// Block = 32 batch rows x one 512-wide K chunk, 4 waves x 128 columns.  Per 64 columns a lane
// (r = lane & 31, half = lane >> 5) takes the 32 consecutive floats h[row r][k0 + 32 half ..]
// and the same span of W[r][..] (through LDS, see the kernel); MFMA step j multiplies element
// j of both (the k index may be permuted freely inside a reduction as long as A and B agree).
// The four waves' 32x32 tiles are added in a fixed order through LDS; per-chunk partials are
// summed in a fixed order by the consumer (deterministic).
constexpr int kSkinnyMaxO = 32;
constexpr int kSkinnyRows = 32;     // batch rows per block
constexpr int kSkinnyChunk = 512;   // K elements per block (one partial per chunk)
typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kSkinnyWaves = 4;     // 128 columns per wave, in steps of 64
constexpr int kSkStep = 64;         // columns per MFMA round
constexpr int kSkStride = 68;       // LDS row stride in floats (16-byte aligned, +4 against banks)

// The matrix instruction wants lane = (row, k-half): read straight from memory that is 32-byte
// pieces of 32 rows per request (14.5 us).  So each wave loads its 32 x 64 tile of h and O x 64
// tile of W row-contiguously (4 rows x 256 B per request), parks them in LDS and reads them back
// in operand order; the next step's global loads are in flight while the MFMAs run.
// MASK: h is the feature matrix BEFORE Dropout(p1); the dropout is applied while the tile is
// parked in LDS: element e = b*K + k owns `bits` (1, 2, 4 or 8) consecutive random bits of `mask`
// (bit offset e*bits), kept iff their value >= thr, kept values times `scale`.  Spares the
// separate dropout pass (a 20 MB write and re-read at bs=256).
// BITS: 0 = the mask's bits per element is the run-time argument; 2 = compile-time (Dropout(.25),
// the reference's value: constant shifts and masks in the decode).
template <int O, bool MASK, int BITS = 0>
__global__ __launch_bounds__(kSkinnyWaves * 64) void skinny_linear_partial_kernel(
    const float* __restrict__ h, const float* __restrict__ W, float* __restrict__ partial, int B,
    int K, const uint8_t* __restrict__ mask, float scale, int thr, int bits_rt) {
  const int bits = BITS ? BITS : bits_rt;
  constexpr int kWRows = (O + 3) / 4 * 4;                                // W tile rows in LDS
  constexpr int kWaveFloats = (32 + kWRows) * kSkStride;
  __shared__ __align__(16) float smem[kSkinnyWaves * kWaveFloats];
  constexpr int kPerWave = kSkinnyChunk / kSkinnyWaves;                  // 128 columns
  constexpr int kSteps = kPerWave / kSkStep;                             // 2
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, half = lane >> 5;
  const int row_base = blockIdx.x * kSkinnyRows, ks = blockIdx.y;
  const int k_w = ks * kSkinnyChunk + wave * kPerWave;
  float* xs = smem + wave * kWaveFloats;            // [32][kSkStride]
  float* ws = xs + 32 * kSkStride;                  // [kWRows][kSkStride]
  // loader mapping: request `it` covers rows 4 it + (lane >> 4), float4 column lane & 15
  const int lr = lane >> 4, lc = 4 * (lane & 15);
  f4 gx[8], gw[kWRows / 4];
  uint32_t gm[8];
  auto fetch = [&](int step) {
    const int k = k_w + kSkStep * step + lc;
    const bool ok = k < K;                          // K % 4 == 0: a float4 is inside or outside
    const f4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int row = row_base + 4 * it + lr;
      const size_t e = (size_t)(row < B ? row : B - 1) * K + (ok ? k : 0);
      const f4 v = *reinterpret_cast<const f4*>(h + e);
      gx[it] = ok ? v : z4;
      if (MASK) {     // the 4*bits random bits of this float4 (e % 4 == 0: byte- or word-aligned)
        const size_t bit = e * (size_t)bits;
        gm[it] = bits == 8   ? *reinterpret_cast<const uint32_t*>(mask + e)
                 : bits == 4 ? (uint32_t)*reinterpret_cast<const uint16_t*>(mask + (bit >> 3))
                             : (uint32_t)mask[bit >> 3] >> (bit & 7);
      }
    }
#pragma unroll
    for (int it = 0; it < kWRows / 4; ++it) {
      const int o = 4 * it + lr;
      const f4 v = *reinterpret_cast<const f4*>(W + (size_t)(o < O ? o : 0) * K + (ok ? k : 0));
      gw[it] = (ok && o < O) ? v : z4;
    }
  };
  fetch(0);
  f16v acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 1
  for (int step = 0; step < kSteps; ++step) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      f4 v = gx[it];
      if (MASK) {
        const uint32_t m = gm[it], fm = (1u << bits) - 1u;
        v.x = (int)(m & fm) >= thr ? v.x * scale : 0.f;
        v.y = (int)((m >> bits) & fm) >= thr ? v.y * scale : 0.f;
        v.z = (int)((m >> (2 * bits)) & fm) >= thr ? v.z * scale : 0.f;
        v.w = (int)((m >> (3 * bits)) & fm) >= thr ? v.w * scale : 0.f;
      }
      *reinterpret_cast<f4*>(xs + (4 * it + lr) * kSkStride + lc) = v;
    }
#pragma unroll
    for (int it = 0; it < kWRows / 4; ++it)
      *reinterpret_cast<f4*>(ws + (4 * it + lr) * kSkStride + lc) = gw[it];
    if (step + 1 < kSteps) fetch(step + 1);
    __syncthreads();                                // tiles complete (all waves run in step)
    f4 xa[8], wa[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      xa[q] = *reinterpret_cast<const f4*>(xs + r * kSkStride + 32 * half + 4 * q);
      const f4 z4 = {0.f, 0.f, 0.f, 0.f};
      wa[q] = r < O ? *reinterpret_cast<const f4*>(ws + (r < O ? r : 0) * kSkStride + 32 * half + 4 * q)
                    : z4;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[q].x, xa[q].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[q].y, xa[q].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[q].z, xa[q].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[q].w, xa[q].w, acc, 0, 0, 0);
    }
    __syncthreads();                                // tiles consumed before they are overwritten
  }
  // fixed-order sum of the waves' tiles (reusing the staging memory), then one partial per block
  float* red = smem;                                // [kSkinnyWaves - 1][16][64]
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) red[((wave - 1) * 16 + i) * 64 + lane] = acc[i];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 0; w < kSkinnyWaves - 1; ++w)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += red[(w * 16 + i) * 64 + lane];
  // C/D layout: column = lane & 31 (batch row), row o = (i & 3) + 8 (i >> 2) + 4 half
  const int row = row_base + r;
  if (row < B) {
    float* dst = partial + ((size_t)ks * B + row) * O;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = (i & 3) + 8 * (i >> 2) + 4 * half;
      if (o < O) dst[o] = acc[i];
    }
  }
}

__global__ void skinny_linear_reduce_kernel(const float* __restrict__ partial,
                                            const float* __restrict__ bias, float* __restrict__ z,
                                            int B, int O, int KS) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * O) return;
  float v = bias ? bias[i % O] : 0.f;
  for (int ks = 0; ks < KS; ++ks) v += partial[(size_t)ks * B * O + i];
  z[i] = v;
}

}  // namespace pcgmix

extern "C" int pcgmix_skinny_linear_splits(int B, int K) {
  if (B <= 0 || K <= 0) return 0;
  return (K + pcgmix::kSkinnyChunk - 1) / pcgmix::kSkinnyChunk;   // one partial per K chunk
}

namespace pcgmix {
// Launch the split-K partial products of z = h W^T (shared with the fused head, pcgmix_head.hip).
hipError_t launch_skinny_partial(const float* h, const float* W, float* partial, int B, int K,
                                 int O, hipStream_t s, const uint8_t* mask, float scale, int thr,
                                 int bits) {
  if (!h || !W || !partial || B <= 0 || K <= 0 || (K & 3) || O <= 0 || O > kSkinnyMaxO)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(W)) & 15)
    return hipErrorInvalidValue;
  if (mask && ((reinterpret_cast<uintptr_t>(mask) & 3) ||
               (bits != 1 && bits != 2 && bits != 4 && bits != 8)))
    return hipErrorInvalidValue;
  const int KS = pcgmix_skinny_linear_splits(B, K);
  dim3 grid((unsigned)((B + kSkinnyRows - 1) / kSkinnyRows), (unsigned)KS),
      block(kSkinnyWaves * 64);
  if (O == 20 && mask && bits == 2) {
    hipLaunchKernelGGL((skinny_linear_partial_kernel<20, true, 2>), grid, block, 0, s, h, W, partial, B,
                       K, mask, scale, thr, bits);
  } else if (O == 20 && mask) {
    hipLaunchKernelGGL((skinny_linear_partial_kernel<20, true>), grid, block, 0, s, h, W, partial, B, K,
                       mask, scale, thr, bits);
  } else if (mask) {
    return hipErrorInvalidValue;                      // the masked variant exists for the Potes head
  } else if (O == 20) {
    hipLaunchKernelGGL((skinny_linear_partial_kernel<20, false>), grid, block, 0, s, h, W, partial, B,
                       K, nullptr, 1.f, 0, 8);
  } else if (O == 8) {
    hipLaunchKernelGGL((skinny_linear_partial_kernel<8, false>), grid, block, 0, s, h, W, partial, B,
                       K, nullptr, 1.f, 0, 8);
  } else if (O == 16) {
    hipLaunchKernelGGL((skinny_linear_partial_kernel<16, false>), grid, block, 0, s, h, W, partial, B,
                       K, nullptr, 1.f, 0, 8);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
}  // namespace pcgmix

extern "C" int pcgmix_skinny_linear_fwd_f32(const float* h, const float* W, const float* bias,
                                            float* partial, float* z, int B, int K, int O,
                                            pcgmix_stream_t stream) {
  using namespace pcgmix;
  if (!z) return hipErrorInvalidValue;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const hipError_t e = launch_skinny_partial(h, W, partial, B, K, O, s, nullptr, 1.f, 0, 8);
  if (e != hipSuccess) return (int)e;
  const int KS = pcgmix_skinny_linear_splits(B, K);
  const int n = B * O;
  hipLaunchKernelGGL(skinny_linear_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     partial, bias, z, B, O, KS);
  return (int)hipGetLastError();
}
