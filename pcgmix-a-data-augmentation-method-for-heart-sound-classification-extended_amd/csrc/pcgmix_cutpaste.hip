// pcgmix_cutpaste.hip — the segment-table copy (the heart-cycle cut-and-paste family in 1D, cutmix and
// durratiocutmix on spectrograms) and durmixrespscale for gfx950 (MI355X).
//
// The reference builds these per sample in a Python loop (a clone, two to four slice copies and a
// copy into data_new, plus a host round trip for the sinusoid); here each call is ONE launch on the
// caller's stream over float32 batches:
//
//   durratiocutmix, wav-durratiocutmix                cutpaste_rows_kernel   augmentations.py:340-366,
//   labelcutmix, lengthcutmix, datasetcutmix,           (B, C, T)            :30-58, :983-1000,
//   wavcutmix  (+ '(smooth)', '(rand)', 'cutout')                            :1101-1213, :1285-1316
//   2D cutmix, durratiocutmix                         cutpaste_rows_kernel   augmentations2d.py:574-617
//                                                       (B, C, F, W) -> (B, C, F, Wo)
//   durmixrespscale                                   splice_scale_kernel    :734-775 (:289-337)
//
// cutpaste_rows_kernel: per sample a table of PCGMIX_PIECE_SEGS ordered segments along one axis — T,
// the columns of a spectrogram, or its frequency rows (the '(rand)durratiocutmix' quirk) — each the
// sample itself, its partner at a shift along that axis, or zeros.  The 1D instantiations add the
// '(smooth)' junction: over [c1-ov, c1+ov) the output is
//   float(double(own[t]) * (1 - s[j]) + double(partner[c2-ov+j]) * s[j]),  j = t - (c1-ov),
// with s = the reference's sigmoid(ov) table (computed on the host by numpy): float64 multiply,
// multiply, add, each rounded on its own, the sum rounded once to float32.  A zero segment wins over
// the window (the 'cutout' suffix is applied after the paste), the window over a copied segment.
// Partner reads at a shift are misaligned: one unaligned 16-byte load per quad, all loads of a lane
// issued before its first store, element loads only for quads that straddle a segment boundary, the
// window or the input's edge; non-temporal stores.  Every source index is range-checked in the kernel,
// whatever the tables hold: an element whose source lies outside the input is 0.
//
// splice_scale_kernel: the splice of pcgmix_mix_warp_f32 without warp (fp32 mul, mul, add,
// uncontracted; '(rand)' offsets) and the float64 row multiply of pcgmix_scale_rows_f32 applied to
// the rounded fp32 blend before the store: y = float(double(splice) * row[t]).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcgmix_kernels.h"

namespace pcgmix {
namespace {

constexpr int kThreadsC = 256;
constexpr int kUnrollC = 4;                        // quads in flight per lane (cut-and-paste)
constexpr int kEpbC = kThreadsC * 4 * kUnrollC;    // output elements per block
constexpr int kMaxOv = PCGMIX_CUTPASTE_MAX_OVERLAP;
constexpr int kBatchPerZ = 32768;                  // gridDim.y is capped at 65535: b = z * 32768 + y

typedef double double2_a __attribute__((ext_vector_type(2), aligned(16)));

// The segment table of one sample, block-uniform (SGPRs), in a form whose lookup is arithmetic only:
// the segment kinds packed two bits each, the shifts as differences between neighbours.  A chain
// of selects over the table's fields ("last segment whose lo <= p") compiles to a dynamic index
// into a private copy of the table, which the compiler places in LDS (16 KB per block and two
// ds_reads per lookup); sums of masked differences stay in registers.
struct Table {
  int lo0, lo1, lo2, lo3, lo4, end;
  int kinds;                 // 2 bits per segment: own, partner, zero (anything else in the table: zero)
  int sh0, d1, d2, d3, d4;   // shift of segment 0, then shift[k] - shift[k-1]
};
struct Piece {
  int k, src, sh;   // k: segment index, -1 before the first segment, 5 at or beyond the end
};

__device__ __forceinline__ int kind_code(int src) {
  return src == PCGMIX_PIECE_OWN ? PCGMIX_PIECE_OWN : src == PCGMIX_PIECE_PARTNER ? PCGMIX_PIECE_PARTNER
                                                                                   : PCGMIX_PIECE_ZERO;
}

__device__ __forceinline__ Table load_table(const int32_t* __restrict__ t) {
  Table P;
  P.lo0 = t[0]; P.lo1 = t[4]; P.lo2 = t[8]; P.lo3 = t[12]; P.lo4 = t[16];
  P.end = t[17];
  P.kinds = kind_code(t[2]) | kind_code(t[6]) << 2 | kind_code(t[10]) << 4 | kind_code(t[14]) << 6 |
            kind_code(t[18]) << 8;
  P.sh0 = t[3];
  P.d1 = t[7] - t[3]; P.d2 = t[11] - t[7]; P.d3 = t[15] - t[11]; P.d4 = t[19] - t[15];
  return P;
}

// Where position p falls: the last segment whose lo <= p (the segments are contiguous and ordered,
// so an empty segment is never chosen for a position inside a non-empty one); zero outside the table.
__device__ __forceinline__ Piece piece_at(const Table& P, int p) {
  const int g1 = p >= P.lo1, g2 = p >= P.lo2, g3 = p >= P.lo3, g4 = p >= P.lo4;
  // ordered lo: the comparisons are monotone, so their count is the index of the last segment reached
  const int k = g1 + g2 + g3 + g4;
  const int sh = P.sh0 + (g1 ? P.d1 : 0) + (g2 ? P.d2 : 0) + (g3 ? P.d3 : 0) + (g4 ? P.d4 : 0);
  const int src = (P.kinds >> (2 * k)) & 3;
  const bool outside = p < P.lo0 || p >= P.end;
  return Piece{p < P.lo0 ? -1 : p >= P.end ? PCGMIX_PIECE_SEGS : k, outside ? PCGMIX_PIECE_ZERO : src,
               outside ? 0 : sh};
}

__device__ __forceinline__ bool copies(const Piece& q) {
  return q.src == PCGMIX_PIECE_OWN || q.src == PCGMIX_PIECE_PARTNER;
}

struct Junction {
  int lo, n, psh, ov;   // window [lo, lo+n), partner index = t + psh, table row ov-1; n == 0: none
};

// One output element at column col of a row whose frequency index is f; ro, rm = that row in the
// sample and in its partner.  ROWS: the segments run along f (the source is q.sh rows away), else
// along col.
template <bool ROWS, bool JUNC>
__device__ __forceinline__ float piece_elem(const Table& P, const Junction& J, const double* __restrict__ sig,
                                            const float* ro, const float* rm, int f, int col, int F, int W) {
  const Piece q = piece_at(P, ROWS ? f : col);
  if (!copies(q)) return 0.f;
  if (ROWS) {
    const int sf = f + q.sh;
    if (sf < 0 || sf >= F || col >= W) return 0.f;
    return (q.src == PCGMIX_PIECE_OWN ? ro : rm)[q.sh * W + col];
  }
  if (JUNC) {
    const int j = col - J.lo;
    if ((unsigned)j < (unsigned)J.n) {
      const int sp = col + J.psh;
      if (sp < 0 || sp >= W) return 0.f;
      const double s = sig[(J.ov - 1) * 2 * kMaxOv + j];
      const double a = __dmul_rn((double)ro[col], __dsub_rn(1.0, s));
      const double b = __dmul_rn((double)rm[sp], s);
      return __double2float_rn(__dadd_rn(a, b));
    }
  }
  const int sc = col + q.sh;
  if (sc < 0 || sc >= W) return 0.f;
  return (q.src == PCGMIX_PIECE_OWN ? ro : rm)[sc];
}

// y (B, R, Wo) from x (B, R, W), R = C * F rows per sample; grid (chunks of the R*Wo output plane,
// batch as (y, z)).  The 1D family is F = 1, R = C, W = Wo = T with the junction window (JUNC); the
// 2D forms have none, and their segments run along the columns or (ROWS, Wo == W) along F.
// VEC: Wo % 4 == 0 (a quad never straddles two rows), W >= 4, y 16-byte aligned.
template <bool VEC, bool ROWS, bool JUNC>
__global__ __launch_bounds__(kThreadsC) void cutpaste_rows_kernel(
    const float* __restrict__ x, float* __restrict__ y, const int32_t* __restrict__ segs,
    const int32_t* __restrict__ mix, const int32_t* __restrict__ junc,
    const double* __restrict__ sig, int B, int R, int F, int Win, int Wo) {
  static_assert(!(ROWS && JUNC), "the junction window runs along the columns");
  // only the 2D column form changes the width: elsewhere one row pitch serves loads and stores
  const int W = (ROWS || JUNC) ? Wo : Win;
  const int b = blockIdx.z * kBatchPerZ + blockIdx.y;
  if (b >= B) return;  // block-uniform
  const Table P = load_table(segs + (size_t)b * PCGMIX_PIECE_SEGS * 4);
  Junction J{0, 0, 0, 0};
  if (JUNC && junc && sig) {
    const int c1 = junc[4 * b], c2 = junc[4 * b + 1], ov = junc[4 * b + 2];
    if (ov >= 1 && ov <= kMaxOv) J = Junction{c1 - ov, 2 * ov, c2 - c1, ov};
  }
  int m = mix[b];
  m = (m < 0 || m >= B) ? b : m;  // memory safety; the host validates as well
  const size_t in_plane = (size_t)R * W;
  const int out_plane = R * Wo;
  const float* xo = x + (size_t)b * in_plane;
  const float* xm = x + (size_t)m * in_plane;
  float* yo = y + (size_t)b * out_plane;
  const int base = (int)blockIdx.x * kEpbC;
  if (VEC) {
    // Phase 1, branch-free: one 16-byte load per quad — its source when the quad lies in one copied
    // segment, outside the window and inside the input (unaligned at a column shift), else a valid
    // address whose value is not used: the sample's own quad where the output plane is the input plane
    // (1D), its first quad otherwise (with Wo > W the output offset lies outside the input).
    // Phase 2: zeros, the element path, the store.
    float4_u v[kUnrollC];
    int mode[kUnrollC], rr[kUnrollC], cc[kUnrollC];  // mode: 0 copy, 1 zero, 2 by element, -1 none
#pragma unroll
    for (int u = 0; u < kUnrollC; ++u) {
      const int o = base + (u * kThreadsC + (int)threadIdx.x) * 4;
      const int oc = o < out_plane ? o : 0;
      const int r = oc / Wo;
      const int col = oc - r * Wo, f = ROWS ? r % F : 0;
      const Piece q0 = piece_at(P, ROWS ? f : col);
      const Piece q3 = ROWS ? q0 : piece_at(P, col + 3);
      const int sf = f + (ROWS ? q0.sh : 0);
      const int sc = col + (ROWS ? 0 : q0.sh);
      const bool one = q0.k == q3.k;
      const bool inside = sf >= 0 && (!ROWS || sf < F) && sc >= 0 && sc + 3 < W;
      const bool window = JUNC && col + 3 >= J.lo && col < J.lo + J.n;
      mode[u] = o >= out_plane ? -1 : !one ? 2 : !copies(q0) ? 1 : (window || !inside) ? 2 : 0;
      const float* p = mode[u] == 0 ? (q0.src == PCGMIX_PIECE_OWN ? xo : xm) + (r - f + sf) * W + sc
                                    : JUNC ? xo + oc : xo;
      v[u] = *reinterpret_cast<const float4_u*>(p);
      rr[u] = r;
      cc[u] = col;
    }
#pragma unroll
    for (int u = 0; u < kUnrollC; ++u) {
      if (mode[u] < 0) continue;
      const int r = rr[u], col = cc[u];
      float4_a w;
      if (mode[u] == 0) {
        w = (float4_a){v[u].x, v[u].y, v[u].z, v[u].w};
      } else if (mode[u] == 1) {
        w = (float4_a){0.f, 0.f, 0.f, 0.f};
      } else {
        const int f = ROWS ? r % F : 0;
        const float* ro = xo + r * W;
        const float* rm = xm + r * W;
        w.x = piece_elem<ROWS, JUNC>(P, J, sig, ro, rm, f, col, F, W);
        w.y = piece_elem<ROWS, JUNC>(P, J, sig, ro, rm, f, col + 1, F, W);
        w.z = piece_elem<ROWS, JUNC>(P, J, sig, ro, rm, f, col + 2, F, W);
        w.w = piece_elem<ROWS, JUNC>(P, J, sig, ro, rm, f, col + 3, F, W);
      }
      __builtin_nontemporal_store(w, reinterpret_cast<float4_a*>(yo + r * Wo + col));
    }
  } else {
    const int end = base + kEpbC < out_plane ? base + kEpbC : out_plane;
    for (int o = base + (int)threadIdx.x; o < end; o += kThreadsC) {
      const int r = o / Wo;
      yo[o] = piece_elem<ROWS, JUNC>(P, J, sig, xo + r * W, xm + r * W, ROWS ? r % F : 0, o - r * Wo, F, W);
    }
  }
}

// float(double(v) * row[t]) as numpy / torch round it (augmentations.py:773-774)
__device__ __forceinline__ float scale64(float v, double r) {
  return __double2float_rn(__dmul_rn((double)v, r));
}

// durmixrespscale.  grid (chunks of the C*T plane, B).  VEC = 4: T % 4 == 0, x, y and row 16-byte
// aligned, U quads per lane; VEC = 1: any T.
template <int VEC, int U>
__global__ __launch_bounds__(kThreadsC) void splice_scale_kernel(
    const float* __restrict__ x, float* __restrict__ y, const int32_t* __restrict__ frames,
    const int32_t* __restrict__ mix_idx, const int32_t* __restrict__ off, float lam, float oml,
    const double* __restrict__ row, int B, int C, int T) {
  const int b = blockIdx.z * kBatchPerZ + blockIdx.y;
  if (b >= B) return;  // block-uniform
  int m = mix_idx[b];
  m = (m < 0 || m >= B) ? b : m;  // memory safety; validated on the host as well
  const StateMap sm = make_state_map(frames, off, b, m, T);
  const int plane = C * T;
  const int epb = kThreadsC * VEC * U;
  const int chunk0 = (int)blockIdx.x * epb;
  const size_t own_base = (size_t)b * plane;
  const size_t par_base = (size_t)m * plane;
  if constexpr (VEC == 4) {
    // The two phases of mix_body (pcgmix_mix.hip) on the same quad_plan / quad_blend: all own, partner
    // and row loads of a lane are in flight together.
    float4_a own[U];
    float4_u par[U];
    double2_a r01[U], r23[U];
    int t0s[U], cs[U], masks[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int i = chunk0 + (q * kThreadsC + (int)threadIdx.x) * 4;
      const bool valid = i < plane;
      const int ii = valid ? i : 0;
      const int c = ii / T;
      const int t0 = ii - c * T;
      int src0;
      const int mask = (valid ? 0x100 : 0) | quad_plan(sm, t0, T, src0);
      own[q] = *reinterpret_cast<const float4_a*>(x + own_base + ii);
      // not predicated (a branch around the load would serialise a lane's loads): a quad without a
      // blended element re-reads its own quad, a line that is in flight already
      size_t poff = (mask & 0xf) ? par_base + (size_t)c * T + src0 : own_base + ii;
      asm volatile("" : "+v"(poff));  // opaque offset, as in mix_body: keeps the fallback a load of its own
      par[q] = *reinterpret_cast<const float4_u*>(x + poff);
      r01[q] = *reinterpret_cast<const double2_a*>(row + t0);
      r23[q] = *reinterpret_cast<const double2_a*>(row + t0 + 2);
      t0s[q] = t0;
      cs[q] = c;
      masks[q] = mask;
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int mask = masks[q];
      if (!(mask & 0x100)) continue;
      const int t0 = t0s[q], c = cs[q];
      const double rw[4] = {r01[q].x, r01[q].y, r23[q].x, r23[q].y};
      float out[4];
      quad_blend(out, own[q], par[q], x + par_base + (size_t)c * T, sm, t0, mask, lam, oml);
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = scale64(out[e], rw[e]);
      const float4_a v4 = {out[0], out[1], out[2], out[3]};
      const int i = chunk0 + (q * kThreadsC + (int)threadIdx.x) * 4;
      __builtin_nontemporal_store(v4, reinterpret_cast<float4_a*>(y + own_base + i));
    }
  } else {
    for (int i = chunk0 + threadIdx.x; i < chunk0 + epb && i < plane; i += kThreadsC) {
      const int c = i / T;
      const int t0 = i - c * T;
      bool hit;
      const int d = blend_shift(sm, t0, hit);
      float v = x[own_base + i];
      if (hit) v = blend(v, x[par_base + (size_t)c * T + t0 + d], lam, oml);
      y[own_base + i] = scale64(v, row[t0]);
    }
  }
}

// grid for `chunks` blocks per sample and B samples; false when it does not fit
inline bool batch_grid(long long chunks, int B, dim3* grid) {
  if (chunks <= 0 || chunks > 0x7fffffffLL || B > kBatchPerZ * 1024) return false;
  *grid = dim3((unsigned)chunks, (unsigned)(B < kBatchPerZ ? B : kBatchPerZ),
               (unsigned)((B + kBatchPerZ - 1) / kBatchPerZ));
  return true;
}

}  // namespace
}  // namespace pcgmix

using namespace pcgmix;

// Launches the segment-table kernel over y (B, R, Wo) from x (B, R, W).
template <bool ROWS, bool JUNC>
static int launch_rows(bool vec, const float* x, float* y, const int32_t* segs, const int32_t* mix,
                       const int32_t* junc, const double* sig, int B, int R, int F, int W, int Wo,
                       pcgmix_stream_t stream) {
  dim3 grid;
  if (!batch_grid(((long long)R * Wo + kEpbC - 1) / kEpbC, B, &grid)) return hipErrorInvalidValue;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((cutpaste_rows_kernel<true, ROWS, JUNC>), grid, dim3(kThreadsC), 0, s, x, y, segs, mix, junc,
                       sig, B, R, F, W, Wo);
  else
    hipLaunchKernelGGL((cutpaste_rows_kernel<false, ROWS, JUNC>), grid, dim3(kThreadsC), 0, s, x, y, segs, mix, junc,
                       sig, B, R, F, W, Wo);
  return hipGetLastError();
}

extern "C" int pcgmix_cutpaste_rows_f32(const float* x, float* y, const int32_t* segs,
                                        const int32_t* mix, const int32_t* junctions,
                                        const double* sigmoid_tab, int B, int C, int T,
                                        pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || T <= 0) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!x || !y || !segs || !mix || x == y || (junctions && !sigmoid_tab)) return hipErrorInvalidValue;
  const long long plane = (long long)C * T;
  // in-sample indices are 32-bit (one integer division per quad)
  if (plane >= (1LL << 31) - kEpbC) return hipErrorInvalidValue;
  // the input and the output may not overlap: every sample reads another sample's rows
  if (ranges_overlap(x, y, (unsigned long long)B * plane * sizeof(float))) return hipErrorInvalidValue;
  return launch_rows<false, true>(T % 4 == 0 && aligned16(x) && aligned16(y), x, y, segs, mix, junctions,
                                  sigmoid_tab, B, C, 1, T, T, stream);
}

extern "C" int pcgmix_piecewise_rows_f32(const float* x, float* y, const int32_t* segs,
                                         const int32_t* mix, int axis, int B, int C, int F, int W,
                                         int Wo, pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || F <= 0 || W <= 0 || Wo <= 0 || (axis != 0 && axis != 1))
    return hipErrorInvalidValue;
  if (axis == 1 && Wo != W) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!x || !y || !segs || !mix || x == y) return hipErrorInvalidValue;
  // in-sample indices are 32-bit (one integer division per quad): both planes below 2^31 - kEpbC
  if ((long long)C * F * Wo >= (1LL << 31) - kEpbC || (long long)C * F * W >= (1LL << 31))
    return hipErrorInvalidValue;
  const bool vec = Wo % 4 == 0 && W >= 4 && aligned16(y);
  return axis == 1 ? launch_rows<true, false>(vec, x, y, segs, mix, nullptr, nullptr, B, C * F, F, W, Wo, stream)
                   : launch_rows<false, false>(vec, x, y, segs, mix, nullptr, nullptr, B, C * F, F, W, Wo, stream);
}

extern "C" int pcgmix_mix_scale_f32(const float* x, float* y, const int32_t* frames,
                                    const int32_t* mix_idx, const int32_t* off, float lam,
                                    const double* row, int B, int C, int T, pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || T <= 0) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!x || !y || !frames || !mix_idx || !row || x == y) return hipErrorInvalidValue;
  const long long plane = (long long)C * T;
  if (plane >= (1LL << 31) - kThreadsC * 8) return hipErrorInvalidValue;
  if (ranges_overlap(x, y, (unsigned long long)B * plane * sizeof(float))) return hipErrorInvalidValue;
  const float oml = 1.0f - lam;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool vec = T % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(row);
  const int U = vec && plane >= 8192 ? 2 : 1;       // as the splice chooses its block (no warp)
  const int epb = kThreadsC * (vec ? 4 : 1) * U;
  dim3 grid;
  if (!batch_grid((plane + epb - 1) / epb, B, &grid)) return hipErrorInvalidValue;
  if (!vec)
    hipLaunchKernelGGL((splice_scale_kernel<1, 1>), grid, dim3(kThreadsC), 0, s, x, y, frames, mix_idx, off, lam,
                       oml, row, B, C, T);
  else if (U == 2)
    hipLaunchKernelGGL((splice_scale_kernel<4, 2>), grid, dim3(kThreadsC), 0, s, x, y, frames, mix_idx, off, lam,
                       oml, row, B, C, T);
  else
    hipLaunchKernelGGL((splice_scale_kernel<4, 1>), grid, dim3(kThreadsC), 0, s, x, y, frames, mix_idx, off, lam,
                       oml, row, B, C, T);
  return hipGetLastError();
}
