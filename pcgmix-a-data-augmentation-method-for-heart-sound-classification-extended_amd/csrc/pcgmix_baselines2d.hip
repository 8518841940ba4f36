// pcgmix_baselines2d.hip — the paper's spectrogram comparison augmentations for gfx950 (MI355X).
//
// The reference runs them through the 2D augment() (augmentations2d.py:461-617); here each is one
// launch on the caller's stream, on (B, C, F, W) float32 batches:
//
//   timemask, freqmask      zero_rects_kernel       x[b, :, f0:f1, t0:t1] = 0           in place
//   cutmix, durratiocutmix  piecewise_rows_kernel   y[b] = own / partner / zero pieces
//   mixup, latentmixup      blend_rows_kernel (pcgmix_baselines.hip) on the flat sample planes
//
// The rectangle kernel touches only the zeroed elements.  The piecewise copy is driven by a
// per-sample table of PCGMIX_PIECE_SEGS segments along one axis (columns, or frequency rows for
// the '(rand)durratiocutmix' quirk); a segment is the sample itself, its partner at a shift along
// that axis, or zeros.  Partner reads at a column shift are misaligned: one unaligned 16-byte load
// per quad, all of a lane's loads issued before its first store (as the splice kernel does,
// DESIGN.md §3.1), element loads only for the quads that straddle two segments.  Every source index is range-checked in the kernel, whatever the table
// holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcgmix_kernels.h"

namespace pcgmix {
namespace {

constexpr int kThreads2 = 256;
constexpr int kUnroll2 = 4;                        // quads in flight per lane
constexpr int kEpb2 = kThreads2 * 4 * kUnroll2;    // output elements per block
constexpr int kZeroChunk = kThreads2 * 4;          // rectangle elements per block
constexpr int kSegs = PCGMIX_PIECE_SEGS;

typedef float float4_a __attribute__((ext_vector_type(4), aligned(16)));
typedef float float4_u __attribute__((ext_vector_type(4), aligned(4)));

// timemask / freqmask (and any per-sample rectangle): rect (B, 4) = [f0, f1, t0, t1), applied to
// every channel, clipped to the plane here as well.  grid (B*C, chunks of the largest rectangle).
__global__ __launch_bounds__(kThreads2) void zero_rects_kernel(float* __restrict__ x,
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
  for (int i = lo + (int)threadIdx.x; i < hi; i += kThreads2) {
    const int r = i / w, c = i - r * w;
    xp[r * W + c] = 0.f;
  }
}

struct Pieces {
  int lo[kSegs], src[kSegs], sh[kSegs];
  int end;  // hi of the last segment: positions at or beyond it are zero
};

// Where position p falls: k = the last segment whose lo <= p (the segments are contiguous and
// ordered, so an empty segment is never chosen for a position inside a non-empty one), -1 before
// the first segment, kSegs at or beyond the end.  Two positions with the same k and every position
// between them lie in one segment.  Selects over constant indices only: the table stays in registers.
struct Piece {
  int k, src, sh;
};

__device__ inline Piece piece_at(const Pieces& P, int p) {
  Piece q{0, P.src[0], P.sh[0]};
#pragma unroll
  for (int j = 1; j < kSegs; ++j)
    if (p >= P.lo[j]) q = Piece{j, P.src[j], P.sh[j]};
  if (p < P.lo[0]) q = Piece{-1, PCGMIX_PIECE_ZERO, 0};
  if (p >= P.end) q = Piece{kSegs, PCGMIX_PIECE_ZERO, 0};
  return q;
}

__device__ inline bool copies(const Piece& q) {
  return q.src == PCGMIX_PIECE_OWN || q.src == PCGMIX_PIECE_PARTNER;
}

// One output element (row r of the (C*F) source rows, frequency f, column col).
template <bool ROWS>
__device__ inline float piece_elem(const Pieces& P, const float* xo, const float* xm, int r,
                                   int f, int col, int F, int W) {
  const Piece q = piece_at(P, ROWS ? f : col);
  if (!copies(q)) return 0.f;
  const float* s = q.src == PCGMIX_PIECE_OWN ? xo : xm;
  if (ROWS) {
    const int sf = f + q.sh;
    if (sf < 0 || sf >= F || col >= W) return 0.f;
    return s[(r - f + sf) * W + col];
  }
  const int sc = col + q.sh;
  if (sc < 0 || sc >= W) return 0.f;
  return s[r * W + sc];
}

// cutmix / durratiocutmix: y (B, C, F, Wo) from x (B, C, F, W).  ROWS: the segments run along F
// (Wo == W), otherwise along the columns.  grid (chunks of the C*F*Wo output plane, B).
template <bool VEC, bool ROWS>
__global__ __launch_bounds__(kThreads2) void piecewise_rows_kernel(
    const float* __restrict__ x, float* __restrict__ y, const int32_t* __restrict__ segs,
    const int32_t* __restrict__ mix, int B, int C, int F, int W, int Wo) {
  const int b = blockIdx.y;
  Pieces P;
  const int32_t* t = segs + (size_t)b * kSegs * 4;
#pragma unroll
  for (int j = 0; j < kSegs; ++j) {
    P.lo[j] = t[4 * j];
    P.src[j] = t[4 * j + 2];
    P.sh[j] = t[4 * j + 3];
  }
  P.end = t[4 * (kSegs - 1) + 1];
  int m = mix[b];
  m = (m < 0 || m >= B) ? b : m;  // memory safety; the host validates as well
  const size_t in_plane = (size_t)C * F * W;
  const int out_plane = C * F * Wo;
  const float* xo = x + (size_t)b * in_plane;
  const float* xm = x + (size_t)m * in_plane;
  float* yo = y + (size_t)b * out_plane;
  const int base = (int)blockIdx.x * kEpb2;
  if (VEC) {  // Wo % 4 == 0 (a quad never straddles two rows) and W >= 4
    // Phase 1, branch-free: one 16-byte load per quad — its source when the quad lies in one copied
    // segment and inside the input (unaligned at a column shift), else the sample's first quad (a
    // valid address whose value is not used).  Phase 2: zeros, element loads for a quad across a
    // segment boundary or the input's edge, and the store.
    float4_u v[kUnroll2];
    int mode[kUnroll2], rr[kUnroll2], cc[kUnroll2];  // mode: 0 copy, 1 zero, 2 by element, -1 none
#pragma unroll
    for (int u = 0; u < kUnroll2; ++u) {
      const int o = base + (u * kThreads2 + (int)threadIdx.x) * 4;
      const int oc = o < out_plane ? o : 0;
      const int r = oc / Wo;
      const int col = oc - r * Wo, f = r % F;
      const Piece q0 = piece_at(P, ROWS ? f : col);
      const Piece q3 = ROWS ? q0 : piece_at(P, col + 3);
      const int sf = ROWS ? f + q0.sh : f;
      const int sc = ROWS ? col : col + q0.sh;
      const bool one = q0.k == q3.k;
      const bool inside = sf >= 0 && sf < F && sc >= 0 && sc + 3 < W;
      mode[u] = o >= out_plane ? -1 : !one ? 2 : !copies(q0) ? 1 : inside ? 0 : 2;
      const float* p = mode[u] == 0 ? (q0.src == PCGMIX_PIECE_OWN ? xo : xm) + (r - f + sf) * W + sc : xo;
      v[u] = *reinterpret_cast<const float4_u*>(p);
      rr[u] = r;
      cc[u] = col;
    }
#pragma unroll
    for (int u = 0; u < kUnroll2; ++u) {
      if (mode[u] < 0) continue;
      const int r = rr[u], col = cc[u], f = r % F;
      float4_a w;
      if (mode[u] == 0) {
        w = (float4_a){v[u].x, v[u].y, v[u].z, v[u].w};
      } else if (mode[u] == 1) {
        w = (float4_a){0.f, 0.f, 0.f, 0.f};
      } else {
        w.x = piece_elem<ROWS>(P, xo, xm, r, f, col, F, W);
        w.y = piece_elem<ROWS>(P, xo, xm, r, f, col + 1, F, W);
        w.z = piece_elem<ROWS>(P, xo, xm, r, f, col + 2, F, W);
        w.w = piece_elem<ROWS>(P, xo, xm, r, f, col + 3, F, W);
      }
      __builtin_nontemporal_store(w, reinterpret_cast<float4_a*>(yo + r * Wo + col));
    }
  } else {
    const int end = base + kEpb2 < out_plane ? base + kEpb2 : out_plane;
    for (int o = base + (int)threadIdx.x; o < end; o += kThreads2) {
      const int r = o / Wo;
      const int col = o - r * Wo, f = r % F;
      yo[o] = piece_elem<ROWS>(P, xo, xm, r, f, col, F, W);
    }
  }
}

inline bool aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace
}  // namespace pcgmix

using namespace pcgmix;

extern "C" int pcgmix_zero_rects_f32(float* x, const int32_t* rect, int B, int C, int F, int W,
                                     int max_area, pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || F <= 0 || W <= 0 || max_area < 0) return hipErrorInvalidValue;
  if (B == 0 || max_area == 0) return hipSuccess;
  if (!x || !rect) return hipErrorInvalidValue;
  const long long planes = (long long)B * C;
  if ((long long)F * W >= (1LL << 31)) return hipErrorInvalidValue;
  const long long area = (long long)F * W < max_area ? (long long)F * W : max_area;
  const long long chunks = (area + kZeroChunk - 1) / kZeroChunk;
  if (planes * kThreads2 >= (1LL << 32) || chunks > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zero_rects_kernel, dim3((unsigned)planes, (unsigned)chunks), dim3(kThreads2), 0,
                     reinterpret_cast<hipStream_t>(stream), x, rect, C, F, W);
  return hipGetLastError();
}

extern "C" int pcgmix_piecewise_rows_f32(const float* x, float* y, const int32_t* segs,
                                         const int32_t* mix, int axis, int B, int C, int F, int W,
                                         int Wo, pcgmix_stream_t stream) {
  if (B < 0 || C <= 0 || F <= 0 || W <= 0 || Wo <= 0 || (axis != 0 && axis != 1))
    return hipErrorInvalidValue;
  if (axis == 1 && Wo != W) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  if (!x || !y || !segs || !mix || x == y || B > 65535) return hipErrorInvalidValue;
  const long long out_plane = (long long)C * F * Wo;
  // in-sample indices are 32-bit (one integer division per quad): both planes below 2^31 - kEpb2
  if (out_plane >= (1LL << 31) - kEpb2 || (long long)C * F * W >= (1LL << 31)) return hipErrorInvalidValue;
  const long long chunks = (out_plane + kEpb2 - 1) / kEpb2;
  const dim3 grid((unsigned)chunks, (unsigned)B);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool vec = Wo % 4 == 0 && W >= 4 && aligned16(y);
  if (axis == 1) {
    if (vec)
      hipLaunchKernelGGL((piecewise_rows_kernel<true, true>), grid, dim3(kThreads2), 0, s, x, y, segs, mix, B, C, F, W, Wo);
    else
      hipLaunchKernelGGL((piecewise_rows_kernel<false, true>), grid, dim3(kThreads2), 0, s, x, y, segs, mix, B, C, F, W, Wo);
  } else {
    if (vec)
      hipLaunchKernelGGL((piecewise_rows_kernel<true, false>), grid, dim3(kThreads2), 0, s, x, y, segs, mix, B, C, F, W, Wo);
    else
      hipLaunchKernelGGL((piecewise_rows_kernel<false, false>), grid, dim3(kThreads2), 0, s, x, y, segs, mix, B, C, F, W, Wo);
  }
  return hipGetLastError();
}
