// Internal header shared by the kernel translation units of libpcgmix_hip.so.
#ifndef PCGMIX_KERNELS_H
#define PCGMIX_KERNELS_H
#include <hip/hip_runtime.h>

#include "pcgmix_hip.h"   // public C ABI (include/)

namespace pcgmix {

inline bool aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

// true when the byte ranges [a, a + bytes) and [b, b + bytes) intersect
inline bool ranges_overlap(const void* a, const void* b, unsigned long long bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + bytes && pb < pa + bytes;
}

// Large dynamic-LDS opt-in is a per-device property of the kernel: raise it once per
// (kernel, device) — `done` is a bitmask indexed by the current device (<= 64 devices).
inline hipError_t allow_large_lds(const void* kernel, unsigned long long* done, int bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = 1ull << (dev & 63);
  if (*done & bit) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) *done |= bit;
  return e;
}

// pcgmix_skinny.hip: split-K partial products of the skinny linear layer (see there).
// mask != nullptr: h holds the features before dropout; element e owns `bits` random bits of mask
// (bit offset e*bits), kept iff their value >= thr, times scale.
hipError_t launch_skinny_partial(const float* h, const float* W, float* partial, int B, int K,
                                 int O, hipStream_t s, const uint8_t* mask, float scale, int thr,
                                 int bits);

// pcgmix_mix.hip: pcgmix_mix_warp_f32 plus an optional payload of pay_n16 16-byte words that
// block (0,0,0) copies from pay_src to pay_dst (both 16-byte aligned device addresses).
// disp_part != nullptr: the per-state offsets are not read from `off` but reduced by every block
// from the displacement search's per-block results (kDispSplit float2 {value, displacement bits}
// per (sample, state); pcgmix_saliency.hip) — the search's own finalize launch is then not needed.
constexpr int kDispSplit = 4;
int launch_mix_warp(const float* x, float* y, const int32_t* frames, const int32_t* mix_idx,
                    const int32_t* off, float lam, const double* knots, const double* spline_op,
                    int n_knots, const int32_t* zero_rect, int B, int C, int T, hipStream_t s,
                    const void* pay_src, void* pay_dst, int pay_n16,
                    const float2* disp_part = nullptr, const int16_t* partners16 = nullptr);

// pcgmix_mix.hip: the plain splice (no offsets, no warp, no rectangle) with its index block in
// the kernel ARGUMENTS instead of device memory: frames (B,5) and partners (B) as int16 in host
// memory, B <= kPackB, T <= 32767, T % 4 == 0, x and y 16-byte aligned.  Returns
// hipErrorInvalidValue when the shape does not qualify (the caller then takes the copy path).
constexpr int kPackB = 256;
constexpr int kPackPayBytes = 320;   // step payload that still fits next to the index block
// Partner indices of up to kPackB samples as int16, two per dword, passed BY VALUE in the kernel
// arguments of the displacement search and of the splice (saliency-guided step: the partners are
// the only per-step index data that depends on the labels — carried by the launches themselves,
// they need no host-to-device copy).  n == 0: not in use, the kernels read mix_idx from memory.
struct PartnerPack {
  int32_t w[kPackB / 2];
  int n;
};
__device__ __forceinline__ int partner_get(const PartnerPack& p, int b) {
  const int w = p.w[b >> 1];
  return (b & 1) ? (w >> 16) : ((int)((unsigned)w << 16) >> 16);
}
inline PartnerPack make_partner_pack(const int16_t* partners16, int B) {
  PartnerPack pk;
  pk.n = 0;
  if (partners16 && B > 0 && B <= kPackB) {
    int16_t* p16 = reinterpret_cast<int16_t*>(pk.w);
    for (int b = 0; b < B; ++b) p16[b] = partners16[b];
    pk.n = B;
  }
  return pk;
}
// pay: up to kPackPayBytes bytes (host) that also travel in the arguments; block (0,0) writes them,
// rounded up to 16, to pay_dst (device, 16-byte aligned) — the step payload of pcgmix_ctx_set_payload.
int launch_mix_karg(const float* x, float* y, const int16_t* frames16, const int16_t* mix16, float lam,
                    int B, int C, int T, hipStream_t s, const void* pay = nullptr, int pay_bytes = 0,
                    void* pay_dst = nullptr);

// The plain splice launched BEFORE its index block exists ("armed"): a strict-signature step is the
// chain  previous splice -> label arg-max -> host (labels -> partners) -> splice,  and with two
// launches the host's reaction includes a launch (3 us) and the time the command processor takes to
// start it (3-4 us).  Armed, ONE kernel is enqueued at the start of the call: its block (0,0) does
// the label arg-max (labels under the step's token to host-mapped memory), then wave 0 of every block
// polls its sample's 64-byte RECORD in host-mapped memory until the host has written it and hands it to
// the block's other waves through LDS (plain kernel: one wide block per sample slice, no block waits for
// another).  The splice + warp kernel still has every sample's first block relay the record through
// device memory (rec_d) to the sample's other blocks.
// A record is six 8-byte words, each = (stamp << 32) | two int16 values; the stamp is the step's
// sequence number, so a word is valid by itself (8-byte aligned loads and stores are single-copy
// atomic on both sides): no flag, no ordering between words, no torn record.  Values: own
// boundaries f[0..4], partner index, the partner's boundaries f[0..4], 0; word 6 = the step's lambda
// (float bits) for the plain launch, which may be made before lambda is drawn.
// stamp | kArmedAbort in a record = "give up": written by the host (bad input after the launch) or
// by a relay that saw nothing within timeout_ticks of the 100 MHz clock (then also *abort_h = seq);
// every wave leaves `y` partly written (the plain kernel has stored the elements that do not depend on the
// record by then, see EdgePack; the splice + warp kernel has stored nothing).
constexpr uint32_t kArmedAbort = 0x80000000u;
constexpr int kArmedRecWords = 8;            // 64 bytes per sample: six index words, lambda, (device) knots-ready
struct ArmedArgs {
  const int64_t* ohe;                        // (B, K) one-hot on the device
  int K;
  unsigned long long* lab64;                 // host-mapped: 64 words = (token << 32) | labels of rows 4l .. 4l+3,
  uint32_t token;                            //   one byte each (K <= 256)
  const unsigned long long* rec_h;           // host-mapped records (kPackB x kArmedRecWords)
  unsigned long long* rec_d;                 // device relay of the same shape
  uint32_t* abort_h;                         // host-mapped
  uint32_t seq;                              // 1 .. 0x7fffffff
  unsigned long long timeout_ticks;
};
// Own cycle [lo, hi) = [frames[b,0], frames[b,4]) of every sample as two int16 in one dword (lo | hi << 16),
// BY VALUE in the plain armed kernel's arguments: known on the host when the kernel is launched, and all the
// kernel needs to tell which output elements are plain copies of the own row whatever partner is drawn (the
// blended ranges lie inside the own cycle).  Those are loaded and stored BEFORE the wait for the record;
// the own values of the others are loaded before it and kept.  n == 0: edges unknown, every element waits.
struct EdgePack {
  uint32_t w[kPackB];
  int n;
};
// Own quads a lane of the plain armed kernel holds in registers across the wait (24 VGPRs): three chunks of
// two quads, which is a whole (4, 5000) sample in one block of kArmedThreads lanes.
constexpr int kArmedHold = 6;
constexpr int kArmedThreads = 1024;
// frames_host: the (B,5) int64 boundaries on the host, or nullptr (no early phase).  A sample whose
// edges are not 0 <= lo <= hi <= T gets [0, T): nothing of it is stored early.  edges_out (kPackB words):
// the dwords the kernel got, for the caller to hold the records against.
int launch_mix_armed(const float* x, float* y, const ArmedArgs& a, int B, int C, int T, hipStream_t s,
                     const void* pay = nullptr, int pay_bytes = 0, void* pay_dst = nullptr,
                     const int64_t* frames_host = nullptr, uint32_t* edges_out = nullptr);
// The same for the splice + warp kernel (durmixmagwarp): knots_host = this step's knots (B, n_knots, C)
// float64 in device-readable pinned memory, knots_dev = device scratch of the same size (each sample's
// relay copies its knots there once), spline_op the constant operator on the device.
int mix_tq_armed_ok(int B, int C, int T, int n_knots);
int launch_mix_tq_armed(const float* x, float* y, const ArmedArgs& a, float lam, const double* knots_host,
                        double* knots_dev, const double* spline_op, int n_knots, int B, int C, int T, hipStream_t s,
                        const void* pay = nullptr, int pay_bytes = 0, void* pay_dst = nullptr);
// first maximum of row b of a (B, K) int64 one-hot matrix (torch.max / np.argmax, augmentations.py:501)
__device__ __forceinline__ int onehot_argmax(const int64_t* __restrict__ ohe, int K, int b) {
  const int64_t* row = ohe + (size_t)b * K;
  if (K == 2 && !(reinterpret_cast<uintptr_t>(ohe) & 15)) {
    // two classes (the reference's data sets): the row is ONE 16-byte load; the loop below is a load,
    // a wait and a compare per class — two memory round trips in the kernel the host waits for
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    const ll2 v = *reinterpret_cast<const ll2*>(row);
    return v.y > v.x ? 1 : 0;
  }
  int best = 0;
  int64_t bv = row[0];
  for (int c = 1; c < K; ++c) {
    const int64_t v = row[c];
    if (v > bv) { bv = v; best = c; }
  }
  return best;
}

// Labels of rows r0 .. r0+3 (rows >= B read row B-1 and report 0) packed one byte each.  For two classes
// the four 16-byte rows are loaded FIRST and compared afterwards: four calls of onehot_argmax compile to
// load, wait, compare four times over — four memory round trips in front of the word the host waits for.
__device__ __forceinline__ uint32_t onehot_argmax4(const int64_t* __restrict__ ohe, int K, int r0, int B) {
  uint32_t packed = 0;
  if (K == 2 && !(reinterpret_cast<uintptr_t>(ohe) & 15)) {
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    ll2 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = r0 + j < B ? r0 + j : B - 1;
      v[j] = *reinterpret_cast<const ll2*>(ohe + (size_t)r * 2);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) packed |= (uint32_t)((r0 + j < B && v[j].y > v[j].x) ? 1 : 0) << (8 * j);
    return packed;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = r0 + j;
    const int best = onehot_argmax(ohe, K, r < B ? r : B - 1);
    packed |= (uint32_t)(r < B ? best & 0xff : 0) << (8 * j);
  }
  return packed;
}

// ---- device code shared by the streaming kernels (pcgmix_mix.hip, pcgmix_cutpaste.hip, pcgmix_baselines.hip)
// 16-byte vector whose address is only known to be 4-byte aligned (partner rows are read at
// an arbitrary sample offset); gfx950 global loads handle the misalignment in hardware.
typedef float float4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef float float4_a __attribute__((ext_vector_type(4), aligned(16)));

struct StateMap {
  int a[4];      // own-side start of the blended range of state k
  int n[4];      // its length (0 = nothing to blend)
  int delta[4];  // partner index = own index + delta
};

// Boundaries of sample b and its partner -> blended ranges.  All inputs are block-uniform.
__device__ __forceinline__ StateMap make_state_map(const int32_t* __restrict__ frames,
                                                   const int32_t* __restrict__ off, int b, int m,
                                                   int T, const float2* __restrict__ part = nullptr) {
  StateMap sm;
  int f1[5], f2[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    f1[k] = frames[b * 5 + k];
    f2[k] = frames[m * 5 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int len1 = f1[k + 1] - f1[k];
    int len2 = f2[k + 1] - f2[k];
    int gap = len2 - len1;
    int agap = gap < 0 ? -gap : gap;
    int o = off ? off[b * 4 + k] : 0;
    if (part) {  // salopt_finalize_kernel's rule: greatest value, smallest displacement on ties
      float bv = -INFINITY;
      int bd = 0x7fffffff;
#pragma unroll
      for (int z = 0; z < kDispSplit; ++z) {
        const float2 p = part[((size_t)b * 4 + k) * kDispSplit + z];
        const int dd = __float_as_int(p.y);
        if (p.x > bv || (p.x == bv && dd < bd)) {
          bv = p.x;
          bd = dd;
        }
      }
      o = bd == 0x7fffffff ? 0 : bd;
    }
    o = o < 0 ? 0 : (o > agap ? agap : o);
    int a = f1[k] + (gap < 0 ? o : 0);
    int s = f2[k] + (gap > 0 ? o : 0);
    int n = len1 < len2 ? len1 : len2;
    // never blend outside the row on either side (malformed frames are rejected on the host;
    // this keeps the kernel memory-safe regardless)
    if (a < 0 || s < 0) n = 0;
    if (n > T - a) n = T - a;
    if (n > T - s) n = T - s;
    if (n < 0) n = 0;
    sm.a[k] = a;
    sm.n[k] = n;
    sm.delta[k] = s - a;
  }
  return sm;
}

// Returns the partner-minus-own index shift for sample position t, or INT_MIN if t is not
// inside a blended range.
__device__ __forceinline__ int blend_shift(const StateMap& sm, int t, bool& hit) {
  int d = 0;
  hit = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    bool in = (unsigned)(t - sm.a[k]) < (unsigned)sm.n[k];
    d = in ? sm.delta[k] : d;
    hit = hit || in;
  }
  return d;
}

__device__ __forceinline__ float blend(float own, float other, float lam, float oml) {
  // x*lam + partner*(1-lam) as three separately rounded fp32 ops (augmentations.py:294)
  return __fadd_rn(__fmul_rn(own, lam), __fmul_rn(other, oml));
}

// One quad of sample positions t0 .. t0+3 of a row against the blended ranges.  The partner quad is
// fetched with ONE unaligned 16-byte load at the shift of the first blended element, from src0 (clamped
// into the row).  Returned mask: bit e = element e blends; bit 4+e = element e blends with a different
// shift (a state boundary inside the quad) or the quad load had to be clamped: patched by a scalar load.
__device__ __forceinline__ int quad_plan(const StateMap& sm, int t0, int T, int& src0) {
  bool hit[4];
  int d[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = blend_shift(sm, t0 + e, hit[e]);
  const int dsel = hit[0] ? d[0] : hit[1] ? d[1] : hit[2] ? d[2] : hit[3] ? d[3] : 0;
  src0 = t0 + dsel;
  src0 = src0 < 0 ? 0 : (src0 > T - 4 ? T - 4 : src0);
  const bool clamped = src0 != t0 + dsel;
  int mask = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (hit[e]) mask |= 1 << e;
    if (hit[e] && (clamped || d[e] != dsel)) mask |= 16 << e;
  }
  return mask;
}

// The quad's four output elements from the own quad, the partner quad quad_plan asked for and its mask;
// par_row = the partner's row (x + partner base + c * T).
__device__ __forceinline__ void quad_blend(float (&out)[4], const float4_a& own, const float4_u& par,
                                           const float* __restrict__ par_row, const StateMap& sm, int t0,
                                           int mask, float lam, float oml) {
  const float o[4] = {own.x, own.y, own.z, own.w};
  const float pv[4] = {par.x, par.y, par.z, par.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = pv[e];
    if (mask & (16 << e)) {  // rare: patch with the element's own shift
      bool h;
      const int de = blend_shift(sm, t0 + e, h);
      v = par_row[t0 + e + de];
    }
    out[e] = (mask & (1 << e)) ? blend(o[e], v, lam, oml) : o[e];
  }
}

// pcgmix_saliency.hip: the displacement search of pcgmix_salopt_disp_f32; disp == nullptr leaves
// the per-block results in `workspace` for launch_mix_warp's disp_part.
// pay_*: pay_n16 16-byte words that one otherwise idle block copies from pay_src (device-readable
// host memory) to pay_dst while the search runs.
// plan != nullptr (plan->n > 0): the launch holds exactly the listed blocks, heaviest first
// (plan_salopt_blocks), instead of the full (sample, slice, state) grid.
constexpr int kDispPlanMax = 1408;   // with the PartnerPack still inside the 4 KB of kernel arguments
struct DispPlan {
  int n;                             // 0: no plan (natural grid)
  uint16_t e[kDispPlanMax];          // (sample << 4) | (state << 2) | slice
};
struct DispNoPlan { int n; };
// Host: the blocks of the search that have candidates — slice z of pair (b, k) holds the
// displacements z*256 .. z*256+255, +1024, ... — ordered by the length of their chain of sums
// (own state's length x passes), longest first, so that the dispatcher deals the long ones out
// first and evenly; a pair without a search gets its slice 0 (which marks all four slices empty).
// frames_h: (B,5) as the device copy; partners as int32 or int16 (one of them).  false: B too
// large or more blocks than the plan holds — launch without a plan.
bool plan_salopt_blocks(const int32_t* frames_h, const int32_t* mix_h, const int16_t* mix16, int B,
                        int T, int max_len, DispPlan* out);
int launch_salopt_search(const float* sal, const int32_t* frames, const int32_t* mix_idx, float lam,
                         int mode, int32_t* disp, void* workspace, int max_len, int B, int T,
                         hipStream_t s, const void* pay_src = nullptr, void* pay_dst = nullptr,
                         int pay_n16 = 0, const int16_t* partners16 = nullptr,
                         const DispPlan* plan = nullptr);

// The random bytes the Potes head's dropouts read (pcgmix_potes_stack_fwd_save_f32 and
// pcgmix_potes_narrow_fwd_f32 fill them on the side of their forward launch): 32-bit word w =
// counter_hash(w, key) — murmur3's 32-bit finaliser, keyed before and inside.
__device__ __forceinline__ uint32_t counter_hash(uint32_t i, uint32_t k0, uint32_t k1) {
  uint32_t h = i * 0x9E3779B1u + k0;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h ^= k1;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
// rnd[0 .. rnd_n16) 16-byte words, by all threads of a launch: `first` is this thread's index in
// the launch, `stride` the launch's thread count.  key != nullptr: the two key words are read from
// device memory (a captured step changes them per replay), else they are (key_lo, key_hi).
__device__ __forceinline__ void counter_hash_fill(uint4* __restrict__ rnd, long long rnd_n16,
                                                  const uint32_t* __restrict__ key, uint32_t key_lo,
                                                  uint32_t key_hi, long long first, long long stride) {
  const uint32_t k0 = key ? key[0] : key_lo, k1 = key ? key[1] : key_hi;
  for (long long i = first; i < rnd_n16; i += stride) {
    const uint32_t c = (uint32_t)i * 4u;
    rnd[i] = make_uint4(counter_hash(c, k0, k1), counter_hash(c + 1, k0, k1),
                        counter_hash(c + 2, k0, k1), counter_hash(c + 3, k0, k1));
  }
}
// Host-side check of the (rnd_out, rnd_bytes) pair of those entry points; rnd_out == NULL: no fill.
inline bool dropout_fill_args_ok(const void* rnd_out, long long rnd_bytes, int N) {
  return !rnd_out || !(rnd_bytes <= 0 || (rnd_bytes & 15) || rnd_bytes > (16ll << 30) ||
                       (reinterpret_cast<uintptr_t>(rnd_out) & 15) || N == 0);
}

// ---- evaluation (pcgmix_eval.hip, pcgmix_head.hip): the row rule of train_model.py:591-670
// One row of logits l[0..C), 1 <= C <= kEvalMaxC: the softmax the reference votes with (:602) and,
// for a label byte y < C, the row's cross entropy as potes_tail_loss_kernel forms it for a one-hot
// target (train_model.py:45-54).  m = max l; e_c = expf(l_c - m); s = sum e_c, c ascending;
// p_c = e_c / s; loss = -((l_y - m) - logf(s)) (0 without a label); the returned vote is the lowest
// index of the maximum of the float32 p — np.argmax of the softmax OUTPUT (:637), not of the logits.
constexpr int kEvalMaxC = 8;
template <typename L>
__device__ __forceinline__ int eval_row(const L& l, int C, int y, float* __restrict__ p, float& loss) {
  float m = l[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
  float e[kEvalMaxC];
  float s = 0.f, ly = 0.f;
#pragma unroll
  for (int c = 0; c < kEvalMaxC; ++c) {
    if (c < C) {
      e[c] = expf(l[c] - m);
      s += e[c];
      ly = c == y ? l[c] : ly;
    }
  }
  int vote = 0;
  float best = 0.f;
#pragma unroll
  for (int c = 0; c < kEvalMaxC; ++c) {
    if (c < C) {
      const float pc = e[c] / s;
      p[c] = pc;
      if (c == 0 || pc > best) {
        best = pc;
        vote = c;
      }
    }
  }
  loss = (y >= 0 && y < C) ? -((ly - m) - logf(s)) : 0.f;
  return vote;
}

}  // namespace pcgmix
#endif
