// The rules the Potes conv-stack translation units share (pcgmix_potes.hip, pcgmix_potes_narrow.hip;
// pcgmix_optim.hip for the gradient layout): written once so the copies cannot drift apart.
#ifndef PCGMIX_POTES_STACK_H
#define PCGMIX_POTES_STACK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcgmix {

constexpr int kPotThreads = 256;
// Gradient columns of the 8/4-channel stack, [gw1 | gb1 | gw2 | gb2] = 8*5 + 8 + 4*8*5 + 4: the
// row length of its per-block partials and the grid of their reduce.
constexpr int kNGrad = 212;

// Geometry of Conv1d(k5, pad1) + MaxPool1d(2), twice, on rows of T samples — the same for every
// width of the ladder.
struct PotesDims {
  int T, P1, P2;       // first- and second-layer pooled lengths
  // bytes per (row, channel) of the routing: s1 (first layer) holds position q in bits 2*((q+1)&3)
  // of byte (q+1)>>2, m2 (second layer) output p in bits 2*(p&3) of byte p>>2
  __host__ __device__ int s1row() const { return (P1 >> 2) + 1; }
  __host__ __device__ int m2row() const { return (P2 + 3) / 4; }
};
__host__ __device__ inline PotesDims potes_dims(int T) {
  PotesDims d;
  d.T = T;
  d.P1 = (T - 2) / 2;           // conv k5 pad1, MaxPool1d(2) floor
  d.P2 = (d.P1 - 2) / 2;
  return d;
}

// ReLU + MaxPool(2) of one pair of conv outputs, branch-free: value, and which of the two won and
// survived (0 none, 1 first, 2 second — torch's max-pool keeps the FIRST maximum: strict '>').
// Written as selects: the nested-if form compiled to an exec-mask branch per position
// (s_and_saveexec / s_cbranch_execz / s_or exec plus hazard nops, ~10 scalar instructions around
// three vector ones).
__device__ __forceinline__ void relu_pool2(float za, float zb, bool valid, float& a, uint32_t& sc) {
  const float ra = fmaxf(za, 0.f), rb = fmaxf(zb, 0.f);
  const bool second = rb > ra;
  const float best = second ? rb : ra;
  const uint32_t code = second ? 2u : (ra > 0.f ? 1u : 0u);
  a = valid ? best : 0.f;
  sc = valid ? code : 0u;
}

// The 2-bit routing codes, four per byte: code p of a row, and the same from a byte that is
// already in a register (kernels that load early and decode late).
__device__ __forceinline__ uint32_t route2_of(uint32_t byte, int p) { return (byte >> (2 * (p & 3))) & 3u; }
__device__ __forceinline__ uint32_t route2(const uint8_t* row, int p) { return route2_of(row[p >> 2], p); }

}  // namespace pcgmix
#endif
