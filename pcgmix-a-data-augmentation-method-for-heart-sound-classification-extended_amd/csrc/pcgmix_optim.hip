// pcgmix_optim.hip — the optimiser step and the gradient reduce it can fold in (gfx950).
//
//   potes_reduce_kernel     fixed-order sum of the 8/4-channel conv stack's per-block gradient
//                           partials (pcgmix_potes.hip writes them)
//   adam_clip_kernel        clip_grad_value_ + Adam for one tensor
//   clip_multi_body         the update of every tensor of a model in one launch, optionally with
//                           that reduce folded in as extra blocks; its two kernels differ only in
//                           the rule they hand it:
//   adam_clip_multi_kernel    AdamRule  clip_grad_value_ + Adam
//   sgd_clip_multi_kernel     SgdRule   clip_grad_value_ + momentum SGD
//   clip_multi_launch       the host side of both: table fill, block counts, launch
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pcgmix_kernels.h"
#include "pcgmix_potes_stack.h"

namespace pcgmix {

// Sum the per-block partial vectors in a fixed order: grads[e] = sum_g partial[g][e].
// Column e of the G partial rows, summed by one 256-thread block in a fixed order (thread t takes
// rows t, t + 256, ...; then a tree over the threads): the value is in red[0] for thread 0.
__device__ __forceinline__ float potes_reduce_column(const float* __restrict__ partial, int G, int e,
                                                     float* red) {
  float a = 0.f;
  for (int g = threadIdx.x; g < G; g += kPotThreads) a += partial[(size_t)g * kNGrad + e];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = kPotThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kPotThreads) void potes_reduce_kernel(const float* __restrict__ partial,
                                                                   float* __restrict__ grads,
                                                                   int G) {
  __shared__ float red[kPotThreads];
  const float v = potes_reduce_column(partial, G, blockIdx.x, red);
  if (threadIdx.x == 0) grads[blockIdx.x] = v;
}

// ---------------------------------------------------------------------------------- optimiser
// clip_grad_value_ + Adam (L2 weight decay) for one parameter tensor in one pass
// (train_model.py:557-558, 404-407, 566).  torch's foreach/fused Adam launches 512-thread blocks
// per 65536-element chunk: the 400k-element `dimreduc.weight` gets 7 blocks (41 us), and value
// clipping is two more foreach launches.  Same update rule as torch.optim.Adam:
//   g = clamp(g, -clip, clip) + wd * p;  m = lerp(m, g, 1-b1);  v = b2*v + (1-b2)*g*g
//   p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
// One element of it, with step_size = lr / (1-b1^t) and inv_bc2_sqrt = 1 / sqrt(1-b2^t):
__device__ __forceinline__ void adam_clip_update(float& p, float& m, float& v, float gi, float clip,
                                                 float wd, float one_m_b1, float b2, float one_m_b2,
                                                 float step_size, float inv_bc2_sqrt, float eps) {
  if (clip > 0.f) gi = fminf(fmaxf(gi, -clip), clip);
  const float pi = p;
  gi = fmaf(wd, pi, gi);
  float mi = m, vi = v;
  mi = fmaf(one_m_b1, gi - mi, mi);                 // exp_avg.lerp_(grad, 1 - beta1)
  vi = fmaf(one_m_b2 * gi, gi, b2 * vi);            // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
  const float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
  p = pi - step_size * (mi / denom);
  m = mi;
  v = vi;
}

__global__ __launch_bounds__(256) void adam_clip_kernel(float* __restrict__ p,
                                                        const float* __restrict__ g,
                                                        float* __restrict__ m,
                                                        float* __restrict__ v, long long n,
                                                        float clip, float wd, float one_m_b1,
                                                        float b2, float one_m_b2, float step_size,
                                                        float inv_bc2_sqrt, float eps) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    adam_clip_update(p[i], m[i], v[i], g[i], clip, wd, one_m_b1, b2, one_m_b2,
                     step_size, inv_bc2_sqrt, eps);
  }
}

// All parameter tensors of a model in ONE launch: eight ~3 us launches (six of them on tensors of
// <= 160 elements) become one.  The tensor table travels by value in the kernel arguments; a block
// owns kAdamEPB consecutive elements of one tensor and finds it by a uniform scan of blk_start.
constexpr int kAdamMaxTensors = 32;
constexpr int kAdamEPB = 1024;
struct AdamTable {
  float* p[kAdamMaxTensors];
  const float* g[kAdamMaxTensors];
  float* m[kAdamMaxTensors];
  float* v[kAdamMaxTensors];
  long long n[kAdamMaxTensors];
  int blk_start[kAdamMaxTensors + 1];
  int count;
};

// clip_grad_value_ + torch.optim.SGD (momentum, L2 weight decay; dampening 0, no nesterov) for one
// element (train_model.py:557-558, 404-405, 566), in torch's _single_tensor_sgd order of roundings:
//   g = clamp(g, -clip, clip);  g = fma(wd, p, g);  b = rn(mom * b) + g;  p = fma(-lr, b, p)
// The momentum line is buf.mul_(mom).add_(grad): a rounded product, then a rounded sum — not an
// fma (the file is compiled with -ffp-contract=off, so the compiler forms none either).  A zero
// buffer makes the first step torch's clone(grad): mom * 0 + g == g.  m == nullptr or mom == 0:
// no momentum, the buffer is neither read nor written.
__device__ __forceinline__ void sgd_clip_update(float& p, float* m, float gi, float clip, float wd,
                                                float mom, float lr) {
  if (clip > 0.f) gi = fminf(fmaxf(gi, -clip), clip);
  const float pi = p;
  if (wd != 0.f) gi = fmaf(wd, pi, gi);              // grad.add(param, alpha=wd)
  if (m != nullptr && mom != 0.f) {
    gi = __fmul_rn(mom, *m) + gi;                     // buf.mul_(mom).add_(grad)
    *m = gi;
  }
  p = fmaf(-lr, gi, pi);                             // param.add_(grad, alpha=-lr)
}

// One launch body for both optimisers.  A rule is a plain struct of the update's scalars, held in
// registers: the kernel builds it from its arguments, load() replaces them from device memory,
// apply() updates element i of tensor t of the table with the gradient gi.
// hyper != nullptr: the scalars are read from device memory instead (pcgmix_adam_hyper's /
// pcgmix_sgd_hyper's layout): a launch captured in a hipGraph then follows OneCycleLR's lr and
// beta1 / momentum, and Adam's bias corrections, from replay to replay.
// partial != nullptr: the launch carries kNGrad EXTRA blocks behind the table's own — block
// red_first + e sums column e of the conv stack's per-block gradient partials exactly as
// potes_reduce_kernel does (same order, same bits), stores it at grads[e] (what the parameters'
// .grad tensors alias) and applies the update to the one element it belongs to: the tensor of the
// table whose gradient pointer lies inside grads[0 .. kNGrad) (such tensors own no blocks of the
// table).  One launch instead of two at the end of a captured training step.
struct AdamRule {      // clip, wd, 1-b1, b2, 1-b2, step_size, 1/sqrt(bc2), eps
  float clip, wd, one_m_b1, b2, one_m_b2, step_size, inv_bc2_sqrt, eps;
  __device__ __forceinline__ void load(const float* __restrict__ hyper) {
    clip = hyper[0]; wd = hyper[1]; one_m_b1 = hyper[2]; b2 = hyper[3];
    one_m_b2 = hyper[4]; step_size = hyper[5]; inv_bc2_sqrt = hyper[6]; eps = hyper[7];
  }
  __device__ __forceinline__ void apply(const AdamTable& tab, int t, long long i, float gi) const {
    adam_clip_update(tab.p[t][i], tab.m[t][i], tab.v[t][i], gi, clip, wd, one_m_b1, b2, one_m_b2,
                     step_size, inv_bc2_sqrt, eps);
  }
};

struct SgdRule {       // the table's v is unused; OneCycleLR moves lr AND momentum
  float clip, wd, mom, lr;
  __device__ __forceinline__ void load(const float* __restrict__ hyper) {
    clip = hyper[0]; wd = hyper[1]; mom = hyper[2]; lr = hyper[3];
  }
  __device__ __forceinline__ void apply(const AdamTable& tab, int t, long long i, float gi) const {
    sgd_clip_update(tab.p[t][i], tab.m[t] ? tab.m[t] + i : nullptr, gi, clip, wd, mom, lr);
  }
};

template <class Rule>
__device__ __forceinline__ void clip_multi_body(const AdamTable& tab, Rule rule,
                                                const float* __restrict__ hyper,
                                                const float* __restrict__ partial,
                                                float* __restrict__ grads, int G, int red_first) {
  if (hyper) rule.load(hyper);
  if (partial && (int)blockIdx.x >= red_first) {
    __shared__ float red[kPotThreads];
    const int e = (int)blockIdx.x - red_first;
    const float gi = potes_reduce_column(partial, G, e, red);
    if (threadIdx.x != 0) return;
    grads[e] = gi;
    const float* ge = grads + e;
    for (int t = 0; t < tab.count; ++t) {
      if (ge >= tab.g[t] && ge < tab.g[t] + tab.n[t]) {
        rule.apply(tab, t, ge - tab.g[t], gi);
        return;
      }
    }
    return;
  }
  int t = 0;
  while (t + 1 < tab.count && (int)blockIdx.x >= tab.blk_start[t + 1]) ++t;
  const float* __restrict__ g = tab.g[t];
  const long long n = tab.n[t];
  const long long base = (long long)((int)blockIdx.x - tab.blk_start[t]) * kAdamEPB;
#pragma unroll
  for (int j = 0; j < kAdamEPB / 256; ++j) {
    const long long i = base + j * 256 + threadIdx.x;
    if (i >= n) break;
    rule.apply(tab, t, i, g[i]);
  }
}

__global__ __launch_bounds__(256) void adam_clip_multi_kernel(AdamTable tab, float clip, float wd,
                                                              float one_m_b1, float b2,
                                                              float one_m_b2, float step_size,
                                                              float inv_bc2_sqrt, float eps,
                                                              const float* __restrict__ hyper,
                                                              const float* __restrict__ partial,
                                                              float* __restrict__ grads, int G,
                                                              int red_first) {
  clip_multi_body(tab, AdamRule{clip, wd, one_m_b1, b2, one_m_b2, step_size, inv_bc2_sqrt, eps},
                  hyper, partial, grads, G, red_first);
}

__global__ __launch_bounds__(256) void sgd_clip_multi_kernel(AdamTable tab, float clip, float wd,
                                                             float mom, float lr,
                                                             const float* __restrict__ hyper,
                                                             const float* __restrict__ partial,
                                                             float* __restrict__ grads, int G,
                                                             int red_first) {
  clip_multi_body(tab, SgdRule{clip, wd, mom, lr}, hyper, partial, grads, G, red_first);
}

}  // namespace pcgmix

extern "C" int pcgmix_adam_hyper(float clip, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, long long step, float* out8) {
  if (!out8 || step < 1) return hipErrorInvalidValue;
  // bias corrections in float64 on the host, as torch computes them from Python floats
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  out8[0] = clip;
  out8[1] = weight_decay;
  out8[2] = 1.0f - beta1;
  out8[3] = beta2;
  out8[4] = 1.0f - beta2;
  out8[5] = (float)((double)lr / bc1);
  out8[6] = (float)(1.0 / std::sqrt(bc2));
  out8[7] = eps;
  return hipSuccess;
}

// The host side of both multi kernels: table fill, block counts and launch, kAdamMaxTensors
// tensors per launch.  Only two things are the optimiser's own: the kernel, and which state
// columns must be there.  Adam needs m[i] and v[i].  SGD has no v (nullptr), and m == nullptr or a
// null m[i] says that tensor has no momentum buffer (need_m: refuse it, the momentum is known to be
// non-zero).
enum class Optim { Adam, Sgd };
static int clip_multi_launch(Optim opt, bool need_m, int n_tensors, float* const* p,
                             const float* const* g, float* const* m, float* const* v,
                             const long long* n, const float* h8, const float* hyper_dev,
                             hipStream_t stream, const float* partial = nullptr,
                             float* grads = nullptr, int G = 0) {
  using namespace pcgmix;
  if (partial && n_tensors > kAdamMaxTensors) return hipErrorInvalidValue;   // one table, one launch
  for (int first = 0; first < n_tensors; first += kAdamMaxTensors) {
    AdamTable tab;
    tab.count = 0;
    int blocks = 0;
    const int last = first + kAdamMaxTensors < n_tensors ? first + kAdamMaxTensors : n_tensors;
    for (int i = first; i < last; ++i) {
      float* const mi = m ? m[i] : nullptr;
      float* const vi = v ? v[i] : nullptr;
      if (n[i] < 0 || (n[i] > 0 && (!p[i] || !g[i] || (need_m && !mi) || (opt == Optim::Adam && !vi))))
        return hipErrorInvalidValue;
      if (n[i] == 0) continue;
      // tensors whose gradient lives in grads[0 .. kNGrad) are updated by the reduction blocks
      const bool deferred = partial && g[i] >= grads && g[i] < grads + kNGrad;
      const long long nb = deferred ? 0 : (n[i] + kAdamEPB - 1) / kAdamEPB;
      if (nb > (1ll << 30) - blocks) return hipErrorInvalidValue;
      const int k = tab.count++;
      tab.p[k] = p[i]; tab.g[k] = g[i]; tab.m[k] = mi; tab.v[k] = vi; tab.n[k] = n[i];
      tab.blk_start[k] = blocks;
      blocks += (int)nb;
    }
    if (tab.count == 0) continue;
    tab.blk_start[tab.count] = blocks;
    const int red_first = blocks;
    if (partial) blocks += kNGrad;
    if (opt == Optim::Adam)
      hipLaunchKernelGGL(adam_clip_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, tab,
                         h8[0], h8[1], h8[2], h8[3], h8[4], h8[5], h8[6], h8[7], hyper_dev, partial,
                         grads, G, red_first);
    else
      hipLaunchKernelGGL(sgd_clip_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, tab,
                         h8[0], h8[1], h8[2], h8[3], hyper_dev, partial, grads, G, red_first);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
  }
  return hipSuccess;
}

extern "C" int pcgmix_adam_clip_multi_dev_f32(int n_tensors, float* const* p, const float* const* g,
                                              float* const* m, float* const* v, const long long* n,
                                              const float* hyper_dev, pcgmix_stream_t stream) {
  if (n_tensors < 0 || !hyper_dev || (n_tensors > 0 && (!p || !g || !m || !v || !n)))
    return hipErrorInvalidValue;
  const float zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return clip_multi_launch(Optim::Adam, true, n_tensors, p, g, m, v, n, zero8, hyper_dev,
                           reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcgmix_adam_clip_multi_reduce_dev_f32(int n_tensors, float* const* p,
                                                     const float* const* g, float* const* m,
                                                     float* const* v, const long long* n,
                                                     const float* hyper_dev, const float* partial,
                                                     float* grads, int G, pcgmix_stream_t stream) {
  if (n_tensors <= 0 || !hyper_dev || !p || !g || !m || !v || !n || !partial || !grads || G <= 0)
    return hipErrorInvalidValue;
  const float zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return clip_multi_launch(Optim::Adam, true, n_tensors, p, g, m, v, n, zero8, hyper_dev,
                           reinterpret_cast<hipStream_t>(stream), partial, grads, G);
}

extern "C" int pcgmix_potes_reduce_f32(const float* partial, float* grads, int G, pcgmix_stream_t stream) {
  if (!partial || !grads || G <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pcgmix::potes_reduce_kernel, dim3(pcgmix::kNGrad), dim3(pcgmix::kPotThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), partial, grads, G);
  return (int)hipGetLastError();
}

extern "C" int pcgmix_adam_clip_multi_f32(int n_tensors, float* const* p, const float* const* g,
                                          float* const* m, float* const* v, const long long* n,
                                          float clip, float lr, float beta1, float beta2, float eps,
                                          float weight_decay, long long step,
                                          pcgmix_stream_t stream) {
  if (n_tensors < 0 || step < 1 || (n_tensors > 0 && (!p || !g || !m || !v || !n)))
    return hipErrorInvalidValue;
  float h8[8];
  pcgmix_adam_hyper(clip, lr, beta1, beta2, eps, weight_decay, step, h8);
  return clip_multi_launch(Optim::Adam, true, n_tensors, p, g, m, v, n, h8, nullptr,
                           reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcgmix_adam_clip_f32(float* p, const float* g, float* m, float* v, long long n,
                                    float clip, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, long long step, pcgmix_stream_t stream) {
  using namespace pcgmix;
  if (!p || !g || !m || !v || n < 0 || step < 1) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  float h8[8];
  pcgmix_adam_hyper(clip, lr, beta1, beta2, eps, weight_decay, step, h8);
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adam_clip_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p, g, m, v, n, h8[0], h8[1], h8[2],
                     h8[3], h8[4], h8[5], h8[6], h8[7]);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------- SGD
extern "C" int pcgmix_sgd_hyper(float clip, float lr, float momentum, float weight_decay,
                                float* out8) {
  if (!out8) return hipErrorInvalidValue;
  out8[0] = clip;
  out8[1] = weight_decay;
  out8[2] = momentum;
  out8[3] = lr;
  out8[4] = out8[5] = out8[6] = out8[7] = 0.f;
  return hipSuccess;
}

extern "C" int pcgmix_sgd_clip_multi_f32(int n_tensors, float* const* p, const float* const* g,
                                         float* const* m, const long long* n, float clip, float lr,
                                         float momentum, float weight_decay,
                                         pcgmix_stream_t stream) {
  if (n_tensors < 0 || (n_tensors > 0 && (!p || !g || !n || (!m && momentum != 0.f))))
    return hipErrorInvalidValue;
  float h8[8];
  pcgmix_sgd_hyper(clip, lr, momentum, weight_decay, h8);
  return clip_multi_launch(Optim::Sgd, momentum != 0.f, n_tensors, p, g,
                           momentum != 0.f ? m : nullptr, nullptr, n, h8, nullptr,
                           reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcgmix_sgd_clip_multi_dev_f32(int n_tensors, float* const* p, const float* const* g,
                                             float* const* m, const long long* n,
                                             const float* hyper_dev, pcgmix_stream_t stream) {
  if (n_tensors < 0 || !hyper_dev || (n_tensors > 0 && (!p || !g || !m || !n)))
    return hipErrorInvalidValue;
  const float zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return clip_multi_launch(Optim::Sgd, false, n_tensors, p, g, m, nullptr, n, zero8, hyper_dev,
                           reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pcgmix_sgd_clip_multi_reduce_dev_f32(int n_tensors, float* const* p,
                                                    const float* const* g, float* const* m,
                                                    const long long* n, const float* hyper_dev,
                                                    const float* partial, float* grads, int G,
                                                    pcgmix_stream_t stream) {
  if (n_tensors <= 0 || !hyper_dev || !p || !g || !m || !n || !partial || !grads || G <= 0)
    return hipErrorInvalidValue;
  const float zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return clip_multi_launch(Optim::Sgd, false, n_tensors, p, g, m, nullptr, n, zero8, hyper_dev,
                           reinterpret_cast<hipStream_t>(stream), partial, grads, G);
}
