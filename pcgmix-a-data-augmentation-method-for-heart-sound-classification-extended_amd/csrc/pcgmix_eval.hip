// pcgmix_eval.hip — the evaluation pass (gfx950): per-cycle softmax, loss and vote, and the
// per-recording reduction, without atomics and with every sum in a stated order.
//
// Reference: train_model.py:591-670 (test_data_accuracy): per batch the softmax of the logits
// (:602) and the criterion (:608-609); per recording the mean of its cycles' softmax rows
// (np.mean(arr, axis=0), :627) or, under '(class_majority)', the bincount of their arg-max votes
// (:634-647).
//
//   eval_rows_kernel        logits (B,C) -> prob (B,C), loss_rows (B), vote (B); one thread per row
//                           (eval_row, pcgmix_kernels.h — the Potes eval head's tail in
//                           pcgmix_head.hip applies the same function to the logits it forms)
//   eval_segments_kernel    one thread per (recording, class) column: walks the recording's cycles
//                           in loader order adding float32, then divides by float(n) — what
//                           np.mean(list_of_rows, axis=0) does, bit for bit; counts the votes for its
//                           class; the class-0 thread adds the recording's row losses in double
//
// These are latency-bound kernels over a few KB: the segment walk requests eight cycles' rows
// before it adds the first, the adds themselves stay sequential (the order is the contract).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pcgmix_kernels.h"

namespace pcgmix {

constexpr int kEvalBlock = 256;
constexpr int kSegBlock = 64;
constexpr int kSegAhead = 8;

__global__ __launch_bounds__(kEvalBlock) void eval_rows_kernel(
    const float* __restrict__ logits, const uint8_t* __restrict__ labels, float* __restrict__ prob,
    float* __restrict__ loss_rows, uint8_t* __restrict__ vote, int B, int C) {
  const int b = blockIdx.x * kEvalBlock + threadIdx.x;
  if (b >= B) return;
  float loss;
  const int v = eval_row(logits + (size_t)b * C, C, labels ? (int)labels[b] : -1,
                         prob + (size_t)b * C, loss);
  loss_rows[b] = loss;
  vote[b] = (uint8_t)v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kSegBlock) void eval_segments_kernel(
    const float* __restrict__ prob, const float* __restrict__ loss_rows,
    const uint8_t* __restrict__ vote, const int32_t* __restrict__ order,
    const int32_t* __restrict__ rec_start, float* __restrict__ mean_p, int32_t* __restrict__ votes,
    double* __restrict__ loss_rec, int N, int R, int C) {
  const int t = blockIdx.x * kSegBlock + threadIdx.x;
  if (t >= R * C) return;
  const int r = t / C, c = t - r * C;
  // the host built and checked order and rec_start; whatever they hold, nothing outside the N rows is read
  const int lo = clampi(rec_start[r], 0, N);
  const int hi = clampi(rec_start[r + 1], lo, N);
  float acc = 0.f;
  double lacc = 0.0;
  int cnt = 0;
  int i = lo;
  for (; i + kSegAhead <= hi; i += kSegAhead) {
    int row[kSegAhead];
    float pv[kSegAhead], lv[kSegAhead];
    uint8_t vv[kSegAhead];
#pragma unroll
    for (int j = 0; j < kSegAhead; ++j) row[j] = clampi(order[i + j], 0, N - 1);
#pragma unroll
    for (int j = 0; j < kSegAhead; ++j) {
      pv[j] = prob[(size_t)row[j] * C + c];
      vv[j] = vote[row[j]];
      lv[j] = c == 0 ? loss_rows[row[j]] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kSegAhead; ++j) {
      acc += pv[j];
      cnt += (int)vv[j] == c ? 1 : 0;
      lacc += (double)lv[j];
    }
  }
  for (; i < hi; ++i) {
    const int row = clampi(order[i], 0, N - 1);
    acc += prob[(size_t)row * C + c];
    cnt += (int)vote[row] == c ? 1 : 0;
    if (c == 0) lacc += (double)loss_rows[row];
  }
  mean_p[t] = acc / (float)(hi - lo);       // an empty recording gives 0/0 = NaN, as np.mean of no rows
  votes[t] = cnt;
  if (c == 0) loss_rec[r] = lacc;
}

}  // namespace pcgmix

extern "C" int pcgmix_eval_rows_f32(const float* logits, const uint8_t* labels, float* prob,
                                    float* loss_rows, uint8_t* vote, int B, int C,
                                    pcgmix_stream_t stream) {
  using namespace pcgmix;
  if (B < 0 || C <= 0 || C > kEvalMaxC) return hipErrorInvalidValue;
  if (B == 0) return 0;
  if (!logits || !prob || !loss_rows || !vote) return hipErrorInvalidValue;
  hipLaunchKernelGGL(eval_rows_kernel, dim3((unsigned)((B + kEvalBlock - 1) / kEvalBlock)),
                     dim3(kEvalBlock), 0, reinterpret_cast<hipStream_t>(stream), logits, labels, prob,
                     loss_rows, vote, B, C);
  return (int)hipGetLastError();
}

extern "C" int pcgmix_eval_segments_f32(const float* prob, const float* loss_rows, const uint8_t* vote,
                                        const int32_t* order, const int32_t* rec_start, float* mean_p,
                                        int32_t* votes, double* loss_rec, int N, int R, int C,
                                        pcgmix_stream_t stream) {
  using namespace pcgmix;
  if (N < 0 || R < 0 || C <= 0 || C > kEvalMaxC || (long long)R * C > 0x7fffffffll)
    return hipErrorInvalidValue;
  if (R == 0) return 0;
  if (N == 0 || !prob || !loss_rows || !vote || !order || !rec_start || !mean_p || !votes || !loss_rec ||
      (reinterpret_cast<uintptr_t>(loss_rec) & 7))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(eval_segments_kernel, dim3((unsigned)((R * C + kSegBlock - 1) / kSegBlock)),
                     dim3(kSegBlock), 0, reinterpret_cast<hipStream_t>(stream), prob, loss_rows, vote,
                     order, rec_start, mean_p, votes, loss_rec, N, R, C);
  return (int)hipGetLastError();
}
