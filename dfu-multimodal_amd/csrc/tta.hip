// Test-time augmentation evaluation (notebooks/test_time_augmentation.py) after the model's
// forward pass over every view: the per-sample reduction of the view logits (:207-229: mean of
// the view probabilities, majority vote of the per-view decisions) and the counts behind the
// script's metrics (:239-246: confusion matrix -> accuracy, F1, sensitivity, specificity; pair
// counts -> AUC-ROC).  Both stay on the device; the host reads the six counts once.
#include "common.h"

#pragma clang fp contract(off)  // the probabilities round like the CPU code

namespace {

constexpr int TPB = 256;

// One thread per sample, its views in row order.  C == 1: p = sigmoid(x), vote = p > 0.5 on the
// rounded fp32 p (so x == 0 votes 0).  C == 2: p = softmax(row)[1], vote = argmax == 1 with the
// first maximum winning (x1 > x0).
template <int C>
__global__ void k_tta_reduce(const float* __restrict__ logits, int samples, int views,
                             float* __restrict__ prob, int64_t* __restrict__ pred) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= samples) return;
  const float* x = logits + (int64_t)i * views * C;
  float sum = 0.f;
  int votes = 0;
  for (int v = 0; v < views; ++v) {
    float p;
    if (C == 1) {
      p = 1.0f / (1.0f + expf(-x[v]));
      votes += p > 0.5f;
    } else {
      const float x0 = x[2 * v], x1 = x[2 * v + 1];
      const float mx = fmaxf(x0, x1);
      const float e0 = expf(x0 - mx), e1 = expf(x1 - mx);
      p = e1 / (e0 + e1);
      votes += x1 > x0;
    }
    sum += p;
  }
  prob[i] = sum / (float)views;
  pred[i] = 2 * votes > views ? 1 : 0;
}

DFU_DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block (bx, by) counts the pairs of its tile of positives (samples [bx * TPB, +TPB) with label
// 1) against its tile of negatives (samples [by * TPB, +TPB) with label 0).  Both tiles are
// staged in LDS with every sample that is not of the tile's class (or past n) replaced by NaN:
// a comparison with NaN is false, so those samples add to neither count and the inner loop is
// branch-free.  Thread t owns positive t and sweeps the negative tile (one LDS broadcast read
// per pair); at most TPB per thread, so int32 holds until the wave reduction, and each wave ends
// with one 64-bit atomicAdd per non-zero count.  The column of blocks by == 0 also counts its
// samples' confusion cell (label * 2 + prediction: tn, fp, fn, tp) by wave ballot.
__global__ void __launch_bounds__(TPB) k_binary_eval_counts(const float* __restrict__ prob,
                                                            const int64_t* __restrict__ pred,
                                                            const int64_t* __restrict__ labels,
                                                            int n,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ float pos[TPB], neg[TPB];
  const int t = threadIdx.x;
  const int i = blockIdx.x * TPB + t, j = blockIdx.y * TPB + t;
  const float none = __builtin_nanf("");
  const int64_t yi = i < n ? labels[i] : -1;
  pos[t] = yi == 1 ? prob[i] : none;
  neg[t] = (j < n && labels[j] == 0) ? prob[j] : none;
  __syncthreads();
  const float p = pos[t];
  int greater = 0, ties = 0;
#pragma unroll 8
  for (int k = 0; k < TPB; ++k) {
    const float q = neg[k];
    greater += p > q;
    ties += p == q;
  }
  greater = wave_sum_i(greater);
  ties = wave_sum_i(ties);
  const bool lane0 = (t & 63) == 0;
  if (lane0 && greater) atomicAdd(counts + 4, (unsigned long long)greater);
  if (lane0 && ties) atomicAdd(counts + 5, (unsigned long long)ties);
  if (blockIdx.y == 0) {
    const int cell = (yi == 0 || yi == 1) ? (int)yi * 2 + (pred[i] != 0) : -1;
    for (int c = 0; c < 4; ++c) {
      const int cnt = __popcll(__ballot(cell == c));
      if (lane0 && cnt) atomicAdd(counts + c, (unsigned long long)cnt);
    }
  }
}

}  // namespace

extern "C" int dfu_tta_reduce(const float* logits, int32_t samples, int32_t views, int32_t C,
                              float* prob_out, int64_t* pred_out, void* stream) {
  DFU_CHECK_ARG(logits && prob_out && pred_out && samples > 0 && views > 0,
                "dfu_tta_reduce: bad args");
  DFU_CHECK_ARG(C == 1 || C == 2, "dfu_tta_reduce: C = %d (1 sigmoid logit or 2 softmax logits)",
                C);
  const dim3 grid((samples + TPB - 1) / TPB);
  if (C == 1)
    hipLaunchKernelGGL(k_tta_reduce<1>, grid, dim3(TPB), 0, (hipStream_t)stream, logits, samples,
                       views, prob_out, pred_out);
  else
    hipLaunchKernelGGL(k_tta_reduce<2>, grid, dim3(TPB), 0, (hipStream_t)stream, logits, samples,
                       views, prob_out, pred_out);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}

extern "C" int dfu_binary_eval_counts(const float* prob, const int64_t* pred,
                                      const int64_t* labels, int32_t n, int64_t* counts,
                                      void* stream) {
  DFU_CHECK_ARG(prob && pred && labels && counts && n > 0 && n < (1 << 24),
                "dfu_binary_eval_counts: bad args");
  const int tiles = (n + TPB - 1) / TPB;  // <= 65535, the grid's y limit
  hipLaunchKernelGGL(k_binary_eval_counts, dim3(tiles, tiles), dim3(TPB), 0, (hipStream_t)stream,
                     prob, pred, labels, n, (unsigned long long*)counts);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}
