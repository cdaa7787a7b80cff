// The curve behind the extended medical metrics (notebooks/extended_metrics.py: roc_curve,
// precision_recall_curve, auc): scikit-learn's _binary_clf_curve on the device.  For every
// distinct score, in descending order, the number of label-1 and of label-0 samples scored at or
// above it.  Rank counting instead of a sort: every sample compares itself with all n, so the
// counts are integers that no arrival order can change, and no float atomics are needed.  The
// cost is n^2 comparisons (1e8 at the 1e4 samples of a test set, 1e12 at the n < 2^20 limit).
#include "common.h"

namespace {

constexpr int TPB = 256;

// Pass 1, thread i: over all j, tp = #{label 1, s_j >= s_i}, fp = #{label 0, s_j >= s_i} and
// earlier = #{valid j < i, s_j == s_i}.  Every block sweeps the n scores in tiles of TPB staged
// in LDS, split by class with everything else (invalid, other class, past n) as NaN: a
// comparison with NaN is false, so the inner loop is branch-free (as k_binary_eval_counts).  An
// invalid i carries NaN itself and counts nothing.  A valid sample with earlier == 0 represents
// its tie group: rep[i] = s_i, else NaN.
__global__ void __launch_bounds__(TPB) k_curve_rank(const float* __restrict__ prob,
                                                    const int64_t* __restrict__ labels, int n,
                                                    float* __restrict__ rep,
                                                    int* __restrict__ tp_ws,
                                                    int* __restrict__ fp_ws,
                                                    int* __restrict__ k_out) {
  __shared__ float pos[TPB], neg[TPB];
  const int t = threadIdx.x;
  const int i = blockIdx.x * TPB + t;
  const float none = __builtin_nanf("");
  if (i == 0) *k_out = 0;  // pass 2 (the next kernel of the stream) adds to it
  float s = none;
  if (i < n) {
    const int64_t y = labels[i];
    if (y == 0 || y == 1) s = prob[i];
  }
  int tp = 0, fp = 0, earlier = 0;
  for (int base = 0; base < n; base += TPB) {
    const int j = base + t;
    const int64_t yj = j < n ? labels[j] : -1;
    const float sj = j < n ? prob[j] : none;
    __syncthreads();  // the previous tile has been read
    pos[t] = yj == 1 ? sj : none;
    neg[t] = yj == 0 ? sj : none;
    __syncthreads();
    const int before = i - base;  // tile entries k < before are samples j < i
#pragma unroll 8
    for (int k = 0; k < TPB; ++k) {
      const float p = pos[k], q = neg[k];
      tp += p >= s;
      fp += q >= s;
      earlier += ((p == s) | (q == s)) & (k < before);
    }
  }
  if (i < n) {
    rep[i] = (s == s && earlier == 0) ? s : none;
    tp_ws[i] = tp;
    fp_ws[i] = fp;
  }
}

// Pass 2, thread i: a representative's slot is the number of representatives with a strictly
// greater score (representatives are pairwise distinct under ==, so the slots are 0 .. K-1, each
// taken once).  It writes its threshold and counts there; K is the number of representatives,
// one integer atomic per wave.
__global__ void __launch_bounds__(TPB) k_curve_place(const float* __restrict__ rep,
                                                     const int* __restrict__ tp_ws,
                                                     const int* __restrict__ fp_ws, int n,
                                                     float* __restrict__ thresholds,
                                                     int64_t* __restrict__ tps,
                                                     int64_t* __restrict__ fps,
                                                     int* __restrict__ k_out) {
  __shared__ float tile[TPB];
  const int t = threadIdx.x;
  const int i = blockIdx.x * TPB + t;
  const float none = __builtin_nanf("");
  const float s = i < n ? rep[i] : none;
  int slot = 0;
  for (int base = 0; base < n; base += TPB) {
    const int j = base + t;
    __syncthreads();
    tile[t] = j < n ? rep[j] : none;
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < TPB; ++k) slot += tile[k] > s;
  }
  const bool is_rep = s == s;
  if (is_rep) {  // slot < K <= n
    thresholds[slot] = s;
    tps[slot] = tp_ws[i];
    fps[slot] = fp_ws[i];
  }
  const int cnt = __popcll(__ballot(is_rep));
  if ((t & 63) == 0 && cnt) atomicAdd(k_out, cnt);
}

}  // namespace

extern "C" int dfu_binary_curve(const float* prob, const int64_t* labels, int32_t n,
                                float* thresholds, int64_t* tps, int64_t* fps, int32_t* k_out,
                                void* workspace, void* stream) {
  DFU_CHECK_ARG(prob && labels && thresholds && tps && fps && k_out && workspace && n > 0 &&
                    n < (1 << 20),
                "dfu_binary_curve: bad args");
  // workspace, 12 n bytes: rep fp32 [n], tp int32 [n], fp int32 [n]
  float* rep = (float*)workspace;
  int* tp_ws = (int*)workspace + n;
  int* fp_ws = tp_ws + n;
  const dim3 grid((n + TPB - 1) / TPB);
  hipLaunchKernelGGL(k_curve_rank, grid, dim3(TPB), 0, (hipStream_t)stream, prob, labels, n, rep,
                     tp_ws, fp_ws, k_out);
  DFU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_curve_place, grid, dim3(TPB), 0, (hipStream_t)stream, rep, tp_ws, fp_ws, n,
                     thresholds, tps, fps, k_out);
  DFU_LAUNCH_CHECK();
  return DFU_OK;
}
