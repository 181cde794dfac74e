// The classifier's per-pixel arithmetic, written once: first-max class, softmax terms, weighted cross-entropy with its gradient, IoU
// confusion ballots, class counts, and the workgroup reduction in front of the atomics.  Every kernel that scores or predicts a pixel
// (loss.hip: wce_kernel, wce_score_kernel, logits_predict_kernel, confusion_kernel; stem_head.hip: head_fused_fwd_kernel) calls these, which
// is why equal logits give equal bits whichever of them ran: dc_head_fwd_loss / _score / _predict against dc_head_fwd followed by
// dc_wce_fused / dc_wce_score / dc_logits_predict.  A kernel keeps its own grid, index walk, wave-uniform trip count and LDS placement.
//   reference: utils/losses.py:28-52 (plain mean of w[y]*CE; the "false positive" factors are identities),
//              torch.max(outputs,1)[1] (train_hdf5_ddp.py:406,458), utils/utils.py:32-60.
#pragma once
#include "common.h"
#include "mask_skill.h"

namespace dc {

constexpr int NC = 3;   // classes

// labels outside [0, NC) come back as -1 (the full 64-bit value is compared, not its low half)
__device__ inline int load_label(const void* labels, int bytes, size_t i) {
  const long long v = mask_value(labels, i, bytes);
  return (v >= 0 && v < NC) ? (int)v : -1;
}

// torch.max's class: the FIRST maximum
struct FirstMax {
  int am;
  float best;
};
__device__ inline FirstMax first_max(float l0, float l1, float l2) {
  FirstMax m{0, l0};
  if (l1 > m.best) { m.best = l1; m.am = 1; }
  if (l2 > m.best) { m.best = l2; m.am = 2; }
  return m;
}

struct SoftmaxTerms {
  float e0, e1, e2, se;   // se = 1 / probability of the first-max class
};
__device__ inline SoftmaxTerms softmax_terms(float l0, float l1, float l2, float best) {
  SoftmaxTerms t;
  t.e0 = expf(l0 - best), t.e1 = expf(l1 - best), t.e2 = expf(l2 - best);
  t.se = t.e0 + t.e1 + t.e2;
  return t;
}

// The quantised probabilities q_c = rint(p_c * 65536) in [0, 65536], p_c = e_c / se in fp32: the ONE chain from logits to q.  What
// probskill.hip bins and scores and what decide.hip thresholds, so that a threshold read off the former's table reproduces its
// forecast bit for bit.
struct ProbQ {
  int q0, q1, q2;
};
__device__ inline ProbQ prob_q(float l0, float l1, float l2) {
  const FirstMax m = first_max(l0, l1, l2);
  const SoftmaxTerms s = softmax_terms(l0, l1, l2, m.best);
  return {__float2int_rn(s.e0 / s.se * 65536.f), __float2int_rn(s.e1 / s.se * 65536.f), __float2int_rn(s.e2 / s.se * 65536.f)};
}
// neither NaN nor an infinity, in all three (the exponent bits)
__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ inline bool logits_finite(float l0, float l1, float l2) { return finite_bits(l0) && finite_bits(l1) && finite_bits(l2); }

struct ClassWeights {
  float w0, w1, w2;
};
__device__ inline ClassWeights load_class_weights(const float* cw) { return {cw[0], cw[1], cw[2]}; }

// One pixel's term w[y] * (logsumexp - l[y]) of the loss sum; with gp its three gradient planes (plane elements apart) get
// grad_scale * w[y] * (softmax - onehot).
// A label outside [0, 3): nn.CrossEntropyLoss raises for it in the reference (losses.py:36).  A kernel cannot raise and this ABI never
// synchronises, so the result is poisoned instead of silently dropping the pixel: the term and this pixel's gradient become NaN, which
// reaches every weight in the same step.
__device__ inline float wce_pixel(float l0, float l1, float l2, float best, int y, const ClassWeights& w, float grad_scale, float* gp,
                                  size_t plane) {
  const SoftmaxTerms t = softmax_terms(l0, l1, l2, best);
  const float lse = best + logf(t.se);
  if ((unsigned)y >= (unsigned)NC) {
    if (gp != nullptr) gp[0] = gp[plane] = gp[2 * plane] = __builtin_nanf("");
    return __builtin_nanf("");
  }
  const float wy = y == 0 ? w.w0 : (y == 1 ? w.w1 : w.w2);
  const float ly = y == 0 ? l0 : (y == 1 ? l1 : l2);
  if (gp != nullptr) {
    const float inv = 1.0f / t.se;
    const float s = wy * grad_scale;
    gp[0] = s * (t.e0 * inv - (y == 0 ? 1.f : 0.f));
    gp[plane] = s * (t.e1 * inv - (y == 1 ? 1.f : 0.f));
    gp[2 * plane] = s * (t.e2 * inv - (y == 2 ? 1.f : 0.f));
  }
  return wy * (lse - ly);
}

__device__ inline unsigned long long wave_count(bool pred) { return __popcll(__ballot(pred)); }

// tp[3], fp[3], fn[3] of utils.py:32-60 as wave-uniform counters.  add() is a ballot: all 64 lanes of the wave must reach it (ok = this
// lane has a pixel), so the loop around it has a wave-uniform trip count.
struct Confusion {
  unsigned long long c[3 * NC] = {};
  __device__ void add(bool ok, int am, int y) {
    const bool eq = ok && (am == y), ne = ok && (am != y);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      c[j] += wave_count(eq && y == j);            // tp: agree and gt == j
      c[NC + j] += wave_count(ne && am == j);      // fp: disagree and pred == j
      c[2 * NC + j] += wave_count(ne && y == j);   // fn: disagree and gt == j
    }
  }
};

// pixels per predicted class, wave-uniform like Confusion
struct ClassCount {
  unsigned long long c[NC] = {};
  __device__ void add(bool ok, int am) {
#pragma unroll
    for (int j = 0; j < NC; ++j) c[j] += wave_count(ok && am == j);
  }
};

// The reduction of a 256-thread workgroup's four waves: stage_* (lane 0 of each wave writes its wave's value to LDS), ONE __syncthreads()
// by the caller, then commit_* (the four are added in wave order and the sum goes to dst[sample] by atomicAdd; a null dst takes nothing).
// s: LDS, 4 * K counters / 4 doubles.
template <int K>
__device__ inline void stage_counts(const unsigned long long (&c)[K], unsigned long long* s) {
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[(threadIdx.x >> 6) * K + k] = c[k];   // wave-uniform already
  }
}
template <int K>
__device__ inline void commit_counts(const unsigned long long* s, unsigned long long* dst, size_t sample) {
  if (threadIdx.x < K && dst != nullptr) {
    const int k = threadIdx.x;
    const unsigned long long c = s[k] + s[K + k] + s[2 * K + k] + s[3 * K + k];
    if (c) atomicAdd(&dst[sample * K + k], c);
  }
}
__device__ inline void stage_loss(double lsum, double* s) {
  lsum = wave_sum(lsum);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = lsum;
}
__device__ inline void commit_loss(const double* s, double* dst, size_t sample) {
  if (threadIdx.x == 0 && dst != nullptr) atomicAdd(dst + sample, s[0] + s[1] + s[2] + s[3]);
}

}  // namespace dc
