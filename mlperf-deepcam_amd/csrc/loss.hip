// Fused weighted cross-entropy forward + backward, first-max argmax and IoU confusion counts in ONE pass over the
// NCHW fp32 logits (HBM-bound: 12 B/pixel read, 12 B/pixel gradient write, 8 B/pixel labels).
//   reference: utils/losses.py:28-52 (plain mean of w[y]*CE; the "false positive" factors are identities),
//              torch.max(outputs,1)[1] (train_hdf5_ddp.py:406,458), utils/utils.py:32-60.
#include "pixel_score.h"

namespace dc {

// The per-pixel arithmetic and the workgroup reduction of the four kernels below are pixel_score.h's; a kernel here is its index walk.
__global__ __launch_bounds__(256) void wce_kernel(int B, long HW, const float* __restrict__ logits,
                                                  const void* __restrict__ labels, int lbytes,
                                                  const float* __restrict__ cw, float grad_scale, double* loss_sum,
                                                  float* __restrict__ dlogits, int64_t* __restrict__ pred,
                                                  unsigned long long* counts) {
  __shared__ double s_loss[4];
  __shared__ unsigned long long s_cnt[4 * 9];
  const long total = (long)B * HW;
  const ClassWeights w = load_class_weights(cw);
  double lsum = 0.0;
  Confusion cf;
  // the trip count is made wave-uniform so that the ballots below see all 64 lanes
  const long stride = (long)gridDim.x * blockDim.x;
  const long first = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long iters = (total + stride - 1) / stride;
  for (long it = 0; it < iters; ++it) {
    const long i = first + it * stride;
    const bool ok = i < total;
    int y = 0, am = 0;
    if (ok) {
      const long b = i / HW, p = i - b * HW;
      const float* lp = logits + (size_t)b * NC * HW + p;
      const float l0 = lp[0], l1 = lp[HW], l2 = lp[2 * HW];
      y = load_label(labels, lbytes, i);
      const FirstMax m = first_max(l0, l1, l2);
      am = m.am;
      lsum += (double)wce_pixel(l0, l1, l2, m.best, y, w, grad_scale, dlogits != nullptr ? dlogits + (size_t)b * NC * HW + p : nullptr, HW);
      if (pred != nullptr) pred[i] = am;
    }
    if (counts != nullptr) cf.add(ok, am, y);
  }
  stage_loss(lsum, s_loss);
  stage_counts(cf.c, s_cnt);
  __syncthreads();
  commit_loss(s_loss, loss_sum, 0);
  commit_counts<9>(s_cnt, counts, 0);
}

// The validation pass: no gradient, no prediction store, and blockIdx.y is the sample, so a workgroup's partial sums belong to one sample
// and land in that sample's entries.
__global__ __launch_bounds__(256) void wce_score_kernel(long HW, const float* __restrict__ logits, const void* __restrict__ labels,
                                                        int lbytes, const float* __restrict__ cw, double* loss_sum,
                                                        unsigned long long* counts) {
  __shared__ double s_loss[4];
  __shared__ unsigned long long s_cnt[4 * 9];
  const int b = blockIdx.y;
  const ClassWeights w = load_class_weights(cw);
  const float* lb = logits + (size_t)b * NC * HW;
  double lsum = 0.0;
  Confusion cf;
  // the trip count is wave-uniform so that the ballots below see all 64 lanes
  const long stride = (long)gridDim.x * blockDim.x;
  const long first = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long iters = (HW + stride - 1) / stride;
  for (long it = 0; it < iters; ++it) {
    const long p = first + it * stride;
    const bool ok = p < HW;
    int y = 0, am = 0;
    if (ok) {
      const float l0 = lb[p], l1 = lb[HW + p], l2 = lb[2 * HW + p];
      y = load_label(labels, lbytes, (size_t)b * HW + p);
      const FirstMax m = first_max(l0, l1, l2);
      am = m.am;
      lsum += (double)wce_pixel(l0, l1, l2, m.best, y, w, 0.f, nullptr, 0);
    }
    cf.add(ok, am, y);
  }
  stage_loss(lsum, s_loss);
  stage_counts(cf.c, s_cnt);
  __syncthreads();
  commit_loss(s_loss, loss_sum, b);
  commit_counts<9>(s_cnt, counts, b);
}

// Inference on stored logits (dc_logits_predict): the first-max class as one byte, optionally its softmax probability, and the pixel count
// per class of each sample; blockIdx.y is the sample as in wce_score_kernel.
__global__ __launch_bounds__(256) void logits_predict_kernel(long HW, const float* __restrict__ logits, uint8_t* __restrict__ mask,
                                                             float* __restrict__ conf, unsigned long long* counts) {
  __shared__ unsigned long long s_cnt[4 * NC];
  const int b = blockIdx.y;
  const float* lb = logits + (size_t)b * NC * HW;
  ClassCount cc;
  // the trip count is wave-uniform so that the ballots below see all 64 lanes
  const long stride = (long)gridDim.x * blockDim.x;
  const long first = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long iters = (HW + stride - 1) / stride;
  for (long it = 0; it < iters; ++it) {
    const long p = first + it * stride;
    const bool ok = p < HW;
    int am = 0;
    if (ok) {
      const float l0 = lb[p], l1 = lb[HW + p], l2 = lb[2 * HW + p];
      const size_t gi = (size_t)b * HW + p;
      const FirstMax m = first_max(l0, l1, l2);
      am = m.am;
      mask[gi] = (uint8_t)am;
      if (conf != nullptr) conf[gi] = 1.0f / softmax_terms(l0, l1, l2, m.best).se;
    }
    if (counts != nullptr) cc.add(ok, am);
  }
  if (counts == nullptr) return;
  stage_counts(cc.c, s_cnt);
  __syncthreads();
  commit_counts<NC>(s_cnt, counts, b);
}

// One thread walks the samples in order: the three running sums do not depend on how anything was scheduled.
__global__ void val_accumulate_kernel(int n_valid, long HW, const double* __restrict__ loss_sum, const long long* __restrict__ counts,
                                      double* acc, double* per_sample) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double a0 = acc[0], a1 = acc[1], a2 = acc[2];
  for (int b = 0; b < n_valid; ++b) {
    const double loss = loss_sum[b] / (double)HW;
    float s = 0.f;
    for (int j = 0; j < NC; ++j) {
      const long long tp = counts[b * 9 + j], fp = counts[b * 9 + 3 + j], fn = counts[b * 9 + 6 + j];
      const long long un = tp + fp + fn;
      // utils.py:55-58: float tensors, tp / union (1 where the union is empty), summed in class order
      s += un == 0 ? 1.0f : (float)tp / (float)un;
    }
    const double iou = (double)(s / 3.0f);
    a0 += 1.0;
    a1 += loss;
    a2 += iou;
    if (per_sample != nullptr) {
      per_sample[2 * b] = loss;
      per_sample[2 * b + 1] = iou;
    }
  }
  acc[0] = a0;
  acc[1] = a1;
  acc[2] = a2;
}

__global__ __launch_bounds__(256) void confusion_kernel(long n, const int64_t* __restrict__ pred,
                                                        const void* __restrict__ labels, int lbytes,
                                                        unsigned long long* counts) {
  __shared__ unsigned long long s_cnt[4 * 9];
  Confusion cf;
  const long stride = (long)gridDim.x * blockDim.x;
  const long first = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long iters = (n + stride - 1) / stride;
  for (long it = 0; it < iters; ++it) {
    const long i = first + it * stride;
    const bool ok = i < n;
    cf.add(ok, ok ? (int)pred[i] : -1, ok ? load_label(labels, lbytes, i) : -2);
  }
  stage_counts(cf.c, s_cnt);
  __syncthreads();
  commit_counts<9>(s_cnt, counts, 0);
}

}  // namespace dc

using namespace dc;

extern "C" int dc_wce_fused(int B, int H, int W, const float* logits_nchw, const void* labels, int label_dtype_bytes,
                            const float* class_weights, float grad_scale, double* loss_sum, float* dlogits,
                            int64_t* pred, int64_t* counts, void* stream) {
  DC_REQUIRE(logits_nchw && labels && class_weights && B > 0 && H > 0 && W > 0, "dc_wce_fused: bad argument");
  DC_REQUIRE(label_dtype_bytes == 1 || label_dtype_bytes == 4 || label_dtype_bytes == 8, "dc_wce_fused: labels must be uint8, int32 or int64");
  const long total = (long)B * H * W;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(wce_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, B, (long)H * W, logits_nchw, labels,
                     label_dtype_bytes, class_weights, grad_scale, loss_sum, dlogits, pred, (unsigned long long*)counts);
  DC_CHECK_LAUNCH();
  return 0;
}

extern "C" int dc_wce_score(int B, int n_valid, int H, int W, const float* logits_nchw, const void* labels, int label_dtype_bytes,
                            const float* class_weights, double* loss_sum, int64_t* counts, void* stream) {
  DC_REQUIRE(logits_nchw && labels && class_weights && loss_sum && counts && B > 0 && H > 0 && W > 0, "dc_wce_score: bad argument");
  DC_REQUIRE(n_valid >= 0 && n_valid <= B, "dc_wce_score: n_valid must lie in [0, B]");
  DC_REQUIRE(label_dtype_bytes == 1 || label_dtype_bytes == 4 || label_dtype_bytes == 8, "dc_wce_score: labels must be uint8, int32 or int64");
  if (n_valid == 0) return 0;
  const long HW = (long)H * W;
  long blocks = (HW + 255) / 256;
  const long cap = (2048 + n_valid - 1) / n_valid;      // dc_wce_fused's 2048 workgroups, shared between the samples
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(wce_score_kernel, dim3((int)blocks, n_valid), dim3(256), 0, (hipStream_t)stream, HW, logits_nchw, labels,
                     label_dtype_bytes, class_weights, loss_sum, (unsigned long long*)counts);
  DC_CHECK_LAUNCH();
  return 0;
}

extern "C" int dc_logits_predict(int B, int n_valid, int H, int W, const float* logits_nchw, uint8_t* mask, float* conf, int64_t* class_counts,
                                 void* stream) {
  DC_REQUIRE(logits_nchw && mask && B > 0 && H > 0 && W > 0, "dc_logits_predict: bad argument");
  DC_REQUIRE(n_valid >= 0 && n_valid <= B, "dc_logits_predict: n_valid must lie in [0, B]");
  if (n_valid == 0) return 0;
  const long HW = (long)H * W;
  long blocks = (HW + 255) / 256;
  const long cap = (2048 + n_valid - 1) / n_valid;      // dc_wce_score's share of workgroups per sample
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(logits_predict_kernel, dim3((int)blocks, n_valid), dim3(256), 0, (hipStream_t)stream, HW, logits_nchw, mask, conf,
                     (unsigned long long*)class_counts);
  DC_CHECK_LAUNCH();
  return 0;
}

extern "C" int dc_val_accumulate(int B, int n_valid, long HW, const double* loss_sum, const int64_t* counts, double* acc,
                                 double* per_sample, void* stream) {
  DC_REQUIRE(loss_sum && counts && acc && B > 0 && HW > 0, "dc_val_accumulate: bad argument");
  DC_REQUIRE(n_valid >= 0 && n_valid <= B, "dc_val_accumulate: n_valid must lie in [0, B]");
  if (n_valid == 0) return 0;
  hipLaunchKernelGGL(val_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, n_valid, HW, loss_sum, (const long long*)counts,
                     acc, per_sample);
  DC_CHECK_LAUNCH();
  return 0;
}

extern "C" int dc_confusion_counts(long n, const int64_t* pred, const void* labels, int label_dtype_bytes,
                                   int64_t* counts, void* stream) {
  DC_REQUIRE(pred && labels && counts && n > 0, "dc_confusion_counts: bad argument");
  DC_REQUIRE(label_dtype_bytes == 1 || label_dtype_bytes == 4 || label_dtype_bytes == 8, "dc_confusion_counts: labels must be uint8, int32 or int64");
  long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(confusion_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, n, pred, labels,
                     label_dtype_bytes, (unsigned long long*)counts);
  DC_CHECK_LAUNCH();
  return 0;
}
