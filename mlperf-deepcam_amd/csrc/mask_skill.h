// What the kernels that read class masks share, written once: the mask-element reader, the running totals of the verification skills,
// and the argument checks their entry points open with.
//   readers    climatology.hip, render.hip, fss.hip, distance.hip, displacement.hip, scale.hip; pixel_score.h's load_label
//   totals     the *_total_kernel of fss.hip, distance.hip, displacement.hip, scale.hip and probskill.hip
//   checks     dc_fss_score, dc_distance_score, dc_displacement_score, dc_scale_score
// A kernel keeps its own grid, block size and launch name; an entry point keeps the requirements that are its own.
// One difference between the four entry points is DELIBERATE: dc_fss_score zeroes rows and pixels of all B frames, and before it looks
// at n_valid, because nn.FractionsSkill documents of the padding frames that "their rows are zero".  The other three promise nothing
// about them: they zero the frames < n_valid only, and nothing at n_valid = 0.
#pragma once
#include <cstdio>
#include "common.h"

namespace dc {

// one element of a mask of 1-, 4- or 8-byte integers, at full width: the ONLY switch on the element size
__device__ inline long long mask_value(const void* m, size_t i, int bytes) {
  long long v;
  if (bytes == 1) v = ((const uint8_t*)m)[i];
  else if (bytes == 4) v = ((const int32_t*)m)[i];
  else v = ((const long long*)m)[i];
  return v;
}
// its class: 1 or 2 for the full-width values 1 and 2, 0 (background) for every other
__device__ inline unsigned mask_class(const void* m, size_t i, int bytes) {
  const long long v = mask_value(m, i, bytes);
  return v == 1 ? 1u : (v == 2 ? 2u : 0u);
}
// its two indicator bits in 16-bit lanes: (value == 1) | (value == 2) << 16
__device__ inline unsigned mask_bits(const void* m, size_t i, int bytes) {
  const long long v = mask_value(m, i, bytes);
  return v == 1 ? 1u : (v == 2 ? 0x10000u : 0u);
}

// One cell of a two-word running total: (total_words[2 cell], total_words[2 cell + 1]) = (lo, hi) takes rows[b * stride + cell] of the
// frames b < n_valid, in frame order.  One thread per cell.
__device__ inline void total_add128(unsigned long long* __restrict__ total_words, const unsigned long long* __restrict__ rows, int stride,
                                    int cell, int n_valid) {
  unsigned long long lo = total_words[2 * cell], hi = total_words[2 * cell + 1];
  for (int b = 0; b < n_valid; ++b) {
    const unsigned long long x = rows[(size_t)b * stride + cell];
    lo += x;
    hi += lo < x;                                   // the carry
  }
  total_words[2 * cell] = lo, total_words[2 * cell + 1] = hi;
}
// ... and of a one-word total
__device__ inline void total_add64(long long* __restrict__ total, const long long* __restrict__ rows, int stride, int cell, int n_valid) {
  long long sum = 0;
  for (int b = 0; b < n_valid; ++b) sum += rows[(size_t)b * stride + cell];
  total[cell] += sum;
}

// The requirements every dc_*_score over two masks opens with; `fn` is the entry point, so the message names the function that was
// called.  0, or dc_fail's code.  The caller's own requirements follow, all of them in front of its first memset or launch.
inline int mask_skill_check(const char* fn, int B, int bmax, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth,
                            int truth_bytes, int row0, int row1) {
  const auto ok_bytes = [](int b) { return b == 1 || b == 4 || b == 8; };
  char range[64];
  snprintf(range, sizeof(range), "B must lie in [1, %d], H and W must be positive", bmax);
  const char* what = B < 1 || B > bmax || H < 1 || W < 1                ? range
                     : (long)H * W >= 2147483648L                        ? "H * W must be below 2^31"
                     : n_valid < 0 || n_valid > B                        ? "n_valid must lie in [0, B]"
                     : !ok_bytes(pred_bytes) || !ok_bytes(truth_bytes)   ? "mask_bytes must be 1, 4 or 8 on either side"
                     : row0 < 0 || row0 >= row1 || row1 > H              ? "the row range must satisfy 0 <= row0 < row1 <= H"
                     : !pred || !truth                                   ? "null pointer"
                     : ((uintptr_t)pred & (pred_bytes - 1)) || ((uintptr_t)truth & (truth_bytes - 1))
                         ? "a mask is not aligned to its element size"
                         : nullptr;
  if (!what) return 0;
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", fn, what);
  return dc_fail(msg, __FILE__, __LINE__);
}

}  // namespace dc
