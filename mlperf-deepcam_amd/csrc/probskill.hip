// Probabilistic verification: the joint histogram behind reliability diagram, Brier score and ROC (dc_prob_score; nn.ProbabilitySkill).
// Per pixel and class c the softmax probability p_c becomes the integer q_c = rint(p_c * 65536); from there on everything is an integer:
// the bin (q_c * K) >> 16, the outcome o_c = (label == c), the cell's count and sum of q, the squared error (q_c - o_c * 65536)^2.
// include/deepcam_hip.h has the definition; this file has the decomposition: one streaming pass between two small launches.
//   prob_zero   zeroes hist and the rows and pixels of the samples < n_valid.
//   prob_hist   A workgroup takes PS_CHUNK consecutive pixels of one sample (blockIdx.y), in PS_CHUNK / PS_PASS passes of 4 pixels per
//               thread.  The vector form (H * W a multiple of 4 and aligned bases) gives a thread 4 NEIGHBOURING pixels by one 16-byte load
//               per plane; the scalar form gives it 4 pixels a workgroup's width apart by 4-byte loads, for every other H * W.  Both end
//               with the same 4 x (q0, q1, q2, label) in registers and share everything behind the loads.
//               The histogram is private to the workgroup, in LDS: [3][2][K] cells of 64 bits, the sum of q in the low 40 bits and the
//               count above them, so that a cell is ONE ds_add_u64 and neither field can wrap (a workgroup sees PS_CHUNK = 2^13 pixels:
//               the sum stays below 2^29, the count below 2^14).  Real frames are > 95 % background: nearly every lane of nearly every
//               wave wants the same three cells, and same-address LDS atomics serialise over the lanes.  So per class the wave takes
//               the cell of its first scored pixel as the reference and counts by ballot how many of its scored pixels (4 per lane)
//               fall into it; if they are PS_MIN_AGG or more, their count is the popcount of the ballots, their sum of q goes through
//               one wave reduction and ONE lane adds for all of them.  Every other pixel is added by its own lane: the pixels of an
//               event inside a wave of background, or all of them where no cell gathers enough.  The workgroup flushes its non-zero
//               cells with 64-bit global atomics, once.
//               The three squared-error sums and the three pixel counters are reduced in registers, then over the wave, then through
//               pixel_score.h's stage / commit into rows[b] and pixels[b].
//   prob_total  total_hist += hist cell by cell; one thread per class walks the samples in order and adds rows[b][c] to the two-word
//               total (lo += x, hi += carry); three threads add the pixel counters, one the frame count.
// Integer sums only: the state does not depend on the schedule or on how the frames are cut into batches.
#include "common.h"
#include "pixel_score.h"

namespace dc {

static constexpr int PS_THREADS = 256;
static constexpr int PS_PASS = PS_THREADS * 4;      // pixels of one pass of a workgroup
static constexpr int PS_PASSES = 8;
static constexpr int PS_CHUNK = PS_PASS * PS_PASSES;   // pixels of a workgroup: 2^13, so a cell's sum of q < 2^29 and its count < 2^14
static constexpr int PS_KMAX = 256;
static constexpr int PS_BMAX = 4095;                // B stays a legal grid.y
static constexpr int PS_NSHIFT = 40;                // an LDS cell: count << 40 | sum q
static constexpr unsigned PS_MIN_AGG = 16;          // fewest pixels of a wave in one cell that are worth a wave reduction
static constexpr unsigned long long PS_QMASK = (1ull << PS_NSHIFT) - 1;

__device__ inline unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(PS_THREADS) void prob_hist_kernel(long HW, const float* __restrict__ logits, const void* __restrict__ labels,
                                                               int lbytes, int K, unsigned long long* __restrict__ hist,
                                                               unsigned long long* __restrict__ rows, unsigned long long* __restrict__ pixels) {
  __shared__ unsigned long long cells[NC * 2 * PS_KMAX];
  __shared__ unsigned long long s_sq[4 * NC], s_px[4 * NC];
  const int t = threadIdx.x, b = blockIdx.y;
  const int ncell = NC * 2 * K;
  for (int i = t; i < ncell; i += PS_THREADS) cells[i] = 0;
  __syncthreads();
  const float* lb = logits + (size_t)b * NC * HW;
  const size_t lab0 = (size_t)b * HW;
  const long base = (long)blockIdx.x * PS_CHUNK;
  unsigned long long sq[NC] = {0, 0, 0};            // this lane's sums of (q_c - o_c * 65536)^2: at most 32 terms of 2^32
  unsigned long long px[NC] = {0, 0, 0};            // wave-uniform: scored, bad label, logit not finite
  // Every trip count below is the same for all lanes of a workgroup: the ballots and shuffles see whole waves.
  for (int pass = 0; pass < PS_PASSES; ++pass) {
    const long p0 = base + (long)pass * PS_PASS;
    if (p0 >= HW) break;
    float l[NC][4];
    int y[4];
    bool ok[4];
    if (VEC) {                                      // HW % 4 == 0: the four pixels are all inside or all outside
      const long p = p0 + 4 * t;
      const bool in = p < HW;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) v = *reinterpret_cast<const float4*>(lb + (size_t)c * HW + p);
        l[c][0] = v.x, l[c][1] = v.y, l[c][2] = v.z, l[c][3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) ok[j] = in, y[j] = in ? load_label(labels, lbytes, lab0 + p + j) : -1;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long p = p0 + j * PS_THREADS + t;
        ok[j] = p < HW;
        l[0][j] = l[1][j] = l[2][j] = 0.f;
        y[j] = -1;
        if (ok[j]) {
          l[0][j] = lb[p], l[1][j] = lb[HW + p], l[2][j] = lb[2 * HW + p];
          y[j] = load_label(labels, lbytes, lab0 + p);
        }
      }
    }
    int q[NC][4];
    bool sc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool badl = ok[j] && y[j] < 0;
      const bool nonf = ok[j] && y[j] >= 0 && !logits_finite(l[0][j], l[1][j], l[2][j]);
      sc[j] = ok[j] && !badl && !nonf;
      px[0] += wave_count(sc[j]), px[1] += wave_count(badl), px[2] += wave_count(nonf);
      const ProbQ pq = prob_q(l[0][j], l[1][j], l[2][j]);
      q[0][j] = pq.q0, q[1][j] = pq.q1, q[2][j] = pq.q2;
    }
    const unsigned long long any = __ballot(sc[0] || sc[1] || sc[2] || sc[3]);
    if (any == 0) continue;                         // wave-uniform
    const int first_lane = __ffsll((long long)any) - 1;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int cell[4];
      bool left[4];                                 // scored and not added yet
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = y[j] == c;
        int bin = (q[c][j] * K) >> 16;
        bin = bin < K - 1 ? bin : K - 1;
        cell[j] = (c * 2 + o) * K + bin;
        left[j] = sc[j];
        if (sc[j]) {
          const long long d = (long long)q[c][j] - (o ? 65536 : 0);
          sq[c] += (unsigned long long)(d * d);
        }
      }
      // The cell of the wave's first scored pixel is the reference -- on real frames the background's.  If at least PS_MIN_AGG of the
      // wave's pixels are in it, they leave through one wave reduction and one add by one lane.  Every condition is wave-uniform.
      const int mine = sc[0] ? cell[0] : (sc[1] ? cell[1] : (sc[2] ? cell[2] : cell[3]));
      const int ref = __shfl(mine, first_lane, 64);
      bool in[4];
      unsigned n = 0, qs = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        in[j] = sc[j] && cell[j] == ref;
        n += (unsigned)wave_count(in[j]);
        qs += in[j] ? (unsigned)q[c][j] : 0u;
      }
      if (n >= PS_MIN_AGG) {
        const unsigned total = wave_sum_u32(qs);    // n <= 256, total <= 2^24
        if ((t & 63) == 0) atomicAdd(&cells[ref], ((unsigned long long)n << PS_NSHIFT) | total);
#pragma unroll
        for (int j = 0; j < 4; ++j) left[j] = left[j] && !in[j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (left[j]) atomicAdd(&cells[cell[j]], (1ull << PS_NSHIFT) | (unsigned long long)q[c][j]);
    }
  }
  __syncthreads();
  for (int i = t; i < ncell; i += PS_THREADS) {
    const unsigned long long v = cells[i];
    if (v) {
      atomicAdd(hist + 2 * (size_t)i, v >> PS_NSHIFT);
      if (v & PS_QMASK) atomicAdd(hist + 2 * (size_t)i + 1, v & PS_QMASK);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) sq[c] = wave_sum_u64(sq[c]);
  stage_counts(sq, s_sq);
  stage_counts(px, s_px);
  __syncthreads();
  commit_counts<NC>(s_sq, rows, b);
  commit_counts<NC>(s_px, pixels, b);
}

// hist and the rows and pixels of the samples < n_valid, zeroed in ONE launch (three memsets would be three)
__global__ __launch_bounds__(256) void prob_zero_kernel(int ncell2, int nrow, long long* __restrict__ hist, long long* __restrict__ rows,
                                                        long long* __restrict__ pixels) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncell2) hist[i] = 0;
  else if (i < ncell2 + nrow) rows[i - ncell2] = 0;
  else if (i < ncell2 + 2 * nrow) pixels[i - ncell2 - nrow] = 0;
}

__global__ __launch_bounds__(256) void prob_total_kernel(int n_valid, int ncell2, const long long* __restrict__ hist,
                                                         const unsigned long long* __restrict__ rows, const long long* __restrict__ pixels,
                                                         long long* __restrict__ total_hist, unsigned long long* __restrict__ total_sq,
                                                         long long* __restrict__ total_pixels, long long* __restrict__ frames) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncell2) {
    const long long v = hist[i];
    if (v) total_hist[i] += v;
  } else if (i < ncell2 + NC) {
    total_add128(total_sq, rows, NC, i - ncell2, n_valid);
  } else if (i < ncell2 + 2 * NC) {
    total_add64(total_pixels, pixels, NC, i - ncell2 - NC, n_valid);
  } else if (i == ncell2 + 2 * NC) {
    frames[0] += n_valid;
  }
}

}  // namespace dc

using namespace dc;

extern "C" int dc_prob_block(int* pixels, int* max_groups) {
  DC_REQUIRE(pixels && max_groups, "dc_prob_block: null argument");
  *pixels = PS_CHUNK;
  *max_groups = 0;                                  // no cap: a workgroup takes one chunk and ends
  return 0;
}

extern "C" int dc_prob_score(int B, int n_valid, int H, int W, const float* logits_nchw, const void* labels, int label_bytes, int K,
                             int64_t* hist, int64_t* rows, int64_t* pixels, int64_t* total_hist, int64_t* total_sq, int64_t* total_pixels,
                             int64_t* frames, void* stream) {
  DC_REQUIRE(B >= 1 && B <= PS_BMAX && H >= 1 && W >= 1, "dc_prob_score: B must lie in [1, 4095], H and W must be positive");
  DC_REQUIRE((long)H * W <= (1L << 30), "dc_prob_score: H * W must not exceed 2^30");
  DC_REQUIRE(n_valid >= 0 && n_valid <= B, "dc_prob_score: n_valid must lie in [0, B]");
  DC_REQUIRE(label_bytes == 1 || label_bytes == 4 || label_bytes == 8, "dc_prob_score: label_bytes must be 1, 4 or 8");
  DC_REQUIRE(K >= 1 && K <= PS_KMAX, "dc_prob_score: K must lie in [1, 256]");
  DC_REQUIRE(logits_nchw && labels && hist && rows && pixels && total_hist && total_sq && total_pixels && frames, "dc_prob_score: null pointer");
  DC_REQUIRE(((uintptr_t)logits_nchw & 3) == 0 && ((uintptr_t)labels & (label_bytes - 1)) == 0,
             "dc_prob_score: logits or labels not aligned to their element size");
  DC_REQUIRE(((uintptr_t)hist & 7) == 0 && ((uintptr_t)rows & 7) == 0 && ((uintptr_t)pixels & 7) == 0 && ((uintptr_t)total_hist & 7) == 0 &&
                 ((uintptr_t)total_sq & 7) == 0 && ((uintptr_t)total_pixels & 7) == 0 && ((uintptr_t)frames & 7) == 0,
             "dc_prob_score: hist, rows, pixels or a total not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  const int ncell2 = NC * 2 * K * 2;
  const int nrow = n_valid * NC;
  hipLaunchKernelGGL(prob_zero_kernel, dim3((ncell2 + 2 * nrow + 255) / 256), dim3(256), 0, st, ncell2, nrow, (long long*)hist, (long long*)rows,
                     (long long*)pixels);
  DC_LAUNCHED("prob_zero");
  if (n_valid == 0) return 0;                       // nothing to read, nothing to add
  const long HW = (long)H * W;
  const unsigned gx = (unsigned)((HW + PS_CHUNK - 1) / PS_CHUNK);
  // 16-byte loads: planes 1 and 2 and every sample start a multiple of HW floats in
  const bool vec = HW % 4 == 0 && ((uintptr_t)logits_nchw & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(prob_hist_kernel<true>, dim3(gx, n_valid), dim3(PS_THREADS), 0, st, HW, logits_nchw, labels, label_bytes, K,
                       (unsigned long long*)hist, (unsigned long long*)rows, (unsigned long long*)pixels);
  else
    hipLaunchKernelGGL(prob_hist_kernel<false>, dim3(gx, n_valid), dim3(PS_THREADS), 0, st, HW, logits_nchw, labels, label_bytes, K,
                       (unsigned long long*)hist, (unsigned long long*)rows, (unsigned long long*)pixels);
  DC_LAUNCHED(vec ? "prob_hist_vec" : "prob_hist");
  hipLaunchKernelGGL(prob_total_kernel, dim3((ncell2 + 2 * NC + 1 + 255) / 256), dim3(256), 0, st, n_valid, ncell2, (const long long*)hist,
                     (const unsigned long long*)rows, (const long long*)pixels, (long long*)total_hist, (unsigned long long*)total_sq,
                     (long long*)total_pixels, (long long*)frames);
  DC_LAUNCHED("prob_total");
  return 0;
}
