// The decision rule: per-class probability thresholds with hysteresis, from the stored logits to a mask (dc_logits_decide,
// dc_hysteresis_select; nn.DecisionRule; predict.py --decision_low / --decision_high / --decision_from).
// Definitions (include/deepcam_hip.h has them with the ABI; tests/util_decide.py states them again in numpy):
//   q_c        pixel_score.h's prob_q: rint(softmax_c * 65536) in fp32, the integer dc_prob_score bins and scores.
//   the rule   four integers in [0, 65537], low[1], low[2], high[1], high[2], high[c] >= low[c]; 65537 is "never" (q <= 65536).
//   candidate  class c in {1, 2} QUALIFIES iff q_c >= low[c].  cand = 0 if neither qualifies, the one that does if only one does, and the
//              class with the larger q if both do -- class 1 on equal q.
//   seed       cand = c != 0 and q_c >= high[c].  The class that lost a conflict seeds nothing.
//   non-finite a pixel with a logit that is NaN or an infinity is background, seeds nothing and is counted.
//   out        out[p] = cand[p] iff the connected component of cand that holds p (dc_mask_components: one class, connectivity 4 or 8,
//              periodic columns with wrap, rows never) holds a seed; else 0.  high == low: every candidate is a seed, out == cand, and the
//              caller runs no component pass -- plain thresholding.
// The decomposition:
//   decide_q / decide_q_vec   one streaming pass over the logits in prob_hist's layout: a workgroup takes DQ_CHUNK consecutive pixels of one
//                 sample (blockIdx.y) in passes of 4 pixels per thread and ends.  The vector form (H * W a multiple of 4, aligned bases)
//                 gives a thread 4 NEIGHBOURING pixels by one 16-byte load per plane and stores cand and seed as one 32-bit word each;
//                 the scalar form gives it 4 pixels a workgroup's width apart by 4-byte loads and stores bytes.  Six counters (candidate
//                 and seed pixels per class, non-finite pixels, conflicts) go through ballots, wave-uniform, then pixel_score.h's stage /
//                 commit: twelve-word rows, the words the select pass fills staged as zeros.  No per-pixel atomics, no LDS beyond the stage.
//   decide_mark   every seed pixel stores 1 at flags[label - 1], the byte of its component's root.  All writers of a byte write the same
//                 value: a plain store, no atomic.  A pixel reads the byte first and skips the store where it already stands -- a frame
//                 that is ONE component of seeds would otherwise send H * W stores to one address.
//   decide_select out = flags[label - 1] ? cand : 0; kept pixels per class, and at root pixels (label - 1 == the pixel's own index) the
//                 candidate and kept events per class.  Per-lane counters, one wave reduction, stage / commit.
// flags is indexed by ROOT, not by a rank: nothing here has an event cap.
#include "common.h"
#include "pixel_score.h"

namespace dc {

static constexpr int DQ_THREADS = 256;
static constexpr int DQ_PASS = DQ_THREADS * 4;      // pixels of one pass of a workgroup
static constexpr int DQ_PASSES = 8;
static constexpr int DQ_CHUNK = DQ_PASS * DQ_PASSES;
static constexpr int DQ_BMAX = 4095;                // B stays a legal grid.y
static constexpr int DQ_NEVER = 65537;
static constexpr int DQ_COUNTS = 12;                // per class candidate, seed, kept pixels, candidate, kept events; non-finite; conflicts

struct DecideRule {
  int low1, low2, high1, high2;
};

struct Decided {
  uint8_t cand, seed;
  bool nonfinite, both;
};
// one pixel: ok = the lane has one (a lane without decides nothing and counts nowhere)
__device__ inline Decided decide_pixel(bool ok, float l0, float l1, float l2, const DecideRule& r) {
  Decided d{0, 0, false, false};
  if (!ok) return d;
  if (!logits_finite(l0, l1, l2)) {
    d.nonfinite = true;
    return d;
  }
  const ProbQ q = prob_q(l0, l1, l2);
  const bool a1 = q.q1 >= r.low1, a2 = q.q2 >= r.low2;
  d.both = a1 && a2;
  const int c = d.both ? (q.q2 > q.q1 ? 2 : 1) : (a1 ? 1 : (a2 ? 2 : 0));
  d.cand = (uint8_t)c;
  d.seed = (uint8_t)((c == 1 && q.q1 >= r.high1) || (c == 2 && q.q2 >= r.high2));
  return d;
}

template <bool VEC>
__global__ __launch_bounds__(DQ_THREADS) void decide_q_kernel(long HW, const float* __restrict__ logits, DecideRule rule,
                                                              uint8_t* __restrict__ cand, uint8_t* __restrict__ seed,
                                                              unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_n[4 * DQ_COUNTS];
  const int t = threadIdx.x, b = blockIdx.y;
  const float* lb = logits + (size_t)b * NC * HW;
  uint8_t* cb = cand + (size_t)b * HW;
  uint8_t* sb = seed ? seed + (size_t)b * HW : nullptr;
  const long base = (long)blockIdx.x * DQ_CHUNK;
  unsigned long long n[DQ_COUNTS] = {};             // wave-uniform; words 2-4 and 7-9 stay 0 here
  // The trip count is the same for all lanes of a workgroup: the ballots see whole waves.
  for (int pass = 0; pass < DQ_PASSES; ++pass) {
    const long p0 = base + (long)pass * DQ_PASS;
    if (p0 >= HW) break;
    Decided d[4];
    if (VEC) {                                      // HW % 4 == 0: the four pixels are all inside or all outside
      const long p = p0 + 4 * t;
      const bool in = p < HW;
      float l[NC][4];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) v = *reinterpret_cast<const float4*>(lb + (size_t)c * HW + p);
        l[c][0] = v.x, l[c][1] = v.y, l[c][2] = v.z, l[c][3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = decide_pixel(in, l[0][j], l[1][j], l[2][j], rule);
      if (in) {
        *reinterpret_cast<uchar4*>(cb + p) = make_uchar4(d[0].cand, d[1].cand, d[2].cand, d[3].cand);
        if (sb) *reinterpret_cast<uchar4*>(sb + p) = make_uchar4(d[0].seed, d[1].seed, d[2].seed, d[3].seed);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long p = p0 + j * DQ_THREADS + t;
        const bool in = p < HW;
        float l0 = 0.f, l1 = 0.f, l2 = 0.f;
        if (in) l0 = lb[p], l1 = lb[HW + p], l2 = lb[2 * HW + p];
        d[j] = decide_pixel(in, l0, l1, l2, rule);
        if (in) {
          cb[p] = d[j].cand;
          if (sb) sb[p] = d[j].seed;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      n[0] += wave_count(d[j].cand == 1), n[1] += wave_count(d[j].seed && d[j].cand == 1);
      n[5] += wave_count(d[j].cand == 2), n[6] += wave_count(d[j].seed && d[j].cand == 2);
      n[10] += wave_count(d[j].nonfinite), n[11] += wave_count(d[j].both);
    }
  }
  stage_counts(n, s_n);
  __syncthreads();
  commit_counts<DQ_COUNTS>(s_n, counts, b);
}

// DS_PX pixels per thread, as dc_mask_select: with `vec` (HW a multiple of 4, aligned bases) one 4-byte load of a byte plane and one 16-byte
// load of the labels, else single bytes and words
static constexpr int DS_PX = 4;

__device__ inline void mark_pixel(uint8_t s, int label, long HW, uint8_t* flags) {
  if (s && (unsigned long)(label - 1) < (unsigned long)HW && !flags[label - 1]) flags[label - 1] = 1;
}

__global__ __launch_bounds__(256) void decide_mark_kernel(long HW, int vec, const uint8_t* __restrict__ seed, const int* __restrict__ labels,
                                                          uint8_t* flags) {
  const size_t base = (size_t)blockIdx.y * HW;
  uint8_t* fl = flags + base;
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * DS_PX;
  if (vec && p0 + DS_PX <= HW) {
    const uchar4 s = *(const uchar4*)(seed + base + p0);
    if (s.x | s.y | s.z | s.w) {                    // most pixels seed nothing: their labels are not read
      const int4 l = *(const int4*)(labels + base + p0);
      mark_pixel(s.x, l.x, HW, fl), mark_pixel(s.y, l.y, HW, fl), mark_pixel(s.z, l.z, HW, fl), mark_pixel(s.w, l.w, HW, fl);
    }
  } else {
    for (int j = 0; j < DS_PX; ++j) {
      const long p = p0 + j;
      if (p < HW && seed[base + p]) mark_pixel(1, labels[base + p], HW, fl);
    }
  }
}

// v: kept pixels, candidate events, kept events of class 1, then of class 2
__device__ inline uint8_t select_pixel(uint8_t m, int label, long p, long HW, const uint8_t* flags, unsigned (&v)[6]) {
  if ((m != 1 && m != 2) || (unsigned long)(label - 1) >= (unsigned long)HW) return 0;
  const bool kept = flags[label - 1] != 0, root = (long)label - 1 == p;
  const int o = m == 1 ? 0 : 3;
#pragma unroll
  for (int i = 0; i < 6; i += 3) {                  // (constant indices: the counters stay in registers)
    v[i] += (o == i && kept) ? 1u : 0u;
    v[i + 1] += (o == i && root) ? 1u : 0u;
    v[i + 2] += (o == i && root && kept) ? 1u : 0u;
  }
  return kept ? m : (uint8_t)0;
}

__global__ __launch_bounds__(256) void decide_select_kernel(long HW, int vec, const uint8_t* __restrict__ cand, const int* __restrict__ labels,
                                                            const uint8_t* __restrict__ flags, uint8_t* __restrict__ out_mask,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_n[4 * DQ_COUNTS];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * HW;
  const uint8_t* fl = flags + base;
  unsigned v[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * DS_PX;
  if (vec && p0 + DS_PX <= HW) {
    const uchar4 m = *(const uchar4*)(cand + base + p0);
    uchar4 o = make_uchar4(0, 0, 0, 0);
    if (m.x | m.y | m.z | m.w) {                    // background reads no labels
      const int4 l = *(const int4*)(labels + base + p0);
      o.x = select_pixel(m.x, l.x, p0, HW, fl, v);
      o.y = select_pixel(m.y, l.y, p0 + 1, HW, fl, v);
      o.z = select_pixel(m.z, l.z, p0 + 2, HW, fl, v);
      o.w = select_pixel(m.w, l.w, p0 + 3, HW, fl, v);
    }
    *(uchar4*)(out_mask + base + p0) = o;
  } else {
    for (int j = 0; j < DS_PX; ++j) {
      const long p = p0 + j;
      if (p < HW) {
        const uint8_t m = cand[base + p];
        out_mask[base + p] = m ? select_pixel(m, labels[base + p], p, HW, fl, v) : (uint8_t)0;
      }
    }
  }
  unsigned long long n[DQ_COUNTS] = {};             // every lane reaches the shuffles: nothing above returns
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    unsigned x = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    n[(i / 3) * 5 + 2 + i % 3] = x;                 // words 2, 3, 4 and 7, 8, 9
  }
  stage_counts(n, s_n);
  __syncthreads();
  commit_counts<DQ_COUNTS>(s_n, counts, b);
}

static int decide_check(int B, int n_valid, int H, int W) {
  DC_REQUIRE(B >= 1 && B <= DQ_BMAX && H >= 1 && W >= 1, "decide: B must lie in [1, 4095], H and W must be positive");
  DC_REQUIRE((long)H * W <= (1L << 30), "decide: H * W must not exceed 2^30");
  DC_REQUIRE(n_valid >= 0 && n_valid <= B, "decide: n_valid must lie in [0, B]");
  return 0;
}

static bool disjoint(const void* a, const void* b, size_t bytes) {
  return (uintptr_t)a + bytes <= (uintptr_t)b || (uintptr_t)b + bytes <= (uintptr_t)a;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_decide_block(int* pixels) {
  DC_REQUIRE(pixels, "dc_decide_block: null argument");
  *pixels = DQ_CHUNK;
  return 0;
}

// the flags plane of dc_hysteresis_select: one byte per pixel, indexed by root
extern "C" size_t dc_decide_workspace(int B, int H, int W) {
  if (B < 1 || B > DQ_BMAX || H < 1 || W < 1 || (long)H * W > (1L << 30)) return 0;
  return ((size_t)B * H * W + 255) & ~(size_t)255;
}

extern "C" int dc_logits_decide(int B, int n_valid, int H, int W, const float* logits_nchw, int low1, int low2, int high1, int high2,
                                uint8_t* cand, uint8_t* seed, int64_t* counts, void* stream) {
  if (int rc = decide_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(low1 >= 0 && low1 <= DQ_NEVER && low2 >= 0 && low2 <= DQ_NEVER && high1 >= 0 && high1 <= DQ_NEVER && high2 >= 0 &&
                 high2 <= DQ_NEVER, "dc_logits_decide: every threshold must lie in [0, 65537]");
  DC_REQUIRE(high1 >= low1 && high2 >= low2, "dc_logits_decide: a high threshold must not be below its low threshold");
  DC_REQUIRE(logits_nchw && cand && counts, "dc_logits_decide: null pointer");
  DC_REQUIRE(seed || (high1 == low1 && high2 == low2), "dc_logits_decide: seed may be null only where high == low for both classes");
  DC_REQUIRE(((uintptr_t)logits_nchw & 3) == 0 && ((uintptr_t)counts & 7) == 0, "dc_logits_decide: logits or counts not aligned to their element size");
  const long HW = (long)H * W;
  DC_REQUIRE(!seed || disjoint(cand, seed, (size_t)B * HW), "dc_logits_decide: seed may not alias cand");
  if (n_valid == 0) return 0;                       // nothing to read, nothing to write
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_valid * DQ_COUNTS * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const unsigned gx = (unsigned)((HW + DQ_CHUNK - 1) / DQ_CHUNK);
  // 16-byte loads and 32-bit stores: planes 1 and 2 and every sample start a multiple of HW elements in
  const bool vec = HW % 4 == 0 && ((uintptr_t)logits_nchw & 15) == 0 && ((uintptr_t)cand & 3) == 0 && ((uintptr_t)seed & 3) == 0;
  const DecideRule rule{low1, low2, high1, high2};
  if (vec)
    hipLaunchKernelGGL(decide_q_kernel<true>, dim3(gx, n_valid), dim3(DQ_THREADS), 0, st, HW, logits_nchw, rule, cand, seed,
                       (unsigned long long*)counts);
  else
    hipLaunchKernelGGL(decide_q_kernel<false>, dim3(gx, n_valid), dim3(DQ_THREADS), 0, st, HW, logits_nchw, rule, cand, seed,
                       (unsigned long long*)counts);
  DC_LAUNCHED(vec ? "decide_q_vec" : "decide_q");
  return 0;
}

extern "C" int dc_hysteresis_select(int B, int n_valid, int H, int W, const uint8_t* cand, const uint8_t* seed, const int32_t* labels,
                                    uint8_t* flags, uint8_t* out_mask, int64_t* counts, void* stream) {
  if (int rc = decide_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(cand && seed && labels && flags && out_mask && counts, "dc_hysteresis_select: null pointer");
  DC_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)counts & 7) == 0, "dc_hysteresis_select: labels or counts not aligned to their element size");
  const long HW = (long)H * W;
  const size_t bytes = (size_t)B * HW;
  DC_REQUIRE(disjoint(out_mask, cand, bytes), "dc_hysteresis_select: out_mask may not alias cand");
  DC_REQUIRE(disjoint(flags, cand, bytes) && disjoint(flags, seed, bytes) && disjoint(flags, out_mask, bytes) && disjoint(out_mask, seed, bytes),
             "dc_hysteresis_select: flags and out_mask may not alias another plane");
  if (n_valid == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)n_valid * HW, st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const int vec = HW % 4 == 0 && ((uintptr_t)cand & 3) == 0 && ((uintptr_t)seed & 3) == 0 && ((uintptr_t)out_mask & 3) == 0 &&
                  ((uintptr_t)labels & 15) == 0;
  const unsigned blocks = (unsigned)((HW + 256 * DS_PX - 1) / (256 * DS_PX));
  hipLaunchKernelGGL(decide_mark_kernel, dim3(blocks, n_valid), dim3(256), 0, st, HW, vec, seed, labels, flags);
  DC_LAUNCHED("decide_mark");
  hipLaunchKernelGGL(decide_select_kernel, dim3(blocks, n_valid), dim3(256), 0, st, HW, vec, cand, labels, flags, out_mask,
                     (unsigned long long*)counts);
  DC_LAUNCHED("decide_select");
  return 0;
}
