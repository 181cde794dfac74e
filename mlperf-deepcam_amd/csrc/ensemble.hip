// The view ensemble: test-time augmentation on a periodic grid (dc_input_view_hwc, dc_ensemble_add, dc_ensemble_pool; nn.ViewEnsemble,
// nn.view_input; predict.py --ensemble_rolls / --ensemble_flip_lat / --ensemble_negate / --ensemble_seam_margin).  The network pads the first
// and the last column with zeros while everything behind it takes the columns as periodic; a column roll is an exact symmetry of the data
// that only the padding breaks, a mirrored hemisphere with the meridional winds negated is the second physical view.  The forecasts of
// several views are pooled pixel by pixel in q, pixel_score.h's integer, and leave as ONE fp32 NCHW logits tensor, the format every consumer
// of the classifier already reads.
// Definitions (include/deepcam_hip.h has them with the ABI; tests/util_ensemble.py states them again in numpy):
//   view       (roll, flip), 0 <= roll < W: view pixel (h, w) shows source pixel src(h, w) = (flip ? H - 1 - h : h, (w + roll) mod W).
//   input      out[n, h, w, j] = scale[j] * (sign[j] * x[n, src(h, w), channels[j]] - shift[j]) in the activation dtype: the expression of
//              stem_head.hip's input_normalize_kernel with the source pixel permuted and the sign applied in physical units, in front of
//              the normalisation.  A null sign multiplies nothing: the identity view then gives that kernel's bits.
//   member m   fp32 NCHW logits in view coordinates, its view, and per SOURCE column a weight wt[W] (uint16 >= 1; null: 1).  At source pixel p
//              with the three logits of the view pixel that shows p: not all finite (logits_finite) -> bad[p] += 1 and nothing else; else
//              with q = prob_q(l0, l1, l2): S_c[p] += wt[col(p)] * q_c, votes[first_max(l).am][p] += 1.  Member 0 also notes first[p] =
//              first_max(l).am, 3 where the pixel was not finite.
//   state      uint32 [B][4][H][W]: the planes S_0, S_1, S_2 and one packed plane -- bits 0-5, 6-11, 12-17 the votes of class 0, 1, 2, bits
//              18-23 bad, bits 24-25 first.  Six bits: at most 63 members.  Member 0 STORES its contribution, the others add to it: nothing
//              clears the state, and one thread owns a pixel, so there are no atomics.  The caller keeps the sum of the members' largest
//              weights at or below 65535, so that S < 65535 * 65537 < 2^32.
//   pool       bad == 0: top = the first class with the largest S_c; L_c = (float)log((double)max(S_c, 1) / (double)S_top), division and
//              log in fp64, one rounding to fp32.  x / x is 1 and log(1) is 0, so L_top == 0.0f, and so is every L_c with S_c == S_top;
//              S_c < S_top gives a quotient of at most 1 - 2^-32 and L_c < 0.  Hence first_max(L) is the integer first maximum of S, ties
//              included.  bad > 0: three NaNs, which dc_prob_score and dc_logits_decide count as not finite.
//   rows       int64 [B][208]: word 64 c + k the pixels of the frame with exactly k votes for class c; word 192 + 4 i + j the pixels whose
//              first is i and whose pooled class is j (3: not finite).
// The decomposition: three streaming passes, each in decide.hip's layout -- a workgroup takes EN_CHUNK consecutive pixels of one sample
// (blockIdx.y) in passes of 4 pixels per thread and ends.
//   view_normalize     a row of the view is a row of the source, rotated: blockIdx.y walks the rows, a thread takes one 16-byte vector of
//                      one output pixel.  With all file channels in file order a pixel of 16 fp32 channels is 64 contiguous bytes and four
//                      lanes (fp32 output; two with bf16) read it by 16-byte loads, as climatology.hip does; the roll moves whole pixels and
//                      the flip whole rows, so the alignment never breaks.  A channel selection gathers by 4-byte loads.
//   ensemble_add_vec   W % 4 == 0 and roll % 4 == 0: a thread owns four consecutive SOURCE pixels; their view pixels are four consecutive
//                      ones too, 16-byte aligned, and never straddle the seam.  One 16-byte load per logit plane, one 16-byte load and store
//                      per state plane (member 0: no load), one 8-byte load of the four weights.
//   ensemble_add       any width and roll: 4-byte loads and stores, 4 pixels a workgroup's width apart.
//   ensemble_pool      16 bytes of state in, 12 bytes of logits out per pixel, 16-byte accesses where H * W % 4 == 0.  The fp64 work is one
//                      division and one log per class that is not at the top.  The 208 counters are cells of a histogram in LDS; a wave
//                      adds the pixels that share the cell of its first pixel by ONE lane (a frame is mostly unanimous background, and
//                      same-address LDS atomics serialise over the lanes).  The workgroup adds its non-zero cells to rows[b] and to the
//                      running totals by 64-bit atomics: integer sums, the same whatever the schedule and however the frames are cut.
#include "common.h"
#include "pixel_score.h"

namespace dc {

static constexpr int EN_THREADS = 256;
static constexpr int EN_PASS = EN_THREADS * 4;      // pixels of one pass of a workgroup
static constexpr int EN_PASSES = 8;
static constexpr int EN_CHUNK = EN_PASS * EN_PASSES;   // pixels of a workgroup: 2^13, so an LDS cell of 32 bits cannot wrap
static constexpr int EN_BMAX = 4095;                // B stays a legal grid.y
static constexpr int EN_MEMBERS = 63;               // a 6-bit vote field
static constexpr int EN_ROW = 208;                  // 3 x 64 vote cells, 4 x 4 (first, pooled) cells
static constexpr int EN_CHANGED = 192;
static constexpr unsigned EN_FIELD = 63u, EN_BAD_SHIFT = 18, EN_FIRST_SHIFT = 24;

// ------------------------------------------------------------------------------------------------ the view of the input
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void view_normalize_kernel(int rows, int H, int W, int Cfile, int Cc, const int* __restrict__ channels,
                                                             const float* __restrict__ sign, const float* __restrict__ x,
                                                             const float* __restrict__ shift, const float* __restrict__ scale, int roll,
                                                             int flip, T* __restrict__ out, int ldo) {
  constexpr int KPV = Elem<T>::kPerVec;
  const int ngroups = Cc / KPV;
  const long per_row = (long)W * ngroups;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int n = row / H, h = row - n * H;
    const int hs = flip ? H - 1 - h : h;
    const float* xr = x + ((size_t)n * H + hs) * W * Cfile;
    T* orow = out + (size_t)row * W * ldo;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < per_row; i += (long)gridDim.x * blockDim.x) {
      const int w = (int)(i / ngroups), cg = (int)(i - (long)w * ngroups);
      int ws = w + roll;                            // roll < W: one subtraction wraps
      if (ws >= W) ws -= W;
      const float* px = xr + (size_t)ws * Cfile;
      float f[KPV];
      if (VEC) {                                    // channels in file order, Cfile a multiple of 4, x 16-byte aligned
#pragma unroll
        for (int e = 0; e < KPV; e += 4) {
          const float4 v = *reinterpret_cast<const float4*>(px + cg * KPV + e);
          f[e] = v.x, f[e + 1] = v.y, f[e + 2] = v.z, f[e + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < KPV; ++e) {
          const int j = cg * KPV + e;
          f[e] = px[channels != nullptr ? channels[j] : j];
        }
      }
#pragma unroll
      for (int e = 0; e < KPV; ++e) {
        const int j = cg * KPV + e;
        float v = f[e];
        if (sign != nullptr) v = sign[j] * v;       // +-1: exact, fused with the subtraction or not
        f[e] = scale[j] * (v - shift[j]);
      }
      vec16 v;
      pack(v, f, T());
      stg16(orow + (size_t)w * ldo + cg * KPV, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------ a member
// One source pixel takes one member.  FIRST (member 0): what s0, s1, s2, pk held is dropped, not read.
template <bool FIRST>
__device__ inline void add_pixel(float l0, float l1, float l2, unsigned wt, unsigned& s0, unsigned& s1, unsigned& s2, unsigned& pk) {
  if (FIRST) s0 = s1 = s2 = pk = 0u;
  if (!logits_finite(l0, l1, l2)) {
    pk += 1u << EN_BAD_SHIFT;
    if (FIRST) pk |= 3u << EN_FIRST_SHIFT;
    return;
  }
  const ProbQ q = prob_q(l0, l1, l2);
  const unsigned am = (unsigned)first_max(l0, l1, l2).am;
  s0 += wt * (unsigned)q.q0, s1 += wt * (unsigned)q.q1, s2 += wt * (unsigned)q.q2;
  pk += 1u << (6u * am);
  if (FIRST) pk |= am << EN_FIRST_SHIFT;
}

// the view pixel (as an offset into a plane) that shows source pixel (hs, ws)
__device__ inline long view_of(int hs, int ws, int H, int W, int roll, int flip) {
  const int h = flip ? H - 1 - hs : hs;
  int w = ws - roll;
  if (w < 0) w += W;
  return (long)h * W + w;
}

template <bool VEC, bool FIRST>
__global__ __launch_bounds__(EN_THREADS) void ensemble_add_kernel(int H, int W, const float* __restrict__ logits, int roll, int flip,
                                                                  const uint16_t* __restrict__ col_weight, unsigned* __restrict__ state) {
  const int t = threadIdx.x, b = blockIdx.y;
  const long HW = (long)H * W;
  const float* lb = logits + (size_t)b * NC * HW;
  unsigned* sb = state + (size_t)b * 4 * HW;
  const long base = (long)blockIdx.x * EN_CHUNK;
  for (int pass = 0; pass < EN_PASSES; ++pass) {
    const long p0 = base + (long)pass * EN_PASS;
    if (p0 >= HW) break;
    if (VEC) {                                      // W % 4 == 0, roll % 4 == 0: four source pixels of one row, four view pixels of one row
      const long p = p0 + 4 * t;
      if (p >= HW) continue;
      const int hs = (int)(p / W), ws = (int)(p - (long)hs * W);
      const long v = view_of(hs, ws, H, W, roll, flip);
      const float4 a0 = *reinterpret_cast<const float4*>(lb + v);
      const float4 a1 = *reinterpret_cast<const float4*>(lb + HW + v);
      const float4 a2 = *reinterpret_cast<const float4*>(lb + 2 * HW + v);
      ushort4 wt = make_ushort4(1, 1, 1, 1);
      if (col_weight != nullptr) wt = *reinterpret_cast<const ushort4*>(col_weight + ws);
      uint4 s0 = make_uint4(0u, 0u, 0u, 0u), s1 = s0, s2 = s0, pk = s0;
      if (!FIRST) {
        s0 = *reinterpret_cast<const uint4*>(sb + p);
        s1 = *reinterpret_cast<const uint4*>(sb + HW + p);
        s2 = *reinterpret_cast<const uint4*>(sb + 2 * HW + p);
        pk = *reinterpret_cast<const uint4*>(sb + 3 * HW + p);
      }
      add_pixel<FIRST>(a0.x, a1.x, a2.x, wt.x, s0.x, s1.x, s2.x, pk.x);
      add_pixel<FIRST>(a0.y, a1.y, a2.y, wt.y, s0.y, s1.y, s2.y, pk.y);
      add_pixel<FIRST>(a0.z, a1.z, a2.z, wt.z, s0.z, s1.z, s2.z, pk.z);
      add_pixel<FIRST>(a0.w, a1.w, a2.w, wt.w, s0.w, s1.w, s2.w, pk.w);
      *reinterpret_cast<uint4*>(sb + p) = s0;
      *reinterpret_cast<uint4*>(sb + HW + p) = s1;
      *reinterpret_cast<uint4*>(sb + 2 * HW + p) = s2;
      *reinterpret_cast<uint4*>(sb + 3 * HW + p) = pk;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long p = p0 + j * EN_THREADS + t;
        if (p >= HW) continue;
        const int hs = (int)(p / W), ws = (int)(p - (long)hs * W);
        const long v = view_of(hs, ws, H, W, roll, flip);
        const unsigned wt = col_weight != nullptr ? col_weight[ws] : 1u;
        unsigned s0 = 0u, s1 = 0u, s2 = 0u, pk = 0u;
        if (!FIRST) s0 = sb[p], s1 = sb[HW + p], s2 = sb[2 * HW + p], pk = sb[3 * HW + p];
        add_pixel<FIRST>(lb[v], lb[HW + v], lb[2 * HW + v], wt, s0, s1, s2, pk);
        sb[p] = s0, sb[HW + p] = s1, sb[2 * HW + p] = s2, sb[3 * HW + p] = pk;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ the pool
// the pooled logits of one pixel; returns the pooled class, 3 where a member was not finite
__device__ inline int pool_pixel(unsigned s0, unsigned s1, unsigned s2, unsigned pk, float& L0, float& L1, float& L2) {
  if ((pk >> EN_BAD_SHIFT) & EN_FIELD) {
    L0 = L1 = L2 = __builtin_nanf("");
    return 3;
  }
  int top = 0;
  unsigned best = s0;
  if (s1 > best) { best = s1; top = 1; }
  if (s2 > best) { best = s2; top = 2; }
  const double den = (double)(best > 1u ? best : 1u);
  // S_c == S_top: the quotient is 1 and its log 0, without the arithmetic
  L0 = s0 == best ? 0.f : (float)log((double)(s0 > 1u ? s0 : 1u) / den);
  L1 = s1 == best ? 0.f : (float)log((double)(s1 > 1u ? s1 : 1u) / den);
  L2 = s2 == best ? 0.f : (float)log((double)(s2 > 1u ? s2 : 1u) / den);
  return top;
}

// cells[cell] += 1 for every lane with ok, the lanes that share the cell of the wave's first such lane through one add.  A ballot: every
// lane of the wave reaches it.
__device__ inline void cell_count(unsigned* cells, bool ok, int cell) {
  const unsigned long long live = __ballot(ok);
  if (live == 0) return;                            // wave-uniform
  const int first_lane = __ffsll((long long)live) - 1;
  const int ref = __shfl(cell, first_lane, 64);
  const bool same = ok && cell == ref;
  const unsigned n = (unsigned)__popcll(__ballot(same));
  if ((int)(threadIdx.x & 63) == first_lane) atomicAdd(&cells[ref], n);
  if (ok && !same) atomicAdd(&cells[cell], 1u);
}

template <bool VEC>
__global__ __launch_bounds__(EN_THREADS) void ensemble_pool_kernel(long HW, int n_valid, const unsigned* __restrict__ state,
                                                                   float* __restrict__ logits, unsigned long long* __restrict__ rows,
                                                                   unsigned long long* __restrict__ totals,
                                                                   unsigned long long* __restrict__ frames) {
  __shared__ unsigned cells[EN_ROW];
  const int t = threadIdx.x, b = blockIdx.y;
  if (t < EN_ROW) cells[t] = 0u;
  __syncthreads();
  const unsigned* sb = state + (size_t)b * 4 * HW;
  float* lb = logits + (size_t)b * NC * HW;
  const long base = (long)blockIdx.x * EN_CHUNK;
  // The trip count is the same for all lanes of a workgroup: the ballots see whole waves.
  for (int pass = 0; pass < EN_PASSES; ++pass) {
    const long p0 = base + (long)pass * EN_PASS;
    if (p0 >= HW) break;
    unsigned s[4][4];                               // [plane][pixel]
    bool ok[4];
    float L[NC][4];
    int pooled[4];
    if (VEC) {                                      // HW % 4 == 0: the four pixels are all inside or all outside
      const long p = p0 + 4 * t;
      const bool in = p < HW;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (in) v = *reinterpret_cast<const uint4*>(sb + (size_t)c * HW + p);
        s[c][0] = v.x, s[c][1] = v.y, s[c][2] = v.z, s[c][3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ok[j] = in;
        pooled[j] = pool_pixel(s[0][j], s[1][j], s[2][j], s[3][j], L[0][j], L[1][j], L[2][j]);
      }
      if (in) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
          *reinterpret_cast<float4*>(lb + (size_t)c * HW + p) = make_float4(L[c][0], L[c][1], L[c][2], L[c][3]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long p = p0 + j * EN_THREADS + t;
        ok[j] = p < HW;
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c][j] = ok[j] ? sb[(size_t)c * HW + p] : 0u;
        pooled[j] = pool_pixel(s[0][j], s[1][j], s[2][j], s[3][j], L[0][j], L[1][j], L[2][j]);
        if (ok[j]) lb[p] = L[0][j], lb[HW + p] = L[1][j], lb[2 * HW + p] = L[2][j];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned pk = s[3][j];
#pragma unroll
      for (int c = 0; c < NC; ++c) cell_count(cells, ok[j], 64 * c + (int)((pk >> (6 * c)) & EN_FIELD));
      cell_count(cells, ok[j], EN_CHANGED + 4 * (int)((pk >> EN_FIRST_SHIFT) & 3u) + pooled[j]);
    }
  }
  __syncthreads();
  if (t < EN_ROW) {
    const unsigned long long v = cells[t];
    if (v) {
      atomicAdd(rows + (size_t)b * EN_ROW + t, v);
      atomicAdd(totals + t, v);
    }
  }
  if (t == 0 && b == 0 && blockIdx.x == 0) atomicAdd(frames, (unsigned long long)n_valid);
}

static int ensemble_check(const char* fn, int B, int n_valid, int H, int W) {
  const char* what = B < 1 || B > EN_BMAX || H < 1 || W < 1 ? "B must lie in [1, 4095], H and W must be positive"
                     : (long)H * W > (1L << 30)             ? "H * W must not exceed 2^30"
                     : n_valid < 0 || n_valid > B           ? "n_valid must lie in [0, B]"
                                                            : nullptr;
  if (!what) return 0;
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", fn, what);
  return dc_fail(msg, __FILE__, __LINE__);
}

}  // namespace dc

using namespace dc;

extern "C" int dc_ensemble_block(int* pixels) {
  DC_REQUIRE(pixels, "dc_ensemble_block: null argument");
  *pixels = EN_CHUNK;
  return 0;
}

extern "C" int dc_input_view_hwc(int dtype, int B, int H, int W, int Cfile, int C, const int* channels, const float* sign, const float* x_hwc,
                                 const float* shift, const float* scale, int roll, int flip, void* out, int ldo, void* stream) {
  if (int rc = ensemble_check("dc_input_view_hwc", B, B, H, W)) return rc;
  DC_REQUIRE(dtype == DC_F32 || dtype == DC_BF16, "dc_input_view_hwc: dtype must be DC_F32 or DC_BF16");
  if (int e = dc_check_view(out, ldo, C, dtype, "dc_input_view_hwc out")) return e;
  DC_REQUIRE(x_hwc && shift && scale && Cfile >= C, "dc_input_view_hwc: null pointer, or fewer file channels than selected ones");
  DC_REQUIRE(((uintptr_t)x_hwc & 3) == 0 && ((uintptr_t)shift & 3) == 0 && ((uintptr_t)scale & 3) == 0 && ((uintptr_t)sign & 3) == 0 &&
                 ((uintptr_t)channels & 3) == 0, "dc_input_view_hwc: a pointer is not aligned to its element size");
  DC_REQUIRE(roll >= 0 && roll < W, "dc_input_view_hwc: roll must lie in [0, W)");
  DC_REQUIRE(flip == 0 || flip == 1, "dc_input_view_hwc: flip must be 0 or 1");
  const int kpv = dtype == DC_BF16 ? 8 : 4;
  const long per_row = (long)W * (C / kpv);
  DC_REQUIRE((long)B * H <= 2147483647L, "dc_input_view_hwc: B * H must be below 2^31");
  const int rows = B * H;
  const unsigned gx = (unsigned)(per_row < 256L * 32 ? (per_row + 255) / 256 : 32);
  const unsigned gy = (unsigned)(rows < (int)(8192 / gx) ? rows : 8192 / gx);
  const bool vec = channels == nullptr && Cfile % 4 == 0 && ((uintptr_t)x_hwc & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
#define VIEW(TT, VV)                                                                                                                        \
  hipLaunchKernelGGL((view_normalize_kernel<TT, VV>), dim3(gx, gy), dim3(256), 0, st, rows, H, W, Cfile, C, channels, sign, x_hwc, shift, \
                     scale, roll, flip, (TT*)out, ldo)
  if (dtype == DC_BF16) {
    if (vec) VIEW(bf16, true); else VIEW(bf16, false);
  } else {
    if (vec) VIEW(float, true); else VIEW(float, false);
  }
#undef VIEW
  DC_LAUNCHED("view_normalize");
  return 0;
}

extern "C" int dc_ensemble_add(int B, int n_valid, int H, int W, const float* logits_nchw, int roll, int flip, const uint16_t* col_weight,
                               int member, uint32_t* state, void* stream) {
  if (int rc = ensemble_check("dc_ensemble_add", B, n_valid, H, W)) return rc;
  DC_REQUIRE(logits_nchw && state, "dc_ensemble_add: null pointer");
  DC_REQUIRE(((uintptr_t)logits_nchw & 3) == 0 && ((uintptr_t)state & 3) == 0 && ((uintptr_t)col_weight & 1) == 0,
             "dc_ensemble_add: logits, state or col_weight not aligned to their element size");
  DC_REQUIRE(roll >= 0 && roll < W, "dc_ensemble_add: roll must lie in [0, W)");
  DC_REQUIRE(flip == 0 || flip == 1, "dc_ensemble_add: flip must be 0 or 1");
  DC_REQUIRE(member >= 0 && member < EN_MEMBERS, "dc_ensemble_add: member must lie in [0, 63)");
  if (n_valid == 0) return 0;                       // nothing to read, nothing to write
  const long HW = (long)H * W;
  const unsigned gx = (unsigned)((HW + EN_CHUNK - 1) / EN_CHUNK);
  // 16-byte loads and stores: every plane and every sample start a multiple of HW elements in, every row a multiple of W
  const bool vec = W % 4 == 0 && roll % 4 == 0 && ((uintptr_t)logits_nchw & 15) == 0 && ((uintptr_t)state & 15) == 0 &&
                   ((uintptr_t)col_weight & 7) == 0;
  hipStream_t st = (hipStream_t)stream;
#define ADD(VV, FF)                                                                                                                   \
  hipLaunchKernelGGL((ensemble_add_kernel<VV, FF>), dim3(gx, n_valid), dim3(EN_THREADS), 0, st, H, W, logits_nchw, roll, flip, col_weight, \
                     (unsigned*)state)
  if (vec) {
    if (member == 0) ADD(true, true); else ADD(true, false);
    DC_LAUNCHED("ensemble_add_vec");
  } else {
    if (member == 0) ADD(false, true); else ADD(false, false);
    DC_LAUNCHED("ensemble_add");
  }
#undef ADD
  return 0;
}

extern "C" int dc_ensemble_pool(int B, int n_valid, int H, int W, int members, const uint32_t* state, float* logits_nchw, int64_t* rows,
                                int64_t* totals, int64_t* frames, void* stream) {
  if (int rc = ensemble_check("dc_ensemble_pool", B, n_valid, H, W)) return rc;
  DC_REQUIRE(members >= 1 && members <= EN_MEMBERS, "dc_ensemble_pool: members must lie in [1, 63]");
  DC_REQUIRE(state && logits_nchw && rows && totals && frames, "dc_ensemble_pool: null pointer");
  DC_REQUIRE(((uintptr_t)state & 3) == 0 && ((uintptr_t)logits_nchw & 3) == 0 && ((uintptr_t)rows & 7) == 0 && ((uintptr_t)totals & 7) == 0 &&
                 ((uintptr_t)frames & 7) == 0, "dc_ensemble_pool: state, logits, rows or a total not aligned to its element size");
  if (n_valid == 0) return 0;                       // nothing to read, nothing to write
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(rows, 0, (size_t)n_valid * EN_ROW * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const long HW = (long)H * W;
  const unsigned gx = (unsigned)((HW + EN_CHUNK - 1) / EN_CHUNK);
  const bool vec = HW % 4 == 0 && ((uintptr_t)state & 15) == 0 && ((uintptr_t)logits_nchw & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(ensemble_pool_kernel<true>, dim3(gx, n_valid), dim3(EN_THREADS), 0, st, HW, n_valid, (const unsigned*)state, logits_nchw,
                       (unsigned long long*)rows, (unsigned long long*)totals, (unsigned long long*)frames);
  else
    hipLaunchKernelGGL(ensemble_pool_kernel<false>, dim3(gx, n_valid), dim3(EN_THREADS), 0, st, HW, n_valid, (const unsigned*)state, logits_nchw,
                       (unsigned long long*)rows, (unsigned long long*)totals, (unsigned long long*)frames);
  DC_LAUNCHED("ensemble_pool");
  return 0;
}
