// Event shapes and the shape filter (dc_component_shape, dc_event_select, dc_mask_select; nn.EventShape, nn.EventFilter).
//
// One row of twelve int64 words per event rank (include/deepcam_hip.h has the definition): boundary pixels, the two face counts, and the
// 2^40-scaled first and second moments of the event's pixels as weighted unit vectors on the sphere.  Every per-pixel term is an integer
// below 2^40 in magnitude and H * W <= 2^22, so every sum fits an int64, is exact and does not depend on the order of arrival.
//   sh_pixel   one workgroup per tile, a thread walks 8 consecutive pixels of a row (the row walk of event_common.h with rows and column
//              groups transposed: SH_STRIDE says why).  The tile's label words and a halo of one pixel (the rows above and below,
//              the columns left and right, the seam's other side under wrap, 0 off the grid) are staged in LDS once, so that the
//              four face tests of a pixel read LDS; a thread reduces each run of one root in registers (n, five column sums, three
//              face counts), multiplies the row's factors in once per run and hands the twelve terms to the workgroup's table in LDS,
//              keyed by root.  Runs that find no slot within SH_PROBES go to the global row directly; filled slots are flushed at the end.
//   sh_select  one thread per event row: the decode formula in fp64, the keep flag, the events kept and dropped per class
//   sh_mask    one streaming pass: the filtered mask and the pixels kept and dropped per class (one atomic per workgroup and counter)
// 64-bit integer atomics only; no workgroup waits for another.
#include "event_common.h"

namespace dc {

static constexpr int SH_FIELDS = 12;
static constexpr int SH_SLOTS = 128;              // per-workgroup table of partial sums: 12 KiB of LDS
static constexpr int SH_PROBES = 4;
static constexpr int SH_LH = CC_TH + 2, SH_LW = CC_TW + 2;
static constexpr int SH_STRIDE = 67;              // words per staged row, odd: a 4-byte LDS read is served in two groups of 32 lanes over 32
                                                  // banks; a group is 8 rows x 4 column groups of 8 words (sh_pixel_kernel's lane layout), its
                                                  // banks 3 row + 8 group (mod 32) are all different at every step of the walk
static constexpr int SH_ROW_TABLES = 6, SH_COL_TABLES = 5;
static constexpr int SH_COUNTS = 8;               // per class: events kept, events dropped, pixels kept, pixels dropped

struct ShRun {                                    // one thread's run of pixels of one component inside one row; the column sums of at most
  int root, n, nb, fv, fh;                        // 8 entries of 2^20 each stay below 2^23
  int scx, ssx, sxx, sxy, syy;
};
struct ShRow {                                    // the row's factors: wy, rc2, rcs, rc3, rc2s, rcs2
  int wy, c2, cs, c3, c2s, cs2;
};

__device__ inline void sh_terms(const ShRun& a, const ShRow& w, long long* t) {
  const long long n20 = (long long)a.n * (1ll << 20);
  t[0] = a.nb;
  t[1] = a.fv;
  t[2] = (long long)a.fh * w.wy;
  t[3] = (long long)w.c2 * a.scx;
  t[4] = (long long)w.c2 * a.ssx;
  t[5] = (long long)w.cs * n20;
  t[6] = (long long)w.c3 * a.sxx;
  t[7] = (long long)w.c3 * a.sxy;
  t[8] = (long long)w.c3 * a.syy;
  t[9] = (long long)w.c2s * a.scx;
  t[10] = (long long)w.c2s * a.ssx;
  t[11] = (long long)w.cs2 * n20;
}

__device__ inline void sh_emit(const int* __restrict__ rank_sample, long HW, int cap, long long* shape_sample, int root, const long long* t) {
  const int rank = event_rank(rank_sample, HW, cap, root);
  if (rank < 0) return;
  unsigned long long* row = (unsigned long long*)(shape_sample + (size_t)rank * SH_FIELDS);
#pragma unroll
  for (int f = 0; f < SH_FIELDS; ++f)
    if (t[f] != 0) atomicAdd(row + f, (unsigned long long)t[f]);
}

__global__ __launch_bounds__(256) void sh_pixel_kernel(int H, int W, int wrap, const int* __restrict__ labels, const int* __restrict__ rowt,
                                                       const int* __restrict__ colt, int cap, const int* __restrict__ rank_map,
                                                       long long* __restrict__ shape) {
  __shared__ int s_lab[SH_LH * SH_STRIDE];
  __shared__ int s_key[SH_SLOTS];
  __shared__ unsigned long long s_sum[SH_SLOTS][SH_FIELDS];
  const long HW = (long)H * W;
  const size_t base = (size_t)blockIdx.z * HW;
  const int* L = labels + base;
  const int* rank_sample = rank_map + base;
  long long* shape_sample = shape + (size_t)blockIdx.z * cap * SH_FIELDS;
  const int r0 = blockIdx.y * CC_TH, c0 = blockIdx.x * CC_TW;
  if (threadIdx.x < SH_SLOTS) {
    const int s = threadIdx.x;
    s_key[s] = -1;
#pragma unroll
    for (int f = 0; f < SH_FIELDS; ++f) s_sum[s][f] = 0ull;
  }
  // the tile and its halo: rows r0 - 1 .. r0 + TH, columns c0 - 1 .. c0 + TW; 0 where there is no pixel
  for (int i = threadIdx.x; i < SH_LH * SH_LW; i += 256) {
    const int lr = i / SH_LW, lc = i % SH_LW;
    const int gr = r0 - 1 + lr;
    int gc = c0 - 1 + lc;
    if (wrap) gc = gc < 0 ? W - 1 : (gc == W ? 0 : gc);
    int v = 0;
    if (gr >= 0 && gr < H && gc >= 0 && gc < W) v = L[(size_t)gr * W + gc];
    s_lab[lr * SH_STRIDE + lc] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // not row_walk_origin: lanes 0 - 31 take 8 rows x the first 4 column groups, the layout SH_STRIDE's bank argument is made for
  const int lr = wave * 8 + (lane & 7), lcb = (lane >> 3) * 8;
  const int r = r0 + lr, cb = c0 + lcb;
  if (r < H) {
    ShRow w;
    w.wy = rowt[r];
    w.c2 = rowt[H + r];
    w.cs = rowt[2 * H + r];
    w.c3 = rowt[3 * H + r];
    w.c2s = rowt[4 * H + r];
    w.cs2 = rowt[5 * H + r];
    const int* mid = s_lab + (lr + 1) * SH_STRIDE + lcb + 1;          // the thread's first pixel
    ShRun a;
    a.root = -1;
    for (int j = 0; j <= 8; ++j) {
      const int c = cb + j;
      const int v = (j < 8 && c < W) ? mid[j] : 0;                    // (column W holds column 0's word under wrap: not a pixel)
      const int root = v - 1;                     // -1: background, the row's end, the run's end
      if (root != a.root) {
        if (a.root >= 0) {
          long long t[SH_FIELDS];
          sh_terms(a, w, t);
          const int hit = slot_claim<SH_SLOTS, SH_PROBES>(s_key, slot_hash<SH_SLOTS>(a.root), a.root);
          if (hit >= 0) {
#pragma unroll
            for (int f = 0; f < SH_FIELDS; ++f)
              if (t[f] != 0) atomicAdd(&s_sum[hit][f], (unsigned long long)t[f]);
          } else {
            sh_emit(rank_sample, HW, cap, shape_sample, a.root, t);
          }
        }
        a.root = root;
        a.n = a.nb = a.fv = a.fh = 0;
        a.scx = a.ssx = a.sxx = a.sxy = a.syy = 0;
      }
      if (root >= 0) {
        const int up = mid[j - SH_STRIDE] != v, dn = mid[j + SH_STRIDE] != v, lf = mid[j - 1] != v, rt = mid[j + 1] != v;
        a.n += 1;
        a.nb += up | dn | lf | rt;
        a.fv += lf + rt;
        a.fh += up + dn;
        a.scx += colt[c];
        a.ssx += colt[W + c];
        a.sxx += colt[2 * W + c];
        a.sxy += colt[3 * W + c];
        a.syy += colt[4 * W + c];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < SH_SLOTS && s_key[threadIdx.x] >= 0) {
    const int s = threadIdx.x;
    long long t[SH_FIELDS];
#pragma unroll
    for (int f = 0; f < SH_FIELDS; ++f) t[f] = (long long)s_sum[s][f];
    sh_emit(rank_sample, HW, cap, shape_sample, s_key[s], t);
  }
}
static_assert(SH_STRIDE >= SH_LW, "sh_pixel_kernel: a staged row holds the tile's columns and the halo");

// lambda+ and lambda- of one event (the decode formula of include/deepcam_hip.h); false when the zeroth moment is 0
__device__ inline bool sh_lambda(long long area, const long long* __restrict__ s, double* lp, double* lm) {
  *lp = *lm = 0.0;
  if (area <= 0) return false;
  const double s0 = (double)area * 0x1p20;
  const double mx = (double)s[3] / s0, my = (double)s[4] / s0, mz = (double)s[5] / s0;
  const double cxx = (double)s[6] / s0 - mx * mx, cxy = (double)s[7] / s0 - mx * my, cyy = (double)s[8] / s0 - my * my;
  const double cxz = (double)s[9] / s0 - mx * mz, cyz = (double)s[10] / s0 - my * mz, czz = (double)s[11] / s0 - mz * mz;
  const double norm = sqrt(mx * mx + my * my + mz * mz);
  double ux = 1.0, uy = 0.0, uz = 0.0;            // the centroid's direction; (1, 0, 0) when the first moment vanishes
  if (norm > 0.0) {
    ux = mx / norm;
    uy = my / norm;
    uz = mz / norm;
  }
  const double h = sqrt(ux * ux + uy * uy);       // cos lat; sin lat = uz; (cos lon, sin lon) = (ux, uy) / h, (1, 0) at a pole
  const double co = h > 0.0 ? ux / h : 1.0, so = h > 0.0 ? uy / h : 0.0;
  const double ex = -so, ey = co;                                     // east
  const double nx = -uz * co, ny = -uz * so, nz = h;                  // north
  const double qx = cxx * nx + cxy * ny + cxz * nz, qy = cxy * nx + cyy * ny + cyz * nz, qz = cxz * nx + cyz * ny + czz * nz;   // C n
  const double a = ex * (cxx * ex + cxy * ey) + ey * (cxy * ex + cyy * ey);
  const double b = ex * qx + ey * qy;
  const double d = nx * qx + ny * qy + nz * qz;
  const double mid = 0.5 * (a + d), half = 0.5 * (a - d), rad = sqrt(half * half + b * b);
  *lp = fmax(mid + rad, 0.0);
  *lm = fmax(mid - rad, 0.0);
  return true;
}

struct ShCriteria {                               // one class's row of `criteria`
  long long min_pixels, min_area;
  double min_len2, min_aspect2;
};

__global__ __launch_bounds__(256) void sh_select_kernel(int cap, const long long* __restrict__ table, const int* __restrict__ ncomp,
                                                        const long long* __restrict__ shape, const ShCriteria* __restrict__ criteria,
                                                        uint8_t* __restrict__ keep, unsigned long long* counts) {
  __shared__ unsigned s_n[4];                     // class 1: kept, dropped; class 2: kept, dropped
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0u;
  __syncthreads();
  const int rows = event_rows(ncomp, b, cap);
  if (k < cap) {
    int kept = 0;
    if (k < rows) {
      const long long* row = table + ((size_t)b * cap + k) * CC_FIELDS;
      const long long cls = row[1], px = row[2], area = row[3];
      if (cls == 1 || cls == 2) {
        const ShCriteria cr = criteria[cls - 1];
        kept = 1;
        if (cr.min_pixels > 0 && px < cr.min_pixels) kept = 0;
        if (cr.min_area > 0 && area < cr.min_area) kept = 0;
        if (cr.min_len2 > 0.0 || cr.min_aspect2 > 0.0) {
          double lp, lm;
          const bool ok = sh_lambda(area, shape + ((size_t)b * cap + k) * SH_FIELDS, &lp, &lm);
          if (cr.min_len2 > 0.0 && !(ok && 12.0 * lp >= cr.min_len2)) kept = 0;
          if (cr.min_aspect2 > 0.0 && !(ok && lp >= cr.min_aspect2 * lm)) kept = 0;
        }
        atomicAdd(&s_n[(cls == 2 ? 2 : 0) + (kept ? 0 : 1)], 1u);
      }
    }
    keep[(size_t)b * cap + k] = (uint8_t)kept;
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_n[threadIdx.x])
    atomicAdd(counts + (size_t)b * SH_COUNTS + (threadIdx.x >> 1) * 4 + (threadIdx.x & 1), (unsigned long long)s_n[threadIdx.x]);
}

// the class a pixel keeps, and its count: v[0..3] = class 1 kept, dropped; class 2 kept, dropped
__device__ inline uint8_t sh_pixel(uint8_t m, int label, long HW, const int* __restrict__ rank_sample, int cap,
                                   const uint8_t* __restrict__ keep_sample, unsigned* v) {
  if (m != 1 && m != 2) return m;                 // background and values >= 3 pass through
  bool kept = true;                               // no row, no criterion: the pixel stays
  const int rank = event_rank(rank_sample, HW, cap, label - 1);
  if (rank >= 0) kept = keep_sample[rank] != 0;
  const int f = (m == 2 ? 2 : 0) + (kept ? 0 : 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] += f == i ? 1u : 0u;   // (constant indices: the four counters stay in registers)
  return kept ? m : (uint8_t)0;
}

// SH_MASK_PX pixels per thread: one 4-byte load of the mask, one 16-byte load of the labels, one 4-byte store when `vec` (HW a multiple of
// 4 and the three bases aligned); single bytes and words otherwise
static constexpr int SH_MASK_PX = 4;
__global__ __launch_bounds__(256) void sh_mask_kernel(long HW, int vec, const uint8_t* __restrict__ mask, const int* __restrict__ labels,
                                                      const int* __restrict__ rank_map, int cap, const uint8_t* __restrict__ keep,
                                                      uint8_t* __restrict__ out_mask, unsigned long long* counts) {
  __shared__ unsigned s_n[4];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * HW;
  const int* rank_sample = rank_map + base;
  const uint8_t* keep_sample = keep + (size_t)b * cap;
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0u;
  __syncthreads();
  unsigned v[4] = {0u, 0u, 0u, 0u};
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * SH_MASK_PX;
  if (vec && p0 + SH_MASK_PX <= HW) {
    const uchar4 m = *(const uchar4*)(mask + base + p0);
    const int4 l = *(const int4*)(labels + base + p0);
    uchar4 o;
    o.x = sh_pixel(m.x, l.x, HW, rank_sample, cap, keep_sample, v);
    o.y = sh_pixel(m.y, l.y, HW, rank_sample, cap, keep_sample, v);
    o.z = sh_pixel(m.z, l.z, HW, rank_sample, cap, keep_sample, v);
    o.w = sh_pixel(m.w, l.w, HW, rank_sample, cap, keep_sample, v);
    *(uchar4*)(out_mask + base + p0) = o;
  } else {
    for (int j = 0; j < SH_MASK_PX; ++j) {
      const long p = p0 + j;
      if (p < HW) out_mask[base + p] = sh_pixel(mask[base + p], labels[base + p], HW, rank_sample, cap, keep_sample, v);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned x = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(&s_n[i], x);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_n[threadIdx.x])
    atomicAdd(counts + (size_t)b * SH_COUNTS + (threadIdx.x >> 1) * 4 + 2 + (threadIdx.x & 1), (unsigned long long)s_n[threadIdx.x]);
}

}  // namespace dc

using namespace dc;

extern "C" int dc_component_shape(int B, int n_valid, int H, int W, const int32_t* labels, const int32_t* rank_map, int cap, int wrap,
                                  const int32_t* row_tables, const int32_t* col_tables, int64_t* shape, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE((long)H * W <= (1L << 22), "dc_component_shape: H * W must be at most 2^22 (the sums stay inside int64)");
  DC_REQUIRE(cap >= 1, "dc_component_shape: cap must be at least 1");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_component_shape: wrap must be 0 or 1");
  DC_REQUIRE(labels && rank_map && row_tables && col_tables && shape, "dc_component_shape: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(shape, 0, (size_t)n_valid * cap * SH_FIELDS * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  hipLaunchKernelGGL(sh_pixel_kernel, cc_tile_grid(H, W, n_valid), dim3(256), 0, st, H, W, wrap, labels, row_tables, col_tables, cap, rank_map,
                     (long long*)shape);
  DC_LAUNCHED("cc_shape");
  return 0;
}

extern "C" int dc_event_select(int B, int n_valid, int cap, const int64_t* table, const int32_t* ncomp, const int64_t* shape,
                               const void* criteria, uint8_t* keep, int64_t* counts, void* stream) {
  if (int rc = cc_check_batch(B, n_valid)) return rc;
  DC_REQUIRE(cap >= 1, "dc_event_select: cap must be at least 1");
  DC_REQUIRE(table && ncomp && shape && criteria && keep && counts, "dc_event_select: null pointer");
  DC_REQUIRE(((uintptr_t)criteria & 7) == 0, "dc_event_select: criteria not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_valid * SH_COUNTS * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  hipLaunchKernelGGL(sh_select_kernel, dim3((cap + 255) / 256, n_valid), dim3(256), 0, st, cap, (const long long*)table, ncomp,
                     (const long long*)shape, (const ShCriteria*)criteria, keep, (unsigned long long*)counts);
  DC_LAUNCHED("cc_shape");
  return 0;
}

extern "C" int dc_mask_select(int B, int n_valid, int H, int W, const uint8_t* mask, const int32_t* labels, const int32_t* rank_map, int cap,
                              const uint8_t* keep, uint8_t* out_mask, int64_t* counts, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(cap >= 1, "dc_mask_select: cap must be at least 1");
  DC_REQUIRE(mask && labels && rank_map && keep && out_mask && counts, "dc_mask_select: null pointer");
  const size_t bytes = (size_t)B * H * W;
  DC_REQUIRE((uintptr_t)out_mask + bytes <= (uintptr_t)mask || (uintptr_t)mask + bytes <= (uintptr_t)out_mask,
             "dc_mask_select: out_mask may not alias mask");
  const long HW = (long)H * W;
  const int vec = HW % 4 == 0 && ((uintptr_t)mask & 3) == 0 && ((uintptr_t)out_mask & 3) == 0 && ((uintptr_t)labels & 15) == 0;
  const long blocks = (HW + 256 * SH_MASK_PX - 1) / (256 * SH_MASK_PX);
  hipLaunchKernelGGL(sh_mask_kernel, dim3((unsigned)blocks, n_valid), dim3(256), 0, (hipStream_t)stream, HW, vec, mask, labels, rank_map, cap,
                     keep, out_mask, (unsigned long long*)counts);
  DC_LAUNCHED("cc_shape");
  return 0;
}
