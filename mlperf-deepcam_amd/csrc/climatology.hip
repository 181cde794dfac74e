// Climatology: the maps over time (dc_climatology_accumulate, dc_climatology_maps; nn.Climatology).  How often a grid point lies inside
// a cyclone or a river, and what the raw fields sum to there -- per group (all, season, month), accumulated on the device from batch to
// batch as integers.  include/deepcam_hip.h has the definition; this file has the decomposition.
//   clim_accumulate<V>  a workgroup owns CL_PIX consecutive pixels, a thread owns one ITEM of a pixel: V consecutive selected channels
//                  (V = 4, the vector form: the selection is the identity over ldc channels, so consecutive items are consecutive 16-byte
//                  pieces of the fields, 1 KiB per wave instruction, and consecutive 32- / 16-byte pieces of `sum` / `n`; V = 1, the scalar
//                  form: any selection, one channel per item, and one item per pixel when no channel is selected).  The thread walks the
//                  batch's frames in order with its partial sums in registers and adds them to the accumulators when the frame's group
//                  changes and at the end: once per run of equal group.  The "all" row is read-modified-written on every flush, a class
//                  row only if the pixel had that class in the run.  Item 0 of a pixel also owns the pixel's two `count` words, thread 0
//                  of workgroup 0 owns `frames`.  Every accumulator word has exactly ONE writer in the grid and the sums are integers:
//                  there is nothing to order, hence no atomics.  Where a pixel has more items than the workgroup has threads per pixel
//                  (more than 16 channels, or more than 4 in the scalar form) a thread takes several items one after the other.
//   clim_maps      one thread per (group, pixel, product): an fp64 quotient of the integers, rounded once more to fp32; the thread of a
//                  pixel's first product also writes the pixel's contour byte.
#include "common.h"
#include "mask_skill.h"

namespace dc {

static constexpr int CL_PIX = 64;                 // pixels of a workgroup: 256 items at 16 channels in the vector form
static constexpr int CL_MAXC = 32;

typedef long long cl_ll2 __attribute__((ext_vector_type(2)));
typedef int cl_i4 __attribute__((ext_vector_type(4)));
typedef float cl_f4 __attribute__((ext_vector_type(4)));

// classes 1 and 2 of a mask element; every other value is background
__device__ inline int cl_class(const void* m, size_t i, int bytes) {
  const long long v = mask_value(m, i, bytes);
  return (v == 1 || v == 2) ? (int)v : 0;
}

template <int V>
struct ClPart {                                   // the partial sums of one row of one item
  long long s[V];
  int n[V];
  __device__ inline void clear() {
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 0, n[j] = 0;
  }
};

// sum[off .. off + V) += part.s, n[off .. off + V) += part.n; V = 4: off % 4 == 0 and both bases 16-byte aligned
template <int V>
__device__ inline void cl_add(long long* __restrict__ sum, int* __restrict__ n, long long off, const ClPart<V>& part) {
  if constexpr (V == 4) {
    cl_ll2* ps = (cl_ll2*)(sum + off);
    cl_i4* pn = (cl_i4*)(n + off);
    cl_ll2 a = ps[0], b = ps[1];
    cl_i4 c = *pn;
    a.x += part.s[0], a.y += part.s[1], b.x += part.s[2], b.y += part.s[3];
    c.x += part.n[0], c.y += part.n[1], c.z += part.n[2], c.w += part.n[3];
    ps[0] = a, ps[1] = b;
    *pn = c;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) sum[off + j] += part.s[j], n[off + j] += part.n[j];
  }
}

template <int V>
__global__ __launch_bounds__(256) void clim_accumulate_kernel(int B, long long HW, int G, const void* __restrict__ mask, int mask_bytes,
                                                              const float* __restrict__ fields, int C, int ldc,
                                                              const int32_t* __restrict__ chan, const int32_t* __restrict__ bits,
                                                              const int32_t* __restrict__ group, long long* __restrict__ frames,
                                                              int32_t* __restrict__ count, long long* __restrict__ sum,
                                                              int32_t* __restrict__ n) {
  if (blockIdx.x == 0 && threadIdx.x == 0)        // frames: one writer in the grid
    for (int b = 0; b < B; ++b) {
      const int g = group[b];
      if (g >= 0 && g < G) frames[g] += 1;
    }
  const int Q = C > 0 ? C / V : 1;                // items of a pixel
  const long long p0 = (long long)blockIdx.x * CL_PIX;
  const int npix = HW - p0 < CL_PIX ? (int)(HW - p0) : CL_PIX;
  const long long row_words = HW * C;             // words of one row of one group in `sum` / `n`
  for (int t = threadIdx.x; t < npix * Q; t += blockDim.x) {
    const int q = t % Q;
    const long long p = p0 + t / Q;
    int sh[V], col[V];                            // the binary scale and the file channel of the item's channels; col < 0: nothing to load
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sh[j] = 0, col[j] = -1;
      if (C > 0) {
        const int c = q * V + j;
        const int ch = chan ? chan[c] : c;
        sh[j] = bits[c];
        col[j] = (ch >= 0 && ch < ldc) ? ch : -1;
      }
    }
    ClPart<V> all, k1, k2;
    int c1 = 0, c2 = 0, cur = -1;
    all.clear(), k1.clear(), k2.clear();
    auto flush = [&]() {                          // the run of group `cur` into the accumulators
      const long long off = (long long)cur * 3 * row_words + p * C + q * V;
      if (C > 0) {
        cl_add<V>(sum, n, off, all);
        if (c1) cl_add<V>(sum, n, off + row_words, k1);
        if (c2) cl_add<V>(sum, n, off + 2 * row_words, k2);
      }
      if (q == 0) {
        if (c1) count[((long long)cur * 2) * HW + p] += c1;
        if (c2) count[((long long)cur * 2 + 1) * HW + p] += c2;
      }
    };
    for (int b = 0; b < B; ++b) {
      const int g = group[b];
      if (g < 0 || g >= G) continue;              // not read at all
      if (g != cur) {
        if (cur >= 0) flush();
        cur = g, c1 = 0, c2 = 0;
        all.clear(), k1.clear(), k2.clear();
      }
      const size_t px = (size_t)b * HW + p;
      const int k = cl_class(mask, px, mask_bytes);
      c1 += k == 1, c2 += k == 2;
      if (C == 0) continue;
      float v[V];
      if constexpr (V == 4) {
        const cl_f4 f = *(const cl_f4*)(fields + px * ldc + q * 4);
        v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = col[j] >= 0 ? fields[px * ldc + col[j]] : __uint_as_float(0x7fc00000u);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double s = rint(ldexp((double)v[j], sh[j]));   // dc_component_fields' rule; NaN and +-Inf fail the comparison as well
        const bool ok = fabs(s) <= 0x1p40;
        const long long qi = ok ? (long long)s : 0;
        all.s[j] += qi, all.n[j] += ok;
        k1.s[j] += k == 1 ? qi : 0, k1.n[j] += ok && k == 1;
        k2.s[j] += k == 2 ? qi : 0, k2.n[j] += ok && k == 2;
      }
    }
    if (cur >= 0) flush();
  }
}

static constexpr unsigned CL_NAN = 0x7fc00000u;

// products int32 [K][3]: (0, class, -) frequency; (1, channel, row) mean; (2, channel, class) share.  Anything else: NaN.
__global__ __launch_bounds__(256) void clim_maps_kernel(int G, long long HW, int C, const long long* __restrict__ frames,
                                                        const int32_t* __restrict__ count, const long long* __restrict__ sum,
                                                        const int32_t* __restrict__ n, const int32_t* __restrict__ bits, int K,
                                                        const int32_t* __restrict__ products, float t1, float t2, float* __restrict__ out,
                                                        uint8_t* __restrict__ contour) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)G * HW * K) return;
  const int k = (int)(item % K);
  const long long gp = item / K, g = gp / HW, p = gp % HW;
  const long long f = frames[g];
  const int kind = products[3 * k], a = products[3 * k + 1], b = products[3 * k + 2];
  float val = __uint_as_float(CL_NAN);
  if (kind == 0 && (a == 1 || a == 2)) {
    val = f == 0 ? 0.f : (float)((double)count[(g * 2 + a - 1) * HW + p] / (double)f);
  } else if (kind == 1 && a >= 0 && a < C && b >= 0 && b < 3) {
    const long long off = ((g * 3 + b) * HW + p) * C + a;
    const int nn = n[off];
    if (nn != 0) val = (float)(ldexp((double)sum[off], -bits[a]) / (double)nn);
  } else if (kind == 2 && a >= 0 && a < C && (b == 1 || b == 2)) {
    const long long off = (g * 3 * HW + p) * C + a;
    const long long sa = sum[off];
    if (sa != 0) val = (float)((double)sum[off + b * HW * C] / (double)sa);
  }
  out[item] = val;
  if (k == 0) {
    const float f1 = f == 0 ? 0.f : (float)((double)count[(g * 2) * HW + p] / (double)f);
    const float f2 = f == 0 ? 0.f : (float)((double)count[(g * 2 + 1) * HW + p] / (double)f);
    contour[gp] = f1 >= t1 ? 1 : (f2 >= t2 ? 2 : 0);
  }
}

}  // namespace dc

using namespace dc;

extern "C" int dc_climatology_block(int* pixels) {
  DC_REQUIRE(pixels, "dc_climatology_block: null argument");
  *pixels = CL_PIX;
  return 0;
}

extern "C" int dc_climatology_accumulate(int B, int H, int W, int G, const void* mask, int mask_bytes, const float* fields, int C, int ldc,
                                         const int32_t* chan, const int32_t* bits, const int32_t* group, int64_t* frames, int32_t* count,
                                         int64_t* sum, int32_t* n, void* stream) {
  DC_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "dc_climatology_accumulate: B must lie in [1, 65535], H and W must be positive");
  DC_REQUIRE((long)H * W < 2147483648L, "dc_climatology_accumulate: H * W must be below 2^31");
  DC_REQUIRE(G >= 1 && G <= 65536, "dc_climatology_accumulate: G must lie in [1, 65536]");
  DC_REQUIRE(mask_bytes == 1 || mask_bytes == 4 || mask_bytes == 8, "dc_climatology_accumulate: mask_bytes must be 1, 4 or 8");
  DC_REQUIRE(C >= 0 && C <= CL_MAXC, "dc_climatology_accumulate: C must lie in [0, 32]");
  DC_REQUIRE(mask && group && frames && count, "dc_climatology_accumulate: null pointer");
  DC_REQUIRE(((uintptr_t)mask & (mask_bytes - 1)) == 0, "dc_climatology_accumulate: the mask is not aligned to its element size");
  DC_REQUIRE(((uintptr_t)group & 3) == 0 && ((uintptr_t)frames & 7) == 0 && ((uintptr_t)count & 3) == 0,
             "dc_climatology_accumulate: group, frames or count not aligned to its element size");
  if (C > 0) {
    DC_REQUIRE(fields && bits && sum && n, "dc_climatology_accumulate: null pointer (fields, bits, sum and n are needed when C > 0)");
    DC_REQUIRE(ldc >= 1 && (chan != nullptr || ldc >= C), "dc_climatology_accumulate: ldc must be positive, and at least C when chan is null");
    DC_REQUIRE(((uintptr_t)fields & 3) == 0 && ((uintptr_t)bits & 3) == 0 && ((uintptr_t)chan & 3) == 0 && ((uintptr_t)sum & 7) == 0 &&
                   ((uintptr_t)n & 3) == 0,
               "dc_climatology_accumulate: fields, bits, chan, sum or n not aligned to its element size");
  } else {
    DC_REQUIRE(fields == nullptr, "dc_climatology_accumulate: fields given with C = 0");
  }
  hipStream_t st = (hipStream_t)stream;
  const long long HW = (long long)H * W;
  const unsigned blocks = (unsigned)((HW + CL_PIX - 1) / CL_PIX);
  // the vector form: the selection is the identity over all ldc channels, whole quads, every 16-byte piece aligned
  const bool vec = C > 0 && chan == nullptr && ldc == C && C % 4 == 0 && ((uintptr_t)fields & 15) == 0 && ((uintptr_t)sum & 15) == 0 &&
                   ((uintptr_t)n & 15) == 0;
  if (vec) {
    const int items = CL_PIX * (C / 4);
    hipLaunchKernelGGL(clim_accumulate_kernel<4>, dim3(blocks), dim3(items < 256 ? items : 256), 0, st, B, HW, G, mask, mask_bytes, fields, C,
                       ldc, chan, bits, group, (long long*)frames, count, (long long*)sum, n);
    DC_LAUNCHED("climatology_accumulate_vec");
  } else {
    const int items = CL_PIX * (C > 0 ? C : 1);
    hipLaunchKernelGGL(clim_accumulate_kernel<1>, dim3(blocks), dim3(items < 256 ? items : 256), 0, st, B, HW, G, mask, mask_bytes, fields, C,
                       ldc, chan, bits, group, (long long*)frames, count, (long long*)sum, n);
    DC_LAUNCHED("climatology_accumulate_scalar");
  }
  return 0;
}

extern "C" int dc_climatology_maps(int G, int H, int W, int C, const int64_t* frames, const int32_t* count, const int64_t* sum,
                                   const int32_t* n, const int32_t* bits, int K, const int32_t* products, float t1, float t2, float* out,
                                   uint8_t* contour, void* stream) {
  DC_REQUIRE(H >= 1 && W >= 1 && (long)H * W < 2147483648L, "dc_climatology_maps: H and W must be positive and H * W below 2^31");
  DC_REQUIRE(G >= 1 && G <= 65536, "dc_climatology_maps: G must lie in [1, 65536]");
  DC_REQUIRE(C >= 0 && C <= CL_MAXC, "dc_climatology_maps: C must lie in [0, 32]");
  DC_REQUIRE(K >= 1 && K <= 256, "dc_climatology_maps: K must lie in [1, 256]");
  DC_REQUIRE(frames && count && products && out && contour, "dc_climatology_maps: null pointer");
  DC_REQUIRE(C == 0 || (sum && n && bits), "dc_climatology_maps: null pointer (sum, n and bits are needed when C > 0)");
  DC_REQUIRE(((uintptr_t)frames & 7) == 0 && ((uintptr_t)sum & 7) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)n & 3) == 0 &&
                 ((uintptr_t)bits & 3) == 0 && ((uintptr_t)products & 3) == 0 && ((uintptr_t)out & 3) == 0,
             "dc_climatology_maps: a pointer is not aligned to its element size");
  const long long HW = (long long)H * W, items = HW * G * K;
  DC_REQUIRE((items + 255) / 256 < 2147483648LL, "dc_climatology_maps: G * H * W * K exceeds the grid");
  hipLaunchKernelGGL(clim_maps_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, HW, C,
                     (const long long*)frames, count, (const long long*)sum, n, bits, K, products, t1, t2, out, contour);
  DC_LAUNCHED("climatology_maps");
  return 0;
}
