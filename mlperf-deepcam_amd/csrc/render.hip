// Frame renderer: the visualiser's picture of a batch, made on the device (dc_render_frames; nn.FrameRenderer).  Per sample one or two
// panels (the prediction above the labels): one channel of the raw fields through a colour table, a graticule blended over it, and the
// outlines of class 1 and class 2 of the panel's mask blended over that.  include/deepcam_hip.h has the rule; everything after the colour
// index is integer arithmetic, and the index itself is two fp32 roundings that numpy repeats, so the bytes equal the checker's.
//   render_paint   source space, one workgroup per RP_TH x RP_TW tile of one sample and panel.  The classes of the tile and a halo of R + 1
//                  (R = (width - 1) / 2; columns modulo W, rows outside the image marked absent) go to LDS as one byte each; then the edge
//                  bytes of the tile and a halo of R (a class pixel with a 4-neighbour of another value; bit 0: class 1, bit 1: class 2);
//                  then the dilation by the (2R + 1)^2 square as a horizontal and a vertical OR.  One byte per source pixel and panel
//                  goes to the workspace.  Every byte of the valid samples' planes is written by every call: nothing of an earlier call
//                  survives in the workspace.
//   render_gather  output space, a thread takes four consecutive pixels of an output row for all panels: the field value is loaded and
//                  mapped through the colour table (in LDS, one word per entry) once, the graticule is blended once, then per panel the
//                  paint bytes decide the two outline blends.  12 bytes per thread and panel leave as three dwords, so a wave writes a
//                  contiguous run of 768 bytes; where W % 4 != 0 or `out` is not 4-byte aligned the same code stores single bytes.
// The field load is strided by ldc floats: with ldc = 16 one dword of every 64-byte segment is used.
#include "common.h"
#include "mask_skill.h"

namespace dc {

static constexpr int RP_TH = 32, RP_TW = 64;      // the source tile: 2048 pixels, 8 per thread of a 256-thread workgroup
static constexpr int RP_RMAX = 3;                 // width 7
static constexpr int RP_CW = RP_TW + 2 * (RP_RMAX + 1), RP_CH = RP_TH + 2 * (RP_RMAX + 1);   // classes: 72 x 40
static constexpr int RP_EW = RP_TW + 2 * RP_RMAX, RP_EH = RP_TH + 2 * RP_RMAX;               // edges: 70 x 38
static constexpr uint8_t RP_ABSENT = 0xff;        // a row outside the image: neither a class nor a neighbour that counts

// classes 1 and 2 of a mask element; every other value is background
__device__ inline uint8_t rp_class(const void* m, size_t i, int bytes) {
  const long long v = mask_value(m, i, bytes);
  return (v == 1 || v == 2) ? (uint8_t)v : (uint8_t)0;
}

__global__ __launch_bounds__(256) void render_paint_kernel(int H, int W, int P, const void* __restrict__ mask_a, int a_bytes,
                                                           const void* __restrict__ mask_b, int b_bytes, int R, uint8_t* __restrict__ paint) {
  __shared__ uint8_t s_cls[RP_CH * RP_CW];        // [lr + h][lc + h], h = R + 1
  __shared__ uint8_t s_edge[RP_EH * RP_EW];       // [lr + R][lc + R]
  __shared__ uint8_t s_hor[RP_EH * RP_TW];        // [lr + R][lc]
  const int b = blockIdx.z / P, p = blockIdx.z % P;
  const void* mask = p == 0 ? mask_a : mask_b;
  const int bytes = p == 0 ? a_bytes : b_bytes;
  const size_t HW = (size_t)H * W, base = (size_t)b * HW;
  const int r0 = blockIdx.y * RP_TH, c0 = blockIdx.x * RP_TW;
  const int h = R + 1;
  {                                               // 1. classes with a halo of h
    const int cw = RP_TW + 2 * h, n = (RP_TH + 2 * h) * cw;
    int cfirst = (c0 - h) % W;                    // the global column of LDS column 0
    if (cfirst < 0) cfirst += W;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int lr = i / cw, lc = i % cw;
      const int r = r0 - h + lr, c = (cfirst + lc) % W;
      s_cls[lr * RP_CW + lc] = (r >= 0 && r < H) ? rp_class(mask, base + (size_t)r * W + c, bytes) : RP_ABSENT;
    }
  }
  __syncthreads();
  {                                               // 2. edge bytes with a halo of R
    const int ew = RP_TW + 2 * R, n = (RP_TH + 2 * R) * ew;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int lr = i / ew, lc = i % ew;
      const uint8_t* q = s_cls + (lr + 1) * RP_CW + lc + 1;
      const uint8_t k = *q;
      uint8_t e = 0;
      if (k == 1 || k == 2) {
        const uint8_t up = q[-RP_CW], dn = q[RP_CW];
        const bool other = (up != k && up != RP_ABSENT) || (dn != k && dn != RP_ABSENT) || q[-1] != k || q[1] != k;
        e = other ? k : (uint8_t)0;               // class 1: bit 0, class 2: bit 1
      }
      s_edge[lr * RP_EW + lc] = e;
    }
  }
  __syncthreads();
  {                                               // 3. OR along the row
    const int n = (RP_TH + 2 * R) * RP_TW;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int lr = i / RP_TW, lc = i % RP_TW;
      const uint8_t* q = s_edge + lr * RP_EW + lc;
      uint8_t v = 0;
      for (int d = 0; d <= 2 * R; ++d) v |= q[d];
      s_hor[i] = v;
    }
  }
  __syncthreads();
  uint8_t* plane = paint + (size_t)blockIdx.z * HW;
#pragma unroll
  for (int k = 0; k < RP_TH * RP_TW / 256; ++k) {  // 4. OR along the column, one byte per source pixel
    const int i = threadIdx.x + k * 256, lr = i / RP_TW, lc = i % RP_TW;
    const int r = r0 + lr, c = c0 + lc;
    if (r >= H || c >= W) continue;
    uint8_t v = 0;
    for (int d = 0; d <= 2 * R; ++d) v |= s_hor[(lr + d) * RP_TW + lc];
    plane[(size_t)r * W + c] = v;
  }
}
static_assert(RP_TH * RP_TW % 256 == 0, "render_paint_kernel: whole pixels per thread");

struct RpColours {
  int missing_rgb, line_argb, class1_argb, class2_argb;
};

// fg (0xAARRGGBB) over rgb (0x00BBGGRR, the byte order of `out`): every channel (fg * a + old * (255 - a) + 127) / 255
__device__ inline unsigned rp_blend(unsigned rgb, int argb) {
  const unsigned a = ((unsigned)argb >> 24) & 255u, na = 255u - a;
  const unsigned r = (((unsigned)argb >> 16) & 255u) * a + (rgb & 255u) * na + 127u;
  const unsigned g = (((unsigned)argb >> 8) & 255u) * a + ((rgb >> 8) & 255u) * na + 127u;
  const unsigned bl = ((unsigned)argb & 255u) * a + ((rgb >> 16) & 255u) * na + 127u;
  return (r / 255u) | ((g / 255u) << 8) | ((bl / 255u) << 16);
}

// VEC: W % 4 == 0 and `out` 4-byte aligned, so a thread's four pixels exist and their 12 bytes are three aligned dwords
template <bool VEC>
__global__ __launch_bounds__(256) void render_gather_kernel(int H, int W, int P, const float* __restrict__ fields, int ch, int ldc, float lo,
                                                            float scale, const uint8_t* __restrict__ lut, int nlut,
                                                            const uint8_t* __restrict__ paint, const int32_t* __restrict__ src_row, int Ho,
                                                            int shift, const uint8_t* __restrict__ row_line,
                                                            const uint8_t* __restrict__ col_line, RpColours col, uint8_t* __restrict__ out) {
  __shared__ unsigned s_lut[256];
  for (int i = threadIdx.x; i < nlut; i += 256) s_lut[i] = (unsigned)lut[3 * i] | ((unsigned)lut[3 * i + 1] << 8) | ((unsigned)lut[3 * i + 2] << 16);
  __syncthreads();
  const int nchunk = (W + 3) / 4;
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long)Ho * nchunk) return;
  const int y = (int)(item / nchunk), x0 = (int)(item % nchunk) * 4;
  const int b = blockIdx.y;
  int r = src_row[y];
  r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
  const size_t HW = (size_t)H * W, row = (size_t)r * W;
  const float* frow = fields + ((size_t)b * HW + row) * ldc + ch;
  const bool yline = row_line[y] != 0;
  int c[4];
  unsigned base[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j;
    c[j] = x + shift < W ? x + shift : x + shift - W;          // x < W and shift < W; beyond the row's end (scalar path only): unused
    base[j] = 0u;
    if (!VEC && x >= W) continue;
    const float v = frow[(size_t)c[j] * ldc];
    unsigned rgb;
    if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) {    // NaN, +-Inf
      rgb = (((unsigned)col.missing_rgb >> 16) & 255u) | ((unsigned)col.missing_rgb & 0xff00u) | (((unsigned)col.missing_rgb & 255u) << 16);
    } else {
      const float t = __fmul_rn(__fsub_rn(v, lo), scale);
      int i;
      if (!(t > 0.f)) i = 0;
      else if (t >= 1.f) i = nlut - 1;
      else {
        i = (int)__fmul_rn(t, (float)nlut);
        i = i > nlut - 1 ? nlut - 1 : i;
      }
      rgb = s_lut[i];
    }
    if (yline || col_line[x] != 0) rgb = rp_blend(rgb, col.line_argb);
    base[j] = rgb;
  }
  for (int p = 0; p < P; ++p) {
    const uint8_t* prow = paint + ((size_t)b * P + p) * HW + row;
    unsigned pb[4];
    if (VEC && (shift & 3) == 0) {                // c[0] % 4 == 0 and c[0] + 3 < W: the four bytes are one aligned word
      const unsigned w = *(const unsigned*)(prow + c[0]);
#pragma unroll
      for (int j = 0; j < 4; ++j) pb[j] = (w >> (8 * j)) & 255u;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) pb[j] = (VEC || x0 + j < W) ? prow[c[j]] : 0u;
    }
    unsigned px[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned rgb = base[j];
      if (pb[j] & 1u) rgb = rp_blend(rgb, col.class1_argb);
      if (pb[j] & 2u) rgb = rp_blend(rgb, col.class2_argb);
      px[j] = rgb;
    }
    uint8_t* o = out + ((((size_t)b * P + p) * Ho + y) * W + x0) * 3;
    if (VEC) {
      unsigned* o4 = (unsigned*)o;
      o4[0] = px[0] | (px[1] << 24);
      o4[1] = (px[1] >> 8) | (px[2] << 16);
      o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x0 + j >= W) continue;
        o[3 * j + 0] = (uint8_t)(px[j] & 255u);
        o[3 * j + 1] = (uint8_t)((px[j] >> 8) & 255u);
        o[3 * j + 2] = (uint8_t)((px[j] >> 16) & 255u);
      }
    }
  }
}

static inline size_t rp_align(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace dc

using namespace dc;

extern "C" int dc_render_tile(int* th, int* tw) {
  DC_REQUIRE(th && tw, "dc_render_tile: null argument");
  *th = RP_TH;
  *tw = RP_TW;
  return 0;
}

// the workspace: paint uint8 [B][panels][H][W]
extern "C" size_t dc_render_workspace(int B, int panels, int H, int W) {
  if (B <= 0 || panels < 1 || panels > 2 || H < 1 || W < 8 || (long)H * W >= 2147483648L) return 0;
  return rp_align((size_t)B * panels * H * W);
}

extern "C" int dc_render_frames(int B, int n_valid, int H, int W, const float* fields, int ch, int ldc, float lo, float scale,
                                const uint8_t* lut, int nlut, const void* mask_a, int a_bytes, const void* mask_b, int b_bytes,
                                const int32_t* src_row, int Ho, int shift, const uint8_t* row_line, const uint8_t* col_line, int missing_rgb,
                                int line_argb, int class1_argb, int class2_argb, int width, uint8_t* out, void* workspace, void* stream) {
  DC_REQUIRE(B > 0 && H >= 1 && W >= 8, "dc_render_frames: B and H must be positive and W at least 8");
  DC_REQUIRE((long)H * W < 2147483648L, "dc_render_frames: H * W must be below 2^31");
  DC_REQUIRE(n_valid > 0 && n_valid <= B, "dc_render_frames: n_valid must lie in [1, B]");
  DC_REQUIRE(n_valid <= 32767, "dc_render_frames: at most 32767 samples per call");
  DC_REQUIRE(Ho >= 1 && (long)Ho * W < 2147483648L, "dc_render_frames: Ho must be positive and Ho * W below 2^31");
  DC_REQUIRE(ldc >= 1 && ch >= 0 && ch < ldc, "dc_render_frames: ch must lie in [0, ldc)");
  DC_REQUIRE(nlut >= 1 && nlut <= 256, "dc_render_frames: nlut must lie in [1, 256]");
  DC_REQUIRE(shift >= 0 && shift < W, "dc_render_frames: shift must lie in [0, W)");
  DC_REQUIRE(width == 1 || width == 3 || width == 5 || width == 7, "dc_render_frames: width must be 1, 3, 5 or 7");
  DC_REQUIRE(a_bytes == 1 || a_bytes == 4 || a_bytes == 8, "dc_render_frames: a_bytes must be 1, 4 or 8");
  DC_REQUIRE(mask_b == nullptr || b_bytes == 1 || b_bytes == 4 || b_bytes == 8, "dc_render_frames: b_bytes must be 1, 4 or 8");
  DC_REQUIRE(fields && lut && mask_a && src_row && row_line && col_line && out && workspace, "dc_render_frames: null pointer");
  DC_REQUIRE(((uintptr_t)workspace & 255) == 0, "dc_render_frames: workspace not 256-byte aligned");
  DC_REQUIRE(((uintptr_t)fields & 3) == 0 && ((uintptr_t)src_row & 3) == 0, "dc_render_frames: fields or src_row not 4-byte aligned");
  DC_REQUIRE(((uintptr_t)mask_a & (a_bytes - 1)) == 0 && (mask_b == nullptr || ((uintptr_t)mask_b & (b_bytes - 1)) == 0),
             "dc_render_frames: a mask is not aligned to its element size");
  DC_REQUIRE((H + RP_TH - 1) / RP_TH <= 65535, "dc_render_frames: H exceeds 65535 tile rows");
  hipStream_t st = (hipStream_t)stream;
  const int P = mask_b ? 2 : 1;
  const int tx = (W + RP_TW - 1) / RP_TW, ty = (H + RP_TH - 1) / RP_TH;
  uint8_t* paint = (uint8_t*)workspace;
  hipLaunchKernelGGL(render_paint_kernel, dim3(tx, ty, n_valid * P), dim3(256), 0, st, H, W, P, mask_a, a_bytes, mask_b, b_bytes,
                     (width - 1) / 2, paint);
  DC_LAUNCHED("render_paint");
  RpColours col;
  col.missing_rgb = missing_rgb;
  col.line_argb = line_argb;
  col.class1_argb = class1_argb;
  col.class2_argb = class2_argb;
  const long items = (long)Ho * ((W + 3) / 4);
  const dim3 grid((unsigned)((items + 255) / 256), n_valid);
  if (W % 4 == 0 && ((uintptr_t)out & 3) == 0)
    hipLaunchKernelGGL(render_gather_kernel<true>, grid, dim3(256), 0, st, H, W, P, fields, ch, ldc, lo, scale, lut, nlut, paint, src_row, Ho,
                       shift, row_line, col_line, col, out);
  else
    hipLaunchKernelGGL(render_gather_kernel<false>, grid, dim3(256), 0, st, H, W, P, fields, ch, ldc, lo, scale, lut, nlut, paint, src_row, Ho,
                       shift, row_line, col_line, col, out);
  DC_LAUNCHED("render_gather");
  return 0;
}
