// Train-time augmentation on the periodic grid (dc_augment_view_hwc; data.Augment, data.InputPipeline(augment=...), train.py
// --augment_roll / --augment_flip_lat / --augment_negate / --augment_seed).  ensemble.hip's view of the input gives ONE (roll, flip) to a whole
// batch and has no labels; the training pipeline wants every sample of a batch at a longitude offset of its own, the mirrored ones with the
// meridional winds negated, and the int64 label map moved with the fields -- in one launch on the copy stream, where today there is one.
// Definitions (include/deepcam_hip.h has them with the ABI; tests/util_augment.py states them again in numpy):
//   view       (roll_n, flip_n) of sample n, 0 <= roll_n < W: view pixel (h, w) shows source pixel src_n(h, w) = (flip_n ? H - 1 - h : h,
//              (w + roll_n) mod W) -- ensemble.hip's.
//   data       out[n, h, w, j] = scale[j] * (s_nj * x[n, src_n(h, w), channels[j]] - shift[j]) in the activation dtype, s_nj = flip_sign[j]
//              where flip_n is set and flip_sign is given, else +1: view_normalize_kernel's expression, so that sample n carries the bits
//              dc_input_view_hwc writes for it alone with (roll_n, flip_n) and sign = flip_n ? flip_sign : NULL, and a batch of identity
//              views the bits of dc_input_normalize_hwc.  +-1 * v is exact, contracted with the subtraction or not.
//   labels     labels_out[n, h, w] = labels_in[n, src_n(h, w)]: 64-bit words moved as they are, never interpreted.
// The views table is HOST memory: it is range-checked and packed, one 32-bit word per sample (bit 31 the flip, the roll below), into the
// kernel arguments before the call returns -- 1 KB at the bound of 256 samples.  The device never indexes by a number the host has not
// checked; a row's word is the same for every lane of its workgroup and is read with a scalar load from the argument segment; there is no
// table in device memory, no extra copy and no pinned buffer.
// The decomposition is view_normalize's: blockIdx.y walks the rows of the batch, a row of the view is a rotated row of the source, a thread
// takes one 16-byte vector of one output pixel.  With all file channels in file order the loads are 16 bytes wide too (the roll moves
// whole pixels and the flip whole rows, so the alignment never breaks); a channel selection gathers by 4-byte loads.  The workgroups of a
// row then move its labels, one 8-byte word per thread.  One stream over the batch: no atomics, no LDS.
#include "common.h"

namespace dc {

static constexpr int AUG_BMAX = 256;                // samples of one call: the table is 1 KB of kernel arguments
static constexpr unsigned AUG_FLIP = 0x80000000u;   // bit 31 of a packed view; the roll (< W <= 2^30) below it

struct AugViews {
  uint32_t w[AUG_BMAX];
};

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void augment_view_kernel(int rows, int H, int W, int Cfile, int Cc, const int* __restrict__ channels,
                                                           const float* __restrict__ flip_sign, const float* __restrict__ x,
                                                           const float* __restrict__ shift, const float* __restrict__ scale,
                                                           const long long* __restrict__ labels_in, long long* __restrict__ labels_out,
                                                           T* __restrict__ out, int ldo, const AugViews views) {
  constexpr int KPV = Elem<T>::kPerVec;
  const int ngroups = Cc / KPV;
  const long per_row = (long)W * ngroups;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int n = row / H, h = row - n * H;         // n < B <= AUG_BMAX: rows = B * H
    const unsigned view = views.w[n];               // the same for the whole workgroup
    const int roll = (int)(view & ~AUG_FLIP);
    const bool flip = (view & AUG_FLIP) != 0u;
    const int hs = flip ? H - 1 - h : h;
    const float* sign = flip ? flip_sign : nullptr;
    const size_t srow = (size_t)n * H + hs;
    const float* xr = x + srow * W * Cfile;
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
    if (labels_in != nullptr) {
      const long long* lr = labels_in + srow * W;
      long long* lo = labels_out + (size_t)row * W;
      for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < W; w += gridDim.x * blockDim.x) {
        int ws = w + roll;
        if (ws >= W) ws -= W;
        lo[w] = lr[ws];
      }
    }
  }
}

}  // namespace dc

using namespace dc;

extern "C" int dc_augment_view_hwc(int dtype, int B, int H, int W, int Cfile, int C, const int* channels, const float* flip_sign,
                                   const float* x_hwc, const float* shift, const float* scale, const int32_t* views_host,
                                   const int64_t* labels_in, int64_t* labels_out, void* out, int ldo, void* stream) {
  DC_REQUIRE(B >= 1 && B <= AUG_BMAX && H >= 1 && W >= 1, "dc_augment_view_hwc: B must lie in [1, 256], H and W must be positive");
  DC_REQUIRE((long)H * W <= (1L << 30), "dc_augment_view_hwc: H * W must not exceed 2^30");
  DC_REQUIRE((long)B * H <= 2147483647L, "dc_augment_view_hwc: B * H must be below 2^31");
  DC_REQUIRE(dtype == DC_F32 || dtype == DC_BF16, "dc_augment_view_hwc: dtype must be DC_F32 or DC_BF16");
  if (int e = dc_check_view(out, ldo, C, dtype, "dc_augment_view_hwc out")) return e;
  DC_REQUIRE(x_hwc && shift && scale && views_host && Cfile >= C,
             "dc_augment_view_hwc: null pointer, or fewer file channels than selected ones");
  DC_REQUIRE((labels_in == nullptr) == (labels_out == nullptr), "dc_augment_view_hwc: labels_in and labels_out are given together or not at all");
  DC_REQUIRE(labels_in == nullptr || labels_in != labels_out, "dc_augment_view_hwc: the labels cannot be moved in place");
  DC_REQUIRE(((uintptr_t)x_hwc & 3) == 0 && ((uintptr_t)shift & 3) == 0 && ((uintptr_t)scale & 3) == 0 && ((uintptr_t)flip_sign & 3) == 0 &&
                 ((uintptr_t)channels & 3) == 0 && ((uintptr_t)views_host & 3) == 0 && ((uintptr_t)labels_in & 7) == 0 &&
                 ((uintptr_t)labels_out & 7) == 0, "dc_augment_view_hwc: a pointer is not aligned to its element size");
  AugViews views;
  for (int n = 0; n < B; ++n) {
    const int roll = views_host[2 * n], flip = views_host[2 * n + 1];
    if (roll < 0 || roll >= W || (flip != 0 && flip != 1)) {
      char msg[160];
      snprintf(msg, sizeof(msg), "dc_augment_view_hwc: view %d is (%d, %d): roll must lie in [0, W) and flip must be 0 or 1", n, roll, flip);
      return dc_fail(msg, __FILE__, __LINE__);
    }
    views.w[n] = (uint32_t)roll | (flip ? AUG_FLIP : 0u);
  }
  for (int n = B; n < AUG_BMAX; ++n) views.w[n] = 0u;
  const int kpv = dtype == DC_BF16 ? 8 : 4;
  const long per_row = (long)W * (C / kpv);
  const int rows = B * H;
  const unsigned gx = (unsigned)(per_row < 256L * 32 ? (per_row + 255) / 256 : 32);
  const unsigned gy = (unsigned)(rows < (int)(8192 / gx) ? rows : 8192 / gx);
  const bool vec = channels == nullptr && Cfile % 4 == 0 && ((uintptr_t)x_hwc & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
#define AUGMENT(TT, VV)                                                                                                                      \
  hipLaunchKernelGGL((augment_view_kernel<TT, VV>), dim3(gx, gy), dim3(256), 0, st, rows, H, W, Cfile, C, channels, flip_sign, x_hwc, shift, \
                     scale, (const long long*)labels_in, (long long*)labels_out, (TT*)out, ldo, views)
  if (dtype == DC_BF16) {
    if (vec) AUGMENT(bf16, true); else AUGMENT(bf16, false);
  } else {
    if (vec) AUGMENT(float, true); else AUGMENT(float, false);
  }
#undef AUGMENT
  DC_LAUNCHED("augment_view");
  return 0;
}
