// Register epilogue of the pointwise tile kernels pw384_kernel and pw192_kernel: from the MFMA accumulators to 16-byte stores and the BatchNorm
// partial sums of the stored values, without a pass through LDS for the outputs.  (pw224_kernel keeps the same steps written out in
// igemm224.hip: its K loop and registers came out differently with this function, and slower.)
//
// A lane holds, per MFMA tile (i, j), channels fg*4 .. +3 of channel block i for pixel fr of pixel block j: 8 bytes.  Lanes l and l ^ 16 trade
// halves of two tiles so that each ends up with 8 consecutive channels of one pixel: 64 contiguous bytes per pixel and store instruction.
#pragma once
#include "igemm.h"
#include "mfma_tile.h"

namespace dc {

// The trade.  (a0, a1) and (b0, b1) are this lane's 4 + 4 values (packed bf16) of tiles A and B.  The even-fg lane keeps A and receives its
// partner's A as the upper half; the odd-fg lane keeps B as the upper half and receives its partner's B as the lower one.
__device__ inline vec16 trade_halves(bool odd, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
  const uint32_t r0 = swap_rows16(odd ? a0 : b0), r1 = swap_rows16(odd ? a1 : b1);
  vec16 v;
  v.w[0] = odd ? r0 : a0;
  v.w[1] = odd ? r1 : a1;
  v.w[2] = odd ? b0 : r0;
  v.w[3] = odd ? b1 : r1;
  return v;
}

// One 16-byte vector on its way out: the optional accumulate (read-modify-write, rounded to bf16 again), the store, and this lane's running
// sums st[sum, sum of squares][channel] of the values as STORED.
__device__ inline void store_and_sum(bf16* dst, vec16 v, bool accumulate, bool do_stats, float (&st)[2][8]) {
  float f[8];
  unpack(v, f, bf16());
  if (accumulate) {
    float o[8];
    unpack(ldg16(dst), o, bf16());
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] += o[e];
    pack(v, f, bf16());
    unpack(v, f, bf16());
  }
  stg16(dst, v);
  if (do_stats) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      st[0][e] += f[e];
      st[1][e] = fmaf(f[e], f[e], st[1][e]);
    }
  }
}

// sums over the 16 pixel lanes of a DPP row; lane fr of the row keeps value fr (which = fr >> 3, channel e = fr & 7)
__device__ inline float row_sums_keep_mine(const float (&st)[2][8], int fr) {
  float mine = 0.f;
#pragma unroll
  for (int w = 0; w < 2; ++w)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = row_sum16(st[w][e]);
      if (fr == w * 8 + e) mine = t;
    }
  return mine;
}

// Two adjacent channel blocks (acc[i0]: channels cpair .. + 15 of the tile, acc[i0 + 1]: cpair + 16 .. + 31) of a wave's NPB pixel blocks: bias, the
// trade, store_and_sum per pixel block, and the wave's sums into red[pixel group][sum, sum of squares][TN] (the kernel folds red[] into its
// slab row or sum row behind a barrier).  n0: first channel of the tile; mg: first pixel of the wave's pixel group grp; fr = lane & 15,
// fg = lane >> 4.
template <int TN, int NCB, int NPB>
__device__ inline void pw_epilogue_pair(const IgemmParams& p, const f32x4 (&acc)[NCB][NPB], int i0, int n0, int cpair, int mg, int grp,
                                                 int fr, int fg, float* red) {
  const int Cout = p.g.Cout;
  const bool odd = fg & 1;
  const bool do_stats = p.slab != nullptr;
  bf16* __restrict__ yg = reinterpret_cast<bf16*>(p.y);
  const int chl = cpair + (odd ? 16 : 0) + (fg >> 1) * 8;                       // first of this lane's 8 channels after the trade
  const int ch0 = n0 + chl;
  const bool chok = ch0 < Cout;                                                 // Cout is a multiple of 8: all or nothing
  float ba[4] = {0.f, 0.f, 0.f, 0.f}, bb[4] = {0.f, 0.f, 0.f, 0.f};             // bias of the channels this lane COMPUTED
  if (p.bias != nullptr) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ca = n0 + cpair + fg * 4 + r, cb = ca + 16;
      if (ca < Cout) ba[r] = p.bias[ca];
      if (cb < Cout) bb[r] = p.bias[cb];
    }
  }
  float st[2][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) st[0][e] = st[1][e] = 0.f;
#pragma unroll
  for (int j = 0; j < NPB; ++j) {
    const int m = mg + j * 16 + fr;
    const uint32_t a0 = pack2_bf16(acc[i0][j][0] + ba[0], acc[i0][j][1] + ba[1]);
    const uint32_t a1 = pack2_bf16(acc[i0][j][2] + ba[2], acc[i0][j][3] + ba[3]);
    const uint32_t b0 = pack2_bf16(acc[i0 + 1][j][0] + bb[0], acc[i0 + 1][j][1] + bb[1]);
    const uint32_t b1 = pack2_bf16(acc[i0 + 1][j][2] + bb[2], acc[i0 + 1][j][3] + bb[3]);
    const vec16 v = trade_halves(odd, a0, a1, b0, b1);
    if (m < p.M && chok) store_and_sum(yg + (size_t)m * p.ldy + ch0, v, p.accumulate, do_stats, st);
  }
  if (do_stats) red[(grp * 2 + (fr >> 3)) * TN + chl + (fr & 7)] = row_sums_keep_mine(st, fr);
}

}  // namespace dc
