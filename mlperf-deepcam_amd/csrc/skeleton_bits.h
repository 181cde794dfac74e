// What the kernels that keep a class plane of one frame as a bit plane in the LDS of one CU share (skeleton.hip: th_thin_kernel;
// skeleton_prune.hip: sp_prune_kernel): the plane's geometry and limits, the class of a lane's pixel for the wave ballot that packs a
// word, and the eight neighbour planes of a word with the funnel shifts that handle the seam.  skeleton.hip has the layout's reasons.
#pragma once
#include "event_common.h"
#include "mask_skill.h"

namespace dc {

static constexpr int TH_THREADS = 1024, TH_WAVES = TH_THREADS / 64;
static constexpr int TH_WPT = 20;                 // words a thread owns at most
static constexpr int TH_SCRATCH = 64;             // bytes behind the plane: the two "anything changed" flags and "not empty"
static constexpr int TH_LDS_MAX = 160 * 1024;     // a gfx950 CU
static_assert((size_t)TH_THREADS * TH_WPT * 8 + TH_SCRATCH >= TH_LDS_MAX, "th_thin: the threads' words cover every plane the LDS holds");

typedef unsigned long long u64;

static inline size_t th_lds_bytes(int H, int W) {
  if (H < 1 || W < 1) return 0;
  const size_t bytes = (size_t)H * ((size_t)(W + 63) / 64) * 8 + TH_SCRATCH;
  return bytes <= (size_t)TH_LDS_MAX ? bytes : 0;
}

// the plane of the western / eastern neighbours of a word's 64 pixels: a funnel shift with the word to the left / right.  `in` is the bit
// that enters: for an inner word the neighbouring word's bit 63 / bit 0; at the seam the row's other end under wrap, 0 without.
__device__ inline u64 th_west(u64 x, u64 left, bool first, int lastbit, int wrap) {
  const u64 in = first ? (wrap ? (left >> lastbit) & 1ull : 0ull) : left >> 63;      // first: `left` is the row's last word
  return (x << 1) | in;
}
__device__ inline u64 th_east(u64 x, u64 right, bool last, int lastbit, int wrap) {
  const u64 in = last ? (wrap ? (right & 1ull) << lastbit : 0ull) : right << 63;     // last: `right` is the row's first word
  return (x >> 1) | in;
}

// the eight neighbour planes of word i (value c) of the plane P: p[0] = P2 (north), clockwise to p[7] = P9 (north-west).  Eight LDS reads.
__device__ inline void th_ring(const u64* P, int i, u64 c, int H, int TW, int lastbit, int wrap, u64* p) {
  const int r = i / TW, cw = i - r * TW;
  const bool first = cw == 0, last = cw == TW - 1;
  const int il = first ? i + TW - 1 : i - 1, ir = last ? i - cw : i + 1;
  const u64 ml = P[il], mr = P[ir];
  u64 u = 0, ul = 0, ur = 0, d = 0, dl = 0, dr = 0;
  if (r > 0) u = P[i - TW], ul = P[il - TW], ur = P[ir - TW];          // rows outside the frame are background
  if (r < H - 1) d = P[i + TW], dl = P[il + TW], dr = P[ir + TW];
  p[0] = u, p[1] = th_east(u, ur, last, lastbit, wrap), p[2] = th_east(c, mr, last, lastbit, wrap);
  p[3] = th_east(d, dr, last, lastbit, wrap), p[4] = d, p[5] = th_west(d, dl, first, lastbit, wrap);
  p[6] = th_west(c, ml, first, lastbit, wrap), p[7] = th_west(u, ul, first, lastbit, wrap);
}

// the class (0, 1, 2) of lane `lane`'s pixel of word `item`; TH_NONE where the word or the column lies outside the plane
static constexpr unsigned TH_NONE = 3u;
static constexpr int TH_BATCH = 4;                // words whose loads a wave keeps in flight together
__device__ inline unsigned th_class(const void* __restrict__ mask, int mask_bytes, size_t base, int item, int n, int TW, int W, int lane) {
  if (item >= n) return TH_NONE;
  const int r = item / TW, col = (item - r * TW) * 64 + lane;
  return col < W ? mask_class(mask, base + (size_t)r * W + col, mask_bytes) : TH_NONE;
}

}  // namespace dc
