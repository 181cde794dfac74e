// Displacement verification: the overlap of the labelled mask with the predicted mask moved by every (dy, dx) of a window of +-R rows and
// columns -- the cross-correlation of two binary fields, per frame and class (1, 2) -- and the shift with the most hits: the rigid-shift
// part of Ebert & McBride's CRA method (dc_displacement_score; nn.DisplacementSkill).  Columns are periodic, rows never: pixels moved over
// a pole are lost.  Integers end to end.  include/deepcam_hip.h has the definitions; this file has the decomposition.
// A wave's ballot packs 64 pixels of a class into one word, and a shift becomes a funnel shift, an AND and a popcount:
//   disp_pack   a workgroup takes one row of one frame and reads both masks.  A wave takes 64 consecutive pixels and __ballot of the class
//               test is the word.  The two label planes are TW = ceil(W / 64) words a row, the bits from W on zero.  The two prediction
//               planes are EXTENDED rows with a periodic halo: bit i of a row is P[(i - R) mod W] for i < W + 2 R and zero behind, PW =
//               ceil((W + 2 R) / 64) + 1 words with the spare one.  The 64 bits that meet label word w under the shift dx are then the
//               bits 64 w + (R - dx) .. + 63 of the extended row: two neighbouring words, whatever W and wherever the seam.  The halo
//               pixels are read a second time (2 R of W); the own bits R .. R + W of a row give the row's predicted pixels, from which
//               `kept` follows, and with the label words the frame's `pixels` (four 64-bit atomics per row at most).
//   disp_corr   a workgroup takes one (frame, class, dy) and a segment of DP_SEG rows of the band.  Lane t <= 2 R is dx = t - R; lane
//               2 R + 1 is the `kept` lane; one wave where 2 R + 2 <= 64, else two.  Per label row y and prediction row y - dy (inside
//               the frame: a uniform bound) the label word is the same for all lanes, a uniform load, and a zero word -- nearly every one
//               on real frames -- is skipped by a uniform branch; else a lane funnels its word out of two words of the extended row,
//               ANDs, popcounts and adds into a 32-bit register (a segment holds fewer than 2^31 pixels).  The kept lane adds the row
//               count of every prediction row it meets.  At the end one 64-bit atomic per lane with a non-zero count: lane t is cell t
//               of row dy + R.  No reduction across lanes, no LDS.
//   disp_best   a workgroup per (frame, class) takes the maximum of the 64-bit key over the table and writes (dy, dx, hits, kept[dy]).
//   disp_total  one thread per cell adds the batch's rows and pixels to the totals, frame by frame; one the frame count.
// The workspace holds the four bit planes and the row counts.  Four launches per call.
#include "common.h"
#include "mask_skill.h"

namespace dc {

static constexpr int DP_BITS = 64;                // pixels of a word = lanes of a wave
static constexpr int DP_SEG = 32;                 // label rows of a workgroup of disp_corr
static constexpr int DP_RMAX = 63;                // 2 R + 2 lanes fit two waves; the key holds dy + R and dx + R in 7 bits each
static constexpr int DP_BMAX = 4095;              // a legal grid.y
static constexpr int DP_PACK = 256;               // threads of disp_pack: four waves share a row's words

__global__ __launch_bounds__(DP_PACK) void disp_pack_kernel(int H, int W, const void* __restrict__ pred, int pred_bytes,
                                                            const void* __restrict__ truth, int truth_bytes, int R, int row0, int row1,
                                                            int TW, int PW, unsigned long long* __restrict__ lab,
                                                            unsigned long long* __restrict__ ext, uint32_t* __restrict__ cnt,
                                                            unsigned long long* __restrict__ pixels) {
  __shared__ unsigned red[DP_PACK / 64][4];
  const int b = blockIdx.y, y = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t row = ((size_t)b * H + y) * W;
  const size_t plane = (size_t)b * 2 * H + y;      // the row of class 1's plane; class 2's is H rows on
  unsigned n[4] = {0, 0, 0, 0};                     // pred 1, pred 2, truth 1, truth 2 of this wave's words
  for (int item = wave; item < PW + TW; item += DP_PACK / 64) {      // the same for the whole wave: every lane votes
    if (item < PW) {
      const int i = item * DP_BITS + lane;          // bit of the extended row
      unsigned c = 0;
      if (i < W + 2 * R) {
        int x = i - R;                              // in [-R, W + R), where R < W
        x = x < 0 ? x + W : (x >= W ? x - W : x);
        c = mask_class(pred, row + x, pred_bytes);
      }
      const unsigned long long m1 = __ballot(c == 1u), m2 = __ballot(c == 2u);
      const unsigned long long own = __ballot(i >= R && i < R + W);   // the bits that are the row itself
      n[0] += (unsigned)__popcll(m1 & own), n[1] += (unsigned)__popcll(m2 & own);
      if (lane == 0) ext[plane * PW + item] = m1, ext[(plane + H) * PW + item] = m2;
    } else {
      const int w = item - PW, j = w * DP_BITS + lane;
      const unsigned c = j < W ? mask_class(truth, row + j, truth_bytes) : 0u;
      const unsigned long long m1 = __ballot(c == 1u), m2 = __ballot(c == 2u);
      n[2] += (unsigned)__popcll(m1), n[3] += (unsigned)__popcll(m2);
      if (lane == 0) lab[plane * TW + w] = m1, lab[(plane + H) * TW + w] = m2;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < 4; ++f) red[wave][f] = n[f];
  }
  __syncthreads();
  if (t < 4) {
    unsigned sum = 0;
#pragma unroll
    for (int w = 0; w < DP_PACK / 64; ++w) sum += red[w][t];
    const int k = t & 1;
    if (t < 2) {                                    // predicted: the row count, and the pixels of the whole frame
      cnt[plane + (size_t)k * H] = sum;
      if (sum) atomicAdd(pixels + ((size_t)b * 2 + k) * 2, (unsigned long long)sum);
    } else if (sum && y >= row0 && y < row1) {      // labelled: inside the band
      atomicAdd(pixels + ((size_t)b * 2 + k) * 2 + 1, (unsigned long long)sum);
    }
  }
}

__global__ __launch_bounds__(128) void disp_corr_kernel(int H, int R, int row0, int row1, int nseg, int TW, int PW,
                                                        const unsigned long long* __restrict__ lab,
                                                        const unsigned long long* __restrict__ ext, const uint32_t* __restrict__ cnt,
                                                        unsigned long long* __restrict__ rows) {
  const int b = blockIdx.y, S = 2 * R + 1;
  int id = blockIdx.x;
  const int seg = id % nseg;
  id /= nseg;
  const int dyi = id % S, k = id / S, dy = dyi - R;
  const int t = threadIdx.x;
  const int y0 = row0 + seg * DP_SEG, y1 = y0 + DP_SEG < row1 ? y0 + DP_SEG : row1;
  const int ya = y0 > dy ? y0 : dy, yb = y1 < H + dy ? y1 : H + dy;           // the label rows whose prediction row y - dy is in the frame
  const int s = t < S ? 2 * R - t : 0;              // R - dx: where the lane's 64 bits start behind those of the label word
  const int o = s & 63;
  const size_t plane = ((size_t)b * 2 + k) * H;
  const unsigned long long* __restrict__ L = lab + plane * TW;
  const unsigned long long* __restrict__ E = ext + plane * PW + (s >> 6);     // word w + 1 + (s >> 6) <= PW - 1
  const uint32_t* __restrict__ C = cnt + plane;
  unsigned acc = 0, kept = 0;                       // the lanes from 2 R + 1 on run the loop at dx = R and drop what they count
  for (int y = ya; y < yb; ++y) {
    const unsigned long long* __restrict__ lrow = L + (size_t)y * TW;
    const unsigned long long* __restrict__ erow = E + (size_t)(y - dy) * PW;
    if (t == S) kept += C[y - dy];                  // the kept lane: the predicted pixels of a row that stays inside the band
    for (int w = 0; w < TW; ++w) {
      const unsigned long long lw = lrow[w];        // uniform
      if (lw == 0ull) continue;
      const unsigned long long lo = erow[w], hi = erow[w + 1];
      const unsigned long long moved = (lo >> o) | ((hi << 1) << (63 - o));   // o = 0: the second term is 0
      acc += (unsigned)__popcll(lw & moved);
    }
  }
  acc = t < S ? acc : kept;
  if (t <= S && acc) atomicAdd(rows + (((size_t)b * 2 + k) * S + dyi) * (S + 1) + t, (unsigned long long)acc);
}

__global__ __launch_bounds__(256) void disp_best_kernel(int R, const long long* __restrict__ rows, long long* __restrict__ best) {
  __shared__ unsigned long long red[4];
  const int S = 2 * R + 1, t = threadIdx.x;
  const long long* __restrict__ table = rows + (size_t)blockIdx.x * S * (S + 1);
  unsigned long long key = 0;
  for (int c = t; c < S * S; c += 256) {
    const int dyi = c / S, dxi = c % S;
    const int dy = dyi - R, dx = dxi - R;
    const unsigned long long hits = (unsigned long long)table[dyi * (S + 1) + dxi];
    const unsigned long long cand = hits << 27 | (unsigned long long)(8191 - (dy * dy + dx * dx)) << 14 |
                                    (unsigned long long)(127 - dyi) << 7 | (unsigned long long)(127 - dxi);
    key = cand > key ? cand : key;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(key, off, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) red[t >> 6] = key;
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) key = red[w] > key ? red[w] : key;
    const int dyi = 127 - (int)((key >> 7) & 127u), dxi = 127 - (int)(key & 127u);
    long long* out = best + (size_t)blockIdx.x * 4;
    out[0] = dyi - R, out[1] = dxi - R, out[2] = (long long)(key >> 27), out[3] = table[dyi * (S + 1) + S];
  }
}

__global__ __launch_bounds__(256) void disp_total_kernel(int n_valid, int R, const long long* __restrict__ rows,
                                                         const long long* __restrict__ pixels, long long* __restrict__ total,
                                                         long long* __restrict__ total_pixels, long long* __restrict__ frames) {
  const int t = blockIdx.x * 256 + threadIdx.x, cells = 2 * (2 * R + 1) * (2 * R + 2);
  if (t < cells) total_add64(total, rows, cells, t, n_valid);
  else if (t < cells + 4) total_add64(total_pixels, pixels, 4, t - cells, n_valid);
  else if (t == cells + 4) frames[0] += n_valid;
}

static bool dp_shape_ok(int B, int H, int W, int R) {
  return B >= 1 && B <= DP_BMAX && H >= 1 && W >= 1 && (long)H * W < 2147483648L && R >= 1 && R <= DP_RMAX && 2 * R + 1 <= W;
}
static inline size_t dp_label_words(int W) { return (size_t)(W + DP_BITS - 1) / DP_BITS; }
static inline size_t dp_pred_words(int W, int R) { return (size_t)(W + 2 * R + DP_BITS - 1) / DP_BITS + 1; }

}  // namespace dc

using namespace dc;

extern "C" int dc_displacement_block(int* bits, int* rows) {
  DC_REQUIRE(bits && rows, "dc_displacement_block: null argument");
  *bits = DP_BITS;
  *rows = DP_SEG;
  return 0;
}

extern "C" size_t dc_displacement_workspace(int B, int H, int W, int R) {
  if (!dp_shape_ok(B, H, W, R)) return 0;
  return (size_t)B * 2 * H * ((dp_label_words(W) + dp_pred_words(W, R)) * sizeof(uint64_t) + sizeof(uint32_t));
}

extern "C" int dc_displacement_score(int B, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth, int truth_bytes,
                                     int R, int row0, int row1, int64_t* rows, int64_t* pixels, int64_t* best, int64_t* total,
                                     int64_t* total_pixels, int64_t* frames, void* workspace, void* stream) {
  if (int e = mask_skill_check("dc_displacement_score", B, DP_BMAX, n_valid, H, W, pred, pred_bytes, truth, truth_bytes, row0, row1)) return e;
  DC_REQUIRE(R >= 1 && R <= DP_RMAX, "dc_displacement_score: the radius R must lie in [1, 63]");
  DC_REQUIRE(2 * R + 1 <= W, "dc_displacement_score: the window 2 R + 1 must not be wider than the frame");
  DC_REQUIRE(rows && pixels && best && total && total_pixels && frames && workspace, "dc_displacement_score: null pointer");
  DC_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)rows & 7) == 0 && ((uintptr_t)pixels & 7) == 0 && ((uintptr_t)best & 7) == 0 &&
                 ((uintptr_t)total & 7) == 0 && ((uintptr_t)total_pixels & 7) == 0 && ((uintptr_t)frames & 7) == 0,
             "dc_displacement_score: workspace, rows, pixels, best or a total not aligned to 8 bytes");
  const int S = 2 * R + 1, nseg = (row1 - row0 + DP_SEG - 1) / DP_SEG;
  DC_REQUIRE((long)nseg * S * 2 <= 2147483647L, "dc_displacement_score: too many row segments for one grid");
  if (n_valid == 0) return 0;                       // nothing to read, nothing to write
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(rows, 0, (size_t)n_valid * 2 * S * (S + 1) * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(pixels, 0, (size_t)n_valid * 4 * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(best, 0, (size_t)n_valid * 8 * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const int TW = (int)dp_label_words(W), PW = (int)dp_pred_words(W, R);
  unsigned long long* lab = (unsigned long long*)workspace;                    // [B][2][H][TW]
  unsigned long long* ext = lab + (size_t)B * 2 * H * TW;                      // [B][2][H][PW]
  uint32_t* cnt = (uint32_t*)(ext + (size_t)B * 2 * H * PW);                   // [B][2][H]
  hipLaunchKernelGGL(disp_pack_kernel, dim3(H, n_valid), dim3(DP_PACK), 0, st, H, W, pred, pred_bytes, truth, truth_bytes, R, row0, row1, TW,
                     PW, lab, ext, cnt, (unsigned long long*)pixels);
  DC_LAUNCHED("disp_pack");
  hipLaunchKernelGGL(disp_corr_kernel, dim3((unsigned)nseg * S * 2, n_valid), dim3(S + 1 <= 64 ? 64 : 128), 0, st, H, R, row0, row1, nseg, TW,
                     PW, (const unsigned long long*)lab, (const unsigned long long*)ext, (const uint32_t*)cnt, (unsigned long long*)rows);
  DC_LAUNCHED("disp_corr");
  hipLaunchKernelGGL(disp_best_kernel, dim3(n_valid * 2), dim3(256), 0, st, R, (const long long*)rows, (long long*)best);
  DC_LAUNCHED("disp_best");
  hipLaunchKernelGGL(disp_total_kernel, dim3((2 * S * (S + 1) + 5 + 255) / 256), dim3(256), 0, st, n_valid, R, (const long long*)rows,
                     (const long long*)pixels, (long long*)total, (long long*)total_pixels, (long long*)frames);
  DC_LAUNCHED("disp_total");
  return 0;
}
