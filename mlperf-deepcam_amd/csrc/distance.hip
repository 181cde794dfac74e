// Distance-map verification: capped squared Euclidean distance maps of two masks and the integers behind the distance measures for binary
// fields (dc_distance_score; nn.DistanceSkill).  For every pixel, side (prediction, labels) and class (1, 2) the map holds d^2 to the nearest
// pixel of that side and class -- columns periodic with wrap, rows never -- where that is <= R^2, and R^2 + 1 ("beyond") otherwise.  From the
// four maps: per frame, class and direction the number of source pixels per ring, the sums of the quantised distance and of d^2, and
// Baddeley's sum of squared differences.  Integers end to end.  include/deepcam_hip.h has the definitions; this file has the decomposition.
// The transform is separable, and the cap makes a window of +-R rows and columns exact:
//   dist_vert   the vertical pass.  A thread owns one column of a segment of DT_TR rows of one frame.  It walks down from R rows above the
//               segment, carrying per indicator field (pred 1, pred 2, truth 1, truth 2) the rows since the field's last pixel, saturated
//               at R + 1 ("none within R"), and stores the four as ONE packed word of bytes per pixel of the segment; then it walks up from
//               R rows below the segment, takes the minimum with the word it stored on the way down (its own store: no other thread touches
//               the column of the segment) and stores the word again.  A whole-column scan would offer B * W threads only; with the halo a
//               frame gives W * H / DT_TR threads, at the price of reading 2 (DT_TR + R) mask rows per DT_TR rows of output.
//   dist_horz   the horizontal pass and the scores.  A workgroup takes a strip of DT_TC columns of DT_HR rows.  Per row it stages the packed
//               words of the strip with a halo of R columns on either side in LDS (columns modulo W with wrap; R + 1 in every byte for a
//               column outside the frame without).  A thread then walks dx = 0, 1, ... for its column: ONE word to the left and one to the
//               right serve all four fields, candidate dx^2 + g^2 per byte, and the walk ends once dx^2 reaches the largest of the four
//               running minima.  A byte of R + 1 gives a candidate above R^2 and so never wins against the initial R^2 + 1: no test of
//               "beyond" in the loop.  With the four d^2 in registers the pixel is scored in place: ring 0 and the beyond ring -- the two
//               that hold nearly every source -- are counted by wave ballots, the other rings by LDS atomics on a workgroup-private
//               histogram of 32-bit cells; the sums and the Baddeley term go through a wave reduction.  Per workgroup one 64-bit global
//               atomic per non-zero cell.  Integer sums: the order does not matter.  The uint16 maps are stored only when asked for.
//   dist_total  one thread per cell adds the batch's frame rows to the totals, frame by frame; two more add the Baddeley sums to their
//               two-word totals (lo += x, hi += carry), one the frame count.
// The workspace holds the packed words, B * H * W * 4 bytes.  Three launches per call.
#include "common.h"
#include "mask_skill.h"

namespace dc {

static constexpr int DT_TC = 256;                 // columns of a strip = threads of a workgroup
static constexpr int DT_TR = 64;                  // rows of a segment of the vertical pass
static constexpr int DT_HR = 8;                   // rows a workgroup of the horizontal pass walks
static constexpr int DT_RMAX = 127;               // R + 1 fits a byte, R^2 + 1 sixteen bits
static constexpr int DT_BMAX = 4095;              // a legal grid.y
static constexpr int DT_SUMS = 10;                // per workgroup: (sum dq, sum d^2) per class and direction, the Baddeley term per class

// one step of the four running row distances: 0 where the field has a pixel in this row, else one more, saturated at far = R + 1
__device__ inline void dt_step(unsigned g[4], unsigned bits, unsigned far) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const unsigned next = g[f] + 1 < far ? g[f] + 1 : far;
    g[f] = ((bits >> f) & 1u) ? 0u : next;
  }
}

__global__ __launch_bounds__(DT_TC) void dist_vert_kernel(int H, int W, const void* __restrict__ pred, int pred_bytes,
                                                          const void* __restrict__ truth, int truth_bytes, int R, int rlo, int rhi,
                                                          int strips, uint32_t* ws) {
  const int b = blockIdx.y;
  const int strip = blockIdx.x % strips, seg = blockIdx.x / strips;
  const int c = strip * DT_TC + threadIdx.x;
  if (c >= W) return;                               // no barrier in this kernel
  const int i0 = rlo + seg * DT_TR;
  const int i1 = i0 + DT_TR < rhi ? i0 + DT_TR : rhi;
  const unsigned far = (unsigned)R + 1u;
  const size_t frame = (size_t)b * H * W;
  unsigned g[4] = {far, far, far, far};
  for (int i = i0 - R > 0 ? i0 - R : 0; i < i1; ++i) {           // down: rows since the last pixel at or above
    const size_t px = frame + (size_t)i * W + c;
    dt_step(g, mask_class(pred, px, pred_bytes) | mask_class(truth, px, truth_bytes) << 2, far);
    if (i >= i0) ws[px] = g[0] | g[1] << 8 | g[2] << 16 | g[3] << 24;
  }
  g[0] = g[1] = g[2] = g[3] = far;
  for (int i = (i1 + R < H ? i1 + R : H) - 1; i >= i0; --i) {    // up: rows to the next pixel at or below; the minimum of both
    const size_t px = frame + (size_t)i * W + c;
    dt_step(g, mask_class(pred, px, pred_bytes) | mask_class(truth, px, truth_bytes) << 2, far);
    if (i < i1) {
      const uint32_t w = ws[px];
      uint32_t out = 0;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const unsigned down = (w >> (8 * f)) & 0xFFu;
        out |= (down < g[f] ? down : g[f]) << (8 * f);
      }
      ws[px] = out;
    }
  }
}

// ring and quantised distance of a map value from the caller's table (ring | dq << 8); a ring the table should not hold is clamped, so
// that a wrong table (device memory: the host never saw it) gives wrong counts, never an access outside the histogram
__device__ inline void dt_lookup(const int32_t* __restrict__ table, unsigned v, int R, unsigned& ring, unsigned& dq) {
  const unsigned e = (unsigned)table[v];
  ring = e & 0xFFu;
  ring = ring < (unsigned)R + 1u ? ring : (unsigned)R + 1u;
  dq = (e >> 8) & 0xFFFFu;
}

__global__ __launch_bounds__(DT_TC) void dist_horz_kernel(int H, int W, int R, const int32_t* __restrict__ table, int wrap, int row0,
                                                          int row1, int rlo, int rhi, int strips, const uint32_t* __restrict__ ws,
                                                          unsigned long long* __restrict__ rows, unsigned long long* __restrict__ baddeley,
                                                          uint16_t* __restrict__ maps) {
  __shared__ uint32_t gw[DT_TC + 2 * DT_RMAX + 2];
  __shared__ uint32_t hist[4 * (DT_RMAX + 2)];      // [class][direction][ring 0 .. R + 1]
  __shared__ unsigned long long red[DT_TC / 64][DT_SUMS];
  const int b = blockIdx.y;
  const int strip = blockIdx.x % strips, grp = blockIdx.x / strips;
  const int c0 = strip * DT_TC;
  const int tcw = W - c0 < DT_TC ? W - c0 : DT_TC;
  const int N = tcw + 2 * R;                        // elements of a row: halo, strip, halo; <= DT_TC + 2 * DT_RMAX
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rings = R + 2;
  const unsigned cap = (unsigned)(R * R) + 1u;      // "beyond"
  const unsigned far = (unsigned)R + 1u;
  const uint32_t absent = far | far << 8 | far << 16 | far << 24;
  const size_t frame = (size_t)b * H * W;
  for (int k = t; k < 4 * rings; k += DT_TC) hist[k] = 0;
  unsigned sums[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // [class][direction][dq, d^2]: <= DT_HR * 32512 per thread
  unsigned long long bad[2] = {0, 0};
  unsigned near[4] = {0, 0, 0, 0}, beyond[4] = {0, 0, 0, 0};    // ring 0 and ring R + 1 of the wave, [class][direction]
  const int ifirst = rlo + grp * DT_HR;
  const int ilast = ifirst + DT_HR < rhi ? ifirst + DT_HR : rhi;
  for (int i = ifirst; i < ilast; ++i) {
    __syncthreads();                                // the previous row's reads are over (and, in front of the first row, hist is zero)
    for (int e = t; e < N; e += DT_TC) {
      int c = c0 - R + e;                           // in (-W, 2 W) under wrap, where 2 R + 1 <= W
      if (wrap) c = c < 0 ? c + W : (c >= W ? c - W : c);
      gw[e] = (c >= 0 && c < W) ? ws[frame + (size_t)i * W + c] : absent;
    }
    __syncthreads();
    unsigned best[4] = {cap, cap, cap, cap};
    const bool mine = t < tcw;
    if (mine) {
      const int x = R + t;                          // x - dx >= 0, x + dx < N
      unsigned reach = cap;                         // the largest of the four minima
      for (int dx = 0; dx <= R; ++dx) {
        const unsigned dx2 = (unsigned)(dx * dx);
        if (dx2 >= reach) break;                    // no column this far or farther can lower any of the four
        const uint32_t wl = gw[x - dx], wr = gw[x + dx];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const unsigned gl = (wl >> (8 * f)) & 0xFFu, gr = (wr >> (8 * f)) & 0xFFu;
          const unsigned gm = gl < gr ? gl : gr;
          const unsigned cand = dx2 + gm * gm;      // a byte of R + 1 gives more than R^2: it never wins against cap
          best[f] = cand < best[f] ? cand : best[f];
        }
        const unsigned m01 = best[0] > best[1] ? best[0] : best[1], m23 = best[2] > best[3] ? best[2] : best[3];
        reach = m01 > m23 ? m01 : m23;
      }
      if (maps) {
#pragma unroll
        for (int f = 0; f < 4; ++f) maps[((size_t)b * 4 + f) * H * W + (size_t)i * W + c0 + t] = (uint16_t)best[f];
      }
    }
    if (i < row0 || i >= row1) continue;            // the same for the whole workgroup: the row is mapped, not scored
    const bool scored = mine;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned dP = best[k], dT = best[2 + k];
      unsigned ringP, dqP, ringT, dqT;
      dt_lookup(table, dP, R, ringP, dqP);
      dt_lookup(table, dT, R, ringT, dqT);
      if (scored) {
        const long long wP = dP >= cap ? 256 * R : (int)dqP, wT = dT >= cap ? 256 * R : (int)dqT;
        bad[k] += (unsigned long long)((wP - wT) * (wP - wT));
      }
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {           // 0 miss: from the labelled pixels to the prediction; 1 false alarm: the reverse
        const bool source = scored && (dir == 0 ? dT : dP) == 0;
        const unsigned d2 = dir == 0 ? dP : dT, ring = dir == 0 ? ringP : ringT, dq = dir == 0 ? dqP : dqT;
        const int cell = k * 2 + dir;
        near[cell] += (unsigned)__popcll(__ballot(source && ring == 0));
        beyond[cell] += (unsigned)__popcll(__ballot(source && ring == far));
        if (source && ring != 0 && ring != far) atomicAdd(&hist[cell * rings + ring], 1u);
        if (source && d2 < cap) sums[cell * 2] += dq, sums[cell * 2 + 1] += d2;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int cell = 0; cell < 4; ++cell) {
      if (near[cell]) atomicAdd(&hist[cell * rings], near[cell]);
      if (beyond[cell]) atomicAdd(&hist[cell * rings + R + 1], beyond[cell]);
    }
  }
#pragma unroll
  for (int v = 0; v < DT_SUMS; ++v) {
    unsigned long long a = v < 8 ? (unsigned long long)sums[v] : bad[v - 8];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
    if (lane == 0) red[wave][v] = a;
  }
  __syncthreads();
  unsigned long long* frame_rows = rows + (size_t)b * 4 * (R + 4);
  if (t < DT_SUMS) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < DT_TC / 64; ++w) sum += red[w][t];
    if (sum) {
      if (t < 8) atomicAdd(frame_rows + (t >> 1) * (R + 4) + R + 2 + (t & 1), sum);
      else atomicAdd(baddeley + (size_t)b * 2 + (t - 8), sum);
    }
  }
  for (int k = t; k < 4 * rings; k += DT_TC) {
    const unsigned n = hist[k];
    if (n) atomicAdd(frame_rows + (k / rings) * (R + 4) + k % rings, (unsigned long long)n);
  }
}

__global__ __launch_bounds__(256) void dist_total_kernel(int n_valid, int R, const long long* __restrict__ rows,
                                                         const unsigned long long* __restrict__ baddeley, long long* __restrict__ total,
                                                         unsigned long long* __restrict__ total_baddeley, long long* __restrict__ frames) {
  const int t = blockIdx.x * 256 + threadIdx.x, cells = 4 * (R + 4);
  if (t < cells) total_add64(total, rows, cells, t, n_valid);
  else if (t < cells + 2) total_add128(total_baddeley, baddeley, 2, t - cells, n_valid);
  else if (t == cells + 2) frames[0] += n_valid;
}

static bool dt_shape_ok(int B, int H, int W, int R) {
  return B >= 1 && B <= DT_BMAX && H >= 1 && W >= 1 && (long)H * W < 2147483648L && R >= 1 && R <= DT_RMAX;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_distance_block(int* cols, int* rows) {
  DC_REQUIRE(cols && rows, "dc_distance_block: null argument");
  *cols = DT_TC;
  *rows = DT_TR;
  return 0;
}

extern "C" size_t dc_distance_workspace(int B, int H, int W, int R) {
  if (!dt_shape_ok(B, H, W, R)) return 0;
  return (size_t)B * H * W * sizeof(uint32_t);
}

extern "C" int dc_distance_score(int B, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth, int truth_bytes,
                                 int R, const int32_t* table, int wrap, int row0, int row1, int64_t* rows, int64_t* baddeley,
                                 int64_t* total, int64_t* total_baddeley, int64_t* frames, uint16_t* maps, void* workspace, void* stream) {
  if (int e = mask_skill_check("dc_distance_score", B, DT_BMAX, n_valid, H, W, pred, pred_bytes, truth, truth_bytes, row0, row1)) return e;
  DC_REQUIRE(R >= 1 && R <= DT_RMAX, "dc_distance_score: the radius R must lie in [1, 127]");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_distance_score: wrap must be 0 or 1");
  DC_REQUIRE(!wrap || 2 * R + 1 <= W, "dc_distance_score: with wrap the window 2 R + 1 must not be wider than the frame");
  DC_REQUIRE(table && rows && baddeley && total && total_baddeley && frames && workspace,
             "dc_distance_score: null pointer");
  DC_REQUIRE(((uintptr_t)table & 3) == 0 && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)maps & 1) == 0 && ((uintptr_t)rows & 7) == 0 &&
                 ((uintptr_t)baddeley & 7) == 0 && ((uintptr_t)total & 7) == 0 && ((uintptr_t)total_baddeley & 7) == 0 &&
                 ((uintptr_t)frames & 7) == 0,
             "dc_distance_score: table, workspace, maps, rows, baddeley or a total not aligned to its element size");
  if (n_valid == 0) return 0;                       // nothing to read, nothing to write
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(rows, 0, (size_t)n_valid * 4 * (R + 4) * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(baddeley, 0, (size_t)n_valid * 2 * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const int strips = (W + DT_TC - 1) / DT_TC;
  const int rlo = maps ? 0 : row0, rhi = maps ? H : row1;        // the maps cover every row, the scores the band alone
  const unsigned gx_vert = (unsigned)strips * (unsigned)((rhi - rlo + DT_TR - 1) / DT_TR);
  const unsigned gx_horz = (unsigned)strips * (unsigned)((rhi - rlo + DT_HR - 1) / DT_HR);
  hipLaunchKernelGGL(dist_vert_kernel, dim3(gx_vert, n_valid), dim3(DT_TC), 0, st, H, W, pred, pred_bytes, truth, truth_bytes, R, rlo, rhi,
                     strips, (uint32_t*)workspace);
  DC_LAUNCHED("dist_vert");
  hipLaunchKernelGGL(dist_horz_kernel, dim3(gx_horz, n_valid), dim3(DT_TC), 0, st, H, W, R, table, wrap, row0, row1, rlo, rhi, strips,
                     (const uint32_t*)workspace, (unsigned long long*)rows, (unsigned long long*)baddeley, maps);
  DC_LAUNCHED("dist_horz");
  hipLaunchKernelGGL(dist_total_kernel, dim3((4 * (R + 4) + 3 + 255) / 256), dim3(256), 0, st, n_valid, R, (const long long*)rows,
                     (const unsigned long long*)baddeley, (long long*)total, (unsigned long long*)total_baddeley, (long long*)frames);
  DC_LAUNCHED("dist_total");
  return 0;
}
