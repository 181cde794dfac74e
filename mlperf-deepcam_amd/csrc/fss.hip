// Neighbourhood verification: the sums behind the Fractions Skill Score (dc_fss_score; nn.FractionsSkill).  For every frame, class and
// window of n x n grid pixels, (A, B, C) = (sum (F - O)^2, sum F^2, sum O^2) over the pixels of a row band, F and O the numbers of
// predicted and labelled pixels of the class inside the window around the pixel -- periodic in longitude, zero beyond the poles.  Integers
// end to end.  include/deepcam_hip.h has the definition; this file has the decomposition: a separable box sum through a slab of packed words.
//   fss_rows   the horizontal pass.  A workgroup takes a strip of FS_TC columns of FS_FR rows of one frame.  Per row it reads the strip of
//              both masks ONCE with a halo of R columns on either side (R the largest radius of the call's windows; the halo's columns taken
//              modulo W, or as zeros without wrap), turns every pixel into four indicator bits in two words of 2 x 16-bit lanes (pred 1 |
//              pred 2, truth 1 | truth 2), and builds the inclusive prefix sums of the <= FS_TC + 254 elements in LDS: two elements per
//              thread, a wave scan by lane shifts, the four wave totals through LDS.  Because the prefix is LOCAL to strip plus halo there
//              is no wrap term and no bound on W from the 16-bit lanes.  Per window a thread then forms E[x + r + 1] - E[x - r] for its
//              column: lane-wise differences of monotone sums never borrow, each of the four is <= 255, and they leave as ONE packed word
//              (F1 | F2 << 8 | O1 << 16 | O2 << 24) into the slab -- consecutive lanes, consecutive words.  The strip's own indicator counts
//              of the rows inside the band go to `pixels`, one 64-bit atomic per wave and counter.
//   fss_cols   the vertical pass and the reduction.  A thread owns one column of a segment of FS_TR rows of the band, for one frame and
//              window: it sums the words of the 2 r + 1 rows around the segment's first row, then slides down, adding the word that enters
//              and subtracting the one that leaves.  The four running sums (<= 255 * 255) sit in two registers of 2 x 16-bit lanes; a lane
//              never borrows, because what leaves was added before.  Per pixel the three squared terms of both classes go into 64-bit
//              registers; a wave reduction and LDS bring them to six 64-bit integer atomics per workgroup into `rows`.
//   fss_total  one thread per (class, window, term) adds the batch's rows, in frame order, to the two-word running totals (lo += x,
//              hi += carry); four more threads add the pixel counts, one the frame count.
// The workspace holds one slab of B * H * W words per window: one horizontal pass reads the masks once and writes every window, one
// vertical pass takes all of them (grid.y = frame x window), three launches per call.  Measured against a loop over the windows on ONE
// reused slab (15 launches at 7 windows, each of them too small a grid to fill the chip): 0.23 ms against 0.64 ms per batch of 8 at
// 768 x 1152 (profiles/fss.txt).
#include "common.h"
#include "mask_skill.h"

namespace dc {

static constexpr int FS_TC = 256;                 // columns of a strip = threads of a workgroup
static constexpr int FS_TR = 64;                  // rows of a segment of the vertical pass
static constexpr int FS_FR = 4;                   // rows a workgroup of the horizontal pass walks
static constexpr int FS_RMAX = 127;               // n = 2 r + 1 <= 255: a row's count fits a byte, a window's 16 bits
static constexpr int FS_SMAX = 16;
static constexpr int FS_BMAX = 4095;              // B * S stays a legal grid.y
static constexpr unsigned FS_LANES = 0x00FF00FFu;

// the radius of window s, or -1 where the table (device memory: the host never saw it) holds one the call cannot serve
__device__ inline int fs_radius(const int32_t* __restrict__ radius, int s, int W, int wrap) {
  const int r = radius[s];
  return (r >= 0 && r <= FS_RMAX && (!wrap || 2 * r + 1 <= W)) ? r : -1;
}

__global__ __launch_bounds__(FS_TC) void fss_rows_kernel(int B, int H, int W, const void* __restrict__ pred, int pred_bytes,
                                                         const void* __restrict__ truth, int truth_bytes, int S,
                                                         const int32_t* __restrict__ radius, int wrap, int row0, int row1, int rlo, int rhi,
                                                         int strips, uint32_t* __restrict__ slab, unsigned long long* __restrict__ pixels) {
  __shared__ uint32_t ep[2 * FS_TC + 2], eq[2 * FS_TC + 2];     // E[0] = 0, E[e + 1] = the inclusive prefix at element e
  __shared__ uint32_t wp[FS_TC / 64], wq[FS_TC / 64];
  const int b = blockIdx.y;
  const int strip = blockIdx.x % strips, grp = blockIdx.x / strips;
  const int c0 = strip * FS_TC;
  const int tcw = W - c0 < FS_TC ? W - c0 : FS_TC;
  int R = 0;
  for (int s = 0; s < S; ++s) {
    const int r = fs_radius(radius, s, W, wrap);
    R = r > R ? r : R;
  }
  const int N = tcw + 2 * R;                        // elements of a row: halo, strip, halo; <= FS_TC + 2 * FS_RMAX
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t frame = (size_t)b * H * W;
  unsigned cp = 0, cq = 0;                          // the strip's own indicator counts inside the band: at most 2 * FS_FR per lane
  const int ifirst = rlo + grp * FS_FR;
  const int ilast = ifirst + FS_FR < rhi ? ifirst + FS_FR : rhi;
  for (int i = ifirst; i < ilast; ++i) {
    unsigned vp[2], vq[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = 2 * t + j;
      vp[j] = vq[j] = 0;
      if (e < N) {
        int c = c0 - R + e;                         // in (-W, 2 W) under wrap, where 2 R + 1 <= W
        if (wrap) c = c < 0 ? c + W : (c >= W ? c - W : c);
        if (c >= 0 && c < W) {
          const size_t px = frame + (size_t)i * W + c;
          vp[j] = mask_bits(pred, px, pred_bytes);
          vq[j] = mask_bits(truth, px, truth_bytes);
        }
        if (i >= row0 && i < row1 && e >= R && e < R + tcw) cp += vp[j], cq += vq[j];
      }
    }
    const unsigned sp = vp[0] + vp[1], sq = vq[0] + vq[1];
    unsigned ip = sp, iq = sq;                      // the wave's inclusive scan: every lane of 16 bits stays below N <= 510
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(ip, o, 64), uq = __shfl_up(iq, o, 64);
      if (lane >= o) ip += up, iq += uq;
    }
    if (lane == 63) wp[wave] = ip, wq[wave] = iq;
    __syncthreads();                                // the wave totals are there; the previous row's reads of E are over
    unsigned xp = ip - sp, xq = iq - sq;            // exclusive, over the workgroup
    for (int w = 0; w < wave; ++w) xp += wp[w], xq += wq[w];
    if (t == 0) ep[0] = 0, eq[0] = 0;
    ep[2 * t + 1] = xp + vp[0], ep[2 * t + 2] = xp + sp;
    eq[2 * t + 1] = xq + vq[0], eq[2 * t + 2] = xq + sq;
    __syncthreads();
    if (t < tcw) {
      for (int s = 0; s < S; ++s) {
        const int r = fs_radius(radius, s, W, wrap);
        if (r < 0) continue;                        // the window is not served: fss_cols skips it too, its rows stay zero
        const int x = R + t;                        // the element of this thread's column; x - r >= 0, x + r + 1 <= N
        const unsigned dp = ep[x + r + 1] - ep[x - r], dq = eq[x + r + 1] - eq[x - r];
        const uint32_t word = (dp & 0xFFu) | ((dp >> 16) << 8) | ((dq & 0xFFu) << 16) | ((dq >> 16) << 24);
        slab[(((size_t)s * B + b) * H + i) * W + c0 + t] = word;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cp += __shfl_down(cp, o, 64), cq += __shfl_down(cq, o, 64);   // <= 64 * 2 * FS_FR per lane of 16 bits
  if (lane == 0) {
    unsigned long long* px = pixels + (size_t)b * 4;             // [class][side]
    if (cp & 0xFFFFu) atomicAdd(px + 0, (unsigned long long)(cp & 0xFFFFu));
    if (cq & 0xFFFFu) atomicAdd(px + 1, (unsigned long long)(cq & 0xFFFFu));
    if (cp >> 16) atomicAdd(px + 2, (unsigned long long)(cp >> 16));
    if (cq >> 16) atomicAdd(px + 3, (unsigned long long)(cq >> 16));
  }
}

__global__ __launch_bounds__(FS_TC) void fss_cols_kernel(int B, int H, int W, int S, const int32_t* __restrict__ radius,
                                                         int wrap, int row0, int row1, int strips, const uint32_t* __restrict__ slab,
                                                         unsigned long long* __restrict__ rows) {
  __shared__ unsigned long long red[FS_TC / 64][6];
  const int b = blockIdx.y / S, s = blockIdx.y % S;
  const int r = fs_radius(radius, s, W, wrap);
  if (r < 0) return;                                // the whole workgroup: nothing was written for this window
  const int strip = blockIdx.x % strips, seg = blockIdx.x / strips;
  const int c = strip * FS_TC + threadIdx.x;
  const int i0 = row0 + seg * FS_TR;
  const int i1 = i0 + FS_TR < row1 ? i0 + FS_TR : row1;
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};   // class 1: A, B, C; class 2: A, B, C
  if (c < W) {
    const uint32_t* __restrict__ col = slab + ((size_t)s * B + b) * H * W + c;
    unsigned a1 = 0, a2 = 0;                        // (F1 | O1 << 16), (F2 | O2 << 16): every lane <= 255 * 255
    const int lo = i0 - r > 0 ? i0 - r : 0, hi = i0 + r < H - 1 ? i0 + r : H - 1;
#pragma unroll 4
    for (int i = lo; i <= hi; ++i) {
      const uint32_t w = col[(size_t)i * W];
      a1 += w & FS_LANES, a2 += (w >> 8) & FS_LANES;
    }
#pragma unroll 2
    for (int i = i0; i < i1; ++i) {
      const unsigned long long f1 = a1 & 0xFFFFu, o1 = a1 >> 16, f2 = a2 & 0xFFFFu, o2 = a2 >> 16;
      const long long d1 = (long long)f1 - (long long)o1, d2 = (long long)f2 - (long long)o2;
      acc[0] += (unsigned long long)(d1 * d1), acc[1] += f1 * f1, acc[2] += o1 * o1;
      acc[3] += (unsigned long long)(d2 * d2), acc[4] += f2 * f2, acc[5] += o2 * o2;
      if (i + 1 < i1) {                             // slide to row i + 1: row i + 1 + r enters, row i - r leaves
        const int in = i + 1 + r, out = i - r;
        const uint32_t wi = in < H ? col[(size_t)in * W] : 0u;
        const uint32_t wo = out >= 0 ? col[(size_t)out * W] : 0u;
        a1 += wi & FS_LANES, a2 += (wi >> 8) & FS_LANES;
        a1 -= wo & FS_LANES, a2 -= (wo >> 8) & FS_LANES;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < 6; ++v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[v] += __shfl_down(acc[v], o, 64);
    if (lane == 0) red[wave][v] = acc[v];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < FS_TC / 64; ++w) sum += red[w][threadIdx.x];
    const int k = threadIdx.x / 3, term = threadIdx.x % 3;
    if (sum) atomicAdd(rows + (((size_t)b * 2 + k) * S + s) * 3 + term, sum);
  }
}

__global__ __launch_bounds__(128) void fss_total_kernel(int n_valid, int S, const unsigned long long* __restrict__ rows,
                                                        const long long* __restrict__ pixels, unsigned long long* __restrict__ total,
                                                        long long* __restrict__ total_pixels, long long* __restrict__ frames) {
  const int t = threadIdx.x, words = 2 * S * 3;     // <= 96
  if (t < words) total_add128(total, rows, words, t, n_valid);
  else if (t < words + 4) total_add64(total_pixels, pixels, 4, t - words, n_valid);
  else if (t == words + 4) frames[0] += n_valid;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_fss_block(int* cols, int* rows) {
  DC_REQUIRE(cols && rows, "dc_fss_block: null argument");
  *cols = FS_TC;
  *rows = FS_TR;
  return 0;
}

extern "C" size_t dc_fss_workspace(int B, int H, int W, int S) {
  if (B < 1 || B > FS_BMAX || H < 1 || W < 1 || (long)H * W >= 2147483648L || S < 1 || S > FS_SMAX) return 0;
  return (size_t)B * S * H * W * sizeof(uint32_t);
}

extern "C" int dc_fss_score(int B, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth, int truth_bytes, int S,
                            const int32_t* radius, int wrap, int row0, int row1, int64_t* rows, int64_t* pixels, int64_t* total,
                            int64_t* total_pixels, int64_t* frames, void* workspace, void* stream) {
  if (int e = mask_skill_check("dc_fss_score", B, FS_BMAX, n_valid, H, W, pred, pred_bytes, truth, truth_bytes, row0, row1)) return e;
  DC_REQUIRE(S >= 1 && S <= FS_SMAX, "dc_fss_score: S must lie in [1, 16]");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_fss_score: wrap must be 0 or 1");
  DC_REQUIRE(radius && rows && pixels && total && total_pixels && frames && workspace, "dc_fss_score: null pointer");
  DC_REQUIRE(((uintptr_t)radius & 3) == 0 && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)rows & 7) == 0 && ((uintptr_t)pixels & 7) == 0 &&
                 ((uintptr_t)total & 7) == 0 && ((uintptr_t)total_pixels & 7) == 0 && ((uintptr_t)frames & 7) == 0,
             "dc_fss_score: radius, workspace, rows, pixels or a total not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(rows, 0, (size_t)B * 2 * S * 3 * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(pixels, 0, (size_t)B * 4 * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  if (n_valid == 0) return 0;                       // nothing to read, nothing to add
  const int strips = (W + FS_TC - 1) / FS_TC;
  // the rows the vertical pass can reach from the band with the widest window
  const int rlo = row0 - FS_RMAX > 0 ? row0 - FS_RMAX : 0, rhi = (long)row1 + FS_RMAX < H ? row1 + FS_RMAX : H;
  const unsigned gx_rows = (unsigned)strips * (unsigned)((rhi - rlo + FS_FR - 1) / FS_FR);
  const unsigned gx_cols = (unsigned)strips * (unsigned)((row1 - row0 + FS_TR - 1) / FS_TR);
  hipLaunchKernelGGL(fss_rows_kernel, dim3(gx_rows, n_valid), dim3(FS_TC), 0, st, B, H, W, pred, pred_bytes, truth, truth_bytes, S, radius,
                     wrap, row0, row1, rlo, rhi, strips, (uint32_t*)workspace, (unsigned long long*)pixels);
  DC_LAUNCHED("fss_rows");
  hipLaunchKernelGGL(fss_cols_kernel, dim3(gx_cols, n_valid * S), dim3(FS_TC), 0, st, B, H, W, S, radius, wrap, row0, row1, strips,
                     (const uint32_t*)workspace, (unsigned long long*)rows);
  DC_LAUNCHED("fss_cols");
  hipLaunchKernelGGL(fss_total_kernel, dim3(1), dim3(128), 0, st, n_valid, S, (const unsigned long long*)rows, (const long long*)pixels,
                     (unsigned long long*)total, (long long*)total_pixels, (long long*)frames);
  DC_LAUNCHED("fss_total");
  return 0;
}
