// Scale-separation verification: the sums behind the intensity-scale skill score (dc_scale_score; nn.ScaleSkill).  For every frame,
// class, column origin c and level j = 0 .. L, (A, B, C) = (sum (S_F - S_O)^2, sum S_F^2, sum S_O^2) over the disjoint blocks of side
// 2^j that tile a row band from (row0, c) on, S_F and S_O the numbers of predicted and labelled pixels of the class in a block -- columns
// periodic, rows never.  The energies of the 2-D Haar components follow on the host from differences of these block sums.  Integers end
// to end.  include/deepcam_hip.h has the definition; this file has the decomposition: a hierarchical block-sum reduction.
//   scale_sums    A workgroup of four waves takes one SC_TILE x SC_TILE tile of one (frame, origin), aligned to the band's block grid:
//                 rows from row0, columns from the origin, modulo W.  A thread owns a 4 x 4 block: it reads its 16 pixels of both masks
//                 ONCE and forms levels 0, 1 and 2 in registers; (S_F, S_O) of a class ride as the two 16-bit halves of one word (a sum up
//                 to level 6 is at most 4096).  Threads map to blocks in Morton order -- bit 2 i of the thread index is bit i of the
//                 block's column, bit 2 i + 1 of its row -- so the four siblings of a level-3, -4 or -5 block are __shfl_xor partners (1
//                 and 2, 4 and 8, 16 and 32) and a wave is one 32 x 32 block; level 6 goes across the four waves through LDS.  After the
//                 two exchanges of a level every lane of the block holds its sum and squares it: the level's terms then need only the
//                 reduction steps ABOVE the block.  A workgroup's term is at most 4^j * 4096 <= 2^24: 32-bit partials.  Every non-zero
//                 cell leaves as one 64-bit global atomic.  Levels above L are not formed.  T = 2^L divides the band's rows and W, so a
//                 tile at the band's lower edge or the row's end holds WHOLE blocks of every level <= L; the pixels outside are not read
//                 and count nothing.  For L > 6 (where T, a multiple of the tile, leaves no partial tile) the tile's four sums go to the
//                 workspace.  The workgroups of origin 0 also count `pixels`.
//   scale_coarse  only for L > 6: one workgroup per (frame, origin) forms the blocks of 2 x 2 and 4 x 4 tiles from the workspace.  A
//                 256 x 256 block full of a class sums to 2^16 and squares to 2^32: the sums are 32-bit words of their own here, the
//                 squares 64-bit.
//   scale_total   one thread per cell adds the batch's rows, in frame order, to the two-word running totals (lo += x, hi += carry);
//                 four more threads add the pixel counts, one the frame count.
// The origins live in device memory, so a table entry outside [0, T) is found here, not on the host: that origin's workgroups leave, its
// rows stay zero (origin 0's still count the pixels, on the grid of column 0).
#include "common.h"
#include "mask_skill.h"

namespace dc {

static constexpr int SC_TILE = 64;                // a tile: 16 x 16 threads of 4 x 4 pixels; a level-6 block
static constexpr int SC_THREADS = 256;
static constexpr int SC_LMAX = 8;
static constexpr int SC_OMAX = 8;
static constexpr int SC_BMAX = 4095;              // B * O stays a legal grid.y
static constexpr int SC_TLEVELS = 7;              // levels 0 .. 6 are formed inside a tile
static constexpr int SC_TOTAL_THREADS = 512;      // >= 2 * SC_OMAX * (SC_LMAX + 1) * 3 + 5

// bits 0, 2, 4, 6 of t as a 4-bit number: one coordinate of the Morton order
__device__ inline int sc_even_bits(unsigned t) {
  t &= 0x55u;
  t = (t | (t >> 1)) & 0x33u;
  t = (t | (t >> 2)) & 0x0Fu;
  return (int)t;
}

// the three squared terms of one class word S_F | S_O << 16, both halves <= 4096
__device__ inline void sc_square(unsigned w, unsigned* acc) {
  const unsigned f = w & 0xFFFFu, o = w >> 16;
  const int d = (int)f - (int)o;
  acc[0] += (unsigned)(d * d), acc[1] += f * f, acc[2] += o * o;
}

// sums the six terms of a level over the lanes that differ in the bits FROM and above; lane 0 ends up with the wave's sum
template <int FROM>
__device__ inline void sc_reduce(unsigned* acc) {
#pragma unroll
  for (int v = 0; v < 6; ++v) {
#pragma unroll
    for (int o = FROM; o < 64; o <<= 1) acc[v] += __shfl_xor(acc[v], o, 64);
  }
}

__global__ __launch_bounds__(SC_THREADS) void scale_sums_kernel(int H, int W, const void* __restrict__ pred, int pred_bytes,
                                                                const void* __restrict__ truth, int truth_bytes, int L, int O,
                                                                const int32_t* __restrict__ origins, int row0, int row1, int tiles_x,
                                                                int tiles_y, unsigned long long* __restrict__ rows,
                                                                unsigned long long* __restrict__ pixels, uint32_t* __restrict__ tile_sums) {
  __shared__ unsigned red[SC_THREADS / 64][(SC_TLEVELS - 1) * 6];
  __shared__ unsigned top[SC_THREADS / 64][2];
  const int b = blockIdx.y / O, o = blockIdx.y % O;
  int c = origins[o];
  const bool served = c >= 0 && c < (1 << L);
  if (!served) {
    if (o != 0) return;                             // the whole workgroup: this origin's rows stay zero
    c = 0;                                          // origin 0 still counts the pixels
  }
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r0 = row0 + ty * SC_TILE + 4 * sc_even_bits(t >> 1);        // the thread's first row
  const int u0 = tx * SC_TILE + 4 * sc_even_bits(t);                    // ... and first column, counted from the origin
  const size_t frame = (size_t)b * H * W;
  unsigned acc[SC_TLEVELS - 1][6];                  // levels 0 .. 5; per class A, B, C
#pragma unroll
  for (int j = 0; j < SC_TLEVELS - 1; ++j) {
#pragma unroll
    for (int v = 0; v < 6; ++v) acc[j][v] = 0;
  }
  unsigned w1 = 0, w2 = 0;                          // the thread's 4 x 4 block: S_F | S_O << 16 of class 1 and of class 2
#pragma unroll
  for (int q = 0; q < 4; ++q) {                     // its four 2 x 2 blocks
    unsigned q1 = 0, q2 = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = r0 + 2 * (q >> 1) + (e >> 1), u = u0 + 2 * (q & 1) + (e & 1);
      if (r < row1 && u < W) {                      // c < T <= W and u < W: one subtraction wraps the column
        const int col = c + u >= W ? c + u - W : c + u;
        const size_t px = frame + (size_t)r * W + col;
        const unsigned p = mask_bits(pred, px, pred_bytes), y = mask_bits(truth, px, truth_bytes);
        const unsigned f1 = p & 1u, f2 = p >> 16, o1 = y & 1u, o2 = y >> 16;
        acc[0][0] += f1 ^ o1, acc[0][1] += f1, acc[0][2] += o1;
        acc[0][3] += f2 ^ o2, acc[0][4] += f2, acc[0][5] += o2;
        q1 += f1 | (o1 << 16), q2 += f2 | (o2 << 16);
      }
    }
    if (L >= 1) sc_square(q1, acc[1]), sc_square(q2, acc[1] + 3);
    w1 += q1, w2 += q2;
  }
  if (L >= 2) sc_square(w1, acc[2]), sc_square(w2, acc[2] + 3);
  sc_reduce<1>(acc[0]);
  if (L >= 1) sc_reduce<1>(acc[1]);
  if (L >= 2) sc_reduce<1>(acc[2]);
  if (L >= 3) {                                     // 8 x 8: the lanes that differ in bits 0 and 1
    w1 += __shfl_xor(w1, 1, 64), w2 += __shfl_xor(w2, 1, 64);
    w1 += __shfl_xor(w1, 2, 64), w2 += __shfl_xor(w2, 2, 64);
    sc_square(w1, acc[3]), sc_square(w2, acc[3] + 3);                   // the same in all four lanes: reduce over the blocks only
    sc_reduce<4>(acc[3]);
  }
  if (L >= 4) {                                     // 16 x 16
    w1 += __shfl_xor(w1, 4, 64), w2 += __shfl_xor(w2, 4, 64);
    w1 += __shfl_xor(w1, 8, 64), w2 += __shfl_xor(w2, 8, 64);
    sc_square(w1, acc[4]), sc_square(w2, acc[4] + 3);
    sc_reduce<16>(acc[4]);
  }
  if (L >= 5) {                                     // 32 x 32: the wave
    w1 += __shfl_xor(w1, 16, 64), w2 += __shfl_xor(w2, 16, 64);
    w1 += __shfl_xor(w1, 32, 64), w2 += __shfl_xor(w2, 32, 64);
    sc_square(w1, acc[5]), sc_square(w2, acc[5] + 3);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < SC_TLEVELS - 1; ++j) {
#pragma unroll
      for (int v = 0; v < 6; ++v) red[wave][j * 6 + v] = acc[j][v];
    }
    top[wave][0] = w1, top[wave][1] = w2;           // the wave's sums, complete from L = 5 on; read for L >= 6 only
  }
  __syncthreads();
  if (t < SC_TLEVELS * 6) {
    const int j = t / 6, v = t % 6, k = v / 3, term = v % 3;
    unsigned sum = 0;
    if (j < SC_TLEVELS - 1) {
      if (j <= L) sum = red[0][t] + red[1][t] + red[2][t] + red[3][t];
    } else if (L >= 6) {                            // 64 x 64: the tile
      const unsigned w = top[0][k] + top[1][k] + top[2][k] + top[3][k];
      unsigned sq[3] = {0, 0, 0};
      sc_square(w, sq);
      sum = sq[term];
    }
    if (sum && served) atomicAdd(rows + ((((size_t)b * 2 + k) * O + o) * (L + 1) + j) * 3 + term, (unsigned long long)sum);
    if (sum && o == 0 && j == 0 && term) atomicAdd(pixels + (size_t)b * 4 + k * 2 + (term - 1), (unsigned long long)sum);
  }
  if (L > 6 && served && t < 2) {                   // the tile's sums for scale_coarse: (S_F, S_O) of class 1, of class 2
    const unsigned w = top[0][t] + top[1][t] + top[2][t] + top[3][t];
    uint32_t* cell = tile_sums + ((((size_t)b * O + o) * tiles_y + ty) * tiles_x + tx) * 4 + 2 * t;
    cell[0] = w & 0xFFFFu, cell[1] = w >> 16;
  }
}

__global__ __launch_bounds__(SC_THREADS) void scale_coarse_kernel(int L, int O, const int32_t* __restrict__ origins, int tiles_x, int tiles_y,
                                                                  const uint32_t* __restrict__ tile_sums,
                                                                  unsigned long long* __restrict__ rows) {
  __shared__ unsigned long long red[SC_THREADS / 64][12];
  const int b = blockIdx.x / O, o = blockIdx.x % O;
  const int c = origins[o];
  if (c < 0 || c >= (1 << L)) return;               // the whole workgroup: scale_sums wrote no sums for this origin
  const uint32_t* __restrict__ sums = tile_sums + ((size_t)b * O + o) * tiles_y * tiles_x * 4;
  unsigned long long acc[12];                       // level 7: class 1 A, B, C, class 2 A, B, C; level 8 likewise
#pragma unroll
  for (int v = 0; v < 12; ++v) acc[v] = 0;
#pragma unroll
  for (int j = SC_TLEVELS; j <= SC_LMAX; ++j) {
    if (j > L) break;
    const int n = 1 << (j - 6);                     // tiles along a block's side; T divides both extents, so n divides both counts
    const int bx = tiles_x / n, blocks = (tiles_y / n) * bx;
    for (int i = threadIdx.x; i < blocks; i += SC_THREADS) {
      const int y0 = (i / bx) * n, x0 = (i % bx) * n;
      uint32_t s[4] = {0, 0, 0, 0};                 // up to 2^16 each: words of their own
      for (int y = 0; y < n; ++y) {
        for (int x = 0; x < n; ++x) {
          const uint32_t* cell = sums + ((size_t)(y0 + y) * tiles_x + x0 + x) * 4;
          s[0] += cell[0], s[1] += cell[1], s[2] += cell[2], s[3] += cell[3];
        }
      }
      unsigned long long* a = acc + (j - SC_TLEVELS) * 6;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const long long f = s[2 * k], q = s[2 * k + 1], d = f - q;      // squares up to 2^32: 64 bits
        a[3 * k] += (unsigned long long)(d * d), a[3 * k + 1] += (unsigned long long)(f * f), a[3 * k + 2] += (unsigned long long)(q * q);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < 12; ++v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc[v] += __shfl_down(acc[v], s, 64);
    if (lane == 0) red[wave][v] = acc[v];
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    const int j = SC_TLEVELS + threadIdx.x / 6, k = (threadIdx.x % 6) / 3, term = threadIdx.x % 3;
    // this workgroup alone writes the cells of levels 7 and 8 of (b, o), zeroed by the call: a plain store
    if (j <= L) rows[((((size_t)b * 2 + k) * O + o) * (L + 1) + j) * 3 + term] = red[0][threadIdx.x] + red[1][threadIdx.x] +
                                                                                   red[2][threadIdx.x] + red[3][threadIdx.x];
  }
}

__global__ __launch_bounds__(SC_TOTAL_THREADS) void scale_total_kernel(int n_valid, int cells, const unsigned long long* __restrict__ rows,
                                                                       const long long* __restrict__ pixels,
                                                                       unsigned long long* __restrict__ total,
                                                                       long long* __restrict__ total_pixels, long long* __restrict__ frames) {
  const int t = threadIdx.x;                        // cells = 2 * O * (L + 1) * 3 <= 432
  if (t < cells) total_add128(total, rows, cells, t, n_valid);
  else if (t < cells + 4) total_add64(total_pixels, pixels, 4, t - cells, n_valid);
  else if (t == cells + 4) frames[0] += n_valid;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_scale_block(int* cols, int* rows) {
  DC_REQUIRE(cols && rows, "dc_scale_block: null argument");
  *cols = SC_TILE;
  *rows = SC_TILE;
  return 0;
}

extern "C" size_t dc_scale_workspace(int B, int H, int W, int L, int O) {
  if (B < 1 || B > SC_BMAX || H < 1 || W < 1 || (long)H * W >= 2147483648L || L < 1 || L > SC_LMAX || O < 1 || O > SC_OMAX) return 0;
  if (H < (1 << L) || (W & ((1 << L) - 1)) != 0) return 0;                       // no band of T rows fits, or T does not divide W
  return (size_t)B * O * ((H + SC_TILE - 1) / SC_TILE) * ((W + SC_TILE - 1) / SC_TILE) * 4 * sizeof(uint32_t);
}

extern "C" int dc_scale_score(int B, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth, int truth_bytes, int L,
                              int O, const int32_t* origins, int row0, int row1, int64_t* rows, int64_t* pixels, int64_t* total,
                              int64_t* total_pixels, int64_t* frames, void* workspace, void* stream) {
  if (int e = mask_skill_check("dc_scale_score", B, SC_BMAX, n_valid, H, W, pred, pred_bytes, truth, truth_bytes, row0, row1)) return e;
  DC_REQUIRE(L >= 1 && L <= SC_LMAX, "dc_scale_score: the levels L must lie in [1, 8]");
  DC_REQUIRE(O >= 1 && O <= SC_OMAX, "dc_scale_score: the number of origins O must lie in [1, 8]");
  DC_REQUIRE(((row1 - row0) & ((1 << L) - 1)) == 0 && (W & ((1 << L) - 1)) == 0,
             "dc_scale_score: the tile T = 2^L must divide the rows of the band and W");
  DC_REQUIRE(origins && rows && pixels && total && total_pixels && frames && workspace, "dc_scale_score: null pointer");
  DC_REQUIRE(((uintptr_t)origins & 3) == 0 && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)rows & 7) == 0 && ((uintptr_t)pixels & 7) == 0 &&
                 ((uintptr_t)total & 7) == 0 && ((uintptr_t)total_pixels & 7) == 0 && ((uintptr_t)frames & 7) == 0,
             "dc_scale_score: origins, workspace, rows, pixels or a total not aligned to its element size");
  if (n_valid == 0) return 0;                       // nothing to read, nothing to zero, nothing to add
  hipStream_t st = (hipStream_t)stream;
  const int cells = 2 * O * (L + 1) * 3;
  hipError_t e = hipMemsetAsync(rows, 0, (size_t)n_valid * cells * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(pixels, 0, (size_t)n_valid * 4 * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const int tiles_x = (W + SC_TILE - 1) / SC_TILE, tiles_y = (row1 - row0 + SC_TILE - 1) / SC_TILE;
  hipLaunchKernelGGL(scale_sums_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y, n_valid * O), dim3(SC_THREADS), 0, st, H, W, pred,
                     pred_bytes, truth, truth_bytes, L, O, origins, row0, row1, tiles_x, tiles_y, (unsigned long long*)rows,
                     (unsigned long long*)pixels, (uint32_t*)workspace);
  DC_LAUNCHED("scale_sums");
  if (L >= SC_TLEVELS) {
    hipLaunchKernelGGL(scale_coarse_kernel, dim3(n_valid * O), dim3(SC_THREADS), 0, st, L, O, origins, tiles_x, tiles_y,
                       (const uint32_t*)workspace, (unsigned long long*)rows);
    DC_LAUNCHED("scale_coarse");
  }
  hipLaunchKernelGGL(scale_total_kernel, dim3(1), dim3(SC_TOTAL_THREADS), 0, st, n_valid, cells, (const unsigned long long*)rows,
                     (const long long*)pixels, (unsigned long long*)total, (long long*)total_pixels, (long long*)frames);
  DC_LAUNCHED("scale_total");
  return 0;
}
