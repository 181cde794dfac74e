// Skeletons and axis lengths of events (dc_mask_thin, dc_thin_lds_bytes, dc_skeleton_stats; nn.EventAxis).  include/deepcam_hip.h has the
// definitions -- Guo and Hall's two-subiteration thinning, the link rule, the row of seven words; this file has the decomposition.
//
//   th_thin    ONE workgroup per (class, valid sample) thins the whole class plane of its frame inside the LDS and never leaves its CU.
//              The plane is a bit plane, H rows of TW = ceil(W / 64) words of 64 pixels (bit b of word w is column 64 w + b; the bits from
//              W on in a row's last word are zero and stay zero): 768 x 1152 is 13 824 words, 110 592 bytes of the CU's 160 KiB.
//              pack     a wave takes 64 consecutive columns of a row; __ballot of the class test is the word (as disp_pack does).
//              sub-pass thread t owns the words t, t + 1024, t + 2048, ... (consecutive lanes read consecutive words: no bank conflict).
//                       For an owned word that is not zero it reads the eight words around it (the rows above and below, the words left
//                       and right; the row's other end at the seam), forms the eight neighbour planes P2 .. P9 with funnel shifts and
//                       evaluates the rule for 64 pixels at once, bit-sliced: C == 1 as "exactly one of four", N1 and N2 as 3-bit sums
//                       from one full and one half adder each, 2 <= min(N1, N2) <= 3 as "both at least 2 and not both 4".  About 60
//                       64-bit operations decide 64 pixels.  A zero word deletes nothing and costs one LDS read; frames are about 97 %
//                       background.
//              hazard   a sub-pass judges every pixel against the plane as it stood when the sub-pass began.  A thread keeps the delete
//                       words of ITS words in registers (del[]): every LDS read of the sub-pass lies before the first barrier, every
//                       `plane &= ~del` behind it, and each word is written by its owner alone.  The second barrier ends the sub-pass and
//                       carries "anything deleted": a wave that deleted sets flag[s] (s = 0 for A, 1 for B) before it, everybody reads it
//                       behind it.  flag[1 - s] is cleared between the two barriers of sub-pass s: its last readers passed it before
//                       they reached this sub-pass's first barrier, its next writers come after this sub-pass's second.
//              expand   a wave per word again, 64 consecutive bytes per store.  Both workgroups of a frame write the same byte plane, so
//                       each owns the pixels of one side of the ORIGINAL mask, which it reads again: class 2's workgroup the pixels that
//                       were 2, class 1's all others.  No byte has two writers and no memset is needed.
//   Workgroup size and words per thread.  The LDS bounds the plane at 20 472 words.  1024 threads (16 waves, 4 per SIMD, 128 VGPRs each)
//   own at most TH_WPT = 20 words: del[] is 40 VGPRs, a word's nine operands and eight planes about 40 more, so the kernel stays well
//   inside 128 without spilling (the build's resource report: no scratch).  Half the threads would double del[] to 80 registers for no
//   gain -- the loop is bound by LDS latency, which more waves hide -- and the barrier count per pass (4) does not depend on it.
//   Thinning is serial in its passes and a batch of 8 frames fills 16 of the 256 CUs; the plane is not split across CUs.
//
//   ax_stats   one workgroup per 32 x 64 tile (event_common.h).  The tile and a halo of one pixel are staged in LDS as "label word where
//              the skeleton has a pixel, else 0" (the label is read only under a skeleton pixel), so the eight neighbour tests of a pixel are
//              LDS compares.  A thread walks 8 consecutive pixels of a row and reduces each run of one root in registers; a run goes to
//              the workgroup's slot table (slot_claim), a full table sends it to its global row, filled slots are flushed at the end.
//              event_shape.hip's staging, lane layout and row stride (SH_STRIDE has the bank argument), with this kernel's seven terms.
// 64-bit integer atomics only; no workgroup waits for another.
#include "skeleton_bits.h"

namespace dc {

// n >= 2 and n == 4 of n = a + b + c + d, bit-sliced: a full adder on (a, b, c), a half adder on its sum and d
__device__ inline void th_sum4(u64 a, u64 b, u64 c, u64 d, u64* ge2, u64* eq4) {
  const u64 s = a ^ b ^ c, c1 = (a & b) | (c & (a ^ b));
  const u64 c2 = s & d;                           // n = (s ^ d) + 2 (c1 + c2): bit 1 = c1 ^ c2, bit 2 = c1 & c2
  *ge2 = c1 | c2;
  *eq4 = c1 & c2;
}

// the pixels of word i (value c, not zero) that sub-pass SUB (0: A, 1: B) deletes
template <int SUB>
__device__ inline u64 th_delete(const u64* P, int i, u64 c, int H, int TW, int lastbit, int wrap) {
  u64 p[8];
  th_ring(P, i, c, H, TW, lastbit, wrap, p);
  const u64 p2 = p[0], p3 = p[1], p4 = p[2], p5 = p[3], p6 = p[4], p7 = p[5], p8 = p[6], p9 = p[7];
  // C == 1: exactly one of the four terms -- odd parity, and no pair (three terms hold one of the two pairs)
  const u64 t1 = ~p2 & (p3 | p4), t2 = ~p4 & (p5 | p6), t3 = ~p6 & (p7 | p8), t4 = ~p8 & (p9 | p2);
  const u64 c1 = (t1 ^ t2 ^ t3 ^ t4) & ~((t1 & t2) | (t3 & t4));
  // 2 <= min(N1, N2) <= 3: both sums at least 2, not both 4
  u64 g1, f1, g2, f2;
  th_sum4(p9 | p2, p3 | p4, p5 | p6, p7 | p8, &g1, &f1);
  th_sum4(p2 | p3, p4 | p5, p6 | p7, p8 | p9, &g2, &f2);
  const u64 nok = g1 & g2 & ~(f1 & f2);
  const u64 m = SUB == 0 ? (p6 | p7 | ~p9) & p8 : (p2 | p3 | ~p5) & p4;
  return c & c1 & nok & ~m;
}

// one sub-pass over the plane of n words; true when any pixel of the plane was deleted.  Every thread of the workgroup calls it.
template <int SUB>
__device__ inline bool th_subpass(u64* P, volatile unsigned* flag, int n, int H, int TW, int lastbit, int wrap) {
  u64 del[TH_WPT];
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));                   // opaque: a word's row, column and neighbour indices are computed where they are used and
                                                  // not kept across the passes, where twenty words' worth of them would crowd out del[]
#pragma unroll
  for (int k = 0; k < TH_WPT; ++k) {
    const int i = tid + k * TH_THREADS;
    del[k] = 0;
    if (i < n) {
      const u64 c = P[i];
      if (c) del[k] = th_delete<SUB>(P, i, c, H, TW, lastbit, wrap);
    }
    __builtin_amdgcn_sched_barrier(0);            // one word at a time: interleaving the unrolled bodies only costs registers
  }
  __syncthreads();                                // every read of this sub-pass lies before this barrier, every write behind it
  u64 any = 0;
#pragma unroll
  for (int k = 0; k < TH_WPT; ++k)
    if (del[k]) {
      P[tid + k * TH_THREADS] &= ~del[k];
      any |= del[k];
    }
  if (threadIdx.x == 0) flag[SUB ^ 1] = 0u;
  if (__ballot(any != 0) && (threadIdx.x & 63) == 0) flag[SUB] = 1u;
  __syncthreads();
  return flag[SUB] != 0u;
}

__global__ __launch_bounds__(TH_THREADS) void th_thin_kernel(int H, int W, const void* __restrict__ mask, int mask_bytes, int wrap,
                                                             int max_iters, uint8_t* __restrict__ skeleton, int* __restrict__ iters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int TW = (W + 63) / 64, n = H * TW, lastbit = (W - 1) & 63;
  u64* P = (u64*)smem;
  volatile unsigned* flag = (volatile unsigned*)(smem + (size_t)n * 8);
  const unsigned cls = blockIdx.x + 1;
  const int b = blockIdx.y;
  const size_t base = (size_t)b * H * W;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < 3) flag[threadIdx.x] = 0u;   // A's, B's, and "the packed plane holds a pixel"
  __syncthreads();
  // pack: a wave's ballot over 64 consecutive columns is one word; TH_BATCH words' loads are in flight together
  u64 some = 0;
  for (int item0 = wave; item0 < n; item0 += TH_BATCH * TH_WAVES) {
    unsigned c[TH_BATCH];
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) c[q] = th_class(mask, mask_bytes, base, item0 + q * TH_WAVES, n, TW, W, lane);
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) {
      const int item = item0 + q * TH_WAVES;
      const u64 w = __ballot(c[q] == cls);
      if (item < n && lane == 0) P[item] = w;
      some |= w;
    }
  }
  if (some != 0 && lane == 0) flag[2] = 1u;
  __syncthreads();
  int passes = 1, converged = 1;                  // an empty plane: the one pass that deletes nothing, not run
  if (flag[2] != 0u) {
    passes = 0, converged = 0;
    while (passes < max_iters) {
      const bool a = th_subpass<0>(P, flag, n, H, TW, lastbit, wrap);
      const bool bb = th_subpass<1>(P, flag, n, H, TW, lastbit, wrap);
      ++passes;
      if (!a && !bb) {
        converged = 1;
        break;
      }
    }
  }
  // expand: class 2's workgroup owns the pixels whose mask was 2, class 1's every other pixel (TH_NONE: not a pixel)
  for (int item0 = wave; item0 < n; item0 += TH_BATCH * TH_WAVES) {
    unsigned c[TH_BATCH];
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) c[q] = th_class(mask, mask_bytes, base, item0 + q * TH_WAVES, n, TW, W, lane);
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) {
      const int item = item0 + q * TH_WAVES;
      if (c[q] != TH_NONE && (c[q] == 2u) == (cls == 2u)) {
        const int r = item / TW;
        skeleton[base + (size_t)r * W + (item - r * TW) * 64 + lane] = (P[item] >> lane) & 1ull ? (uint8_t)cls : (uint8_t)0;
      }
    }
  }
  if (threadIdx.x == 0) {
    iters[(b * 2 + (int)cls - 1) * 2] = passes;
    iters[(b * 2 + (int)cls - 1) * 2 + 1] = converged;
  }
}

// ---- the statistics of a skeleton ------------------------------------------------------------------------------------------------------
static constexpr int AX_FIELDS = 7;               // skeleton_pixels, endpoints, junctions, links_ew, links_ns, links_diag, length_m
static constexpr int AX_SLOTS = 128, AX_PROBES = 4;
static constexpr int AX_LH = CC_TH + 2, AX_LW = CC_TW + 2;
static constexpr int AX_STRIDE = 67;              // event_shape.hip's SH_STRIDE: odd, the lane layout below reads conflict-free
static_assert(AX_STRIDE >= AX_LW, "ax_stats_kernel: a staged row holds the tile's columns and the halo");

struct AxRun {                                    // one thread's run of skeleton pixels of one event inside one row (at most 8 pixels)
  int root, n, ends, junctions, ew, ns, diag;
};

__device__ inline void ax_terms(const AxRun& a, const int* __restrict__ lt, long long* t) {
  t[0] = a.n, t[1] = a.ends, t[2] = a.junctions, t[3] = a.ew, t[4] = a.ns, t[5] = a.diag;
  t[6] = (long long)a.ew * lt[0] + (long long)a.ns * lt[1] + (long long)a.diag * lt[2];
}

__device__ inline void ax_emit(const int* __restrict__ rank_sample, long HW, int cap, long long* rows_sample, int root, const long long* t) {
  const int rank = event_rank(rank_sample, HW, cap, root);
  if (rank < 0) return;
  u64* row = (u64*)(rows_sample + (size_t)rank * AX_FIELDS);
#pragma unroll
  for (int f = 0; f < AX_FIELDS; ++f)
    if (t[f] != 0) atomicAdd(row + f, (u64)t[f]);
}

__global__ __launch_bounds__(256) void ax_zero_kernel(long n, long long* __restrict__ rows) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) rows[i] = 0;
}

__global__ __launch_bounds__(256) void ax_stats_kernel(int H, int W, int wrap, const uint8_t* __restrict__ skeleton,
                                                       const int* __restrict__ labels, const int* __restrict__ link, int cap,
                                                       const int* __restrict__ rank_map, long long* __restrict__ rows) {
  __shared__ int s_lab[AX_LH * AX_STRIDE];
  __shared__ int s_key[AX_SLOTS];
  __shared__ u64 s_sum[AX_SLOTS][AX_FIELDS];
  const long HW = (long)H * W;
  const size_t base = (size_t)blockIdx.z * HW;
  const uint8_t* S = skeleton + base;
  const int* L = labels + base;
  const int* rank_sample = rank_map + base;
  long long* rows_sample = rows + (size_t)blockIdx.z * cap * AX_FIELDS;
  const int r0 = blockIdx.y * CC_TH, c0 = blockIdx.x * CC_TW;
  if (threadIdx.x < AX_SLOTS) {
    const int s = threadIdx.x;
    s_key[s] = -1;
#pragma unroll
    for (int f = 0; f < AX_FIELDS; ++f) s_sum[s][f] = 0ull;
  }
  // the tile and its halo: rows r0 - 1 .. r0 + TH, columns c0 - 1 .. c0 + TW; the label word under a skeleton pixel, 0 everywhere else
  for (int i = threadIdx.x; i < AX_LH * AX_LW; i += 256) {
    const int lr = i / AX_LW, lc = i % AX_LW;
    const int gr = r0 - 1 + lr;
    int gc = c0 - 1 + lc;
    if (wrap) gc = gc < 0 ? W - 1 : (gc == W ? 0 : gc);
    int v = 0;
    if (gr >= 0 && gr < H && gc >= 0 && gc < W && S[(size_t)gr * W + gc] != 0) v = L[(size_t)gr * W + gc];
    s_lab[lr * AX_STRIDE + lc] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = wave * 8 + (lane & 7), lcb = (lane >> 3) * 8;          // sh_pixel_kernel's lane layout
  const int r = r0 + lr, cb = c0 + lcb;
  if (r < H) {
    const int* lt = link + (size_t)r * 3;
    const int* mid = s_lab + (lr + 1) * AX_STRIDE + lcb + 1;            // the thread's first pixel
    AxRun a;
    a.root = -1;
    for (int j = 0; j <= 8; ++j) {
      const int v = (j < 8 && cb + j < W) ? mid[j] : 0;                 // (column W holds column 0's word under wrap: not a pixel)
      const int root = v - 1;                     // -1: no skeleton pixel, the row's end, the run's end
      if (root != a.root) {
        if (a.root >= 0) {
          long long t[AX_FIELDS];
          ax_terms(a, lt, t);
          const int hit = slot_claim<AX_SLOTS, AX_PROBES>(s_key, slot_hash<AX_SLOTS>(a.root), a.root);
          if (hit >= 0) {
#pragma unroll
            for (int f = 0; f < AX_FIELDS; ++f)
              if (t[f] != 0) atomicAdd(&s_sum[hit][f], (u64)t[f]);
          } else {
            ax_emit(rank_sample, HW, cap, rows_sample, a.root, t);
          }
        }
        a.root = root;
        a.n = a.ends = a.junctions = a.ew = a.ns = a.diag = 0;
      }
      if (root >= 0) {
        const int* p = mid + j;                   // the ring, clockwise from north
        const int n2 = p[-AX_STRIDE] == v, n3 = p[-AX_STRIDE + 1] == v, n4 = p[1] == v, n5 = p[AX_STRIDE + 1] == v;
        const int n6 = p[AX_STRIDE] == v, n7 = p[AX_STRIDE - 1] == v, n8 = p[-1] == v, n9 = p[-AX_STRIDE - 1] == v;
        const int count = n2 + n3 + n4 + n5 + n6 + n7 + n8 + n9;
        const int rises = (n3 > n2) + (n4 > n3) + (n5 > n4) + (n6 > n5) + (n7 > n6) + (n8 > n7) + (n9 > n8) + (n2 > n9);
        a.n += 1;
        a.ends += count == 1;
        a.junctions += rises >= 3;
        a.ew += n4;
        a.ns += n6;
        a.diag += (n5 > (n4 | n6)) + (n7 > (n8 | n6));                  // a diagonal beside a corner pixel is the corner, not a link
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < AX_SLOTS && s_key[threadIdx.x] >= 0) {
    const int s = threadIdx.x;
    long long t[AX_FIELDS];
#pragma unroll
    for (int f = 0; f < AX_FIELDS; ++f) t[f] = (long long)s_sum[s][f];
    ax_emit(rank_sample, HW, cap, rows_sample, s_key[s], t);
  }
}

}  // namespace dc

using namespace dc;

extern "C" size_t dc_thin_lds_bytes(int H, int W) { return th_lds_bytes(H, W); }

extern "C" int dc_mask_thin(int B, int n_valid, int H, int W, const void* mask, int mask_bytes, int wrap, int max_iters, uint8_t* skeleton,
                            int32_t* iters, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(mask_bytes == 1 || mask_bytes == 4 || mask_bytes == 8, "dc_mask_thin: mask_bytes must be 1, 4 or 8");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_mask_thin: wrap must be 0 or 1");
  DC_REQUIRE(max_iters >= 1, "dc_mask_thin: max_iters must be at least 1");
  DC_REQUIRE(mask && skeleton && iters, "dc_mask_thin: null pointer");
  DC_REQUIRE(((uintptr_t)mask & (mask_bytes - 1)) == 0, "dc_mask_thin: the mask is not aligned to its element size");
  const size_t lds = th_lds_bytes(H, W);
  DC_REQUIRE(lds != 0, "dc_mask_thin: the bit plane of H x W does not fit the LDS of one CU (H * ceil(W / 64) * 8 + 64 bytes of 160 KiB)");
  const size_t px = (size_t)B * H * W;
  DC_REQUIRE((uintptr_t)skeleton + px <= (uintptr_t)mask || (uintptr_t)mask + px * mask_bytes <= (uintptr_t)skeleton,
             "dc_mask_thin: skeleton may not alias mask");
  DC_ONCE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&th_thin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TH_LDS_MAX));
  hipLaunchKernelGGL(th_thin_kernel, dim3(2, n_valid), dim3(TH_THREADS), lds, (hipStream_t)stream, H, W, mask, mask_bytes, wrap, max_iters,
                     skeleton, iters);
  DC_LAUNCHED("skel_thin");
  return 0;
}

extern "C" int dc_skeleton_stats(int B, int n_valid, int H, int W, const uint8_t* skeleton, const int32_t* labels, const void* ws, int cap,
                                 int wrap, const int32_t* link_table, int64_t* rows, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(cap >= 1, "dc_skeleton_stats: cap must be at least 1");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_skeleton_stats: wrap must be 0 or 1");
  DC_REQUIRE(skeleton && labels && ws && link_table && rows, "dc_skeleton_stats: null pointer");
  DC_REQUIRE(((uintptr_t)ws & 3) == 0 && ((uintptr_t)rows & 7) == 0, "dc_skeleton_stats: the workspace or the rows are not aligned");
  hipStream_t st = (hipStream_t)stream;
  const long words = (long)n_valid * cap * AX_FIELDS;
  hipLaunchKernelGGL(ax_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, words, (long long*)rows);
  DC_LAUNCHED("skel_stats");
  hipLaunchKernelGGL(ax_stats_kernel, cc_tile_grid(H, W, n_valid), dim3(256), 0, st, H, W, wrap, skeleton, labels, link_table, cap,
                     (const int*)ws, (long long*)rows);
  DC_LAUNCHED("skel_stats");
  return 0;
}
