// Storm-centred composites (dc_composite_centers, dc_composite_accumulate; nn.StormComposite): windows of the raw fields around every
// event's centre, summed over the events of a group as integers, with the azimuthal sums per distance bin.  include/deepcam_hip.h has the
// definition; this file has the decomposition.
//   comp_centers     one thread per catalogue row: the row's category, its centre pixel out of the EventFields word, its group and
//                    intensity bin; the five counters go through LDS, one atomic per workgroup and counter.
//   comp_accumulate<V>  the inverted gather.  A thread owns one ITEM of the window: V consecutive selected channels of one cell (V = 4, the
//                    vector form: the selection is the identity over ldc channels, so for a fixed event the lanes of a wave read
//                    consecutive 16-byte pieces, four lanes per 16-channel pixel, split only where the window crosses the seam; V = 1, the
//                    scalar form: any selection).  blockIdx.x picks 256 items, blockIdx.y a SLICE of the batch: a frame's catalogue rows cut
//                    into ksplit ranges of whole 256-row blocks, none shorter than a chunk, as many as bring the grid to about
//                    CP_TARGET_WGS workgroups.
//                    A workgroup scans its slices' `centers` 256 rows at a time and compacts the composited events into a worklist in LDS
//                    (CP_CHUNK entries: centre row and column, frame, group, label word); when the list is full, and at the end, it is
//                    worked off one GROUP at a time, smallest first: every thread walks the chunk's events of that group with its partial
//                    sums in registers and adds them to the accumulators once, the radial bins are summed in LDS and leave with one 64-bit
//                    atomic per workgroup and word.  Slices and chunks meet in integer atomics: nothing depends on the order.
//                    Where the radial table does not fit LDS (NB * C > CP_RAD_WORDS) the radial adds go to global memory directly.
#include "common.h"

namespace dc {

static constexpr int CP_CHUNK = 512;              // events of a worklist chunk
static constexpr int CP_MAXC = 32;
static constexpr int CP_MAXR = 40;
static constexpr int CP_RAD_WORDS = 4096;         // radial words (NB * C) the LDS table holds: 48 KiB
static constexpr int CP_TARGET_WGS = 2048;        // a frame's rows are cut into slices until the grid has about this many workgroups
static constexpr int CP_COUNTS = 5;               // composited, no_center, below_min_pixels, other_class, uncatalogued
static constexpr int CP_TABLE_FIELDS = 10, CP_FIELD_STATS = 6;

typedef float cp_f4 __attribute__((ext_vector_type(4)));

// the order-preserving key of dc_component_fields
__device__ inline unsigned cp_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void comp_centers_kernel(int cap, long long HW, const long long* __restrict__ table,
                                                           const int32_t* __restrict__ ncomp, const long long* __restrict__ ftable, int Cf,
                                                           int center_channel, int stat, int class_mask, long long min_pixels,
                                                           const int32_t* __restrict__ frame_group, int G, const float* __restrict__ edges,
                                                           int NE, int32_t* __restrict__ centers, int32_t* __restrict__ egroup,
                                                           unsigned long long* counts) {
  __shared__ unsigned s_n[CP_COUNTS];
  const int b = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < CP_COUNTS) s_n[threadIdx.x] = 0u;
  __syncthreads();
  const int fg = frame_group[b];
  const bool frame_ok = fg >= 0 && fg < G;
  const int total = ncomp[b * 3];
  const int rows = total < 0 ? 0 : (total > cap ? cap : total);
  if (k < cap) {
    int center = -1, eg = -1;
    if (frame_ok && k < rows) {
      const size_t e = (size_t)b * cap + k;
      const long long cls = table[e * CP_TABLE_FIELDS + 1], px = table[e * CP_TABLE_FIELDS + 2];
      int cat;
      if (!((cls == 1 || cls == 2) && ((class_mask >> (int)cls) & 1))) cat = 3;
      else if (px < min_pixels) cat = 2;
      else {
        const unsigned long long word = (unsigned long long)ftable[(e * Cf + center_channel) * CP_FIELD_STATS + stat];
        const bool empty = stat == 0 ? word == ~0ull : word == 0ull;
        const unsigned low = (unsigned)(word & 0xFFFFFFFFull);
        const unsigned p = stat == 0 ? low : 0xFFFFFFFFu - low;
        if (empty || (long long)p >= HW) cat = 1;      // a pixel off the grid is no centre either: nothing is read through it
        else {
          cat = 0;
          const unsigned key = (unsigned)(word >> 32);
          int bin = 0;
          for (int i = 0; i < NE; ++i) bin += key >= cp_key(edges[i]);
          center = (int)p;
          eg = fg * (NE + 1) + bin;
        }
      }
      atomicAdd(&s_n[cat], 1u);
    }
    centers[(size_t)b * cap + k] = center;
    egroup[(size_t)b * cap + k] = eg;
  }
  if (k == 0 && frame_ok && total > cap) atomicAdd(&s_n[4], (unsigned)(total - cap));
  __syncthreads();
  if (threadIdx.x < CP_COUNTS && s_n[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)s_n[threadIdx.x]);
}

template <int V>
__global__ __launch_bounds__(256) void comp_accumulate_kernel(int n_valid, int ksplit, int slice_rows, int H, int W, int cap, int R, int GT,
                                                              const int32_t* __restrict__ centers, const int32_t* __restrict__ egroup,
                                                              const long long* __restrict__ table, const int32_t* __restrict__ labels,
                                                              const float* __restrict__ fields, int C, int ldc,
                                                              const int32_t* __restrict__ chan, const int32_t* __restrict__ bits,
                                                              unsigned negate_mask, int flip_south, const uint8_t* __restrict__ rbin, int NB,
                                                              int rad_lds, unsigned long long* events, unsigned long long* sum, int32_t* n,
                                                              int32_t* inside, unsigned long long* rsum, unsigned long long* rn) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cp_smem[];
  __shared__ int s_r0[CP_CHUNK], s_c0[CP_CHUNK], s_b[CP_CHUNK], s_g[CP_CHUNK], s_lab[CP_CHUNK];
  __shared__ int s_count;
  const int radw = rad_lds ? NB * C : 0;            // the LDS radial table: int64 [NB][C] sums, then int32 [NB][C] numbers
  unsigned long long* s_rs = (unsigned long long*)cp_smem;
  unsigned* s_rn = (unsigned*)(cp_smem + (size_t)radw * 8);
  const int tid = threadIdx.x;
  const int S = 2 * R + 1, Q = C / V;
  const int t = blockIdx.x * 256 + tid;
  const bool live = t < S * S * Q;
  const int q = t % Q, cell = t / Q;
  const int di = cell / S - R, dj = cell % S - R, adj = dj < 0 ? -dj : dj;
  int sh[V], col[V];
  bool neg[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sh[j] = 0, col[j] = -1, neg[j] = false;
    if (live) {
      const int c = q * V + j;
      const int ch = chan ? chan[c] : c;
      sh[j] = bits[c];
      col[j] = (ch >= 0 && ch < ldc) ? ch : -1;
      neg[j] = (negate_mask >> c) & 1u;
    }
  }
  for (int i = tid; i < radw; i += 256) s_rs[i] = 0ull, s_rn[i] = 0u;
  if (tid == 0) s_count = 0;
  __syncthreads();

  // the chunk's events, one group at a time
  auto work = [&]() {
    const int count = s_count;
    int last = -1;
    for (;;) {
      int cur = 0x7fffffff;
      for (int e = 0; e < count; ++e) {
        const int g = s_g[e];
        cur = (g > last && g < cur) ? g : cur;
      }
      if (cur == 0x7fffffff) break;
      long long ps[V];
      int pn[V], pin = 0, nev = 0;
#pragma unroll
      for (int j = 0; j < V; ++j) ps[j] = 0, pn[j] = 0;
      for (int e = 0; e < count; ++e) {
        if (s_g[e] != cur) continue;
        ++nev;
        if (!live) continue;
        const int r0 = s_r0[e], c0 = s_c0[e];
        const bool south = flip_south && 2 * r0 < H - 1;
        const int r = south ? r0 - di : r0 + di;
        if (r < 0 || r >= H) continue;                // no wrap over the poles
        int c = c0 + dj;
        c = c < 0 ? c + W : (c >= W ? c - W : c);    // S <= W: one step is enough
        const size_t px = ((size_t)s_b[e] * H + r) * W + c;
        if (q == 0) pin += labels[px] == s_lab[e];
        float v[V];
        if constexpr (V == 4) {
          const cp_f4 f = *(const cp_f4*)(fields + px * ldc + q * 4);
          v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) v[j] = col[j] >= 0 ? fields[px * ldc + col[j]] : __uint_as_float(0x7fc00000u);
        }
        int k = 255;
        if (rbin) k = rbin[((size_t)r0 * S + (r - r0 + R)) * (R + 1) + adj];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const double s = rint(ldexp((double)v[j], sh[j]));   // NaN and +-Inf fail the comparison as well
          const bool ok = fabs(s) <= 0x1p28;
          long long qi = ok ? (long long)s : 0;
          if (neg[j] && south) qi = -qi;
          ps[j] += qi, pn[j] += ok;
          if (ok && k < NB) {
            const int w = k * C + q * V + j;
            if (rad_lds) {
              atomicAdd(&s_rs[w], (unsigned long long)qi);
              atomicAdd(&s_rn[w], 1u);
            } else {
              atomicAdd(&rsum[(size_t)cur * NB * C + w], (unsigned long long)qi);
              atomicAdd(&rn[(size_t)cur * NB * C + w], 1ull);
            }
          }
        }
      }
      if (live) {
        const size_t off = ((size_t)cur * S * S + cell) * C + q * V;
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (pn[j]) {
            atomicAdd(&sum[off + j], (unsigned long long)ps[j]);
            atomicAdd(&n[off + j], pn[j]);
          }
        if (q == 0 && pin) atomicAdd(&inside[(size_t)cur * S * S + cell], pin);
      }
      if (blockIdx.x == 0 && tid == 0) atomicAdd(&events[cur], (unsigned long long)nev);
      if (radw) {
        __syncthreads();
        for (int i = tid; i < radw; i += 256) {
          const unsigned cnt = s_rn[i];
          if (cnt) {
            atomicAdd(&rsum[(size_t)cur * radw + i], s_rs[i]);
            atomicAdd(&rn[(size_t)cur * radw + i], (unsigned long long)cnt);
            s_rs[i] = 0ull, s_rn[i] = 0u;
          }
        }
        __syncthreads();
      }
      last = cur;
    }
  };

  for (int u = blockIdx.y; u < n_valid * ksplit; u += gridDim.y) {
    const int b = u / ksplit, part = u % ksplit;
    const int kend = (part + 1) * slice_rows < cap ? (part + 1) * slice_rows : cap;
    for (int k0 = part * slice_rows; k0 < kend; k0 += 256) {
      const int k = k0 + tid;
      if (k < kend) {
        const size_t e = (size_t)b * cap + k;
        const int p = centers[e], g = egroup[e];
        if (p >= 0 && p < H * W && g >= 0 && g < GT) {
          const int slot = atomicAdd(&s_count, 1);
          s_r0[slot] = p / W, s_c0[slot] = p % W, s_b[slot] = b, s_g[slot] = g;
          s_lab[slot] = (int)table[e * CP_TABLE_FIELDS] + 1;
        }
      }
      __syncthreads();
      const int filled = s_count;
      __syncthreads();                              // everyone has read the count before the next rows move it
      if (filled > CP_CHUNK - 256) {                // the next 256 rows might not fit
        work();
        __syncthreads();
        if (tid == 0) s_count = 0;
        __syncthreads();
      }
    }
  }
  work();
}

}  // namespace dc

using namespace dc;

extern "C" int dc_composite_chunk(int* events) {
  DC_REQUIRE(events, "dc_composite_chunk: null argument");
  *events = CP_CHUNK;
  return 0;
}

extern "C" int dc_composite_centers(int B, int n_valid, int H, int W, int cap, const int64_t* table, const int32_t* ncomp,
                                    const int64_t* ftable, int Cf, int center_channel, int stat, int class_mask, long min_pixels,
                                    const int32_t* frame_group, int G, const float* edges, int NE, int32_t* centers, int32_t* egroup,
                                    int64_t* counts, void* stream) {
  DC_REQUIRE(B > 0 && n_valid > 0 && n_valid <= B && n_valid <= 65535, "dc_composite_centers: n_valid must lie in [1, min(B, 65535)]");
  DC_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= (1L << 22), "dc_composite_centers: H and W must be positive and H * W at most 2^22");
  DC_REQUIRE(cap >= 1 && cap <= (1 << 22), "dc_composite_centers: cap must lie in [1, 2^22]");
  DC_REQUIRE(Cf >= 1 && Cf <= CP_MAXC && center_channel >= 0 && center_channel < Cf,
             "dc_composite_centers: Cf must lie in [1, 32] and center_channel in [0, Cf)");
  DC_REQUIRE(stat == 0 || stat == 1, "dc_composite_centers: stat must be 0 (min) or 1 (max)");
  DC_REQUIRE(class_mask >= 1 && class_mask <= 6 && (class_mask & 1) == 0, "dc_composite_centers: class_mask must be 2, 4 or 6");
  DC_REQUIRE(min_pixels >= 0, "dc_composite_centers: min_pixels must not be negative");
  DC_REQUIRE(G >= 1 && NE >= 0 && NE <= 255 && (long)G * (NE + 1) <= 65536, "dc_composite_centers: G >= 1, 0 <= NE <= 255, G * (NE + 1) <= 65536");
  DC_REQUIRE(table && ncomp && ftable && frame_group && centers && egroup && counts && (NE == 0 || edges), "dc_composite_centers: null pointer");
  DC_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)ftable & 7) == 0 && ((uintptr_t)counts & 7) == 0 && ((uintptr_t)ncomp & 3) == 0 &&
                 ((uintptr_t)frame_group & 3) == 0 && ((uintptr_t)edges & 3) == 0 && ((uintptr_t)centers & 3) == 0 && ((uintptr_t)egroup & 3) == 0,
             "dc_composite_centers: a pointer is not aligned to its element size");
  hipLaunchKernelGGL(comp_centers_kernel, dim3((cap + 255) / 256, n_valid), dim3(256), 0, (hipStream_t)stream, cap, (long long)H * W,
                     (const long long*)table, ncomp, (const long long*)ftable, Cf, center_channel, stat, class_mask, (long long)min_pixels,
                     frame_group, G, edges, NE, centers, egroup, (unsigned long long*)counts);
  DC_LAUNCHED("composite_centers");
  return 0;
}

extern "C" int dc_composite_accumulate(int B, int n_valid, int H, int W, int cap, int R, int GT, const int32_t* centers, const int32_t* egroup,
                                       const int64_t* table, const int32_t* labels, const float* fields, int C, int ldc, const int32_t* chan,
                                       const int32_t* bits, int negate_mask, int flip_south, const uint8_t* rbin, int NB, int64_t* events,
                                       int64_t* sum, int32_t* n, int32_t* inside, int64_t* rsum, int64_t* rn, void* stream) {
  DC_REQUIRE(B > 0 && n_valid > 0 && n_valid <= B && n_valid <= 65535, "dc_composite_accumulate: n_valid must lie in [1, min(B, 65535)]");
  DC_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= (1L << 22), "dc_composite_accumulate: H and W must be positive and H * W at most 2^22");
  DC_REQUIRE(cap >= 1 && cap <= (1 << 22), "dc_composite_accumulate: cap must lie in [1, 2^22]");
  DC_REQUIRE(R >= 1 && R <= CP_MAXR && 2 * R + 1 <= W, "dc_composite_accumulate: R must lie in [1, 40] and 2 R + 1 may not exceed W");
  DC_REQUIRE(GT >= 1 && GT <= 65536, "dc_composite_accumulate: GT must lie in [1, 65536]");
  DC_REQUIRE(C >= 1 && C <= CP_MAXC, "dc_composite_accumulate: C must lie in [1, 32]");
  DC_REQUIRE(ldc >= 1 && (chan != nullptr || ldc >= C), "dc_composite_accumulate: ldc must be positive, and at least C when chan is null");
  DC_REQUIRE(flip_south == 0 || flip_south == 1, "dc_composite_accumulate: flip_south must be 0 or 1");
  DC_REQUIRE(rbin ? (NB >= 1 && NB <= 255) : NB == 0, "dc_composite_accumulate: NB must lie in [1, 255] with rbin, and be 0 without");
  DC_REQUIRE(centers && egroup && table && labels && fields && bits && events && sum && n && inside, "dc_composite_accumulate: null pointer");
  DC_REQUIRE(rbin == nullptr || (rsum && rn), "dc_composite_accumulate: null pointer (rsum and rn are needed with rbin)");
  DC_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)events & 7) == 0 && ((uintptr_t)sum & 7) == 0 && ((uintptr_t)rsum & 7) == 0 &&
                 ((uintptr_t)rn & 7) == 0 && ((uintptr_t)centers & 3) == 0 && ((uintptr_t)egroup & 3) == 0 && ((uintptr_t)labels & 3) == 0 &&
                 ((uintptr_t)fields & 3) == 0 && ((uintptr_t)chan & 3) == 0 && ((uintptr_t)bits & 3) == 0 && ((uintptr_t)n & 3) == 0 &&
                 ((uintptr_t)inside & 3) == 0,
             "dc_composite_accumulate: a pointer is not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  const int S = 2 * R + 1;
  const int S2 = S * S, row_blocks = (cap + 255) / 256;
  const int rad_lds = NB * C <= CP_RAD_WORDS;
  const size_t smem = rad_lds ? (size_t)NB * C * 12 : 0;
  // the vector form: the selection is the identity over all ldc channels, whole quads, every 16-byte piece aligned
  const bool vec = chan == nullptr && ldc == C && C % 4 == 0 && ((uintptr_t)fields & 15) == 0;
  // the grid: x over the window's items, y over the slices -- a frame's rows in ksplit ranges of whole 256-row blocks, none shorter than a
  // chunk of rows, as many as bring the grid to about CP_TARGET_WGS workgroups
  const int xblocks = (S2 * (vec ? C / 4 : C) + 255) / 256;
  const int want = CP_TARGET_WGS / (xblocks * n_valid);
  const int most = row_blocks / (CP_CHUNK / 256) < 1 ? 1 : row_blocks / (CP_CHUNK / 256);
  const int ksplit = want < 1 ? 1 : (want > most ? most : want);
  const int slice_rows = (row_blocks + ksplit - 1) / ksplit * 256;
  const long slices = (long)n_valid * ksplit;
  const dim3 grid(xblocks, (unsigned)(slices < 65535 ? slices : 65535));
  if (vec) {
    hipLaunchKernelGGL(comp_accumulate_kernel<4>, grid, dim3(256), smem, st, n_valid, ksplit, slice_rows, H, W, cap, R, GT, centers, egroup,
                       (const long long*)table, labels, fields, C, ldc, chan, bits, (unsigned)negate_mask, flip_south, rbin, NB, rad_lds,
                       (unsigned long long*)events, (unsigned long long*)sum, n, inside, (unsigned long long*)rsum, (unsigned long long*)rn);
    DC_LAUNCHED("composite_accumulate_vec");
  } else {
    hipLaunchKernelGGL(comp_accumulate_kernel<1>, grid, dim3(256), smem, st, n_valid, ksplit, slice_rows, H, W, cap, R, GT, centers, egroup,
                       (const long long*)table, labels, fields, C, ldc, chan, bits, (unsigned)negate_mask, flip_south, rbin, NB, rad_lds,
                       (unsigned long long*)events, (unsigned long long*)sum, n, inside, (unsigned long long*)rsum, (unsigned long long*)rn);
    DC_LAUNCHED("composite_accumulate_scalar");
  }
  return 0;
}
