// Event catalogue: connected components of a class mask and their statistics (dc_mask_components, dc_component_stats; nn.EventCatalog).
//
// Classes 1 and 2 are foreground, everything else background.  A component is a maximal set of pixels of ONE class connected under 4- or
// 8-connectivity; with wrap the columns are periodic (column W-1 touches column 0), the rows never are.  Every foreground pixel ends up
// with 1 + the smallest linear index r * W + c of its component (its root), background with 0.
//
// The label map doubles as the parent array of a union-find forest.  The encoding is the final one from the first store on: a word holds
// parent + 1 (0: background), a root holds its own index + 1.  Two invariants carry every argument below:
//   (I1) a parent's index is never larger than its child's, and equal only at a root, so every walk towards a root strictly descends and
//        ends by itself, whatever other workgroups do meanwhile and however stale the words it reads are;
//   (I2) every word a pixel's entry has EVER held names a pixel of its component, so a walk over old values still ends inside the component.
// Links change by atomicMin only (I1 holds: both candidates are smaller than the child).  When an atomicMin replaces a link a -> old by
// a -> b, the caller goes on to unite old and b, which restores the equivalence the replaced link stood for (Playne & Hawick 2018, Komura
// 2015).  No workgroup waits for another: the order of the phases is the order of the launches on one stream.
//   cc_tile     one workgroup labels a TH x TW tile in LDS (union-find on local indices) and stores parent = the tile-local root
//   cc_merge    one thread per pixel on a tile border or on the seam unites it with its neighbours across that border
//   cc_flatten  every pixel's word becomes root + 1
//   cc_stats    roots are flagged, ranked by an order-preserving prefix count per sample, and the ten fields accumulated into row `rank`
#include "common.h"

namespace dc {

static constexpr int CC_TH = 32, CC_TW = 64;      // the tile: 2048 pixels, 8 per thread of a 256-thread workgroup, 10 KiB of LDS
static constexpr int CC_TPX = CC_TH * CC_TW;
static constexpr int CC_CHUNK = 256;              // pixels per workgroup of the root count and rank passes (one per thread)
static constexpr int CC_FIELDS = 10;
static constexpr int CC_SLOTS = 128;              // per-workgroup table of partial sums in the statistics pass
static constexpr int CC_PROBES = 4;

__device__ inline int cc_class(uint8_t m) { return (m == 1 || m == 2) ? (int)m : 0; }

// ---- LDS forest (local indices, parent stored plain: root = self) ------------------------------------------------------------------
__device__ inline int lds_find(int* s, int x) {
  for (;;) {
    const int p = __hip_atomic_load(s + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p >= x || p < 0) return x;      // root (p == x); anything else cannot occur and ends the walk as well
    x = p;
  }
}
// max(a, b) strictly falls from one round to the next, so the loop ends after at most CC_TPX rounds
__device__ inline void lds_union(int* s, int a, int b) {
  for (;;) {
    a = lds_find(s, a);
    b = lds_find(s, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(s + a, b);
    if (old >= a) return;               // a was a root and now hangs below b
    a = old;                            // a had been linked meanwhile: its former parent and b are still to be united
  }
}

// ---- global forest (sample-local linear indices, words hold parent + 1) ----------------------------------------------------------
__device__ inline int g_find(const int* L, int x) {
  for (;;) {
    const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
    if (p >= x || p < 0) return x;
    x = p;
  }
}
__device__ inline void g_union(int* L, int a, int b) {
  for (;;) {
    a = g_find(L, a);
    b = g_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b + 1) - 1;
    if (old >= a) return;
    a = old;
  }
}

// ---- phase 1 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_tile_kernel(int H, int W, const uint8_t* __restrict__ mask, int conn8, int* __restrict__ labels) {
  __shared__ int s_par[CC_TPX];
  __shared__ uint8_t s_cls[CC_TPX];
  const int r0 = blockIdx.y * CC_TH, c0 = blockIdx.x * CC_TW;
  const size_t base = (size_t)blockIdx.z * H * W;
#pragma unroll
  for (int k = 0; k < CC_TPX / 256; ++k) {
    const int i = threadIdx.x + k * 256, r = r0 + i / CC_TW, c = c0 + i % CC_TW;
    s_cls[i] = (r < H && c < W) ? (uint8_t)cc_class(mask[base + (size_t)r * W + c]) : (uint8_t)0;
    s_par[i] = i;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_TPX / 256; ++k) {
    const int i = threadIdx.x + k * 256, lr = i / CC_TW, lc = i % CC_TW;
    const int cl = s_cls[i];
    if (cl == 0) continue;
    if (lc > 0 && s_cls[i - 1] == cl) lds_union(s_par, i, i - 1);
    if (lr > 0) {
      if (s_cls[i - CC_TW] == cl) {
        lds_union(s_par, i, i - CC_TW);           // (8-connectivity: the upper diagonals touch that pixel, nothing more to unite)
      } else if (conn8) {
        if (lc > 0 && s_cls[i - CC_TW - 1] == cl) lds_union(s_par, i, i - CC_TW - 1);
        if (lc < CC_TW - 1 && s_cls[i - CC_TW + 1] == cl) lds_union(s_par, i, i - CC_TW + 1);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_TPX / 256; ++k) {
    const int i = threadIdx.x + k * 256, r = r0 + i / CC_TW, c = c0 + i % CC_TW;
    if (r >= H || c >= W) continue;
    int v = 0;
    if (s_cls[i] != 0) {
      const int root = lds_find(s_par, i);        // the tile's row-major order is the image's: the local minimum is the global one
      v = (r0 + root / CC_TW) * W + (c0 + root % CC_TW) + 1;
    }
    labels[base + (size_t)r * W + c] = v;
  }
}

// ---- phase 2 ---------------------------------------------------------------------------------------------------------------------
// Work items of one sample: first the pixels of the rows that begin a tile row (all but the first), then the pixels of the columns that
// begin a tile column (all but the first) and, with wrap, of column 0, whose left neighbour is column W - 1.
__device__ inline void cc_link(int* L, const uint8_t* m, int W, int cl, int p, int r, int c) {
  const int q = r * W + c;
  if (cc_class(m[q]) == cl) g_union(L, p, q);
}
__global__ __launch_bounds__(256) void cc_merge_kernel(int H, int W, const uint8_t* __restrict__ mask, int conn8, int wrap, int* labels,
                                                       long n_row_items, long n_items) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_items) return;
  const size_t base = (size_t)blockIdx.y * H * W;
  const uint8_t* m = mask + base;
  int* L = labels + base;
  if (t < n_row_items) {
    const int r = ((int)(t / W) + 1) * CC_TH, c = (int)(t % W);
    const int p = r * W + c, cl = cc_class(m[p]);
    if (cl == 0) return;
    cc_link(L, m, W, cl, p, r - 1, c);
    if (conn8) {
      if (c > 0) cc_link(L, m, W, cl, p, r - 1, c - 1);
      else if (wrap) cc_link(L, m, W, cl, p, r - 1, W - 1);
      if (c < W - 1) cc_link(L, m, W, cl, p, r - 1, c + 1);
      else if (wrap) cc_link(L, m, W, cl, p, r - 1, 0);
    }
    return;
  }
  const long u = t - n_row_items;
  const int k = (int)(u / H), r = (int)(u % H);
  const int ncol = (W - 1) / CC_TW;               // interior column borders
  const int c = k < ncol ? (k + 1) * CC_TW : 0, cn = k < ncol ? c - 1 : W - 1;
  const int p = r * W + c, cl = cc_class(m[p]);
  if (cl == 0) return;
  cc_link(L, m, W, cl, p, r, cn);
  if (conn8) {
    if (r > 0) cc_link(L, m, W, cl, p, r - 1, cn);
    if (r < H - 1) cc_link(L, m, W, cl, p, r + 1, cn);
  }
}

// ---- phase 3 ---------------------------------------------------------------------------------------------------------------------
// Other threads' stores of this launch replace a word by its root's, an ancestor as well (I2): whichever a walk reads, it ends at the root.
__global__ __launch_bounds__(256) void cc_flatten_kernel(long HW, int* labels) {
  int* L = labels + (size_t)blockIdx.y * HW;
  const long stride = (long)gridDim.x * 256;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += stride) {
    const int v = L[p];
    if (v <= 0 || v == (int)p + 1) continue;
    const int root = g_find(L, v - 1);
    if (root + 1 != v) L[p] = root + 1;
  }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------
// exclusive prefix sum of v over the 256 threads; *total: the sum.  s_w: four words of LDS, free again when the call returns.
// T: int, or long long where the sum can pass 2^31 (the step rows of dc_track_cycles)
template <typename T>
__device__ inline T block_excl_scan(T v, T* s_w, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T n = __shfl_up(incl, o, 64);
    if (lane >= o) incl += n;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const T w = s_w[k];
    if (k < wave) before += w;
    all += w;
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// roots (total, class 1) of every chunk of CC_CHUNK consecutive pixels
__global__ __launch_bounds__(256) void cc_count_kernel(long HW, const uint8_t* __restrict__ mask, const int* __restrict__ labels, long nchunk,
                                                       int* __restrict__ chunk_cnt) {
  __shared__ int s_w[4];
  const size_t base = (size_t)blockIdx.y * HW;
  const long p = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
  const bool root = p < HW && labels[base + p] == (int)p + 1;
  const bool one = root && mask[base + p] == 1;
  int tot, tot1;
  block_excl_scan(root ? 1 : 0, s_w, &tot);
  block_excl_scan(one ? 1 : 0, s_w, &tot1);
  if (threadIdx.x == 0) {
    int* o = chunk_cnt + ((size_t)blockIdx.y * nchunk + blockIdx.x) * 2;
    o[0] = tot;
    o[1] = tot1;
  }
}

// one workgroup per sample: the chunks' counts become exclusive offsets, the sums go to ncomp
__global__ __launch_bounds__(256) void cc_offsets_kernel(long nchunk, const int* __restrict__ chunk_cnt, int* __restrict__ chunk_off,
                                                         int* __restrict__ ncomp) {
  __shared__ int s_w[4];
  const int* cnt = chunk_cnt + (size_t)blockIdx.x * nchunk * 2;
  int* off = chunk_off + (size_t)blockIdx.x * nchunk;
  int carry = 0, carry1 = 0;
  for (long k0 = 0; k0 < nchunk; k0 += 256) {     // uniform trip count: every thread reaches the barriers inside the scans
    const long k = k0 + threadIdx.x;
    const int v = k < nchunk ? cnt[2 * k] : 0, v1 = k < nchunk ? cnt[2 * k + 1] : 0;
    int tot, tot1;
    const int ex = block_excl_scan(v, s_w, &tot);
    block_excl_scan(v1, s_w, &tot1);
    if (k < nchunk) off[k] = carry + ex;
    carry += tot;
    carry1 += tot1;
  }
  if (threadIdx.x == 0) {
    ncomp[blockIdx.x * 3 + 0] = carry;
    ncomp[blockIdx.x * 3 + 1] = carry1;
    ncomp[blockIdx.x * 3 + 2] = carry - carry1;
  }
}

// every root learns its rank (kept in rank_map at the root's pixel) and opens its row: root, class, first row
__global__ __launch_bounds__(256) void cc_rank_kernel(long HW, int W, const uint8_t* __restrict__ mask, const int* __restrict__ labels, long nchunk,
                                                      const int* __restrict__ chunk_off, int cap, int* __restrict__ rank_map,
                                                      long long* __restrict__ table) {
  __shared__ int s_w[4];
  const size_t base = (size_t)blockIdx.y * HW;
  const long p = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
  const bool root = p < HW && labels[base + p] == (int)p + 1;
  int tot;
  const int ex = block_excl_scan(root ? 1 : 0, s_w, &tot);
  if (!root) return;
  const int rank = chunk_off[(size_t)blockIdx.y * nchunk + blockIdx.x] + ex;
  rank_map[base + p] = rank;
  if (rank < cap) {
    long long* row = table + ((size_t)blockIdx.y * cap + rank) * CC_FIELDS;
    row[0] = p;
    row[1] = mask[base + p];
    row[7] = p / W;                               // the root is the component's first pixel in row-major order: its row is the smallest
  }
}

struct CcPart {                                   // one thread's run of pixels of one component inside one row
  int root, n, seam;
  long long scx, ssx;
};

__device__ inline void cc_emit(const int* __restrict__ rank_sample, long HW, int cap, long long* table_sample, int root, long long n,
                               long long area, long long sr, long long scx, long long ssx, int rmax, int seam) {
  if (root < 0 || root >= HW) return;
  const int rank = rank_sample[root];
  if (rank < 0 || rank >= cap) return;            // beyond the table: counted in ncomp only
  unsigned long long* row = (unsigned long long*)(table_sample + (size_t)rank * CC_FIELDS);
  atomicAdd(row + 2, (unsigned long long)n);
  atomicAdd(row + 3, (unsigned long long)area);
  atomicAdd(row + 4, (unsigned long long)sr);
  atomicAdd(row + 5, (unsigned long long)scx);
  atomicAdd(row + 6, (unsigned long long)ssx);
  atomicMax(row + 8, (unsigned long long)rmax);
  if (seam) atomicOr(row + 9, (unsigned long long)seam);
}

// One workgroup per tile; a thread walks 8 consecutive pixels of a row and hands each run of one component to the workgroup's table in LDS
// (most pixels of a tile share one or two roots); runs that find no slot within CC_PROBES go to the global row directly.  Field 9 collects
// bit 0 (a pixel in column 0) and bit 1 (a pixel in column W - 1) here; cc_seam_kernel turns it into the flag.
__global__ __launch_bounds__(256) void cc_accumulate_kernel(int H, int W, const int* __restrict__ labels, const int* __restrict__ wy,
                                                            const int* __restrict__ cx, const int* __restrict__ sx, int cap,
                                                            const int* __restrict__ rank_map, long long* __restrict__ table) {
  __shared__ int s_key[CC_SLOTS];
  __shared__ unsigned long long s_sum[CC_SLOTS][5];
  __shared__ int s_rmax[CC_SLOTS], s_seam[CC_SLOTS];
  const long HW = (long)H * W;
  const size_t base = (size_t)blockIdx.z * HW;
  const int* rank_sample = rank_map + base;
  long long* table_sample = table + (size_t)blockIdx.z * cap * CC_FIELDS;
  if (threadIdx.x < CC_SLOTS) {
    const int s = threadIdx.x;
    s_key[s] = -1;
    s_rmax[s] = 0;
    s_seam[s] = 0;
#pragma unroll
    for (int f = 0; f < 5; ++f) s_sum[s][f] = 0ull;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.y * CC_TH + wave * 8 + lane / 8, cb = blockIdx.x * CC_TW + (lane % 8) * 8;
  if (r < H) {
    const int wr = wy[r];
    CcPart a;
    a.root = -1;
    for (int j = 0; j <= 8; ++j) {
      const int c = cb + j;
      const int v = (j < 8 && c < W) ? labels[base + (size_t)r * W + c] : 0;
      const int root = v - 1;                     // -1: background, the row's end, the run's end
      if (root != a.root) {
        if (a.root >= 0) {
          int s = (int)(((unsigned)a.root * 2654435761u) >> 25), hit = -1;
#pragma unroll
          for (int t = 0; t < CC_PROBES && hit < 0; ++t) {
            const int old = atomicCAS(&s_key[s], -1, a.root);
            if (old == -1 || old == a.root) hit = s;
            s = (s + 1) & (CC_SLOTS - 1);
          }
          if (hit >= 0) {
            atomicAdd(&s_sum[hit][0], (unsigned long long)a.n);
            atomicAdd(&s_sum[hit][1], (unsigned long long)((long long)a.n * wr));
            atomicAdd(&s_sum[hit][2], (unsigned long long)((long long)a.n * r));
            atomicAdd(&s_sum[hit][3], (unsigned long long)a.scx);
            atomicAdd(&s_sum[hit][4], (unsigned long long)a.ssx);
            atomicMax(&s_rmax[hit], r);
            if (a.seam) atomicOr(&s_seam[hit], a.seam);
          } else {
            cc_emit(rank_sample, HW, cap, table_sample, a.root, a.n, (long long)a.n * wr, (long long)a.n * r, a.scx, a.ssx, r, a.seam);
          }
        }
        a.root = root;
        a.n = 0;
        a.seam = 0;
        a.scx = a.ssx = 0;
      }
      if (root >= 0) {
        a.n += 1;
        a.scx += cx[c];
        a.ssx += sx[c];
        a.seam |= (c == 0 ? 1 : 0) | (c == W - 1 ? 2 : 0);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < CC_SLOTS && s_key[threadIdx.x] >= 0) {
    const int s = threadIdx.x;
    cc_emit(rank_sample, HW, cap, table_sample, s_key[s], (long long)s_sum[s][0], (long long)s_sum[s][1], (long long)s_sum[s][2],
            (long long)s_sum[s][3], (long long)s_sum[s][4], s_rmax[s], s_seam[s]);
  }
}

__global__ __launch_bounds__(256) void cc_seam_kernel(int cap, long long* __restrict__ table) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cap) return;
  long long* row = table + ((size_t)blockIdx.y * cap + k) * CC_FIELDS;
  const long long bits = row[9];
  if (bits != 0) row[9] = bits == 3 ? 1 : 0;
}

static inline size_t cc_align(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace dc

using namespace dc;

extern "C" int dc_mask_components_tile(int* th, int* tw) {
  DC_REQUIRE(th && tw, "dc_mask_components_tile: null argument");
  *th = CC_TH;
  *tw = CC_TW;
  return 0;
}

// the workspace: rank_map int32 [B][HW] | chunk_cnt int32 [B][nchunk][2] | chunk_off int32 [B][nchunk]
extern "C" size_t dc_mask_components_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const size_t HW = (size_t)H * W, nchunk = (HW + CC_CHUNK - 1) / CC_CHUNK;
  return cc_align((size_t)B * HW * 4) + cc_align((size_t)B * nchunk * 8) + cc_align((size_t)B * nchunk * 4);
}

static int cc_check(int B, int n_valid, int H, int W) {
  DC_REQUIRE(B > 0 && H > 0 && W > 0, "components: B, H and W must be positive");
  DC_REQUIRE(n_valid > 0 && n_valid <= B, "components: n_valid must lie in [1, B]");
  DC_REQUIRE(n_valid <= 65535, "components: at most 65535 samples per call");
  DC_REQUIRE((long)H * W < 2147483647L, "components: H * W must be below 2^31 - 1 (labels are int32)");
  DC_REQUIRE((H + CC_TH - 1) / CC_TH <= 65535, "components: H exceeds 65535 tile rows");
  return 0;
}

extern "C" int dc_mask_components(int B, int n_valid, int H, int W, const uint8_t* mask, int connectivity, int wrap, int32_t* labels,
                                  void* workspace, void* stream) {
  DC_REQUIRE(connectivity == 4 || connectivity == 8, "dc_mask_components: connectivity must be 4 or 8");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_mask_components: wrap must be 0 or 1");
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(mask && labels, "dc_mask_components: null pointer");
  (void)workspace;                                // the forest lives in the label map itself
  hipStream_t st = (hipStream_t)stream;
  const int conn8 = connectivity == 8;
  const int tx = (W + CC_TW - 1) / CC_TW, ty = (H + CC_TH - 1) / CC_TH;
  hipLaunchKernelGGL(cc_tile_kernel, dim3(tx, ty, n_valid), dim3(256), 0, st, H, W, mask, conn8, labels);
  DC_LAUNCHED("cc_tile");
  const long n_row_items = (long)(ty - 1) * W, n_items = n_row_items + (long)(tx - 1 + (wrap ? 1 : 0)) * H;
  if (n_items > 0) {
    hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)((n_items + 255) / 256), n_valid), dim3(256), 0, st, H, W, mask, conn8, wrap, labels,
                       n_row_items, n_items);
    DC_LAUNCHED("cc_merge");
  }
  const long HW = (long)H * W;
  long blocks = (HW + 255) / 256;
  const long share = (4096 + n_valid - 1) / n_valid;
  if (blocks > share) blocks = share;
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)blocks, n_valid), dim3(256), 0, st, HW, labels);
  DC_LAUNCHED("cc_flatten");
  return 0;
}

extern "C" int dc_component_stats(int B, int n_valid, int H, int W, const uint8_t* mask, const int32_t* labels, const int32_t* wy,
                                  const int32_t* cx, const int32_t* sx, int cap, int64_t* table, int32_t* ncomp, void* workspace,
                                  void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(cap >= 1, "dc_component_stats: cap must be at least 1");
  DC_REQUIRE(mask && labels && wy && cx && sx && table && ncomp && workspace, "dc_component_stats: null pointer");
  DC_REQUIRE(((uintptr_t)workspace & 3) == 0, "dc_component_stats: workspace not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long HW = (long)H * W, nchunk = (HW + CC_CHUNK - 1) / CC_CHUNK;
  char* ws = (char*)workspace;
  int* rank_map = (int*)ws;
  int* chunk_cnt = (int*)(ws + cc_align((size_t)B * HW * 4));
  int* chunk_off = (int*)((char*)chunk_cnt + cc_align((size_t)B * nchunk * 8));
  hipError_t e = hipMemsetAsync(table, 0, (size_t)B * cap * CC_FIELDS * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)nchunk, n_valid), dim3(256), 0, st, HW, mask, labels, nchunk, chunk_cnt);
  DC_LAUNCHED("cc_stats");
  hipLaunchKernelGGL(cc_offsets_kernel, dim3(n_valid), dim3(256), 0, st, nchunk, chunk_cnt, chunk_off, ncomp);
  DC_LAUNCHED("cc_stats");
  hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)nchunk, n_valid), dim3(256), 0, st, HW, W, mask, labels, nchunk, chunk_off, cap, rank_map,
                     (long long*)table);
  DC_LAUNCHED("cc_stats");
  const int tx = (W + CC_TW - 1) / CC_TW, ty = (H + CC_TH - 1) / CC_TH;
  hipLaunchKernelGGL(cc_accumulate_kernel, dim3(tx, ty, n_valid), dim3(256), 0, st, H, W, labels, wy, cx, sx, cap, rank_map, (long long*)table);
  DC_LAUNCHED("cc_stats");
  hipLaunchKernelGGL(cc_seam_kernel, dim3((cap + 255) / 256, n_valid), dim3(256), 0, st, cap, (long long*)table);
  DC_LAUNCHED("cc_stats");
  return 0;
}

// ---- event shapes and the shape filter (dc_component_shape, dc_event_select, dc_mask_select; nn.EventShape, nn.EventFilter) -----------
// One row of twelve int64 words per event rank (include/deepcam_hip.h has the definition): boundary pixels, the two face counts, and the
// 2^40-scaled first and second moments of the event's pixels as weighted unit vectors on the sphere.  Every per-pixel term is an integer
// below 2^40 in magnitude and H * W <= 2^22, so every sum fits an int64, is exact and does not depend on the order of arrival.
//   sh_pixel   one workgroup per tile, a thread walks 8 consecutive pixels of a row as in cc_accumulate.  The tile's label words and a halo of one pixel (the rows above
//              and below, the columns left and right, the seam's other side under wrap, 0 off the grid) are staged in LDS once, so that
//              the four face tests of a pixel read LDS; a thread reduces each run of one root in registers (n, five column sums, three
//              face counts), multiplies the row's factors in once per run and hands the twelve terms to the workgroup's table in LDS,
//              keyed by root.  Runs that find no slot within SH_PROBES go to the global row directly; filled slots are flushed at the end.
//   sh_select  one thread per event row: the decode formula in fp64, the keep flag, the events kept and dropped per class
//   sh_mask    one streaming pass: the filtered mask and the pixels kept and dropped per class (one atomic per workgroup and counter)
// 64-bit integer atomics only; no workgroup waits for another.
namespace dc {

static constexpr int SH_FIELDS = 12;
static constexpr int SH_SLOTS = 128;              // per-workgroup table of partial sums: 12 KiB of LDS
static constexpr int SH_PROBES = 4;
static constexpr int SH_LH = CC_TH + 2, SH_LW = CC_TW + 2;
static constexpr int SH_STRIDE = 67;              // words per staged row, odd: a 4-byte LDS read is served in two groups of 32 lanes over 32
                                                  // banks; a group is 8 rows x 4 column groups of 8 words (sh_pixel_kernel's lane layout), its
                                                  // banks 3 row + 8 group (mod 32) are all different at every step of the walk
static constexpr int SH_ROW_TABLES = 6, SH_COL_TABLES = 5;
static constexpr int SH_COUNTS = 8;               // per class: events kept, events dropped, pixels kept, pixels dropped

struct ShRun {                                    // one thread's run of pixels of one component inside one row; the column sums of at most
  int root, n, nb, fv, fh;                        // 8 entries of 2^20 each stay below 2^23
  int scx, ssx, sxx, sxy, syy;
};
struct ShRow {                                    // the row's factors: wy, rc2, rcs, rc3, rc2s, rcs2
  int wy, c2, cs, c3, c2s, cs2;
};

__device__ inline void sh_terms(const ShRun& a, const ShRow& w, long long* t) {
  const long long n20 = (long long)a.n * (1ll << 20);
  t[0] = a.nb;
  t[1] = a.fv;
  t[2] = (long long)a.fh * w.wy;
  t[3] = (long long)w.c2 * a.scx;
  t[4] = (long long)w.c2 * a.ssx;
  t[5] = (long long)w.cs * n20;
  t[6] = (long long)w.c3 * a.sxx;
  t[7] = (long long)w.c3 * a.sxy;
  t[8] = (long long)w.c3 * a.syy;
  t[9] = (long long)w.c2s * a.scx;
  t[10] = (long long)w.c2s * a.ssx;
  t[11] = (long long)w.cs2 * n20;
}

__device__ inline void sh_emit(const int* __restrict__ rank_sample, long HW, int cap, long long* shape_sample, int root, const long long* t) {
  if (root < 0 || root >= HW) return;
  const int rank = rank_sample[root];
  if (rank < 0 || rank >= cap) return;            // beyond the table: no row
  unsigned long long* row = (unsigned long long*)(shape_sample + (size_t)rank * SH_FIELDS);
#pragma unroll
  for (int f = 0; f < SH_FIELDS; ++f)
    if (t[f] != 0) atomicAdd(row + f, (unsigned long long)t[f]);
}

__global__ __launch_bounds__(256) void sh_pixel_kernel(int H, int W, int wrap, const int* __restrict__ labels, const int* __restrict__ rowt,
                                                       const int* __restrict__ colt, int cap, const int* __restrict__ rank_map,
                                                       long long* __restrict__ shape) {
  __shared__ int s_lab[SH_LH * SH_STRIDE];
  __shared__ int s_key[SH_SLOTS];
  __shared__ unsigned long long s_sum[SH_SLOTS][SH_FIELDS];
  const long HW = (long)H * W;
  const size_t base = (size_t)blockIdx.z * HW;
  const int* L = labels + base;
  const int* rank_sample = rank_map + base;
  long long* shape_sample = shape + (size_t)blockIdx.z * cap * SH_FIELDS;
  const int r0 = blockIdx.y * CC_TH, c0 = blockIdx.x * CC_TW;
  if (threadIdx.x < SH_SLOTS) {
    const int s = threadIdx.x;
    s_key[s] = -1;
#pragma unroll
    for (int f = 0; f < SH_FIELDS; ++f) s_sum[s][f] = 0ull;
  }
  // the tile and its halo: rows r0 - 1 .. r0 + TH, columns c0 - 1 .. c0 + TW; 0 where there is no pixel
  for (int i = threadIdx.x; i < SH_LH * SH_LW; i += 256) {
    const int lr = i / SH_LW, lc = i % SH_LW;
    const int gr = r0 - 1 + lr;
    int gc = c0 - 1 + lc;
    if (wrap) gc = gc < 0 ? W - 1 : (gc == W ? 0 : gc);
    int v = 0;
    if (gr >= 0 && gr < H && gc >= 0 && gc < W) v = L[(size_t)gr * W + gc];
    s_lab[lr * SH_STRIDE + lc] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = wave * 8 + (lane & 7), lcb = (lane >> 3) * 8;        // lanes 0 - 31: 8 rows x the first 4 column groups (SH_STRIDE)
  const int r = r0 + lr, cb = c0 + lcb;
  if (r < H) {
    ShRow w;
    w.wy = rowt[r];
    w.c2 = rowt[H + r];
    w.cs = rowt[2 * H + r];
    w.c3 = rowt[3 * H + r];
    w.c2s = rowt[4 * H + r];
    w.cs2 = rowt[5 * H + r];
    const int* mid = s_lab + (lr + 1) * SH_STRIDE + lcb + 1;          // the thread's first pixel
    ShRun a;
    a.root = -1;
    for (int j = 0; j <= 8; ++j) {
      const int c = cb + j;
      const int v = (j < 8 && c < W) ? mid[j] : 0;                    // (column W holds column 0's word under wrap: not a pixel)
      const int root = v - 1;                     // -1: background, the row's end, the run's end
      if (root != a.root) {
        if (a.root >= 0) {
          long long t[SH_FIELDS];
          sh_terms(a, w, t);
          int s = (int)(((unsigned)a.root * 2654435761u) >> 25), hit = -1;
#pragma unroll
          for (int p = 0; p < SH_PROBES && hit < 0; ++p) {
            const int old = atomicCAS(&s_key[s], -1, a.root);
            if (old == -1 || old == a.root) hit = s;
            s = (s + 1) & (SH_SLOTS - 1);
          }
          if (hit >= 0) {
#pragma unroll
            for (int f = 0; f < SH_FIELDS; ++f)
              if (t[f] != 0) atomicAdd(&s_sum[hit][f], (unsigned long long)t[f]);
          } else {
            sh_emit(rank_sample, HW, cap, shape_sample, a.root, t);
          }
        }
        a.root = root;
        a.n = a.nb = a.fv = a.fh = 0;
        a.scx = a.ssx = a.sxx = a.sxy = a.syy = 0;
      }
      if (root >= 0) {
        const int up = mid[j - SH_STRIDE] != v, dn = mid[j + SH_STRIDE] != v, lf = mid[j - 1] != v, rt = mid[j + 1] != v;
        a.n += 1;
        a.nb += up | dn | lf | rt;
        a.fv += lf + rt;
        a.fh += up + dn;
        a.scx += colt[c];
        a.ssx += colt[W + c];
        a.sxx += colt[2 * W + c];
        a.sxy += colt[3 * W + c];
        a.syy += colt[4 * W + c];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < SH_SLOTS && s_key[threadIdx.x] >= 0) {
    const int s = threadIdx.x;
    long long t[SH_FIELDS];
#pragma unroll
    for (int f = 0; f < SH_FIELDS; ++f) t[f] = (long long)s_sum[s][f];
    sh_emit(rank_sample, HW, cap, shape_sample, s_key[s], t);
  }
}
static_assert(SH_SLOTS == 128, "sh_pixel_kernel: the slot index is the hash's top 7 bits");
static_assert(SH_STRIDE >= SH_LW, "sh_pixel_kernel: a staged row holds the tile's columns and the halo");

// lambda+ and lambda- of one event (the decode formula of include/deepcam_hip.h); false when the zeroth moment is 0
__device__ inline bool sh_lambda(long long area, const long long* __restrict__ s, double* lp, double* lm) {
  *lp = *lm = 0.0;
  if (area <= 0) return false;
  const double s0 = (double)area * 0x1p20;
  const double mx = (double)s[3] / s0, my = (double)s[4] / s0, mz = (double)s[5] / s0;
  const double cxx = (double)s[6] / s0 - mx * mx, cxy = (double)s[7] / s0 - mx * my, cyy = (double)s[8] / s0 - my * my;
  const double cxz = (double)s[9] / s0 - mx * mz, cyz = (double)s[10] / s0 - my * mz, czz = (double)s[11] / s0 - mz * mz;
  const double norm = sqrt(mx * mx + my * my + mz * mz);
  double ux = 1.0, uy = 0.0, uz = 0.0;            // the centroid's direction; (1, 0, 0) when the first moment vanishes
  if (norm > 0.0) {
    ux = mx / norm;
    uy = my / norm;
    uz = mz / norm;
  }
  const double h = sqrt(ux * ux + uy * uy);       // cos lat; sin lat = uz; (cos lon, sin lon) = (ux, uy) / h, (1, 0) at a pole
  const double co = h > 0.0 ? ux / h : 1.0, so = h > 0.0 ? uy / h : 0.0;
  const double ex = -so, ey = co;                                     // east
  const double nx = -uz * co, ny = -uz * so, nz = h;                  // north
  const double qx = cxx * nx + cxy * ny + cxz * nz, qy = cxy * nx + cyy * ny + cyz * nz, qz = cxz * nx + cyz * ny + czz * nz;   // C n
  const double a = ex * (cxx * ex + cxy * ey) + ey * (cxy * ex + cyy * ey);
  const double b = ex * qx + ey * qy;
  const double d = nx * qx + ny * qy + nz * qz;
  const double mid = 0.5 * (a + d), half = 0.5 * (a - d), rad = sqrt(half * half + b * b);
  *lp = fmax(mid + rad, 0.0);
  *lm = fmax(mid - rad, 0.0);
  return true;
}

struct ShCriteria {                               // one class's row of `criteria`
  long long min_pixels, min_area;
  double min_len2, min_aspect2;
};

__global__ __launch_bounds__(256) void sh_select_kernel(int cap, const long long* __restrict__ table, const int* __restrict__ ncomp,
                                                        const long long* __restrict__ shape, const ShCriteria* __restrict__ criteria,
                                                        uint8_t* __restrict__ keep, unsigned long long* counts) {
  __shared__ unsigned s_n[4];                     // class 1: kept, dropped; class 2: kept, dropped
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0u;
  __syncthreads();
  int rows = ncomp[b * 3];
  rows = rows < 0 ? 0 : (rows > cap ? cap : rows);
  if (k < cap) {
    int kept = 0;
    if (k < rows) {
      const long long* row = table + ((size_t)b * cap + k) * CC_FIELDS;
      const long long cls = row[1], px = row[2], area = row[3];
      if (cls == 1 || cls == 2) {
        const ShCriteria cr = criteria[cls - 1];
        kept = 1;
        if (cr.min_pixels > 0 && px < cr.min_pixels) kept = 0;
        if (cr.min_area > 0 && area < cr.min_area) kept = 0;
        if (cr.min_len2 > 0.0 || cr.min_aspect2 > 0.0) {
          double lp, lm;
          const bool ok = sh_lambda(area, shape + ((size_t)b * cap + k) * SH_FIELDS, &lp, &lm);
          if (cr.min_len2 > 0.0 && !(ok && 12.0 * lp >= cr.min_len2)) kept = 0;
          if (cr.min_aspect2 > 0.0 && !(ok && lp >= cr.min_aspect2 * lm)) kept = 0;
        }
        atomicAdd(&s_n[(cls == 2 ? 2 : 0) + (kept ? 0 : 1)], 1u);
      }
    }
    keep[(size_t)b * cap + k] = (uint8_t)kept;
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_n[threadIdx.x])
    atomicAdd(counts + (size_t)b * SH_COUNTS + (threadIdx.x >> 1) * 4 + (threadIdx.x & 1), (unsigned long long)s_n[threadIdx.x]);
}

// the class a pixel keeps, and its count: v[0..3] = class 1 kept, dropped; class 2 kept, dropped
__device__ inline uint8_t sh_pixel(uint8_t m, int label, long HW, const int* __restrict__ rank_sample, int cap,
                                   const uint8_t* __restrict__ keep_sample, unsigned* v) {
  if (m != 1 && m != 2) return m;                 // background and values >= 3 pass through
  bool kept = true;                               // no row, no criterion: the pixel stays
  const int root = label - 1;
  if (root >= 0 && root < HW) {
    const int rank = rank_sample[root];
    if (rank >= 0 && rank < cap) kept = keep_sample[rank] != 0;
  }
  const int f = (m == 2 ? 2 : 0) + (kept ? 0 : 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] += f == i ? 1u : 0u;   // (constant indices: the four counters stay in registers)
  return kept ? m : (uint8_t)0;
}

// SH_MASK_PX pixels per thread: one 4-byte load of the mask, one 16-byte load of the labels, one 4-byte store when `vec` (HW a multiple of
// 4 and the three bases aligned); single bytes and words otherwise
static constexpr int SH_MASK_PX = 4;
__global__ __launch_bounds__(256) void sh_mask_kernel(long HW, int vec, const uint8_t* __restrict__ mask, const int* __restrict__ labels,
                                                      const int* __restrict__ rank_map, int cap, const uint8_t* __restrict__ keep,
                                                      uint8_t* __restrict__ out_mask, unsigned long long* counts) {
  __shared__ unsigned s_n[4];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * HW;
  const int* rank_sample = rank_map + base;
  const uint8_t* keep_sample = keep + (size_t)b * cap;
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0u;
  __syncthreads();
  unsigned v[4] = {0u, 0u, 0u, 0u};
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * SH_MASK_PX;
  if (vec && p0 + SH_MASK_PX <= HW) {
    const uchar4 m = *(const uchar4*)(mask + base + p0);
    const int4 l = *(const int4*)(labels + base + p0);
    uchar4 o;
    o.x = sh_pixel(m.x, l.x, HW, rank_sample, cap, keep_sample, v);
    o.y = sh_pixel(m.y, l.y, HW, rank_sample, cap, keep_sample, v);
    o.z = sh_pixel(m.z, l.z, HW, rank_sample, cap, keep_sample, v);
    o.w = sh_pixel(m.w, l.w, HW, rank_sample, cap, keep_sample, v);
    *(uchar4*)(out_mask + base + p0) = o;
  } else {
    for (int j = 0; j < SH_MASK_PX; ++j) {
      const long p = p0 + j;
      if (p < HW) out_mask[base + p] = sh_pixel(mask[base + p], labels[base + p], HW, rank_sample, cap, keep_sample, v);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned x = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(&s_n[i], x);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_n[threadIdx.x])
    atomicAdd(counts + (size_t)b * SH_COUNTS + (threadIdx.x >> 1) * 4 + 2 + (threadIdx.x & 1), (unsigned long long)s_n[threadIdx.x]);
}

}  // namespace dc

extern "C" int dc_component_shape(int B, int n_valid, int H, int W, const int32_t* labels, const int32_t* rank_map, int cap, int wrap,
                                  const int32_t* row_tables, const int32_t* col_tables, int64_t* shape, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE((long)H * W <= (1L << 22), "dc_component_shape: H * W must be at most 2^22 (the sums stay inside int64)");
  DC_REQUIRE(cap >= 1, "dc_component_shape: cap must be at least 1");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_component_shape: wrap must be 0 or 1");
  DC_REQUIRE(labels && rank_map && row_tables && col_tables && shape, "dc_component_shape: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(shape, 0, (size_t)n_valid * cap * SH_FIELDS * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const int tx = (W + CC_TW - 1) / CC_TW, ty = (H + CC_TH - 1) / CC_TH;
  hipLaunchKernelGGL(sh_pixel_kernel, dim3(tx, ty, n_valid), dim3(256), 0, st, H, W, wrap, labels, row_tables, col_tables, cap, rank_map,
                     (long long*)shape);
  DC_LAUNCHED("cc_shape");
  return 0;
}

extern "C" int dc_event_select(int B, int n_valid, int cap, const int64_t* table, const int32_t* ncomp, const int64_t* shape,
                               const void* criteria, uint8_t* keep, int64_t* counts, void* stream) {
  DC_REQUIRE(B > 0 && n_valid > 0 && n_valid <= B && n_valid <= 65535, "dc_event_select: n_valid must lie in [1, min(B, 65535)]");
  DC_REQUIRE(cap >= 1, "dc_event_select: cap must be at least 1");
  DC_REQUIRE(table && ncomp && shape && criteria && keep && counts, "dc_event_select: null pointer");
  DC_REQUIRE(((uintptr_t)criteria & 7) == 0, "dc_event_select: criteria not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_valid * SH_COUNTS * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  hipLaunchKernelGGL(sh_select_kernel, dim3((cap + 255) / 256, n_valid), dim3(256), 0, st, cap, (const long long*)table, ncomp,
                     (const long long*)shape, (const ShCriteria*)criteria, keep, (unsigned long long*)counts);
  DC_LAUNCHED("cc_shape");
  return 0;
}

extern "C" int dc_mask_select(int B, int n_valid, int H, int W, const uint8_t* mask, const int32_t* labels, const int32_t* rank_map, int cap,
                              const uint8_t* keep, uint8_t* out_mask, int64_t* counts, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(cap >= 1, "dc_mask_select: cap must be at least 1");
  DC_REQUIRE(mask && labels && rank_map && keep && out_mask && counts, "dc_mask_select: null pointer");
  const size_t bytes = (size_t)B * H * W;
  DC_REQUIRE((uintptr_t)out_mask + bytes <= (uintptr_t)mask || (uintptr_t)mask + bytes <= (uintptr_t)out_mask,
             "dc_mask_select: out_mask may not alias mask");
  const long HW = (long)H * W;
  const int vec = HW % 4 == 0 && ((uintptr_t)mask & 3) == 0 && ((uintptr_t)out_mask & 3) == 0 && ((uintptr_t)labels & 15) == 0;
  const long blocks = (HW + 256 * SH_MASK_PX - 1) / (256 * SH_MASK_PX);
  hipLaunchKernelGGL(sh_mask_kernel, dim3((unsigned)blocks, n_valid), dim3(256), 0, (hipStream_t)stream, HW, vec, mask, labels, rank_map, cap,
                     keep, out_mask, (unsigned long long*)counts);
  DC_LAUNCHED("cc_shape");
  return 0;
}

// ---- overlap of two catalogues (dc_component_overlap, dc_event_scores; nn.EventMatcher) -----------------------------------------------
// Two catalogues of the same frames, a and b: which component of a shares pixels with which of b, and how many; per component, how many
// of its pixels the other mask covers with the same class.  Nothing here says which side is a prediction: tracking links the catalogues
// of two time steps through the same pass.
//   ov_pixel    one workgroup per tile, a thread walks 8 consecutive pixels of a row as cc_accumulate does; a run of one (root a, root b)
//               pair goes to the workgroup's table in LDS, keyed by the two roots and the "same class" bit (one fact per pair: a component
//               has one class).  Runs that find no slot within OV_PROBES, and at the end the LDS slots, go to ov_emit: the two rank
//               lookups, the coverage adds, and the pair's count into the sample's open-addressing table in the workspace.
//               The thread whose compare-and-swap opens a slot draws a ticket from the sample's counter and, while tickets are below
//               pair_cap, notes the slot under it.
//   ov_compact  one thread per ticket writes its slot as a row; the counter gives the rows stored and the overflow flag
//   ov_scores   one workgroup per sample counts hits, misses, false alarms and matched detections and adds them to the running sums
// The global table has at least 2 * pair_cap slots and a key is probed through ALL of them before it is given up: with at most pair_cap
// distinct pairs every one finds a slot, whatever the order of arrival.  A key that was refused once is refused for ever (slots never
// empty again), so a pair is stored with all of its pixels or not at all; refusals happen only when every slot is taken, which is more
// than pair_cap pairs and raises the flag.  Integer atomics only; no workgroup waits for another.
namespace dc {

static constexpr int OV_SLOTS = 256;              // per-workgroup table of pair counts: 3 KiB of LDS, one slot per thread at the flush
static constexpr int OV_PROBES = 4;
static constexpr unsigned long long OV_EMPTY = ~0ull;
static constexpr int OV_SCORE_FIELDS = 8, OV_ACC_WORDS = 10;

static inline long ov_slots(int pair_cap) {       // a power of two, at least twice the rows
  long s = 16;
  while (s < 2L * pair_cap) s <<= 1;
  return s;
}

__device__ inline unsigned ov_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return (unsigned)k;
}

struct OvSample {                                 // one sample's slices
  const int *rank_a, *rank_b;
  unsigned long long *cover_a, *cover_b, *slots;  // slots: [nslots][2] = key (0: empty, else ((rank a << 32) | rank b) + 1), pixels
  unsigned* opened;                               // slots opened so far = distinct pairs in the table
  int* ticket_slot;                               // [pair_cap]: the slot the k-th opener took
  int cap_a, cap_b, pair_cap;
  unsigned slot_mask;
  long HW;
};

__device__ inline void ov_emit(const OvSample& S, int root_a, int root_b, int same, unsigned n) {
  if (root_a < 0 || root_a >= S.HW || root_b < 0 || root_b >= S.HW) return;
  const int ra = S.rank_a[root_a], rb = S.rank_b[root_b];
  const bool in_a = ra >= 0 && ra < S.cap_a, in_b = rb >= 0 && rb < S.cap_b;
  if (same) {                                     // whatever becomes of the pair: the other side's component may be beyond its table
    if (in_a) atomicAdd(S.cover_a + ra, (unsigned long long)n);
    if (in_b) atomicAdd(S.cover_b + rb, (unsigned long long)n);
  }
  if (!in_a || !in_b) return;
  const unsigned long long key = (((unsigned long long)ra << 32) | (unsigned)rb) + 1ull;
  unsigned h = ov_hash(key) & S.slot_mask;
  for (unsigned t = 0; t <= S.slot_mask; ++t) {
    unsigned long long* s = S.slots + 2 * (size_t)h;
    unsigned long long k = __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0ull) {
      k = atomicCAS(s, 0ull, key);
      if (k == 0ull) {
        k = key;
        const unsigned ticket = atomicAdd(S.opened, 1u);
        if (ticket < (unsigned)S.pair_cap) S.ticket_slot[ticket] = (int)h;
      }
    }
    if (k == key) {
      atomicAdd(s + 1, (unsigned long long)n);
      return;
    }
    h = (h + 1) & S.slot_mask;
  }
}

__global__ __launch_bounds__(256) void ov_pixel_kernel(int H, int W, const uint8_t* __restrict__ mask_a, const int* __restrict__ labels_a,
                                                       const int* __restrict__ rank_a, int cap_a, const uint8_t* __restrict__ mask_b,
                                                       const int* __restrict__ labels_b, const int* __restrict__ rank_b, int cap_b,
                                                       unsigned long long* cover_a, unsigned long long* cover_b, unsigned long long* slots,
                                                       long nslots, unsigned* opened, int* ticket_slot, int pair_cap) {
  __shared__ unsigned long long s_key[OV_SLOTS];
  __shared__ unsigned s_cnt[OV_SLOTS];
  OvSample S;
  S.HW = (long)H * W;
  const size_t base = (size_t)blockIdx.z * S.HW;
  S.rank_a = rank_a + base;
  S.rank_b = rank_b + base;
  S.cover_a = cover_a + (size_t)blockIdx.z * cap_a;
  S.cover_b = cover_b + (size_t)blockIdx.z * cap_b;
  S.slots = slots + (size_t)blockIdx.z * nslots * 2;
  S.opened = opened + blockIdx.z;
  S.ticket_slot = ticket_slot + (size_t)blockIdx.z * pair_cap;
  S.cap_a = cap_a;
  S.cap_b = cap_b;
  S.pair_cap = pair_cap;
  S.slot_mask = (unsigned)(nslots - 1);
  s_key[threadIdx.x] = OV_EMPTY;
  s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.y * CC_TH + wave * 8 + lane / 8, cb = blockIdx.x * CC_TW + (lane % 8) * 8;
  if (r < H) {
    unsigned long long key[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cb + j;
      key[j] = OV_EMPTY;
      if (c < W) {
        const size_t p = base + (size_t)r * W + c;
        const int la = labels_a[p], lb = labels_b[p];
        const int ca = cc_class(mask_a[p]), cl = cc_class(mask_b[p]);
        if (la > 0 && lb > 0)
          key[j] = ((unsigned long long)(ca != 0 && ca == cl) << 62) | ((unsigned long long)(la - 1) << 31) | (unsigned long long)(lb - 1);
      }
    }
    unsigned long long cur = OV_EMPTY;
    unsigned n = 0;
#pragma unroll
    for (int j = 0; j <= 8; ++j) {
      const unsigned long long k = j < 8 ? key[j] : OV_EMPTY;   // the row's end closes the run
      if (k != cur) {
        if (cur != OV_EMPTY) {
          int s = (int)(ov_hash(cur) >> 24), hit = -1;          // OV_SLOTS = 2^8
#pragma unroll
          for (int t = 0; t < OV_PROBES && hit < 0; ++t) {
            const unsigned long long old = atomicCAS(&s_key[s], OV_EMPTY, cur);
            if (old == OV_EMPTY || old == cur) hit = s;
            s = (s + 1) & (OV_SLOTS - 1);
          }
          if (hit >= 0) atomicAdd(&s_cnt[hit], n);
          else ov_emit(S, (int)((cur >> 31) & 0x7fffffffull), (int)(cur & 0x7fffffffull), (int)(cur >> 62), n);
        }
        cur = k;
        n = 0;
      }
      if (k != OV_EMPTY) n += 1;
    }
  }
  __syncthreads();
  const unsigned long long k = s_key[threadIdx.x];
  if (k != OV_EMPTY) ov_emit(S, (int)((k >> 31) & 0x7fffffffull), (int)(k & 0x7fffffffull), (int)(k >> 62), s_cnt[threadIdx.x]);
}
static_assert(OV_SLOTS == 256, "ov_pixel_kernel: one LDS slot per thread, the slot index is the hash's top 8 bits");
static_assert(CC_TH == 32 && CC_TW == 64, "ov_pixel_kernel: 4 waves x 8 rows, 8 lanes x 8 columns cover exactly one 32 x 64 tile");

__global__ __launch_bounds__(256) void ov_compact_kernel(long nslots, const unsigned long long* __restrict__ slots,
                                                         const unsigned* __restrict__ opened, const int* __restrict__ ticket_slot, int pair_cap,
                                                         long long* __restrict__ pairs, int* __restrict__ npairs) {
  const unsigned n = opened[blockIdx.y];
  const int stored = n < (unsigned)pair_cap ? (int)n : pair_cap;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    npairs[blockIdx.y * 2 + 0] = stored;
    npairs[blockIdx.y * 2 + 1] = n > (unsigned)pair_cap ? 1 : 0;
  }
  if (i >= stored) return;
  const long h = ticket_slot[(size_t)blockIdx.y * pair_cap + i];
  if (h < 0 || h >= nslots) return;
  const unsigned long long* T = slots + ((size_t)blockIdx.y * nslots + h) * 2;
  const unsigned long long key = T[0] - 1ull;
  long long* out = pairs + ((size_t)blockIdx.y * pair_cap + i) * 3;
  out[0] = (long long)(key >> 32);
  out[1] = (long long)(key & 0xffffffffull);
  out[2] = (long long)T[1];
}

// counts of one side's scored components into v[first] (unmatched) and v[first + 1] (matched), per class
__device__ inline void ov_score_side(int cap, const long long* __restrict__ table, const int* __restrict__ ncomp,
                                     const long long* __restrict__ cover, long long min_pixels, int cover_q, unsigned* s_n, int unmatched,
                                     int matched) {
  const int b = blockIdx.x;
  int rows = ncomp[b * 3];
  rows = rows < 0 ? 0 : (rows > cap ? cap : rows);
  unsigned v[4] = {0u, 0u, 0u, 0u};               // class 1: unmatched, matched; class 2: unmatched, matched
  for (int k = threadIdx.x; k < rows; k += 256) {
    const long long* row = table + ((size_t)b * cap + k) * CC_FIELDS;
    const long long cls = row[1], px = row[2];
    if ((cls != 1 && cls != 2) || px < min_pixels) continue;
    const long long cov = cover[(size_t)b * cap + k];
    const int f = (cls == 2 ? 2 : 0) + ((cov >= 1 && cov * 1024 >= (long long)cover_q * px) ? 1 : 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += f == i ? 1u : 0u;
  }
  if (v[0]) atomicAdd(&s_n[0 + unmatched], v[0]);
  if (v[1]) atomicAdd(&s_n[0 + matched], v[1]);
  if (v[2]) atomicAdd(&s_n[4 + unmatched], v[2]);
  if (v[3]) atomicAdd(&s_n[4 + matched], v[3]);
}

__global__ __launch_bounds__(256) void ov_scores_kernel(int cap_a, const long long* __restrict__ table_a, const int* __restrict__ ncomp_a,
                                                        const long long* __restrict__ cover_a, int cap_b, const long long* __restrict__ table_b,
                                                        const int* __restrict__ ncomp_b, const long long* __restrict__ cover_b,
                                                        const int* __restrict__ npairs, long long min_pixels, int cover_q,
                                                        long long* __restrict__ scores, unsigned long long* acc) {
  __shared__ unsigned s_n[OV_SCORE_FIELDS];       // per class: hits, misses, false alarms, matched detections
  const int b = blockIdx.x;
  if (threadIdx.x < OV_SCORE_FIELDS) s_n[threadIdx.x] = 0u;
  __syncthreads();
  ov_score_side(cap_b, table_b, ncomp_b, cover_b, min_pixels, cover_q, s_n, 1, 0);
  ov_score_side(cap_a, table_a, ncomp_a, cover_a, min_pixels, cover_q, s_n, 2, 3);
  __syncthreads();
  if (threadIdx.x < OV_SCORE_FIELDS) {
    scores[(size_t)b * OV_SCORE_FIELDS + threadIdx.x] = (long long)s_n[threadIdx.x];
    if (s_n[threadIdx.x]) atomicAdd(acc + threadIdx.x, (unsigned long long)s_n[threadIdx.x]);
  } else if (threadIdx.x == 8) {
    atomicAdd(acc + 8, 1ull);
  } else if (threadIdx.x == 9) {
    if (ncomp_a[b * 3] > cap_a || ncomp_b[b * 3] > cap_b || npairs[b * 2 + 1] != 0) atomicAdd(acc + 9, 1ull);
  }
}

}  // namespace dc

extern "C" int dc_component_overlap_lds_slots(int* slots) {
  DC_REQUIRE(slots, "dc_component_overlap_lds_slots: null argument");
  *slots = OV_SLOTS;
  return 0;
}

extern "C" size_t dc_component_overlap_workspace(int B, int pair_cap) {
  if (B <= 0 || pair_cap <= 0 || pair_cap > (1 << 24)) return 0;
  return cc_align((size_t)B * (size_t)ov_slots(pair_cap) * 16) + cc_align((size_t)B * 4) + cc_align((size_t)B * pair_cap * 4);
}

extern "C" int dc_component_overlap(int B, int n_valid, int H, int W, const uint8_t* mask_a, const int32_t* labels_a, const int32_t* rank_a,
                                    int cap_a, const uint8_t* mask_b, const int32_t* labels_b, const int32_t* rank_b, int cap_b, int pair_cap,
                                    int64_t* pairs, int32_t* npairs, int64_t* cover_a, int64_t* cover_b, void* workspace, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(cap_a >= 1 && cap_b >= 1, "dc_component_overlap: cap_a and cap_b must be at least 1");
  DC_REQUIRE(pair_cap >= 1 && pair_cap <= (1 << 24), "dc_component_overlap: pair_cap must lie in [1, 2^24]");
  DC_REQUIRE(mask_a && labels_a && rank_a && mask_b && labels_b && rank_b && pairs && npairs && cover_a && cover_b && workspace,
             "dc_component_overlap: null pointer");
  DC_REQUIRE(((uintptr_t)workspace & 255) == 0, "dc_component_overlap: workspace not 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long nslots = ov_slots(pair_cap);
  // the workspace: slots int64 [B][nslots][2] | opened uint32 [B] | ticket_slot int32 [B][pair_cap]
  unsigned long long* slots = (unsigned long long*)workspace;
  const size_t table_bytes = cc_align((size_t)B * nslots * 16);
  unsigned* opened = (unsigned*)((char*)workspace + table_bytes);
  int* ticket_slot = (int*)((char*)opened + cc_align((size_t)B * 4));
  hipError_t e = hipMemsetAsync(pairs, 0, (size_t)B * pair_cap * 3 * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(cover_a, 0, (size_t)B * cap_a * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(cover_b, 0, (size_t)B * cap_b * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(slots, 0, table_bytes + cc_align((size_t)B * 4), st);      // the table and the counters behind it
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const int tx = (W + CC_TW - 1) / CC_TW, ty = (H + CC_TH - 1) / CC_TH;
  hipLaunchKernelGGL(ov_pixel_kernel, dim3(tx, ty, n_valid), dim3(256), 0, st, H, W, mask_a, labels_a, rank_a, cap_a, mask_b, labels_b, rank_b,
                     cap_b, (unsigned long long*)cover_a, (unsigned long long*)cover_b, slots, nslots, opened, ticket_slot, pair_cap);
  DC_LAUNCHED("cc_overlap");
  hipLaunchKernelGGL(ov_compact_kernel, dim3((pair_cap + 255) / 256, n_valid), dim3(256), 0, st, nslots, slots, opened, ticket_slot, pair_cap,
                     (long long*)pairs, npairs);
  DC_LAUNCHED("cc_overlap");
  return 0;
}

extern "C" int dc_event_scores(int B, int n_valid, int cap_a, const int64_t* table_a, const int32_t* ncomp_a, const int64_t* cover_a, int cap_b,
                               const int64_t* table_b, const int32_t* ncomp_b, const int64_t* cover_b, const int32_t* npairs, long min_pixels,
                               int cover_q, int64_t* scores, int64_t* acc, void* stream) {
  DC_REQUIRE(B > 0 && n_valid > 0 && n_valid <= B, "dc_event_scores: n_valid must lie in [1, B]");
  DC_REQUIRE(cap_a >= 1 && cap_b >= 1, "dc_event_scores: cap_a and cap_b must be at least 1");
  DC_REQUIRE(cover_q >= 1 && cover_q <= 1024, "dc_event_scores: cover_q must lie in [1, 1024]");
  DC_REQUIRE(table_a && ncomp_a && cover_a && table_b && ncomp_b && cover_b && npairs && scores && acc, "dc_event_scores: null pointer");
  hipLaunchKernelGGL(ov_scores_kernel, dim3(n_valid), dim3(256), 0, (hipStream_t)stream, cap_a, (const long long*)table_a, ncomp_a,
                     (const long long*)cover_a, cap_b, (const long long*)table_b, ncomp_b, (const long long*)cover_b, npairs,
                     (long long)(min_pixels < 1 ? 1 : min_pixels), cover_q, (long long*)scores, (unsigned long long*)acc);
  DC_LAUNCHED("cc_overlap");
  return 0;
}

// ---- per-event statistics of the input fields (dc_component_fields; nn.EventFields) ---------------------------------------------------
// One row of six int64 words per (event rank, channel): min, max, sum, wsum, nonfinite, saturated (include/deepcam_hip.h has the
// definition).  The extremes are 64-bit words (order-preserving key of the float << 32 | pixel), so ONE unsigned atomicMin / atomicMax
// settles value and position together, ties on the smallest pixel; the sums are int64 sums of values quantised PER PIXEL (rint of an
// exact fp64 scaling), so they are sums of integers.  Minimum, maximum and integer addition are associative and commutative: the row
// does not depend on the order in which pixels, runs, LDS slots and workgroups arrive.
//   fs_init     the empty row (-1, 0, 0, 0, 0, 0) into every row of the valid samples, 16 bytes per thread
//   fs_pixel    one workgroup per tile, the thread layout of cc_accumulate.  A thread reads its 8 labels first and touches the fields of
//               foreground pixels only (a pixel's channels are contiguous: 16-byte loads where the layout allows).  Per group of FS_GROUP
//               channels it reduces each run of one root in registers and hands the run to the workgroup's table in LDS, keyed by root
//               (64-bit LDS atomics); runs that find no slot within FS_PROBES go to the global row directly, and so do the two counters,
//               which real data leaves at zero.  At the end every filled slot looks its rank up once and issues its global atomics.
// Integer and 64-bit atomics only; no workgroup waits for another.
namespace dc {

static constexpr int FS_SLOT_BITS = 5, FS_SLOTS = 1 << FS_SLOT_BITS;   // LDS: FS_SLOTS * C * 32 bytes + keys and ranks: 16.2 KiB at C = 16
static constexpr int FS_PROBES = 4;
static constexpr int FS_GROUP = 4;                // channels reduced at a time: one 16-byte load per pixel, 40 registers of partial results
static constexpr int FS_STATS = 6, FS_MAX_C = 32;
static constexpr unsigned long long FS_NONE = ~0ull;

__global__ __launch_bounds__(256) void fs_init_kernel(long npieces, ulonglong2* __restrict__ ftable) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npieces) return;
  ftable[i] = make_ulonglong2(i % 3 == 0 ? FS_NONE : 0ull, 0ull);     // a row is three pieces: (min, max) (sum, wsum) (nonfinite, saturated)
}

struct FsRun {                                    // one thread's run of pixels of one component, FS_GROUP channels of it
  unsigned long long kmin[FS_GROUP], kmax[FS_GROUP];
  long long sum[FS_GROUP], wsum[FS_GROUP];
  int nonfinite[FS_GROUP], saturated[FS_GROUP];
};

__device__ inline void fs_clear(FsRun& a) {
#pragma unroll
  for (int i = 0; i < FS_GROUP; ++i) {
    a.kmin[i] = FS_NONE;
    a.kmax[i] = 0ull;
    a.sum[i] = a.wsum[i] = 0;
    a.nonfinite[i] = a.saturated[i] = 0;
  }
}

// one value of pixel p (sample-local index) into channel i of the run; wf = wy[r] * 2^-20, exact
__device__ inline void fs_take(FsRun& a, int i, float v, unsigned p, int bits, double wf) {
  const unsigned u = __float_as_uint(v);
  if ((u & 0x7f800000u) == 0x7f800000u) {         // NaN, +-Inf
    a.nonfinite[i] += 1;
    return;
  }
  const unsigned long long key = (u & 0x80000000u) ? (u ^ 0xffffffffu) : (u | 0x80000000u);
  const unsigned long long lo = (key << 32) | p, hi = (key << 32) | (0xffffffffu - p);
  a.kmin[i] = lo < a.kmin[i] ? lo : a.kmin[i];
  a.kmax[i] = hi > a.kmax[i] ? hi : a.kmax[i];
  const double s = ldexp((double)v, bits);        // exact: a float times a power of two stays inside fp64 for every bits the host hands out
  const double q = rint(s);
  if (!(fabs(q) <= 0x1p40)) {
    a.saturated[i] += 1;
    return;
  }
  a.sum[i] += (long long)q;
  a.wsum[i] += (long long)rint(s * wf);           // one rounded product of two exact factors, then rint
}

struct FsSample {                                 // one sample's slices
  const int* rank;
  unsigned long long* ftable;
  long HW;
  int cap, C;
};

__device__ inline unsigned long long* fs_row(const FsSample& S, int root, int ch) {
  if (root < 0 || root >= S.HW) return nullptr;
  const int k = S.rank[root];
  if (k < 0 || k >= S.cap) return nullptr;        // beyond the table: no row
  return S.ftable + ((size_t)k * S.C + ch) * FS_STATS;
}

__device__ inline void fs_emit(unsigned long long* row, unsigned long long kmin, unsigned long long kmax, long long sum, long long wsum,
                               int nonfinite, int saturated) {
  if (kmin != FS_NONE) {
    atomicMin(row + 0, kmin);
    atomicMax(row + 1, kmax);
  }
  if (sum != 0) atomicAdd(row + 2, (unsigned long long)sum);
  if (wsum != 0) atomicAdd(row + 3, (unsigned long long)wsum);
  if (nonfinite != 0) atomicAdd(row + 4, (unsigned long long)nonfinite);
  if (saturated != 0) atomicAdd(row + 5, (unsigned long long)saturated);
}

// a finished run: into the slot of its root, or to the global rows when the table has no room for the root
__device__ inline void fs_flush(const FsSample& S, int* s_key, unsigned long long* s_tab, int root, int g, int nch, const FsRun& a) {
  int s = (int)(((unsigned)root * 2654435761u) >> (32 - FS_SLOT_BITS)), hit = -1;
#pragma unroll
  for (int t = 0; t < FS_PROBES && hit < 0; ++t) {
    const int old = atomicCAS(&s_key[s], -1, root);
    if (old == -1 || old == root) hit = s;
    s = (s + 1) & (FS_SLOTS - 1);
  }
#pragma unroll
  for (int i = 0; i < FS_GROUP; ++i) {
    if (i >= nch) break;
    if (hit >= 0) {
      unsigned long long* T = s_tab + ((size_t)hit * S.C + g + i) * 4;
      if (a.kmin[i] != FS_NONE) {
        atomicMin(T + 0, a.kmin[i]);
        atomicMax(T + 1, a.kmax[i]);
      }
      if (a.sum[i] != 0) atomicAdd(T + 2, (unsigned long long)a.sum[i]);
      if (a.wsum[i] != 0) atomicAdd(T + 3, (unsigned long long)a.wsum[i]);
      if ((a.nonfinite[i] | a.saturated[i]) != 0) {
        unsigned long long* row = fs_row(S, root, g + i);
        if (row) fs_emit(row, FS_NONE, 0ull, 0, 0, a.nonfinite[i], a.saturated[i]);
      }
    } else {
      unsigned long long* row = fs_row(S, root, g + i);
      if (row) fs_emit(row, a.kmin[i], a.kmax[i], a.sum[i], a.wsum[i], a.nonfinite[i], a.saturated[i]);
    }
  }
}

// FS_GROUP channels of one pixel, zeros where `on` is false: one 16-byte load (ldc % 4 == 0, a 16-byte aligned base and g % 4 == 0 put
// g + 4 <= ldc, inside the pixel) or up to four scalar ones
template <bool VEC>
__device__ inline void fs_load(float* v, const float* q, int nch, bool on) {
#pragma unroll
  for (int i = 0; i < FS_GROUP; ++i) v[i] = 0.f;
  if (!on) return;
  if (VEC) {
    const float4 t = *(const float4*)q;
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < FS_GROUP; ++i)
      if (i < nch) v[i] = q[i];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void fs_pixel_kernel(int H, int W, const int* __restrict__ labels, const int* __restrict__ rank_map, int cap,
                                                       const float* __restrict__ fields, int C, int ldc, const int* __restrict__ scale_bits,
                                                       const int* __restrict__ wy, unsigned long long* ftable) {
  extern __shared__ unsigned long long fs_lds[];  // table [FS_SLOTS][C][4] = min, max, sum, wsum | keys int [FS_SLOTS]
  unsigned long long* s_tab = fs_lds;
  int* s_key = (int*)(fs_lds + (size_t)FS_SLOTS * C * 4);
  FsSample S;
  S.HW = (long)H * W;
  const size_t base = (size_t)blockIdx.z * S.HW;
  S.rank = rank_map + base;
  S.ftable = ftable + (size_t)blockIdx.z * cap * C * FS_STATS;
  S.cap = cap;
  S.C = C;
  for (int i = threadIdx.x; i < FS_SLOTS * C * 4; i += 256) s_tab[i] = (i & 3) == 0 ? FS_NONE : 0ull;
  if (threadIdx.x < FS_SLOTS) s_key[threadIdx.x] = -1;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.y * CC_TH + wave * 8 + lane / 8, cb = blockIdx.x * CC_TW + (lane % 8) * 8;
  if (r < H && cb < W) {
    const int* lab = labels + base + (size_t)r * W + cb;
    unsigned fg = 0u, brk = 0u;                   // bit j: pixel j is foreground; it begins a run (its root is not its left neighbour's)
    int prev = -1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int rt = (cb + j < W ? lab[j] : 0) - 1;                                 // -1: background, beyond the row's end
      fg |= rt >= 0 ? 1u << j : 0u;
      brk |= rt >= 0 && rt != prev ? 1u << j : 0u;
      prev = rt;
    }
    if (fg != 0u) {                               // (about one thread in ten on real masks: the others never touch the fields)
      const double wf = (double)wy[r] * 0x1p-20;
      const unsigned p0 = (unsigned)(r * W + cb);
      const float* px = fields + (base + (size_t)r * W + cb) * ldc;
      for (int g = 0; g < C; g += FS_GROUP) {
        const int nch = C - g < FS_GROUP ? C - g : FS_GROUP;
        int bits[FS_GROUP];
#pragma unroll
        for (int i = 0; i < FS_GROUP; ++i) bits[i] = i < nch ? scale_bits[g + i] : 0;
        FsRun a;
        fs_clear(a);
        int cur = -1;
        float v[FS_GROUP], nx[FS_GROUP];
        fs_load<VEC>(v, px + g, nch, (fg & 1u) != 0u);
#pragma unroll 1
        for (int j = 0; j < 8; ++j) {             // a plain loop: one copy of the body keeps the registers, and with them the occupancy
          fs_load<VEC>(nx, px + (size_t)(j + 1) * ldc + g, nch, j < 7 && ((fg >> (j + 1)) & 1u) != 0u);   // the next pixel's, in flight
          const bool here = ((fg >> j) & 1u) != 0u;
          if (cur >= 0 && (!here || ((brk >> j) & 1u) != 0u)) {
            fs_flush(S, s_key, s_tab, cur, g, nch, a);
            cur = -1;
          }
          if (here) {
            if (cur < 0) {
              cur = lab[j] - 1;                   // the run's root: read again (a cache hit) rather than kept in eight registers
              fs_clear(a);
            }
#pragma unroll
            for (int i = 0; i < FS_GROUP; ++i)
              if (i < nch) fs_take(a, i, v[i], p0 + j, bits[i], wf);
          }
#pragma unroll
          for (int i = 0; i < FS_GROUP; ++i) v[i] = nx[i];
        }
        if (cur >= 0) fs_flush(S, s_key, s_tab, cur, g, nch, a);
      }
    }
  }
  __syncthreads();
  __shared__ int s_rank[FS_SLOTS];
  if (threadIdx.x < FS_SLOTS) {                   // one rank lookup per filled slot
    const int rt = s_key[threadIdx.x];
    int k = -1;
    if (rt >= 0 && rt < S.HW) {
      k = S.rank[rt];
      if (k < 0 || k >= cap) k = -1;
    }
    s_rank[threadIdx.x] = k;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < FS_SLOTS * C; i += 256) {
    const int k = s_rank[i / C];
    if (k < 0) continue;
    const unsigned long long* T = s_tab + (size_t)i * 4;
    fs_emit(S.ftable + ((size_t)k * C + i % C) * FS_STATS, T[0], T[1], (long long)T[2], (long long)T[3], 0, 0);
  }
}
static_assert(FS_GROUP == 4, "fs_pixel_kernel: a channel group is one float4");
static_assert(CC_TH == 32 && CC_TW == 64, "fs_pixel_kernel: 4 waves x 8 rows, 8 lanes x 8 columns cover exactly one 32 x 64 tile");

}  // namespace dc

extern "C" int dc_component_fields_lds_slots(int* slots) {
  DC_REQUIRE(slots, "dc_component_fields_lds_slots: null argument");
  *slots = FS_SLOTS;
  return 0;
}

extern "C" int dc_component_fields(int B, int n_valid, int H, int W, const int32_t* labels, const int32_t* rank_map, int cap,
                                   const float* fields, int C, int ldc, const int32_t* scale_bits, const int32_t* wy, int64_t* ftable,
                                   void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE((long)H * W <= (1L << 22), "dc_component_fields: H * W must be at most 2^22 (the pixel shares a word with the key; sums stay in int64)");
  DC_REQUIRE(C >= 1 && C <= FS_MAX_C, "dc_component_fields: C must lie in [1, 32]");
  DC_REQUIRE(ldc >= C, "dc_component_fields: ldc must be at least C");
  DC_REQUIRE(cap >= 1, "dc_component_fields: cap must be at least 1");
  DC_REQUIRE((long)n_valid * cap * C * 3 < 2147483647L * 256, "dc_component_fields: n_valid * cap * C is too large");
  DC_REQUIRE(labels && rank_map && fields && scale_bits && wy && ftable, "dc_component_fields: null pointer");
  DC_REQUIRE(((uintptr_t)ftable & 15) == 0, "dc_component_fields: ftable not 16-byte aligned");
  DC_REQUIRE(((uintptr_t)fields & 3) == 0, "dc_component_fields: fields not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long npieces = (long)n_valid * cap * C * 3;
  hipLaunchKernelGGL(fs_init_kernel, dim3((unsigned)((npieces + 255) / 256)), dim3(256), 0, st, npieces, (ulonglong2*)ftable);
  DC_LAUNCHED("cc_fields");
  const int tx = (W + CC_TW - 1) / CC_TW, ty = (H + CC_TH - 1) / CC_TH;
  const size_t lds = (size_t)FS_SLOTS * C * 32 + FS_SLOTS * sizeof(int);
  const bool vec = ldc % 4 == 0 && ((uintptr_t)fields & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(fs_pixel_kernel<true>, dim3(tx, ty, n_valid), dim3(256), lds, st, H, W, labels, rank_map, cap, fields, C, ldc,
                       scale_bits, wy, (unsigned long long*)ftable);
  else
    hipLaunchKernelGGL(fs_pixel_kernel<false>, dim3(tx, ty, n_valid), dim3(256), lds, st, H, W, labels, rank_map, cap, fields, C, ldc,
                       scale_bits, wy, (unsigned long long*)ftable);
  DC_LAUNCHED("cc_fields");
  return 0;
}

// ---- event tracks (dc_track_append, dc_track_link, dc_track_resolve; nn.EventTracker) ------------------------------------------------
// The events of a time series, numbered in the order frames and ranks arrive, and a second union-find forest over those numbers: two
// events of consecutive frames that share a pixel of their class are united, a track is a tree.  `parent` is int32 [event_cap] in the
// plain encoding of the LDS forest above (a root names itself), and the two invariants of this file's header carry over word for word:
//   (I1) dc_track_append writes parent[e] = e before any launch on the stream can meet e, and afterwards an entry changes by atomicMin
//        only (tk_union) or, in tk_flatten, to the root a walk from it ended at; both are smaller than the entry's index or equal to
//        what it held.  A link joins an event with one of the frame before, whose number is smaller (the numbers grow with the frames),
//        and unites the two ROOTS, the larger below the smaller: every link goes to a smaller number, every walk descends and ends.
//   (I2) every value parent[e] ever held names an event of e's track: itself, a root it was united with, or the root of a later walk.
// So it does not matter whether the entries of earlier calls are flattened, partly flattened (a resolve in the middle of the series) or
// as the unions left them: a union through them still ends at the two current roots.  When an atomicMin replaces a -> old by a -> b the
// loop goes on with (old, b), as g_union does.  The state survives from call to call in device memory; nothing is read on the host.
//   tk_first    one workgroup: the prefix sum of min(ncomp, cap) over the batch's frames on top of the events seen so far, the counters
//   tk_fill     16 threads per new event: its row of the store (frame, rank, the ten catalogue columns) and parent[e] = e
//   tk_link     one thread per 4 consecutive pixels of a frame pair, both masks as one word each where the layout allows; labels and ranks
//               are read only where both masks hold the same class 1 or 2.  A thread skips a pixel whose two labels equal those of the
//               foreground pixel before it (its own, or the last one of its left lane): a run costs one union.  A repeated union that
//               slips through is two finds and no atomic.
//   tk_flatten, tk_count, tk_offsets, tk_rank, tk_gather    (resolve) every entry becomes its root, the roots are ranked in order as
//               cc_count / cc_offsets / cc_rank rank root pixels, and every event adds itself to its track's row with 64-bit integer
//               atomics (sums and unsigned maxima: no result depends on the order of arrival).  A track's root is its smallest event
//               number, so its id, its class and its first frame are the root's own and need no atomic.
namespace dc {

static constexpr int TK_STORE = 12, TK_TRACK = 8;  // store row: frame, rank, the catalogue's CC_FIELDS; track row: id, class, events, first, last, pixels, peak, area
static constexpr int TK_CHUNK = 256;               // events per workgroup of the root count and rank passes
static constexpr unsigned long long TK_NONE = ~0ull;
static_assert(TK_STORE == CC_FIELDS + 2, "tk_fill_kernel: a store row is (frame, rank) and a catalogue row");

__device__ inline int tk_find(const int* P, int x) {
  for (;;) {
    const int p = __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= x || p < 0) return x;      // root (p == x); anything else cannot occur and ends the walk as well
    x = p;
  }
}
__device__ inline void tk_union(int* P, int a, int b) {
  for (;;) {
    a = tk_find(P, a);
    b = tk_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b);
    if (old >= a) return;               // a was a root and now hangs below b
    a = old;                            // a had been linked meanwhile: its former parent and b are still to be united
  }
}

__device__ inline int tk_rows(const int* __restrict__ ncomp, int j, int cap) {
  const int all = ncomp[j * 3];
  return all < 0 ? 0 : (all > cap ? cap : all);
}

__global__ __launch_bounds__(256) void tk_first_kernel(int n_valid, int cap, const int* __restrict__ ncomp, long long event_cap, long long* state,
                                                       long long* __restrict__ first) {
  __shared__ int s_w[4];
  __shared__ long long s_base;
  if (threadIdx.x == 0) s_base = state[0] + state[2];
  __syncthreads();
  const long long base = s_base;
  long long carry = 0, cut = 0;
  for (int j0 = 0; j0 < n_valid; j0 += 256) {      // uniform trip count: every thread reaches the barriers inside the scans
    const int j = j0 + threadIdx.x;
    const int v = j < n_valid ? tk_rows(ncomp, j, cap) : 0, t = j < n_valid && ncomp[j * 3] > cap ? 1 : 0;
    int tot, tot_t;
    const int ex = block_excl_scan(v, s_w, &tot);
    block_excl_scan(t, s_w, &tot_t);
    if (j < n_valid) first[j] = base + carry + ex;
    carry += tot;
    cut += tot_t;
  }
  if (threadIdx.x == 0) {                          // the only reader of the state is this workgroup, and it has read it
    const long long all = base + carry, stored = all < event_cap ? all : event_cap;
    state[0] = stored;
    state[1] += n_valid;
    state[2] = all - stored;
    state[3] += cut;
  }
}

__global__ __launch_bounds__(256) void tk_fill_kernel(int cap, const long long* __restrict__ table, const int* __restrict__ ncomp, long long frame0,
                                                      long long event_cap, const long long* __restrict__ first, int* __restrict__ parent,
                                                      long long* __restrict__ store) {
  const int j = blockIdx.y, k = blockIdx.x * 16 + (threadIdx.x >> 4), f = threadIdx.x & 15;
  if (k >= tk_rows(ncomp, j, cap) || f >= TK_STORE) return;
  const long long e = first[j] + k;
  if (e < 0 || e >= event_cap) return;             // beyond the store: counted in the state only
  store[e * TK_STORE + f] = f == 0 ? frame0 + j : f == 1 ? (long long)k : table[((size_t)j * cap + k) * CC_FIELDS + (f - 2)];
  if (f == 0) parent[e] = (int)e;
}

struct TkPair {                                    // one frame pair's slices and what every lookup needs
  const int *rank_a, *rank_b;
  long long first_a, first_b, event_cap, min_pixels;
  const long long* store;
  int* parent;
  long HW;
  int cap;
};

__device__ inline void tk_link(const TkPair& S, int root_a, int root_b) {
  if (root_a < 0 || root_a >= S.HW || root_b < 0 || root_b >= S.HW) return;
  const int ra = S.rank_a[root_a], rb = S.rank_b[root_b];
  if (ra < 0 || ra >= S.cap || rb < 0 || rb >= S.cap) return;                   // no row in its frame's table: no event
  const long long ea = S.first_a + ra, eb = S.first_b + rb;
  if (ea < 0 || ea >= S.event_cap || eb < 0 || eb >= S.event_cap) return;       // not stored
  if (S.min_pixels > 1 && (S.store[ea * TK_STORE + 4] < S.min_pixels || S.store[eb * TK_STORE + 4] < S.min_pixels)) return;
  tk_union(S.parent, (int)ea, (int)eb);
}

template <bool VEC>
__global__ __launch_bounds__(256) void tk_link_kernel(long HW, const uint8_t* __restrict__ mask_a, const int* __restrict__ labels_a,
                                                      const int* __restrict__ rank_a, const long long* __restrict__ first_a,
                                                      const uint8_t* __restrict__ mask_b, const int* __restrict__ labels_b,
                                                      const int* __restrict__ rank_b, const long long* __restrict__ first_b, int cap,
                                                      long long event_cap, long long min_pixels, const long long* store, int* parent) {
  const size_t base = (size_t)blockIdx.y * HW;
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  unsigned wa = 0u, wb = 0u;                       // four mask bytes of each side; zero (background) beyond the frame's end
  if (p0 < HW) {
    if (VEC) {                                     // HW % 4 == 0 and 4-byte aligned bases: the word lies inside the frame
      wa = *(const unsigned*)(mask_a + base + p0);
      wb = *(const unsigned*)(mask_b + base + p0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p0 + i < HW) {
          wa |= (unsigned)mask_a[base + p0 + i] << (8 * i);
          wb |= (unsigned)mask_b[base + p0 + i] << (8 * i);
        }
    }
  }
  unsigned long long key[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned ca = (wa >> (8 * i)) & 255u, cb = (wb >> (8 * i)) & 255u;
    key[i] = TK_NONE;
    if (ca == cb && (ca == 1u || ca == 2u)) {
      const int la = labels_a[base + p0 + i], lb = labels_b[base + p0 + i];
      if (la > 0 && lb > 0) key[i] = ((unsigned long long)(unsigned)la << 32) | (unsigned)lb;
    }
  }
  // every lane is still here: the last pixel of the left lane (the frame is one flat run of pixels; lane 0 starts afresh)
  unsigned long long prev = __shfl_up(key[3], 1, 64);
  if ((threadIdx.x & 63) == 0) prev = TK_NONE;
  if ((key[0] & key[1] & key[2] & key[3]) == TK_NONE) return;
  TkPair S;
  S.rank_a = rank_a + base;
  S.rank_b = rank_b + base;
  S.first_a = first_a[blockIdx.y];
  S.first_b = first_b[blockIdx.y];
  S.event_cap = event_cap;
  S.min_pixels = min_pixels;
  S.store = store;
  S.parent = parent;
  S.HW = HW;
  S.cap = cap;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned long long k = key[i];
    if (k == TK_NONE || k == prev) continue;
    prev = k;
    tk_link(S, (int)(k >> 32) - 1, (int)(k & 0xffffffffull) - 1);
  }
}

__global__ __launch_bounds__(256) void tk_flatten_kernel(const long long* __restrict__ state, int* parent) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= state[0]) return;
  const int v = parent[e];
  if (v < 0 || v >= (int)e) return;
  const int root = tk_find(parent, v);             // other threads' stores of this launch replace an entry by its root, an ancestor (I2)
  if (root != v) parent[e] = root;
}

// roots (total, class 1) of every chunk of TK_CHUNK consecutive events
__global__ __launch_bounds__(256) void tk_count_kernel(const long long* __restrict__ state, const int* __restrict__ parent,
                                                       const long long* __restrict__ store, int* __restrict__ chunk_cnt) {
  __shared__ int s_w[4];
  const long long e = (long long)blockIdx.x * TK_CHUNK + threadIdx.x;
  const bool root = e < state[0] && parent[e] == (int)e;
  const bool one = root && store[e * TK_STORE + 3] == 1;
  int tot, tot1;
  block_excl_scan(root ? 1 : 0, s_w, &tot);
  block_excl_scan(one ? 1 : 0, s_w, &tot1);
  if (threadIdx.x == 0) {
    chunk_cnt[(size_t)blockIdx.x * 2 + 0] = tot;
    chunk_cnt[(size_t)blockIdx.x * 2 + 1] = tot1;
  }
}

// one workgroup: the live chunks' counts become exclusive offsets, the sums go to ntracks
__global__ __launch_bounds__(256) void tk_offsets_kernel(const long long* __restrict__ state, const int* __restrict__ chunk_cnt,
                                                         int* __restrict__ chunk_off, long long track_cap, long long* __restrict__ ntracks) {
  __shared__ int s_w[4];
  const long long nchunk = (state[0] + TK_CHUNK - 1) / TK_CHUNK;
  int carry = 0, carry1 = 0;
  for (long long k0 = 0; k0 < nchunk; k0 += 256) {
    const long long k = k0 + threadIdx.x;
    const int v = k < nchunk ? chunk_cnt[2 * k] : 0, v1 = k < nchunk ? chunk_cnt[2 * k + 1] : 0;
    int tot, tot1;
    const int ex = block_excl_scan(v, s_w, &tot);
    block_excl_scan(v1, s_w, &tot1);
    if (k < nchunk) chunk_off[k] = carry + ex;
    carry += tot;
    carry1 += tot1;
  }
  if (threadIdx.x == 0) {
    ntracks[0] = carry;
    ntracks[1] = carry1;
    ntracks[2] = carry - carry1;
    ntracks[3] = carry < track_cap ? (long long)carry : track_cap;
  }
}

// every root learns its row (kept in row_of at the root's own index) and opens it: id, class, first frame
__global__ __launch_bounds__(256) void tk_rank_kernel(const long long* __restrict__ state, const int* __restrict__ parent,
                                                      const long long* __restrict__ store, const int* __restrict__ chunk_off, int track_cap,
                                                      int* __restrict__ row_of, long long* __restrict__ tracks) {
  __shared__ int s_w[4];
  const long long e = (long long)blockIdx.x * TK_CHUNK + threadIdx.x;
  const bool root = e < state[0] && parent[e] == (int)e;
  int tot;
  const int ex = block_excl_scan(root ? 1 : 0, s_w, &tot);
  if (!root) return;
  const int row = chunk_off[blockIdx.x] + ex;
  row_of[e] = row;
  if (row < track_cap) {
    long long* t = tracks + (size_t)row * TK_TRACK;
    t[0] = e;
    t[1] = store[e * TK_STORE + 3];
    t[3] = store[e * TK_STORE + 0];                // the smallest event number of the track lies in its earliest frame
  }
}

__global__ __launch_bounds__(256) void tk_gather_kernel(const long long* __restrict__ state, const int* __restrict__ parent,
                                                        const long long* __restrict__ store, const int* __restrict__ row_of, int track_cap,
                                                        int* __restrict__ track_of, long long* tracks) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= state[0]) return;
  const int root = parent[e];
  const int row = root >= 0 && root <= (int)e ? row_of[root] : -1;
  if (row < 0 || row >= track_cap) {
    track_of[e] = -1;
    return;
  }
  track_of[e] = row;
  const long long* s = store + e * TK_STORE;
  const unsigned long long frame = (unsigned long long)s[0], pixels = (unsigned long long)s[4];
  unsigned long long* t = (unsigned long long*)(tracks + (size_t)row * TK_TRACK);
  atomicAdd(t + 2, 1ull);
  atomicMax(t + 4, frame);
  atomicAdd(t + 5, pixels);
  atomicMax(t + 6, (pixels << 32) | (0xffffffffull - frame));
  atomicAdd(t + 7, (unsigned long long)s[5]);
}

static int tk_check_caps(int event_cap) {
  DC_REQUIRE(event_cap >= 1 && event_cap <= (1 << 30), "tracks: event_cap must lie in [1, 2^30]");
  return 0;
}

}  // namespace dc

// the workspace: row_of int32 [event_cap] | chunk_cnt int32 [nchunk][2] | chunk_off int32 [nchunk]
extern "C" size_t dc_track_workspace(int event_cap) {
  if (event_cap < 1 || event_cap > (1 << 30)) return 0;
  const size_t nchunk = ((size_t)event_cap + TK_CHUNK - 1) / TK_CHUNK;
  return cc_align((size_t)event_cap * 4) + cc_align(nchunk * 8) + cc_align(nchunk * 4);
}

extern "C" int dc_track_append(int B, int n_valid, int cap, const int64_t* table, const int32_t* ncomp, long frame0, int event_cap,
                               int64_t* state, int64_t* first, int32_t* parent, int64_t* store, void* stream) {
  DC_REQUIRE(B > 0 && n_valid > 0 && n_valid <= B, "dc_track_append: n_valid must lie in [1, B]");
  DC_REQUIRE(n_valid <= 65535, "dc_track_append: at most 65535 frames per call");
  DC_REQUIRE(cap >= 1 && cap <= (1 << 22), "dc_track_append: cap must lie in [1, 2^22]");
  if (int rc = tk_check_caps(event_cap)) return rc;
  DC_REQUIRE(frame0 >= 0 && frame0 + n_valid <= 2147483647L, "dc_track_append: frame numbers must stay below 2^31");
  DC_REQUIRE(table && ncomp && state && first && parent && store, "dc_track_append: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tk_first_kernel, dim3(1), dim3(256), 0, st, n_valid, cap, ncomp, (long long)event_cap, (long long*)state, (long long*)first);
  DC_LAUNCHED("cc_tracks");
  hipLaunchKernelGGL(tk_fill_kernel, dim3((cap + 15) / 16, n_valid), dim3(256), 0, st, cap, (const long long*)table, ncomp, (long long)frame0,
                     (long long)event_cap, (const long long*)first, parent, (long long*)store);
  DC_LAUNCHED("cc_tracks");
  return 0;
}

extern "C" int dc_track_link(int n, int H, int W, const uint8_t* mask_a, const int32_t* labels_a, const int32_t* rank_a, const int64_t* first_a,
                             const uint8_t* mask_b, const int32_t* labels_b, const int32_t* rank_b, const int64_t* first_b, int cap,
                             int event_cap, long min_pixels, const int64_t* store, int32_t* parent, void* stream) {
  DC_REQUIRE(n >= 0 && n <= 65535, "dc_track_link: n must lie in [0, 65535]");
  DC_REQUIRE(H > 0 && W > 0, "dc_track_link: H and W must be positive");
  DC_REQUIRE((long)H * W < 2147483647L, "dc_track_link: H * W must be below 2^31 - 1 (labels are int32)");
  DC_REQUIRE(cap >= 1, "dc_track_link: cap must be at least 1");
  if (int rc = tk_check_caps(event_cap)) return rc;
  DC_REQUIRE((long)event_cap <= ((1L << 43) - 1) / ((long)H * W), "dc_track_link: event_cap * H * W * 2^20 must stay below 2^63 (a track's area sum)");
  DC_REQUIRE(min_pixels >= 0, "dc_track_link: min_pixels must not be negative");
  DC_REQUIRE(mask_a && labels_a && rank_a && first_a && mask_b && labels_b && rank_b && first_b && store && parent, "dc_track_link: null pointer");
  if (n == 0) return 0;
  const long HW = (long)H * W;
  const bool vec = W % 4 == 0 && (((uintptr_t)mask_a | (uintptr_t)mask_b) & 3) == 0;
  const dim3 grid((unsigned)((HW + 1023) / 1024), n);
  if (vec)
    hipLaunchKernelGGL(tk_link_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, HW, mask_a, labels_a, rank_a, (const long long*)first_a,
                       mask_b, labels_b, rank_b, (const long long*)first_b, cap, (long long)event_cap, (long long)min_pixels,
                       (const long long*)store, parent);
  else
    hipLaunchKernelGGL(tk_link_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, HW, mask_a, labels_a, rank_a, (const long long*)first_a,
                       mask_b, labels_b, rank_b, (const long long*)first_b, cap, (long long)event_cap, (long long)min_pixels,
                       (const long long*)store, parent);
  DC_LAUNCHED("cc_tracks");
  return 0;
}

extern "C" int dc_track_resolve(int event_cap, int track_cap, const int64_t* state, int32_t* parent, const int64_t* store, int32_t* track_of,
                                int64_t* tracks, int64_t* ntracks, void* workspace, void* stream) {
  if (int rc = tk_check_caps(event_cap)) return rc;
  DC_REQUIRE(track_cap >= 1 && track_cap <= event_cap, "dc_track_resolve: track_cap must lie in [1, event_cap]");
  DC_REQUIRE(state && parent && store && track_of && tracks && ntracks && workspace, "dc_track_resolve: null pointer");
  DC_REQUIRE(((uintptr_t)workspace & 255) == 0, "dc_track_resolve: workspace not 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t nchunk = ((size_t)event_cap + TK_CHUNK - 1) / TK_CHUNK;
  int* row_of = (int*)workspace;
  int* chunk_cnt = (int*)((char*)workspace + cc_align((size_t)event_cap * 4));
  int* chunk_off = (int*)((char*)chunk_cnt + cc_align(nchunk * 8));
  hipError_t e = hipMemsetAsync(tracks, 0, (size_t)track_cap * TK_TRACK * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const dim3 grid((unsigned)nchunk);
  hipLaunchKernelGGL(tk_flatten_kernel, grid, dim3(256), 0, st, (const long long*)state, parent);
  DC_LAUNCHED("cc_tracks");
  hipLaunchKernelGGL(tk_count_kernel, grid, dim3(256), 0, st, (const long long*)state, parent, (const long long*)store, chunk_cnt);
  DC_LAUNCHED("cc_tracks");
  hipLaunchKernelGGL(tk_offsets_kernel, dim3(1), dim3(256), 0, st, (const long long*)state, chunk_cnt, chunk_off, (long long)track_cap,
                     (long long*)ntracks);
  DC_LAUNCHED("cc_tracks");
  hipLaunchKernelGGL(tk_rank_kernel, grid, dim3(256), 0, st, (const long long*)state, parent, (const long long*)store, chunk_off, track_cap, row_of,
                     (long long*)tracks);
  DC_LAUNCHED("cc_tracks");
  hipLaunchKernelGGL(tk_gather_kernel, grid, dim3(256), 0, st, (const long long*)state, parent, (const long long*)store, row_of, track_cap, track_of,
                     (long long*)tracks);
  DC_LAUNCHED("cc_tracks");
  return 0;
}

// ---- storm life cycles (dc_track_fields_append, dc_track_cycles; nn.TrackFields) -------------------------------------------------------
// The join of the two products above: dc_track_fields_append files every event's field rows (dc_component_fields) under its event number,
// next to the tracker's store, and dc_track_cycles groups them by (track, frame) when life cycles are read.  Links join consecutive
// frames only, so the frames of a track form an interval and every one of them holds an event of the track: the step rows of track row t
// are the frames[t] = last - first + 1 rows from offsets[t] on, offsets a prefix sum over the selected track rows.  No sort, no search.
// A row is stored iff it ends inside step_cap; the offsets grow with t, so the stored rows are a prefix of the selected ones and the
// stored step rows are exactly the first ncycles[2].
//   tf_file     (append) one thread per 16 bytes of a new event's field rows
//   tf_count, tf_offsets, tf_rank    the prefix sum of the selected rows' frame counts, as tk_count / tk_offsets / tk_rank rank roots, in
//               int64; tf_rank writes offsets and adds the stored step rows and the rows left out (one atomic each per workgroup)
//   tf_init     zeros into the stored step rows, the empty row into their field rows and into the lifetime rows of every track row
//   tf_event    one thread per (stored event, channel): its field row into the step's with the atomics of fs_emit; the channel-0 thread also
//               adds the event's store columns to the step row and writes the row's track and frame (every event of a step writes the
//               same two values)
//   tf_life<0>  one thread per (stored step row, channel): (key, frame) into the track's lifetime words, one atomicMin and one atomicMax
//   tf_life<1>  the same threads: the step whose (key, frame) won stores its pixel -- (track, frame) names one step row, so one writer
// Minimum, maximum and integer addition only: no result depends on the order of arrival.
namespace dc {

static constexpr int TF_STEP = 8, TF_LIFE = 4;     // step row: track, frame, events, pixels, area, sum_row, sum_cx, sum_sx; lifetime row: min, its pixel, max, its pixel
static constexpr int TF_INIT_BLOCKS = 1 << 16;     // tf_init strides over its pieces with at most this many workgroups
static_assert(FS_STATS == 6, "tf_file, tf_init, tf_event: a field row is three 16-byte pieces");

__global__ __launch_bounds__(256) void tf_file_kernel(int cap, const int* __restrict__ ncomp, const long long* __restrict__ first, int C,
                                                      long long event_cap, const ulonglong2* __restrict__ ftable, ulonglong2* __restrict__ fstore) {
  const int j = blockIdx.y;
  const long per = (long)C * 3, i = (long)blockIdx.x * 256 + threadIdx.x;
  const long k = i / per;
  if (k >= tk_rows(ncomp, j, cap)) return;
  const long long e = first[j] + k;
  if (e < 0 || e >= event_cap) return;             // beyond the store: no field row either
  fstore[(size_t)e * per + (i - k * per)] = ftable[((size_t)j * cap + k) * per + (i - k * per)];
}

// the frames of track row t if it is selected, else 0 (a track has at least one frame)
__device__ inline long long tf_frames(const long long* __restrict__ ntracks, const long long* __restrict__ tracks, long long t, int min_frames,
                                      int class_mask) {
  if (t >= ntracks[3]) return 0;
  const long long* r = tracks + (size_t)t * TK_TRACK;
  const long long n = r[4] - r[3] + 1, cls = r[1];
  if (n < 1 || n < min_frames || cls < 1 || cls > 2 || !((class_mask >> (int)cls) & 1)) return 0;
  return n;
}

__global__ __launch_bounds__(256) void tf_count_kernel(const long long* __restrict__ ntracks, const long long* __restrict__ tracks, int min_frames,
                                                       int class_mask, long long* __restrict__ chunk_cnt) {
  __shared__ long long s_w[4];
  const long long v = tf_frames(ntracks, tracks, (long long)blockIdx.x * TK_CHUNK + threadIdx.x, min_frames, class_mask);
  long long tot, tot_n;
  block_excl_scan<long long>(v, s_w, &tot);
  block_excl_scan<long long>(v > 0 ? 1 : 0, s_w, &tot_n);
  if (threadIdx.x == 0) {
    chunk_cnt[(size_t)blockIdx.x * 2 + 0] = tot;
    chunk_cnt[(size_t)blockIdx.x * 2 + 1] = tot_n;
  }
}

__global__ __launch_bounds__(256) void tf_offsets_kernel(const long long* __restrict__ ntracks, const long long* __restrict__ chunk_cnt,
                                                         long long* __restrict__ chunk_off, long long* __restrict__ ncycles) {
  __shared__ long long s_w[4];
  const long long nchunk = (ntracks[3] + TK_CHUNK - 1) / TK_CHUNK;
  long long carry = 0, carry_n = 0;
  for (long long k0 = 0; k0 < nchunk; k0 += 256) {
    const long long k = k0 + threadIdx.x;
    const long long v = k < nchunk ? chunk_cnt[2 * k] : 0, vn = k < nchunk ? chunk_cnt[2 * k + 1] : 0;
    long long tot, tot_n;
    const long long ex = block_excl_scan<long long>(v, s_w, &tot);
    block_excl_scan<long long>(vn, s_w, &tot_n);
    if (k < nchunk) chunk_off[k] = carry + ex;
    carry += tot;
    carry_n += tot_n;
  }
  if (threadIdx.x == 0) {
    ncycles[0] = carry_n;
    ncycles[1] = carry;
    ncycles[2] = 0;                                // tf_rank adds to these two
    ncycles[3] = 0;
  }
}

__global__ __launch_bounds__(256) void tf_rank_kernel(const long long* __restrict__ ntracks, const long long* __restrict__ tracks, int min_frames,
                                                      int class_mask, const long long* __restrict__ chunk_off, long long step_cap,
                                                      long long* __restrict__ offsets, long long* ncycles) {
  __shared__ long long s_w[4];
  const long long t = (long long)blockIdx.x * TK_CHUNK + threadIdx.x;
  if ((long long)blockIdx.x * TK_CHUNK >= ntracks[3]) return;   // the whole workgroup: tf_offsets wrote no offset for this chunk
  const long long v = tf_frames(ntracks, tracks, t, min_frames, class_mask);
  long long tot, rows, left;
  const long long need = chunk_off[blockIdx.x] + block_excl_scan<long long>(v, s_w, &tot);
  const bool stored = v > 0 && need + v <= step_cap;
  block_excl_scan<long long>(stored ? v : 0, s_w, &rows);
  block_excl_scan<long long>(v > 0 && !stored ? 1 : 0, s_w, &left);
  if (t < ntracks[3]) offsets[t] = v == 0 ? -1 : stored ? need : -2;
  if (threadIdx.x == 0) {
    if (rows != 0) atomicAdd((unsigned long long*)ncycles + 2, (unsigned long long)rows);
    if (left != 0) atomicAdd((unsigned long long*)ncycles + 3, (unsigned long long)left);
  }
}

// pieces of 16 bytes: 4 per stored step row, 3 C per stored step row of the fields, 2 C per track row
__global__ __launch_bounds__(256) void tf_init_kernel(int C, const long long* __restrict__ ntracks, const long long* __restrict__ ncycles,
                                                      ulonglong2* __restrict__ steps, ulonglong2* __restrict__ step_fields,
                                                      ulonglong2* __restrict__ track_fields) {
  const long long n = ncycles[2], m = ntracks[3];
  const long long a = n * (TF_STEP / 2), b = a + n * C * 3, all = b + m * C * 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < all; i += (long long)gridDim.x * 256) {
    if (i < a)
      steps[i] = make_ulonglong2(0ull, 0ull);
    else if (i < b)
      step_fields[i - a] = make_ulonglong2((i - a) % 3 == 0 ? FS_NONE : 0ull, 0ull);
    else
      track_fields[i - b] = make_ulonglong2((i - b) % 2 == 0 ? FS_NONE : 0ull, FS_NONE);   // (-1, -1) and (0, -1)
  }
}

__global__ __launch_bounds__(256) void tf_event_kernel(int C, long long step_cap, const long long* __restrict__ state,
                                                       const long long* __restrict__ store, const int* __restrict__ track_of,
                                                       const long long* __restrict__ tracks, const long long* __restrict__ offsets,
                                                       const ulonglong2* __restrict__ fstore, long long* steps, unsigned long long* step_fields) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, e = i / C;
  const int ch = (int)(i - e * C);
  if (e >= state[0]) return;
  const int t = track_of[e];
  if (t < 0) return;                               // its track has no row
  const long long off = offsets[t];
  if (off < 0) return;                             // not selected, or not stored
  const long long* s = store + e * TK_STORE;
  const long long frames = tracks[(size_t)t * TK_TRACK + 4] - tracks[(size_t)t * TK_TRACK + 3] + 1;
  const long long d = s[0] - tracks[(size_t)t * TK_TRACK + 3];
  if (d < 0 || d >= frames || off + d >= step_cap) return;   // cannot occur: the frame lies inside its track's interval, the row inside the table
  const long long row = off + d;
  const ulonglong2* src = fstore + ((size_t)e * C + ch) * 3;
  const ulonglong2 lohi = src[0], sums = src[1], cnts = src[2];
  unsigned long long* q = step_fields + ((size_t)row * C + ch) * FS_STATS;
  fs_emit(q, lohi.x, lohi.y, (long long)sums.x, (long long)sums.y, 0, 0);
  if (cnts.x != 0) atomicAdd(q + 4, cnts.x);
  if (cnts.y != 0) atomicAdd(q + 5, cnts.y);
  if (ch != 0) return;
  long long* r = steps + (size_t)row * TF_STEP;
  r[0] = t;                                        // every event of the step stores the same two values
  r[1] = s[0];
  atomicAdd((unsigned long long*)r + 2, 1ull);
  atomicAdd((unsigned long long*)r + 3, (unsigned long long)s[4]);
  atomicAdd((unsigned long long*)r + 4, (unsigned long long)s[5]);
  atomicAdd((unsigned long long*)r + 5, (unsigned long long)s[6]);
  atomicAdd((unsigned long long*)r + 6, (unsigned long long)s[7]);
  atomicAdd((unsigned long long*)r + 7, (unsigned long long)s[8]);
}

template <int PASS>
__global__ __launch_bounds__(256) void tf_life_kernel(int C, long long track_cap, const long long* __restrict__ ncycles,
                                                      const long long* __restrict__ steps, const unsigned long long* __restrict__ step_fields,
                                                      unsigned long long* track_fields) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, row = i / C;
  const int ch = (int)(i - row * C);
  if (row >= ncycles[2]) return;
  const long long t = steps[(size_t)row * TF_STEP + 0];
  const unsigned long long frame = (unsigned long long)steps[(size_t)row * TF_STEP + 1] & 0xffffffffull;
  if (t < 0 || t >= track_cap) return;             // cannot occur: every stored step row holds an event of a stored track
  const unsigned long long* q = step_fields + ((size_t)row * C + ch) * FS_STATS;
  const unsigned long long lo = q[0], hi = q[1];
  if (lo == FS_NONE) return;                       // no finite value in this step (then hi is empty as well)
  unsigned long long* life = track_fields + ((size_t)t * C + ch) * TF_LIFE;
  const unsigned long long wlo = (lo & ~0xffffffffull) | frame, whi = (hi & ~0xffffffffull) | (0xffffffffull - frame);
  if (PASS == 0) {
    atomicMin(life + 0, wlo);
    atomicMax(life + 2, whi);
  } else {
    if (life[0] == wlo) life[1] = lo & 0xffffffffull;
    if (life[2] == whi) life[3] = 0xffffffffull - (hi & 0xffffffffull);
  }
}

static int tf_check(int event_cap, int track_cap, int C) {
  if (int rc = tk_check_caps(event_cap)) return rc;
  DC_REQUIRE(track_cap >= 1 && track_cap <= event_cap, "track fields: track_cap must lie in [1, event_cap]");
  DC_REQUIRE(C >= 1 && C <= FS_MAX_C, "track fields: C must lie in [1, 32]");
  return 0;
}

}  // namespace dc

// the workspace: chunk_cnt int64 [nchunk][2] | chunk_off int64 [nchunk], nchunk chunks of TK_CHUNK track rows
extern "C" size_t dc_track_cycles_workspace(int event_cap, int track_cap) {
  if (event_cap < 1 || event_cap > (1 << 30) || track_cap < 1 || track_cap > event_cap) return 0;
  const size_t nchunk = ((size_t)track_cap + TK_CHUNK - 1) / TK_CHUNK;
  return cc_align(nchunk * 16) + cc_align(nchunk * 8);
}

extern "C" int dc_track_fields_append(int B, int n_valid, int cap, const int32_t* ncomp, const int64_t* first, const int64_t* ftable, int C,
                                      int event_cap, int64_t* fstore, void* stream) {
  DC_REQUIRE(B > 0 && n_valid > 0 && n_valid <= B, "dc_track_fields_append: n_valid must lie in [1, B]");
  DC_REQUIRE(n_valid <= 65535, "dc_track_fields_append: at most 65535 frames per call");
  DC_REQUIRE(cap >= 1 && cap <= (1 << 22), "dc_track_fields_append: cap must lie in [1, 2^22]");
  if (int rc = tf_check(event_cap, 1, C)) return rc;
  DC_REQUIRE(ncomp && first && ftable && fstore, "dc_track_fields_append: null pointer");
  DC_REQUIRE((((uintptr_t)ftable | (uintptr_t)fstore) & 15) == 0, "dc_track_fields_append: ftable or fstore not 16-byte aligned");
  const long pieces = (long)cap * C * 3;
  hipLaunchKernelGGL(tf_file_kernel, dim3((unsigned)((pieces + 255) / 256), n_valid), dim3(256), 0, (hipStream_t)stream, cap, ncomp,
                     (const long long*)first, C, (long long)event_cap, (const ulonglong2*)ftable, (ulonglong2*)fstore);
  DC_LAUNCHED("cc_track_fields");
  return 0;
}

extern "C" int dc_track_cycles(int event_cap, int track_cap, int step_cap, int C, int min_frames, int class_mask, const int64_t* state,
                               const int64_t* store, const int32_t* track_of, const int64_t* tracks, const int64_t* ntracks,
                               const int64_t* fstore, int64_t* offsets, int64_t* steps, int64_t* step_fields, int64_t* track_fields,
                               int64_t* ncycles, void* workspace, void* stream) {
  if (int rc = tf_check(event_cap, track_cap, C)) return rc;
  DC_REQUIRE(step_cap >= 1, "dc_track_cycles: step_cap must lie in [1, 2^31 - 1]");
  DC_REQUIRE(min_frames >= 0, "dc_track_cycles: min_frames must not be negative");
  DC_REQUIRE(class_mask >= 1 && class_mask <= 6, "dc_track_cycles: class_mask must lie in [1, 6] (bit 1: class 1, bit 2: class 2)");
  DC_REQUIRE(state && store && track_of && tracks && ntracks && fstore && offsets && steps && step_fields && track_fields && ncycles && workspace,
             "dc_track_cycles: null pointer");
  DC_REQUIRE((((uintptr_t)fstore | (uintptr_t)steps | (uintptr_t)step_fields | (uintptr_t)track_fields) & 15) == 0,
             "dc_track_cycles: fstore, steps, step_fields or track_fields not 16-byte aligned");
  DC_REQUIRE(((uintptr_t)workspace & 255) == 0, "dc_track_cycles: workspace not 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t nchunk = ((size_t)track_cap + TK_CHUNK - 1) / TK_CHUNK;
  long long* chunk_cnt = (long long*)workspace;
  long long* chunk_off = (long long*)((char*)workspace + cc_align(nchunk * 16));
  const long long *nt = (const long long*)ntracks, *tr = (const long long*)tracks;
  long long* nc = (long long*)ncycles;
  hipLaunchKernelGGL(tf_count_kernel, dim3((unsigned)nchunk), dim3(256), 0, st, nt, tr, min_frames, class_mask, chunk_cnt);
  DC_LAUNCHED("cc_track_fields");
  hipLaunchKernelGGL(tf_offsets_kernel, dim3(1), dim3(256), 0, st, nt, chunk_cnt, chunk_off, nc);
  DC_LAUNCHED("cc_track_fields");
  hipLaunchKernelGGL(tf_rank_kernel, dim3((unsigned)nchunk), dim3(256), 0, st, nt, tr, min_frames, class_mask, chunk_off, (long long)step_cap,
                     (long long*)offsets, nc);
  DC_LAUNCHED("cc_track_fields");
  const size_t pieces = (size_t)step_cap * (TF_STEP / 2 + (size_t)C * 3) + (size_t)track_cap * C * 2;
  const size_t init_blocks = (pieces + 255) / 256;
  hipLaunchKernelGGL(tf_init_kernel, dim3((unsigned)(init_blocks < (size_t)TF_INIT_BLOCKS ? init_blocks : (size_t)TF_INIT_BLOCKS)), dim3(256), 0, st,
                     C, nt, nc, (ulonglong2*)steps, (ulonglong2*)step_fields, (ulonglong2*)track_fields);
  DC_LAUNCHED("cc_track_fields");
  hipLaunchKernelGGL(tf_event_kernel, dim3((unsigned)(((size_t)event_cap * C + 255) / 256)), dim3(256), 0, st, C, (long long)step_cap,
                     (const long long*)state, (const long long*)store, track_of, tr, (const long long*)offsets, (const ulonglong2*)fstore,
                     (long long*)steps, (unsigned long long*)step_fields);
  DC_LAUNCHED("cc_track_fields");
  const dim3 life((unsigned)(((size_t)step_cap * C + 255) / 256));
  hipLaunchKernelGGL(tf_life_kernel<0>, life, dim3(256), 0, st, C, (long long)track_cap, nc, (const long long*)steps,
                     (const unsigned long long*)step_fields, (unsigned long long*)track_fields);
  DC_LAUNCHED("cc_track_fields");
  hipLaunchKernelGGL(tf_life_kernel<1>, life, dim3(256), 0, st, C, (long long)track_cap, nc, (const long long*)steps,
                     (const unsigned long long*)step_fields, (unsigned long long*)track_fields);
  DC_LAUNCHED("cc_track_fields");
  return 0;
}
