// Event catalogue: connected components of a class mask and their statistics (dc_mask_components, dc_component_stats; nn.EventCatalog).
//
// Classes 1 and 2 are foreground, everything else background.  A component is a maximal set of pixels of ONE class connected under 4- or
// 8-connectivity; with wrap the columns are periodic (column W-1 touches column 0), the rows never are.  Every foreground pixel ends up
// with 1 + the smallest linear index r * W + c of its component (its root), background with 0.
//
// The label map doubles as the parent array of a union-find forest.  The encoding is the final one from the first store on: a word holds
// parent + 1 (0: background), a root holds its own index + 1.  The forest, its invariants I1 and I2 and the argument that every walk and
// every union ends are in event_common.h; here a node is a pixel, a set a component, and a word changes by forest_union's atomicMin or,
// in cc_flatten, to the root a walk from it ended at (I1 and I2 hold for both).  No workgroup waits for another: the order of the
// phases is the order of the launches on one stream.
//   cc_tile     one workgroup labels a TH x TW tile in LDS (union-find on local indices) and stores parent = the tile-local root
//   cc_merge    one thread per pixel on a tile border or on the seam unites it with its neighbours across that border
//   cc_flatten  every pixel's word becomes root + 1
//   cc_stats    roots are flagged, ranked by an order-preserving prefix count per sample, and the ten fields accumulated into row `rank`
#include "event_common.h"

namespace dc {

static constexpr int CC_TPX = CC_TH * CC_TW;      // 10 KiB of LDS in cc_tile
static constexpr int CC_CHUNK = 256;              // pixels per workgroup of the root count and rank passes (one per thread)
static constexpr int CC_SLOTS = 128;              // per-workgroup table of partial sums in the statistics pass
static constexpr int CC_PROBES = 4;

// the tile's forest in LDS (local indices, plain encoding) and the sample's in the label map (sample-local linear indices, parent + 1)
__device__ inline int lds_find(const int* s, int x) { return forest_find<0, __HIP_MEMORY_SCOPE_WORKGROUP>(s, x); }
__device__ inline void lds_union(int* s, int a, int b) { forest_union<0, __HIP_MEMORY_SCOPE_WORKGROUP>(s, a, b); }
__device__ inline int g_find(const int* L, int x) { return forest_find<1, __HIP_MEMORY_SCOPE_AGENT>(L, x); }
__device__ inline void g_union(int* L, int a, int b) { forest_union<1, __HIP_MEMORY_SCOPE_AGENT>(L, a, b); }

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
// roots (total, class 1) of every chunk of CC_CHUNK consecutive pixels
__global__ __launch_bounds__(256) void cc_count_kernel(long HW, const uint8_t* __restrict__ mask, const int* __restrict__ labels, long nchunk,
                                                       int* __restrict__ chunk_cnt) {
  __shared__ int s_w[4];
  const size_t base = (size_t)blockIdx.y * HW;
  const long p = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
  const bool root = p < HW && labels[base + p] == (int)p + 1;
  const bool one = root && mask[base + p] == 1;
  chunk_count(root ? 1 : 0, one ? 1 : 0, s_w, chunk_cnt + ((size_t)blockIdx.y * nchunk + blockIdx.x) * 2);
}

// one workgroup per sample: the chunks' counts become exclusive offsets, the sums go to ncomp
__global__ __launch_bounds__(256) void cc_offsets_kernel(long nchunk, const int* __restrict__ chunk_cnt, int* __restrict__ chunk_off,
                                                         int* __restrict__ ncomp) {
  __shared__ int s_w[4];
  int carry, carry1;
  chunk_offsets(nchunk, chunk_cnt + (size_t)blockIdx.x * nchunk * 2, chunk_off + (size_t)blockIdx.x * nchunk, s_w, &carry, &carry1);
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
  const int rank = event_rank(rank_sample, HW, cap, root);
  if (rank < 0) return;
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
  int r, cb;
  row_walk_origin(&r, &cb);
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
          const int hit = slot_claim<CC_SLOTS, CC_PROBES>(s_key, slot_hash<CC_SLOTS>(a.root), a.root);
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

extern "C" int dc_mask_components(int B, int n_valid, int H, int W, const uint8_t* mask, int connectivity, int wrap, int32_t* labels,
                                  void* workspace, void* stream) {
  DC_REQUIRE(connectivity == 4 || connectivity == 8, "dc_mask_components: connectivity must be 4 or 8");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_mask_components: wrap must be 0 or 1");
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(mask && labels, "dc_mask_components: null pointer");
  (void)workspace;                                // the forest lives in the label map itself
  hipStream_t st = (hipStream_t)stream;
  const int conn8 = connectivity == 8;
  const dim3 tiles = cc_tile_grid(H, W, n_valid);
  hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(256), 0, st, H, W, mask, conn8, labels);
  DC_LAUNCHED("cc_tile");
  const long n_row_items = (long)(tiles.y - 1) * W, n_items = n_row_items + (long)(tiles.x - 1 + (wrap ? 1 : 0)) * H;
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
  hipLaunchKernelGGL(cc_accumulate_kernel, cc_tile_grid(H, W, n_valid), dim3(256), 0, st, H, W, labels, wy, cx, sx, cap, rank_map,
                     (long long*)table);
  DC_LAUNCHED("cc_stats");
  hipLaunchKernelGGL(cc_seam_kernel, dim3((cap + 255) / 256, n_valid), dim3(256), 0, st, cap, (long long*)table);
  DC_LAUNCHED("cc_stats");
  return 0;
}
