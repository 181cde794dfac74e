// Per-event statistics of the input fields (dc_component_fields; nn.EventFields).
//
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
#include "event_common.h"

namespace dc {

static constexpr int FS_SLOTS = 32;               // LDS: FS_SLOTS * C * 32 bytes + keys and ranks: 16.2 KiB at C = 16
static constexpr int FS_PROBES = 4;
static constexpr int FS_GROUP = 4;                // channels reduced at a time: one 16-byte load per pixel, 40 registers of partial results

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
  const int k = event_rank(S.rank, S.HW, S.cap, root);
  return k < 0 ? nullptr : S.ftable + ((size_t)k * S.C + ch) * FS_STATS;
}

// a finished run: into the slot of its root, or to the global rows when the table has no room for the root
__device__ inline void fs_flush(const FsSample& S, int* s_key, unsigned long long* s_tab, int root, int g, int nch, const FsRun& a) {
  const int hit = slot_claim<FS_SLOTS, FS_PROBES>(s_key, slot_hash<FS_SLOTS>(root), root);
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
  int r, cb;
  row_walk_origin(&r, &cb);
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
  if (threadIdx.x < FS_SLOTS) s_rank[threadIdx.x] = event_rank(S.rank, S.HW, cap, s_key[threadIdx.x]);   // one lookup per filled slot
  __syncthreads();
  for (int i = threadIdx.x; i < FS_SLOTS * C; i += 256) {
    const int k = s_rank[i / C];
    if (k < 0) continue;
    const unsigned long long* T = s_tab + (size_t)i * 4;
    fs_emit(S.ftable + ((size_t)k * C + i % C) * FS_STATS, T[0], T[1], (long long)T[2], (long long)T[3], 0, 0);
  }
}
static_assert(FS_GROUP == 4, "fs_pixel_kernel: a channel group is one float4");

}  // namespace dc

using namespace dc;

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
  const size_t lds = (size_t)FS_SLOTS * C * 32 + FS_SLOTS * sizeof(int);
  const bool vec = ldc % 4 == 0 && ((uintptr_t)fields & 15) == 0;
  hipLaunchKernelGGL(vec ? fs_pixel_kernel<true> : fs_pixel_kernel<false>, cc_tile_grid(H, W, n_valid), dim3(256), lds, st, H, W, labels, rank_map,
                     cap, fields, C, ldc, scale_bits, wy, (unsigned long long*)ftable);
  DC_LAUNCHED("cc_fields");
  return 0;
}
