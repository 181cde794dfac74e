// What the event kernels share (components.hip, event_shape.hip, event_match.hip, event_fields.hip, tracks.hip, track_match.hip): the tile and the entry
// checks, the union-find forest, the per-workgroup slot table, the rank lookup, the row walk, the block scan and the count / offsets
// compaction.  Everything is inline: a kernel compiles these as it would compile a copy of its own.
#pragma once
#include "common.h"

namespace dc {

static constexpr int CC_TH = 32, CC_TW = 64;      // the tile: 2048 pixels, 8 per thread of a 256-thread workgroup
static constexpr int CC_FIELDS = 10;              // words of a catalogue row
static constexpr int FS_STATS = 6, FS_MAX_C = 32; // words of a field row (min, max, sum, wsum, nonfinite, saturated); channels at most
static constexpr unsigned long long FS_NONE = ~0ull;   // the empty minimum of a field row
// the tracker's tables (tracks.hip fills them, track_match.hip reads them)
static constexpr int TK_STORE = 12, TK_TRACK = 8;  // store row: frame, rank, the catalogue's CC_FIELDS; track row: id, class, events, first, last, pixels, peak, area
static constexpr int TK_CHUNK = 256;               // events per workgroup of the root count and rank passes

__device__ inline int cc_class(uint8_t m) { return (m == 1 || m == 2) ? (int)m : 0; }

// ---- entry checks, the workspace's alignment, the tile grid --------------------------------------------------------------------------
static inline size_t cc_align(size_t v) { return (v + 255) / 256 * 256; }

// the batch of an entry whose grid takes n_valid as its y or z extent
static inline int cc_check_batch(int B, int n_valid) {
  DC_REQUIRE(B > 0, "events: B must be positive");
  DC_REQUIRE(n_valid > 0 && n_valid <= B, "events: n_valid must lie in [1, B]");
  DC_REQUIRE(n_valid <= 65535, "events: at most 65535 samples per call");
  return 0;
}

static inline int cc_check(int B, int n_valid, int H, int W) {
  if (int rc = cc_check_batch(B, n_valid)) return rc;
  DC_REQUIRE(H > 0 && W > 0, "events: H and W must be positive");
  DC_REQUIRE((long)H * W < 2147483647L, "events: H * W must be below 2^31 - 1 (labels are int32)");
  DC_REQUIRE((H + CC_TH - 1) / CC_TH <= 65535, "events: H exceeds 65535 tile rows");
  return 0;
}

// one workgroup per tile of every valid sample
static inline dim3 cc_tile_grid(int H, int W, int n_valid) { return dim3((W + CC_TW - 1) / CC_TW, (H + CC_TH - 1) / CC_TH, n_valid); }

// the rows of sample j that its table holds: min(ncomp, cap)
__device__ inline int event_rows(const int* __restrict__ ncomp, int j, int cap) {
  const int all = ncomp[j * 3];
  return all < 0 ? 0 : (all > cap ? cap : all);
}

// ---- the forest ----------------------------------------------------------------------------------------------------------------------
// A union-find forest over indices 0 .. n - 1 in an int32 array.  A word holds parent + BIAS: BIAS 1 leaves 0 for "no node" (the label
// map: background), BIAS 0 is the plain encoding; a root holds its own index.  SCOPE is the memory scope of the walk's relaxed loads:
// workgroup for a forest in LDS, agent for one in device memory.  Two invariants carry every argument about a forest:
//   (I1) a parent's index is never larger than its child's, and equal only at a root, so every walk towards a root strictly descends and
//        ends by itself, whatever other workgroups do meanwhile and however stale the words it reads are;
//   (I2) every word a node's entry has EVER held names a node of its set, so a walk over old values still ends inside the set.
// Links change by atomicMin only (I1 holds: both candidates are smaller than the child).  When an atomicMin replaces a link a -> old by
// a -> b, forest_union goes on to unite old and b, which restores the equivalence the replaced link stood for (Playne & Hawick 2018,
// Komura 2015).  max(a, b) strictly falls from one round of forest_union to the next, so its loop ends after at most n rounds.  No
// workgroup waits for another.  A file that keeps a forest says how its stores keep I1 and I2; the walks are these two functions.
template <int BIAS, int SCOPE>
__device__ inline int forest_find(const int* P, int x) {
  static_assert(BIAS == 0 || BIAS == 1, "forest_find: a word holds parent or parent + 1");
  for (;;) {
    const int p = __hip_atomic_load(P + x, __ATOMIC_RELAXED, SCOPE) - BIAS;
    if (p >= x || p < 0) return x;      // root (p == x); anything else cannot occur and ends the walk as well
    x = p;
  }
}
template <int BIAS, int SCOPE>
__device__ inline void forest_union(int* P, int a, int b) {
  for (;;) {
    a = forest_find<BIAS, SCOPE>(P, a);
    b = forest_find<BIAS, SCOPE>(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b + BIAS) - BIAS;
    if (old >= a) return;               // a was a root and now hangs below b
    a = old;                            // a had been linked meanwhile: its former parent and b are still to be united
  }
}

// ---- the per-workgroup slot table ----------------------------------------------------------------------------------------------------
// A pixel kernel reduces its tile's runs in LDS before it touches the global rows: SLOTS keys (a power of two), linear probing.  Only the
// claim is shared; the value arrays beside the keys and their flush are each kernel's own.
static constexpr int slot_log2(int slots) { return slots <= 1 ? 0 : 1 + slot_log2(slots >> 1); }

// the start slot of a root: the top log2 SLOTS bits of the multiplicative hash
template <int SLOTS>
__device__ inline int slot_hash(int root) {
  static_assert(SLOTS >= 2 && (1 << slot_log2(SLOTS)) == SLOTS, "slot_hash: the shift leaves log2 SLOTS bits, SLOTS is a power of two");
  return (int)(((unsigned)root * 2654435761u) >> (32 - slot_log2(SLOTS)));
}

// The slot that holds `key` or was empty and now does, within PROBES slots from `start` on; -1: none, the run goes to its global row.
// K: int (empty -1) or unsigned long long (empty ~0); neither is a key.
template <int SLOTS, int PROBES, typename K>
__device__ inline int slot_claim(K* s_key, int start, K key) {
  static_assert((SLOTS & (SLOTS - 1)) == 0, "slot_claim: the probe wraps with a mask");
  constexpr K EMPTY = (K) ~(K)0;
  int s = start, hit = -1;
#pragma unroll
  for (int t = 0; t < PROBES && hit < 0; ++t) {
    const K old = atomicCAS(&s_key[s], EMPTY, key);
    if (old == EMPTY || old == key) hit = s;
    s = (s + 1) & (SLOTS - 1);
  }
  return hit;
}

// the 32 hashed bits of a 64-bit key of an open-addressing table in device memory (event_match.hip, track_match.hip)
__device__ inline unsigned key_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return (unsigned)k;
}

// ---- rank lookup ---------------------------------------------------------------------------------------------------------------------
// the table row of the event whose root pixel is `root` (rank_sample: the sample's slice of dc_component_stats' rank map), -1 where the
// root lies outside the frame or the event beyond the table (counted in ncomp only)
__device__ inline int event_rank(const int* __restrict__ rank_sample, long HW, int cap, int root) {
  if (root < 0 || root >= HW) return -1;
  const int rank = rank_sample[root];
  return rank < 0 || rank >= cap ? -1 : rank;
}

// ---- the row walk --------------------------------------------------------------------------------------------------------------------
// One workgroup per tile, a thread walks 8 consecutive pixels of a row: row *r, columns *cb .. *cb + 7 (either may lie beyond the frame).
// A wave reads 8 rows x 64 consecutive columns.
__device__ inline void row_walk_origin(int* r, int* cb) {
  static_assert(CC_TH == 32 && CC_TW == 64, "row_walk_origin: 4 waves x 8 rows, 8 lanes x 8 columns cover exactly one 32 x 64 tile");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  *r = blockIdx.y * CC_TH + wave * 8 + lane / 8;
  *cb = blockIdx.x * CC_TW + (lane % 8) * 8;
}

// ---- block scan and compaction -------------------------------------------------------------------------------------------------------
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

// Ranking the flagged items of a long array in order takes three passes over chunks of 256 items (one per thread):
//   count    chunk_count: a workgroup per chunk stores the chunk's two totals (the ranked quantity, and a second one that is only summed)
//   offsets  chunk_offsets: ONE workgroup turns the first totals into exclusive offsets and returns both grand totals
//   rank     a workgroup per chunk scans its items again on top of its chunk's offset
template <typename T>
__device__ inline void chunk_count(T v, T v1, T* s_w, T* __restrict__ cnt_pair) {
  T tot, tot1;
  block_excl_scan(v, s_w, &tot);
  block_excl_scan(v1, s_w, &tot1);
  if (threadIdx.x == 0) {
    cnt_pair[0] = tot;
    cnt_pair[1] = tot1;
  }
}
template <typename T>
__device__ inline void chunk_offsets(long long nchunk, const T* __restrict__ cnt, T* __restrict__ off, T* s_w, T* total, T* total1) {
  T carry = 0, carry1 = 0;
  for (long long k0 = 0; k0 < nchunk; k0 += 256) {   // uniform trip count: every thread reaches the barriers inside the scans
    const long long k = k0 + threadIdx.x;
    const T v = k < nchunk ? cnt[2 * k] : 0, v1 = k < nchunk ? cnt[2 * k + 1] : 0;
    T tot, tot1;
    const T ex = block_excl_scan(v, s_w, &tot);
    block_excl_scan(v1, s_w, &tot1);
    if (k < nchunk) off[k] = carry + ex;
    carry += tot;
    carry1 += tot1;
  }
  *total = carry;
  *total1 = carry1;
}

// ---- a field row's atomics -----------------------------------------------------------------------------------------------------------
// one partial result into a field row: min, max, sum, wsum, nonfinite, saturated (event_fields.hip has the encoding)
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

}  // namespace dc
