// Overlap of two catalogues (dc_component_overlap, dc_event_scores; nn.EventMatcher).
//
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
#include "event_common.h"

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
  if (root_a < 0 || root_a >= S.HW || root_b < 0 || root_b >= S.HW) return;     // both roots first: the two lookups are then plain loads
  const int ra = event_rank(S.rank_a, S.HW, S.cap_a, root_a), rb = event_rank(S.rank_b, S.HW, S.cap_b, root_b);   // in flight together
  const bool in_a = ra >= 0, in_b = rb >= 0;
  if (same) {                                     // whatever becomes of the pair: the other side's component may be beyond its table
    if (in_a) atomicAdd(S.cover_a + ra, (unsigned long long)n);
    if (in_b) atomicAdd(S.cover_b + rb, (unsigned long long)n);
  }
  if (!in_a || !in_b) return;
  const unsigned long long key = (((unsigned long long)ra << 32) | (unsigned)rb) + 1ull;
  unsigned h = key_hash(key) & S.slot_mask;
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
  int r, cb;
  row_walk_origin(&r, &cb);
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
          const int hit = slot_claim<OV_SLOTS, OV_PROBES>(s_key, (int)(key_hash(cur) >> (32 - slot_log2(OV_SLOTS))), cur);
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
static_assert(OV_SLOTS == 256, "ov_pixel_kernel: one LDS slot per thread, a power of two for the start slot's shift");

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
  const int rows = event_rows(ncomp, b, cap);
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

using namespace dc;

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
  hipLaunchKernelGGL(ov_pixel_kernel, cc_tile_grid(H, W, n_valid), dim3(256), 0, st, H, W, mask_a, labels_a, rank_a, cap_a, mask_b, labels_b, rank_b,
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
