// The main course of an event: the longest path through its skeleton by a double sweep (dc_skeleton_course, dc_course_node_cap;
// nn.EventAxis(course=True), nn.EventFilter(axis_measure="course")).  include/deepcam_hip.h has the definitions word for word -- the link
// graph, the three sweeps, the ties; this file has the decomposition.
//
//   co_zero    the rows of the valid samples, so that the course kernel can use them as the per-event workspace of its reductions.
//   co_course  ONE workgroup of 1024 threads per (class, valid sample), as th_thin_kernel and sp_prune_kernel.  It keeps no bit plane: a
//              compact list of at most CO_NODES = 8192 nodes in LDS, so it does not depend on the plane fitting there.
//              build    the frame's skeleton bytes are streamed with 16-byte loads, CO_AHEAD in flight per thread.  A pixel of the class
//                       whose label has a row (event_rank) takes the next id from an LDS counter, records pixel and rank under that id
//                       and writes the id (uint16) to node_ws at the pixel; its event's node count goes through a slot table in LDS
//                       (slot_claim) to column 0 of the row.  The same pass writes the zero bytes of `course`: class 2's workgroup owns
//                       the bytes whose skeleton byte is 2, class 1's all others; a byte that became a node below the cap is written
//                       later by the node's owner and by nobody here, so no byte has two writers.  Node order is the order of the
//                       counter and arbitrary: nothing below depends on it.
//              edges    behind a fence and a barrier thread t owns the nodes t, t + 1024, ... (at most CO_NPT = 8).  It reads the
//                       skeleton byte and label of the node's 8 neighbours (sparse: from L2), applies the diagonal rule, fetches the ids
//                       of the linked neighbours from node_ws and keeps them, two uint16 to a register, with the node's row: 5 VGPRs a
//                       node.  The link table of the frame's rows sits in LDS; a link's weight is read there when it is relaxed.
//              sweep    distances are uint32 in LDS, CO_INF = unreached.  In a round every thread relaxes its own nodes in place,
//                       d[p] = min(d[p], d[q] + w(p, q)) over its links, against neighbours that change meanwhile.
//              hazard   that is sound: a distance only ever decreases, each is written by its owner alone, every value a node ever holds
//                       is the length of some path from the source (so never below the shortest), and a round in which nothing changed
//                       saw every d[p] <= d[q] + w: the shortest distances, which are the only fixed point with d[source] = 0.  After t
//                       rounds every node whose shortest path has at most t links is final whatever the interleaving (induction over t:
//                       its predecessor was final one round earlier and is read at or after that), so `nodes` rounds always suffice.
//                       The result does not depend on the order; the NUMBER of rounds does, and is reported, not specified.  One
//                       barrier a round.  "Anything changed" travels through two words by round parity, as th_subpass's flags do, but
//                       stamped, not cleared: a wave that lowered a distance in round t stores t + 1 to word t & 1 before the round's
//                       barrier, everybody compares behind it.  The word's previous stamp (t - 1) never equals t + 1, its next writers
//                       come behind the barrier of round t + 1 and its readers of round t have passed that barrier by then -- with one
//                       barrier a round a flag that had to be cleared would race with its slowest reader.
//                       All events of the plane are swept at once: they are disconnected.
//              reduce   between the sweeps: the farthest node of every event by a 64-bit atomicMax of (d << 32) | (0xFFFFFFFF - pixel)
//                       into the event's row (ties: the smallest pixel), the start by an atomicMax of 0xFFFFFFFF - pixel.  Only this
//                       workgroup touches the rows of its class, so a fence and a barrier order the atomics before the loads that pick
//                       the next sweep's source.  d_a stays in the owner's registers during the third sweep; then the owner marks its
//                       nodes with d_a + d_b == course_m, counts them into the row, and the start node of every event replaces the
//                       keys in its row by the columns the header names.
//   Registers: 8 nodes x (4 id words + row + d_a) = 48 VGPRs of state; the build's resource report is in DESIGN 7x (no scratch).
//   LDS: pixel, rank and distance of 8192 nodes (96 KiB), the slot table (8 KiB), 12 bytes per row of the frame and 64 of scratch.
// 64-bit integer atomics only; no workgroup waits for another.
#include "skeleton_bits.h"

namespace dc {

static constexpr int CO_THREADS = TH_THREADS;
static constexpr int CO_NPT = 8;                   // nodes a thread owns at most
static constexpr int CO_NODES = CO_THREADS * CO_NPT;
static constexpr int CO_FIELDS = 7;                // nodes, start, start_ecc_m, end_a, end_b, course_pixels, course_m
static constexpr int CO_SLOTS = 1024, CO_PROBES = 4;
static constexpr int CO_AHEAD = 3;                 // 16-byte loads a thread keeps in flight
static constexpr int CO_SCRATCH = 64;              // the node counter and the two stamped words
static constexpr unsigned CO_INF = 0xFFFFFFFFu, CO_NONE = 0xFFFFu;
static_assert(CO_NODES >= 8192 && CO_NODES < (int)CO_NONE, "co_course: a node id is a uint16 and 0xFFFF is no node");
static_assert(CO_SLOTS == CO_THREADS, "co_course: one thread flushes one slot");

static inline size_t co_lds_bytes(int H) {
  const size_t bytes = (size_t)CO_NODES * 12 + (size_t)CO_SLOTS * 8 + (size_t)H * 12 + CO_SCRATCH;
  return bytes <= (size_t)TH_LDS_MAX ? bytes : 0;
}

struct CoFrame {                                   // what the build's pixel step needs, per workgroup
  const uint8_t* S;
  const int* L;
  const int* rank_sample;
  long long* rows;
  uint8_t* C;
  uint16_t* ids;
  int* s_pix;
  int* s_rank;
  int* s_key;
  unsigned* s_cnt;
  int* s_n;
  long HW;
  int cap;
  unsigned cls;
};

// one byte of the stream: v at pixel `pix`.  Writes the zero the workgroup owes `course` there, unless the pixel becomes a node below the cap.
__device__ inline void co_pixel(const CoFrame& f, unsigned v, int pix) {
  if (v != f.cls) {
    if ((v == 2u) == (f.cls == 2u)) f.C[pix] = 0;  // class 1 owns everything that is not 2
    return;
  }
  const int rank = event_rank(f.rank_sample, f.HW, f.cap, f.L[pix] - 1);
  if (rank < 0) {
    f.C[pix] = 0;
    return;
  }
  const int hit = slot_claim<CO_SLOTS, CO_PROBES>(f.s_key, slot_hash<CO_SLOTS>(rank), rank);
  if (hit >= 0) atomicAdd(&f.s_cnt[hit], 1u);
  else atomicAdd((u64*)(f.rows + (size_t)rank * CO_FIELDS), 1ull);
  const int id = atomicAdd(f.s_n, 1);
  if (id < CO_NODES) {
    f.s_pix[id] = pix;
    f.s_rank[id] = rank;
    f.ids[pix] = (uint16_t)id;
  } else {                                         // beyond the cap: the (frame, class) is not measured
    f.C[pix] = 0;
    atomicMin(f.rows + (size_t)rank * CO_FIELDS + 6, -1ll);
  }
}

__device__ inline u64 co_row_load(const long long* p) {
  return (u64)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline unsigned co_d_load(const unsigned* d, unsigned i) {
  return __hip_atomic_load(d + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the atomics and stores of the whole workgroup so far, visible to all its loads from here on
__device__ inline void co_fence_barrier() {
  __threadfence();
  __syncthreads();
  __threadfence();
}

__global__ __launch_bounds__(256) void co_zero_kernel(long n, long long* __restrict__ rows) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) rows[i] = 0;
}

__global__ __launch_bounds__(CO_THREADS) void co_course_kernel(int H, int W, const uint8_t* __restrict__ skeleton,
                                                               const int* __restrict__ labels, const int* __restrict__ rank_map, int cap,
                                                               int wrap, const int* __restrict__ link, long long* __restrict__ rows,
                                                               uint8_t* __restrict__ course, int* __restrict__ status,
                                                               uint16_t* __restrict__ node_ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* s_pix = (int*)smem;
  int* s_rank = s_pix + CO_NODES;
  unsigned* s_d = (unsigned*)(s_rank + CO_NODES);
  int* s_key = (int*)(s_d + CO_NODES);
  unsigned* s_cnt = (unsigned*)(s_key + CO_SLOTS);
  int* s_lt = (int*)(s_cnt + CO_SLOTS);
  int* s_n = s_lt + (size_t)H * 3;
  volatile unsigned* s_stamp = (volatile unsigned*)(s_n + 1);
  const unsigned cls = blockIdx.x + 1;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const long HW = (long)H * W;
  const size_t base = (size_t)b * HW;
  CoFrame f;
  f.S = skeleton + base, f.L = labels + base, f.rank_sample = rank_map + base;
  f.rows = rows + (size_t)b * cap * CO_FIELDS;
  f.C = course + base, f.ids = node_ws + base;
  f.s_pix = s_pix, f.s_rank = s_rank, f.s_key = s_key, f.s_cnt = s_cnt, f.s_n = s_n;
  f.HW = HW, f.cap = cap, f.cls = cls;
  int* st = status + ((size_t)b * 2 + cls - 1) * 3;

  s_key[tid] = -1, s_cnt[tid] = 0u;
  if (tid == 0) *s_n = 0;
  if (tid < 2) s_stamp[tid] = 0u;
  for (int i = tid; i < H * 3; i += CO_THREADS) s_lt[i] = link[i];
  __syncthreads();

  // ---- build: the stream.  [0, head) and [head + 16 nvec, HW) bytewise, the vectors between them aligned to 16 bytes
  {
    const long head = min(HW, (long)((16 - ((uintptr_t)f.S & 15)) & 15));
    const long nvec = (HW - head) / 16;
    const bool vec_store = (((uintptr_t)(f.C + head)) & 15) == 0;
    // fewer than 16 bytes at either end: one each for the first 32 threads, behind their vectors
    const long edge = tid < 16 ? (long)tid : head + nvec * 16 + (tid - 16);
    bool edge_left = tid < 32 && (tid < 16 ? edge < head : edge < HW);
    auto load = [&](long v) { return v < nvec ? ldg16(f.S + head + v * 16) : zero16(); };
    vec16 x0 = load(tid), x1 = load(tid + (long)CO_THREADS), x2 = load(tid + 2l * CO_THREADS);   // CO_AHEAD loads in flight
    long v = tid;
#pragma unroll 1
    for (;;) {
      vec16 x = x0;
      int p0, bytes;
      if (v < nvec) {
        p0 = (int)(head + v * 16), bytes = 16;
        x0 = x1, x1 = x2, x2 = load(v + (long)CO_AHEAD * CO_THREADS);
        v += CO_THREADS;
      } else if (edge_left) {
        p0 = (int)edge, bytes = 1, edge_left = false;
        x.w[0] = f.S[edge];
      } else {
        break;
      }
      if (bytes == 16 && (x.w[0] | x.w[1] | x.w[2] | x.w[3]) == 0u && vec_store) {
        if (cls == 1u) stg16(f.C + p0, zero16());
      } else {
#pragma unroll 1
        for (int k = 0; k < bytes; ++k) {
          const unsigned word = k < 4 ? x.w[0] : (k < 8 ? x.w[1] : (k < 12 ? x.w[2] : x.w[3]));
          co_pixel(f, (word >> ((k & 3) * 8)) & 0xFFu, p0 + k);
        }
      }
    }
  }
  co_fence_barrier();
  const int total = *s_n;
  const int nn = total < CO_NODES ? total : CO_NODES;
  if (s_key[tid] >= 0) atomicAdd((u64*)(f.rows + (size_t)s_key[tid] * CO_FIELDS), (u64)s_cnt[tid]);
  if (total > CO_NODES) {                          // over the cap: nodes and -1 in the rows, no course byte set
    for (int i = tid; i < CO_NODES; i += CO_THREADS) {
      f.C[s_pix[i]] = 0;
      atomicMin(f.rows + (size_t)s_rank[i] * CO_FIELDS + 6, -1ll);
    }
    if (tid == 0) st[0] = total, st[1] = 0, st[2] = 1;
    return;
  }
  if (nn == 0) {
    if (tid == 0) st[0] = 0, st[1] = 0, st[2] = 0;
    return;
  }

  // ---- edges: the ids of the linked neighbours, clockwise from north, two to a word (j even: low half), and the node's row
  unsigned nb[CO_NPT][4];
  int row[CO_NPT];
#pragma unroll
  for (int k = 0; k < CO_NPT; ++k) {
    const int i = tid + k * CO_THREADS;
    nb[k][0] = nb[k][1] = nb[k][2] = nb[k][3] = 0xFFFFFFFFu;
    row[k] = 0;
    if (i < nn) {
      const int pix = s_pix[i];
      const int r = pix / W, c = pix - r * W;
      const int lab = f.L[pix];
      const int dr[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, dc[8] = {0, 1, 1, 1, 0, -1, -1, -1};
      int q[8];
      unsigned n = 0;                              // bit j: neighbour j is a skeleton pixel of this class with this label
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int rr = r + dr[j];
        int cc = c + dc[j];
        if (wrap) cc = cc < 0 ? W - 1 : (cc == W ? 0 : cc);
        q[j] = rr * W + cc;
        if (rr >= 0 && rr < H && cc >= 0 && cc < W && f.S[q[j]] == cls && f.L[q[j]] == lab) n |= 1u << j;
      }
      // a diagonal beside a corner pixel is the corner, not a link (dc_skeleton_stats' rule)
      unsigned e = n & 0x55u;
      if ((n & 0x02u) && !(n & 0x05u)) e |= 0x02u;
      if ((n & 0x08u) && !(n & 0x14u)) e |= 0x08u;
      if ((n & 0x20u) && !(n & 0x50u)) e |= 0x20u;
      if ((n & 0x80u) && !(n & 0x41u)) e |= 0x80u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned id = (e >> j) & 1u ? (unsigned)f.ids[q[j]] : CO_NONE;
        nb[k][j >> 1] = (j & 1) ? (nb[k][j >> 1] & 0x0000FFFFu) | (id << 16) : (nb[k][j >> 1] & 0xFFFF0000u) | id;
      }
      row[k] = r;
      atomicMax((u64*)(f.rows + (size_t)s_rank[i] * CO_FIELDS + 1), (u64)(0xFFFFFFFFu - (unsigned)pix));   // the start: the smallest pixel
    }
  }
  co_fence_barrier();

  // ---- three sweeps: from s, from a, from b
  unsigned da[CO_NPT];
  unsigned t = 0;                                  // rounds run so far, over the sweeps: the stamps never repeat
#pragma unroll 1
  for (int sweep = 0; sweep < 3; ++sweep) {
    const int src_col = sweep == 0 ? 1 : 2 + sweep;  // the key whose low word names the source: start, end_a, end_b
#pragma unroll
    for (int k = 0; k < CO_NPT; ++k) {
      const int i = tid + k * CO_THREADS;
      if (i < nn) {
        const unsigned key = (unsigned)co_row_load(f.rows + (size_t)s_rank[i] * CO_FIELDS + src_col);
        s_d[i] = (0xFFFFFFFFu - key) == (unsigned)s_pix[i] ? 0u : CO_INF;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int round = 0; round < nn; ++round) {
      bool changed = false;
#pragma unroll
      for (int k = 0; k < CO_NPT; ++k) {
        // opaque: the 64 "has a link" tests are the same in every round, and hoisted out of the rounds their lane masks would take 128 SGPRs
        asm volatile("" : "+v"(nb[k][0]), "+v"(nb[k][1]), "+v"(nb[k][2]), "+v"(nb[k][3]));
        const int i = tid + k * CO_THREADS;
        if (i < nn && (nb[k][0] & nb[k][1] & nb[k][2] & nb[k][3]) != 0xFFFFFFFFu) {
          const unsigned d0 = co_d_load(s_d, i);
          unsigned best = d0;
          const int* lt = s_lt + row[k] * 3;
          // the link's weight: E-W on the node's row; N-S and diagonal from the upper end's row
          const int wofs[8] = {-3 + 1, -3 + 2, 0, 2, 1, 2, 0, -3 + 2};
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const unsigned id = (nb[k][j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
            if (id != CO_NONE) {
              const unsigned dq = co_d_load(s_d, id);
              if (dq != CO_INF) {
                const unsigned cand = dq + (unsigned)lt[wofs[j]];
                best = cand < best ? cand : best;
              }
            }
          }
          if (best < d0) {
            __hip_atomic_store(s_d + i, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            changed = true;
          }
        }
      }
      if (__ballot(changed) && lane == 0) s_stamp[t & 1u] = t + 1u;
      __syncthreads();
      const bool more = s_stamp[t & 1u] == t + 1u;
      ++t;
      if (!more) break;
    }
    if (sweep < 2) {                               // the farthest node of every event: end_a after the first sweep, end_b after the second
#pragma unroll
      for (int k = 0; k < CO_NPT; ++k) {
        const int i = tid + k * CO_THREADS;
        da[k] = CO_INF;
        if (i < nn) {
          const unsigned d = s_d[i];
          da[k] = d;
          if (d != CO_INF)
            atomicMax((u64*)(f.rows + (size_t)s_rank[i] * CO_FIELDS + 3 + sweep), ((u64)d << 32) | (u64)(0xFFFFFFFFu - (unsigned)s_pix[i]));
        }
      }
      co_fence_barrier();
    }
  }

  // ---- mark: on some shortest a - b path
#pragma unroll
  for (int k = 0; k < CO_NPT; ++k) {
    const int i = tid + k * CO_THREADS;
    if (i < nn) {
      long long* r = f.rows + (size_t)s_rank[i] * CO_FIELDS;
      const unsigned db = s_d[i];
      const u64 course_m = co_row_load(r + 4) >> 32;
      const bool on = da[k] != CO_INF && db != CO_INF && (u64)da[k] + (u64)db == course_m;
      f.C[s_pix[i]] = on ? (uint8_t)cls : (uint8_t)0;
      if (on) atomicAdd((u64*)(r + 5), 1ull);
    }
  }
  co_fence_barrier();
  // ---- the start node of an event turns the keys of its row into the row's columns
#pragma unroll
  for (int k = 0; k < CO_NPT; ++k) {
    const int i = tid + k * CO_THREADS;
    if (i < nn) {
      long long* r = f.rows + (size_t)s_rank[i] * CO_FIELDS;
      const unsigned start = 0xFFFFFFFFu - (unsigned)co_row_load(r + 1);
      if (start == (unsigned)s_pix[i]) {
        const u64 ka = co_row_load(r + 3), kb = co_row_load(r + 4);
        r[1] = (long long)start;
        r[2] = (long long)(ka >> 32);
        r[3] = (long long)(0xFFFFFFFFu - (unsigned)ka);
        r[4] = (long long)(0xFFFFFFFFu - (unsigned)kb);
        r[6] = (long long)(kb >> 32);
      }
    }
  }
  if (tid == 0) st[0] = nn, st[1] = (int)t, st[2] = 0;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_course_node_cap(void) { return CO_NODES; }

extern "C" int dc_skeleton_course(int B, int n_valid, int H, int W, const uint8_t* skeleton, const int32_t* labels, const void* ws, int cap,
                                  int wrap, const int32_t* link_table, int64_t* rows, uint8_t* course, int32_t* status, void* node_ws,
                                  void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(cap >= 1, "dc_skeleton_course: cap must be at least 1");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_skeleton_course: wrap must be 0 or 1");
  DC_REQUIRE(skeleton && labels && ws && link_table && rows && course && status && node_ws, "dc_skeleton_course: null pointer");
  DC_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)link_table & 3) == 0 && ((uintptr_t)rows & 7) == 0 &&
                 ((uintptr_t)status & 3) == 0 && ((uintptr_t)node_ws & 1) == 0,
             "dc_skeleton_course: a buffer is not aligned to its element size");
  const size_t lds = co_lds_bytes(H);
  DC_REQUIRE(lds != 0, "dc_skeleton_course: the link table of H rows does not fit the LDS beside the node list (H * 12 + 106 560 bytes of 160 KiB)");
  const size_t px = (size_t)B * H * W;
  struct Span { const void* p; size_t n; const char* name; };
  const Span in[] = {{skeleton, px, "skeleton"}, {labels, px * 4, "labels"}, {ws, px * 4, "ws"}, {link_table, (size_t)H * 12, "link_table"}};
  const Span out[] = {{rows, (size_t)B * cap * CO_FIELDS * 8, "rows"}, {course, px, "course"}, {status, (size_t)B * 24, "status"},
                      {node_ws, px * 2, "node_ws"}};
  auto apart = [](const Span& a, const Span& b) {
    return (uintptr_t)a.p + a.n <= (uintptr_t)b.p || (uintptr_t)b.p + b.n <= (uintptr_t)a.p;
  };
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j) DC_REQUIRE(apart(out[i], in[j]), "dc_skeleton_course: an output (rows, course, status, node_ws) overlaps an input");
    for (int j = i + 1; j < 4; ++j) DC_REQUIRE(apart(out[i], out[j]), "dc_skeleton_course: rows, course, status and node_ws may not overlap");
  }
  hipStream_t st = (hipStream_t)stream;
  const long words = (long)n_valid * cap * CO_FIELDS;
  hipLaunchKernelGGL(co_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, words, (long long*)rows);
  DC_LAUNCHED("skel_course");
  DC_ONCE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&co_course_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TH_LDS_MAX));
  hipLaunchKernelGGL(co_course_kernel, dim3(2, n_valid), dim3(CO_THREADS), lds, st, H, W, skeleton, labels, (const int*)ws, cap, wrap,
                     link_table, (long long*)rows, course, status, (uint16_t*)node_ws);
  DC_LAUNCHED("skel_course");
  return 0;
}
