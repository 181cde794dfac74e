// Predicted against labelled storm tracks (dc_track_match_append, dc_track_match_resolve; nn.TrackMatcher).
//
// The join of three things the device already holds: the pair table of one EventMatcher call (which event of catalogue a shares pixels
// with which of catalogue b, per frame), the event numbers the two trackers gave those events (`first`), and -- when results are read --
// the track rows of both trackers (`track_of`).  An overlap of two events of the same class is filed as a LINK (event a, event b, shared
// pixels) in a store that lives across calls; the resolve groups the links by (track row a, track row b).
//   tm_file     (append) one thread per stored row of a frame's pair table: the two event numbers, the two classes from the trackers'
//               stores, a ticket from the counter, the row.  A thread whose ticket lies beyond the store gives it back and counts the
//               link as dropped: tickets below link_cap are drawn exactly once each (no ticket beyond is drawn before every one below
//               is, and the count only falls back to link_cap), so state[0] ends as min(all, link_cap) whatever the order.
//   tm_count, tm_offsets, tm_rank    (resolve) the step offsets of both sides, blockIdx.y the side: a track's frames are an interval, so
//               its (track, frame) steps are the frames[t] bytes from off[t] on, off the prefix sum over the track rows by the count /
//               offsets / rank passes of event_common.h.  The steps of a side number at most its stored events.
//   tm_link     one thread per stored link: marks the step of each side with a plain byte store (every writer stores the same 1), adds the
//               shared pixels per track, finds or opens the (row a, row b) slot of the pair table and adds there; then claims the
//               (pair slot, frame) key of the frame table, and the ONE thread whose compare-and-swap opens that key adds 1 to the pair's
//               common frames.
//   tm_sum      one thread per track row: the marked steps of its interval, the scores (one atomic per workgroup and counter)
//   tm_compact  one thread per ticket writes its slot as a row
// The pair table has at least 2 * pair_cap slots and a key is probed through ALL of them before it is given up, as in event_match.hip:
// with at most pair_cap distinct pairs every one finds a slot.  The frame table has at least 2 * link_cap slots for at most link_cap keys:
// it never fills.  Minimum, maximum, integer addition and idempotent stores only: apart from the order of the rows (and, with overflow,
// which rows are kept) no result depends on the order of arrival.  The pass is bound by the latency of its dependent atomics, not by
// bandwidth; nothing is staged in LDS.
#include "event_common.h"

namespace dc {

static constexpr int TM_LINK = 3, TM_PAIR = 8, TM_SLOT = 6;   // link row; track-pair row; pair slot: key, overlaps, common, shared, ~first, last
static constexpr int TM_LINK_CAP_MAX = 1 << 26, TM_PAIR_CAP_MAX = 1 << 24;

static inline size_t tm_slots(size_t rows) {      // a power of two, at least twice the rows
  size_t s = 16;
  while (s < 2 * rows) s <<= 1;
  return s;
}

__global__ __launch_bounds__(256) void tm_file_kernel(int cap_a, int cap_b, int pair_cap, const long long* __restrict__ pairs,
                                                      const int* __restrict__ npairs, const int* __restrict__ ncomp_a,
                                                      const long long* __restrict__ first_a, long long event_cap_a,
                                                      const long long* __restrict__ store_a, const int* __restrict__ ncomp_b,
                                                      const long long* __restrict__ first_b, long long event_cap_b,
                                                      const long long* __restrict__ store_b, long long link_cap, long long* __restrict__ links,
                                                      unsigned long long* state) {
  const int j = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    atomicAdd(state + 2, 1ull);
    if (npairs[j * 2 + 1] != 0 || ncomp_a[j * 3] > cap_a || ncomp_b[j * 3] > cap_b) atomicAdd(state + 3, 1ull);
  }
  const int stored = npairs[j * 2];
  if (i >= stored || i >= pair_cap) return;
  const long long* row = pairs + ((size_t)j * pair_cap + i) * 3;
  const long long ra = row[0], rb = row[1], shared = row[2];
  if (ra < 0 || ra >= event_rows(ncomp_a, j, cap_a) || rb < 0 || rb >= event_rows(ncomp_b, j, cap_b)) return;   // no event of its catalogue
  const long long ea = first_a[j] + ra, eb = first_b[j] + rb;
  if (ea < 0 || ea >= event_cap_a || eb < 0 || eb >= event_cap_b) return;                                      // not stored
  const long long cls = store_a[ea * TK_STORE + 3];
  if ((cls != 1 && cls != 2) || store_b[eb * TK_STORE + 3] != cls) return;                                       // the pair table lists every class
  const unsigned long long ticket = atomicAdd(state + 0, 1ull);
  if (ticket >= (unsigned long long)link_cap) {
    atomicAdd(state + 0, ~0ull);                   // the ticket goes back: the count ends at link_cap
    atomicAdd(state + 1, 1ull);
    return;
  }
  long long* out = links + ticket * TM_LINK;
  out[0] = ea;
  out[1] = eb;
  out[2] = shared;
}

struct TmSide {                                    // one tracker's resolved tables and this side's slices of the workspace
  const int* track_of;
  const long long *tracks, *ntracks;
  long long *off, *chunk_cnt, *chunk_off;          // off: the first step of every track row
  uint8_t* flags;                                  // one byte per step
  unsigned long long* cover;                       // [track_cap][2]: matched frames, shared pixels
  long long event_cap;
  int track_cap;
};
struct TmSides {
  TmSide s[2];
};

// the stored rows of a side, and the frames of row t (0 beyond them)
__device__ inline long long tm_rows(const TmSide& S) {
  const long long n = S.ntracks[3];
  return n < 0 ? 0 : (n > S.track_cap ? (long long)S.track_cap : n);
}
__device__ inline long long tm_frames(const TmSide& S, long long t) {
  if (t >= tm_rows(S)) return 0;
  const long long n = S.tracks[(size_t)t * TK_TRACK + 4] - S.tracks[(size_t)t * TK_TRACK + 3] + 1;
  return n < 0 ? 0 : n;
}

__global__ __launch_bounds__(256) void tm_count_kernel(TmSides P) {
  __shared__ long long s_w[4];
  const TmSide& S = P.s[blockIdx.y];
  if ((long long)blockIdx.x * TK_CHUNK >= tm_rows(S)) return;          // the whole workgroup: tm_offsets reads the live chunks only
  chunk_count<long long>(tm_frames(S, (long long)blockIdx.x * TK_CHUNK + threadIdx.x), 0, s_w, S.chunk_cnt + (size_t)blockIdx.x * 2);
}

__global__ __launch_bounds__(256) void tm_offsets_kernel(TmSides P) {
  __shared__ long long s_w[4];
  const TmSide& S = P.s[blockIdx.y];
  long long carry, carry1;
  chunk_offsets((tm_rows(S) + TK_CHUNK - 1) / TK_CHUNK, S.chunk_cnt, S.chunk_off, s_w, &carry, &carry1);
}

__global__ __launch_bounds__(256) void tm_rank_kernel(TmSides P) {
  __shared__ long long s_w[4];
  const TmSide& S = P.s[blockIdx.y];
  if ((long long)blockIdx.x * TK_CHUNK >= tm_rows(S)) return;
  const long long t = (long long)blockIdx.x * TK_CHUNK + threadIdx.x;
  long long tot;
  const long long off = S.chunk_off[blockIdx.x] + block_excl_scan<long long>(tm_frames(S, t), s_w, &tot);
  if (t < tm_rows(S)) S.off[t] = off;
}

// the step of (track row t, frame) of a side: marked, and the shared pixels added to the track
__device__ inline void tm_mark(const TmSide& S, int t, long long frame, unsigned long long shared) {
  const long long d = frame - S.tracks[(size_t)t * TK_TRACK + 3], i = S.off[t] + d;
  if (d >= 0 && d < tm_frames(S, t) && i >= 0 && i < S.event_cap) S.flags[i] = 1;       // never outside: the frame lies in its track's interval
  atomicAdd(S.cover + (size_t)t * 2 + 1, shared);
}

__global__ __launch_bounds__(256) void tm_link_kernel(TmSides P, const long long* __restrict__ state, const long long* __restrict__ links,
                                                      long long link_cap, const long long* __restrict__ store_a, unsigned long long* ptab,
                                                      unsigned pmask, unsigned long long* ftab, unsigned fmask, unsigned* opened,
                                                      int* __restrict__ ticket_slot, int pair_cap, unsigned long long* counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = state[0];
  if (i >= n || i >= link_cap) return;
  const TmSide &A = P.s[0], &B = P.s[1];
  const long long ea = links[i * TM_LINK + 0], eb = links[i * TM_LINK + 1];
  const unsigned long long shared = (unsigned long long)links[i * TM_LINK + 2];
  if (ea < 0 || ea >= A.event_cap || eb < 0 || eb >= B.event_cap) return;               // cannot occur: the append stores stored events only
  const int ta = A.track_of[ea], tb = B.track_of[eb];
  if (ta < 0 || ta >= tm_rows(A) || tb < 0 || tb >= tm_rows(B)) {                       // a track without a row
    atomicAdd(counts + 2, 1ull);
    return;
  }
  const long long frame = store_a[ea * TK_STORE + 0];                                   // both events lie in this frame
  tm_mark(A, ta, frame, shared);
  tm_mark(B, tb, frame, shared);
  const unsigned long long key = (((unsigned long long)(unsigned)ta << 32) | (unsigned)tb) + 1ull;
  unsigned h = key_hash(key) & pmask;
  bool found = false;
  for (unsigned t = 0; t <= pmask; ++t) {
    unsigned long long* s = ptab + (size_t)h * TM_SLOT;
    unsigned long long k = __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0ull) {
      k = atomicCAS(s, 0ull, key);
      if (k == 0ull) {
        k = key;
        const unsigned ticket = atomicAdd(opened, 1u);
        if (ticket < (unsigned)pair_cap) ticket_slot[ticket] = (int)h;
      }
    }
    if (k == key) {
      found = true;
      break;
    }
    h = (h + 1) & pmask;
  }
  if (!found) return;                              // every slot holds another pair: more than pair_cap pairs, the flag is raised
  unsigned long long* s = ptab + (size_t)h * TM_SLOT;
  atomicAdd(s + 1, 1ull);
  atomicAdd(s + 3, shared);
  atomicMax(s + 4, 0xffffffffull - ((unsigned long long)frame & 0xffffffffull));        // the smallest frame: an empty word is 0
  atomicMax(s + 5, (unsigned long long)frame);
  const unsigned long long fkey = (((unsigned long long)h << 32) | ((unsigned long long)frame & 0xffffffffull)) + 1ull;
  unsigned g = key_hash(fkey) & fmask;
  for (unsigned t = 0; t <= fmask; ++t) {          // at most link_cap keys in at least 2 * link_cap slots: ends at an empty slot or its own
    unsigned long long k = __hip_atomic_load(ftab + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0ull) {
      k = atomicCAS(ftab + g, 0ull, fkey);
      if (k == 0ull) {
        atomicAdd(s + 2, 1ull);                    // the opener of (pair, frame): one per distinct common frame
        return;
      }
    }
    if (k == fkey) return;
    g = (g + 1) & fmask;
  }
}

__global__ __launch_bounds__(256) void tm_sum_kernel(TmSides P, int min_frames, int cover_q, unsigned long long* scores) {
  __shared__ unsigned s_n[4];                      // class 1: unmatched, matched; class 2: unmatched, matched
  const TmSide& S = P.s[blockIdx.y];
  if ((long long)blockIdx.x * 256 >= tm_rows(S)) return;
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0u;
  __syncthreads();
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long frames = tm_frames(S, t);
  if (t < tm_rows(S)) {
    const long long off = S.off[t];
    long long matched = 0;
    if (off >= 0 && off + frames <= S.event_cap)
      for (long long d = 0; d < frames; ++d) matched += S.flags[off + d];
    S.cover[(size_t)t * 2] = (unsigned long long)matched;
    const long long cls = S.tracks[(size_t)t * TK_TRACK + 1];
    if ((cls == 1 || cls == 2) && frames >= (min_frames < 1 ? 1 : min_frames))
      atomicAdd(&s_n[(cls == 2 ? 2 : 0) + ((matched >= 1 && matched * 1024 >= (long long)cover_q * frames) ? 1 : 0)], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_n[threadIdx.x]) {       // side b: hits (0), misses (1); side a: false alarms (2), matched detections (3)
    const int cls = threadIdx.x >> 1, hit = threadIdx.x & 1;
    const int field = blockIdx.y == 1 ? (hit ? 0 : 1) : (hit ? 3 : 2);
    atomicAdd(scores + cls * 4 + field, (unsigned long long)s_n[threadIdx.x]);
  }
}

__global__ __launch_bounds__(256) void tm_compact_kernel(const unsigned long long* __restrict__ ptab, unsigned pmask,
                                                         const unsigned* __restrict__ opened, const int* __restrict__ ticket_slot, int pair_cap,
                                                         const long long* __restrict__ tracks_a, long long* __restrict__ tpairs,
                                                         long long* counts) {
  const unsigned n = *opened;
  const int stored = n < (unsigned)pair_cap ? (int)n : pair_cap;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    counts[0] = stored;
    counts[1] = n > (unsigned)pair_cap ? 1 : 0;
  }
  if (i >= stored) return;
  const unsigned h = (unsigned)ticket_slot[i];
  if (h > pmask) return;
  const unsigned long long* s = ptab + (size_t)h * TM_SLOT;
  const unsigned long long key = s[0] - 1ull;
  long long* out = tpairs + (size_t)i * TM_PAIR;
  out[0] = (long long)(key >> 32);
  out[1] = (long long)(key & 0xffffffffull);
  out[2] = tracks_a[(size_t)(key >> 32) * TK_TRACK + 1];
  out[3] = (long long)s[1];
  out[4] = (long long)s[2];
  out[5] = (long long)s[3];
  out[6] = (long long)(0xffffffffull - s[4]);
  out[7] = (long long)s[5];
}

static bool tm_caps_ok(int event_cap_a, int event_cap_b, int track_cap_a, int track_cap_b, int link_cap, int pair_cap) {
  return event_cap_a >= 1 && event_cap_a <= (1 << 30) && event_cap_b >= 1 && event_cap_b <= (1 << 30) && track_cap_a >= 1 &&
         track_cap_a <= event_cap_a && track_cap_b >= 1 && track_cap_b <= event_cap_b && link_cap >= 1 && link_cap <= TM_LINK_CAP_MAX &&
         pair_cap >= 1 && pair_cap <= TM_PAIR_CAP_MAX;
}

// the workspace: what a resolve clears -- ptab | ftab | opened | flags a | flags b -- then ticket_slot | per side off, chunk_cnt, chunk_off
struct TmLayout {
  size_t ptab, ftab, opened, flags[2], cleared, ticket, off[2], cnt[2], coff[2], total;
  size_t pslots, fslots;
};
static TmLayout tm_layout(int event_cap_a, int event_cap_b, int track_cap_a, int track_cap_b, int link_cap, int pair_cap) {
  TmLayout L;
  const int event_cap[2] = {event_cap_a, event_cap_b}, track_cap[2] = {track_cap_a, track_cap_b};
  L.pslots = tm_slots((size_t)pair_cap);
  L.fslots = tm_slots((size_t)link_cap);
  size_t at = 0;
  L.ptab = at, at += cc_align(L.pslots * TM_SLOT * 8);
  L.ftab = at, at += cc_align(L.fslots * 8);
  L.opened = at, at += cc_align(4);
  for (int k = 0; k < 2; ++k) L.flags[k] = at, at += cc_align((size_t)event_cap[k]);
  L.cleared = at;
  L.ticket = at, at += cc_align((size_t)pair_cap * 4);
  for (int k = 0; k < 2; ++k) {
    const size_t nchunk = ((size_t)track_cap[k] + TK_CHUNK - 1) / TK_CHUNK;
    L.off[k] = at, at += cc_align((size_t)track_cap[k] * 8);
    L.cnt[k] = at, at += cc_align(nchunk * 16);
    L.coff[k] = at, at += cc_align(nchunk * 8);
  }
  L.total = at;
  return L;
}

}  // namespace dc

using namespace dc;

extern "C" size_t dc_track_match_workspace(int event_cap_a, int event_cap_b, int track_cap_a, int track_cap_b, int link_cap, int pair_cap) {
  if (!tm_caps_ok(event_cap_a, event_cap_b, track_cap_a, track_cap_b, link_cap, pair_cap)) return 0;
  return tm_layout(event_cap_a, event_cap_b, track_cap_a, track_cap_b, link_cap, pair_cap).total;
}

extern "C" int dc_track_match_append(int B, int n_valid, int cap_a, int cap_b, int pair_cap, const int64_t* pairs, const int32_t* npairs,
                                     const int32_t* ncomp_a, const int64_t* first_a, int event_cap_a, const int64_t* store_a,
                                     const int32_t* ncomp_b, const int64_t* first_b, int event_cap_b, const int64_t* store_b, int link_cap,
                                     int64_t* links, int64_t* state, void* stream) {
  if (int rc = cc_check_batch(B, n_valid)) return rc;
  DC_REQUIRE(cap_a >= 1 && cap_a <= (1 << 22) && cap_b >= 1 && cap_b <= (1 << 22), "dc_track_match_append: cap_a and cap_b must lie in [1, 2^22]");
  DC_REQUIRE(tm_caps_ok(event_cap_a, event_cap_b, 1, 1, link_cap, pair_cap),
             "dc_track_match_append: event_cap must lie in [1, 2^30], link_cap in [1, 2^26], pair_cap in [1, 2^24]");
  DC_REQUIRE(pairs && npairs && ncomp_a && first_a && store_a && ncomp_b && first_b && store_b && links && state,
             "dc_track_match_append: null pointer");
  hipLaunchKernelGGL(tm_file_kernel, dim3((pair_cap + 255) / 256, n_valid), dim3(256), 0, (hipStream_t)stream, cap_a, cap_b, pair_cap,
                     (const long long*)pairs, npairs, ncomp_a, (const long long*)first_a, (long long)event_cap_a, (const long long*)store_a,
                     ncomp_b, (const long long*)first_b, (long long)event_cap_b, (const long long*)store_b, (long long)link_cap,
                     (long long*)links, (unsigned long long*)state);
  DC_LAUNCHED("cc_track_match");
  return 0;
}

extern "C" int dc_track_match_resolve(int event_cap_a, int event_cap_b, int track_cap_a, int track_cap_b, int link_cap, int pair_cap,
                                      int min_frames, int cover_q, const int64_t* state, const int64_t* links, const int64_t* store_a,
                                      const int32_t* track_of_a, const int64_t* tracks_a, const int64_t* ntracks_a, const int32_t* track_of_b,
                                      const int64_t* tracks_b, const int64_t* ntracks_b, int64_t* tpairs, int64_t* cover_a, int64_t* cover_b,
                                      int64_t* scores, int64_t* counts, void* workspace, void* stream) {
  DC_REQUIRE(tm_caps_ok(event_cap_a, event_cap_b, track_cap_a, track_cap_b, link_cap, pair_cap),
             "dc_track_match_resolve: event_cap must lie in [1, 2^30], track_cap in [1, event_cap], link_cap in [1, 2^26], pair_cap in [1, 2^24]");
  DC_REQUIRE(min_frames >= 0, "dc_track_match_resolve: min_frames must not be negative");
  DC_REQUIRE(cover_q >= 1 && cover_q <= 1024, "dc_track_match_resolve: cover_q must lie in [1, 1024]");
  DC_REQUIRE(state && links && store_a && track_of_a && tracks_a && ntracks_a && track_of_b && tracks_b && ntracks_b && tpairs && cover_a &&
                 cover_b && scores && counts && workspace,
             "dc_track_match_resolve: null pointer");
  DC_REQUIRE(((uintptr_t)workspace & 255) == 0, "dc_track_match_resolve: workspace not 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const TmLayout L = tm_layout(event_cap_a, event_cap_b, track_cap_a, track_cap_b, link_cap, pair_cap);
  char* ws = (char*)workspace;
  TmSides P;
  const int32_t* track_of[2] = {track_of_a, track_of_b};
  const int64_t *tracks[2] = {tracks_a, tracks_b}, *ntracks[2] = {ntracks_a, ntracks_b};
  int64_t* cover[2] = {cover_a, cover_b};
  const int event_cap[2] = {event_cap_a, event_cap_b}, track_cap[2] = {track_cap_a, track_cap_b};
  for (int k = 0; k < 2; ++k) {
    TmSide& S = P.s[k];
    S.track_of = track_of[k];
    S.tracks = (const long long*)tracks[k];
    S.ntracks = (const long long*)ntracks[k];
    S.off = (long long*)(ws + L.off[k]);
    S.chunk_cnt = (long long*)(ws + L.cnt[k]);
    S.chunk_off = (long long*)(ws + L.coff[k]);
    S.flags = (uint8_t*)(ws + L.flags[k]);
    S.cover = (unsigned long long*)cover[k];
    S.event_cap = event_cap[k];
    S.track_cap = track_cap[k];
  }
  hipError_t e = hipMemsetAsync(ws, 0, L.cleared, st);
  if (e == hipSuccess) e = hipMemsetAsync(tpairs, 0, (size_t)pair_cap * TM_PAIR * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(cover_a, 0, (size_t)track_cap_a * 2 * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(cover_b, 0, (size_t)track_cap_b * 2 * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(scores, 0, 8 * sizeof(int64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const int max_tracks = track_cap_a > track_cap_b ? track_cap_a : track_cap_b;
  const dim3 chunks((unsigned)(((size_t)max_tracks + TK_CHUNK - 1) / TK_CHUNK), 2);
  hipLaunchKernelGGL(tm_count_kernel, chunks, dim3(256), 0, st, P);
  DC_LAUNCHED("cc_track_match");
  hipLaunchKernelGGL(tm_offsets_kernel, dim3(1, 2), dim3(256), 0, st, P);
  DC_LAUNCHED("cc_track_match");
  hipLaunchKernelGGL(tm_rank_kernel, chunks, dim3(256), 0, st, P);
  DC_LAUNCHED("cc_track_match");
  unsigned long long* ptab = (unsigned long long*)(ws + L.ptab);
  unsigned* opened = (unsigned*)(ws + L.opened);
  int* ticket_slot = (int*)(ws + L.ticket);
  hipLaunchKernelGGL(tm_link_kernel, dim3((unsigned)(((size_t)link_cap + 255) / 256)), dim3(256), 0, st, P, (const long long*)state,
                     (const long long*)links, (long long)link_cap, (const long long*)store_a, ptab, (unsigned)(L.pslots - 1),
                     (unsigned long long*)(ws + L.ftab), (unsigned)(L.fslots - 1), opened, ticket_slot, pair_cap, (unsigned long long*)counts);
  DC_LAUNCHED("cc_track_match");
  hipLaunchKernelGGL(tm_sum_kernel, chunks, dim3(256), 0, st, P, min_frames, cover_q, (unsigned long long*)scores);
  DC_LAUNCHED("cc_track_match");
  hipLaunchKernelGGL(tm_compact_kernel, dim3((pair_cap + 255) / 256), dim3(256), 0, st, (const unsigned long long*)ptab, (unsigned)(L.pslots - 1),
                     (const unsigned*)opened, (const int*)ticket_slot, pair_cap, (const long long*)tracks_a, (long long*)tpairs,
                     (long long*)counts);
  DC_LAUNCHED("cc_track_match");
  return 0;
}
