// Event tracks (dc_track_append, dc_track_link, dc_track_resolve; nn.EventTracker) and, in this file's second half, the storm life
// cycles that read the tracker's store (dc_track_fields_append, dc_track_cycles; nn.TrackFields).
//
// The events of a time series, numbered in the order frames and ranks arrive, and a union-find forest over those numbers: two events
// of consecutive frames that share a pixel of their class are united, a track is a tree.  `parent` is int32 [event_cap] in the plain
// encoding of event_common.h's forest (a root names itself); its two invariants hold here because:
//   (I1) dc_track_append writes parent[e] = e before any launch on the stream can meet e, and afterwards an entry changes by atomicMin
//        only (tk_union) or, in tk_flatten, to the root a walk from it ended at; both are smaller than the entry's index or equal to
//        what it held.  A link joins an event with one of the frame before, whose number is smaller (the numbers grow with the frames),
//        and unites the two ROOTS, the larger below the smaller: every link goes to a smaller number, every walk descends and ends.
//   (I2) every value parent[e] ever held names an event of e's track: itself, a root it was united with, or the root of a later walk.
// So it does not matter whether the entries of earlier calls are flattened, partly flattened (a resolve in the middle of the series) or
// as the unions left them: a union through them still ends at the two current roots.  The state survives from call to call in device
// memory; nothing is read on the host.
//   tk_first    one workgroup: the prefix sum of min(ncomp, cap) over the batch's frames on top of the events seen so far, the counters
//   tk_fill     16 threads per new event: its row of the store (frame, rank, the ten catalogue columns) and parent[e] = e
//   tk_link     one thread per 4 consecutive pixels of a frame pair, both masks as one word each where the layout allows; labels and ranks
//               are read only where both masks hold the same class 1 or 2.  A thread skips a pixel whose two labels equal those of the
//               foreground pixel before it (its own, or the last one of its left lane): a run costs one union.  A repeated union that
//               slips through is two finds and no atomic.
//   tk_flatten, tk_count, tk_offsets, tk_rank, tk_gather    (resolve) every entry becomes its root, the roots are ranked in order by
//               the count / offsets / rank passes of event_common.h, and every event adds itself to its track's row with 64-bit integer
//               atomics (sums and unsigned maxima: no result depends on the order of arrival).  A track's root is its smallest event
//               number, so its id, its class and its first frame are the root's own and need no atomic.
#include "event_common.h"

namespace dc {

static constexpr unsigned long long TK_NONE = ~0ull;
static_assert(TK_STORE == CC_FIELDS + 2, "tk_fill_kernel: a store row is (frame, rank) and a catalogue row");

__device__ inline int tk_find(const int* P, int x) { return forest_find<0, __HIP_MEMORY_SCOPE_AGENT>(P, x); }
__device__ inline void tk_union(int* P, int a, int b) { forest_union<0, __HIP_MEMORY_SCOPE_AGENT>(P, a, b); }

__global__ __launch_bounds__(256) void tk_first_kernel(int n_valid, int cap, const int* __restrict__ ncomp, long long event_cap, long long* state,
                                                       long long* __restrict__ first) {
  __shared__ int s_w[4];
  __shared__ long long s_base;
  if (threadIdx.x == 0) s_base = state[0] + state[2];
  __syncthreads();
  const long long base = s_base;
  long long carry = 0, cut = 0;
  // not chunk_offsets: the values are computed, not read as pairs, and int scans feed int64 sums on top of a base
  for (int j0 = 0; j0 < n_valid; j0 += 256) {      // uniform trip count: every thread reaches the barriers inside the scans
    const int j = j0 + threadIdx.x;
    const int v = j < n_valid ? event_rows(ncomp, j, cap) : 0, t = j < n_valid && ncomp[j * 3] > cap ? 1 : 0;
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
  if (k >= event_rows(ncomp, j, cap) || f >= TK_STORE) return;
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
  if (root_a < 0 || root_a >= S.HW || root_b < 0 || root_b >= S.HW) return;     // both roots first: the two lookups are then plain loads
  const int ra = event_rank(S.rank_a, S.HW, S.cap, root_a), rb = event_rank(S.rank_b, S.HW, S.cap, root_b);   // in flight together
  if (ra < 0 || rb < 0) return;                                                 // no row in its frame's table: no event
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
  chunk_count(root ? 1 : 0, one ? 1 : 0, s_w, chunk_cnt + (size_t)blockIdx.x * 2);
}

// one workgroup: the live chunks' counts become exclusive offsets, the sums go to ntracks
__global__ __launch_bounds__(256) void tk_offsets_kernel(const long long* __restrict__ state, const int* __restrict__ chunk_cnt,
                                                         int* __restrict__ chunk_off, long long track_cap, long long* __restrict__ ntracks) {
  __shared__ int s_w[4];
  int carry, carry1;
  chunk_offsets((state[0] + TK_CHUNK - 1) / TK_CHUNK, chunk_cnt, chunk_off, s_w, &carry, &carry1);
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

// the two append entries: a batch of frames and their catalogue's rows
static int tk_check_append(int B, int n_valid, int cap, int event_cap) {
  if (int rc = cc_check_batch(B, n_valid)) return rc;
  DC_REQUIRE(cap >= 1 && cap <= (1 << 22), "tracks: cap must lie in [1, 2^22]");
  return tk_check_caps(event_cap);
}

}  // namespace dc

using namespace dc;

// the workspace: row_of int32 [event_cap] | chunk_cnt int32 [nchunk][2] | chunk_off int32 [nchunk]
extern "C" size_t dc_track_workspace(int event_cap) {
  if (event_cap < 1 || event_cap > (1 << 30)) return 0;
  const size_t nchunk = ((size_t)event_cap + TK_CHUNK - 1) / TK_CHUNK;
  return cc_align((size_t)event_cap * 4) + cc_align(nchunk * 8) + cc_align(nchunk * 4);
}

extern "C" int dc_track_append(int B, int n_valid, int cap, const int64_t* table, const int32_t* ncomp, long frame0, int event_cap,
                               int64_t* state, int64_t* first, int32_t* parent, int64_t* store, void* stream) {
  if (int rc = tk_check_append(B, n_valid, cap, event_cap)) return rc;
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
  hipLaunchKernelGGL(vec ? tk_link_kernel<true> : tk_link_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, HW, mask_a, labels_a, rank_a,
                     (const long long*)first_a, mask_b, labels_b, rank_b, (const long long*)first_b, cap, (long long)event_cap,
                     (long long)min_pixels, (const long long*)store, parent);
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
// The join of the tracker above and the field rows of event_fields.hip: dc_track_fields_append files every event's field rows (dc_component_fields) under its event number,
// next to the tracker's store, and dc_track_cycles groups them by (track, frame) when life cycles are read.  Links join consecutive
// frames only, so the frames of a track form an interval and every one of them holds an event of the track: the step rows of track row t
// are the frames[t] = last - first + 1 rows from offsets[t] on, offsets a prefix sum over the selected track rows.  No sort, no search.
// A row is stored iff it ends inside step_cap; the offsets grow with t, so the stored rows are a prefix of the selected ones and the
// stored step rows are exactly the first ncycles[2].
//   tf_file     (append) one thread per 16 bytes of a new event's field rows
//   tf_count, tf_offsets, tf_rank    the prefix sum of the selected rows' frame counts by the count / offsets / rank passes again, in
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
  if (k >= event_rows(ncomp, j, cap)) return;
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
  chunk_count<long long>(v, v > 0 ? 1 : 0, s_w, chunk_cnt + (size_t)blockIdx.x * 2);
}

__global__ __launch_bounds__(256) void tf_offsets_kernel(const long long* __restrict__ ntracks, const long long* __restrict__ chunk_cnt,
                                                         long long* __restrict__ chunk_off, long long* __restrict__ ncycles) {
  __shared__ long long s_w[4];
  long long carry, carry_n;
  chunk_offsets((ntracks[3] + TK_CHUNK - 1) / TK_CHUNK, chunk_cnt, chunk_off, s_w, &carry, &carry_n);
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
  if (int rc = tk_check_append(B, n_valid, cap, event_cap)) return rc;
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
