// Mask morphology: dilation, erosion, hole filling and reconstruction of class planes (dc_mask_morph; nn.MaskMorphology).
// include/deepcam_hip.h has the operators word for word; this file has the decomposition.  skeleton_bits.h has the bit plane it shares
// with th_thin_kernel and sp_prune_kernel.
//
//   morph_planes   ONE workgroup of 1024 threads per (class, valid sample) keeps the class plane as a bit plane in LDS (th_thin_kernel's
//                  layout; the bits from W on in a row's last word are zero and stay zero), runs the class's whole program there and
//                  stores the final plane as words.  At 768 x 1152 one plane fits the LDS and two do not.
//     pack         a wave's __ballot over 64 consecutive columns is one word.
//     DILATE       thread t owns the words t, t + 1024, ... (at most TH_WPT = 20).  An elementary step reads the ring of every owned
//                  word (th_ring: the funnel shifts handle the seam), keeps c | N4 or c | N8 in nw[], and writes it behind a barrier:
//                  every read of a step lies before the barrier, every write behind it, a word is written by its owner alone.
//     ERODE        with its foreground padding erosion is the dual of dilation with background padding, and the structuring elements
//                  are symmetric: the owner complements its words inside the frame, the r dilation steps run, the owner complements
//                  again.  Two owner-only passes instead of a second operator.
//     FILL         X u (C \ R) is the frame without R, so the step floods R and complements: mask m = ~X inside the frame, plane =
//                  m on the polar rows (and on the two edge columns without wrap), mo_propagate on the 4-neighbours, plane = ~plane inside the frame.
//     RECONSTRUCT  the seeds move to registers, the waves pack the original plane again from the input (nothing of it is kept across
//                  the program), m = that plane, plane = seeds & m, mo_propagate on the 8-neighbours.
//     propagate    monotone growth inside a fixed mask: the fixed point is unique and any order of updates reaches it, so the
//                  relaxation is in place and chaotic, ONE barrier a round (skeleton_course.hip makes the same argument for its
//                  distances).  A reader may see a neighbour's word as it was or as it will be; both lie below the fixed point.  For
//                  these steps a thread owns a RUN of consecutive rows of one word column (mo_run: thread t has column t % TW, so
//                  consecutive lanes read consecutive words) and keeps the run's mask words in registers, m[] (40 VGPRs).  In a round
//                  it sweeps the run down and then up: a word takes its neighbours' bits (4 or 8 planes) and fills whole runs of its
//                  mask at once by the carry of an addition (mo_flood), and the next row reads what the thread has just written.  A
//                  flood thus crosses a thread's rows in one round: the open background of 768 x 1152, 14 rows a thread, needs about
//                  H / 14 rounds from the poles and not H / 2.  A word whose mask is zero, or that is full, costs no neighbour read.
//                  A round that changed nothing ends the step; `rounds` counts it.  Four flags rotate: round q sets flag[q & 3] and
//                  clears flag[(q + 1) & 3], whose last readers passed the barrier before the last one.  The cap of H * W rounds
//                  cannot cut a real flood: every round but the last adds a pixel outside the marker.
//     store        the owner stores its words: uint64 [B][2][H][TW].  Thread 0 zeroes the four counters of its class and frame.
//   morph_compose  one streaming pass, 16 pixels a thread: a 16-byte load of the mask, one word of each plane (16 divides 64: the
//                  pixels share it), the composition rule, a 16-byte store.  The four counters of each class are popcounts of 16-bit
//                  lane masks, summed by wave shuffles and LDS; one 64-bit atomic per workgroup and non-zero counter.  Masks of wider
//                  elements, and widths that are no multiple of 16, take the same pass pixel by pixel.
// Integer arithmetic only; no workgroup waits for another.
#include <cstdio>
#include "skeleton_bits.h"

namespace dc {

static constexpr int MO_STEPS = 8;
static constexpr int MO_DILATE = 1, MO_ERODE = 2, MO_FILL = 3, MO_RECONSTRUCT = 4;
static constexpr int MO_COUNTS = 4;               // pixels_in, pixels_out, added, removed
static constexpr int MO_PX = 16;                  // pixels per thread of morph_compose

// the bits of a word of column cw that lie inside the frame
__device__ inline u64 mo_valid(int cw, int TW, int lastbit) { return cw == TW - 1 ? ~0ull >> (63 - lastbit) : ~0ull; }

// every run of m that holds a bit of s (a subset of m), from that bit towards bit 63: the carry of m + s runs to the run's end
__device__ inline u64 mo_up(u64 s, u64 m) { return (((m + s) ^ m) & m) | s; }
// ... and in both directions
__device__ inline u64 mo_flood(u64 s, u64 m) { return mo_up(s, m) | __brevll(mo_up(__brevll(s), __brevll(m))); }

// one elementary dilation of word i: the word and its four or eight neighbour planes
__device__ inline u64 mo_dilate_word(const u64* P, int i, int H, int TW, int lastbit, int wrap, bool eight) {
  const u64 c = P[i];
  u64 p[8];
  th_ring(P, i, c, H, TW, lastbit, wrap, p);
  u64 v = c | p[0] | p[2] | p[4] | p[6];
  if (eight) v |= p[1] | p[3] | p[5] | p[7];
  return v & mo_valid(i % TW, TW, lastbit);
}

// One relaxation of the word at (r, cw) inside its mask m: true when it grew.  The plane's word is a subset of m throughout.  Four reads
// give the planes of the 4-neighbours; `eight` (uniform) adds the four diagonal words and their planes, with th_ring's formulas.
__device__ __forceinline__ bool mo_grow(u64* P, int r, int cw, u64 m, bool eight, int H, int TW, int lastbit, int wrap) {
  if (m == 0) return false;
  const int i = r * TW + cw;
  const u64 x = P[i];
  if (x == m) return false;
  const bool first = cw == 0, last = cw == TW - 1;
  const int il = first ? i + TW - 1 : i - 1, ir = last ? i - cw : i + 1;
  const u64 ml = P[il], mr = P[ir];
  const u64 u = r > 0 ? P[i - TW] : 0ull, d = r < H - 1 ? P[i + TW] : 0ull;
  u64 s = x | u | d | th_west(x, ml, first, lastbit, wrap) | th_east(x, mr, last, lastbit, wrap);
  if (eight) {
    u64 ul = 0, ur = 0, dl = 0, dr = 0;
    if (r > 0) ul = P[il - TW], ur = P[ir - TW];
    if (r < H - 1) dl = P[il + TW], dr = P[ir + TW];
    s |= th_west(u, ul, first, lastbit, wrap) | th_east(u, ur, last, lastbit, wrap) | th_west(d, dl, first, lastbit, wrap) |
         th_east(d, dr, last, lastbit, wrap);
  }
  const u64 nw = mo_flood(s & m, m);
  if (nw == x) return false;
  P[i] = nw;
  return true;
}

// A thread's run for the propagation steps: `len` consecutive words of the column-major order, from row r0 of column cw0 on.  With
// segs > 0 (the usual case: TW * segs <= 1024) thread t has rows [seg * rps, ...) of column t % TW, seg = t / TW, and a run never leaves
// its column.  With segs == 0 (a plane of more than 1024 columns of words, or one a few words short of the LDS) the runs cut the
// column-major order into 1024 pieces of rps words, and a run may pass from the foot of a column to the head of the next.
struct MoRun {
  int cw0, r0, len;
};
__device__ inline MoRun mo_run(int t, int H, int TW, int n, int rps, int segs) {
  MoRun u;
  if (segs > 0) {
    const int seg = t / TW;
    u.cw0 = t - seg * TW, u.r0 = seg * rps;
    u.len = seg < segs ? min(rps, H - u.r0) : 0;
  } else {
    const int q0 = t * rps;
    u.len = max(0, min(rps, n - q0));
    u.cw0 = q0 / H, u.r0 = q0 - u.cw0 * H;
  }
  return u;
}

// the words of a run, in order: `body` sees k = 0 .. len - 1 and the word's row r and column cw
#define MO_RUN_DOWN(run, r, cw, body)              \
  {                                                \
    int r = (run).r0, cw = (run).cw0;              \
    _Pragma("unroll") for (int k = 0; k < TH_WPT; ++k) { \
      if (k < (run).len) {                         \
        body;                                      \
        if (++r == H) r = 0, ++cw;                 \
      }                                            \
    }                                              \
  }

// Grows the plane inside m[] to its fixed point; returns the rounds run (the final empty one counted) and *converged.  rr: the running
// round number of the workgroup, which picks the flags.  Every thread calls it; the plane stands when it returns.
__device__ __forceinline__ int mo_propagate(u64* P, volatile unsigned* flag, const MoRun& run, const u64* m, bool eight, int H, int TW, int lastbit, int wrap,
                                   int cap, unsigned* rr, int* converged) {
  int rounds = 0;
  *converged = 0;
  while (rounds < cap) {
    const unsigned f = *rr & 3u;
    if (threadIdx.x == 0) flag[(*rr + 1u) & 3u] = 0u;
    bool grew = false;
    int r = run.r0, cw = run.cw0;
    asm volatile("" : "+v"(r), "+v"(cw));         // opaque, as th_subpass's tid: twenty words' indices and seam tests are computed where
                                                  // they are used, not hoisted out of the rounds or kept from one sweep to the next
#pragma unroll
    for (int k = 0; k < TH_WPT; ++k)
      if (k < run.len) {
        grew |= mo_grow(P, r, cw, m[k], eight, H, TW, lastbit, wrap);
        if (++r == H) r = 0, ++cw;
        __builtin_amdgcn_sched_barrier(0);        // one word at a time: interleaving the unrolled bodies only costs registers
      }
    asm volatile("" : "+v"(r), "+v"(cw));
#pragma unroll
    for (int k = TH_WPT - 1; k >= 0; --k)
      if (k < run.len) {
        if (r == 0) r = H - 1, --cw;
        else --r;
        grew |= mo_grow(P, r, cw, m[k], eight, H, TW, lastbit, wrap);
        __builtin_amdgcn_sched_barrier(0);
      }
    if (__ballot(grew) && (threadIdx.x & 63) == 0) flag[f] = 1u;
    __syncthreads();
    ++rounds, ++*rr;
    if (flag[f] == 0u) {
      *converged = 1;
      break;
    }
  }
  return rounds;
}

// packs the plane `cls` of the frame at `base` into P; ends with a barrier
__device__ inline void mo_pack(u64* P, const void* __restrict__ mask, int mask_bytes, size_t base, unsigned cls, int n, int TW, int W) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int item0 = wave; item0 < n; item0 += TH_BATCH * TH_WAVES) {
    unsigned c[TH_BATCH];
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) c[q] = th_class(mask, mask_bytes, base, item0 + q * TH_WAVES, n, TW, W, lane);
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) {
      const int item = item0 + q * TH_WAVES;
      const u64 w = __ballot(c[q] == cls);
      if (item < n && lane == 0) P[item] = w;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(TH_THREADS) void morph_planes_kernel(int H, int W, const void* __restrict__ mask, int mask_bytes, int wrap,
                                                                  u64 program_1, u64 program_2, int rps, int segs, u64* __restrict__ planes,
                                                                  u64* __restrict__ counts, int* __restrict__ rounds_out,
                                                                  int* __restrict__ converged_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int TW = (W + 63) / 64, n = H * TW, lastbit = (W - 1) & 63;
  u64* P = (u64*)smem;
  volatile unsigned* flag = (volatile unsigned*)(smem + (size_t)n * 8);
  const unsigned cls = blockIdx.x + 1;
  const int b = blockIdx.y, slot = b * 2 + (int)cls - 1;
  const size_t base = (size_t)b * H * W;
  const u64 program = cls == 1 ? program_1 : program_2;
  const int cap = H * W;
  int tid = threadIdx.x;
#define MO_OPAQUE_TID() asm volatile("" : "+v"(tid))   // as in th_subpass: a word's indices are computed where they are used
  if (threadIdx.x < 4) flag[threadIdx.x] = 0u;
  if (threadIdx.x < MO_COUNTS) counts[(size_t)slot * MO_COUNTS + threadIdx.x] = 0ull;
  mo_pack(P, mask, mask_bytes, base, cls, n, TW, W);
  const MoRun run = mo_run(threadIdx.x, H, TW, n, rps, segs);
  unsigned rr = 0;
  int all_converged = 1;
  for (int step = 0; step < MO_STEPS; ++step) {
    const int code = (int)((program >> (8 * step)) & 0xFFull), op = code >> 5, radius = code & 31;
    int step_rounds = 0;
    if (op == MO_DILATE || op == MO_ERODE) {
      if (op == MO_ERODE) {                       // the dual: complement inside the frame, dilate, complement
        MO_OPAQUE_TID();
#pragma unroll
        for (int k = 0; k < TH_WPT; ++k) {
          const int i = tid + k * TH_THREADS;
          if (i < n) P[i] = ~P[i] & mo_valid(i % TW, TW, lastbit);
        }
        __syncthreads();
      }
      for (int j = 1; j <= radius; ++j) {
        u64 nw[TH_WPT];
        MO_OPAQUE_TID();
#pragma unroll
        for (int k = 0; k < TH_WPT; ++k) {
          const int i = tid + k * TH_THREADS;
          nw[k] = 0;
          if (i < n) nw[k] = mo_dilate_word(P, i, H, TW, lastbit, wrap, (j & 1) == 0);
          __builtin_amdgcn_sched_barrier(0);      // one word at a time: interleaving the unrolled bodies only costs registers
        }
        __syncthreads();                          // the plane has been read
#pragma unroll
        for (int k = 0; k < TH_WPT; ++k)
          if (nw[k]) P[tid + k * TH_THREADS] = nw[k];      // (a zero result: the word was zero and stays)
        __syncthreads();
      }
      if (op == MO_ERODE) {
        MO_OPAQUE_TID();
#pragma unroll
        for (int k = 0; k < TH_WPT; ++k) {
          const int i = tid + k * TH_THREADS;
          if (i < n) P[i] = ~P[i] & mo_valid(i % TW, TW, lastbit);
        }
        __syncthreads();
      }
    } else if (op == MO_FILL || op == MO_RECONSTRUCT) {
      const bool fill = op == MO_FILL;
      u64 m[TH_WPT];
#pragma unroll
      for (int k = 0; k < TH_WPT; ++k) m[k] = 0;
      if (fill) {                                 // the frame without the flood: m = ~X, the plane takes the marker
        MO_RUN_DOWN(run, r, cw, {
          const int i = r * TW + cw;
          const u64 valid = mo_valid(cw, TW, lastbit);
          m[k] = ~P[i] & valid;
          u64 marker = (r == 0 || r == H - 1) ? valid : 0ull;
          if (!wrap) marker |= (cw == 0 ? 1ull : 0ull) | (cw == TW - 1 ? 1ull << lastbit : 0ull);
          P[i] = m[k] & marker;                   // the run's own word: nobody else reads it before the barrier
        });
      } else {                                    // the seeds move to m[], the original plane is packed again, m[] becomes that plane
        MO_RUN_DOWN(run, r, cw, { m[k] = P[r * TW + cw]; });
        __syncthreads();
        mo_pack(P, mask, mask_bytes, base, cls, n, TW, W);
        MO_RUN_DOWN(run, r, cw, {
          const int i = r * TW + cw;
          const u64 seeds = m[k];
          m[k] = P[i];
          P[i] = seeds & m[k];
        });
      }
      __syncthreads();
      int conv;
      step_rounds = mo_propagate(P, flag, run, m, !fill, H, TW, lastbit, wrap, cap, &rr, &conv);
      all_converged &= conv;
      if (fill) {
        MO_RUN_DOWN(run, r, cw, {
          const int i = r * TW + cw;
          P[i] = ~P[i] & mo_valid(cw, TW, lastbit);
        });
        __syncthreads();
      }
    }
    if (threadIdx.x == 0) rounds_out[slot * MO_STEPS + step] = step_rounds;
  }
  u64* out = planes + (size_t)slot * n;
  for (int i = threadIdx.x; i < n; i += TH_THREADS) out[i] = P[i];
  if (threadIdx.x == 0) converged_out[slot] = all_converged;
#undef MO_OPAQUE_TID
}

// the output byte of a pixel whose input is c (full width) and whose planes hold x1 and x2
__device__ inline unsigned mo_pixel(long long c, bool x1, bool x2) {
  if (c >= 3 && c <= 255) return (unsigned)c;
  if (c == 1 && x1) return 1u;
  if (c == 2 && x2) return 2u;
  return x1 ? 1u : (x2 ? 2u : 0u);
}

__global__ __launch_bounds__(256) void morph_compose_kernel(int H, int W, int vec, const void* __restrict__ mask, int mask_bytes,
                                                            const u64* __restrict__ planes, uint8_t* __restrict__ out_mask, u64* counts) {
  __shared__ unsigned s_n[2 * MO_COUNTS];
  const int TW = (W + 63) / 64, n = H * TW, b = blockIdx.y;
  const long HW = (long)H * W;
  const size_t base = (size_t)b * HW;
  const u64* X1 = planes + (size_t)(b * 2) * n;
  const u64* X2 = X1 + n;
  if (threadIdx.x < 2 * MO_COUNTS) s_n[threadIdx.x] = 0u;
  __syncthreads();
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * MO_PX;
  unsigned in1 = 0, in2 = 0, o1 = 0, o2 = 0;      // one bit per pixel of this thread
  if (vec && p0 < HW) {                           // W is a multiple of 16: the 16 pixels lie in one row and in one word
    const int r = (int)(p0 / W), c0 = (int)(p0 - (long)r * W);
    const int sh = c0 & 63;
    const unsigned x1 = (unsigned)(X1[r * TW + (c0 >> 6)] >> sh) & 0xFFFFu, x2 = (unsigned)(X2[r * TW + (c0 >> 6)] >> sh) & 0xFFFFu;
    const uint4 v = *(const uint4*)((const uint8_t*)mask + base + p0);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o[q] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int px = q * 4 + j;
        const unsigned c = (w[q] >> (8 * j)) & 0xFFu;
        const unsigned y = mo_pixel(c, (x1 >> px) & 1u, (x2 >> px) & 1u);
        o[q] |= y << (8 * j);
        in1 |= (c == 1u ? 1u : 0u) << px, in2 |= (c == 2u ? 1u : 0u) << px;
        o1 |= (y == 1u ? 1u : 0u) << px, o2 |= (y == 2u ? 1u : 0u) << px;
      }
    }
    *(uint4*)(out_mask + base + p0) = make_uint4(o[0], o[1], o[2], o[3]);
  } else if (!vec) {
    for (int px = 0; px < MO_PX; ++px) {
      const long p = p0 + px;
      if (p < HW) {
        const int r = (int)(p / W), col = (int)(p - (long)r * W);
        const int i = r * TW + (col >> 6);
        const long long c = mask_value(mask, base + p, mask_bytes);
        const unsigned y = mo_pixel(c, (X1[i] >> (col & 63)) & 1ull, (X2[i] >> (col & 63)) & 1ull);
        out_mask[base + p] = (uint8_t)y;
        in1 |= (c == 1 ? 1u : 0u) << px, in2 |= (c == 2 ? 1u : 0u) << px;
        o1 |= (y == 1u ? 1u : 0u) << px, o2 |= (y == 2u ? 1u : 0u) << px;
      }
    }
  }
  unsigned v[2 * MO_COUNTS] = {(unsigned)__popc(in1), (unsigned)__popc(o1), (unsigned)__popc(o1 & ~in1), (unsigned)__popc(in1 & ~o1),
                               (unsigned)__popc(in2), (unsigned)__popc(o2), (unsigned)__popc(o2 & ~in2), (unsigned)__popc(in2 & ~o2)};
#pragma unroll
  for (int i = 0; i < 2 * MO_COUNTS; ++i) {
    unsigned x = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(&s_n[i], x);
  }
  __syncthreads();
  if (threadIdx.x < 2 * MO_COUNTS && s_n[threadIdx.x])
    atomicAdd(counts + (size_t)b * 2 * MO_COUNTS + threadIdx.x, (u64)s_n[threadIdx.x]);
}

// 0 where the program word is well formed, else the message in msg (the wording nn.morph_program uses too)
static int mo_check_program(unsigned long long program, char* msg, size_t cap) {
  bool ended = false;
  for (int i = 0; i < MO_STEPS; ++i) {
    const int code = (int)((program >> (8 * i)) & 0xFFull), op = code >> 5, r = code & 31;
    if (ended) {
      if (code != 0) return snprintf(msg, cap, "morph program: step %d: a byte after the end byte is not zero", i), 1;
      continue;
    }
    if (op == 0) {
      if (r != 0) return snprintf(msg, cap, "morph program: step %d: an end byte must be zero", i), 1;
      ended = true;
    } else if (op > MO_RECONSTRUCT) {
      return snprintf(msg, cap, "morph program: step %d: op %d is not defined (1 DILATE, 2 ERODE, 3 FILL, 4 RECONSTRUCT)", i, op), 1;
    } else if (op == MO_DILATE || op == MO_ERODE) {
      if (r < 1) return snprintf(msg, cap, "morph program: step %d: a radius must lie in [1, 31], got %d", i, r), 1;
    } else if (r != 0) {
      return snprintf(msg, cap, "morph program: step %d: FILL and RECONSTRUCT take r = 0, got %d", i, r), 1;
    }
  }
  return 0;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_mask_morph(int B, int n_valid, int H, int W, const void* mask, int mask_bytes, int wrap, unsigned long long program_1,
                             unsigned long long program_2, uint8_t* out_mask, int64_t* counts, int32_t* rounds, int32_t* converged,
                             void* planes, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(mask_bytes == 1 || mask_bytes == 4 || mask_bytes == 8, "dc_mask_morph: mask_bytes must be 1, 4 or 8");
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_mask_morph: wrap must be 0 or 1");
  char msg[160];
  if (mo_check_program(program_1, msg, sizeof(msg)) || mo_check_program(program_2, msg, sizeof(msg))) return dc_fail(msg, __FILE__, __LINE__);
  DC_REQUIRE(mask && out_mask && counts && rounds && converged && planes, "dc_mask_morph: null pointer");
  DC_REQUIRE(((uintptr_t)mask & (mask_bytes - 1)) == 0, "dc_mask_morph: the mask is not aligned to its element size");
  DC_REQUIRE(((uintptr_t)planes & 7) == 0 && ((uintptr_t)counts & 7) == 0, "dc_mask_morph: the planes or the counts are not 8-byte aligned");
  const size_t lds = th_lds_bytes(H, W);
  DC_REQUIRE(lds != 0, "dc_mask_morph: the bit plane of H x W does not fit the LDS of one CU (H * ceil(W / 64) * 8 + 64 bytes of 160 KiB)");
  const size_t px = (size_t)B * H * W;
  DC_REQUIRE((uintptr_t)out_mask + px <= (uintptr_t)mask || (uintptr_t)mask + px * mask_bytes <= (uintptr_t)out_mask,
             "dc_mask_morph: out_mask may not alias mask");
  const int TW = (W + 63) / 64, n = H * TW;
  int rps = 0, segs = 0;                          // the propagation's runs (mo_run): whole columns cut into segs pieces where that fits
  for (int r = 1; r <= TH_WPT && !rps; ++r)
    if ((long)TW * ((H + r - 1) / r) <= TH_THREADS) rps = r, segs = (H + r - 1) / r;
  if (!rps) rps = (n + TH_THREADS - 1) / TH_THREADS;
  hipStream_t st = (hipStream_t)stream;
  DC_ONCE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&morph_planes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TH_LDS_MAX));
  hipLaunchKernelGGL(morph_planes_kernel, dim3(2, n_valid), dim3(TH_THREADS), lds, st, H, W, mask, mask_bytes, wrap, (u64)program_1,
                     (u64)program_2, rps, segs, (u64*)planes, (u64*)counts, rounds, converged);
  DC_LAUNCHED("morph_planes");
  const long HW = (long)H * W;
  const int vec = mask_bytes == 1 && W % MO_PX == 0 && ((uintptr_t)mask & 15) == 0 && ((uintptr_t)out_mask & 15) == 0;
  const long blocks = (HW + 256 * MO_PX - 1) / (256 * MO_PX);
  hipLaunchKernelGGL(morph_compose_kernel, dim3((unsigned)blocks, n_valid), dim3(256), 0, st, H, W, vec, mask, mask_bytes,
                     (const u64*)planes, out_mask, (u64*)counts);
  DC_LAUNCHED("morph_compose");
  return 0;
}
