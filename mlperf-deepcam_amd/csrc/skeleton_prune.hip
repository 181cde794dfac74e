// Spur pruning of skeletons and the axis criterion of the event filter (dc_skeleton_prune, dc_event_select_axis; nn.EventAxis(prune=),
// nn.EventFilter(min_axis_km=)).  include/deepcam_hip.h has the rule word for word -- endpoints, backward and forward neighbours, the
// shrink rounds, the regrowth; this file has the decomposition.  skeleton_bits.h has what it shares with th_thin_kernel.
//
//   sp_prune   ONE workgroup of 1024 threads per (class, valid sample), the class plane as a bit plane in LDS (th_thin_kernel's layout:
//              thread t owns the words t, t + 1024, ...; at most TH_WPT = 20).  At 768 x 1152 ONE plane fits the LDS and two do not, so
//              whatever a phase needs beside the plane lives in the registers of the word's owner or is packed again from the byte map:
//              pack     a wave's __ballot over 64 consecutive bytes of `skeleton` is one word.
//              shrink   a round is two sub-steps.  Sub-step 1 reads the ring of every owned word that is not zero, counts it bit-sliced
//                       (sp_ends) and keeps the word's A and Bc bits in a[] and bc[]; behind the barrier the owner writes S' = S & ~a.
//                       Sub-step 2 re-reads the ring, now of S', for the words whose bc is not zero -- endpoints without a backward
//                       neighbour, a few per frame -- keeps B = bc & (any neighbour) in bc[], and behind the barrier writes S'' = S' & ~B.
//                       A wave that deleted sets flag[round & 1] before the round's last barrier; everybody reads it behind it.  The
//                       other flag is cleared between the round's first two barriers: its last readers read it before they reached the
//                       first, its next writers come behind the next round's third.  Four barriers a round; every LDS read of a sub-step
//                       lies before a barrier and every write behind one; a word is written by its owner alone.
//              seeds    with X1 in the plane, the owner forms g[] = E(X1) | isolated(X1) of its words (ring reads; barrier).
//              expand   a wave per word again: lane b reads the input byte, stores X1's bit to `pruned` and the ballot packs
//                       D = input & ~X1, which the wave writes over the word it has just read -- the plane now holds D (barrier).  Both
//                       workgroups of a frame write one byte plane: class 2's owns the bytes whose input was 2, class 1's all others.
//              regrow   the owner moves its D words to d[] and writes g[] in their place: the plane holds G (barrier).  A round reads the
//                       ring of G for the owned words whose d is not zero, keeps add = dilate8(G) & d & ~G in a[], and ORs it in behind
//                       the barrier; flags as above, two barriers a round.  G never leaves X1 | D, so G & d is what regrew.
//              store    the owner leaves G & d in the plane (barrier), the wave-per-word loop stores the class on those bytes: the lane
//                       that wrote a byte in `expand` is the one that writes it now.  removed = popcount(d & ~G), summed by wave
//                       shuffles and sixteen partial sums in LDS: one store per (class, frame), no atomics, no memset.
//   Registers: two arrays of 20 words at a time (a[] and bc[]; g[] alone; d[] and a[]), 80 VGPRs, beside a word's ring and adders.  The
//   resource report of the build is in DESIGN 7w (no scratch).
//   sp_select  one thread per event row: keep -> 0 and one event from kept to dropped where the axis falls short.  Integer compares and
//              integer atomics only.
#include "skeleton_bits.h"

namespace dc {

static constexpr int SP_MAX_SPUR = 1024;
static constexpr int AXIS_FIELDS = 7, AXIS_LENGTH = 6;   // a row of dc_skeleton_stats and its length_m
static constexpr int SEL_COUNTS = 8;                      // dc_event_select's counts per sample: per class events kept, dropped, pixels kept, dropped

// of word c (not zero) and its ring p: the endpoints E, the isolated pixels, and the pixels with a backward neighbour (P8, P9, P2, P3).
// The ring is counted bit-sliced: three adders give the ones (s) and four carries of weight two; "exactly two, consecutive" is "two" and
// one of the eight Pi & Pi+1.
__device__ inline void sp_ends(u64 c, const u64* p, u64* ends, u64* alone, u64* back) {
  const u64 x1 = p[0] ^ p[1], s1 = x1 ^ p[2], c1 = (p[0] & p[1]) | (p[2] & x1);
  const u64 x2 = p[3] ^ p[4], s2 = x2 ^ p[5], c2 = (p[3] & p[4]) | (p[5] & x2);
  const u64 s3 = p[6] ^ p[7], c3 = p[6] & p[7];
  const u64 x4 = s1 ^ s2, s = x4 ^ s3, c4 = (s1 & s2) | (s3 & x4);  // count = s + 2 (c1 + c2 + c3 + c4)
  const u64 anyc = c1 | c2 | c3 | c4;
  const u64 onec = (c1 ^ c2 ^ c3 ^ c4) & ~((c1 & c2) | (c3 & c4));  // exactly one carry: odd parity and no pair
  const u64 pair = (p[0] & p[1]) | (p[1] & p[2]) | (p[2] & p[3]) | (p[3] & p[4]) | (p[4] & p[5]) | (p[5] & p[6]) | (p[6] & p[7]) | (p[7] & p[0]);
  *ends = c & ((s & ~anyc) | (~s & onec & pair));
  *alone = c & ~(s | anyc);
  *back = p[6] | p[7] | p[0] | p[1];
}

// the class of the lane's input byte for word `item`, as th_class gives it
__device__ inline unsigned sp_class(const uint8_t* __restrict__ skeleton, size_t base, int item, int n, int TW, int W, int lane) {
  return th_class(skeleton, 1, base, item, n, TW, W, lane);
}

__global__ __launch_bounds__(TH_THREADS) void sp_prune_kernel(int H, int W, const uint8_t* __restrict__ skeleton, int wrap, int spur,
                                                              uint8_t* __restrict__ pruned, int* __restrict__ removed) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int TW = (W + 63) / 64, n = H * TW, lastbit = (W - 1) & 63;
  u64* P = (u64*)smem;
  volatile unsigned* flag = (volatile unsigned*)(smem + (size_t)n * 8);
  const unsigned cls = blockIdx.x + 1;
  const int b = blockIdx.y;
  const size_t base = (size_t)b * H * W;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int tid = threadIdx.x;
#define SP_OPAQUE_TID() asm volatile("" : "+v"(tid))   // as in th_subpass: a word's row, column and neighbour indices are computed where
                                                       // they are used, not hoisted out of the rounds, where twenty words' worth of them
                                                       // would crowd out the word arrays
  if (threadIdx.x < 2) flag[threadIdx.x] = 0u;
  // pack
  for (int item0 = wave; item0 < n; item0 += TH_BATCH * TH_WAVES) {
    unsigned c[TH_BATCH];
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) c[q] = sp_class(skeleton, base, item0 + q * TH_WAVES, n, TW, W, lane);
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) {
      const int item = item0 + q * TH_WAVES;
      const u64 w = __ballot(c[q] == cls);
      if (item < n && lane == 0) P[item] = w;
    }
  }
  __syncthreads();
  u64 a[TH_WPT];
  {  // ---- shrink
    u64 bc[TH_WPT];
    for (int round = 0; round < spur; ++round) {
      const int f = round & 1;
      SP_OPAQUE_TID();
#pragma unroll
      for (int k = 0; k < TH_WPT; ++k) {
        const int i = tid + k * TH_THREADS;
        a[k] = 0, bc[k] = 0;
        if (i < n) {
          const u64 c = P[i];
          if (c) {
            u64 p[8], ends, alone, back;
            th_ring(P, i, c, H, TW, lastbit, wrap, p);
            sp_ends(c, p, &ends, &alone, &back);
            a[k] = ends & back, bc[k] = ends & ~back;
          }
        }
        __builtin_amdgcn_sched_barrier(0);        // one word at a time: interleaving the unrolled bodies only costs registers
      }
      __syncthreads();                            // S has been read
      u64 any = 0;
#pragma unroll
      for (int k = 0; k < TH_WPT; ++k)
        if (a[k]) {
          P[tid + k * TH_THREADS] &= ~a[k];
          any |= a[k];
        }
      if (threadIdx.x == 0) flag[f ^ 1] = 0u;
      __syncthreads();                            // S' stands
      SP_OPAQUE_TID();
#pragma unroll
      for (int k = 0; k < TH_WPT; ++k) {
        if (bc[k]) {                              // rare: an endpoint without a backward neighbour
          const int i = tid + k * TH_THREADS;
          u64 p[8];
          th_ring(P, i, P[i], H, TW, lastbit, wrap, p);
          bc[k] &= p[0] | p[1] | p[2] | p[3] | p[4] | p[5] | p[6] | p[7];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();                            // S' has been read
#pragma unroll
      for (int k = 0; k < TH_WPT; ++k)
        if (bc[k]) {
          P[tid + k * TH_THREADS] &= ~bc[k];
          any |= bc[k];
        }
      if (__ballot(any != 0) && lane == 0) flag[f] = 1u;
      __syncthreads();                            // S'' stands
      if (flag[f] == 0u) break;
    }
  }
  // ---- seeds: E(X1) and the isolated pixels of X1, of the owned words (a[] is g[] from here to the regrowth)
  SP_OPAQUE_TID();
#pragma unroll
  for (int k = 0; k < TH_WPT; ++k) {
    const int i = tid + k * TH_THREADS;
    a[k] = 0;
    if (i < n) {
      const u64 c = P[i];
      if (c) {
        u64 p[8], ends, alone, back;
        th_ring(P, i, c, H, TW, lastbit, wrap, p);
        sp_ends(c, p, &ends, &alone, &back);
        a[k] = ends | alone;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();                                // X1's rings have been read
  // ---- expand X1 into `pruned`; the word becomes D = input & ~X1.  A word is read and written by one wave, in this order.
  for (int item0 = wave; item0 < n; item0 += TH_BATCH * TH_WAVES) {
    unsigned c[TH_BATCH];
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) c[q] = sp_class(skeleton, base, item0 + q * TH_WAVES, n, TW, W, lane);
#pragma unroll
    for (int q = 0; q < TH_BATCH; ++q) {
      const int item = item0 + q * TH_WAVES;
      const bool kept = item < n && ((P[item] >> lane) & 1ull) != 0;
      if (c[q] != TH_NONE && (c[q] == 2u) == (cls == 2u)) {
        const int r = item / TW;
        pruned[base + (size_t)r * W + (item - r * TW) * 64 + lane] = kept ? (uint8_t)cls : (uint8_t)0;
      }
      const u64 w = __ballot(c[q] == cls && !kept);
      if (item < n && lane == 0) P[item] = w;
    }
  }
  __syncthreads();                                // the plane holds D
  u64 d[TH_WPT];
  u64 some = 0;
#pragma unroll
  for (int k = 0; k < TH_WPT; ++k) {
    const int i = tid + k * TH_THREADS;
    d[k] = 0;
    if (i < n) {
      d[k] = P[i];
      P[i] = a[k];                                // the owner's own word: no other thread reads it in this step
      some |= d[k];
    }
  }
  if (__ballot(some != 0) && lane == 0) flag[spur & 1] = 1u;          // (clear: by the shrink's last round, or never set)
  __syncthreads();                                // the plane holds G0
  // ---- regrow: G <- G | (dilate8(G) & D), spur rounds at most, none where nothing was removed
  if (flag[spur & 1] != 0u) {
    __syncthreads();                              // everybody has read the flag
    if (threadIdx.x < 2) flag[threadIdx.x] = 0u;
    for (int round = 0; round < spur; ++round) {
      const int f = round & 1;
      SP_OPAQUE_TID();
#pragma unroll
      for (int k = 0; k < TH_WPT; ++k) {
        a[k] = 0;
        if (d[k]) {
          const int i = tid + k * TH_THREADS;
          const u64 g = P[i];
          u64 p[8];
          th_ring(P, i, g, H, TW, lastbit, wrap, p);
          a[k] = (p[0] | p[1] | p[2] | p[3] | p[4] | p[5] | p[6] | p[7]) & d[k] & ~g;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();                            // G has been read (and the flags' clearing above, in round 0, lies before it)
      u64 any = 0;
#pragma unroll
      for (int k = 0; k < TH_WPT; ++k)
        if (a[k]) {
          P[tid + k * TH_THREADS] |= a[k];
          any |= a[k];
        }
      if (threadIdx.x == 0 && round > 0) flag[f ^ 1] = 0u;   // read behind the previous round's last barrier, before this round's first
      if (__ballot(any != 0) && lane == 0) flag[f] = 1u;
      __syncthreads();
      if (flag[f] == 0u) break;
    }
  }
  // ---- store what regrew, count what stayed away
  int gone = 0;
#pragma unroll
  for (int k = 0; k < TH_WPT; ++k) {
    const int i = tid + k * TH_THREADS;
    if (i < n) {
      const u64 g = P[i];
      gone += __popcll(d[k] & ~g);
      P[i] = g & d[k];
    }
  }
  __syncthreads();                                // the plane holds the regrown pixels
  for (int item = wave; item < n; item += TH_WAVES) {
    const u64 w = P[item];
    if ((w >> lane) & 1ull) {
      const int r = item / TW;
      pruned[base + (size_t)r * W + (item - r * TW) * 64 + lane] = (uint8_t)cls;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) gone += __shfl_down(gone, o, 64);
  __syncthreads();                                // the plane has been read: its first 64 bytes take the waves' sums
  int* part = (int*)smem;
  if (lane == 0) part[wave] = gone;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < TH_WAVES; ++w) total += part[w];
    removed[b * 2 + (int)cls - 1] = total;
  }
#undef SP_OPAQUE_TID
}

__global__ __launch_bounds__(256) void sp_select_kernel(int cap, const long long* __restrict__ table, const int* __restrict__ ncomp,
                                                        const long long* __restrict__ axis_rows, long long min1, long long min2,
                                                        uint8_t* __restrict__ keep, unsigned long long* counts) {
  __shared__ unsigned s_n[2];                     // events that this workgroup drops, per class
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < 2) s_n[threadIdx.x] = 0u;
  __syncthreads();
  if (k < event_rows(ncomp, b, cap)) {
    const size_t e = (size_t)b * cap + k;
    const long long cls = table[e * CC_FIELDS + 1];
    if ((cls == 1 || cls == 2) && keep[e] != 0) {
      const long long need = cls == 1 ? min1 : min2;
      if (need > 0 && axis_rows[e * AXIS_FIELDS + AXIS_LENGTH] < need) {
        keep[e] = 0;
        atomicAdd(&s_n[cls - 1], 1u);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_n[threadIdx.x]) {
    unsigned long long* c = counts + (size_t)b * SEL_COUNTS + threadIdx.x * 4;
    atomicAdd(c, 0ull - (unsigned long long)s_n[threadIdx.x]);       // kept
    atomicAdd(c + 1, (unsigned long long)s_n[threadIdx.x]);          // dropped
  }
}

}  // namespace dc

using namespace dc;

extern "C" int dc_skeleton_prune(int B, int n_valid, int H, int W, const uint8_t* skeleton, int wrap, int spur, uint8_t* pruned,
                                 int32_t* removed, void* stream) {
  if (int rc = cc_check(B, n_valid, H, W)) return rc;
  DC_REQUIRE(wrap == 0 || wrap == 1, "dc_skeleton_prune: wrap must be 0 or 1");
  DC_REQUIRE(spur >= 1 && spur <= SP_MAX_SPUR, "dc_skeleton_prune: spur must lie in [1, 1024]");
  DC_REQUIRE(skeleton && pruned && removed, "dc_skeleton_prune: null pointer");
  const size_t lds = th_lds_bytes(H, W);
  DC_REQUIRE(lds != 0, "dc_skeleton_prune: the bit plane of H x W does not fit the LDS of one CU (H * ceil(W / 64) * 8 + 64 bytes of 160 KiB)");
  const size_t px = (size_t)B * H * W;
  DC_REQUIRE((uintptr_t)pruned + px <= (uintptr_t)skeleton || (uintptr_t)skeleton + px <= (uintptr_t)pruned,
             "dc_skeleton_prune: pruned may not alias skeleton");
  DC_ONCE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sp_prune_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TH_LDS_MAX));
  hipLaunchKernelGGL(sp_prune_kernel, dim3(2, n_valid), dim3(TH_THREADS), lds, (hipStream_t)stream, H, W, skeleton, wrap, spur, pruned,
                     removed);
  DC_LAUNCHED("skel_prune");
  return 0;
}

extern "C" int dc_event_select_axis(int B, int n_valid, int cap, const int64_t* table, const int32_t* ncomp, const int64_t* axis_rows,
                                    long long min_axis_m_1, long long min_axis_m_2, uint8_t* keep, int64_t* counts, void* stream) {
  if (int rc = cc_check_batch(B, n_valid)) return rc;
  DC_REQUIRE(cap >= 1, "dc_event_select_axis: cap must be at least 1");
  DC_REQUIRE(min_axis_m_1 >= 0 && min_axis_m_2 >= 0, "dc_event_select_axis: a threshold must be at least 0");
  DC_REQUIRE(table && ncomp && axis_rows && keep && counts, "dc_event_select_axis: null pointer");
  hipLaunchKernelGGL(sp_select_kernel, dim3((cap + 255) / 256, n_valid), dim3(256), 0, (hipStream_t)stream, cap, (const long long*)table, ncomp,
                     (const long long*)axis_rows, min_axis_m_1, min_axis_m_2, keep, (unsigned long long*)counts);
  DC_LAUNCHED("skel_prune");
  return 0;
}
