// Tile primitives shared by the hand-scheduled MFMA kernels (igemm192 / 224 / 256 / 256p / 384, wgrad384) and the LDS-DMA kernels around them.
#pragma once
#include <type_traits>

#include "common.h"

namespace dc {

// operands of __builtin_amdgcn_global_load_lds / raw_ptr_buffer_load_lds (the gfx950 LDS-DMA)
typedef __attribute__((address_space(1))) const void* gas_ptr;
typedef __attribute__((address_space(3))) void* lds_ptr;

// byte offset of 16-byte slot `slot` of a 64-byte K row (32 bf16): XOR swizzle, 4 slots per row
__device__ inline int swz64(int row, int slot) { return row * 64 + ((slot ^ ((row >> 1) & 3)) << 4); }

// lane ^ 16 exchange (the two 16-lane rows of a 32-lane half swap): ds_swizzle in bit-mask mode, no LDS memory involved
__device__ inline uint32_t swap_rows16(uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F); }
// sum over the 16 lanes of a DPP row (xor 1, xor 2, half mirror, mirror): every lane ends with the same bits
__device__ inline float row_sum16(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));   // row_mirror
  return v;
}

// MFMA as a (volatile) statement: keeps its place between the hand-placed LDS reads and waits below.
__device__ inline void mfma_v(f32x4& c, const bf16x8& av, const bf16x8& bv) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(av), "v"(bv));
}

// LDS fragment reads and their waits are written out: the compiler's own s_waitcnt placement waits lgkmcnt(0) in front of every
// block of MFMAs, i.e. also for the fragment it has just requested for the NEXT block (one exposed LDS latency per block on a
// SIMD that has no second wave to hide it).  Reads issued here are invisible to that pass; every consumer is one of the (volatile)
// MFMA statements above, placed behind a counted wait.
template <int OFF>
__device__ inline void lds_read16(bf16x8& dst, uint32_t addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int N>
__device__ inline void lgkm_wait() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// f(integral_constant<int, I>) for I = I .. N-1, unrolled at compile time: block indices reach the waits and offsets above as constants
template <int I, int N, typename F>
__device__ inline void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

}  // namespace dc
