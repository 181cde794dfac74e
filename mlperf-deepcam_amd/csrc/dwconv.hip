// Depthwise 3x3 convolution of SeparableConv2d_same (fixed_padding + groups=C conv), NHWC, HBM-bound.
// One lane owns one 16-byte channel group (8 bf16 / 4 f32 channels) so every global access is a full vector and
// a wave covers up to 1 KiB of contiguous channels; each thread walks PX output pixels along W with the nine
// per-channel weights held in registers.  Forward / data-gradient read the weights repacked as [9][C] fp32.
#include <stdio.h>

#include <initializer_list>

#include "common.h"
#include "dwtile.h"
#include "bn_fin.h"
#include "dwtile_common.h"

namespace dc {

constexpr int DW_PX = 4;  // output pixels per thread (along W)

// weights arrive packed as [9][C] fp32 (dc_dwconv_pack_weights): one thread's 8 (4) channels of a tap are 1-2 vector loads
template <typename T>
__device__ inline void load_w9(const float* __restrict__ wp, int c0, int C, float (&wr)[9][Elem<T>::kPerVec]) {
  constexpr int KPV = Elem<T>::kPerVec;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const float4* src = reinterpret_cast<const float4*>(wp + (size_t)t * C + c0);
#pragma unroll
    for (int q = 0; q < KPV / 4; ++q) {
      const float4 v = src[q];
      wr[t][4 * q] = v.x; wr[t][4 * q + 1] = v.y; wr[t][4 * q + 2] = v.z; wr[t][4 * q + 3] = v.w;
    }
  }
}

// Fused producer: when pscale != nullptr the depthwise input is the RAW (pre-BatchNorm) conv output and the kernel applies
// v = x*scale[c] + shift[c] (and ReLU) to every in-bounds element as it is loaded; the zero padding stays zero.  The
// normalised activation is then never materialised in HBM.
template <int KPV>
__device__ inline void dw_prologue(float (&f)[KPV], const float* __restrict__ pscale, const float* __restrict__ pshift, int prelu, int c0) {
#pragma unroll
  for (int e = 0; e < KPV; ++e) {
    float v = fmaf(f[e], pscale[c0 + e], pshift[c0 + e]);
    f[e] = prelu ? fmaxf(v, 0.f) : v;
  }
}

__global__ void dw_pack_kernel(const float* __restrict__ master, float* __restrict__ packed, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * C) return;
  const int c = i / 9, t = i % 9;
  packed[(size_t)t * C + c] = master[i];
}

// mode 0: forward   out[n,oy,ox] = sum_t in[n, oy*s - d + ky*d, ox*s - d + kx*d] * w[t]
// mode 1: dgrad     out[n,iy,ix] = sum_t in[n, (iy + d - ky*d)/s, (ix + d - kx*d)/s] * w[t]   (when divisible) [+ addend]
template <typename T, int MODE>
__global__ __launch_bounds__(256) void dw_kernel(const T* __restrict__ in, int ldin, const float* __restrict__ w,
                                                 const T* __restrict__ addend, int ldadd, T* __restrict__ out,
                                                 int ldout, int N, int Hin, int Win, int Hout, int Wout, int C,
                                                 int stride, int dil, const float* __restrict__ pscale,
                                                 const float* __restrict__ pshift, int prelu) {
  constexpr int KPV = Elem<T>::kPerVec;
  const int ngroups = C / KPV;
  const int wq = (Wout + DW_PX - 1) / DW_PX;
  const long total = (long)N * Hout * wq * ngroups;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(idx % ngroups);
    long r = idx / ngroups;
    const int xq = (int)(r % wq);
    r /= wq;
    const int oy = (int)(r % Hout);
    const int n = (int)(r / Hout);
    const int c0 = cg * KPV;
    float wr[9][KPV];
    load_w9<T>(w, c0, C, wr);
#pragma unroll
    for (int j = 0; j < DW_PX; ++j) {
      const int ox = xq * DW_PX + j;
      if (ox >= Wout) break;
      float acc[KPV];
#pragma unroll
      for (int e = 0; e < KPV; ++e) acc[e] = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        int iy;
        bool yok;
        if (MODE == 0) {
          iy = oy * stride - dil + ky * dil;
          yok = (unsigned)iy < (unsigned)Hin;
        } else {
          const int a = oy + dil - ky * dil;
          yok = a >= 0 && (a % stride) == 0;
          iy = a / stride;
          yok = yok && iy < Hin;
        }
        if (!yok) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          int ix;
          bool xok;
          if (MODE == 0) {
            ix = ox * stride - dil + kx * dil;
            xok = (unsigned)ix < (unsigned)Win;
          } else {
            const int a = ox + dil - kx * dil;
            xok = a >= 0 && (a % stride) == 0;
            ix = a / stride;
            xok = xok && ix < Win;
          }
          if (!xok) continue;
          float f[KPV];
          unpack(ldg16(in + ((size_t)(n * Hin + iy) * Win + ix) * ldin + c0), f, T());
          if (MODE == 0 && pscale != nullptr) dw_prologue<KPV>(f, pscale, pshift, prelu, c0);
#pragma unroll
          for (int e = 0; e < KPV; ++e) acc[e] = fmaf(f[e], wr[ky * 3 + kx][e], acc[e]);
        }
      }
      const size_t opix = (size_t)(n * Hout + oy) * Wout + ox;
      if (MODE == 1 && addend != nullptr) {
        float f[KPV];
        unpack(ldg16(addend + opix * ldadd + c0), f, T());
#pragma unroll
        for (int e = 0; e < KPV; ++e) acc[e] += f[e];
      }
      vec16 v;
      pack(v, acc, T());
      stg16(out + opix * ldout + c0, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stride-1 fast path (60 of the 63 depthwise layers).  The generic kernel above is latency-bound: it issues nine dependent
// batches of loads per pixel.  Here a thread owns DW_PX=4 consecutive output pixels of one channel group and first issues
// ALL loads of their 3 x (4+2*DIL) input window (18 or 24 independent 16-byte loads in flight), then does the arithmetic.
// The data gradient of a stride-1 depthwise conv is the same stencil with the taps reversed (FLIP) plus the optional addend.
template <typename T, int DIL, bool FLIP>
__global__ __launch_bounds__(256) void dw_s1_kernel(const T* __restrict__ in, int ldin, const float* __restrict__ wp,
                                                    const T* __restrict__ addend, int ldadd, T* __restrict__ out, int ldout,
                                                    int N, int H, int W, int C, const float* __restrict__ pscale,
                                                    const float* __restrict__ pshift, int prelu) {
  constexpr int KPV = Elem<T>::kPerVec;
  constexpr int WC = DW_PX + 2 * DIL;  // window columns
  const int ngroups = C / KPV;
  const int wq = (W + DW_PX - 1) / DW_PX;
  const int total = N * H * wq * ngroups;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cg = idx % ngroups;
  int r = idx / ngroups;
  const int xq = r % wq;
  r /= wq;
  const int oy = r % H;
  const int n = r / H;
  const int c0 = cg * KPV;
  const int x0 = xq * DW_PX;
  vec16 win[3][WC];
  unsigned inb = 0;   // bit (ky*WC + c): window element is inside the image
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy - DIL + ky * DIL;
    const bool yok = (unsigned)iy < (unsigned)H;
    const T* rowp = in + ((size_t)(n * H + (yok ? iy : 0)) * W) * ldin + c0;
#pragma unroll
    for (int c = 0; c < WC; ++c) {
      const int ix = x0 - DIL + c;
      const bool ok = yok && (unsigned)ix < (unsigned)W;
      win[ky][c] = ok ? ldg16(rowp + (size_t)ix * ldin) : zero16();
      inb |= (ok ? 1u : 0u) << (ky * WC + c);
    }
  }
  float acc[DW_PX][KPV];
#pragma unroll
  for (int j = 0; j < DW_PX; ++j)
#pragma unroll
    for (int e = 0; e < KPV; ++e) acc[j][e] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    float wk[3][KPV];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int t = FLIP ? 8 - (ky * 3 + kx) : ky * 3 + kx;
      const float4* src = reinterpret_cast<const float4*>(wp + (size_t)t * C + c0);
#pragma unroll
      for (int q = 0; q < KPV / 4; ++q) {
        const float4 v = src[q];
        wk[kx][4 * q] = v.x; wk[kx][4 * q + 1] = v.y; wk[kx][4 * q + 2] = v.z; wk[kx][4 * q + 3] = v.w;
      }
    }
#pragma unroll
    for (int c = 0; c < WC; ++c) {
      float f[KPV];
      unpack(win[ky][c], f, T());
      if (!FLIP && pscale != nullptr && ((inb >> (ky * WC + c)) & 1u)) dw_prologue<KPV>(f, pscale, pshift, prelu, c0);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int j = c - kx * DIL;          // output pixel that sees window column c through tap kx
        if (j >= 0 && j < DW_PX) {
#pragma unroll
          for (int e = 0; e < KPV; ++e) acc[j][e] = fmaf(f[e], wk[kx][e], acc[j][e]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < DW_PX; ++j) {
    const int ox = x0 + j;
    if (ox < W) {
      const size_t opix = (size_t)(n * H + oy) * W + ox;
      if (FLIP && addend != nullptr) {
        float f[KPV];
        unpack(ldg16(addend + opix * ldadd + c0), f, T());
#pragma unroll
        for (int e = 0; e < KPV; ++e) acc[j][e] += f[e];
      }
      vec16 v;
      pack(v, acc[j], T());
      stg16(out + opix * ldout + c0, v);
    }
  }
}

// Stride-1 weight gradient: a thread owns 4 consecutive pixels x one channel group, loads their dy and the 3 x (4+2*DIL)
// window of x at once, and adds the 9 x KPV products; lanes of a wave = consecutive channel groups (x pixel strips), the
// strips of a block are folded through LDS, one partial row per block goes to the slab.
template <typename T, int DIL>
__global__ __launch_bounds__(256) void dw_s1_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int lddy,
                                                          float* __restrict__ slab, int N, int H, int W, int C, int strips_per_block,
                                                          int cgw, const float* __restrict__ pscale,
                                                          const float* __restrict__ pshift, int prelu) {
  constexpr int KPV = Elem<T>::kPerVec;
  constexpr int WC = DW_PX + 2 * DIL;
  extern __shared__ __attribute__((aligned(16))) float red[];   // [256/cgw][9][cgw]
  const int ngroups = C / KPV;
  const int cgl = threadIdx.x % cgw, sl = threadIdx.x / cgw;   // lane -> (channel group, strip lane)
  const int nsl = 256 / cgw;
  const int cg = blockIdx.x * cgw + cgl;
  const int c0 = cg * KPV;
  const bool cok = cg < ngroups;
  const int wq = (W + DW_PX - 1) / DW_PX;
  const int nstrips = N * H * wq;
  const int sbeg = blockIdx.y * strips_per_block;
  const int send = min(nstrips, sbeg + strips_per_block);
  float acc[9][KPV];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < KPV; ++e) acc[t][e] = 0.f;
  if (cok) {
    for (int sidx = sbeg + sl; sidx < send; sidx += nsl) {
      const int xq = sidx % wq;
      int r = sidx / wq;
      const int oy = r % H;
      const int n = r / H;
      const int x0 = xq * DW_PX;
      vec16 g[DW_PX], win[3][WC];
      unsigned inb = 0;
#pragma unroll
      for (int j = 0; j < DW_PX; ++j)
        g[j] = (x0 + j < W) ? ldg16(dy + ((size_t)(n * H + oy) * W + x0 + j) * lddy + c0) : zero16();
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy - DIL + ky * DIL;
        const bool yok = (unsigned)iy < (unsigned)H;
        const T* rowp = x + ((size_t)(n * H + (yok ? iy : 0)) * W) * ldx + c0;
#pragma unroll
        for (int c = 0; c < WC; ++c) {
          const int ix = x0 - DIL + c;
          const bool ok = yok && (unsigned)ix < (unsigned)W;
          win[ky][c] = ok ? ldg16(rowp + (size_t)ix * ldx) : zero16();
          inb |= (ok ? 1u : 0u) << (ky * WC + c);
        }
      }
      float gf[DW_PX][KPV];
#pragma unroll
      for (int j = 0; j < DW_PX; ++j) unpack(g[j], gf[j], T());
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int c = 0; c < WC; ++c) {
          float f[KPV];
          unpack(win[ky][c], f, T());
          if (pscale != nullptr && ((inb >> (ky * WC + c)) & 1u)) dw_prologue<KPV>(f, pscale, pshift, prelu, c0);
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int j = c - kx * DIL;
            if (j >= 0 && j < DW_PX) {
#pragma unroll
              for (int e = 0; e < KPV; ++e) acc[ky * 3 + kx][e] = fmaf(gf[j][e], f[e], acc[ky * 3 + kx][e]);
            }
          }
        }
    }
  }
  // fold the strip lanes of the block, one channel element at a time
#pragma unroll
  for (int e = 0; e < KPV; ++e) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) red[(sl * 9 + t) * cgw + cgl] = acc[t][e];
    __syncthreads();
    for (int i = threadIdx.x; i < 9 * cgw; i += 256) {
      const int t = i / cgw, l = i % cgw;
      const int c = (blockIdx.x * cgw + l) * KPV + e;
      if (c < C) {
        float a = 0.f;
        for (int q = 0; q < nsl; ++q) a += red[(q * 9 + t) * cgw + l];
        slab[((size_t)blockIdx.y * 9 + t) * C + c] = a;
      }
    }
  }
}

// Weight gradient: dw[c][t] = sum over output pixels of dy[n,oy,ox,c] * x[n, oy*s - d + ky*d, ox*s - d + kx*d, c].
// A wave is tiled as CGW channel groups x (64/CGW) pixels so that thin layers (128 channels = 16 groups) still use all 64
// lanes; the pixel sub-lanes are folded with shuffles, the block's 4 waves through LDS, and every block leaves one
// partial row in slab[pixel block][9][C] (reduced in a fixed order afterwards: deterministic, no atomics).
template <typename T, int CGW>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ dy,
                                                       int lddy, float* __restrict__ slab, int N, int Hi, int Wi,
                                                       int Ho, int Wo, int C, int stride, int dil, int pix_per_block,
                                                       const float* __restrict__ pscale, const float* __restrict__ pshift,
                                                       int prelu) {
  constexpr int KPV = Elem<T>::kPerVec;
  constexpr int PPW = 64 / CGW;
  __shared__ float red[4][9][CGW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cgl = lane % CGW, psub = lane / CGW;
  const int cg = blockIdx.x * CGW + cgl;
  const int c0 = cg * KPV;
  const bool cok = c0 < C;
  const long P = (long)N * Ho * Wo;
  const long pbeg = (long)blockIdx.y * pix_per_block;
  const long pend = pbeg + pix_per_block < P ? pbeg + pix_per_block : P;
  float acc[9][KPV];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < KPV; ++e) acc[t][e] = 0.f;
  if (cok) {
    for (long pix = pbeg + wave * PPW + psub; pix < pend; pix += 4 * PPW) {
      const int ox = (int)(pix % Wo);
      const long r = pix / Wo;
      const int oy = (int)(r % Ho);
      const int n = (int)(r / Ho);
      float g[KPV];
      unpack(ldg16(dy + (size_t)pix * lddy + c0), g, T());
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - dil + ky * dil;
        if ((unsigned)iy >= (unsigned)Hi) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox * stride - dil + kx * dil;
          if ((unsigned)ix >= (unsigned)Wi) continue;
          float f[KPV];
          unpack(ldg16(x + ((size_t)(n * Hi + iy) * Wi + ix) * ldx + c0), f, T());
          if (pscale != nullptr) dw_prologue<KPV>(f, pscale, pshift, prelu, c0);
#pragma unroll
          for (int e = 0; e < KPV; ++e) acc[ky * 3 + kx][e] = fmaf(g[e], f[e], acc[ky * 3 + kx][e]);
        }
      }
    }
  }
  // fold the pixel sub-lanes of the wave
#pragma unroll
  for (int off = CGW; off < 64; off <<= 1)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < KPV; ++e) acc[t][e] += __shfl_xor(acc[t][e], off, 64);
  // combine the 4 waves, one channel element at a time
#pragma unroll
  for (int e = 0; e < KPV; ++e) {
    __syncthreads();
    if (psub == 0)
#pragma unroll
      for (int t = 0; t < 9; ++t) red[wave][t][cgl] = acc[t][e];
    __syncthreads();
    for (int i = threadIdx.x; i < 9 * CGW; i += 256) {
      const int t = i / CGW, l = i % CGW;
      const int c = (blockIdx.x * CGW + l) * KPV + e;
      if (c < C) slab[((size_t)blockIdx.y * 9 + t) * C + c] = red[0][t][l] + red[1][t][l] + red[2][t][l] + red[3][t][l];
    }
  }
}

// grad[c][t] = sum over rows of slab[row][t][c]: 8 columns x 32 row-lanes per block, fp64, fixed order
__global__ __launch_bounds__(256) void dw_wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ grad, int rows, int C) {
  __shared__ double red[32][8];
  const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int n = 9 * C;
  const int i = blockIdx.x * 8 + cl;
  double a = 0.0;
  if (i < n)
    for (int r = rl; r < rows; r += 32) a += (double)slab[(size_t)r * n + i];
  red[rl][cl] = a;
  __syncthreads();
  if (threadIdx.x < 8 && blockIdx.x * 8 + threadIdx.x < n) {
    const int j = blockIdx.x * 8 + threadIdx.x;
    double s2 = 0.0;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) s2 += red[k][threadIdx.x];
    const int t = j / C, c = j % C;
    grad[(size_t)c * 9 + t] = (float)s2;
  }
}

// channel groups per wave row: the power of two that wastes the fewest lanes (ties -> wider, better coalescing)
static int dw_pick_cgw(int ngroups) {
  int best = 64, waste = cdiv(ngroups, 64) * 64 - ngroups;
  for (int w = 32; w >= 8; w >>= 1) {
    const int ws = cdiv(ngroups, w) * w - ngroups;
    if (ws < waste) { best = w; waste = ws; }
  }
  return best;
}

static int dw_out(int Hi, int stride, int dil) { return (Hi + 2 * dil - 2 * dil - 1) / stride + 1; }
static int dw_pix_per_block(long P) {
  long ppb = (P + 255) / 256;  // at most 256 pixel blocks (= slab rows)
  if (ppb < 32) ppb = 32;
  return (int)ppb;
}

// The one routing decision (dwtile.h): the queries the engine sizes its slabs from and the dispatchers read the same answer.
DwRoute dw_route(DwDir dir, int dtype, int C, int stride, int dil, int N, int Hi, int Wi) {
  if ((dtype != DC_BF16 && dtype != DC_F32) || C <= 0 || N <= 0 || Hi <= 0 || Wi <= 0) return {DW_NONE, 0};
  if (stride == 1 && (dil == 1 || dil == 2)) {
    if (!g_options.dw_tile) return {DW_WIN, 0};
    // the persistent pipelined kernel serves the data gradients (52.0 -> 41.5 us with BatchNorm sums and weight gradient on the 728-channel
    // layers at local batch 8); the forward pass stays on the tiled kernel unless option "dw_pipe" = 2 (23.4 vs 24.1 us plain, 34.5 vs
    // 31.7 us with the BatchNorm applied on load: its in-place transform pass costs eight waves more than it costs three co-resident
    // workgroups).  It is not given tensors of 2^31 pixels or more: the tiled launcher gets those calls, and refuses them.
    const bool piped = dir == DW_DGRAD || (dir == DW_FWD && dw_pipe_forward());
    const int pr = piped && (long)N * Hi * Wi < (1L << 31) ? dw_pipe_rows(dtype, C, dil, N, Hi, Wi) : 0;   // one slab row per workgroup
    if (pr > 0) return {DW_PIPE, pr};
    return {DW_TILE, dw_tile_rows(dtype, C, N, Hi, Wi)};
  }
  // the stride-2 data-gradient kernel walks its tiles: one row per workgroup
  if (stride == 2 && dil == 1 && g_options.dw_tile) return {DW_TILE_S2, dw_tile_s2_dgrad_rows(dtype, C, N, Hi, Wi)};
  return {DW_REG, 0};
}

}  // namespace dc

using namespace dc;

// the generic kernel: any stride and dilation
static int launch_dw(const DwCall& c) {
  const int Ho = dw_out(c.Hi, c.stride, c.dil), Wo = dw_out(c.Wi, c.stride, c.dil);
  // forward: x [Hi,Wi] -> y [Ho,Wo]; data gradient: gather from dy [Ho,Wo] into dx [Hi,Wi]
  const int Hin = c.flip ? Ho : c.Hi, Win = c.flip ? Wo : c.Wi, Hout = c.flip ? c.Hi : Ho, Wout = c.flip ? c.Wi : Wo;
  const long total = (long)c.N * Hout * ((Wout + DW_PX - 1) / DW_PX) * (c.C / (c.dtype == DC_BF16 ? 8 : 4));
  long blocks = (total + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
#define DW(TT, MODE) hipLaunchKernelGGL((dw_kernel<TT, MODE>), dim3((int)blocks), dim3(256), 0, c.st, (const TT*)c.in, c.ldin, c.wp, (const TT*)c.addend, c.ldadd, (TT*)c.out, c.ldout, c.N, Hin, Win, Hout, Wout, c.C, c.stride, c.dil, c.pscale, c.pshift, c.prelu)
  if (c.dtype == DC_BF16) { if (c.flip) DW(bf16, 1); else DW(bf16, 0); }
  else                    { if (c.flip) DW(float, 1); else DW(float, 0); }
#undef DW
  DC_LAUNCHED(c.flip ? "dw_reg_dgrad" : "dw_reg_fwd");
  return 0;
}

// the stride-1 register-window kernels (option "dw_tile" = 0)
static int launch_dw_s1(const DwCall& c) {
  const long total = (long)c.N * c.Hi * ((c.Wi + DW_PX - 1) / DW_PX) * (c.C / (c.dtype == DC_BF16 ? 8 : 4));
  DC_REQUIRE(total < (1L << 31), "dc_dwconv: tensor too large for the stride-1 fast path");
  dim3 grid((unsigned)((total + 255) / 256));
#define DW_S1(TT, D, F) hipLaunchKernelGGL((dw_s1_kernel<TT, D, F>), grid, dim3(256), 0, c.st, (const TT*)c.in, c.ldin, c.wp, (const TT*)c.addend, c.ldadd, (TT*)c.out, c.ldout, c.N, c.Hi, c.Wi, c.C, c.pscale, c.pshift, c.prelu)
  DW_S1_CASES(c, DW_S1)
#undef DW_S1
  DC_LAUNCHED(c.flip ? "dw_win_dgrad" : "dw_win_fwd");
  return 0;
}

static int dw_dispatch(const DwCall& c) {
  switch (dw_route(c.flip ? DW_DGRAD : DW_FWD, c.dtype, c.C, c.stride, c.dil, c.N, c.Hi, c.Wi).family) {
    case DW_PIPE: return launch_dw_pipe(c);
    case DW_TILE: return launch_dw_tile(c);
    case DW_TILE_S2: return launch_dw_tile_s2(c);
    case DW_WIN: return launch_dw_s1(c);
    case DW_REG: return launch_dw(c);
    default: return dc_fail("dc_dwconv: shape not served", __FILE__, __LINE__);
  }
}

static int dw_check(int dtype, int C, int stride, int dil, int N, int Hi, int Wi) {
  DC_REQUIRE(dtype == DC_F32 || dtype == DC_BF16, "dc_dwconv: bad dtype");
  DC_REQUIRE(stride == 1 || stride == 2, "dc_dwconv: stride must be 1 or 2");
  DC_REQUIRE(dil >= 1 && C > 0 && N > 0 && Hi > 0 && Wi > 0, "dc_dwconv: bad shape");
  return 0;
}

// The argument check of the forward and data-gradient entry points: the shape; the views of in ("x" / "dy") and out ("y" / "dx"), of the
// rider's tensor c.bs.y under the name the entry point gives it (null: the call has none), of the residual BatchNorm's input and of an
// addend that is there; then the entry point's own requirements in order, each with its refusal.  `name`: the entry point in view errors.
struct DwReq { bool ok; const char* msg; };
static int dw_check_call(const char* name, const DwCall& c, const char* rider, std::initializer_list<DwReq> reqs) {
  const auto view = [&](const void* p, int ld, const char* what) {
    char full[96];
    snprintf(full, sizeof(full), "%s %s", name, what);
    return dc_check_view(p, ld, c.C, c.dtype, full);
  };
  int e = dw_check(c.dtype, c.C, c.stride, c.dil, c.N, c.Hi, c.Wi);
  if (!e) e = view(c.in, c.ldin, c.flip ? "dy" : "x");
  if (!e) e = view(c.out, c.ldout, c.flip ? "dx" : "y");
  if (!e && rider != nullptr) e = view(c.bs.y, c.bs.ldy, rider);
  if (!e && c.res.on()) e = view(c.res.y, c.res.ldy, "ybn");
  if (!e && c.addend != nullptr) e = view(c.addend, c.ldadd, "addend");
  for (const DwReq& r : reqs)
    if (!e && !r.ok) e = dc_fail(r.msg, __FILE__, __LINE__);
  return e;
}

// a call's shape, in the order every entry point of the C ABI lists it, its direction and its stream
static DwCall dw_call(bool flip, int dtype, int C, int stride, int dil, int N, int Hi, int Wi, void* stream) {
  DwCall c;
  c.flip = flip; c.dtype = dtype; c.C = C; c.stride = stride; c.dil = dil; c.N = N; c.Hi = Hi; c.Wi = Wi; c.st = (hipStream_t)stream;
  return c;
}

// The riders of a data gradient.  bn_rider: the sums of the BatchNorm in front of the layer (input ybn; a SUM ROW when sum_row) and, with
// wslab, this layer's weight-gradient rows, its forward input being act(ybn*mscale + mshift).  wgrad_rider: the weight-gradient rows alone,
// the forward input being the stored x, or act(x*pscale + pshift) of it.  (DwBnStats in member order: y, ldy, mean, invstd, mscale, mshift, relu,
// slab, rows, wslab)
static DwBnStats bn_rider(const void* ybn, int ldybn, const float* mean, const float* invstd, const float* mscale, const float* mshift, int relu,
                          float* slab, float* wslab = nullptr, bool sum_row = false) {
  return {ybn, ldybn, mean, invstd, mscale, mshift, relu ? 1 : 0, slab, sum_row ? SUM_ROW : 0, wslab};
}
static DwBnStats wgrad_rider(const void* x, int ldx, const float* pscale, const float* pshift, int prelu, float* wslab) {
  return {x, ldx, nullptr, nullptr, pscale, pshift, (pscale != nullptr && prelu) ? 1 : 0, nullptr, 0, wslab};
}

extern "C" int dc_dwconv_pack_weights(int C, const float* master, float* packed, void* stream) {
  DC_REQUIRE(C > 0 && C % 4 == 0 && master && packed, "dc_dwconv_pack_weights: bad argument");
  DC_REQUIRE(((uintptr_t)packed & 15) == 0, "dc_dwconv_pack_weights: packed buffer must be 16-byte aligned");
  hipLaunchKernelGGL(dw_pack_kernel, dim3(cdiv(9 * C, 256)), dim3(256), 0, (hipStream_t)stream, master, packed, C);
  DC_CHECK_LAUNCH();
  return 0;
}

extern "C" int dc_dwconv_fwd(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* x, int ldx,
                             const float* w, void* y, int ldy, const float* pscale, const float* pshift, int prelu,
                             void* stream) {
  DwCall c = dw_call(false, dtype, C, stride, dil, N, Hi, Wi, stream);
  c.in = x; c.ldin = ldx; c.wp = w; c.out = y; c.ldout = ldy; c.pscale = pscale; c.pshift = pshift; c.prelu = prelu;
  if (int e = dw_check_call("dc_dwconv_fwd", c, nullptr, {{w != nullptr, "dc_dwconv_fwd: null weights"},
                            {(pscale == nullptr) == (pshift == nullptr), "dc_dwconv_fwd: pscale and pshift go together"}})) return e;
  return dw_dispatch(c);
}

// dc_dwconv_fwd reading through a BatchNorm(+ReLU) whose finalize it runs itself: the producer left a SHORT slab of partial sums
// (rows <= dc_bn_bwd_apply_fin_max_rows()), every workgroup sums it for its own channels while its halo tile travels (same order, same bits as
// dc_bn_finalize), the workgroups of pixel tile 0 store scale / shift / save_mean / save_invstd and the running statistics.
extern "C" int dc_dwconv_fwd_fin_ok(int dtype, int C, int stride, int dil, int N, int Hi, int Wi) {
  return !dw_pipe_forward() && dw_route(DW_FWD, dtype, C, stride, dil, N, Hi, Wi).family == DW_TILE && C % (dtype == DC_BF16 ? 8 : 4) == 0;
}
extern "C" int dc_dwconv_fwd_fin(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* x, int ldx, const float* w,
                                 void* y, int ldy, int prelu, long count, const float* slab, int rows, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                 float* scale, float* shift, float* save_mean, float* save_invstd, void* stream) {
  DwCall c = dw_call(false, dtype, C, stride, dil, N, Hi, Wi, stream);
  c.in = x; c.ldin = ldx; c.wp = w; c.out = y; c.ldout = ldy; c.prelu = prelu;
  if (int e = dw_check_call("dc_dwconv_fwd_fin", c, nullptr,
                            {{w && slab && gamma && beta && scale && shift && (rows > 0 || rows == SUM_ROW), "dc_dwconv_fwd_fin: null argument"},
                             {((uintptr_t)slab & 15) == 0, "dc_dwconv_fwd_fin: the slab is read with 16-byte loads (16-byte aligned)"},
                             {dc_dwconv_fwd_fin_ok(dtype, C, stride, dil, N, Hi, Wi) != 0, "dc_dwconv_fwd_fin: shape not served (dc_dwconv_fwd_fin_ok)"},
                             {count > 1, "Expected more than 1 value per channel when training"}})) return e;
  const BnFinArgs a = bn_fin_args(C, count, slab, rows, 0, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, scale,
                                  shift, save_mean, save_invstd);
  c.fin = &a;
  return dw_dispatch(c);
}

extern "C" int dc_dwconv_dgrad(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                               const float* w, const void* addend, int ldadd, void* dx, int lddx, void* stream) {
  DwCall c = dw_call(true, dtype, C, stride, dil, N, Hi, Wi, stream);
  c.in = dy; c.ldin = lddy; c.wp = w; c.addend = addend; c.ldadd = ldadd; c.out = dx; c.ldout = lddx;
  if (int e = dw_check_call("dc_dwconv_dgrad", c, nullptr, {{w != nullptr, "dc_dwconv_dgrad: null weights"}})) return e;
  return dw_dispatch(c);
}

// slab rows of the BatchNorm sums that ride along with the data gradient; 0: the register kernels serve the shape, they take no riders
extern "C" int dc_dwconv_dgrad_bnstats_rows(int dtype, int C, int stride, int dil, int N, int Hi, int Wi) {
  return dw_route(DW_DGRAD, dtype, C, stride, dil, N, Hi, Wi).rows;
}

extern "C" int dc_dwconv_dgrad_bnstats(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                       const float* w, void* dx, int lddx, const void* ybn, int ldybn, const float* save_mean,
                                       const float* save_invstd, const float* mscale, const float* mshift, int relu, float* slab,
                                       void* stream) {
  DwCall c = dw_call(true, dtype, C, stride, dil, N, Hi, Wi, stream);
  c.in = dy; c.ldin = lddy; c.wp = w; c.out = dx; c.ldout = lddx;
  c.bs = bn_rider(ybn, ldybn, save_mean, save_invstd, mscale, mshift, relu, slab);
  if (int e = dw_check_call("dc_dwconv_dgrad_bnstats", c, "y", {{w && save_mean && save_invstd && slab, "dc_dwconv_dgrad_bnstats: null argument"},
                             {!relu || (mscale && mshift), "dc_dwconv_dgrad_bnstats: the ReLU mask needs the forward scale / shift vectors"},
                             {dc_dwconv_dgrad_bnstats_rows(dtype, C, stride, dil, N, Hi, Wi) > 0, "dc_dwconv_dgrad_bnstats: shape not served by the tiled kernels"}})) return e;
  return dw_dispatch(c);
}

// The same with THIS depthwise layer's weight gradient taken from the same dy window (tiled and pipelined kernels, at most DWT_MAX_ROWS
// rows): wslab receives dc_dwconv_dgrad_wgrad_rows rows of [9][C] partial sums; dc_dwconv_wgrad_reduce adds them into grad_w.  The
// layer's forward input is act(ybn*mscale + mshift) (the never-stored BatchNorm output), so nothing is read that the data gradient
// with statistics does not read already.
extern "C" int dc_dwconv_dgrad_wgrad_rows(int dtype, int C, int stride, int dil, int N, int Hi, int Wi) {
  const int rows = dw_route(DW_DGRAD, dtype, C, stride, dil, N, Hi, Wi).rows;
  return rows > 0 && rows <= DWT_MAX_ROWS ? rows : 0;
}

// 1: the data gradients that take BatchNorm sums (dc_dwconv_dgrad_bnstats_wgrad_sum, dc_dwconv_dgrad_wgrad_bnres_sum) serve this shape: the
// persistent pipelined kernel (dwpipe.hip), whose workgroups add their sums to ONE fp64 row (bn_fin.h: SUM_ROW)
extern "C" int dc_dwconv_dgrad_sum_row_ok(int dtype, int C, int stride, int dil, int N, int Hi, int Wi) {
  return dw_route(DW_DGRAD, dtype, C, stride, dil, N, Hi, Wi).family == DW_PIPE;
}

// the three forms of dc_dwconv_dgrad_bnstats_wgrad: plain, with a sum row (which names the plain form in what both check), onto an addend
enum BnwForm { BNW_PLAIN, BNW_SUM, BNW_ADD };
static int dgrad_bnstats_wgrad_impl(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy, const float* w,
                                    const void* addend, int ldadd, void* dx, int lddx, const void* ybn, int ldybn, const float* save_mean,
                                    const float* save_invstd, const float* mscale, const float* mshift, int relu, float* slab, float* wslab,
                                    void* stream, BnwForm form) {
  const bool sum_row = form == BNW_SUM, add = form == BNW_ADD;
  DwCall c = dw_call(true, dtype, C, stride, dil, N, Hi, Wi, stream);
  c.in = dy; c.ldin = lddy; c.wp = w; c.addend = addend; c.ldadd = ldadd; c.out = dx; c.ldout = lddx;
  c.bs = bn_rider(ybn, ldybn, save_mean, save_invstd, mscale, mshift, relu, slab, wslab, sum_row);
  if (int e = dw_check_call(add ? "dc_dwconv_dgrad_bnstats_wgrad_add" : "dc_dwconv_dgrad_bnstats_wgrad", c, "y",
                            {{!add || stride == 1, "dc_dwconv_dgrad_bnstats_wgrad_add: stride 1"},
                             {w && save_mean && save_invstd && slab && wslab && mscale && mshift,
                              add ? "dc_dwconv_dgrad_bnstats_wgrad_add: null argument" : "dc_dwconv_dgrad_bnstats_wgrad: null argument"},
                             {dc_dwconv_dgrad_wgrad_rows(dtype, C, stride, dil, N, Hi, Wi) > 0,
                              add ? "dc_dwconv_dgrad_bnstats_wgrad_add: shape not served" : "dc_dwconv_dgrad_bnstats_wgrad: shape not served"},
                             {!sum_row || (dc_dwconv_dgrad_sum_row_ok(dtype, C, stride, dil, N, Hi, Wi) && ((uintptr_t)slab & 7) == 0),
                              "dc_dwconv_dgrad_bnstats_wgrad_sum: shape not served (dc_dwconv_dgrad_sum_row_ok), or the sum row is not double[2][C]"}})) return e;
  return dw_dispatch(c);
}
extern "C" int dc_dwconv_dgrad_bnstats_wgrad(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                             const float* w, void* dx, int lddx, const void* ybn, int ldybn, const float* save_mean,
                                             const float* save_invstd, const float* mscale, const float* mshift, int relu, float* slab,
                                             float* wslab, void* stream) {
  return dgrad_bnstats_wgrad_impl(dtype, C, stride, dil, N, Hi, Wi, dy, lddy, w, nullptr, 0, dx, lddx, ybn, ldybn, save_mean, save_invstd, mscale, mshift,
                                  relu, slab, wslab, stream, BNW_PLAIN);
}
// ... with the two BatchNorm sums added to a SUM ROW: `slab` is double[2][C] (sum g, sum g*xhat), zeroed by the caller; dc_bn_bwd_finalize and
// dc_bn_bwd_apply_fin take it with rows = -1
extern "C" int dc_dwconv_dgrad_bnstats_wgrad_sum(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                                 const float* w, void* dx, int lddx, const void* ybn, int ldybn, const float* save_mean,
                                                 const float* save_invstd, const float* mscale, const float* mshift, int relu, float* slab,
                                                 float* wslab, void* stream) {
  return dgrad_bnstats_wgrad_impl(dtype, C, stride, dil, N, Hi, Wi, dy, lddy, w, nullptr, 0, dx, lddx, ybn, ldybn, save_mean, save_invstd, mscale, mshift,
                                  relu, slab, wslab, stream, BNW_SUM);
}
// ... when this layer is not the only reader of the BatchNorm's output: the data gradient is added onto what the
// other readers left in `addend` (may alias dx) and the sums are those of the COMPLETE gradient -- the caller makes this layer the last
// writer (block 1's first depthwise layer behind the shortcut conv: the BatchNorm in front of both is bn2, whose 226 MB output gradient and
// input a separate dc_bn_bwd_reduce pass would read once more).  Stride 1.
extern "C" int dc_dwconv_dgrad_bnstats_wgrad_add(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                                 const float* w, const void* addend, int ldadd, void* dx, int lddx, const void* ybn, int ldybn,
                                                 const float* save_mean, const float* save_invstd, const float* mscale, const float* mshift, int relu,
                                                 float* slab, float* wslab, void* stream) {
  return dgrad_bnstats_wgrad_impl(dtype, C, stride, dil, N, Hi, Wi, dy, lddy, w, addend, ldadd, dx, lddx, ybn, ldybn, save_mean, save_invstd, mscale, mshift,
                                  relu, slab, wslab, stream, BNW_ADD);
}

// Data gradient (optionally accumulated onto `addend`) plus this layer's weight-gradient rows when the layer's forward input is a
// STORED tensor x (pscale == null) or act(x*pscale + pshift) of one: the first separable conv of an Xception block, whose input is the
// block input and whose data gradient joins the shortcut's.
extern "C" int dc_dwconv_dgrad_wgrad(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                     const float* w, const void* addend, int ldadd, void* dx, int lddx, const void* x, int ldx,
                                     const float* pscale, const float* pshift, int prelu, float* wslab, void* stream) {
  DwCall c = dw_call(true, dtype, C, stride, dil, N, Hi, Wi, stream);
  c.in = dy; c.ldin = lddy; c.wp = w; c.addend = addend; c.ldadd = ldadd; c.out = dx; c.ldout = lddx;
  c.bs = wgrad_rider(x, ldx, pscale, pshift, prelu, wslab);
  if (int e = dw_check_call("dc_dwconv_dgrad_wgrad", c, "x", {{w && wslab && (pscale == nullptr) == (pshift == nullptr), "dc_dwconv_dgrad_wgrad: bad argument"},
                             {dc_dwconv_dgrad_wgrad_rows(dtype, C, stride, dil, N, Hi, Wi) > 0, "dc_dwconv_dgrad_wgrad: shape not served"}})) return e;
  return dw_dispatch(c);
}

// dc_dwconv_dgrad_wgrad on a layer whose stored input x is a BatchNorm output with a residual, relu(bn(ybn) + r) -- the first separable conv
// of an Xception block reading the previous block's output -- and whose data gradient is the LAST contribution to d(x): the kernel also
// takes that BatchNorm's backward sums (g = dx masked by x > 0 when relu; slab[2][rows][C]), so dc_bn_bwd_reduce's pass over dx, ybn and x
// disappears.  Served by the persistent kernel only, at dilation 1 (rows = 0: use dc_dwconv_dgrad_wgrad + dc_bn_bwd_reduce).
// relu = 2 (where dc_dwconv_dgrad_wgrad_bnres_masked says 1): dx is stored masked by x > 0 as well, i.e. as the g that BatchNorm's apply pass
// and the shortcut need -- dc_bn_bwd_apply then runs with relu = 0, reads no `out` and writes no `g_out`.
extern "C" int dc_dwconv_dgrad_wgrad_bnres_rows(int dtype, int C, int stride, int dil, int N, int Hi, int Wi) {
  const DwRoute r = dw_route(DW_DGRAD, dtype, C, stride, dil, N, Hi, Wi);
  return r.family == DW_PIPE && dil == 1 ? r.rows : 0;
}
extern "C" int dc_dwconv_dgrad_wgrad_bnres_masked(int dtype, int C, int stride, int dil, int N, int Hi, int Wi) {
  return g_options.dw_res_masked && dc_dwconv_dgrad_wgrad_bnres_rows(dtype, C, stride, dil, N, Hi, Wi) > 0 ? 1 : 0;
}

static int dgrad_wgrad_bnres_impl(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                  const float* w, const void* addend, int ldadd, void* dx, int lddx, const void* x, int ldx,
                                  float* wslab, const void* ybn, int ldybn, const float* save_mean, const float* save_invstd,
                                  int relu, float* slab, void* stream, bool sum_row) {
  DwCall c = dw_call(true, dtype, C, stride, dil, N, Hi, Wi, stream);
  c.in = dy; c.ldin = lddy; c.wp = w; c.addend = addend; c.ldadd = ldadd; c.out = dx; c.ldout = lddx;
  c.bs = wgrad_rider(x, ldx, nullptr, nullptr, 0, wslab);
  c.res.y = ybn; c.res.ldy = ldybn; c.res.mean = save_mean; c.res.invstd = save_invstd; c.res.relu = relu; c.res.slab = slab; c.res.sum_row = sum_row ? 1 : 0;
  if (int e = dw_check_call("dc_dwconv_dgrad_wgrad_bnres", c, "x", {{w && wslab && save_mean && save_invstd && slab, "dc_dwconv_dgrad_wgrad_bnres: null argument"},
                             {dc_dwconv_dgrad_wgrad_bnres_rows(dtype, C, stride, dil, N, Hi, Wi) > 0, "dc_dwconv_dgrad_wgrad_bnres: shape not served"},
                             {relu >= 0 && relu <= 2, "dc_dwconv_dgrad_wgrad_bnres: relu is 0, 1 (mask the sums) or 2 (mask the sums and the stored dx)"},
                             {relu != 2 || dc_dwconv_dgrad_wgrad_bnres_masked(dtype, C, stride, dil, N, Hi, Wi), "dc_dwconv_dgrad_wgrad_bnres: relu = 2 is switched off (option dw_res_masked)"},
                             {!sum_row || ((uintptr_t)slab & 7) == 0, "dc_dwconv_dgrad_wgrad_bnres_sum: a sum row is double[2][C]"}})) return e;
  return dw_dispatch(c);
}
extern "C" int dc_dwconv_dgrad_wgrad_bnres(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                           const float* w, const void* addend, int ldadd, void* dx, int lddx, const void* x, int ldx,
                                           float* wslab, const void* ybn, int ldybn, const float* save_mean, const float* save_invstd,
                                           int relu, float* slab, void* stream) {
  return dgrad_wgrad_bnres_impl(dtype, C, stride, dil, N, Hi, Wi, dy, lddy, w, addend, ldadd, dx, lddx, x, ldx, wslab, ybn, ldybn, save_mean, save_invstd,
                                relu, slab, stream, false);
}
// ... with the residual BatchNorm's two sums added to a SUM ROW (double[2][C], zeroed by the caller; served wherever the plain form is)
extern "C" int dc_dwconv_dgrad_wgrad_bnres_sum(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                               const float* w, const void* addend, int ldadd, void* dx, int lddx, const void* x, int ldx,
                                               float* wslab, const void* ybn, int ldybn, const float* save_mean, const float* save_invstd,
                                               int relu, float* slab, void* stream) {
  return dgrad_wgrad_bnres_impl(dtype, C, stride, dil, N, Hi, Wi, dy, lddy, w, addend, ldadd, dx, lddx, x, ldx, wslab, ybn, ldybn, save_mean, save_invstd,
                                relu, slab, stream, true);
}

extern "C" int dc_dwconv_wgrad_reduce(int C, int rows, const float* wslab, float* grad_w, void* stream) {
  DC_REQUIRE(C > 0 && rows > 0 && wslab && grad_w, "dc_dwconv_wgrad_reduce: bad argument");
  return dw_tile_reduce(wslab, grad_w, rows, C, (hipStream_t)stream);
}

extern "C" size_t dc_dwconv_wgrad_workspace(int C, int N, int Hi, int Wi, int stride) {
  const int Ho = dw_out(Hi, stride, 1), Wo = dw_out(Wi, stride, 1);
  const long P = (long)N * Ho * Wo;
  const int ppb = dw_pix_per_block(P);
  int rows = (int)((P + ppb - 1) / ppb);
  if (rows < 256) rows = 256;            // the stride-1 register-window path uses up to 256 slab rows
  size_t bytes = (size_t)rows * 9 * C * sizeof(float);
  if (stride == 1) {
    const size_t tb = dw_tile_wgrad_workspace(C, N, Hi, Wi);
    if (tb > bytes) bytes = tb;
  } else {
    long tiles = (long)N * cdiv(Ho, 4) * cdiv(Wo, 8);           // stride-2 tiled path: 4 x (8..32) output tiles, one slab row each at most
    if (tiles > DWT_MAX_ROWS) tiles = DWT_MAX_ROWS;
    const size_t tb = (size_t)tiles * 9 * C * sizeof(float);
    if (tb > bytes) bytes = tb;
  }
  return bytes;
}

extern "C" int dc_dwconv_wgrad(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* x, int ldx,
                               const void* dy, int lddy, void* workspace, float* grad_w, const float* pscale,
                               const float* pshift, int prelu, void* stream) {
  if (int e = dw_check(dtype, C, stride, dil, N, Hi, Wi)) return e;
  if (int e = dc_check_view(x, ldx, C, dtype, "dc_dwconv_wgrad x")) return e;
  if (int e = dc_check_view(dy, lddy, C, dtype, "dc_dwconv_wgrad dy")) return e;
  DC_REQUIRE(workspace != nullptr && grad_w != nullptr, "dc_dwconv_wgrad: null argument");
  DwWgradCall c;
  c.dtype = dtype; c.stride = stride; c.dil = dil; c.N = N; c.C = C; c.Hi = Hi; c.Wi = Wi; c.st = (hipStream_t)stream;
  c.x = x; c.ldx = ldx; c.dy = dy; c.lddy = lddy; c.slab = (float*)workspace; c.grad_w = grad_w; c.pscale = pscale; c.pshift = pshift; c.prelu = prelu;
  const DwFamily family = dw_route(DW_WGRAD, dtype, C, stride, dil, N, Hi, Wi).family;
  if (family == DW_TILE) return launch_dw_tile_wgrad(c);
  if (family == DW_TILE_S2) return launch_dw_tile_s2_wgrad(c);
  // the register kernels: the stride-1 window form (option "dw_tile" = 0), or the generic one for any stride and dilation
  const int kpv = dtype == DC_BF16 ? 8 : 4;
  const int cgw = dw_pick_cgw(C / kpv);
  int rows;
  if (family == DW_WIN) {
    const int nstrips = N * Hi * ((Wi + DW_PX - 1) / DW_PX);
    const int nsl = 256 / cgw;
    int spb = cdiv(nstrips, 256);
    if (spb < 2 * nsl) spb = 2 * nsl;
    spb = cdiv(spb, nsl) * nsl;
    rows = cdiv(nstrips, spb);
    dim3 fgrid(cdiv(C / kpv, cgw), rows);
    const size_t lds = (size_t)256 * 9 * sizeof(float);
#define DW_WS1(TT, D) hipLaunchKernelGGL((dw_s1_wgrad_kernel<TT, D>), fgrid, dim3(256), lds, c.st, (const TT*)c.x, c.ldx, (const TT*)c.dy, c.lddy, c.slab, N, Hi, Wi, C, spb, cgw, c.pscale, c.pshift, c.prelu)
    if (dtype == DC_BF16) { if (dil == 1) DW_WS1(bf16, 1); else DW_WS1(bf16, 2); }
    else                  { if (dil == 1) DW_WS1(float, 1); else DW_WS1(float, 2); }
#undef DW_WS1
    DC_LAUNCHED("dw_win_wgrad");
  } else {
    const int Ho = dw_out(Hi, stride, dil), Wo = dw_out(Wi, stride, dil);
    const long P = (long)N * Ho * Wo;
    const int ppb = dw_pix_per_block(P);
    rows = (int)((P + ppb - 1) / ppb);
    dim3 grid(cdiv(C / kpv, cgw), rows);
#define DW_WG(TT, W) hipLaunchKernelGGL((dw_wgrad_kernel<TT, W>), grid, dim3(256), 0, c.st, (const TT*)c.x, c.ldx, (const TT*)c.dy, c.lddy, c.slab, N, Hi, Wi, Ho, Wo, C, stride, dil, ppb, c.pscale, c.pshift, c.prelu)
    if (dtype == DC_BF16) {
      if (cgw == 64) DW_WG(bf16, 64); else if (cgw == 32) DW_WG(bf16, 32); else if (cgw == 16) DW_WG(bf16, 16); else DW_WG(bf16, 8);
    } else {
      if (cgw == 64) DW_WG(float, 64); else if (cgw == 32) DW_WG(float, 32); else if (cgw == 16) DW_WG(float, 16); else DW_WG(float, 8);
    }
#undef DW_WG
    DC_LAUNCHED("dw_reg_wgrad");
  }
  hipLaunchKernelGGL(dw_wgrad_reduce_kernel, dim3(cdiv(9 * C, 8)), dim3(256), 0, c.st, (const float*)c.slab, grad_w, rows, C);
  DC_LAUNCHED("dw_reg_reduce");
  return 0;
}
