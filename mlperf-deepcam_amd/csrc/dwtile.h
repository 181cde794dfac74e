// Host side of the depthwise 3x3 layers: the call records the C ABI in dwconv.hip fills, the route that names the kernel family serving a
// shape, and one launcher per family (dwtile.hip: stride 1, dwpipe.hip: persistent stride 1, dwtile_s2.hip: stride 2; the register
// kernels are dwconv.hip's own).  A launcher launches its own kernels and nothing else: dw_route decides, dwconv.hip dispatches on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "dwtile_common.h"

namespace dc {

struct BnFinArgs;   // bn_fin.h
// the BatchNorm whose stored output relu(bn(y) + residual) is a depthwise layer's input: its backward sums ride along with that layer's data
// gradient (dwpipe.hip, PM_RES)
struct DwResStats {
  const void* y = nullptr; int ldy = 0;
  const float* mean = nullptr; const float* invstd = nullptr; int relu = 0;
  float* slab = nullptr;   // null: off
  bool on() const { return slab != nullptr; }
  int sum_row = 0;  // slab is a SUM ROW (bn_fin.h): double[2][C], zeroed by the caller, added to by every workgroup
};

// One forward (flip = false: in = x, out = y) or data-gradient (flip = true: in = dy, out = dx) launch.  Value-initialised it is a plain
// forward pass with every rider off.  Hi, Wi are the FORWARD layer's input extents, as in the C ABI; a launcher derives the ones it needs.
struct DwCall {
  int dtype = DC_F32, stride = 1, dil = 1, N = 0, C = 0, Hi = 0, Wi = 0;
  bool flip = false;
  const void* in = nullptr; int ldin = 0;
  const float* wp = nullptr;                                // packed taps [9][C]
  const void* addend = nullptr; int ldadd = 0;              // data gradient only: dx = conv + addend (may alias out)
  void* out = nullptr; int ldout = 0;
  const float* pscale = nullptr; const float* pshift = nullptr; int prelu = 0;   // forward: BatchNorm (+ReLU) applied to `in` as it is loaded
  DwBnStats bs;                     // data gradient: BatchNorm sums (bs.slab) and / or this layer's weight-gradient rows (bs.wslab)
  DwResStats res;                   // data gradient on the pipelined kernel: the residual BatchNorm's sums
  const BnFinArgs* fin = nullptr;   // forward on the tiled kernel: the producing BatchNorm's finalize runs in the kernel
  hipStream_t st = nullptr;
};

// One weight-gradient launch: partial rows into slab, reduced into grad_w[C][9].  The layer's input is x, or act(x*pscale + pshift).
struct DwWgradCall {
  int dtype = DC_F32, stride = 1, dil = 1, N = 0, C = 0, Hi = 0, Wi = 0;
  const void* x = nullptr; int ldx = 0; const void* dy = nullptr; int lddy = 0;
  float* slab = nullptr; float* grad_w = nullptr;
  const float* pscale = nullptr; const float* pshift = nullptr; int prelu = 0;
  hipStream_t st = nullptr;
};

// Which kernel family serves a shape in a direction under the current options, and how many slab rows the riders of its data gradient write
// (BatchNorm sums, weight-gradient rows; 0: no riders).  The C ABI's queries, from which the engine sizes its slabs, and the dispatchers read it.
enum DwFamily { DW_NONE, DW_REG, DW_WIN, DW_TILE, DW_TILE_S2, DW_PIPE };
enum DwDir { DW_FWD, DW_DGRAD, DW_WGRAD };
struct DwRoute { DwFamily family; int rows; };
DwRoute dw_route(DwDir dir, int dtype, int C, int stride, int dil, int N, int Hi, int Wi);

// M(T, DIL, FLIP) for the dtype, the dilation (1 or 2) and the direction of the stride-1 call c
#define DW_S1_CASES(c, M)                                                             \
  if ((c).dtype == DC_BF16) {                                                         \
    if ((c).dil == 1) { if ((c).flip) M(bf16, 1, true); else M(bf16, 1, false); }     \
    else              { if ((c).flip) M(bf16, 2, true); else M(bf16, 2, false); }     \
  } else {                                                                            \
    if ((c).dil == 1) { if ((c).flip) M(float, 1, true); else M(float, 1, false); }   \
    else              { if ((c).flip) M(float, 2, true); else M(float, 2, false); }   \
  }

constexpr int DWT_MAX_ROWS = 2048;   // most partial rows the weight-gradient slab may hold

int launch_dw_tile(const DwCall& c);
int dw_tile_rows(int dtype, int C, int N, int H, int W);   // pixel tiles of the stride-1 kernels = slab rows of the fused BN statistics
int launch_dw_tile_wgrad(const DwWgradCall& c);
size_t dw_tile_wgrad_workspace(int C, int N, int H, int W);
int dw_tile_reduce(const float* slab, float* grad_w, int rows, int C, hipStream_t st);   // grad[c][t] = sum of slab rows (fp64, fixed order)

// persistent pipelined kernel (dwpipe.hip): bf16, >= 64 channels, image extents multiples of 8.  dw_pipe_rows: workgroups per channel
// block = slab rows of the sums that ride along with the data gradient; 0 = shape not served (or switched off: option "dw_pipe")
int dw_pipe_rows(int dtype, int C, int dil, int N, int H, int W);
int launch_dw_pipe(const DwCall& c);
bool dw_pipe_forward();

// stride-2 kernels (dwtile_s2.hip): forward / data gradient by c.flip; the weight gradient's partial rows and their reduction
int launch_dw_tile_s2(const DwCall& c);
int launch_dw_tile_s2_wgrad(const DwWgradCall& c);
int dw_tile_s2_dgrad_rows(int dtype, int C, int N, int Hi, int Wi);

}  // namespace dc
