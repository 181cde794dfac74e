/* deepcam_hip.h -- C ABI of libdeepcam_hip.so: the MI355X (gfx950) kernels of the DeepCAM train step.
 *
 * The reference (azrael417/mlperf-deepcam) has no native code and no FFI: its hot path is the chain of
 * PyTorch/cuDNN/apex operator calls made by src/deepCam/train_hdf5_ddp.py:345-371.  Each entry point below
 * replaces one such operator call site (cited per function, paths relative to src/deepCam/), with plain
 * pointers and sizes only.  The Python host (mlperf-deepcam_amd/) binds them with ctypes; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless a parameter says "host".  `stream` is a hipStream_t.
 *   - Activations are channels-last: element (n,h,w,c) of a view lives at ptr[((n*H+h)*W+w)*ld + c];
 *     `ld` >= C lets a view be a channel slice of a wider buffer (this is how torch.cat disappears).
 *     ptr and ld*sizeof(elem) must be 16-byte aligned; C must be a multiple of 8 (true for every layer).
 *   - `dtype` selects the storage type of activations, activation gradients and packed GEMM weights:
 *     DC_BF16 (MFMA v_mfma_f32_16x16x32_bf16, fp32 accumulate) or DC_F32 (v_mfma_f32_16x16x4_f32, exact fp32).
 *     Master weights, gradients of weights, BN statistics, the loss and the optimizer state are always fp32.
 *   - Every function returns 0 on success.  On failure it returns non-zero and dc_last_error() describes it
 *     (bad shape/alignment => nothing was launched).  No function synchronises, allocates or frees.
 */
#ifndef DEEPCAM_HIP_H_
#define DEEPCAM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { DC_F32 = 0, DC_BF16 = 1 };
enum { DC_ADAM = 0, DC_ADAMW = 1, DC_LAMB = 2 };

const char* dc_last_error(void);
int dc_version(void);
/* Kernel switches (tests and A/B measurements inside one process): they force a kernel at shapes its planner would not give it, or keep
 * it off.  "igemm256": 0 = 128 x 128 tiles only, 1 = planner picks per layer (default), 2 = 256 x 256 eight-wave kernel wherever
 * eligible.  "pw384", "pw224", "pw192", "igemm256p", "wgrad384", "thin_tile", "head_*_fused", "dw_tile", "dw_pipe", "dw_res_masked", "bn_apply_rows"
 * and their like: see the table in README.md and the .hip files.  An unknown name is an error. */
int dc_set_option(const char* name, int value);
/* Every dc_set_option switch back to its default (the library's own table; also what a freshly loaded library holds). */
int dc_reset_options(void);

/* Launch record (tests): which kernel served each call.  Several kernel families stand behind one entry point, chosen on the host by
 * eligibility predicates, a cost model and the switches above; between dc_launch_log_begin and dc_launch_log_end every launch the CALLING
 * THREAD issues through this library notes the name of its family.  Host state only, thread-local, off by default; nothing changes on the
 * device.  A recorded launch list (dc_program_run) replays through the same entry points and is recorded like direct calls; replaying a
 * captured graph launches nothing from the library and leaves no names.
 *   dc_launch_log_begin  starts an empty record; an error while one is open on this thread.
 *   dc_launch_log_end    stops recording and writes the names in launch order, joined by '\n', into buf (NUL-terminated; no launches: "").
 *                        An error when no record is open, when cap is too small for the names, or when more launches were issued than the
 *                        fixed-size record holds (4096); the record is closed in every case.
 * The names, one per family and template variant the dispatcher distinguishes:
 *   dense forward / data gradient (dc_conv_fwd*, dc_conv_dgrad*):
 *     tiny_gemm                             at most 16 pixels of a pointwise layer
 *     thin_fwd, thin_tile                   the thin stem convolutions: gather form, LDS-tiled form
 *     igemm128_bf16, igemm128_f32           128 x 128 tiles; igemm128_bf16_zfill / igemm128_f32_zfill: one launch over phase (0, 0) that
 *     igemm128_f32out                       zero-fills the three empty phases; _f32out: bf16 operands, fp32 output
 *     igemm256, igemm256p                   256 x 256 tiles; the persistent form
 *     igemm256_splitk, igemm256_splitk_fold 256 x 256 tiles cut along K, and the kernel that sums the cuts
 *     pw384_256, pw384_128, pw384_256_k64   pointwise, 384 channels wide: 256- / 128-pixel tiles of 32-deep stages, 256-pixel tiles of 64-deep stages
 *     pw224_384, pw224_192, pw192           pointwise, 224-pixel tiles 384 / 192 channels wide; 128 x 192 tiles
 *   dense weight gradient (dc_conv_wgrad*):
 *     thin_wgrad                            the stem layers' one-pass kernel
 *     wgrad384_pw, wgrad384_3x3, wgrad384_convT   256 x 384 tiles: pointwise, 3 x 3 "same", ConvTranspose2d
 *     wgrad128_bf16, wgrad128_f32, wgrad128_bnin  the plain split kernels on 128 x 128 tiles; _bnin: operand transformed while staged
 *     wgrad_reduce, fold                    the sum over the splits of one layer; dc_fold_slabs
 *   depthwise (dc_dwconv_*), each as _fwd / _dgrad / _wgrad:
 *     dw_reg_*, dw_win_*                    register kernels: any stride and dilation; the stride-1 window (dw_reg_reduce sums their wgrad rows)
 *     dw_tile_*, dw_tile_s2_*               LDS-tiled kernels, stride 1 and stride 2 (dw_tile_reduce sums their wgrad rows)
 *     dwpipe_fwd, dwpipe_dgrad              the persistent pipelined kernel (its data gradient carries the weight-gradient rows)
 *     dwpipe_dgrad_masked                   ... its data gradient that stores dx masked by the stored input (dc_dwconv_dgrad_wgrad_bnres, relu = 2)
 *   head: head_fwd_fused | the GEMM's name then head_combine; head_dgrad_stream, head_dgrad_stream_wgrad (weight gradient riding along),
 *     head_dgrad_apply | the GEMM's name
 *   BatchNorm apply: bn_apply_rows, bn_apply
 *   event catalogue (dc_mask_components, dc_component_stats): cc_tile, cc_merge, cc_flatten (tile labelling in LDS, the unions across
 *     tile borders and the seam, root + 1 into every pixel), cc_stats (every launch of the statistics call)
 *   event matching (dc_component_overlap, dc_event_scores): cc_overlap (every launch of both calls)
 *   event intensities (dc_component_fields): cc_fields (the init and the pixel pass)
 *   event shapes and the shape filter (dc_component_shape, dc_event_select, dc_mask_select): cc_shape (every launch of the three calls)
 *   event tracks (dc_track_append, dc_track_link, dc_track_resolve): cc_tracks (every launch of the three calls)
 *   storm life cycles (dc_track_fields_append, dc_track_cycles): cc_track_fields (every launch of both calls)
 *   track verification (dc_track_match_append, dc_track_match_resolve): cc_track_match (every launch of both calls)
 *   frame renderer (dc_render_frames): render_paint (the outlines of both classes, one byte per source pixel and panel), render_gather
 *     (colour table, graticule and outlines into the RGB bytes)
 *   climatology (dc_climatology_accumulate, dc_climatology_maps): climatology_accumulate_vec (16-byte loads, four lanes per 16-channel
 *     pixel), climatology_accumulate_scalar (any channel selection, and none), climatology_maps
 *   storm composites (dc_composite_centers, dc_composite_accumulate): composite_centers, composite_accumulate_vec (16-byte loads, four
 *     lanes per 16-channel pixel), composite_accumulate_scalar (any channel selection)
 *   neighbourhood verification (dc_fss_score): fss_rows (the horizontal box sums of four indicator fields, one packed word per pixel),
 *     fss_cols (the vertical sliding sums, the squared terms and their reduction), fss_total (the two-word running totals)
 *   probabilistic verification (dc_prob_score): prob_zero (this call's outputs), then prob_hist_vec (16-byte loads, H * W a multiple of 4)
 *     or prob_hist (4-byte loads, any H * W): the joint histogram in LDS, the squared errors and the pixel counters; prob_total (the
 *     running totals)
 *   decision rule (dc_logits_decide, dc_hysteresis_select): decide_q_vec (16-byte loads and 32-bit stores, H * W a multiple of 4) or
 *     decide_q (4-byte loads, byte stores, any H * W): candidates, seeds and their counters; decide_mark (a seed flags its component's
 *     root), decide_select (the mask of the flagged components, the kept pixels and the events)
 *   view ensemble (dc_input_view_hwc, dc_ensemble_add, dc_ensemble_pool): view_normalize (the rolled, mirrored and normalised input);
 *     ensemble_add_vec (16-byte loads and stores: W and roll multiples of 4) or ensemble_add (4-byte accesses, any width and roll): one
 *     member into the state; ensemble_pool (the pooled logits, the vote counters and their running totals)
 *   train-time augmentation (dc_augment_view_hwc): augment_view (a batch normalised with every sample in a view of its own, the label map
 *     moved with it)
 *   distance-map verification (dc_distance_score): dist_vert (the row distances of four indicator fields, one packed word per pixel),
 *     dist_horz (the capped squared distance maps, the ring counters, the sums and the Baddeley term), dist_total (the running totals)
 *   displacement verification (dc_displacement_score): disp_pack (the four bit planes, the predicted pixels per row, the pixel counts),
 *     disp_corr (the overlap table and `kept`), disp_best (the best shift per frame and class), disp_total (the running totals)
 *   scale-separation verification (dc_scale_score): scale_sums (the block sums of levels 0 .. 6 per tile, the pixel counts), scale_coarse
 *     (levels 7 and 8 from the tiles' sums; launched only for L > 6), scale_total (the running totals)
 *   aux                                  every other launch site (one entry per checked site: packing, gathers, finalizes, reductions, ...) */
int dc_launch_log_begin(void);
int dc_launch_log_end(char* buf, size_t cap);

/* Streams for the host runtime.  The reference leaves stream management to PyTorch/apex (its DDP overlaps the all-reduce
 * on a side stream, train_hdf5_ddp.py:227,363); here the weight-gradient kernels run beside the backward chain on a stream
 * of the LOWEST priority (level < 0; 0 = default, > 0 = highest), created non-blocking.  The caller owns the stream. */
int dc_stream_create(int level, void** stream);
int dc_stream_destroy(void* stream);
int dc_stream_priority_range(int* least, int* greatest);
/* `to_stream` waits for everything enqueued on `from_stream` so far (the reference's loop relies on PyTorch's stream semantics for the
 * same order, train_hdf5_ddp.py:358-364: backward, all-reduce, optimizer). */
int dc_stream_fence(void* from_stream, void* to_stream);
int dc_memset_async(void* dst, int byte, size_t bytes, void* stream);
/* dst[0 .. bytes) = src[0 .. bytes), both in device memory, in stream order.  A word-argument call, so that the two copies that keep virtual
 * rank 0's BatchNorm running buffers across the micro-batches of one step (the buffers a checkpoint of rank 0 holds, train_hdf5_ddp.py:515-527)
 * are part of a recorded launch list. */
int dc_memcpy_async(void* dst, const void* src, size_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The launch list of a train step as a C object.  The reference's step is the Python loop body train_hdf5_ddp.py:345-371, a chain of
 * operator calls; here it is ~700 calls of THIS header per step.  A program records such a chain once (entry point name + argument
 * words in issue order, stream fences included) and dc_program_run issues it again from C, with no interpreter between two launches.
 *   words:  one 8-byte word per argument in declaration order -- ints / longs / size_t sign-extended, float as the bit pattern of the
 *           double of equal value, pointers as they are.  Pointers to HOST objects (dc_conv_desc, dc_fold_entry tables, pointer arrays)
 *           are recorded as addresses: the caller keeps those objects alive and unchanged while the program lives.
 *   slots:  NULL, or per argument -1 (use the word) or a slot index whose value dc_program_bind supplies before a run (a batch pointer).
 * Every int-returning entry point of this header except dc_program_* itself can be recorded.
 * ------------------------------------------------------------------------------------------------ */
int dc_program_create(void** program);
int dc_program_destroy(void* program);
int dc_program_append(void* program, const char* entry_point, int nargs, const long long* words, const int* slots);
int dc_program_bind(void* program, int slot, long long word);
int dc_program_len(void* program);
const char* dc_program_op_name(void* program, int index);
int dc_program_run(void* program, int* failed_op);   /* first failing call's code; *failed_op = its index or -1 */

/* ------------------------------------------------------------------------------------------------
 * Dense convolution family: nn.Conv2d (k=1 or 3, stride 1|2, dilation, zero padding) and
 * nn.ConvTranspose2d(k=3, stride=2, padding=1, output_padding=1), all lowered to one gather-form
 * implicit GEMM on MFMA.  Reference call sites: architecture/deeplab_xception.py:60,65 (pointwise),
 * :74 (skip), :149 (conv2), :291-292 (ASPP, atrous), :426,430,434 (1x1), :352-374 (decoder convs and
 * transposed convs).  Backward entry points replace what autograd dispatches at train_hdf5_ddp.py:363.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int dtype;      /* DC_F32 | DC_BF16 */
  int k;          /* 1 or 3 */
  int stride;     /* 1 or 2 */
  int pad;
  int dil;
  int transposed; /* 1: ConvTranspose2d k3 s2 p1 op1 (stride/pad/dil fields ignored) */
  int cin;
  int cout;
} dc_conv_desc;


/* Output extent of the forward op for an Hi x Wi input. */
int dc_conv_out_hw(const dc_conv_desc* d, int Hi, int Wi, int* Ho, int* Wo);

/* Pack the fp32 master weight (PyTorch layout: [cout][cin][k][k], or [cin][cout][k][k] when transposed)
 * into the two GEMM operand layouts, both in `dtype`:  wf[tap][cout][cin'] (forward) and
 * wb[tap][cin][cout'] (data gradient), where the K extent of a row (cin', cout') is rounded up to 64 elements (32 below 64
 * channels) so that every bf16 row starts on a 128-byte boundary: a 128-byte K piece of a row is then ONE L2 line for the
 * LDS-DMA loaders (728 -> 768; 64-byte boundaries -- 736 -- filled 18 % slower, profiles/r05_fill_bench_align.txt).
 * dc_conv_packed_elems gives the element counts to allocate (and thereby the strides: wf_elems / (taps * cout)).  Either
 * output may be NULL. */
int dc_conv_packed_elems(const dc_conv_desc* d, size_t* wf_elems, size_t* wb_elems);
int dc_conv_pack_weights(const dc_conv_desc* d, const float* master, void* wf, void* wb, void* stream);

/* All layers in one launch.  table_dev: device array of `nentries` records {const float* master; void* wf; void* wb; int cin, cout,
 * taps, kind;} (40 bytes, natural alignment); kind 0 = conv, 1 = transposed conv (both as dc_conv_pack_weights), 2 = depthwise
 * (as dc_dwconv_pack_weights: cout = C, wf = fp32 [9][C]).  Dense entries are packed in `dtype`. */
int dc_pack_all(int dtype, const void* table_dev, int nentries, void* stream);

/* Rows of the per-tile BatchNorm partial-statistics slab that dc_conv_fwd writes when stat_slab != NULL:
 * slab is float[2][rows][cout] (sum, sum of squares of the STORED outputs). */
int dc_conv_stat_rows(const dc_conv_desc* d, int N, int Hi, int Wi);

/* y = conv(x, w) [+ bias];  accumulate != 0 adds into the existing y instead of overwriting. */
int dc_conv_fwd(const dc_conv_desc* d, int N, int Hi, int Wi, const void* x, int ldx, const void* wf,
                const float* bias, void* y, int ldy, float* stat_slab, int accumulate, void* stream);

/* dc_conv_fwd / dc_conv_dgrad given BOTH packed images of the layer (replaces the same call sites: F.conv2d of the `pointwise` convs at
 * architecture/deeplab_xception.py:60,65 and their autograd data gradient).  `wb` here / `wf` below is the image the plain entry point does not
 * take; its rows are [k][n] for the GEMM in question, so a pointwise layer's weight stages can be 32-deep slabs of whole L2 lines
 * (csrc/igemm224.hip: 224 x 384 tiles, three-deep operand rings).  Layers that kernel does not serve run exactly as through the plain entry
 * points.  Outputs are bit-identical to the plain calls; the BatchNorm partial sums come in another summation order (one slab row per
 * 224-pixel tile; with slab_rows = 0 the slab keeps dc_conv_stat_rows rows, the other rows written as zeros). */
int dc_conv_fwd_kn(const dc_conv_desc* d, int N, int Hi, int Wi, const void* x, int ldx, const void* wf, const void* wb,
                   const float* bias, void* y, int ldy, float* stat_slab, int slab_rows, int accumulate, void* stream);
/* Rows of the slab dc_conv_fwd_kn writes when slab_rows carries this value: one per 224-pixel tile where igemm224.hip serves the layer
 * (fewer, and none of them zeros), dc_conv_stat_rows elsewhere.  slab_rows = 0: the dc_conv_stat_rows layout whatever kernel runs.  The call
 * fails if slab_rows is not what the launch writes (the planner's answer changed between the query and the call). */
int dc_conv_stat_rows_kn(const dc_conv_desc* d, int N, int Hi, int Wi);
/* 1 where dc_conv_fwd_kn takes slab_rows = -1 for this layer (the pointwise tile kernels igemm224.hip and igemm192.hip): stat_slab is then a SUM ROW -- double[2][Cout] (sum, sum of squares), zeroed by
 * the caller -- that every tile of the launch adds its channel sums to with fp64 atomics, instead of one fp32 row per tile.  (The addends
 * are the fp32 sums a row slab would hold; their fp64 sum is exact, hence independent of the arrival order and equal to what dc_bn_finalize
 * computes from the rows.)  dc_bn_finalize, dc_bn_apply_fin and dc_dwconv_fwd_fin take such a slab with rows = -1: two numbers per channel to
 * read, so the consumer of the coefficients runs the finalize itself at any tensor size and the finalize launch leaves the dependent chain
 * (nn.BatchNorm2d in training mode behind every pointwise conv of the middle flow, deeplab_xception.py:62-66,104-119). */
int dc_conv_sum_row_kn(const dc_conv_desc* d, int N, int Hi, int Wi);
int dc_conv_dgrad_kn(const dc_conv_desc* d, int N, int Hi, int Wi, const void* dy, int lddy, const void* wb, const void* wf,
                     void* dx, int lddx, int accumulate, void* stream);

/* Same as dc_conv_fwd, but the result is stored as fp32 (y: float NHWC, ldy in floats) whatever d->dtype is:
 * used where the consumer must not see bf16-rounded sums (the classifier head's logits). */
int dc_conv_fwd_f32out(const dc_conv_desc* d, int N, int Hi, int Wi, const void* x, int ldx, const void* wf,
                       float* y, int ldy, void* stream);

/* The ASPP head (deeplab_xception.py:282-302; aspp2..aspp4 called at :445-447) runs three 3x3 convolutions of dilation 6 / 12 / 18
 * (padding == dilation, stride 1) over ONE input.  This entry point computes `count` (<= 4) such convolutions in one launch:
 * member b uses dilation dils[b] (host array), packed weights wfs[b], output view ys[b] (all with ldy) and statistics slab
 * stat_slabs[b] (NULL array: no statistics).  d->dil / d->pad are ignored, d->k must be 3 and d->stride 1.  Results are
 * bit-identical to `count` dc_conv_fwd calls (which is what runs when the fused kernel does not serve the dtype). */
int dc_conv_fwd_dilated_group(const dc_conv_desc* d, int N, int Hi, int Wi, int count, const int* dils, const void* x, int ldx,
                              const void* const* wfs, void* const* ys, int ldy, float* const* stat_slabs, void* stream);
/* The same launch with a caller-owned workspace: where dc_conv_fwd_dilated_group_workspace(...) > 0 (the launch would leave more than half of
 * the chip idle under a long K loop -- local batch 2: 81 tiles of 576 K steps) and `ws` holds that many bytes, every tile's K loop is split over
 * several workgroups (fp32 partial tiles in ws) and a second kernel sums the splits in a fixed order, stores the outputs and takes the
 * BatchNorm sums: another order of the K sum than the unsplit launch (not its bits), deterministic.  SURVEY section 2.3 K3: "needs split-K
 * to fill 256 CUs".  ws NULL or too small: the unsplit launch. */
size_t dc_conv_fwd_dilated_group_workspace(const dc_conv_desc* d, int N, int Hi, int Wi, int count, const int* dils);
int dc_conv_fwd_dilated_group_ws(const dc_conv_desc* d, int N, int Hi, int Wi, int count, const int* dils, const void* x, int ldx,
                                 const void* const* wfs, void* const* ys, int ldy, float* const* stat_slabs, void* ws, size_t ws_bytes,
                                 void* stream);

/* dx = conv_backward_data(dy, w).  Hi, Wi are the FORWARD input extents (= extents of dx). */
int dc_conv_dgrad(const dc_conv_desc* d, int N, int Hi, int Wi, const void* dy, int lddy, const void* wb,
                  void* dx, int lddx, int accumulate, void* stream);
/* The same data gradient when dx is the gradient w.r.t. a BatchNorm(+ReLU) output act(bn(y)) that feeds only this conv
 * (deeplab_xception.py:361-374 and the other conv -> BatchNorm -> ReLU -> conv chains): the BatchNorm's backward sums (sum g,
 * sum g*xhat; g = the stored dx masked by y*mscale + mshift > 0 when relu) are taken in the epilogue into slab[2][rows][C],
 * rows = dc_conv_dgrad_bnstats_rows (0: this layer is not served), so dc_bn_bwd_reduce's pass over dx and y is not needed.
 * dx is written, never accumulated. */
int dc_conv_dgrad_bnstats_rows(const dc_conv_desc* d, int N, int Hi, int Wi);
int dc_conv_dgrad_bnstats(const dc_conv_desc* d, int N, int Hi, int Wi, const void* dy, int lddy, const void* wb, void* dx,
                          int lddx, const void* y, int ldy, const float* mean, const float* invstd, const float* mscale,
                          const float* mshift, int relu, float* slab, void* stream);

/* grad_w (fp32, PyTorch master layout) = conv_backward_weight(x, dy).  Split over the pixel axis into fp32
 * partial slabs in `workspace` (dc_conv_wgrad_workspace bytes), then reduced deterministically. */
size_t dc_conv_wgrad_workspace(const dc_conv_desc* d, int N, int Hi, int Wi);
int dc_conv_wgrad(const dc_conv_desc* d, int N, int Hi, int Wi, const void* x, int ldx, const void* dy,
                  int lddy, void* workspace, size_t workspace_bytes, float* grad_w, void* stream);

/* The same for `count` layers of ONE geometry in one launch (count <= 16 where the 256 x 384 kernel serves the layer -- pointwise layers,
 * stride-1 3 x 3 layers, transposed convolutions: csrc/wgrad384.hip --, <= 4 on the 256 x 256 kernel): xs / dys / grad_ws are host arrays of
 * `count` device pointers (same ldx / lddy).  Replaces the per-layer conv_backward_weight calls autograd makes for the pointwise
 * convs of the middle-flow Blocks (deeplab_xception.py:69-122, 211-226): the layers share the launch, so each is cut into fewer,
 * longer pixel splits.  Results are bit-identical run to run (fixed-order reduction); layers the grouped kernel does not serve
 * are computed by `count` plain dc_conv_wgrad calls. */
size_t dc_conv_wgrad_group_workspace(const dc_conv_desc* d, int N, int Hi, int Wi, int count);
int dc_conv_wgrad_group(const dc_conv_desc* d, int N, int Hi, int Wi, int count, const void* const* xs, int ldx,
                        const void* const* dys, int lddy, void* workspace, size_t workspace_bytes,
                        float* const* grad_ws, void* stream);

/* Slab-only form of the two calls above: the split-K partial sums of `count` layers of one geometry (count > 1: the grouped launch
 * must serve the layer, dc_conv_wgrad_plan fails otherwise) are left in slabs[l] ([splits][taps][Cout][Cin] floats each,
 * dc_conv_wgrad_plan's slab_bytes) and NOT reduced: dc_fold_slabs adds the slabs of many layers in one launch.  `splits` must be the
 * value dc_conv_wgrad_plan returned (the call fails if tuning options changed the plan in between).  Same reference call site:
 * autograd's conv_backward_weight at train_hdf5_ddp.py:363. */
int dc_conv_wgrad_plan(const dc_conv_desc* d, int N, int Hi, int Wi, int count, int* splits, size_t* slab_bytes);
int dc_conv_wgrad_partial(const dc_conv_desc* d, int N, int Hi, int Wi, int count, const void* const* xs, int ldx,
                          const void* const* dys, int lddy, float* const* slabs, int splits, void* stream);

/* grad (fp32, PyTorch master layout) = fixed-order sum of the partial slabs of n layers, ONE launch per 24 entries (host array; the
 * table travels in the kernel arguments).  kind DC_FOLD_CONV: slab [splits][taps][co][ci] -> grad [co][ci][taps] (Conv2d.weight);
 * DC_FOLD_CONVT: -> grad [ci][co][taps] (ConvTranspose2d.weight); DC_FOLD_DW: slab [splits = rows][9][co = C] -> grad [C][1][3][3]
 * (taps = 9, ci = 1; the rows dc_dwconv_dgrad_bnstats_wgrad / dc_dwconv_dgrad_wgrad leave).  Bit-identical to the per-layer
 * reductions inside dc_conv_wgrad / dc_dwconv_wgrad_reduce whatever the grouping.  Replaces the accumulation step of autograd's
 * conv_backward_weight for all layers of an Xception block at once (train_hdf5_ddp.py:363). */
enum { DC_FOLD_CONV = 0, DC_FOLD_CONVT = 1, DC_FOLD_DW = 2 };
typedef struct dc_fold_entry {
  const float* slab;
  float* grad;
  int kind, splits, taps, co, ci;
} dc_fold_entry;
int dc_fold_slabs(const dc_fold_entry* entries, int n, void* stream);

/* grad_bias[c] = sum over M rows of dy (the one biased conv, deeplab_xception.py:366). */
int dc_colsum(int dtype, long M, int C, const void* dy, int lddy, float* out, void* workspace, void* stream);
size_t dc_colsum_workspace(long M, int C);

/* ------------------------------------------------------------------------------------------------
 * Depthwise 3x3 ("SeparableConv2d_same.conv1" after fixed_padding): deeplab_xception.py:45-51,58-59,63-64.
 * Zero padding of `dil` on every side is implicit.  Forward and data-gradient take the weights repacked as
 * fp32 [9][C] (`wp`, from dc_dwconv_pack_weights); the weight gradient comes back in the master layout [C][1][3][3].
 * ------------------------------------------------------------------------------------------------ */
int dc_dwconv_pack_weights(int C, const float* master, float* packed, void* stream);
/* pscale/pshift (both or neither; fp32[C]) fuse the PRECEDING BatchNorm (+ReLU when prelu != 0) into the load: x is then the
 * raw conv output and every in-bounds element is read as act(x*pscale[c] + pshift[c]); padding stays zero. */
int dc_dwconv_fwd(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* x, int ldx,
                  const float* wp, void* y, int ldy, const float* pscale, const float* pshift, int prelu, void* stream);
/* dc_dwconv_fwd through a training-mode BatchNorm(+ReLU) whose dc_bn_finalize it runs itself (SeparableConv2d_same after bn + relu inside a
 * Block, deeplab_xception.py:83-98, at small batch): x is the raw output of the convolution in front of that BatchNorm, slab[2][rows][C]
 * its partial sums with rows <= dc_bn_bwd_apply_fin_max_rows().  Every workgroup sums the slab for its own channels while its halo tile
 * travels (order and bits of dc_bn_finalize); the workgroups of pixel tile 0 store scale / shift / save_mean / save_invstd and update
 * the running statistics.  The slab is read with 16-byte loads: 16-byte aligned (as are dc_bn_apply_fin's and dc_bn_bwd_apply_fin's).
 * dc_dwconv_fwd_fin_ok: 1 when the shape is served (stride 1, dilation 1 or 2, the tiled kernel). */
int dc_dwconv_fwd_fin_ok(int dtype, int C, int stride, int dil, int N, int Hi, int Wi);
int dc_dwconv_fwd_fin(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* x, int ldx, const float* w, void* y, int ldy,
                      int prelu, long count, const float* slab, int rows, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float* scale, float* shift,
                      float* save_mean, float* save_invstd, void* stream);
/* dx = dw_backward_data(dy) [+ addend]  (addend: same shape as dx, e.g. the residual branch's gradient) */
int dc_dwconv_dgrad(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                    const float* wp, const void* addend, int ldadd, void* dx, int lddx, void* stream);
/* Data gradient that also takes the backward statistics of the BatchNorm(+ReLU) whose (never materialised) output fed this
 * depthwise conv: dx as dc_dwconv_dgrad (no addend), and slab[2][rows][C] = per-tile partial sums of g and g*xhat with
 * g = dx masked by (ybn*mscale + mshift > 0) when relu, xhat = (ybn - save_mean)*save_invstd.  rows =
 * dc_dwconv_dgrad_bnstats_rows(...) (0: shape not served, use dc_dwconv_dgrad + dc_bn_bwd_reduce); finish with dc_bn_bwd_finalize.
 * Replaces one full read of dx and ybn per such BatchNorm (autograd of nn.BatchNorm2d after deeplab_xception.py:65). */
int dc_dwconv_dgrad_bnstats_rows(int dtype, int C, int stride, int dil, int N, int Hi, int Wi);
int dc_dwconv_dgrad_bnstats(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                            const float* wp, void* dx, int lddx, const void* ybn, int ldybn, const float* save_mean,
                            const float* save_invstd, const float* mscale, const float* mshift, int relu, float* slab, void* stream);
/* dc_dwconv_dgrad_bnstats that ALSO takes this depthwise layer's weight gradient (reference: SeparableConv2d_same.conv1,
 * deeplab_xception.py:54-66, whose .grad autograd fills at train_hdf5_ddp.py:363) from the same dy window: the layer's forward input
 * is the never-stored act(ybn*mscale + mshift), recomputed from the ybn the statistics read anyway.  wslab: dc_dwconv_dgrad_wgrad_rows
 * rows (0: shape not served -- stride 2, large images) of [9][C] floats; dc_dwconv_wgrad_reduce adds the rows into grad_w (master
 * layout [C][1][3][3]) in a fixed order and may run on another stream once the producing call has been ordered before it. */
int dc_dwconv_dgrad_wgrad_rows(int dtype, int C, int stride, int dil, int N, int Hi, int Wi);
int dc_dwconv_dgrad_bnstats_wgrad(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                  const float* w_packed, void* dx, int lddx, const void* ybn, int ldybn, const float* save_mean,
                                  const float* save_invstd, const float* mscale, const float* mshift, int relu, float* slab,
                                  float* wslab, void* stream);
/* The same when this layer is not the only reader of that BatchNorm's output: dx = conv^T(dy) + addend (what the other readers left; may alias
 * dx), the sums are those of the complete gradient -- the caller makes this layer the LAST writer (stride 1). */
int dc_dwconv_dgrad_bnstats_wgrad_add(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                      const float* w, const void* addend, int ldadd, void* dx, int lddx, const void* ybn, int ldybn,
                                      const float* save_mean, const float* save_invstd, const float* mscale, const float* mshift, int relu,
                                      float* slab, float* wslab, void* stream);
/* The same fusion where the layer's forward input is a stored tensor x, or act(x*pscale + pshift) of one: data gradient (written, or
 * added onto `addend`: the first separable conv of an Xception block, whose input gradient joins the shortcut's) plus weight-gradient
 * rows; no BatchNorm sums. */
int dc_dwconv_dgrad_wgrad(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                          const float* w_packed, const void* addend, int ldadd, void* dx, int lddx, const void* x, int ldx,
                          const float* pscale, const float* pshift, int prelu, float* wslab, void* stream);
/* dc_dwconv_dgrad_wgrad where the stored input x is itself relu(bn(ybn) + residual), the output of the previous Xception block
 * (deeplab_xception.py:99-122: `x += skip`, then the next block's in-place ReLU), and this data gradient is the LAST contribution to d(x):
 * that BatchNorm's backward sums (sum g, sum g*xhat; g = the stored dx masked by x > 0 when relu) are taken on the way out into
 * slab[2][rows][C], so dc_bn_bwd_reduce's pass over dx, ybn and x is not needed.  rows = dc_dwconv_dgrad_wgrad_bnres_rows (also the
 * rows of wslab; 0: not served -- use dc_dwconv_dgrad_wgrad and dc_bn_bwd_reduce).
 * relu = 2: the sums are masked as with relu = 1 AND dx is stored masked: dx = 0 wherever x > 0 is false (the bits of masking the rounded
 * value after the store).  The stored dx then is g itself: dc_bn_bwd_apply[_fin] takes it with relu = 0, without `out` and without `g_out`
 * (same dy, bit for bit, as relu = 1 with out = x on the unmasked dx), and the shortcut's gradient is that buffer -- two tensor passes fewer
 * per block end.  Served where dc_dwconv_dgrad_wgrad_bnres_masked says 1 (the shapes of _rows, while option "dw_res_masked" is on);
 * elsewhere relu = 2 is an error. */
int dc_dwconv_dgrad_wgrad_bnres_rows(int dtype, int C, int stride, int dil, int N, int Hi, int Wi);
int dc_dwconv_dgrad_wgrad_bnres_masked(int dtype, int C, int stride, int dil, int N, int Hi, int Wi);
int dc_dwconv_dgrad_wgrad_bnres(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                const float* w_packed, const void* addend, int ldadd, void* dx, int lddx, const void* x, int ldx,
                                float* wslab, const void* ybn, int ldybn, const float* save_mean, const float* save_invstd, int relu,
                                float* slab, void* stream);
/* The two data gradients above that take BatchNorm sums, with the sums added to a SUM ROW (see dc_conv_sum_row_kn): `slab` is double[2][C]
 * (sum g, sum g*xhat), zeroed by the caller; every workgroup of the persistent kernel adds its two sums per channel with fp64 atomics (exact,
 * hence the bits of the row slab's column sums in any arrival order).  dc_bn_bwd_finalize and dc_bn_bwd_apply_fin take the row with rows = -1,
 * so the BatchNorm-backward apply runs the finalize itself at any tensor size.  dc_dwconv_dgrad_sum_row_ok: 1 where both are served. */
int dc_dwconv_dgrad_sum_row_ok(int dtype, int C, int stride, int dil, int N, int Hi, int Wi);
int dc_dwconv_dgrad_bnstats_wgrad_sum(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                      const float* w_packed, void* dx, int lddx, const void* ybn, int ldybn, const float* save_mean,
                                      const float* save_invstd, const float* mscale, const float* mshift, int relu, float* slab,
                                      float* wslab, void* stream);
int dc_dwconv_dgrad_wgrad_bnres_sum(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* dy, int lddy,
                                    const float* w_packed, const void* addend, int ldadd, void* dx, int lddx, const void* x, int ldx,
                                    float* wslab, const void* ybn, int ldybn, const float* save_mean, const float* save_invstd, int relu,
                                    float* slab, void* stream);
int dc_dwconv_wgrad_reduce(int C, int rows, const float* wslab, float* grad_w, void* stream);
size_t dc_dwconv_wgrad_workspace(int C, int N, int Hi, int Wi, int stride);
int dc_dwconv_wgrad(int dtype, int C, int stride, int dil, int N, int Hi, int Wi, const void* x, int ldx,
                    const void* dy, int lddy, void* workspace, float* grad_w, const float* pscale, const float* pshift,
                    int prelu, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (train and eval) fused with ReLU and the residual add: deeplab_xception.py:86,92,97,
 * 146-147,150,180-186,293-302,353-371,427,431,435 and the `x += skip` at :120.
 * Statistics are fp32 per-tile partials combined in fp64.
 * ------------------------------------------------------------------------------------------------ */
int dc_bn_stat_rows(long M);
int dc_bn_stats(int dtype, long M, int C, const void* x, int ldx, float* slab, void* stream);
/* slab[2][rows][C] -> batch mean / biased var -> scale = gamma*rsqrt(var+eps), shift = beta - mean*scale;
 * running_mean/var (momentum, unbiased var) and num_batches_tracked (int64) are updated when non-NULL.
 * The slab is CONSUMED: above 1024 rows it is folded in two stages and the first stage leaves its fp64 results in the slab itself
 * (same for dc_bn_bwd_finalize). */
int dc_bn_finalize(int C, long count, float* slab, int rows, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                   float eps, float* scale, float* shift, float* save_mean, float* save_invstd, void* stream);
/* eval mode: scale/shift from the running statistics */
int dc_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, float* scale, float* shift, void* stream);
/* Every BatchNorm of a network in one launch (net.eval(), train_hdf5_ddp.py:425: the coefficients change only when the weights or the
 * running statistics do).  table_dev: device array of n records (56 bytes, natural alignment); per channel the arithmetic of
 * dc_bn_eval_coeffs with the caller's eps, so the coefficients are bit-equal to n calls of it. */
typedef struct dc_bn_eval_entry {
  const float* gamma;
  const float* beta;
  const float* running_mean;
  const float* running_var;
  float* scale;
  float* shift;
  int C;
  float eps;
} dc_bn_eval_entry;
int dc_bn_eval_coeffs_all(const dc_bn_eval_entry* table_dev, int n, void* stream);
/* out = act(y*scale + shift [+ residual]),  act = ReLU when relu != 0 */
int dc_bn_apply(int dtype, long M, int C, const void* y, int ldy, const float* scale, const float* shift,
                const void* residual, int ldr, int relu, void* out, int ldo, void* stream);
/* dc_bn_finalize + dc_bn_apply in one launch (nn.BatchNorm2d in training mode, deeplab_xception.py:104-119 block outputs at small batch):
 * for a SHORT slab, rows <= dc_bn_bwd_apply_fin_max_rows(), every block of the apply kernel sums the slab for its own channels -- the order
 * and the bits of dc_bn_finalize -- and block row 0 stores scale / shift / save_mean / save_invstd and updates the running statistics.
 * The slab is read, not consumed. */
int dc_bn_apply_fin(int dtype, long M, int C, long count, const void* y, int ldy, const float* slab, int rows, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                    float* scale, float* shift, float* save_mean, float* save_invstd, const void* residual, int ldr, int relu, void* out,
                    int ldo, void* stream);
/* backward, step 1: g = dout * (out > 0 if relu), partial sums of g and g*xhat -> slab[2][rows][C].
 * relu == 2: the activation was fused into its consumer and never stored; the mask is recomputed as
 * y*mscale[c] + mshift[c] > 0 (the forward scale/shift vectors), `out` is ignored. */
int dc_bn_bwd_reduce(int dtype, long M, int C, const void* dout, int lddo, const void* y, int ldy,
                     const void* out, int ldout, int relu, const float* save_mean, const float* save_invstd,
                     float* slab, const float* mscale, const float* mshift, void* stream);
/* dc_bn_bwd_reduce with the two sums added to a SUM ROW (see dc_conv_sum_row_kn): `slab` is double[2][C], zeroed by the caller; every block of the
 * pass adds its share with fp64 atomics (at most 2 048 per channel).  dc_bn_bwd_finalize / dc_bn_bwd_apply_fin take it with rows = -1: the
 * two-stage fold of a long slab and the finalize launch leave the chain. */
int dc_bn_bwd_reduce_sum(int dtype, long M, int C, const void* dout, int lddo, const void* y, int ldy,
                     const void* out, int ldout, int relu, const float* save_mean, const float* save_invstd,
                     float* slab, const float* mscale, const float* mshift, void* stream);
/* step 2: dgamma, dbeta (fp32, written to the gradient arena) */
int dc_bn_bwd_finalize(int C, float* slab, int rows, float* dgamma, float* dbeta, void* stream);
/* step 3: dy = gamma*invstd*(g - dbeta/count - xhat*dgamma/count);  g is also stored when g_out != NULL */
int dc_bn_bwd_apply(int dtype, long M, int C, long count, const void* dout, int lddo, const void* y, int ldy,
                    const void* out, int ldout, int relu, const float* gamma, const float* save_mean,
                    const float* save_invstd, const float* dgamma, const float* dbeta, void* dy, int lddy,
                    void* g_out, int ldg, const float* mscale, const float* mshift, void* stream);
/* dc_bn_bwd_finalize + dc_bn_bwd_apply in ONE launch for a short slab (rows <= dc_bn_bwd_apply_fin_max_rows(): the slabs the persistent
 * depthwise data-gradient kernels leave for the 728-channel layers have 42 rows): every block sums the slab rows of its own channels in
 * dc_bn_bwd_finalize's order (same bits), the first row of blocks stores dgamma / dbeta.  One kernel and one dependent kernel boundary less per
 * BatchNorm of the middle flow (autograd's batch_norm_backward at train_hdf5_ddp.py:363). */
int dc_bn_bwd_apply_fin_max_rows(void);
int dc_bn_bwd_apply_fin(int dtype, long M, int C, long count, const void* dout, int lddo, const void* y, int ldy,
                        const void* out, int ldout, int relu, const float* gamma, const float* save_mean,
                        const float* save_invstd, const float* slab, int rows, float* dgamma, float* dbeta, void* dy, int lddy,
                        void* g_out, int ldg, const float* mscale, const float* mshift, void* stream);

/* Backward of o = [relu](bn(y) [+ residual]) for a BatchNorm in EVAL mode (frozen statistics), in one pass: nn.BatchNorm2d after .eval(),
 * i.e. F.batch_norm(training=False) with running_mean / running_var, whose backward is the affine map of those statistics (torch's
 * batch_norm_backward with train=false; deeplab_xception.py BatchNorms, autograd through a trained model).  g = dout * mask (relu 0: no
 * mask, 1: out > 0, 2: y * mscale + mshift > 0 with the eval scale / shift of dc_bn_eval_coeffs; `out` is read for relu 1 only),
 * dx = g * gamma * rsqrt(running_var + eps), g is also stored when g_out != NULL (the residual's gradient), and the partial sums
 * (sum g, sum g * (y - running_mean) * rsqrt(running_var + eps)) go to slab[2][rows][C], rows = dc_bn_stat_rows(M), the layout
 * dc_bn_bwd_reduce leaves: dc_bn_bwd_finalize(C, slab, rows, dgamma, dbeta) completes the parameter gradients.  The running statistics
 * are read, never written. */
int dc_bn_bwd_frozen(int dtype, long M, int C, const void* dout, int lddo, const void* y, int ldy, const void* out, int ldout, int relu,
                     const float* gamma, const float* running_mean, const float* running_var, float eps, void* dx, int lddx,
                     void* g_out, int ldg, float* slab, const float* mscale, const float* mshift, void* stream);

/* SeparableConv2d_same.forward as ONE operator (deeplab_xception.py:62-66: depthwise 3x3 "same", then pointwise 1x1) for the entry flow's thin
 * layers: d [N,H,W,Cin] = depthwise(act(x)) -- act = the producer's BatchNorm(+ReLU), applied on load when pscale / pshift are given, as in
 * dc_dwconv_fwd, whose bits d has -- and y [N,H,W,Cout] = pointwise(d), with the BatchNorm partial sums of the stored y in slab
 * [2][slab_rows][Cout] (NULL: none): the kernel fills dc_sepconv_fwd_rows(...) rows, one per workgroup, and zeroes the caller's other rows.
 * Served (rows > 0): bf16, stride 1, dilation 1, Cout 128, Cin 64 / 128, H % 8 == 0, W % 16 (Cin 128) or 32 (Cin 64) == 0, at least 65 536
 * pixels -- block 1 of the entry flow, where both halves are HBM-bound and d would otherwise be read back by a second launch.  wdw: the packed
 * depthwise taps (dc_dwconv_pack_weights), wf: the packed pointwise forward operand (dc_conv_pack_weights). */
int dc_sepconv_fwd_rows(int dtype, int Cin, int Cout, int stride, int dil, int N, int H, int W);
int dc_sepconv_fwd(int dtype, int Cin, int Cout, int N, int H, int W, const void* x, int ldx, const float* pscale, const float* pshift,
                   int prelu, const float* wdw, void* d, int ldd, const void* wf, void* y, int ldy, float* slab, int slab_rows, void* stream);

/* dc_bn_bwd_apply of a BatchNorm + dc_conv_dgrad + the weight gradient of the pointwise (1x1, stride 1) conv in front of it in ONE pass over
 * (dout, y, x): dy = the BatchNorm's input gradient (relu 2: dout masked by y * mscale + mshift > 0; relu 0: no mask) is formed in registers,
 * rounded to bf16 as dc_bn_bwd_apply stores it, and feeds both products from LDS; it is never written.  dx [M][Cin] = dy . W (wb: the packed
 * data-gradient operand of dc_conv_pack_weights); wslab [rows][Cout][Cin] fp32 = one partial weight gradient per workgroup, rows =
 * dc_pw_bn_bwd_rows(...) (0: shape not served -- bf16, Cout 128 with Cin 64 / 128 or Cout 256 with Cin 128 / 256, at least 65 536 pixels: the entry flow's first two blocks, whose 226 - 453 MB
 * tensors make all three passes HBM-bound), summed by dc_fold_slabs (DC_FOLD_CONV, splits = rows, taps = 1).  dgamma / dbeta: the finished
 * parameter gradients (dc_bn_bwd_finalize).  wslab_rows: the rows the caller allocated wslab (and planned its fold) for; the call fails if that is
 * not what dc_pw_bn_bwd_rows returns for the shape now.  Replaces autograd's batch_norm_backward + conv2d backward of SeparableConv2d_same.pointwise
 * (deeplab_xception.py:62-66, 84-101; train_hdf5_ddp.py:363). */
int dc_pw_bn_bwd_rows(int dtype, int Cin, int Cout, long M);
int dc_pw_bn_bwd(int dtype, long M, int Cin, int Cout, long count, const void* dout, int lddo, const void* y, int ldy, int relu,
                 const float* gamma, const float* save_mean, const float* save_invstd, const float* dgamma, const float* dbeta,
                 const float* mscale, const float* mshift, const void* x, int ldx, const void* wb, void* dx, int lddx, float* wslab, int wslab_rows,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Entry stem: Conv2d(16->32, k3, s2, p1) reading the caller's NCHW fp32 batch directly
 * (deeplab_xception.py:145,197).  Output NHWC `dtype`.  Also writes the BN partial-statistics slab.
 * ------------------------------------------------------------------------------------------------ */
int dc_stem_stat_rows(int N, int H, int W);
int dc_stem_fwd(int dtype, int N, int Cin, int H, int W, const float* x_nchw, const float* w /*[32][Cin][3][3]*/,
                void* y, int ldy, float* stat_slab, void* stream);
size_t dc_stem_wgrad_workspace(int N, int Cin, int H, int W);
int dc_stem_wgrad(int dtype, int N, int Cin, int H, int W, const float* x_nchw, const void* dy, int lddy,
                  void* workspace, float* grad_w, void* stream);
/* data gradient of the stem conv (conv2d(x, w, stride 2, padding 1) w.r.t. x, torch's convolution_backward input gradient) for any
 * Cin <= 16: dy NHWC [N][Ho][Wo][32] `dtype` (leading dimension lddy), w the fp32 master weight [32][Cin][3][3], dx the caller's NCHW fp32
 * [N][Cin][H][W] (8-byte aligned), OVERWRITTEN.  A gather: every element of dx is written exactly once, no atomics (deterministic). */
int dc_stem_dgrad(int dtype, int N, int Cin, int H, int W, const void* dy, int lddy, const float* w, float* dx_nchw, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Classifier head: ConvTranspose2d(256->n_classes=3, k3, s2, p1, op1), deeplab_xception.py:374,382.
 * Reads NHWC `dtype`, writes the NCHW fp32 logits the reference API returns.  Runs as GEMMs on the MFMA kernels:
 * P[pixel][co,tap] = x . W (27 products per input pixel, fp32) followed by the sub-pixel tap combination.
 * ------------------------------------------------------------------------------------------------ */
size_t dc_head_workspace(int dtype, int N, int Cin, int Hi, int Wi);
int dc_head_fwd(int dtype, int N, int Cin, int Hi, int Wi, const void* x, int ldx,
                const float* w /*[Cin][3][3][3]*/, float* logits_nchw, void* workspace, void* stream);
/* dc_head_fwd with the loss pass of dc_wce_fused on the logits while they are in registers (reference: upsample.last_deconv,
 * deeplab_xception.py:374,382, followed by fp_loss, utils/losses.py:35-50, argmax train_hdf5_ddp.py:406 and the IoU counts of
 * utils/utils.py:32-60): same logits, loss, gradient, predictions and counts bit for bit as the two calls.  logits_nchw may be
 * null (bf16, Cin = 256: the fused kernel then never stores them); the loss arguments are dc_wce_fused's. */
int dc_head_fwd_loss(int dtype, int N, int Cin, int Hi, int Wi, const void* x, int ldx, const float* w, float* logits_nchw,
                     void* workspace, const void* labels, int label_dtype_bytes, const float* class_weights, float grad_scale,
                     double* loss_sum, float* dlogits, int64_t* pred, int64_t* counts, void* stream);
/* dx = d(loss)/dx and grad_w (master layout) from the NCHW fp32 logit gradient, in one call (they share the gathered
 * 27-tap gradient image).  workspace: dc_head_workspace bytes, 256-byte aligned. */
int dc_head_bwd(int dtype, int N, int Cin, int Hi, int Wi, const void* x, int ldx, const float* dlogits_nchw,
                const float* w, void* dx, int lddx, float* grad_w, void* workspace, void* stream);
/* dc_head_bwd when x = act(bn(bn_y)) (upsample.deconv3: ConvTranspose2d -> BatchNorm2d -> ReLU, deeplab_xception.py:371-373): the
 * data gradient also leaves that BatchNorm's backward sums in bn_slab[2][cdiv(N*Hi*Wi, 128)][Cin] (see dc_conv_dgrad_bnstats). */
int dc_head_bwd_bnstats(int dtype, int N, int Cin, int Hi, int Wi, const void* x, int ldx, const float* dlogits_nchw,
                        const float* w, void* dx, int lddx, float* grad_w, void* workspace, const void* bn_y, int bn_ldy,
                        const float* bn_mean, const float* bn_invstd, const float* bn_mscale, const float* bn_mshift,
                        int bn_relu, float* bn_slab, void* stream);

/* The head on a BatchNorm(+ReLU) output that is never stored (upsample.deconv3's BatchNorm2d + ReLU in front of last_deconv,
 * deeplab_xception.py:371-374): y is the raw output of the convolution in front of that BatchNorm, scale / shift its forward
 * coefficients (dc_bn_finalize / dc_bn_eval_coeffs); the head forms act(y * scale + shift) while loading (fp32 fma, rounded to bf16:
 * the bits dc_bn_apply would have stored), so dc_bn_apply + dc_head_fwd[_loss] and these calls give the same logits bit for bit.
 * bf16, Cin = 256 only (the fused head kernel). */
int dc_head_fwd_bnin(int dtype, int N, int Cin, int Hi, int Wi, const void* y, int ldy, const float* scale, const float* shift,
                     int relu, const float* w, float* logits_nchw, void* workspace, void* stream);
int dc_head_fwd_loss_bnin(int dtype, int N, int Cin, int Hi, int Wi, const void* y, int ldy, const float* scale, const float* shift,
                          int relu, const float* w, float* logits_nchw, void* workspace, const void* labels, int label_dtype_bytes,
                          const float* class_weights, float grad_scale, double* loss_sum, float* dlogits, int64_t* pred,
                          int64_t* counts, void* stream);
/* dc_head_fwd / dc_head_fwd_bnin with dc_wce_score's per-sample epilogue on the logits while they are in registers (the validation
 * forward, train_hdf5_ddp.py:452-460: net.eval() forward, fp_loss, compute_score): no gradient, no prediction store.  Only the first
 * n_valid samples are computed.  Same logits bit for bit as the siblings, so the same counts as dc_head_fwd[_bnin] + dc_wce_score.
 * logits_nchw may be null (bf16, Cin = 256: a workgroup of the fused kernel works on ONE sample, so its sums are that sample's);
 * every other configuration stores the logits and runs dc_wce_score on them. */
int dc_head_fwd_score(int dtype, int N, int n_valid, int Cin, int Hi, int Wi, const void* x, int ldx, const float* w,
                      float* logits_nchw, void* workspace, const void* labels, int label_dtype_bytes, const float* class_weights,
                      double* loss_sum /*[N]*/, int64_t* counts /*[N][9]*/, void* stream);
int dc_head_fwd_score_bnin(int dtype, int N, int n_valid, int Cin, int Hi, int Wi, const void* y, int ldy, const float* scale,
                           const float* shift, int relu, const float* w, float* logits_nchw, void* workspace, const void* labels,
                           int label_dtype_bytes, const float* class_weights, double* loss_sum, int64_t* counts, void* stream);
/* dc_head_fwd / dc_head_fwd_bnin for inference on unlabelled data (nn.Predictor, predict.py; reference: the net.eval() forward and
 * torch.max(outputs, 1)[1] of train_hdf5_ddp.py:452-458, on a batch that has no labels): the epilogue of dc_logits_predict on the logits
 * while they are in registers.  Only the first n_valid samples are computed; the bytes of the others stay as they were.
 *   mask          uint8 [N][2Hi][2Wi]   first-max class (strict >, classes ascending: dc_wce_fused's pred)
 *   conf          fp32  [N][2Hi][2Wi]   its softmax probability 1 / sum_k exp(l_k - max)                    (NULL to skip)
 *   class_counts  int64 [N][3]          [n][j] += pixels of sample n with class j; the caller zeroes         (NULL to skip)
 * Same logits bit for bit as the siblings, so the same outputs as dc_head_fwd[_bnin] + dc_logits_predict.  logits_nchw may be null
 * (bf16, Cin = 256: the fused kernel); every other configuration stores the logits and runs dc_logits_predict on them. */
int dc_head_fwd_predict(int dtype, int N, int n_valid, int Cin, int Hi, int Wi, const void* x, int ldx, const float* w,
                        float* logits_nchw, void* workspace, uint8_t* mask, float* conf, int64_t* class_counts, void* stream);
int dc_head_fwd_predict_bnin(int dtype, int N, int n_valid, int Cin, int Hi, int Wi, const void* y, int ldy, const float* scale,
                             const float* shift, int relu, const float* w, float* logits_nchw, void* workspace, uint8_t* mask,
                             float* conf, int64_t* class_counts, void* stream);
/* dc_head_bwd for that case: the weight gradient forms the head's input from y itself (register-staged 128-tile kernel); bn_slab != NULL
 * also leaves the BatchNorm's backward sums there as dc_head_bwd_bnstats does (bn_mean / bn_invstd then required).
 * parts: 3 = everything; 1 = the gathered gradient image + the data gradient (+ sums); 2 = the weight gradient alone, which reads the
 * image a parts = 1 call left in `workspace` -- the caller may issue it on another stream ordered behind that call (the engine's
 * weight-gradient stream), since nothing on the chain waits for grad_w. */
int dc_head_bwd_bnin(int dtype, int N, int Cin, int Hi, int Wi, const void* y, int ldy, const float* scale, const float* shift,
                     int relu, const float* dlogits_nchw, const float* w, void* dx, int lddx, float* grad_w, void* workspace,
                     const float* bn_mean, const float* bn_invstd, float* bn_slab, int parts, void* stream);
/* dx == NULL in dc_head_bwd_bnin (bf16, 256 channels, bn_slab given): the head's data gradient -- 906 MB at local batch 8, read once, by that
 * BatchNorm's backward -- is not stored; the sums are taken all the same.  After dc_bn_bwd_finalize(bn_slab) this second pass forms the
 * gradient again (one MFMA step from the gathered image still in `workspace`) and writes the BatchNorm INPUT's gradient
 * dy = gamma*invstd*(g - dbeta/count - xhat*dgamma/count), bit-equal to the stored-dx path + dc_bn_bwd_apply(relu = 2): the pair moves
 * 2.9 GB instead of 4.6 (deeplab_xception.py:371-374 backward). */
int dc_head_bwd_bnin_apply(int dtype, int N, int Cin, int Hi, int Wi, const void* y, int ldy, const float* scale, const float* shift,
                           int relu, const float* gamma, const float* bn_mean, const float* bn_invstd, const float* dgamma,
                           const float* dbeta, long count, void* dy, int lddy, void* workspace, void* stream);

/* NCHW fp32 (the layout train_hdf5_ddp.py:348 hands over) -> NHWC `dtype`: the one layout pass of the step. */
int dc_nchw_to_nhwc(int dtype, int N, int C, int H, int W, const float* x_nchw, void* out, int ldo, void* stream);

/* Input pipeline (data/cam_hdf5_dataset.py:96-102,122-129): the dataset files are HWC fp32, already channels-last.
 * out[p][j] = scale[j] * (x_hwc[p][channels[j]] - shift[j])  (channels == NULL: identity), written as NHWC `dtype`.
 * Replaces the reference's numpy transpose + normalise on the host; with it the step has no layout pass at all. */
int dc_input_normalize_hwc(int dtype, long npix, int Cfile, int C, const int* channels, const float* x_hwc,
                           const float* shift, const float* scale, void* out, int ldo, void* stream);

/* The same arithmetic written as the reference's NCHW fp32 batch [N][C][HW] (any C >= 1): for --channels subsets
 * (train_hdf5_ddp.py:561) whose count is not a multiple of the 16-byte vector, which run dc_stem_fwd on NCHW fp32 input. */
int dc_input_normalize_hwc_to_nchw(int N, long HW, int Cfile, int C, const int* channels, const float* x_hwc,
                                   const float* shift, const float* scale, float* out_nchw, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Loss and metric: utils/losses.py:28-52 (fp_loss == plain mean of weighted CE), torch.max(.,1)[1]
 * (train_hdf5_ddp.py:406,458) and utils/utils.py:32-60 (compute_score) in one pass over the logits.
 *   loss_sum   double[1]   += sum over pixels of w[y]*(lse - logit[y])          (caller zeroes, divides)
 *   dlogits    fp32 NCHW   = w[y]*(softmax - onehot)*grad_scale                 (NULL to skip)
 *   pred       int64 [B,H,W] first-max argmax                                   (NULL to skip)
 *   counts     int64[9]    += tp[3], fp[3], fn[3]                               (NULL to skip)
 * label_dtype_bytes: 1 (uint8), 4 (int32) or 8 (int64) labels.  A label outside [0,3) -- for which the reference's
 * nn.CrossEntropyLoss raises -- makes loss_sum and that pixel's dlogits NaN (nothing here synchronises, so nothing can raise).
 * ------------------------------------------------------------------------------------------------ */
int dc_wce_fused(int B, int H, int W, const float* logits_nchw, const void* labels, int label_dtype_bytes,
                 const float* class_weights /*device float[3]*/, float grad_scale, double* loss_sum,
                 float* dlogits, int64_t* pred, int64_t* counts, void* stream);
/* compute_score on existing prediction / label maps (int64), counts int64[9] += */
int dc_confusion_counts(long n, const int64_t* pred, const void* labels, int label_dtype_bytes, int64_t* counts,
                        void* stream);

/* The validation pass's metric (train_hdf5_ddp.py:423-512: batch-1 fp_loss and compute_score, then the mean over SAMPLES) on a batch:
 * dc_wce_fused's loss and count arithmetic statement for statement, without gradient and prediction store, accumulated PER SAMPLE.
 *   loss_sum   double[B]     [b] += sum over sample b's pixels of w[y]*(lse - logit[y])   (caller zeroes)
 *   counts     int64[B][9]   [b] += tp[3], fp[3], fn[3] of sample b                       (caller zeroes)
 * A workgroup belongs to one sample (blockIdx.y), so no partial sum mixes two.  Samples >= n_valid (the padding of a ragged last
 * batch) are not read and their entries not written.  A label outside [0,3) makes THAT sample's loss_sum NaN. */
int dc_wce_score(int B, int n_valid, int H, int W, const float* logits_nchw, const void* labels, int label_dtype_bytes,
                 const float* class_weights /*device float[3]*/, double* loss_sum, int64_t* counts, void* stream);
/* One launch, one thread, samples in order: for b < n_valid  loss = loss_sum[b] / HW,  iou = compute_score's value from counts[b]
 * (utils/utils.py:53-60: fp32 tp / (tp + fp + fn) per class, 1 where the union is 0, mean of the three), then
 * acc[0] += 1, acc[1] += loss, acc[2] += iou  (the three running sums of train_hdf5_ddp.py:470-480; the result does not depend on
 * scheduling).  per_sample (double[B][2], may be NULL) receives (loss, iou) of every valid sample. */
int dc_val_accumulate(int B, int n_valid, long HW, const double* loss_sum, const int64_t* counts, double* acc /*[3]*/,
                      double* per_sample, void* stream);

/* Inference on stored logits (nn.predict_from_logits; the fp32 engine of nn.Predictor; reference: torch.max(outputs, 1)[1],
 * train_hdf5_ddp.py:458): mask / conf / class_counts of dc_head_fwd_predict from fp32 NCHW logits [B][3][H][W], statement for statement
 * the fused kernel's arithmetic.  A workgroup belongs to one sample; samples >= n_valid are neither read nor written. */
int dc_logits_predict(int B, int n_valid, int H, int W, const float* logits_nchw, uint8_t* mask, float* conf /*may be NULL*/,
                      int64_t* class_counts /*[B][3], may be NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Event catalogue (nn.EventCatalog; predict.py --events): connected components of a class mask and one row of statistics per component.
 * Nothing like it exists in the reference, which stops at the mask; its visualiser rolls the fields by W / 2 because they are global
 * longitude bands, hence `wrap`.  Everything is integer arithmetic: equal inputs give equal bits whatever the scheduling.
 *   mask    uint8 [B][H][W]   classes 1 and 2 are foreground; 0 and every value >= 3 are background
 *   A component is a maximal set of pixels of ONE class connected under `connectivity` 4 or 8.  Rows are never periodic; with wrap = 1 the
 *   columns are (column W-1 touches column 0, under 8-connectivity diagonally too).
 *   labels  int32 [B][H][W]   0 for background, else 1 + the smallest r * W + c of the pixel's component (its root)
 *   table   int64 [B][cap][10], zeroed by the call; row k of a sample is the component with the k-th smallest root:
 *           root, class, pixels, sum wy[r], sum r, sum cx[c], sum sx[c], smallest row, largest row, seam (1: pixels in column 0 AND in column W-1)
 *   ncomp   int32 [B][3]      components: all, class 1, class 2 -- not capped: with all > cap the table holds the first cap rows by root
 *   wy [H], cx [W], sx [W]    int32 weights of a row / a column (nn.event_weight_tables: 2^20-scaled cos(lat), cos(lon), sin(lon))
 * Samples from n_valid on are not read and their slices of labels and ncomp not written (the whole table is zeroed).
 * dc_mask_components_tile: the tile of the labelling kernel (tests derive their shapes from it); dc_mask_components_workspace: bytes of
 * the workspace both calls take (256-byte aligned; dc_component_stats keeps ranks and prefix counts there); both are host functions.
 * connectivity 4 or 8, 0 < n_valid <= B, H * W < 2^31 - 1, cap >= 1.  Neither call synchronises; dc_component_stats reads the labels
 * dc_mask_components left on the same stream. */
int dc_mask_components_tile(int* th, int* tw);
size_t dc_mask_components_workspace(int B, int H, int W);
int dc_mask_components(int B, int n_valid, int H, int W, const uint8_t* mask, int connectivity, int wrap, int32_t* labels,
                       void* workspace, void* stream);
int dc_component_stats(int B, int n_valid, int H, int W, const uint8_t* mask, const int32_t* labels, const int32_t* wy,
                       const int32_t* cx, const int32_t* sx, int cap, int64_t* table, int32_t* ncomp, void* workspace, void* stream);

/* Overlap of two catalogues of the same frames (nn.EventMatcher; predict.py --verify): which component of catalogue a shares pixels with
 * which of catalogue b, and how much of each component the other mask covers.  a and b are any two catalogues of equal B, H, W -- a
 * prediction and its labels, or two consecutive time steps; nothing below depends on which is which.  Integer arithmetic throughout.
 *   mask_x    uint8 [B][H][W]   as above      labels_x  int32 [B][H][W]  as dc_mask_components leaves them
 *   rank_x    int32 [B][H][W]   the rank map of dc_component_stats: the first B * H * W words of ITS workspace; at a root pixel the row
 *                               index of that component, undefined elsewhere (only root pixels are read)
 *   pairs     int64 [B][pair_cap][3], zeroed by the call for all B samples: one row (rank a, rank b, shared pixels) per distinct pair of
 *             components with at least one pixel in common, whatever their classes.  Pairs with rank a >= cap_a or rank b >= cap_b are
 *             not listed.  The order of the rows is unspecified (sort on the host); rows from the stored count on are zero.
 *   npairs    int32 [B][2]: rows stored, overflow flag.  With at most pair_cap listable pairs all are stored and the flag is 0, whatever
 *             the scheduling (a pair is given up only after the whole table was probed).  Otherwise the flag is 1, pair_cap rows are
 *             stored (which ones is unspecified), and each of them is a distinct true pair with its full count.  Samples >= n_valid: not written.
 *   cover_a   int64 [B][cap_a], cover_b int64 [B][cap_b], zeroed by the call for all B samples: per component of rank < cap the number
 *             of its pixels at which the OTHER mask has the same class.  Accumulated by the pixel pass itself: exact also when the pair
 *             table overflows, and it counts the other side's components of any rank.
 *   workspace dc_component_overlap_workspace(B, pair_cap) bytes (a host function; 0 for arguments out of range), 256-byte aligned: the
 *             open-addressing pair table, int64 [B][slots][2] with slots = the power of two >= max(16, 2 * pair_cap), a counter of
 *             opened slots per sample and int32 [B][pair_cap] slot indices; the call clears what it needs cleared.
 * 0 < n_valid <= B, cap_a, cap_b >= 1, 1 <= pair_cap <= 2^24.  Samples from n_valid on are not read.  Does not synchronise; reads what
 * dc_mask_components and dc_component_stats left for BOTH catalogues on the same stream.
 * dc_component_overlap_lds_slots: the slots of the per-workgroup pair table in LDS (tests build a tile with more distinct pairs than that
 * from it, so that the runs which find no slot there and go to the global table directly stay exercised if the table grows). */
int dc_component_overlap_lds_slots(int* slots);
size_t dc_component_overlap_workspace(int B, int pair_cap);
int dc_component_overlap(int B, int n_valid, int H, int W, const uint8_t* mask_a, const int32_t* labels_a, const int32_t* rank_a, int cap_a,
                         const uint8_t* mask_b, const int32_t* labels_b, const int32_t* rank_b, int cap_b, int pair_cap, int64_t* pairs,
                         int32_t* npairs, int64_t* cover_a, int64_t* cover_b, void* workspace, void* stream);
/* Event scores from two tables and their coverage.  A component of class k in {1, 2} is SCORED when its pixels >= max(min_pixels, 1) and
 * its rank < cap (it has a row); a scored component is MATCHED when cover >= 1 and cover * 1024 >= cover_q * pixels (1 <= cover_q <= 1024).
 *   table_x, ncomp_x  as dc_component_stats leaves them; cover_x, npairs as dc_component_overlap leaves them
 *   scores  int64 [B][2][4], per class 1, 2: hits (matched in b), misses (unmatched in b), false alarms (unmatched in a), matched
 *           detections (matched in a).  Samples >= n_valid: not written.
 *   acc     int64 [10], NOT zeroed by the call: += the 8 sums over the valid samples, acc[8] += n_valid, acc[9] += the number of valid
 *           samples with more components than a cap or with the pair overflow flag set (non-zero: something was truncated).
 * Does not synchronise; the result does not depend on scheduling. */
int dc_event_scores(int B, int n_valid, int cap_a, const int64_t* table_a, const int32_t* ncomp_a, const int64_t* cover_a, int cap_b,
                    const int64_t* table_b, const int32_t* ncomp_b, const int64_t* cover_b, const int32_t* npairs, long min_pixels,
                    int cover_q, int64_t* scores, int64_t* acc, void* stream);

/* Per-event statistics of the input fields (nn.EventFields; predict.py --event_fields): for every event of a catalogue and every channel
 * of the raw fields the minimum and its pixel, the maximum and its pixel, a plain sum and an area-weighted sum -- a cyclone's pressure
 * minimum and where it sits, its maximum wind, a river's mean water vapour.  One pass over the label map; field values are loaded at
 * foreground pixels only.  Every result is exact and independent of the order in which pixels arrive (minimum, maximum, integer sums).
 *   labels      int32 [B][H][W]       as dc_mask_components leaves them
 *   rank_map    int32 [B][H][W]       the rank map of dc_component_stats (the first B * H * W words of its workspace), cap its row capacity
 *   fields      fp32 [B][H][W][ldc]   channel-last, physical units; channels 0 .. C-1 are used, 1 <= C <= 32, ldc >= C.  16-byte loads
 *                                     when ldc % 4 == 0 and the base is 16-byte aligned, scalar loads otherwise
 *   scale_bits  int32 [C], device     the sums' binary scale per channel (nn.event_field_bits: 39 - exponent of the recorded range)
 *   wy          int32 [H]             the catalogue's cos(lat) * 2^20 table
 *   ftable      int64 [B][cap][C][6]  16-byte aligned; row (k, ch) belongs to the event of rank k (row k of dc_component_stats):
 *                                     min, max, sum, wsum, nonfinite, saturated
 * For every foreground pixel p = r * W + c (labels[p] > 0) with k = rank_map[labels[p] - 1] in [0, cap) and every channel ch, v =
 * fields[b][r][c][ch]:
 *   v is NaN or +-Inf:  nonfinite += 1, nothing else.  Otherwise, with key(v) = bits ^ 0xFFFFFFFF if the sign bit is set, else
 *   bits | 0x80000000 (an order-preserving 32-bit key: -0.0 < +0.0, denormals in their places):
 *   min  = the unsigned 64-bit minimum of (key(v) << 32) | p                   (empty: all ones, -1 as int64)
 *   max  = the unsigned 64-bit maximum of (key(v) << 32) | (0xFFFFFFFF - p)    (empty: 0)
 *          both name the SMALLEST pixel index among equal values
 *   q = rint(ldexp((double)v, scale_bits[ch])), ties to even.  |q| > 2^40: saturated += 1 and v takes no part in either sum (it does in
 *   min and max).  Otherwise  sum += (int64)q  and  wsum += (int64)rint(ldexp((double)v, scale_bits[ch]) * ((double)wy[r] * 2^-20))
 *   (two exact factors, one rounded fp64 product, rint).  A sum of n values is within n * 2^-(scale_bits + 1) of the real one.
 * H * W <= 2^22 (the pixel shares a word with the key, and 2^40 * H * W stays inside int64).  Rows of valid samples without an event
 * (from min(ncomp, cap) on) hold the empty row (-1, 0, 0, 0, 0, 0); samples from n_valid on are neither read nor written.  Does not
 * synchronise; reads what dc_mask_components and dc_component_stats left on the same stream.
 * dc_component_fields_lds_slots: the roots the per-workgroup table in LDS holds (tests build a tile with more roots than that, so that
 * the runs which go to the global rows directly stay exercised if the table grows). */
int dc_component_fields_lds_slots(int* slots);
int dc_component_fields(int B, int n_valid, int H, int W, const int32_t* labels, const int32_t* rank_map, int cap, const float* fields,
                        int C, int ldc, const int32_t* scale_bits, const int32_t* wy, int64_t* ftable, void* stream);

/* Event shapes (nn.EventShape; predict.py --event_shape): one row of geometry per event of a catalogue -- what tells a long narrow
 * atmospheric river from a compact cyclone -- from exact integer sums in one pass over the label map.
 *   labels, rank_map, cap   as dc_component_fields takes them; wrap: the catalogue's flag
 *   row_tables  int32 [6][H]: wy, rc2, rcs, rc3, rc2s, rcs2     col_tables  int32 [5][W]: cx, sx, cxx, cxy, cyy
 *               (nn.event_shape_tables.  With cl = cos lat, sl = sin lat at the latitudes of nn.event_weight_tables and co = cos lon,
 *               so = sin lon at lon_c = -180 + 360 c / W degrees, each 2^20-scaled and rounded as wy is:  wy = cl, rc2 = cl^2,
 *               rcs = cl sl, rc3 = cl^3, rc2s = cl^2 sl, rcs2 = cl sl^2;  cx = co, sx = so, cxx = co^2, cxy = co so, cyy = so^2.
 *               The columns are a PERIODIC grid, column W-1 one step west of column 0 as `wrap` has it, so a shape rolled across the
 *               seam keeps its moments; the catalogue's own cx / sx, at linspace(-180, 180, W), hold the seam meridian twice.)
 *   shape       int64 [B][cap][12], zeroed by the call for the samples below n_valid; row k belongs to the event of rank k (row k of
 *               dc_component_stats), events of rank >= cap have no row.  With "not of the same component" meaning: a different label
 *               word (background or another event), or off the grid -- rows are never periodic; columns are with wrap = 1 (column W-1 is
 *               column 0's left neighbour), otherwise off the grid too.  Only the four edge neighbours make faces, under 8-connectivity too.
 *     0      boundary pixels: pixels of the event with at least one 4-neighbour that is not of the same component
 *     1      exposed vertical faces: (pixel, left-or-right neighbour) pairs whose neighbour is not of the same component
 *     2      exposed horizontal faces, weighted: sum of wy[r] over (pixel, upper-or-lower neighbour) pairs whose neighbour is not of the
 *            same component
 *     3-5    S_x = sum rc2[r] cx[c],  S_y = sum rc2[r] sx[c],  S_z = sum rcs[r] 2^20
 *     6-11   S_xx = sum rc3[r] cxx[c],  S_xy = sum rc3[r] cxy[c],  S_yy = sum rc3[r] cyy[c],  S_xz = sum rc2s[r] cx[c],
 *            S_yz = sum rc2s[r] sx[c],  S_zz = sum rcs2[r] 2^20
 *   A pixel is the unit vector u = (cl co, cl so, sl) with weight cl: fields 3-11 are the 2^40-scaled first and second moments
 *   sum w u and sum w u u^T on the sphere; the 2^40-scaled zeroth moment is field 3 of the catalogue's row times 2^20.  Nothing depends on
 *   a column anchor, so an event across the seam is no special case.  Every per-pixel term is below 2^40 in magnitude and H * W <= 2^22
 *   (refused otherwise): every sum fits an int64, is exact and independent of the order of arrival.
 *   The decode (nn.EventShape.decode; dc_event_select evaluates lambda+- in fp64): with S0 the zeroth moment, m = S1 / S0,
 *   C = S2 / S0 - m m^T, c = m / |m| ((1, 0, 0) when |m| = 0), lat = asin c_z, lon = atan2(c_y, c_x), e = (-sin lon, cos lon, 0),
 *   n = (-sin lat cos lon, -sin lat sin lon, cos lat), a = e^T C e, b = e^T C n, d = n^T C n,
 *   lambda+- = (a + d) / 2 +- sqrt(((a - d) / 2)^2 + b^2), clamped at 0.  sqrt(12 lambda+-) are the sides of the uniform strip with these
 *   second moments in chord space; nn.EventShape turns 12 lambda+ into the angle of the great-circle arc with that moment
 *   (6 (1 - sin t / t) = 12 lambda+), and nn.EventFilter.length_units a length in km into min_len2 the same way.
 * Samples from n_valid on are neither read nor written.  Does not synchronise; reads what dc_mask_components and dc_component_stats left
 * on the same stream.
 *
 * The filter (nn.EventFilter; predict.py --event_filter).  dc_event_select, one thread per event row:
 *   table, ncomp  as dc_component_stats leaves them; shape as dc_component_shape leaves it
 *   criteria  device, 8-byte aligned: two rows, class 1 then class 2, each { int64 min_pixels, int64 min_area (units of the catalogue's
 *             field 3), double min_len2, double min_aspect2 }
 *   An event of class k in {1, 2} with a row (rank < min(ncomp all, cap)) is KEPT iff  pixels >= min_pixels[k]  and  area >= min_area[k]
 *   and  12 lambda+ >= min_len2[k]  and  lambda+ >= min_aspect2[k] lambda-.  A criterion of 0 is off; an event whose zeroth moment is 0
 *   fails every active shape criterion (the last two).
 *   keep    uint8 [B][cap]: 1 for a kept event, 0 for a dropped one and for rows without an event
 *   counts  int64 [B][8], zeroed by the call for the samples below n_valid: per class (1, then 2) events kept, events dropped, pixels
 *           kept, pixels dropped; this call fills the events, dc_mask_select adds the pixels
 * dc_mask_select, one streaming pass: out_mask[p] = mask[p] where mask[p] is background or >= 3; for a pixel of class 1 or 2 its class
 * iff its event is kept or has no row (rank >= cap: no criterion was evaluated, ncomp tells the caller), 0 otherwise.  out_mask may not
 * alias mask.  Samples from n_valid on are neither read nor written, in either call; neither synchronises. */
int dc_component_shape(int B, int n_valid, int H, int W, const int32_t* labels, const int32_t* rank_map, int cap, int wrap,
                       const int32_t* row_tables, const int32_t* col_tables, int64_t* shape, void* stream);
int dc_event_select(int B, int n_valid, int cap, const int64_t* table, const int32_t* ncomp, const int64_t* shape, const void* criteria,
                    uint8_t* keep, int64_t* counts, void* stream);
int dc_mask_select(int B, int n_valid, int H, int W, const uint8_t* mask, const int32_t* labels, const int32_t* rank_map, int cap,
                   const uint8_t* keep, uint8_t* out_mask, int64_t* counts, void* stream);

/* Event tracks (nn.EventTracker; predict.py --tracks): the events of a TIME SERIES of frames linked into tracks on the device -- how long
 * a cyclone or a river lived, where it went, when it peaked.  The catalogue above treats a frame in isolation; here the state lives in
 * device memory from one call to the next, and only small tables ever cross the bus.  Everything is integer arithmetic: equal inputs give
 * equal bits whatever the scheduling and however the frames were cut into batches.
 *   Frames are numbered 0, 1, 2, ... in the order they are given.  The EVENTS of a frame are the rows of its catalogue table, rank k <
 *   min(ncomp all, cap); the event number of (frame f, rank k) is the count of events in the frames before f, plus k.  Events with a
 *   number >= event_cap are counted, not stored, and take part in nothing.
 *   Two stored events of consecutive frames are LINKED when they have the same class, at least one pixel (r, c) belongs to both (the two
 *   masks hold that class there), and each has at least max(min_pixels, 1) pixels.  No dilation, no gap frames, never across classes.
 *   A TRACK is a connected component of the stored events under these links (merges and splits stay inside one track); its id is the
 *   smallest event number it holds, and track rows are ordered by id.
 *   state     int64 [4], device, kept across calls (zero it to start a series): events stored, frames seen, events not stored because
 *             the store was full, frames whose catalogue was truncated (ncomp all > cap)
 *   parent    int32 [event_cap]: the forest over event numbers, a root names itself.  Between calls every entry names an event of its own
 *             track with a number not larger than its own; dc_track_resolve leaves the smallest (the id) in every stored entry.
 *   store     int64 [event_cap][12]: frame, rank, then the ten columns of the event's catalogue row unchanged
 * dc_track_append numbers the events of a batch: frames j < n_valid of (table, ncomp) as dc_component_stats left them, frame j being frame
 * number frame0 + j (the caller counts frames; frame0 + n_valid < 2^31).
 *   first     int64 [B]: [j] = the event number of rank 0 of frame j, the prefix sum of min(ncomp all, cap) over the frames before it on
 *             top of state[0] + state[2], read on the device.  Entries from n_valid on are not written.
 *   For every new stored event e: parent[e] = e and store[e] is filled.  state is advanced.  1 <= cap <= 2^22.
 * dc_track_link unites the events of n frame pairs in one pass over both masks: pair j is frame j of side a (the EARLIER frame) against
 * frame j of side b, every array with the per-frame stride H * W (first_x: one entry per frame), so the pairs inside a batch are the
 * batch's own arrays as a and the same arrays advanced by one frame as b, n = n_valid - 1; one more call with n = 1 links a frame kept
 * from the call before.  mask_x, labels_x, rank_x as dc_component_overlap takes them; labels and ranks are read only where both masks
 * hold the same class 1 or 2.  The masks are loaded 4 bytes at a time where W % 4 == 0 and both bases are 4-byte aligned, bytewise
 * otherwise.  Events of rank >= cap, of number >= event_cap or (min_pixels > 1) of fewer than min_pixels pixels (store column 4) are
 * skipped.  n = 0 launches nothing.  0 <= n <= 65535, H * W < 2^31 - 1, event_cap * H * W * 2^20 < 2^63 (a track's area sum fits).
 * dc_track_resolve is called when tracks are read; it may be called at any point of a series and changes no later result.
 *   track_of  int32 [event_cap]: per stored event the row of its track, -1 where that row is >= track_cap; entries from state[0] on are
 *             not written
 *   tracks    int64 [track_cap][8], zeroed by the call: id, class, events, first frame, last frame, pixels (summed over the events),
 *             peak = the unsigned maximum over the events of (pixels << 32) | (0xFFFFFFFF - frame) (the largest event, the earliest frame
 *             among equals), area (the sum of the events' column `sum wy[r]`)
 *   ntracks   int64 [4]: tracks of any class, of class 1, of class 2 -- not capped --, rows stored = min(all, track_cap)
 *   workspace dc_track_workspace(event_cap) bytes (a host function; 0 for arguments out of range), 256-byte aligned; holds nothing
 *             between calls
 * 1 <= event_cap <= 2^30, 1 <= track_cap <= event_cap.  The grids are sized from event_cap; the kernels read the live count from state.
 * No call synchronises or reads anything on the host; all of them run on the caller's stream, in its order. */
size_t dc_track_workspace(int event_cap);
int dc_track_append(int B, int n_valid, int cap, const int64_t* table, const int32_t* ncomp, long frame0, int event_cap, int64_t* state,
                    int64_t* first, int32_t* parent, int64_t* store, void* stream);
int dc_track_link(int n, int H, int W, const uint8_t* mask_a, const int32_t* labels_a, const int32_t* rank_a, const int64_t* first_a,
                  const uint8_t* mask_b, const int32_t* labels_b, const int32_t* rank_b, const int64_t* first_b, int cap, int event_cap,
                  long min_pixels, const int64_t* store, int32_t* parent, void* stream);
int dc_track_resolve(int event_cap, int track_cap, const int64_t* state, int32_t* parent, const int64_t* store, int32_t* track_of,
                     int64_t* tracks, int64_t* ntracks, void* workspace, void* stream);

/* Storm life cycles (nn.TrackFields; predict.py --track_fields): the join of the two sections above on the device -- per track and frame
 * the field statistics of the track's events in that frame (a cyclone's centre and intensity per time step), per track the lifetime
 * extremes with the frame and pixel where they occurred.  Integer arithmetic and order-independent 64-bit atomics only: equal inputs
 * give equal bits whatever the scheduling and however the frames were cut into batches.
 *   Links join consecutive frames only (no gap frames; a cut links nothing), so the frames of a track form an INTERVAL: every frame from
 *   its first to its last holds at least one event of it.  A STEP is a (track, frame) pair of that interval; track row t has
 *   frames[t] = last - first + 1 steps, and step (t, f) is row offsets[t] + f - first[t] of the step tables.
 *   fstore    int64 [event_cap][C][6], 16-byte aligned, kept across calls next to the tracker's store: the field rows of event e, in the
 *             format of dc_component_fields (min, max, sum, wsum, nonfinite, saturated).  48 * C bytes per event slot: 403 MB at
 *             event_cap = 2^19 and C = 16.
 * dc_track_fields_append files a batch's field rows: row k < min(ncomp all, cap) of frame j < n_valid of ftable ([B][cap][C][6], as
 * dc_component_fields left it) is copied unchanged to event number e = first[j] + k, first as dc_track_append just wrote it for the same
 * batch; events with e >= event_cap are skipped.  It runs after dc_track_append and dc_component_fields on the same stream.  16-byte loads
 * and stores.  1 <= n_valid <= B, n_valid <= 65535, 1 <= cap <= 2^22.
 * dc_track_cycles is called when life cycles are read, after dc_track_resolve on the same stream; it reads what that call left (state,
 * store, track_of, tracks, ntracks) and fstore, and changes none of them.  It may be called at any point of a series.
 *   SELECTED  track row t < ntracks[3] with frames[t] >= max(min_frames, 1) and bit `class` of class_mask set (class_mask in [1, 6]:
 *             bit 1 is class 1, bit 2 is class 2).  need[t] = the sum of frames over the selected rows before t (the uncapped layout).
 *   STORED    a selected row with need[t] + frames[t] <= step_cap: it lies wholly inside the first step_cap rows of the uncapped layout.
 *             The stored rows are a prefix of the selected ones.  Events with track_of < 0 or of a track that is not stored take part in
 *             nothing.
 *   offsets   int64 [track_cap]: need[t] for stored rows, -1 for rows not selected, -2 for rows selected but not stored; entries from
 *             ntracks[3] on are not written
 *   ncycles   int64 [4]: tracks selected, step rows needed (not capped), step rows stored, tracks selected but not stored
 *   steps     int64 [step_cap][8], 16-byte aligned; the first ncycles[2] rows are written, the others untouched: track row, frame, the
 *             number of the track's events in that frame, and the sums over those events of the store columns pixels, area (sum wy[r]),
 *             sum_row, sum_cx, sum_sx -- so a step of two fragments has their joint centroid
 *   step_fields  int64 [step_cap][C][6], 16-byte aligned, the same rows: the events' field rows merged -- min = the unsigned 64-bit
 *             minimum of their min words, max = the unsigned maximum of their max words (both still name the smallest pixel among equal
 *             values, across fragments as within one event), sum, wsum, nonfinite, saturated = int64 sums (a step covers at most H * W
 *             pixels: the bound of dc_component_fields holds).  Empty: (-1, 0, 0, 0, 0, 0).
 *   track_fields  int64 [track_cap][C][4], 16-byte aligned; rows below ntracks[3] are written: the lifetime extremes of a stored track
 *             over its steps that have a finite value.  Words 0, 1: the lexicographic minimum of (key, frame, pixel) -- the value, the
 *             EARLIEST frame among equals, then the smallest pixel -- as (key << 32) | frame and the pixel; empty (-1, -1).  Words 2, 3:
 *             the largest key, then the earliest frame, then the smallest pixel, as (key << 32) | (0xFFFFFFFF - frame) and the pixel;
 *             empty (0, -1).  Rows of tracks that are not stored hold the empty values.  Lifetime SUMS are not kept: a long track can
 *             pass int64 in units of the per-pixel quantum; add the step sums on the host.
 *   workspace dc_track_cycles_workspace(event_cap, track_cap) bytes (a host function; 0 for arguments out of range), 256-byte aligned;
 *             holds nothing between calls
 * 1 <= C <= 32, 1 <= step_cap <= 2^31 - 1, min_frames >= 0, event_cap and track_cap as dc_track_resolve takes them, frames < 2^31 (the
 * tracker's limit) and H * W <= 2^22 (the limit of the field words).  The grids are sized from the capacities; the kernels read the live
 * counts (state[0], ntracks[3], ncycles[2]) on the device.  No call synchronises or reads anything on the host. */
size_t dc_track_cycles_workspace(int event_cap, int track_cap);
int dc_track_fields_append(int B, int n_valid, int cap, const int32_t* ncomp, const int64_t* first, const int64_t* ftable, int C,
                           int event_cap, int64_t* fstore, void* stream);
int dc_track_cycles(int event_cap, int track_cap, int step_cap, int C, int min_frames, int class_mask, const int64_t* state,
                    const int64_t* store, const int32_t* track_of, const int64_t* tracks, const int64_t* ntracks, const int64_t* fstore,
                    int64_t* offsets, int64_t* steps, int64_t* step_fields, int64_t* track_fields, int64_t* ncycles, void* workspace,
                    void* stream);

/* Track verification (nn.TrackMatcher; predict.py --verify_tracks): predicted against labelled storm tracks -- how many labelled storms
 * were found over most of their life, how many predicted ones exist nowhere in the labels, how early or late genesis and decay are.  The
 * join of three things the device already holds: the pair table of dc_component_overlap per frame, the event numbers of dc_track_append
 * and the track rows of dc_track_resolve.  Integer arithmetic; equal inputs give equal results however the frames are cut into batches.
 *   Side a and side b are the two catalogues of ONE overlap call (a: the prediction, b: the labels), each with a tracker of its own; both
 *   trackers are given the same frames in the same calls, so their frame numbers agree.
 *   An OVERLAP is a row (rank a, rank b, shared) of frame j's pair table whose two events are stored -- rank below min(ncomp all, cap) of
 *   its catalogue, event number first_x[j] + rank below event_cap_x -- and have the same class 1 or 2 (column 3 of the trackers' stores;
 *   the pair table lists pairs of any classes).  It is filed as a LINK (event number a, event number b, shared pixels).
 *   links     int64 [link_cap][3], kept across calls; the order of the rows is unspecified.  When the store is full, which links are
 *             dropped is unspecified; every stored row is a true overlap with its full count.
 *   state     int64 [4], device, kept across calls (zero it to start a series): links stored = min(all, link_cap), links not stored
 *             because the store was full, frames filed, frames whose pair table had its overflow flag set or whose catalogue (either
 *             side) was truncated
 * dc_track_match_append files a batch in ONE launch, behind dc_component_overlap and both dc_track_append calls of that batch on the same
 * stream: pairs / npairs ([B][pair_cap][3], [B][2]) as the overlap call left them, ncomp_x, first_x and store_x as the catalogues and the
 * trackers left them.  Samples from n_valid on are not read.
 * dc_track_match_resolve is called when results are read, after dc_track_resolve of BOTH trackers on the same stream; it reads what those
 * calls left (track_of_x, tracks_x, ntracks_x; store_a for the frame of a link), changes nothing an append depends on and may run at any
 * point of a series.  It zeroes what it fills.  A link belongs to the TRACK PAIR (row a, row b) = (track_of_a[event a],
 * track_of_b[event b]); links with a track_of of -1 on either side are counted and take part in nothing.
 *   tpairs    int64 [pair_cap][8], zeroed by the call: row a, row b, class, overlaps (links of the pair), common frames (DISTINCT frames
 *             with at least one link of the pair; merges and splits put several links of one pair into one frame), shared pixels (summed
 *             over the links), first common frame, last common frame.  The order of the rows is unspecified (sort on the host).
 *   cover_x   int64 [track_cap_x][2], zeroed by the call (rows without a track stay zero): matched frames = the DISTINCT frames of the
 *             track in which at least one of its events has a link to any track of the other side with a row; shared pixels = the sum
 *             over its links.  Accumulated by the link pass itself: exact also when the pair table overflows.
 *   A track is SCORED when it has a row, its class is 1 or 2 and frames = last - first + 1 >= max(min_frames, 1).  It is MATCHED when
 *   matched >= 1 and matched * 1024 >= cover_q * frames: the event rule of dc_event_scores with frames in place of pixels.  Coverage, not
 *   a pairwise overlap ratio, decides: a labelled storm predicted as two tracks with a missed frame in between is still found.
 *   scores    int64 [2][4], per class 1, 2: hits (scored b tracks that are matched), misses (... that are not), false alarms (scored a
 *             tracks that are not matched), matched detections (scored a tracks that are)
 *   counts    int64 [4]: track-pair rows stored, the pair overflow flag, links skipped for a missing track row, 0 (spare).  With at most
 *             pair_cap distinct track pairs all are stored and the flag is 0, whatever the scheduling (a pair is given up only after the
 *             whole table was probed).  Otherwise the flag is 1, pair_cap rows are stored (which ones is unspecified) and each of them
 *             is a distinct true pair with its full counts; state, cover_x, scores and counts[2] stay exact.  When links were dropped
 *             (state[1] > 0) the results are those of the stored links.
 *   workspace dc_track_match_workspace(...) bytes (a host function; 0 for arguments out of range), 256-byte aligned; holds nothing
 *             between calls: the pair table (the power of two >= max(16, 2 * pair_cap) slots of 48 bytes), the (pair, frame) table
 *             (the power of two >= max(16, 2 * link_cap) words: it cannot fill), one byte per (track, frame) step of each side (at most
 *             event_cap_x: the frames of a track form an interval, each holding an event of it), pair_cap ticket words and the step
 *             offsets (8 bytes per track row and side).  The call clears what it needs cleared.
 * Every result is independent of scheduling except the row order of links and tpairs.  1 <= link_cap <= 2^26, 1 <= pair_cap <= 2^24,
 * min_frames >= 0, 1 <= cover_q <= 1024, cap_x in [1, 2^22], event_cap_x and track_cap_x as dc_track_resolve takes them.  The grids are
 * sized from the capacities; the kernels read the live counts on the device.  No call synchronises or reads anything on the host.
 * Nothing is staged in LDS (there is no dc_track_match_lds_slots): the link pass works on the device tables directly. */
size_t dc_track_match_workspace(int event_cap_a, int event_cap_b, int track_cap_a, int track_cap_b, int link_cap, int pair_cap);
int dc_track_match_append(int B, int n_valid, int cap_a, int cap_b, int pair_cap, const int64_t* pairs, const int32_t* npairs,
                          const int32_t* ncomp_a, const int64_t* first_a, int event_cap_a, const int64_t* store_a, const int32_t* ncomp_b,
                          const int64_t* first_b, int event_cap_b, const int64_t* store_b, int link_cap, int64_t* links, int64_t* state,
                          void* stream);
int dc_track_match_resolve(int event_cap_a, int event_cap_b, int track_cap_a, int track_cap_b, int link_cap, int pair_cap, int min_frames,
                           int cover_q, const int64_t* state, const int64_t* links, const int64_t* store_a, const int32_t* track_of_a,
                           const int64_t* tracks_a, const int64_t* ntracks_a, const int32_t* track_of_b, const int64_t* tracks_b,
                           const int64_t* ntracks_b, int64_t* tpairs, int64_t* cover_a, int64_t* cover_b, int64_t* scores, int64_t* counts,
                           void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frame renderer (nn.FrameRenderer; predict.py --plots, train.py --plots): the picture the reference's visualiser draws on the host
 * (utils/visualizer.py, CamVisualizer.plot: the field of one channel through a colour table, the class-1 and class-2 regions of the
 * prediction outlined above the same field with the labels' regions outlined, rolled so that longitude 0 is in the middle, rows spaced
 * by the Gall stereographic projection, a graticule), made on the device as 8-bit RGB.  Only the colour index is floating point, two
 * separately rounded fp32 operations; everything after it is integer arithmetic: equal inputs give equal bytes.
 *   fields     fp32 [B][H][W][ldc]      channel-last, physical units; channel ch is drawn, 0 <= ch < ldc
 *   lo, scale  the drawn range: t = (v - lo) * scale, normally scale = 1 / (hi - lo) rounded to fp32
 *   lut        uint8 [nlut][3], device  the colour table (R, G, B), 1 <= nlut <= 256
 *   mask_a     [B][H][W] of 1-, 4- or 8-byte integers (a_bytes, as dc_wce_score takes labels): values 1 and 2 are the classes, every
 *              other value is background.  mask_b likewise (b_bytes); mask_b == NULL: one panel, P = 1, else P = 2 (a above b)
 *   src_row    int32 [Ho], device       the source row of every output row; ANY values, clamped to [0, H - 1]; need not be monotone
 *   shift      0 <= shift < W           output column x shows source column (x + shift) mod W
 *   row_line   uint8 [Ho], col_line uint8 [W], device: non-zero = a graticule line through that output row / column
 *   missing_rgb 0x00RRGGBB; line_argb, class1_argb, class2_argb 0xAARRGGBB (plain ints)
 *   width      1, 3, 5 or 7: the outlines' width in source pixels, R = (width - 1) / 2
 *   out        uint8 [B][P][Ho][W][3]
 *   workspace  dc_render_workspace(B, P, H, W) bytes, 256-byte aligned: one byte per source pixel and panel.  Every call overwrites
 *              all of it that it reads.
 * For every valid sample b, panel p and output pixel (y, x), with r = clamp(src_row[y]), c = (x + shift) mod W, m = the panel's mask:
 *   1. v = fields[b][r][c][ch].  NaN or +-Inf: the colour is missing_rgb.  Otherwise t = fl32(fl32(v - lo) * scale) (two roundings,
 *      nothing fused); i = 0 unless t > 0 (so also where t is NaN, which takes a non-finite lo or scale), i = nlut - 1 if t >= 1, else
 *      i = min(nlut - 1, (int)fl32(t * nlut)); the colour is lut[i].
 *   2. If row_line[y] or col_line[x] is non-zero, line_argb is blended over the colour.
 *   3. class1_argb is blended over it where (r, c) lies on the outline of class 1 of m, then class2_argb likewise for class 2.
 *   blend(fg, a): every channel becomes (fg * a + old * (255 - a) + 127) / 255 in integer arithmetic.
 *   An EDGE pixel of class k is a pixel of class k with at least one of its four neighbours not of class k; rows r +- 1 count only where
 *   they exist, columns are periodic (c +- 1 modulo W).  The OUTLINE of class k is every pixel (r, c) with an edge pixel of class k at
 *   (r + dy, (c + dx) mod W) for some |dy|, |dx| <= R with the row in range.  The outline lives in source space: output rows that show
 *   the same source row show the same outline.
 * W >= 8, H >= 1, H * W < 2^31, Ho * W < 2^31, 0 < n_valid <= B (at most 32767).  Samples from n_valid on are neither read nor
 * written.  Does not synchronise.  dc_render_tile: the source tile of the outline pass (tests derive their shapes from it);
 * dc_render_workspace: 0 for arguments out of range.  Both are host functions. */
int dc_render_tile(int* th, int* tw);
size_t dc_render_workspace(int B, int panels, int H, int W);
int dc_render_frames(int B, int n_valid, int H, int W, const float* fields, int ch, int ldc, float lo, float scale, const uint8_t* lut,
                     int nlut, const void* mask_a, int a_bytes, const void* mask_b /*may be NULL*/, int b_bytes, const int32_t* src_row,
                     int Ho, int shift, const uint8_t* row_line, const uint8_t* col_line, int missing_rgb, int line_argb, int class1_argb,
                     int class2_argb, int width, uint8_t* out, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Climatology (nn.Climatology; predict.py --climatology): the maps over time -- how often a grid point lies inside a cyclone or a river,
 * what the raw fields are there when it does, and what share of a field's total the events account for.  The accumulators live in device
 * memory from call to call, owned by the caller, who zeroes them to start.  Everything is an integer sum: the state after a sequence of
 * frames does not depend on how the sequence was cut into batches, nor on the order of arrival.
 *   G groups (1, 4 seasons, 12 months, ...), frames of H x W pixels, C >= 0 selected channels, bits[c] per selected channel
 *   (nn.event_field_bits).
 *   frames  int64 [G]               frames added to group g
 *   count   int32 [G][2][H][W]      frames in which the pixel was class 1 / class 2
 *   sum     int64 [G][3][H][W][C]   row 0 "all", row 1 "class 1", row 2 "class 2": the sum of q over the frames of that row
 *   n       int32 [G][3][H][W][C]   how many values that sum holds
 * dc_climatology_accumulate, one pass over a batch:
 *   mask    [B][H][W] of 1-, 4- or 8-byte integers (mask_bytes, as dc_render_frames takes them): 1 and 2 are the classes, every other
 *           value is background
 *   fields  fp32 [B][H][W][ldc], channel-last, physical units; NULL exactly when C == 0 (then bits, chan, sum and n are not touched)
 *   chan    int32 [C], device: the index of every selected channel among the ldc channels of a pixel; NULL: the first C channels in order
 *   bits    int32 [C], device       group  int32 [B], device
 * For frame b with g = group[b] in [0, G), pixel p, class k = mask[b][p] and channel value v = fields[b][p][chan[c]]:
 *   frames[g] += 1, once per frame.  k in {1, 2}: count[g][k - 1][p] += 1.
 *   q = rint(ldexp((double)v, bits[c])), ties to even (dc_component_fields' rule).  If v is finite and |q| <= 2^40:
 *   sum[g][0][p][c] += q, n[g][0][p][c] += 1, and for k in {1, 2} the same into row k.  NaN, +-Inf and saturated values add nothing: they
 *   show up as frames - n and count - n.
 * A frame with group[b] < 0 is not read at all (padding samples, gaps, n_valid).  An index >= G is the caller's error (the table is on
 * the device, the host cannot see it): such a frame is skipped as well rather than written out of bounds, and so is a chan entry outside
 * [0, ldc).
 * No atomics: one thread owns a pixel's channel (quad), walks the frames in order with its partial sums in registers and adds them to
 * the accumulators once per run of equal group; every accumulator word has exactly one writer.  The "all" row is read-modified-written
 * once per pixel and run, a class row only where the pixel had that class in the run.  With chan == NULL, ldc == C, C % 4 == 0 and
 * fields, sum and n 16-byte aligned the fields are loaded 16 bytes per lane on consecutive addresses (C = 16: four lanes per pixel) and
 * the accumulators move in 16-byte pieces; every other layout takes scalar loads.  All offsets into sum / n are 64-bit.
 * 1 <= B <= 65535, H * W < 2^31, 1 <= G <= 65536, 0 <= C <= 32, ldc >= 1 (>= C with chan == NULL).  The caller keeps every group below
 * 2^31 - 1 frames: then neither int32 count / n nor int64 sum (2^40 * 2^31 < 2^63) can overflow.
 * dc_climatology_maps, called when maps are read or drawn: K products of the accumulators as fp32 [G][H][W][K] -- with ldc = K exactly
 * what dc_render_frames takes as `fields` of a batch of G -- and a contour mask uint8 [G][H][W] for it to outline.
 *   products  int32 [K][3], device: (0, k, -) the frequency of class k; (1, c, r) the mean of selected channel c in row r; (2, c, k) the
 *             share of class k in selected channel c.  A triple that is none of these gives NaN.
 *   frequency  (float)((double)count / (double)frames), 0 where frames == 0
 *   mean       (float)(ldexp((double)sum, -bits[c]) / (double)n), NaN where n == 0
 *   share      (float)((double)sum_k / (double)sum_all), NaN where sum_all == 0
 *   The two roundings (the fp64 quotient, then fp32) are part of the definition; NaN is the word 0x7FC00000.
 *   contour    1 where frequency_1 >= t1, else 2 where frequency_2 >= t2, else 0 (the fp32 frequencies above against fp32 thresholds)
 *   1 <= K <= 256, G * H * W * K / 256 < 2^31.
 * dc_climatology_block: the pixels one workgroup of the accumulate kernel covers (a host function; tests derive their shapes from it).
 * Neither device call synchronises; both run on the caller's stream.
 * ------------------------------------------------------------------------------------------------ */
int dc_climatology_block(int* pixels);
int dc_climatology_accumulate(int B, int H, int W, int G, const void* mask, int mask_bytes, const float* fields /*NULL when C == 0*/, int C,
                              int ldc, const int32_t* chan /*may be NULL*/, const int32_t* bits, const int32_t* group, int64_t* frames,
                              int32_t* count, int64_t* sum, int32_t* n, void* stream);
int dc_climatology_maps(int G, int H, int W, int C, const int64_t* frames, const int32_t* count, const int64_t* sum, const int32_t* n,
                        const int32_t* bits, int K, const int32_t* products, float t1, float t2, float* out, uint8_t* contour, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Storm-centred composites (nn.StormComposite; predict.py --composites): the fields in STORM coordinates -- a window of S x S grid pixels,
 * S = 2 R + 1, around every event's centre, summed cell by cell over the events of a group, and the sums per great-circle distance from
 * the centre.  The centre is a field extreme that dc_component_fields located (a cyclone's pressure minimum).  The accumulators live in
 * device memory from call to call, owned by the caller, who zeroes them to start.  Everything is an integer sum: the state after a
 * sequence of frames does not depend on how it was cut into batches, on the order of arrival, or on scheduling.
 * dc_composite_centers, one thread per catalogue row (b, k), b < n_valid, k < cap:
 *   table, ncomp  as dc_component_stats leaves them       ftable  int64 [B][cap][Cf][6] as dc_component_fields leaves it, 1 <= Cf <= 32
 *   center_channel in [0, Cf), stat 0 = the minimum's pixel, 1 = the maximum's
 *   class_mask    bit 1 is class 1, bit 2 is class 2 (2, 4 or 6)          min_pixels >= 0
 *   frame_group   int32 [B], device: the group of every frame, G groups    edges  fp32 [NE], device, ascending, 0 <= NE <= 255 (NULL
 *                 allowed when NE == 0); G * (NE + 1) <= 65536
 *   centers       int32 [B][cap]: the centre pixel r0 * W + c0 -- the low 32 bits of the min word, or 0xFFFFFFFF minus the low 32 bits
 *                 of the max word --, -1 where the row is not composited
 *   egroup        int32 [B][cap]: frame_group[b] * (NE + 1) + bin, -1 where centers is -1.  bin = the number of edges e with centre
 *                 value >= e, compared as the order-preserving 32-bit keys of dc_component_fields (unsigned integers: exact, and
 *                 -0.0 < +0.0 as everywhere else)
 *   counts        int64 [5], NOT zeroed by the call: += composited, no_center, below_min_pixels, other_class, uncatalogued; added with
 *                 one atomic per workgroup and counter, as dc_mask_select does
 *   A row k < min(ncomp[b][0], cap) of a frame with frame_group[b] in [0, G) falls into the FIRST category that applies, in this order:
 *   other_class (its class is not 1 or 2, or its bit of class_mask is clear), below_min_pixels (pixels < min_pixels), no_center (the
 *   field row is empty: min == -1, or max == 0; a pixel index >= H * W counts here too, so nothing is ever read through it), else
 *   composited.  uncatalogued += max(ncomp[b][0] - cap, 0) per such frame.  Rows from min(ncomp, cap) on get -1.  Frames with
 *   frame_group[b] < 0 or >= G get -1 everywhere and count nothing.  Samples from n_valid on are neither read nor written.
 * dc_composite_accumulate adds the windows of a batch.  1 <= R <= 40, S <= W, GT = G * (NE + 1) <= 65536, 1 <= C <= 32 selected channels.
 *   events  int64 [GT]             events added to group g
 *   sum     int64 [GT][S][S][C]    the sum of q per cell and selected channel       n  int32 [GT][S][S][C]  how many values it holds
 *   inside  int32 [GT][S][S]       events whose own pixels cover the cell (the mean footprint of the storms)
 *   rsum    int64 [GT][NB][C], rn int64 [GT][NB][C]: the same sums per distance bin
 *   centers, egroup  as dc_composite_centers leaves them      table (for each event's root), labels int32 [B][H][W] as
 *           dc_mask_components leaves them
 *   fields  fp32 [B][H][W][ldc], channel-last, physical units      chan  int32 [C], device, or NULL: as dc_climatology_accumulate
 *   bits    int32 [C], device (nn.composite_bits)                  negate_mask  bit ch: selected channel ch changes sign in a
 *           southern event        flip_south 0 or 1
 *   rbin    uint8 [H][S][R + 1], device (nn.composite_radius_table), or NULL with NB = 0 (rsum and rn are then not touched); 1 <= NB <= 255
 * For every event with centre (r0, c0) and g = egroup in [0, GT), and every cell (i, j) with di = i - R, dj = j - R:
 *   The event is SOUTHERN iff flip_south is set and 2 r0 < H - 1 (row 0 is -90 degrees, as nn.event_weight_tables has it; the equator row
 *   of an odd H is not southern).  The source row is r = r0 - di for a southern event, else r0 + di: di > 0 is poleward in both
 *   hemispheres, and the reflection turns the southern sense of rotation into the northern one.  The source column is c = (c0 + dj)
 *   mod W: columns are periodic.  A cell whose row falls outside [0, H) adds nothing anywhere -- no wrap over the poles; n shows the gap.
 *   events[g] += 1, once per event.  inside[g][i][j] += 1 where labels[b][r][c] == root + 1.
 *   Per selected channel ch: v = fields[b][r][c][chan[ch]], q = rint(ldexp((double)v, bits[ch])), ties to even.  Only finite v with
 *   |q| <= 2^28 take part.  Bit ch of negate_mask set and the event southern: q = -q (the meridional wind components, whose sign the
 *   reflection reverses).  sum[g][i][j][ch] += q, n[g][i][j][ch] += 1.
 *   With rbin: k = rbin[r0][(r - r0) + R][|dj|], indexed with the TRUE source row whether flipped or not.  k < NB: rsum[g][k][ch] += q,
 *   rn[g][k][ch] += 1.
 * An entry of centers outside [0, H * W) or of egroup outside [0, GT) skips its event, and so does a chan entry outside [0, ldc) its
 * channel, rather than reading or writing out of bounds.  Samples from n_valid on are neither read nor written.
 * Capacity: a radial word takes at most S^2 < 2^13 values of at most 2^28 per event.  The caller keeps every group below 2^21 events:
 * then no int64 word (2^13 * 2^28 * 2^21 < 2^63) and no int32 word (n, inside < 2^21) can overflow.
 * The gather is inverted: a thread owns a cell's channel quad (one channel in the scalar form), walks the batch's composited events --
 * compacted into worklist chunks in LDS -- with its partial sums in registers and adds them once per chunk and group; the batch's rows
 * are cut into slices that meet in 64-bit integer atomics; the radial bins are reduced in LDS and leave with one 64-bit atomic per workgroup and
 * word (straight to global memory where NB * C > 4096).  With chan == NULL, ldc == C, C % 4 == 0 and fields 16-byte aligned the fields
 * are loaded 16 bytes per lane on consecutive addresses, split only at the seam; every other layout takes scalar loads.
 * dc_composite_chunk: the events of a worklist chunk (a host function; tests build a frame with more events than that).
 * Neither device call synchronises.  Both run on the caller's stream, behind the catalogue's and the dc_component_fields call of the
 * same batch.
 * ------------------------------------------------------------------------------------------------ */
int dc_composite_chunk(int* events);
int dc_composite_centers(int B, int n_valid, int H, int W, int cap, const int64_t* table, const int32_t* ncomp, const int64_t* ftable,
                         int Cf, int center_channel, int stat, int class_mask, long min_pixels, const int32_t* frame_group, int G,
                         const float* edges /*may be NULL when NE == 0*/, int NE, int32_t* centers, int32_t* egroup, int64_t* counts,
                         void* stream);
int dc_composite_accumulate(int B, int n_valid, int H, int W, int cap, int R, int GT, const int32_t* centers, const int32_t* egroup,
                            const int64_t* table, const int32_t* labels, const float* fields, int C, int ldc,
                            const int32_t* chan /*may be NULL*/, const int32_t* bits, int negate_mask, int flip_south,
                            const uint8_t* rbin /*may be NULL*/, int NB, int64_t* events, int64_t* sum, int32_t* n, int32_t* inside,
                            int64_t* rsum, int64_t* rn, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Neighbourhood verification (nn.FractionsSkill; predict.py --fss): the integer sums behind the Fractions Skill Score (Roberts & Lean
 * 2008), FSS = 1 - sum (F - O)^2 / (sum F^2 + sum O^2), per frame, class and window, and their running totals over all frames.  The score
 * asks at which spatial scale a prediction becomes skilful: a cyclone displaced by a few grid points scores 0 per pixel and may miss
 * its match per object, yet has FSS (n - d) / n at a window of n > d pixels.  Everything is an integer; the quotient is taken on the host.
 *   pred, truth  [B][H][W] of 1-, 4- or 8-byte integers (pred_bytes, truth_bytes, as dc_climatology_accumulate takes a mask): 1 and 2
 *                are the classes, every other value (0, 3, 255, -1, 257, ...) is background
 *   radius       int32 [S], DEVICE memory (a host pointer would not survive a recorded launch list): window s has n_s = 2 radius[s] + 1
 *                pixels a side
 *   wrap         1: columns are taken modulo W (longitude is periodic); 0: columns outside [0, W) contribute 0
 *   row0, row1   the band of rows that is scored
 * For frame b < n_valid, class k in {1, 2} and window s: F(i, j) = the number of pixels of pred[b] == k in the n_s x n_s window centred on
 * (i, j), O(i, j) the same of truth[b]; rows outside [0, H) contribute 0 (zero padding at the poles), also when the window's centre lies
 * inside the band and part of the window outside it -- the band selects the centres, not the pixels counted.
 *   rows    int64 [B][2][S][3]   rows[b][k - 1][s] = (A, B, C) = (sum (F - O)^2, sum F^2, sum O^2) over row0 <= i < row1 and all j
 *   pixels  int64 [B][2][2]      pixels[b][k - 1] = (# pred[b] == k, # truth[b] == k) over the same rows
 * Both are ZEROED by the call and then written; the rows of frames b >= n_valid stay zero and those frames are not read.
 *   total         int64 [2][S][3][2]  per class, window and term a TWO-WORD running total (lo, hi) of `rows` over all frames since the
 *                 caller zeroed it: lo += x, hi += carry -- the value is (hi << 64) | lo with lo taken as unsigned.  One word would not
 *                 do: at a window of 255 pixels a frame of 768 x 1152 can add 2^51.7 to a term, and 2,500 such frames -- less than two
 *                 years of six-hourly data -- pass 2^63.
 *   total_pixels  int64 [2][2], frames int64 [1]: the running sums of `pixels` and of n_valid, plain int64.
 * A single thread per total walks b = 0 .. n_valid - 1 in order, so the state is the same however a sequence is cut into batches.
 * Bounds: 1 <= B <= 4095, 0 <= n_valid <= B, H * W < 2^31, 1 <= S <= 16, 0 <= row0 < row1 <= H, 0 <= radius[s] <= 127 (n_s <= 255), and with
 * wrap also n_s <= W, so that a periodic window counts no column twice.  With n <= 255 a window count is at most 65025, a squared term at
 * most 2^32 and a frame's sum below 2^63: the int64 rows cannot overflow.  The host checks what it can see; a radius outside its bounds is
 * the caller's error (the table is on the device): that window is skipped, its rows stay zero, nothing is read or written out of bounds.
 * The box sum is separable: fss_rows reads both masks, builds per row the prefix sums of the four indicator fields (pred 1, pred 2, truth
 * 1, truth 2) in LDS and stores the four horizontal window counts, each <= 255, as one packed 32-bit word per pixel into the workspace;
 * fss_cols slides a window of those words down every column, squares, and reduces to six 64-bit integer atomics per workgroup (integer
 * sums: order does not matter); fss_total adds the batch to the totals.  One horizontal pass writes every window, a slab per window:
 *   workspace  dc_fss_workspace(B, H, W, S) bytes = B * S * H * W * 4, 4-byte aligned; 0 = arguments out of range.
 * dc_fss_block: the columns of a strip and the rows of a segment one workgroup covers (a host function; tests derive shapes from it).
 * dc_fss_score makes no synchronisation and runs on the caller's stream; a failed argument check sets the message and launches nothing.
 * ------------------------------------------------------------------------------------------------ */
int dc_fss_block(int* cols, int* rows);
size_t dc_fss_workspace(int B, int H, int W, int S);
int dc_fss_score(int B, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth, int truth_bytes, int S,
                 const int32_t* radius /*device*/, int wrap, int row0, int row1, int64_t* rows, int64_t* pixels, int64_t* total,
                 int64_t* total_pixels, int64_t* frames, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Distance-map verification (nn.DistanceSkill; predict.py --distance_skill): capped squared Euclidean distance maps of both masks and the
 * integers behind the distance measures for binary fields -- mean error distance in both directions, (partial) Hausdorff distance,
 * Baddeley's (1992) Delta, and hit rate / success ratio with a displacement of up to r grid points forgiven.  They answer "how far, in
 * grid points, is the predicted object from the labelled one", which neither the per-pixel, the per-object nor the neighbourhood scores
 * do.  Everything is an integer; the quotients and roots are taken on the host (nn.DistanceSkill.decode).
 *   pred, truth  [B][H][W] of 1-, 4- or 8-byte integers (pred_bytes, truth_bytes): class k in {1, 2} is the full-width value k, every
 *                other value (0, 3, 255, -1, 257, 2^32 + 1, ...) is background -- dc_fss_score's rule
 *   metric       d^2((y, x), (y', x')) = (y - y')^2 + dx^2 with dx = min(|x - x'|, W - |x - x'|) under wrap and |x - x'| otherwise.  Rows are
 *                never periodic.  Distances are GRID PIXELS: no latitude weighting, no kilometres
 *   R            the cap, 1 <= R <= 127, with wrap also 2 R + 1 <= W.  A map value is the minimum of d^2 over the pixels of a side and
 *                class where that is <= R^2, and R^2 + 1 ("beyond") otherwise, also where the frame has no such pixel.  The cap makes a
 *                window of +-R rows and columns exact: a nearest pixel within R lies inside it, and if none lies within R every pixel
 *                inside it is farther than R too.  Values fit uint16
 *   maps         uint16 [B][2][2][H][W], side (0 prediction, 1 labels) then class - 1; may be NULL.  0: the pixel itself is of that side
 *                and class.  Written for ALL rows, whatever the row range
 *   table        int32 [R^2 + 2], DEVICE memory, built by the host (nn.distance_table): entry v = ring(v) | dq(v) << 8, ring(v) in bits
 *                0-7 the smallest integer j with j^2 >= v, dq(v) in bits 8-23 = rint(sqrt(v) * 256) in double precision; the last entry
 *                (v = R^2 + 1, beyond) holds ring R + 1 and dq 0.  A ring above R + 1 in the table counts as R + 1
 *   directions   per class: 0 "miss", the sources are the labelled pixels and the distance is to the nearest predicted pixel; 1 "false
 *                alarm", the sources are the predicted pixels and the distance is to the nearest labelled pixel.  A source pixel of a
 *                side is a pixel whose own map value is 0
 *   rows         int64 [B][2 classes][2 directions][R + 4]: cells 0 .. R + 1 count the sources per ring(distance) -- ring 0 is |P and T|,
 *                ring R + 1 the sources beyond the cap --, cell R + 2 is the sum of dq and cell R + 3 the sum of d^2 over the sources
 *                within the cap
 *   baddeley     int64 [B][2]: per class the sum over pixels of (w_P - w_T)^2, w = dq(map value) within the cap and 256 R beyond:
 *                Baddeley's Delta with p = 2 and the cut-off transformation w = min(d, c) at c = R, scaled by 256^2
 *   row0, row1   only sources and Baddeley pixels in these rows count; targets anywhere in the frame still do
 * rows and baddeley of the frames below n_valid are zeroed by the call, in stream order, and then written; frames from n_valid on are
 * neither read nor written, in any buffer, and n_valid == 0 launches nothing.
 *   total           int64 [2][2][R + 4] += rows over the valid frames.  A frame adds at most H * W * 32512 to a cell, below 2^37 at
 *                   768 x 1152: a single word lasts 2^26 such frames
 *   total_baddeley  int64 [2][2]: per class a TWO-WORD total (lo, hi), dc_fss_score's convention: lo += x, hi += carry.  A frame of
 *                   768 x 1152 can add 2^50
 *   frames          int64 [1] += n_valid
 * The sums are integers and every total is added frame by frame by one thread: the state does not depend on the schedule or on how a
 * sequence is cut into batches.  Bounds: 1 <= B <= 4095, 0 <= n_valid <= B, H * W < 2^31, 0 <= row0 < row1 <= H; pointers aligned to their
 * element size.
 * The transform is separable.  dist_vert gives, per pixel and indicator field (pred 1, pred 2, truth 1, truth 2), the rows g <= R + 1 to the
 * nearest pixel of the field in the same column -- a thread per column of a segment of rows with a halo of R rows above and below, which
 * the cap makes exact -- as one byte each of a packed 32-bit word; dist_horz stages those words of a strip and a halo of R columns in
 * LDS, takes min over |dx| <= R of dx^2 + g^2 per field, a tap to the left and one to the right serving all four fields, stops once dx^2
 * reaches the largest running minimum, and scores the pixel in place (ring counters in an LDS histogram, sums by wave reduction, one
 * 64-bit atomic per non-zero cell and workgroup); dist_total adds the batch to the totals.
 *   workspace  dc_distance_workspace(B, H, W, R) bytes = B * H * W * 4, 4-byte aligned; 0 = arguments out of range.
 * dc_distance_block: the columns of a strip and the rows of a segment one workgroup covers (a host function; tests derive shapes from it).
 * dc_distance_score makes no synchronisation and runs on the caller's stream; a failed argument check sets the message and launches
 * nothing.
 * ------------------------------------------------------------------------------------------------ */
int dc_distance_block(int* cols, int* rows);
size_t dc_distance_workspace(int B, int H, int W, int R);
int dc_distance_score(int B, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth, int truth_bytes, int R,
                      const int32_t* table /*device*/, int wrap, int row0, int row1, int64_t* rows, int64_t* baddeley, int64_t* total,
                      int64_t* total_baddeley, int64_t* frames, uint16_t* maps /*may be NULL*/, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Displacement verification (nn.DisplacementSkill; predict.py --displacement): the overlap of the labelled mask with the predicted mask
 * moved by every (dy, dx) of a window -- the cross-correlation of two binary fields -- and the shift with the most hits: the rigid-shift
 * part of Ebert & McBride's (2000) CRA method, the field-deformation family of Gilleland et al. (2009).  It answers "how much of the miss
 * is the prediction lying two pixels too far north", which the distance measures (no direction), the matched events' centroids (overlapping
 * objects only) and the FSS (a scale, not a vector) do not.  Everything is an integer; the host decodes (nn.DisplacementSkill.decode).
 *   pred, truth  [B][H][W] of 1-, 4- or 8-byte integers (pred_bytes, truth_bytes), each side with its own element size: class k in {1, 2}
 *                is the full-width value k, every other value (0, 3, 255, -1, 257, 2^32 + 1, ...) is background -- dc_fss_score's rule.
 *                P_k, T_k: the indicator fields of class k
 *   columns      periodic, always (a regional grid is out of scope); rows are never periodic
 *   R            the radius of the window, 1 <= R <= 63, with 2 R + 1 <= W
 *   row0, row1   the band, 0 <= row0 < row1 <= H
 * The prediction moved by (dy, dx), |dy|, |dx| <= R, is P'_k(y, x) = P_k(y - dy, (x - dx) mod W) where 0 <= y - dy < H and 0 elsewhere:
 * pixels moved over a pole are lost.
 *   hits[b][k][dy][dx] = #{(y, x): row0 <= y < row1, T_k(y, x) = 1, P'_k(y, x) = 1}
 *   kept[b][k][dy]     = #{(y', x): P_k(y', x) = 1, row0 <= y' + dy < row1}, the predicted pixels inside the band after the move; it does
 *                        not depend on dx
 *   rows         int64 [B][2][2 R + 1][2 R + 2]: cells 0 .. 2 R of row dy + R are the hits for dx = -R .. R, cell 2 R + 1 is kept
 *   pixels       int64 [B][2][2]: per class (the predicted pixels of the WHOLE frame, the labelled pixels inside the band)
 *   best         int64 [B][2][4]: (dy, dx, hits, kept[dy]) of the best shift, the one with the most hits (the maximum of the
 *                cross-correlation; not the minimum squared error, which rewards pushing a false alarm out of the band or over a pole).
 *                Ties go to the smaller dy^2 + dx^2, then the smaller dy, then the smaller dx: a table without hits gives (0, 0).  The
 *                order is the maximum of one 64-bit key, hits << 27 | (8191 - (dy^2 + dx^2)) << 14 | (127 - (dy + R)) << 7 |
 *                (127 - (dx + R)), which H * W < 2^31 keeps below 2^58
 * rows, pixels and best of the frames below n_valid are zeroed by the call, in stream order, and then written; frames from n_valid on are
 * neither read nor written, in any buffer, and n_valid == 0 launches nothing.
 *   total         int64 [2][2 R + 1][2 R + 2] += rows over the valid frames; single words: a frame adds at most H * W to a cell
 *   total_pixels  int64 [2][2] += pixels
 *   frames        int64 [1] += n_valid
 * The sums are integers and every total is added frame by frame by one thread: the state does not depend on the schedule or on how a
 * sequence is cut into batches.  Bounds: 1 <= B <= 4095, 0 <= n_valid <= B, H * W < 2^31; masks aligned to their element size, every other
 * pointer to 8 bytes.
 * disp_pack turns both masks into bit planes, a wave's ballot of the class test being one word of 64 pixels: label rows of ceil(W / 64)
 * words, and prediction rows EXTENDED by a periodic halo, bit i = P[(i - R) mod W] for i < W + 2 R, in ceil((W + 2 R) / 64) + 1 words, so
 * that the 64 bits meeting a label word under any dx are a funnel shift of two neighbouring words; it also counts the predicted pixels
 * per row and `pixels`.  disp_corr gives a workgroup one (frame, class, dy) and a segment of rows of the band, a lane one dx: the label
 * word is uniform and skipped when zero, else AND and popcount into a register, one 64-bit atomic per lane at the end; one more lane sums
 * the row counts into kept.  disp_best takes the maximum of the key, disp_total adds the batch to the totals.
 *   workspace  dc_displacement_workspace(B, H, W, R) bytes, 8-byte aligned: the bit planes and the row counts, B * 2 * H * ((ceil(W / 64)
 *              + ceil((W + 2 R) / 64) + 1) * 8 + 4); 0 = arguments out of range.
 * dc_displacement_block: the pixels of a word and the label rows of a segment one workgroup of disp_corr covers (a host function; tests
 * derive shapes from it).  dc_displacement_score makes no synchronisation and runs on the caller's stream; a failed argument check sets
 * the message and launches nothing.
 * ------------------------------------------------------------------------------------------------ */
int dc_displacement_block(int* bits, int* rows);
size_t dc_displacement_workspace(int B, int H, int W, int R);
int dc_displacement_score(int B, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth, int truth_bytes, int R,
                          int row0, int row1, int64_t* rows, int64_t* pixels, int64_t* best, int64_t* total, int64_t* total_pixels,
                          int64_t* frames, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scale-separation verification (nn.ScaleSkill; predict.py --scale_skill): the integers behind the intensity-scale skill score of Casati,
 * Ross & Stephenson (2004) with the energies of Casati (2010), the scale-separation family of Gilleland et al. (2009).  The binary error
 * field of a class is split by a 2-D Haar transform into components of spatial scale 1, 2, 4, ... grid pixels; the squared error and the
 * energy of prediction and labels are reported per scale.  It answers "at which scale does the error sit", which the FSS (everything below
 * the window), the best shift (one vector) and the distance maps (a length without a scale) do not.  Everything is an integer; the host
 * decodes (nn.ScaleSkill.decode).
 *   pred, truth  [B][H][W] of 1-, 4- or 8-byte integers (pred_bytes, truth_bytes), each side with its own element size: class k in {1, 2}
 *                is the full-width value k, every other value is background -- dc_fss_score's rule
 *   row0, row1   the band, 0 <= row0 < row1 <= H
 *   L            the levels, 1 <= L <= 8; the tile T = 2^L must divide both row1 - row0 and W (row0 itself may be any row)
 *   origins      int32 [O] in DEVICE memory (a host pointer would not survive a recorded launch list), 1 <= O <= 8, each 0 <= c < T
 * For origin c the band is tiled by blocks of side 2^j, j = 0 .. L, on a grid that starts at row row0 and column c; columns are taken
 * modulo W, so a block may lie across the seam; rows are never periodic.  S_F, S_O: the pixels of a block with pred == k, truth == k.
 *   rows    int64 [B][2][O][L + 1][3]: per frame, class, origin and level (A, B, C) = (sum (S_F - S_O)^2, sum S_F^2, sum S_O^2) over the
 *           blocks of that level
 *   pixels  int64 [B][2][2]: per class (# pred == k, # truth == k) inside the band
 * rows and pixels of the frames below n_valid are zeroed by the call, in stream order, and then written; frames from n_valid on are
 * neither read nor written, in any buffer, and n_valid == 0 launches nothing.  An origin outside [0, T) is the caller's error that only
 * the device can see: it is skipped, its rows stay zero, and nothing is read or written out of bounds.
 *   total         int64 [2][O][L + 1][3][2] += rows over the valid frames, as two-word integers (lo, hi) in dc_fss_score's convention,
 *                 lo += x, hi += carry: a frame adds up to H * W * 4^L < 2^47 to a cell, so one word would last 65,536 frames only
 *   total_pixels  int64 [2][2] += pixels
 *   frames        int64 [1] += n_valid
 * At level 0 A is the number of mismatched pixels, B and C equal `pixels`, the triple does not depend on the origin and equals
 * dc_fss_score's row of window 1 on the same band.  With Q_j any of A, B, C at level j, the Haar component of scale 2^j carries
 * E_j = (4 Q_j - Q_{j+1}) / 4^(j+1) for j < L (the detail between the block means of side 2^j and 2^(j+1)) and E_L = Q_L / 4^L (the
 * father component: the tile means); the E_j are non-negative and sum to Q_0.
 * The sums are integers and every total is added frame by frame by one thread: the state does not depend on the schedule or on how a
 * sequence is cut into batches.  Bounds: 1 <= B <= 4095, 0 <= n_valid <= B, H * W < 2^31; masks aligned to their element size, origins
 * and workspace to 4 bytes, every other pointer to 8.
 * scale_sums gives a workgroup one 64 x 64 tile of one (frame, origin) and a thread one 4 x 4 block, in Morton order, so that levels 0 to
 * 2 stay in registers, 3 to 5 are lane exchanges and 6 goes through LDS; one 64-bit atomic per non-zero cell.  For L > 6 it leaves each
 * tile's four sums in the workspace and scale_coarse forms levels 7 and 8 from them (sums up to 2^16 in 32-bit words, squares up to 2^32
 * in 64 bits).  scale_total adds the batch to the totals.
 *   workspace  dc_scale_workspace(B, H, W, L, O) bytes, 4-byte aligned: four 32-bit sums per tile, B * O * ceil(H / 64) * ceil(W / 64)
 *              * 16, whatever L (read and written for L > 6 only); 0 = arguments out of range (T > H or T does not divide W included).
 * dc_scale_block: the columns and rows of the workgroup tile (a host function; tests derive shapes from it).  dc_scale_score makes no
 * synchronisation and runs on the caller's stream; a failed argument check sets the message and launches nothing.
 * ------------------------------------------------------------------------------------------------ */
int dc_scale_block(int* cols, int* rows);
size_t dc_scale_workspace(int B, int H, int W, int L, int O);
int dc_scale_score(int B, int n_valid, int H, int W, const void* pred, int pred_bytes, const void* truth, int truth_bytes, int L, int O,
                   const int32_t* origins /*device*/, int row0, int row1, int64_t* rows, int64_t* pixels, int64_t* total,
                   int64_t* total_pixels, int64_t* frames, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Probabilistic verification (nn.ProbabilitySkill; predict.py --prob_skill): the integers behind the reliability diagram, the Brier score
 * with Murphy's (1973) decomposition, and POD / POFD / CSI per probability threshold with ROC and AUC (Mason 1982), per class, from the
 * classifier's softmax probabilities -- not from the argmax mask that every other verification family scores.  One joint histogram per
 * class (probability bin x whether the label is that class, with the sum of the probabilities per cell) and one sum of squared errors
 * answer all three; the host decodes them (nn.ProbabilitySkill.decode).
 * Per pixel, with its logits l0, l1, l2 and its label (load_label of csrc/pixel_score.h: 1-, 4- or 8-byte integers, the full value compared):
 *   p_c   = e_c / se in fp32, (e, se) = softmax_terms(l0, l1, l2, first_max(l0, l1, l2).best)
 *   q_c   = __float2int_rn(p_c * 65536.f), in [0, 65536]; o_c = (label == c)
 *   bin_c = min(K - 1, (q_c * K) >> 16): a function of the INTEGER q; the forecast "class c at threshold k / K" is bin_c >= k
 * A pixel whose label is outside [0, 3) is counted in pixels[b][1] and contributes nothing else; otherwise a pixel with a logit that is
 * not finite is counted in pixels[b][2] and contributes nothing else; every other pixel is scored and counted in pixels[b][0].  From q on
 * everything is an integer: equal logits give equal state whatever the schedule and however the frames are cut into batches.
 *   logits_nchw   fp32 [B][3][H][W]; labels [B][H][W] of label_bytes = 1, 4 or 8
 *   K             bins, 1 .. 256
 *   hist          int64 [3][2][K][2]  class, outcome, bin, (n, sum q) over THIS call's frames b < n_valid; zeroed by the call
 *   rows          int64 [B][3]        per sample and class sum (q_c - o_c * 65536)^2, the Brier score's numerator scaled by 2^32
 *   pixels        int64 [B][3]        (scored, label outside [0, 3), a logit not finite)
 *                 rows and pixels of the samples < n_valid are zeroed by the call, in stream order, and then written; the samples
 *                 >= n_valid are neither read nor written, in any buffer.
 *   total_hist    int64 [3][2][K][2]  += hist
 *   total_sq      int64 [3][2]        per class a TWO-WORD running total (lo, hi) of rows, dc_fss_score's convention: lo += x,
 *                 hi += carry, the value (hi << 64) | lo with lo taken as unsigned.  A frame can add 2^30 * 2^32 = 2^62.
 *   total_pixels  int64 [3], frames int64 [1]: += pixels, += n_valid
 * Bounds: 1 <= B <= 4095, 0 <= n_valid <= B, H * W <= 2^30, so that total_hist's sum of q holds 2^63 / (2^30 * 2^16) = 2^17 frames of
 * the largest size and 2^27 of 768 x 1152.  Pointers are aligned to their element size.
 * prob_hist gives every workgroup dc_prob_block's `pixels` consecutive pixels of one sample and a private histogram in LDS (64-bit cells,
 * count << 40 | sum q, which cannot wrap within that many pixels); per class a wave whose scored pixels all fall into one cell adds once,
 * from one lane; the workgroup flushes its non-zero cells by 64-bit global atomics.  Where H * W is a multiple of 4 and the logits are
 * 16-byte aligned the loads are 16 bytes wide (prob_hist_vec), else 4 (prob_hist).  prob_zero clears this call's outputs in front of it,
 * prob_total adds the call to the totals behind it: three launches, with n_valid == 0 only the first.
 * dc_prob_block: the pixels one workgroup takes, and the cap on the workgroups per sample (0: none -- a workgroup takes one chunk and
 * ends, there is no grid-stride loop).  A host function; tests derive shapes from it.
 * dc_prob_score makes no synchronisation and runs on the caller's stream; a failed argument check sets the message and launches nothing.
 * ------------------------------------------------------------------------------------------------ */
int dc_prob_block(int* pixels, int* max_groups);
int dc_prob_score(int B, int n_valid, int H, int W, const float* logits_nchw, const void* labels, int label_bytes, int K, int64_t* hist,
                  int64_t* rows, int64_t* pixels, int64_t* total_hist, int64_t* total_sq, int64_t* total_pixels, int64_t* frames,
                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * The decision rule (nn.DecisionRule; predict.py --decision_low / --decision_high / --decision_from): a mask from the stored logits by
 * per-class probability thresholds, with hysteresis -- instead of the argmax, which the class weights of the training bias on purpose.
 * dc_prob_score measures what every threshold would give; this applies one.  Per pixel with its logits l0, l1, l2:
 *   q_c        dc_prob_score's integer, by the same inline function (csrc/pixel_score.h: prob_q): p_c = e_c / se in fp32 with (e, se) =
 *              softmax_terms(l, first_max(l).best), q_c = __float2int_rn(p_c * 65536.f), in [0, 65536]
 *   the rule   four integers in [0, 65537]: low[1], low[2], high[1], high[2] with high[c] >= low[c]; 65537 means "never"
 *   candidate  class c in {1, 2} QUALIFIES iff q_c >= low[c].  cand is 0 if neither class qualifies, the qualifying class if only one
 *              does, and the class with the larger q if both do; class 1 wins on equal q
 *   seed       the pixel is a seed iff cand = c != 0 and q_c >= high[c]; a pixel that lost the conflict is no seed of the class that lost
 *   non-finite a pixel with any logit that is NaN or an infinity is background, is no seed, and is counted
 *   out        out[p] = cand[p] iff the connected component of cand that holds p contains at least one seed, else 0; the component is
 *              dc_mask_components': one class, connectivity 4 or 8, columns periodic with wrap, rows never
 * With high == low for both classes every candidate is a seed and out == cand: plain thresholding, for which the caller runs no
 * component pass.  dc_prob_score's forecast "class c at threshold k / K", min(K - 1, (q * K) >> 16) >= k, is q >= ceil(k * 65536 / K) for
 * k < K and "never" for k = K (nn.decision_q_from_bin): a threshold read off its table reproduces the scored forecast bit for bit.
 *   logits_nchw  fp32 [B][3][H][W]
 *   cand, seed   uint8 [B][H][W]: the candidate class; 1 at a seed.  seed may be NULL iff high == low for both classes
 *   labels       int32 [B][H][W], what dc_mask_components left for cand on the same stream
 *   flags        uint8 [B][H][W] (dc_decide_workspace bytes), indexed by root (label - 1): zeroed by dc_hysteresis_select in stream order
 *                for the samples below n_valid, then 1 at the root of every component that holds a seed.  By root, not by rank: there is
 *                no event cap anywhere in this path
 *   out_mask     uint8 [B][H][W]; may not alias cand
 *   counts       int64 [B][12]: words 0-4 for class 1 -- candidate pixels, seed pixels, kept pixels, candidate events, kept events --,
 *                words 5-9 the same for class 2, word 10 the pixels with a non-finite logit, word 11 the pixels where both classes
 *                qualified.  dc_logits_decide zeroes the rows of the samples below n_valid and fills the candidate, seed, non-finite and
 *                conflict words; dc_hysteresis_select adds the kept pixels and, counted at root pixels, the events.  On the
 *                plain-threshold route the caller copies candidate pixels into kept pixels and the event words stay 0
 * dc_logits_decide is one streaming pass: a workgroup takes dc_decide_block's `pixels` consecutive pixels of one sample and ends.  Where
 * H * W is a multiple of 4, the logits are 16-byte aligned and cand and seed 4-byte aligned, the loads are 16 bytes wide and four pixels
 * leave in one 32-bit store per plane (decide_q_vec), else 4-byte loads and byte stores (decide_q).  The counters go through ballots and
 * one workgroup reduction; there are no per-pixel atomics.  dc_hysteresis_select makes two launches: decide_mark, in which every seed
 * pixel stores 1 at its root's flag (all writers of a byte write the same value, so a plain store serves), and decide_select.
 * Samples from n_valid on are neither read nor written, in any buffer; n_valid == 0 launches nothing; nothing synchronises; a failed
 * argument check sets the message and launches nothing.  Bounds: 1 <= B <= 4095, 0 <= n_valid <= B, H * W <= 2^30, pointers aligned to
 * their element size.  dc_decide_block and dc_decide_workspace (0: arguments out of range) are host functions.
 * ------------------------------------------------------------------------------------------------ */
int dc_decide_block(int* pixels);
size_t dc_decide_workspace(int B, int H, int W);
int dc_logits_decide(int B, int n_valid, int H, int W, const float* logits_nchw, int low1, int low2, int high1, int high2, uint8_t* cand,
                     uint8_t* seed /*may be NULL iff high == low*/, int64_t* counts /*[B][12]*/, void* stream);
int dc_hysteresis_select(int B, int n_valid, int H, int W, const uint8_t* cand, const uint8_t* seed, const int32_t* labels, uint8_t* flags,
                         uint8_t* out_mask, int64_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The view ensemble (nn.ViewEnsemble, nn.view_input; predict.py --ensemble_rolls / --ensemble_flip_lat / --ensemble_negate /
 * --ensemble_seam_margin): test-time augmentation on the periodic grid.  Every convolution pads the first and the last column with zeros,
 * while everything behind the classifier takes the columns as periodic; a column roll is an exact symmetry of the data that only the
 * padding breaks, and a mirrored hemisphere with the meridional winds negated is the second physical view.  The forecasts of several views
 * are pooled per pixel in q, dc_prob_score's integer, and leave as ONE fp32 NCHW logits tensor: its mask is dc_logits_predict of it, its q
 * is prob_q of it, its thresholds are dc_logits_decide of it, and no consumer changes.
 *   view       (roll, flip) with 0 <= roll < W and flip in {0, 1}: view pixel (h, w) shows source pixel
 *              src(h, w) = (flip ? H - 1 - h : h, (w + roll) mod W)
 *   input      dc_input_view_hwc: out[n, h, w, j] = scale[j] * (sign[j] * x[n, src(h, w), channels[j]] - shift[j]), converted to the
 *              activation dtype.  sign[j] is +1 or -1 (NULL: all +1) and is applied in physical units, in front of the normalisation.  The
 *              expression is dc_input_normalize_hwc's with the source pixel permuted: the identity view with a NULL sign gives that
 *              call's bits.  NHWC output only
 *   member m   fp32 NCHW logits in VIEW coordinates, with the view and an optional weight per SOURCE column, wt[W] (uint16, at least 1;
 *              NULL: 1).  For source pixel p take the three logits at the view pixel that shows p.  If they are not all finite (an
 *              exponent of all ones) then bad[p] += 1 and nothing else happens at p.  Otherwise, with q = prob_q(l0, l1, l2) (csrc/
 *              pixel_score.h, the chain of dc_prob_score and dc_logits_decide) and am the first maximum of (l0, l1, l2):
 *              S_c[p] += wt[col(p)] * q_c, votes_am[p] += 1, and for m == 0 first[p] = am -- 3 where the pixel was not finite
 *   state      uint32 [B][4][H][W]: the planes S_0, S_1, S_2 and one packed plane: bits 0-5, 6-11, 12-17 the votes of class 0, 1, 2,
 *              bits 18-23 bad, bits 24-25 first.  Six bits: at most 63 members.  Member 0 STORES its contribution and the others add to
 *              it, so nothing has to clear the state; one thread owns a pixel, so there are no atomics.  The caller keeps the sum of the
 *              members' largest weights at or below 65535 (S < 2^32) and adds no 64th member: nn.ViewEnsemble refuses both
 *   pool       dc_ensemble_pool, for every pixel with bad == 0: top is the first class with the largest S_c, and
 *              L_c = (float) log((double) max(S_c, 1) / (double) S_top), division and log in fp64, one rounding to fp32.  So L_top is
 *              0.0f exactly, S_c == S_top gives 0.0f as well, and S_c < S_top gives L_c < 0: the first maximum of L is the integer first
 *              maximum of (S_0, S_1, S_2), ties included, and prob_q(L)_c stands within 0.75 of 65536 * max(S_c, 1) / sum_k max(S_k, 1).
 *              A pixel with bad > 0 gets three NaNs, which dc_prob_score and dc_logits_decide count as not finite
 *   logits_nchw  of dc_ensemble_pool: fp32 [B][3][H][W], the pooled forecast
 *   rows       int64 [B][208], zeroed by the call for the samples below n_valid, in stream order: word 64 c + k the pixels of the frame
 *              with exactly k votes for class c; word 192 + 4 i + j the pixels whose first is i and whose pooled class is j (3: not
 *              finite on either side)
 *   totals     int64 [208] += rows over the samples below n_valid; frames int64 [1] += n_valid.  Integer sums: the same however the
 *              frames are cut into batches
 * All three are streaming passes in dc_logits_decide's layout: a workgroup takes dc_ensemble_block's `pixels` consecutive pixels of one
 * sample and ends.  view_normalize gives one 16-byte vector of an output pixel to a thread; where all file channels are taken in file
 * order (channels NULL, Cfile a multiple of 4, x_hwc 16-byte aligned) the loads are 16 bytes wide too -- the roll moves whole pixels and
 * the flip whole rows, so the alignment never breaks.  dc_ensemble_add: where W and roll are multiples of 4, logits and state 16-byte and
 * col_weight 8-byte aligned, a thread owns four consecutive source pixels, whose view pixels are consecutive and aligned too
 * (ensemble_add_vec); else 4-byte accesses (ensemble_add).  dc_ensemble_pool counts through cells in LDS, the pixels of a wave that share
 * a cell by one lane, and one workgroup reduction with 64-bit atomics per non-zero cell; there are no per-pixel global atomics.
 * Samples from n_valid on are neither read nor written, in any buffer; n_valid == 0 launches nothing; nothing synchronises; a failed
 * argument check sets the message and launches nothing.  Bounds: 1 <= B <= 4095, 0 <= n_valid <= B, H * W <= 2^30, 0 <= roll < W,
 * 0 <= member < 63, 1 <= members <= 63, pointers aligned to their element size (out as dc_input_normalize_hwc's).  dc_input_view_hwc
 * takes all B samples.  dc_ensemble_block is a host function: the pixels one workgroup takes; tests derive shapes from it.
 * ------------------------------------------------------------------------------------------------ */
int dc_ensemble_block(int* pixels);
int dc_input_view_hwc(int dtype, int B, int H, int W, int Cfile, int C, const int* channels /*NULL: the first C*/,
                      const float* sign /*NULL: all +1*/, const float* x_hwc, const float* shift, const float* scale, int roll, int flip,
                      void* out, int ldo, void* stream);
int dc_ensemble_add(int B, int n_valid, int H, int W, const float* logits_nchw, int roll, int flip,
                    const uint16_t* col_weight /*NULL: 1*/, int member, uint32_t* state, void* stream);
int dc_ensemble_pool(int B, int n_valid, int H, int W, int members, const uint32_t* state, float* logits_nchw, int64_t* rows /*[B][208]*/,
                     int64_t* totals /*[208]*/, int64_t* frames /*[1]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Train-time augmentation (data.Augment, data.InputPipeline(augment=...); train.py --augment_roll / --augment_flip_lat / --augment_negate /
 * --augment_seed): the two exact symmetries of the view ensemble above, applied while a training batch is staged, so that the network sees
 * every sample at a longitude offset of its own and learns that the seam of the zero padding is nowhere in particular.  The reference
 * shuffles its file list once and never again (data/cam_hdf5_dataset.py:39-41), so every epoch shows the same batches pixel for pixel;
 * per-epoch views are the variety a long run gets.  ONE launch stages the whole batch: dc_input_view_hwc gives one view to all B samples,
 * negates unconditionally and has no labels.
 *   views_host HOST memory, int32 [B][2]: (roll_n, flip_n) of sample n with 0 <= roll_n < W and flip_n in {0, 1}.  View pixel (h, w) of
 *              sample n shows source pixel src_n(h, w) = (flip_n ? H - 1 - h : h, (w + roll_n) mod W), the view ensemble's definition.
 *              The table is read and checked BEFORE THE CALL RETURNS and travels, packed into one 32-bit word per sample, in the kernel
 *              arguments (1 KB at B = 256): the device never indexes by a number the host has not range-checked, a row's word is uniform
 *              over its workgroup and read by a scalar load, and there is no table in device memory, no extra copy, no pinned buffer.
 *              The caller may reuse the array as soon as the call has returned.  Because a host pointer is read at call time the call is
 *              NOT meant for dc_program_* recording (a replay would read whatever the array holds then, or a dead address); the input
 *              pipeline is not part of the recorded step
 *   data       out[n, h, w, j] = scale[j] * (s_nj * x[n, src_n(h, w), channels[j]] - shift[j]), converted to the activation dtype, NHWC
 *              with leading dimension ldo.  s_nj = flip_sign[j] where flip_n is set and flip_sign is not NULL, else +1: only the mirrored
 *              samples have their meridional winds negated, in physical units, in front of the normalisation
 *   labels     labels_out[n, h, w] = labels_in[n, src_n(h, w)], int64 [B][H][W] both: the words are moved verbatim and not interpreted, so
 *              an out-of-range label stays what it was, for the loss kernel to flag.  Both NULL: the data alone.  Never in place
 *   bits       sample n of `out` is what dc_input_view_hwc writes for that sample alone with (roll_n, flip_n) and sign = flip_n ?
 *              flip_sign : NULL; a batch of identity views is dc_input_normalize_hwc bit for bit (+-1 * v is exact, whether or not it
 *              is contracted with the subtraction)
 * The kernel (augment_view) has view_normalize's decomposition: blockIdx.y walks the B * H rows, a row of the view is a rotated row of the
 * source, a thread takes one 16-byte vector of one output pixel.  Where all file channels are taken in file order (channels NULL, Cfile a
 * multiple of 4, x_hwc 16-byte aligned) the loads are 16 bytes wide too -- the roll moves whole pixels and the flip whole rows, so the
 * alignment never breaks; a channel selection gathers by 4-byte loads.  The workgroups of a row then move its labels by 8-byte words.  One
 * streaming pass, 64 + 8 bytes in and 32 + 8 bytes out per pixel (bf16, 16 channels); no atomics, no LDS.
 * Nothing synchronises; a failed argument check sets the message and launches nothing.  Refused: B outside [1, 256]; a view outside the
 * ranges above; a dtype other than DC_F32 / DC_BF16; a NULL x_hwc, shift, scale, out or views_host; one label pointer without the other;
 * labels_in == labels_out; a pointer not aligned to its element (out and ldo as dc_input_normalize_hwc's); Cfile < C; B * H >= 2^31 or
 * H * W > 2^30.
 * ------------------------------------------------------------------------------------------------ */
int dc_augment_view_hwc(int dtype, int B, int H, int W, int Cfile, int C, const int* channels /*NULL: the first C*/,
                        const float* flip_sign /*NULL: all +1*/, const float* x_hwc, const float* shift, const float* scale,
                        const int32_t* views_host /*[B][2]: roll, flip -- HOST memory*/,
                        const int64_t* labels_in /*[B][H][W] or NULL*/, int64_t* labels_out /*NULL iff labels_in is*/,
                        void* out, int ldo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image-pool branch helpers (deeplab_xception.py:425,449-450): AdaptiveAvgPool2d((1,1)), the 1x1 ->
 * HxW "bilinear" broadcast and their backward passes.  The per-sample vectors ([N][C]: out, g, v below) are ALWAYS
 * fp32 whatever `dtype` the NHWC side uses: the branch's BatchNorm sees only N values per channel.
 * ------------------------------------------------------------------------------------------------ */
int dc_avgpool_fwd(int dtype, int N, int HW, int C, const void* x, int ldx, void* out /*[N][C]*/, void* stream);
/* dx[n,p,c] += g[n,c] / HW */
int dc_avgpool_bwd_add(int dtype, int N, int HW, int C, const void* g, void* dx, int lddx, void* stream);
/* out[n,p,c] = v[n,c] */
int dc_broadcast_hw(int dtype, int N, int HW, int C, const void* v, void* out, int ldo, void* stream);
/* g[n,c] = sum_p dout[n,p,c] */
int dc_sum_hw(int dtype, int N, int HW, int C, const void* dout, int lddo, void* g, void* stream);
/* dst = src (NHWC view copy, e.g. gradient slices) */
int dc_copy_view(int dtype, long M, int C, const void* src, int lds, void* dst, int ldd, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizers over one flat fp32 arena: torch.optim.Adam / AdamW (train_hdf5_ddp.py:213-216) and LAMB
 * (apex FusedLAMB, :218; this project's own definition).  `step` is the 1-based step count.
 * `lr` is read from a device float so that a captured hipGraph follows the LR schedule.
 * ------------------------------------------------------------------------------------------------ */
int dc_adam_step(int kind, long n, float* p, const float* g, float* m, float* v, const float* lr_dev,
                 float beta1, float beta2, float eps, float weight_decay, const int* step_dev, float grad_scale,
                 void* stream);
/* LAMB: tensor t occupies [offsets[t], offsets[t+1]) of the arena (device int64[ntensors+1]).
 * workspace: dc_lamb_workspace_words(ntensors, n) 4-byte words (partial sums of the global norm, chunk plan, per-chunk
 * norms and the n-element update direction).  p, g, m, v and workspace must be 16-byte aligned.  `g` is only read (as apex FusedLAMB leaves .grad intact).
 * As apex with use_nvlamb=False, the per-tensor trust ratio is applied only when weight_decay != 0.
 * No atomics: the update is bit-identical from run to run. */
size_t dc_lamb_workspace_words(int ntensors, long n);
int dc_lamb_step(int ntensors, const int64_t* offsets_dev, long n, float* p, const float* g, float* m, float* v,
                 const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                 const int* step_dev, float max_grad_norm, float grad_scale, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient payload of the data-parallel all-reduce (train_hdf5_ddp.py:227,363: apex / torch DDP reduce the gradients the
 * optimizer reads; SURVEY 5.8: 225.8 MB fp32 or 112.9 MB bf16 per step).  The fp32 arena stays the master copy:
 * dc_grad_pack_bf16 rounds a bucket (round-to-nearest-even) into the send buffer the collective sums in bf16,
 * dc_grad_unpack_bf16 widens the reduced buffer back into the arena.  n elements; both pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------------ */
int dc_grad_pack_bf16(long n, const float* g, void* out_bf16, void* stream);
int dc_grad_unpack_bf16(long n, const void* in_bf16, float* g, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient accumulation over virtual ranks: K micro-batches on one device stand for K data-parallel ranks, whose gradients apex /
 * torch DDP sum and divide by the world size before the one optimizer update (train_hdf5_ddp.py:227,359-363).  Called on a bucket
 * range of the gradient arena (g) and the same range of the accumulation arena (acc) as the bucket becomes ready during backward:
 *   first != 0:  acc[i] = g[i]      (overwrites: acc may hold anything, NaN included; nothing clears the arena)
 *   first == 0:  acc[i] += g[i]     (fp32)
 * Any n >= 0.  g and acc need not be 16-byte aligned, but must sit at the SAME offset from a 16-byte boundary (the same range of two
 * arenas does); the elements in front of the first boundary and behind the last whole vector take a scalar path.  One thread owns one
 * element and there are no atomics: the sum is bit-identical from run to run, and in the order of the calls.
 * ------------------------------------------------------------------------------------------------ */
int dc_grad_accumulate(long n, const float* g, float* acc, int first, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The gradient all-reduce itself, inside the library (csrc/comm.cpp; SURVEY section 8b: grad_allreduce_{enqueue,wait} over a raw RCCL
 * communicator).  Replaces the reducer of apex / torch DistributedDataParallel: train_hdf5_ddp.py:227 (construction: one communicator per
 * process) and :363 (loss.backward(): bucketed all-reduces overlapped with the rest of backward).
 *   dc_comm_unique_id        rank 0: 128 bytes (ncclGetUniqueId) that the host program hands to every rank by any out-of-band channel
 *   dc_comm_create           every rank: ncclCommInitRank on the current device + a communication stream of the library's own.
 *                            world == 1 with id128 == NULL: no RCCL at all (enqueue / wait are no-ops)
 *   dc_comm_adopt            wrap an ncclComm_t the caller already has (not destroyed by dc_comm_destroy)
 *   dc_comm_create_callback  transport = a host function (tests: torch.distributed over gloo); sync_stream != 0: the compute stream is
 *                            synchronised before every call back (device buffers)
 *   dc_grad_allreduce_enqueue  the communication stream waits for everything enqueued on compute_stream so far, then sums
 *                            buf[0 .. count) (DC_F32 or DC_BF16) across the ranks IN PLACE on it; returns at once
 *   dc_grad_allreduce_wait   compute_stream waits for every collective enqueued so far (the optimizer goes behind it)
 * enqueue / wait take word-sized arguments only, so dc_program_append records them like any kernel launch.
 * ------------------------------------------------------------------------------------------------ */
typedef int (*dc_allreduce_callback)(void* ctx, void* buf, size_t count, int dtype);
int dc_comm_unique_id(void* id128);
int dc_comm_create(const void* id128, int rank, int world, void** comm);
int dc_comm_adopt(void* nccl_comm, int rank, int world, void** comm);
int dc_comm_create_callback(dc_allreduce_callback fn, void* ctx, int rank, int world, int sync_stream, void** comm);
int dc_comm_destroy(void* comm);
/* transport: 0 none (single rank), 1 RCCL, 2 callback; enqueued: calls of dc_grad_allreduce_enqueue so far */
int dc_comm_info(void* comm, int* rank, int* world, int* transport, long* enqueued);
int dc_grad_allreduce_enqueue(void* comm, void* buf, size_t count, int dtype, void* compute_stream);
int dc_grad_allreduce_wait(void* comm, void* compute_stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPCAM_HIP_H_ */
