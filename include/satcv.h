/*
 * satcv.h -- C ABI of the MI355X-native U-Net / ASPP tile pipeline (libsatcv.so).
 *
 * The reference (mjevans26/Satellite_ComputerVision) has no FFI for this path:
 * every tensor op of utils/model_tools.py is delegated to tf.keras layers.  Each
 * entry point below therefore replaces one Keras layer call site (cited) and is
 * what the reference-side binding would call instead of TensorFlow (see
 * INTEGRATION.md for the ctypes stub).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types.
 *   - every function returns int: 0 = SATCV_OK, <0 = error; satcv_last_error()
 *     returns a thread-local message.
 *   - all tensor pointers are DEVICE pointers owned by the caller; the library
 *     never allocates or frees tensor memory and never synchronises the stream.
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous.
 *   - activations are NHWC (channels contiguous), storage type `dtype`
 *     (SATCV_F32 or SATCV_BF16), channel counts padded to a multiple of 16.
 *     Accumulation, BN statistics, losses, gradients of weights and the
 *     optimizer are always fp32.
 */
#ifndef SATCV_H
#define SATCV_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Per-channel statistics rows (BatchNorm forward sum / sum-of-squares, backward sum g / sum g*xhat) are accumulated in DOUBLE:
 * the replica rows are filled with atomics whose order varies from run to run, and fp32 rounding differences in the resulting
 * scale/shift flip ReLU masks (a batch-64 U-Net's gradient moved by 2e-3 between two runs on the same batch).  In double the
 * order only matters at 1e-16, so the fp32 quantities derived from the rows are reproducible. */
typedef double satcv_stat_t;

enum { SATCV_OK = 0, SATCV_ERR_INVALID = -1, SATCV_ERR_HIP = -2, SATCV_ERR_UNSUPPORTED = -3 };
enum { SATCV_F32 = 0, SATCV_BF16 = 1,
       SATCV_FP8 = 2 /* OCP e4m3fn storage, inference only: ingest, pack_weights, conv2d_igemm (pipelined kernel), maxpool,
                        affine_requant, head_fwd */,
       SATCV_FP8X = 3 /* same NHWC e4m3 activations, but weights packed in 16-channel granules ([tap][K/16][Npad][16]) and
                         the convolution on the block-scaled K=64 MFMA (2x the bf16 rate); needs channels % 64 == 0.
                         Only pack_weights and conv2d_igemm take it. */,
       SATCV_F64 = 4 /* the statistics rows (satcv_stat_t); only satcv_allreduce takes it */ };
/* rows of replicated per-channel accumulators (sum rows in order to consume) */
#define SATCV_STAT_ROWS 32

const char* satcv_version(void);
const char* satcv_last_error(void);
/* out[0]=CU count, out[1]=LDS bytes/CU, out[2]=wave size, out[3]=gfx arch number (950) */
int satcv_device_info(int32_t* out4);

/* ---------------------------------------------------------------- data movement
 * f32 NHWC (n,h,w,c) -> dtype NHWC (n,h,w,cpad), zero-filling channels [c,cpad).
 * Replaces the implicit float32 feed of Model.predict/fit (utils/prediction_tools.py:152). */
int satcv_ingest_nhwc(const float* src, void* dst, int64_t npix, int32_t c, int32_t cpad,
                      int32_t dtype, void* stream);
/* same with a multiplier (the fp8 path feeds x/q_in so that the reflectances use the upper e4m3 range) */
int satcv_ingest_nhwc_scaled(const float* src, void* dst, int64_t npix, int32_t c, int32_t cpad, float mul, int32_t dtype, void* stream);
/* planar CHW (c,h,w) per tile, any of u8/u16/f32 (src_kind 0/1/2), scaled by `scale`
 * -> dtype NHWC (n,h,w,cpad): (float)value * scale in float32, then the storage rounding; channels [c,cpad) zero.  dtype SATCV_F32 or
 * SATCV_BF16.  Mirrors the CHW->HWC + rescale of utils/processing.py:544-613.  Refused: null pointers, n, c, h or w <= 0, cpad < c,
 * cpad % 8 != 0, another src_kind or dtype. */
int satcv_ingest_chw(const void* src, int32_t src_kind, float scale, void* dst, int32_t n,
                     int32_t c, int32_t h, int32_t w, int32_t cpad, int32_t dtype, void* stream);

/* Keras HWIO fp32 master kernel (kh,kw,cin,cout) -> packed operand images.
 *   fwd   : [kh*kw][cin_pad/8][cout_pad][8]   (B operand of the forward implicit GEMM)
 *   dgrad : [kh*kw][cout_pad8/8][cin_pad32][8] spatially flipped, in/out swapped
 * transposed=1: source is a Conv2DTranspose kernel (kh,kw,cout,cin) (utils/model_tools.py:306);
 *   fwd   : [1][cin_pad/8][kh*kw*cout][8]  (N index = (i*kw+j)*cout + o)
 *   dgrad : [1][kh*kw*cout/8][cin_pad32][8] (K index = (i*kw+j)*cout + o)
 * Either destination may be NULL.  Every element outside the kernel's (k, n) range is written as +0; dtype SATCV_F32, SATCV_BF16,
 * SATCV_FP8 (saturating round-to-nearest-even) or SATCV_FP8X (forward image only, 16-element granules [tap][K/16][Npad][16]).
 * Refused: a null src; kh, kw, cin or cout <= 0; cin_pad < cin or cin_pad % 16 != 0; SATCV_FP8X with a dgrad destination or without a
 * forward one; another dtype. */
int satcv_pack_weights(const float* src, void* dst_fwd, void* dst_dgrad, int32_t kh, int32_t kw,
                       int32_t cin, int32_t cout, int32_t cin_pad, int32_t transposed,
                       int32_t dtype, void* stream);
/* All layers in one launch: a DEVICE array of jobs (mode 0 conv fwd, 1 conv dgrad, 2 transposed-conv fwd, 3 transposed-conv dgrad;
 * kpad / npad = K and N paddings of the image exactly as satcv_pack_weights derives them) and the exclusive prefix sum of
 * satcv_pack_job_items() over the jobs.  satcv_pack_job_items() is the job's number of 16-byte output items ROUNDED UP TO 256: a block of
 * 256 consecutive items then belongs to one job and the kernel looks its job up once per block; total_items must be the sum of those values
 * (SATCV_ERR_INVALID otherwise).  satcv_pack_job_items() returns -1 for a null job, a mode outside 0..3, kpad <= 0 or kpad % 8 != 0,
 * npad <= 0, or taps, cin or cout <= 0. */
typedef struct { const float* src; void* dst; int32_t mode, taps, cin, cout, kpad, npad; } satcv_pack_job;
int64_t satcv_pack_job_items(const satcv_pack_job* job);
int satcv_pack_weights_batched(const satcv_pack_job* jobs_dev, const int64_t* prefix_dev, int32_t njobs, int64_t total_items, int32_t dtype,
                               void* stream);

/* ------------------------------------------------------------ implicit-GEMM conv
 * One descriptor drives Conv2D forward, its data gradient, Conv2DTranspose(k==s)
 * forward (depth-to-space store) and its data gradient (space-to-depth load).
 * Replaces layers.Conv2D (utils/model_tools.py:178,312,315,405,544-549) and
 * layers.Conv2DTranspose (:306), plus the input-side BatchNormalization+ReLU of the
 * PREVIOUS layer (:179-180, :308-309) which is applied while staging the tile. */
typedef struct satcv_conv_desc {
  const void* x0;          /* source 0, NHWC (n, hin, win, c0)                       */
  const void* x1;          /* optional source 1 (concat along channels), or NULL      */
  int32_t c0, c1;          /* channels of each source (multiples of 16); K = c0+c1     */
  const float* in_scale;   /* optional per-input-channel affine (+ReLU) applied on load */
  const float* in_shift;
  int32_t in_relu;
  const void* w;           /* packed weights (satcv_pack_weights)                     */
  const float* bias;       /* [cstat] or NULL                                         */
  void* y;                 /* output NHWC, channel stride ldy                         */
  int32_t ldy;
  satcv_stat_t* stats;     /* optional [SATCV_STAT_ROWS][2][stats_ld] sum / sum-of-squares
                              of the stored outputs (atomically accumulated)          */
  int32_t stats_ld;
  int32_t n, h, w_;        /* GEMM pixel grid (= output grid, or input grid for mode_out=1) */
  int32_t cout;            /* GEMM N extent (valid columns)                           */
  int32_t cout_pad;        /* N stride of the packed weights                          */
  int32_t kh, kw, dil;     /* taps and dilation ('same' zero padding)                 */
  int32_t mode_in;         /* 0: plain; 1: space-to-depth gather by factor f          */
  int32_t mode_out;        /* 0: plain; 1: depth-to-space scatter by factor f         */
  int32_t f;
  int32_t cstat;           /* modulus mapping N index -> bias/stats channel            */
  int32_t out_relu;        /* clamp outputs at 0 before storing                        */
  int32_t dtype;
  int32_t accumulate;      /* 1: y += result instead of y = result (fan-out of a tensor into several convs);
                            * 2: y = ReLU(y + result), the result rounded to the storage type first (residual join written in place
                            *    over the shortcut; inference) */
  /* strided convolution (ResNet-style, symmetric zero padding dil*(k-1)/2): output grid (n,h,w_), input grid
   * (n,hin,win) with h = (hin-1)/stride+1.  stride 0/1 = dense.  Generic kernel only. */
  int32_t stride, hin, win;
  /* optional per-channel multiplier of the accumulator (indexed like bias): y = act(acc*out_scale + bias).  The folded
   * inference path puts BatchNorm and the fp8 quantisation scales here (q_in*w_scale*bn_scale/q_out). */
  const float* out_scale;
  /* optional fused max-pool (window == stride == pool_f, 'valid') of the STORED outputs, written to pool_y with channel stride
   * pool_ld: layers.MaxPooling2D (utils/model_tools.py:281) of an encoder block in the folded inference graph.  Pipelined kernel
   * only (satcv_conv2d_igemm_pipelined), mode_out 0, h and w_ divisible by pool_f. */
  void* pool_y; int32_t pool_ld, pool_f;
  /* optional: the REDUCE pass of the BatchNormalization backward (satcv_bn_bwd_reduce, utils/model_tools.py:179-180 differentiated) of
   * the layer whose activation gradient this launch writes (the launch is a data gradient: y = dL/d act), done in the epilogue while
   * the tile is on chip.  With bst_y set, `stats` receives  sum g  and  sum g * xhat  in the layout satcv_bn_bwd_finalize reads
   * (instead of sum / sum of squares), where g = y as stored, zeroed where bst_scale*v + bst_shift <= 0 (unless bst_relu == 0),
   * xhat = (v - bst_mean) * bst_rstd and v = that layer's raw convolution output at the same pixel and channel: bst_y (channel
   * stride bst_ld) for channels < bst_split, bst_y1 (stride bst_ld1, channel - bst_split) above it -- bst_y1 NULL: one source.
   * Pipelined kernel, bf16, plain output mode, no accumulate / out_relu / pool_y, and only when the map is a whole number of the
   * kernel's tiles: satcv_conv2d_igemm_pipelined() answers 0 otherwise and the caller keeps the separate reduce launch. */
  const void* bst_y; const void* bst_y1; int32_t bst_ld, bst_ld1, bst_split;
  const float* bst_scale; const float* bst_shift; const float* bst_mean; const float* bst_rstd; int32_t bst_relu;
  /* which tile family may serve this launch: 0 = the library option igemm_m16 decides (default 1: the 16x16x32 tiles only for launches that
   * write statistics, so that inference results are bit-identical across batch splits); 2 = every eligible launch may run on the 16x16x32 /
   * persistent tiles, whose choice depends on the launch's tile count -- what a TRAINING plan asks for, per launch (round 6: this used to be
   * a process-global option toggled around the plan's steps).  Option igemm_m16 = 0 (SATCV_M16=0) still turns those tiles off. */
  int32_t tile_policy;
  /* optional "pair store" (inference only): the two dates of a Siamese U-Net's shared encoder / ASPP layer run as ONE launch of
   * n = 2 * pair_n images, and the channel concatenations concat([enc_b, enc_a]) / concat([aspp_b, aspp_a]) (utils/model_tools.py:608,
   * 613, 624) become an address remap of the store: GEMM image i < pair_n (date a) goes to image i of y at channel offset pair_c0,
   * image i >= pair_n (date b) to image i - pair_n at channel offset pair_c1; y is (pair_n, h, w_, ldy).  A fused max-pool (pool_y)
   * is NOT remapped: it stays (2 * pair_n, h / pool_f, w_ / pool_f, pool_ld), the next shared encoder level's input.  pair_n = 0: off.
   * Pipelined kernels only (satcv_conv2d_igemm_pipelined), no mode_out / accumulate / stats / bst_y, both offsets + cout within ldy
   * and multiples of one 16-byte store vector. */
  int32_t pair_n, pair_c0, pair_c1;
} satcv_conv_desc;
int satcv_conv2d_igemm(const satcv_conv_desc* d, void* stream);
/* 1 if this descriptor runs on the pipelined kernel (required by out_scale / pool_y / the fp8 dtypes), else 0; no launch. */
int satcv_conv2d_igemm_pipelined(const satcv_conv_desc* d);

/* Which kernel form satcv_conv2d_igemm(d) would run under the current options: host only, nothing is launched and no device is touched
 * when ncu > 0 (x0 / x1 / w / y may be null: a null one counts as present and 16-byte aligned; of the others only presence and 16-byte
 * alignment are read).  The query and the launch run the SAME function (igemm_dispatch, conv_igemm.hip), centre-tap rewrite, LDS- and
 * register-fit tests included, so the answer cannot drift from what runs.  ncu: the CU count the persistent kernels size their grids by
 * and the persistent 16x16x32 kernel decides on; 0 asks the device, as a launch does.
 * family says which fields are meaningful:
 *   FAST     igemm_fast_kernel<T, tw, wm, wn, mt, nt, ks, taps, dyn, tl, db, wps, wdma, sk, m16>   (conv_igemm_fast.hip)
 *   GENERIC  igemm_kernel<T, tw, wm, wn, mt, nt, ks>                                               (conv_igemm.hip)
 *   M16      igemm_m16_kernel<tw> (roles = 1) / igemm_m16sym_kernel<tw> (roles = 0); bst: the launch carries the fused sums
 *   M16P     igemm_m16p_kernel<bst, bn>
 *   WS       igemm_ws_kernel<T, cin, nt, wps, wn, dil>
 *   TR       igemm_tr_kernel<cin, cout, th>
 *   CONVT_THIN / CONVT_THIN_DGRAD   convt_thin_kernel<cin, cout, nw, wps, nsplit> / convt_thin_dgrad_kernel<cin, cout, nw, wps>
 * Geometry: imgs images of rpi rows per tile, tiles_x x tiles_y pixel tiles per image group, n_tiles column tiles, nchunks K chunks,
 * ksplit K ranges (split-K, else 1), workgroups of the launch (split-K: of its main kernel), lds_bytes dynamic LDS per workgroup. */
enum { SATCV_CONV_FAMILY_GENERIC = 0, SATCV_CONV_FAMILY_FAST = 1, SATCV_CONV_FAMILY_M16 = 2, SATCV_CONV_FAMILY_M16P = 3, SATCV_CONV_FAMILY_WS = 4,
       SATCV_CONV_FAMILY_TR = 5, SATCV_CONV_FAMILY_CONVT_THIN = 6, SATCV_CONV_FAMILY_CONVT_THIN_DGRAD = 7 };
typedef struct satcv_conv_plan_info {
  int32_t family, dtype;
  int32_t tw, wm, wn, mt, nt, ks, taps, tl, db, wps, wdma, sk, m16, dyn;
  int32_t cin, cout, th, nw, nsplit, dil;      /* WS / TR / CONVT_THIN*: the per-family template arguments */
  int32_t bn, roles, bst;                      /* M16 / M16P */
  int32_t imgs, rpi, tiles_x, tiles_y, n_tiles, nchunks, ksplit;
  int32_t centre_tap;                          /* 1: a strongly dilated 3x3 (dil >= h and w_) runs as the 1x1 conv of its centre tap */
  int64_t workgroups, lds_bytes;
} satcv_conv_plan_info;
int satcv_conv2d_igemm_plan_info(const satcv_conv_desc* d, int32_t ncu, satcv_conv_plan_info* info);

/* Weight gradient of the same convolutions: dW[tap][ci][co] = sum_p X[p+tap][ci]*dY[p][co],
 * written as Keras HWIO fp32.  X is staged with the same optional affine+ReLU as the
 * forward.  Needs a caller-provided fp32 workspace (satcv_conv2d_wgrad_workspace). */
typedef struct satcv_wgrad_desc {
  const void* x0; const void* x1; int32_t c0, c1;
  const float* in_scale; const float* in_shift; int32_t in_relu;
  const void* dy; int32_t lddy;      /* (n, h*f, w*f, lddy) when mode_dy=1 else (n,h,w,lddy) */
  float* dw;                         /* (kh,kw,cin,cout) fp32, or (f,f,cout,cin) when transposed */
  int32_t cin, cout;                 /* real (unpadded) extents written to dw */
  int32_t n, h, w_;
  int32_t kh, kw, dil;
  int32_t mode_dy;                   /* 1: dy is gathered space-to-depth by f (Conv2DTranspose) */
  int32_t f;
  int32_t transposed;                /* dw layout (f,f,cout,cin) */
  float* workspace; int64_t workspace_bytes;
  int32_t dtype;
  int32_t accumulate;                /* dw += result (a layer applied to several inputs: shared weights) */
  int32_t whole_chip;                /* 1: nothing runs beside this launch (the last weight gradient of a backward pass): one workgroup
                                        per CU instead of the 160 that leave room for the other stream's kernels */
  int32_t defer_reduce;              /* 1: the launch only writes its fp32 partial slabs to `workspace` (which then belongs to this layer
                                        until the sum has run); the caller sums them later, many layers per launch:
                                        satcv_conv2d_wgrad_reduce_job + satcv_reduce_slabs_batched.  Plain 1x1 / 3x3 path only. */
} satcv_wgrad_desc;
int64_t satcv_conv2d_wgrad_workspace(const satcv_wgrad_desc* d);
int satcv_conv2d_wgrad(const satcv_wgrad_desc* d, void* stream);

/* Which kernel form satcv_conv2d_wgrad(d) would run under the current options: host only, nothing is launched and no device is
 * touched (the pointers of `d` may be null; their 16-byte alignment is all the plan reads of them).  The query walks the launch path's
 * own decision chain, LDS-fit tests included, so it cannot drift from what runs.  Fields are the template arguments of the chosen
 * instantiation (nks, pix, nw: of the kernel, not of the slab plan) and the slab geometry; on the per-tap path of strongly dilated 3x3
 * layers (per_tap = 1) they describe each of the nine shifted 1x1 launches and their slab sums.  ws_bytes = nsplit * ntaps * kpad *
 * npad * 4 of the described launch (satcv_conv2d_wgrad_workspace is the larger of that and the per-tap plan's). */
enum { SATCV_WGRAD_KERNEL_SINGLE = 0, SATCV_WGRAD_KERNEL_DB = 1, SATCV_WGRAD_KERNEL_DMA = 2 };       /* wgrad_kernel, wgrad_db_kernel, wgrad_dma_kernel */
enum { SATCV_WGRAD_REDUCE_GENERIC = 0, SATCV_WGRAD_REDUCE_4 = 1, SATCV_WGRAD_REDUCE_16 = 2 };          /* wgrad_reduce_kernel, ..4_kernel, ..16_kernel */
typedef struct satcv_wgrad_plan_info {
  int32_t kernel;                    /* SATCV_WGRAD_KERNEL_* */
  int32_t tw, nci, nco, nw, nks, ntaps, pix;
  int32_t db, dma, m16;              /* double-buffered template (db or dma kernel); LDS-DMA kernel; its 16x16x32 variant */
  int32_t nsplit, kpad, npad, n_ci_blk, n_co_blk;
  int32_t reduce;                    /* SATCV_WGRAD_REDUCE_*: the slab sum a launch without defer_reduce ends in */
  int32_t per_tap;                   /* 1: nine shifted 1x1 launches (the 3x3 halo tile does not fit the LDS) */
  int64_t ws_bytes, lds_bytes;
} satcv_wgrad_plan_info;
int satcv_conv2d_wgrad_plan_info(const satcv_wgrad_desc* d, satcv_wgrad_plan_info* info);

/* Deferred, batched slab sum (round 5).  Every weight-gradient launch ends in an ordered sum of its workgroups' fp32 partial slabs into the
 * Keras-layout gradient -- a launch of 5-30 us per layer, 21 per training step.  With defer_reduce the producers skip it; the caller
 * collects one job per layer (the slab geometry the library chose), keeps the layers' workspaces apart, and runs ONE launch over a DEVICE
 * array of jobs + the exclusive prefix sum of satcv_reduce_job_items().  The summation order is fixed (a job's `lanes` partial sums over
 * slabs l, l + lanes, ..., combined in increasing lane order): results are bit-reproducible.  satcv_reduce_job_items() is the job's item
 * count ROUNDED UP TO 16, so that every prefix is a multiple of 16 and a lane group never straddles a wavefront; total_items must be the sum
 * of those values (SATCV_ERR_INVALID otherwise). */
typedef struct satcv_reduce_job {
  const float* ws; float* dw;
  int32_t nslab, taps, kpad, npad, cin, nvalid, transposed, accumulate, lanes, pad_;
} satcv_reduce_job;
int satcv_conv2d_wgrad_reduce_job(const satcv_wgrad_desc* d, satcv_reduce_job* job);      /* the sum satcv_conv2d_wgrad(d) deferred */
int64_t satcv_reduce_job_items(const satcv_reduce_job* job);
int satcv_reduce_slabs_batched(const satcv_reduce_job* jobs_dev, const int64_t* prefix_dev, int32_t njobs, int64_t total_items, void* stream);

/* Fused backward of a thin conv -> BatchNormalization -> ReLU block (conv_batch_act, utils/model_tools.py:174-186; Keras autodiff of
 * Conv2D :178 + BatchNormalization :179 + Activation :180 inside Model.fit): ONE launch replaces satcv_bn_bwd_apply + the data-gradient
 * satcv_conv2d_igemm + satcv_conv2d_wgrad of the layer.  dy = scale * (g * [scale*y+shift > 0] - c1 - xhat * c2) is formed in
 * registers from g (gradient w.r.t. the activated output) and yraw (the conv's stored output) with coef = [c1 | c2] from
 * satcv_bn_bwd_finalize, never written to memory, and used for both products:
 *     dx (n, h, w, lddx)  = conv3x3(dy, w_dgrad)           w_dgrad: the data-gradient operand image of satcv_pack_weights
 *     dw (3, 3, cin, cout) [+]= sum_pixels x (x) dy        x = x0 (| x1) with the optional in_scale / in_shift / in_relu of the forward
 * Limits (else satcv_conv2d_bwd_fused_workspace returns -1 and the caller keeps the three launches): bf16, 3x3, dilation 1, stored input
 * channels c0 + c1 = cin in {32, 64} with cout 32, or 64 with cout 64, maps of whole 8 x 32 tiles (h % 8 == 0, w_ % 32 == 0), g and yraw
 * with the same channel stride ldg.  workspace: fp32 partial sums, one slab per resident workgroup (size from the query). */
typedef struct satcv_bwdf_desc {
  const void* g; const void* yraw; int32_t ldg;
  const float* bn_scale; const float* bn_shift; const float* bn_mean; const float* bn_rstd;
  const float* bn_coef;                /* [2][cout] */
  int32_t linear;                      /* 1: BatchNormalization without ReLU (no mask) */
  const void* x0; const void* x1; int32_t c0, c1;
  const float* in_scale; const float* in_shift; int32_t in_relu;
  const void* w_dgrad;
  void* dx; int32_t lddx;
  float* dw; int32_t cin, cout;
  int32_t n, h, w_;
  int32_t kh, kw, dil;
  float* workspace; int64_t workspace_bytes;
  int32_t dtype;
  int32_t accumulate;                  /* dw += result (shared weights) */
  /* optional: the sums of the BatchNorm backward of the layer BELOW -- the BatchNormalization + ReLU whose scale / shift are this
   * launch's in_scale / in_shift (needs in_relu = 1) -- formed from the stored dx and the staged input: what satcv_bn_bwd_reduce would
   * compute in a pass of its own over dx and that layer's raw output.  [ROWS][2][bst_sums_ld] rows as for satcv_bn_bwd_finalize.
   * The sums are ADDED to the rows (one atomic add per channel and workgroup): the caller zeroes them, or keeps what other launches
   * put there.  xhat is rebuilt from the staged activation a = relu(in_scale * x + in_shift) as (a - in_shift) / in_scale: a channel
   * whose in_scale is exactly 0 gets sum g xhat = 0, because xhat cannot be rebuilt from a constant activation. */
  satcv_stat_t* bst_sums; int32_t bst_sums_ld;
  const float* bst_mean; const float* bst_rstd;
  int32_t bst_act_form;                /* 1: the input x is itself an activation (in_scale NULL: a max-pooled encoder output); the rows get
                                          sum dx [x > 0], sum dx x for satcv_bn_bwd_finalize2 */
  /* optional, encoder_block (utils/model_tools.py:262-286): the block's activated output is ALSO max-pooled 2 x 2 -- g is the gradient
   * of the skip, dpool (n, h/2, w/2, lddp) the gradient of MaxPooling2D's output and amax the arg-max bytes satcv_bn_relu_pool_amax
   * wrote: the launch uses g + (amax == position in the window ? dpool : 0).  Limits: 32 -> 64 channels; or 16 stored channels -> 32
   * with dx == NULL (the first block: fed by the model input, no data gradient). */
  const void* dpool; int32_t lddp; const void* amax;
  /* optional, the block under the 1 x 1 head (utils/model_tools.py:405): g is not read -- it is formed in the loader as
   * g[p][c] = bf16(dlogits[p][0] w[c][0] + dlogits[p][1] w[c][1]), what satcv_head_bwd would have stored as dx (pass dx = NULL there).
   * hg_dlogits (npix, 2) fp32, hg_w the head's Keras kernel (cout, 2) fp32, hg_ncls == 2; 32 -> 32 channels only. */
  const float* hg_dlogits; const float* hg_w; int32_t hg_ncls;
  int32_t defer_reduce;                /* 1: leave the weight-gradient slabs in `workspace` (satcv_conv2d_bwd_fused_reduce_job describes the
                                          deferred sum for satcv_reduce_slabs_batched) */
} satcv_bwdf_desc;
int64_t satcv_conv2d_bwd_fused_workspace(const satcv_bwdf_desc* d);
int satcv_conv2d_bwd_fused(const satcv_bwdf_desc* d, void* stream);
int satcv_conv2d_bwd_fused_reduce_job(const satcv_bwdf_desc* d, satcv_reduce_job* job);

/* Which instantiation satcv_conv2d_bwd_fused(d) would run, and how its persistent workgroups share the tiles: host only, nothing is
 * launched.  ncu > 0 plans for that CU count and does not touch the HIP runtime; ncu == 0 asks the device, as the launch does.  The
 * query walks the launch path's own chain (bwdf_shape_ok -> bwdf_dispatch -> bwdf_launch of csrc/conv_bwd_fused.hip), so it cannot drift
 * from what runs; pointers are read for null-ness and alignment only.  Fields: the template arguments of
 * bwd_fused_kernel<cin, cout, nw, wps, pool, nodg, cins, hg>; bst = 1 where that instantiation carries the fused sums; tiles of 8 x 32
 * pixels; workgroups of the launch, each with a contiguous range of tiles_min or tiles_max (= tiles_min + 1 where the division leaves
 * a remainder) tiles; dynamic LDS per workgroup; ws_bytes = workgroups * 9 * cin * cout * 4, what satcv_conv2d_bwd_fused_workspace
 * answers.  SATCV_ERR_UNSUPPORTED where the workspace query answers -1. */
typedef struct satcv_bwdf_plan_info {
  int32_t cin, cout, nw, wps, pool, nodg, cins, hg;
  int32_t bst, pad_;
  int64_t tiles, workgroups, tiles_min, tiles_max, lds_bytes, ws_bytes;
} satcv_bwdf_plan_info;
int satcv_conv2d_bwd_fused_plan_info(const satcv_bwdf_desc* d, int32_t ncu, satcv_bwdf_plan_info* info);

/* Fused backward of decoder_block's up-sampling path (utils/model_tools.py:306-309: Conv2DTranspose(filters, up_size, strides = up_size) ->
 * concatenate([skip, up]) -> BatchNormalization -> Activation('relu'), differentiated by Keras inside Model.fit), round 5.  For the `up`
 * channels of the concatenation ONE launch replaces satcv_bn_bwd_apply (their half) + the space-to-depth data gradient + the weight gradient:
 *     dup = scale * (g * [scale*yup+shift > 0] - c1 - xhat * c2)   in registers, never stored (g = gradient of the activated concatenation,
 *           its `up` channels; yup = the transposed convolution's stored output; c1, c2 from satcv_bn_bwd_finalize of the concatenation)
 *     dx (n, h, w, lddx)        = sum_{ij, co} dup[(2y+i, 2x+j)][co] K[i][j][co][ci]      w_dgrad: the data-gradient image of satcv_pack_weights(transposed)
 *     dw (2, 2, cout, cin) fp32 = sum_pixels dup x^T                                       (Keras Conv2DTranspose kernel layout)
 * and, with bst_sums, the sums of the BatchNorm backward of the layer whose output x is (as satcv_conv2d_bwd_fused does).  The bias gradient
 * of the transposed convolution is identically zero under the BatchNormalization that follows it.  bf16, f = 2, cout 32 / 64, cin a
 * multiple of 64, rows of w a multiple of 64 / 32 pixels: satcv_convt_bwd_fused_workspace() answers -1 otherwise and the caller keeps the
 * three launches.  The `skip` channels keep satcv_bn_bwd_apply (c = their count). */
typedef struct satcv_ctbf_desc {
  const void* g; int32_t ldg;            /* (n, 2h, 2w, ldg), already offset to the first `up` channel */
  const void* yup; int32_t ldy;          /* (n, 2h, 2w, ldy) */
  const float* bn_scale; const float* bn_shift; const float* bn_mean; const float* bn_rstd;   /* [cout], of the `up` channels */
  const float* bn_c1; const float* bn_c2; int32_t linear;
  const void* x; int32_t ldx;            /* (n, h, w, ldx): the transposed convolution's input, with its pending BatchNorm + ReLU */
  const float* in_scale; const float* in_shift; int32_t in_relu;
  const void* w_dgrad; int32_t w_npad;   /* [4 cout / 8][w_npad][8] */
  void* dx; int32_t lddx;
  float* dw; int32_t cin, cout;
  int32_t n, h, w_, f;                   /* INPUT grid; f = 2 */
  float* workspace; int64_t workspace_bytes;
  int32_t dtype, accumulate, defer_reduce;
  satcv_stat_t* bst_sums; int32_t bst_sums_ld; const float* bst_mean; const float* bst_rstd;
} satcv_ctbf_desc;
int64_t satcv_convt_bwd_fused_workspace(const satcv_ctbf_desc* d);
int satcv_convt_bwd_fused(const satcv_ctbf_desc* d, void* stream);
int satcv_convt_bwd_fused_reduce_job(const satcv_ctbf_desc* d, satcv_reduce_job* job);

/* The same question for satcv_convt_bwd_fused (ctbf_dispatch -> ctbf_launch of csrc/convt_bwd_fused.hip): the template arguments of
 * convt_bwd_fused_kernel<cout4, px, cblk> (4 cout gradient channels, px input pixels per tile, cblk input channels per workgroup), nblk =
 * cin / cblk channel blocks, `slabs` workgroups per channel block (slabs * nblk workgroups in all), tiles of px pixels, tiles_min /
 * tiles_max per slab, dynamic LDS, ws_bytes = slabs * cin * 4 cout * 4.  bst_sums, accumulate and defer_reduce are bound to the descriptor
 * as for satcv_conv2d_bwd_fused: the sums are added to the rows, and a zero in_scale gives sum g xhat = 0. */
typedef struct satcv_ctbf_plan_info {
  int32_t cout4, px, cblk, nblk;
  int64_t slabs, tiles, tiles_min, tiles_max, lds_bytes, ws_bytes;
} satcv_ctbf_plan_info;
int satcv_convt_bwd_fused_plan_info(const satcv_ctbf_desc* d, int32_t ncu, satcv_ctbf_plan_info* info);

/* --------------------------------------------------------------- batch norm
 * layers.BatchNormalization (utils/model_tools.py:179,308,313,316): eps, momentum as given.
 * Training: consume the [ROWS][2][ld] sum/sumsq rows (and zero them), produce per-channel
 * scale=gamma*rstd, shift=beta-mean*scale, mean, rstd, and update the moving statistics
 * `updates` times (2 reproduces the double cba1 call of conv_block.call, :238-239). */
int satcv_bn_finalize_train(satcv_stat_t* stats, int32_t stats_ld, int32_t c, float count,
                            const float* gamma, const float* beta, float eps, float momentum,
                            int32_t updates, int32_t bessel, float* moving_mean, float* moving_var,
                            float* scale, float* shift, float* mean, float* rstd, void* stream);
/* Inference: scale/shift from the moving statistics. */
int satcv_bn_affine_infer(const float* gamma, const float* beta, const float* moving_mean,
                          const float* moving_var, float eps, int32_t c, float* scale, float* shift,
                          void* stream);
/* The same for every BatchNormalization of an inference plan in one launch: `jobs_device` is a DEVICE array of njobs entries. */
typedef struct satcv_bn_affine_job {
  const float* gamma; const float* beta; const float* moving_mean; const float* moving_var;
  float* scale; float* shift; int64_t c;
  /* optional (NULL: not written): bias_eff = scale * conv_bias + shift -- the additive term of a convolution whose epilogue applies
   * its own inference BatchNormalization (out_scale = scale, bias = bias_eff), as the residual joins of the ResNet backbone do */
  const float* conv_bias; float* bias_eff;
} satcv_bn_affine_job;
int satcv_bn_affine_infer_batched(const satcv_bn_affine_job* jobs_device, int32_t njobs, float eps, void* stream);

/* act = relu(scale*yraw+shift) (written if act != NULL), pooled = maxpool_f(act) ('valid'),
 * optional sum/sumsq rows of `act` (feeds the decoder's concat BatchNormalization).
 * act_ld (<= 0: c) and, with stats, stats_ld must be >= c.
 * Replaces Activation('relu') + MaxPooling2D (utils/model_tools.py:180,281). */
int satcv_bn_relu_pool(const void* yraw, const float* scale, const float* shift, void* act, int32_t act_ld,
                       void* pooled, satcv_stat_t* stats, int32_t stats_ld, int32_t n, int32_t h,
                       int32_t w_, int32_t c, int32_t f, int32_t dtype, void* stream);
/* the same, also writing amax (n, h/f, w/f, c) bytes: the position i * f + j of every window's first maximum (what the backward of
 * MaxPooling2D routes the gradient to) -- read by the pooled form of satcv_conv2d_bwd_fused instead of re-scanning the windows */
int satcv_bn_relu_pool_amax(const void* yraw, const float* scale, const float* shift, void* act, int32_t act_ld,
                            void* pooled, void* amax, satcv_stat_t* stats, int32_t stats_ld, int32_t n, int32_t h,
                            int32_t w_, int32_t c, int32_t f, int32_t dtype, void* stream);

/* Backward of  a = relu(scale*y+shift)  (training-mode BN):
 *   g  = (da [+ unpool(dpool)]) * (a > 0)
 *   reduce : sums[row][0][ch] += g ; sums[row][1][ch] += g * xhat
 *   finalize: dbeta=sum g, dgamma=sum g*xhat -> grads, coef (c1=dbeta/M, c2=dgamma/M), zero sums
 *   apply  : dy = scale*(g - c1 - xhat*c2)  (+ optional dbias[ch] += sum dy)            */
typedef struct satcv_bnbwd_desc {
  const void* da; int32_t ldda;        /* grad w.r.t. activation, may be NULL if only dpool */
  const void* dpool; int32_t lddp;     /* optional grad of maxpool_f(a), (n,h/f,w/f,lddp)   */
  int32_t f;
  const void* yraw; int32_t ldy;
  const float* scale; const float* shift; const float* mean; const float* rstd;
  satcv_stat_t* sums; int32_t sums_ld; /* [ROWS][2][sums_ld]                                */
  const float* coef;                   /* [2][c] from finalize (apply only)                 */
  void* dy; int32_t lddy_out;          /* apply output                                      */
  float* dbias;                        /* optional [c], atomically accumulated (apply)      */
  int32_t n, h, w_, c;
  int32_t dtype;
  int32_t linear;                      /* 1: BatchNormalization without the ReLU (residual branch): g = da, no mask   */
  /* optional second source (c_split > 0): the BatchNormalization of concat([skip, up]) (utils/model_tools.py:307-308) in ONE pass
   * over the gradient `da` of the concatenation -- channels [0, c_split) are read from yraw / written to dy as above, channels
   * [c_split, c) from yraw1 (stride ldy1) / to dy1 (stride lddy1).  Dense form only (no dpool, no dbias).  satcv_bn_bwd_apply with
   * dy1 == NULL applies the first c_split channels only (the others' gradient is formed by satcv_convt_bwd_fused in its loader).   */
  const void* yraw1; int32_t ldy1;
  void* dy1; int32_t lddy1;
  int32_t c_split;
  /* optional (apply pass of the two-source form): the first source is the ACTIVATED output a = relu(BN(y_enc)) of an encoder block
   * (the skip of decoder_block, utils/model_tools.py:307) and dy its gradient: also accumulate the sums of THAT BatchNorm's backward
   * in the activated form -- rows [0]: sum dy [a > 0], rows [1]: sum dy a over the c_split skip channels -- which
   * satcv_bn_bwd_finalize2 converts.  Saves the pass satcv_bn_bwd_reduce would make over dy and y_enc. */
  satcv_stat_t* sk_sums; int32_t sk_sums_ld;
} satcv_bnbwd_desc;
int satcv_bn_bwd_reduce(const satcv_bnbwd_desc* d, void* stream);
int satcv_bn_bwd_finalize(satcv_stat_t* sums, int32_t sums_ld, int32_t c, float count, float* dgamma,
                          float* dbeta, float* coef, int32_t accumulate, void* stream);
int satcv_bn_bwd_apply(const satcv_bnbwd_desc* d, void* stream);
/* finalize over two sets of rows: `sums` in the raw form satcv_bn_bwd_reduce writes (may be NULL), `act_sums` in the activated form
 * (sum g [a > 0], sum g a with a = relu(scale * y + shift)) written by producers that only see the activated tensor: the sk_sums of
 * satcv_bn_bwd_apply, a data-gradient launch whose bst_y is the max-pooled activation with unit bst_scale / bst_rstd and zero
 * bst_shift / bst_mean.  sum g xhat = (sum g a - (shift + scale mean) sum g) rstd / scale.  Zeroes both sets of rows. */
int satcv_bn_bwd_finalize2(satcv_stat_t* sums, int32_t sums_ld, satcv_stat_t* act_sums, int32_t act_sums_ld, int32_t c, float count,
                           const float* scale, const float* shift, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                           float* coef, int32_t accumulate, void* stream);

/* Residual blocks of the atrous CNN family (utils/model_tools.py:922-979: ReLU(BN(conv) + shortcut), plain Conv2D layers):
 * satcv_relu_bwd : g[i] = act[i] > 0 ? g[i] : 0 in place (gradient through the ReLU of a materialised activation; the masked
 *                  gradient then serves BOTH addends of the sum).
 * satcv_bias_grad: dbias[ch] += sum over pixels of dy[pix][ch] (a Conv2D that is not followed by BatchNormalization).  With
 *                  `partials` (satcv_bias_grad_workspace bytes) the workgroups write rows that a second launch adds in fixed order
 *                  (bit-reproducible); NULL: float atomics. */
int satcv_relu_bwd(const void* act, void* g, int64_t count, int32_t dtype, void* stream);
int64_t satcv_bias_grad_workspace(int64_t npix, int32_t c);
int satcv_bias_grad(const void* dy, int32_t lddy, int64_t npix, int32_t c, int32_t dtype, float* dbias, float* partials, void* stream);

/* ------------------------------------------ ResNet / DeepLab-v3 inference helpers
 * The reference has no DeepLab-v3/ResNet-50 code (README.md:8 only names it); these ops serve the build-defined
 * configuration of SURVEY.md section 8a row A9.
 * satcv_maxpool: window k, stride s, symmetric padding (ResNet stem 3x3/2).
 * satcv_add_act: out = relu?(affine?(y) + affine?(res)) -- the residual join of a bottleneck.
 * satcv_upsample_head: bilinear x factor (half-pixel centres) of fp32 logits + softmax/argmax or sigmoid/threshold.
 * (satcv_head_fwd with activation 2 writes the raw logits.) */
int satcv_maxpool(const void* x, void* out, int32_t n, int32_t h, int32_t w_, int32_t c, int32_t k, int32_t s,
                  int32_t pad, int32_t dtype, void* stream);
int satcv_add_act(const void* y, const float* y_scale, const float* y_shift, const void* res,
                  const float* res_scale, const float* res_shift, int32_t relu, void* out, int64_t npix,
                  int32_t c, int32_t dtype, void* stream);
/* out = Q(relu?(scale[c]*x + shift[c])) channel-wise between two NHWC tensors with their own channel strides; dtype_out is
 * dtype or SATCV_FP8 (or SATCV_BF16 from SATCV_FP8: where the hybrid fp8 graph hands a tensor to its bf16 levels).  Uses in the folded fp8 inference path: the skip half of concat([skip, up]) -> BN -> ReLU with the
 * requantisation q_skip/q_cat folded into scale/shift (utils/model_tools.py:307-309), and BN+ReLU+quantisation of the
 * first conv block, which is computed in bf16 because the e4m3 rounding of the INPUT bands costs the most accuracy. */
int satcv_affine_requant(const void* x, int32_t ldx, const float* scale, const float* shift, int32_t relu, void* out, int32_t ldo,
                         int64_t npix, int32_t c, int32_t dtype, int32_t dtype_out, void* stream);

int satcv_upsample_head(const float* logits, int32_t n, int32_t h, int32_t w_, int32_t ncls, int32_t factor,
                        int32_t activation, float thresh, float* probs, int32_t* classes, void* stream);

/* ---------------------------------------------------------------- dropout
 * layers.SpatialDropout2D / layers.Dropout (utils/model_tools.py:311, 351, 363, 402), training only.
 * satcv_dropout_mask: counter-based Bernoulli mask, values 0 or 1/(1-rate).
 * satcv_dropout_apply: out = act(x) * mask with act(x) = relu?(scale*x+shift) if scale else x;
 *   mask_mode 0: mask is (n, ldm) [whole feature maps dropped], 1: mask is (n*hw, ldm) [per element];
 *   ldm >= c lets a channel slice of a wider mask be applied.  With scale == NULL this is also the
 *   backward (g * mask). */
int satcv_dropout_mask(uint64_t seed, uint64_t offset, float rate, int64_t count, float* mask, void* stream);
int satcv_dropout_apply(const void* x, int32_t ldx, const float* scale, const float* shift, int32_t relu,
                        const float* mask, int32_t ldm, int32_t mask_mode, void* out, int32_t ldo, int32_t n,
                        int32_t hw, int32_t c, int32_t dtype, void* stream);

/* ------------------------------------------------------------------- head
 * Conv2D(ncls,(1,1),activation) + argmax/threshold (utils/model_tools.py:405-406, :660-661).
 * activation 0: softmax, classes = argmax (ties -> lowest index);
 *            1: sigmoid, classes = probs > thresh.
 * x is the raw output of the last decoder conv; its BN+ReLU is applied on load. */
typedef struct satcv_head_desc {
  const void* x; int32_t ldx; int32_t cin;
  const float* in_scale; const float* in_shift;
  const float* w;            /* fp32 (cin, ncls) = Keras (1,1,cin,ncls) */
  const float* b;            /* [ncls] */
  int32_t ncls; int32_t activation; float thresh;
  float* probs;              /* (npix, ncls) fp32 */
  int32_t* classes;          /* (npix) int32 */
  const float* dlogits;      /* bwd: (npix, ncls) fp32 */
  void* dx; int32_t lddx;    /* bwd: grad w.r.t. the activated input, storage dtype */
  float* dw; float* db;      /* bwd: fp32, atomically accumulated */
  /* bwd, optional: fused first pass of the BatchNorm+ReLU backward of x: with g = dx*(a>0), xhat = (x-mean)*rstd the kernel
   * accumulates per channel sum(g), sum(g*xhat) into bnr_sums ([SATCV_STAT_ROWS][2][bnr_sums_ld]) -- replaces
   * satcv_bn_bwd_reduce for that tensor (register-resident head kernel only) */
  const float* bnr_mean; const float* bnr_rstd; satcv_stat_t* bnr_sums; int32_t bnr_sums_ld;
  int64_t npix;
  int32_t dtype;
  /* bwd, optional: [satcv_head_bwd_workspace(d) bytes] -- every workgroup writes its dW / db partial sums here instead of adding
   * them to dw / db with float atomics; satcv_head_bwd_finalize then adds the rows in fixed order (bit-reproducible gradients) */
  float* partials;
} satcv_head_desc;
int satcv_head_fwd(const satcv_head_desc* d, void* stream);
int satcv_head_bwd(const satcv_head_desc* d, void* stream);
/* bytes of `partials` for this descriptor (0: shape outside the register-resident kernel, which then uses atomics) */
int64_t satcv_head_bwd_workspace(const satcv_head_desc* d);
int satcv_head_bwd_finalize(const satcv_head_desc* d, void* stream);

/* CRC-32C (Castagnoli) of a HOST buffer, continuing from crc_in (0 to start): the checksum of the TFRecord framing that
 * tf.io.TFRecordWriter / tf.data.TFRecordDataset use (utils/prediction_tools.py:221, 404; utils/processing.py:416). */
uint32_t satcv_crc32c(const void* data, uint64_t nbytes, uint32_t crc_in);

/* ------------------------------------------------------------------ tile input pipeline
 * Device version of UNETDataGenerator.__getitem__ (utils/processing.py:456-755) for one source / the labels of one batch.
 * src: planes (n, c, hin, win) of kind 0 u8, 1 u16, 2 f32, 3 i16, 4 f64, 5 i32, 6 i64 (what np.load returned).
 *   x / rescale (float64; 0 = none)                                     -- :551-552, 601, 613 (255 / 10000 / 100 / 2000)
 *   nan_mask: append the mask channel; with replace (to_fit) values that are NaN or < -5000 -- in this channel or an
 *   EARLIER one of the image, as coded -- become N(0,1) draws (counter RNG on seed) and the mask is 1     -- :553-583
 *   nan_mask == 2 (SiameseDataGenerator._get_unet_data, :797-805): mask channel = 1 where NO band of the pixel is NaN or
 *   below -1 after the rescale; NaN elements (only) become U[0,1) draws; the colour augmentation that follows takes its mean
 *   over the replaced values, as the reference does
 *   centre trim to (h, w_)                                                                                 -- :586-590
 *   ch_mean != NULL: (x - mean)*contra_mul + mean*bright_mul, mean = nanmean over (h, w_) per image and channel from
 *   satcv_tile_channel_mean                                             -- utils/array_tools.py:159-186
 *   flip_v, flip_h, rot (np.rot90 k) of the stacked batch               -- utils/array_tools.py:188-213, processing.py:748
 * dst: fp32 NHWC (n, ho, wo, ldc) written at channel offset coff (ho, wo = w_, h when rot is odd).
 * Arithmetic: float32 planes stay float32 (x / (float)rescale, (float)mean, (float) multipliers, every operation rounded on its own, as
 * NumPy does with Python scalars); every other kind is converted to double first.  The colour step is t1 = (v - mean) * contra_mul,
 * t2 = mean * bright_mul, t1 + t2, without contraction; the result is rounded to float32 once.  The centre trim starts at
 * (hin - h) / 2 and (win - w_) / 2, rounded down.
 * Draws: a counter generator keyed on the element's index idx in the SOURCE planes ((image * c + channel) * hin + y) * win + x, so a value
 * does not depend on the morph: r = splitmix64(seed ^ idx * 0xD1342543DE82EF95) (64-bit wrap-around);  U[0,1) = (r >> 11) * 2^-53;
 * N(0,1) = sqrt(-2 log u1) cos(6.283185307179586 u2) in double with u1 = ((r >> 32) + 1) / (2^32 + 1), u2 = (r & 0xffffffff) / 2^32.
 * satcv_tile_channel_mean sums in double and returns NaN for a channel without a valid value; in mode 2 it averages the very draws
 * that satcv_tile_ingest writes.
 * Refused (error code, satcv_last_error naming the entry point, nothing written): a null descriptor, src, dst or mean_out; n, c, h or
 * w_ <= 0; hin < h, win < w_; src_kind outside 0..6; rot outside 0..3; nan_mask outside 0..2; nan_mask 1 together with ch_mean;
 * coff < 0; ldc < coff + c (+ 1 with a mask channel). */
typedef struct {
  const void* src; int32_t src_kind;
  int32_t n, c, hin, win, h, w_;
  double rescale;
  int32_t nan_mask, replace;
  uint64_t seed;
  const double* ch_mean;
  double contra_mul, bright_mul;
  int32_t flip_v, flip_h, rot;
  float* dst; int32_t ldc, coff;
} satcv_tile_desc;
int satcv_tile_channel_mean(const satcv_tile_desc* d, double* mean_out /* (n, c) */, void* stream);
int satcv_tile_ingest(const satcv_tile_desc* d, void* stream);
/* labels (n, 1, hin, win) -> merge_classes (utils/array_tools.py:26-44) as 256-entry look-up tables (-1 = keep): lut on the
 * land-cover value, then lu_lut on the optional land-use array -> trim -> morph -> tf.one_hot(depth nclasses) fp32
 * (utils/processing.py:656-704).  The label value is truncated toward zero (.astype(int)); lut applies to values in [0, 256), lu_lut to
 * land-use values that are integral and in [0, 256).  A label that is NaN, infinite or outside the int64 range gives an all-zero row
 * (the reference's conversion yields an out-of-range integer, which tf.one_hot encodes as zeros); such a land-use value matches no
 * entry.  Any class outside [0, nclasses) gives an all-zero row.
 * Refused (error code, satcv_last_error naming label_onehot, nothing written): a null lc or dst; n, h, w_ or nclasses <= 0; hin < h,
 * win < w_; a kind outside 0..6; lu without lu_lut; rot outside 0..3; coff < 0; ldc < coff + nclasses. */
int satcv_label_onehot(const void* lc, int32_t lc_kind, const int32_t* lut, const void* lu, int32_t lu_kind, const int32_t* lu_lut,
                       int32_t n, int32_t hin, int32_t win, int32_t h, int32_t w_, int32_t nclasses, int32_t flip_v, int32_t flip_h,
                       int32_t rot, float* dst, int32_t ldc, int32_t coff, void* stream);

/* ------------------------------------------------------------------ TFRecord training pipeline
 * Device version of to_tuple (utils/processing.py:335-392) for one BATCH of parsed records, and of the per-record part of
 * make_pred_dataset (utils/prediction_tools.py:159-226).
 * src: (n, k, h, w_) fp32 planar, contiguous; plane j of sample i is feature j of that record as parsed.  kind[j]:
 *   SATCV_PLANE_BAND             continuous band: colour augmentation, then rescale / standardise
 *   SATCV_PLANE_ONEHOT           categorical feature: uint8(v) == e for e < depth[j] as 0/1              -- :349
 *   SATCV_PLANE_RESPONSE         raw response                                                             -- :346
 *   SATCV_PLANE_RESPONSE_ONEHOT  response as one-hot of depth[j]                                          -- :344
 *   SATCV_PLANE_PASS             band copied unchanged (what custom functions append after the rescale, prediction_tools.py:463-464)
 * Feature channels of a pixel, in order: the bands, the passthrough bands, the one-hot features (each group in plane order) -- the
 * order to_tuple concatenates them (:355); label channels: the response planes.
 * Per-sample parameters: params (n, ld_params) fp32 on the device, row = contra[nband] | bright[nband] | flip_lr | flip_ud | rot.
 *   color: (x - m_c) * contra_c + m_c * bright_c per band (aug_tensor_color, :129-152); m_c = the mean over (h, w) of the statistics
 *          table rounded to fp32, or mean_in (n, nband) fp32 when given
 *   mode:  SATCV_RECORD_RESCALE (x - mn) / ((mx - mn) + eps) (rescale_tensor, :281-322), SATCV_RECORD_NORMALIZE
 *          (x - mean) / sqrt(var + eps) (normalize_tensor, :225-279), applied AFTER the colour step; statistics from stat_src:
 *          MOMENTS  mom_a / mom_b per band (min, max or mean, variance)
 *          CHANNEL  per band over (h, w) (axes [0, 1]): the raw min / max of the table pushed through the same fp32 colour expression
 *                   (monotone, so exact); mean and variance in closed form in double
 *          PIXEL    per pixel over the bands of a group (axes [2])
 *          GROUP    over everything of a group (axes [0, 1, 2])
 *          groups: bands [gstart[g], gstart[g] + glen[g]); bands outside every group pass through (normalize_tensor's remainder)
 *   morph: flip left-right, flip up-down, np.rot90 by rot of features and labels as one stack (aug_tensor_morph, :169-183); needs h == w_
 * x: fp32 NHWC (n, h, w_, ld_x) written at channel offset coff_x; y: (n, h, w_, ld_y) at coff_y (may be NULL without response planes).
 * Arithmetic: the colour and rescale expressions are separate correctly rounded fp32 operations in NumPy's order (no FMA).
 *
 * satcv_record_stats fills stats (n, k, 4) doubles = mean, min, max, population variance over (h, w) of every BAND plane: double sums
 * of the fp32 samples in a fixed order, min(16, max(1, h * w_ / 4096)) workgroups per plane and a second stage (no atomics; the order
 * does not depend on n).  stats_ws: n * k * SATCV_RECORD_STAT_SPLITS * 4 doubles are always enough.  A descriptor that names a
 * destination x is checked as satcv_record_to_tuple checks it, so that a transform that will be refused starts no launch at all. */
#define SATCV_RECORD_MAX_PLANES 32
#define SATCV_RECORD_STAT_SPLITS 16
enum { SATCV_PLANE_BAND = 0, SATCV_PLANE_ONEHOT = 1, SATCV_PLANE_RESPONSE = 2, SATCV_PLANE_RESPONSE_ONEHOT = 3, SATCV_PLANE_PASS = 4 };
enum { SATCV_RECORD_NONE = 0, SATCV_RECORD_RESCALE = 1, SATCV_RECORD_NORMALIZE = 2 };
enum { SATCV_STAT_MOMENTS = 0, SATCV_STAT_CHANNEL = 1, SATCV_STAT_PIXEL = 2, SATCV_STAT_GROUP = 3 };
typedef struct satcv_record_desc {
  const float* src;
  int32_t n, k, h, w_;
  int32_t kind[SATCV_RECORD_MAX_PLANES], depth[SATCV_RECORD_MAX_PLANES];
  const float* params; int32_t ld_params;
  int32_t color, morph, mode, stat_src;
  int32_t ngroups, gstart[SATCV_RECORD_MAX_PLANES], glen[SATCV_RECORD_MAX_PLANES];
  float mom_a[SATCV_RECORD_MAX_PLANES], mom_b[SATCV_RECORD_MAX_PLANES];
  float eps;
  double* stats; double* stats_ws; int64_t stats_ws_bytes;
  const float* mean_in;
  float* x; int32_t ld_x, coff_x;
  float* y; int32_t ld_y, coff_y;
} satcv_record_desc;
int satcv_record_stats(const satcv_record_desc* d, void* stream);
int satcv_record_to_tuple(const satcv_record_desc* d, void* stream);

/* ------------------------------------------------------------------ device-resident scene prediction
 * The sliding-window loop of predict_pc_local / predict_chips (utils/prediction_tools.py:133-156) with the scene and the
 * prediction map resident on the device.  `origins` is a device int32 (total, 2) table of (y, x): the upper-left corner of each
 * chip's CENTRE in scene coordinates -- what generate_chip_indices (:87-109) returns -- uploaded once per scene; a launch
 * takes chips [first, first + n).
 *
 * satcv_scene_gather replaces the window slicing of :149 and np.array([chip]) of :152.
 *   src: scene (h, w_, c), HWC contiguous, of kind 0 u8, 1 u16, 2 f32, 3 i16 (the kinds of satcv_tile_desc)
 *   value = (float)((double)src / rescale), rescale 0 = none (satcv_tile_ingest's convention)
 *   chip k reads scene rows y - off .. y - off + side - 1 and columns likewise (off = buff / 2, side = kernel + buff).
 *   Out-of-scene coordinates are mirrored without repeating the edge sample (np.pad mode='reflect': i < 0 -> -i,
 *   i >= h -> 2 (h - 1) - i) and then clamped to [0, h - 1]: the kernel never reads outside the scene, whatever the table holds
 *   dst: fp32 NHWC (n, side, side, ldc) written at channel offset coff */
typedef struct {
  const void* src; int32_t src_kind;
  int32_t h, w_, c;
  double rescale;
  const int32_t* origins; int32_t total, first, n;
  int32_t off, side;
  float* dst; int32_t ldc, coff;
} satcv_scene_gather_desc;
int satcv_scene_gather(const satcv_scene_gather_desc* d, void* stream);
/* satcv_scene_scatter replaces the crop and `template[...] +=` of :154 and the crops of :267 / :349.
 *   src: (n, sh, sw, lds) of kind 2 f32 (probabilities) or 5 i32 (classes), channels [c0, c0 + nc)
 *   the crop_h x crop_w window starting at (crop_y, crop_x) of chip k is placed at map position origins[first + k], clipped to
 *   [0, h) x [0, w_)
 *   dst: map (h, w_, ldd) of kind 2 f32 or 0 u8 (class maps: needs an i32 source and accumulate 0), written at channel offset doff;
 *   accumulate 1: dst += src, 0: dst = src
 * Contract: the placed windows of the chips of ONE launch are pairwise disjoint (plain read-modify-write, no atomics); launches on a
 * stream are ordered, so overlapping chips go into separate launches and the result is deterministic. */
typedef struct {
  const void* src; int32_t src_kind;
  int32_t n, sh, sw, lds, c0, nc;
  int32_t crop_y, crop_x, crop_h, crop_w;
  const int32_t* origins; int32_t total, first;
  void* dst; int32_t dst_kind;
  int32_t h, w_, ldd, doff;
  int32_t accumulate;
} satcv_scene_scatter_desc;
int satcv_scene_scatter(const satcv_scene_scatter_desc* d, void* stream);
/* satcv_series_gather: the gather of the ConvLSTM2D time-series models.  One launch cuts chips [first, first + n) out of a resident
 * time stack and writes them as the time-major input tensor those models read (satcv_ingest_seq's output layout).  It replaces, for
 * a chip batch, the host steps of LSTMDataGenerator.__getitem__ (utils/processing.py:937-972): the window slicing of the
 * (T, C, H, W) arrays, np.moveaxis(batch, 2, 4), normalize_timeseries (utils/processing.py:185-193: arr / maxval, NaN -> 0), the
 * cast to float32, and the ingest into the storage type.
 *   src:     (t, c, h, w_) planar, contiguous, of kind 1 u16, 2 f32 or 3 i16 (the kinds of satcv_tile_desc); the launch reads the
 *            first `steps` acquisitions, 1 <= steps <= t
 *   value = (float)((double)src / maxval), NaN becoming 0; maxval != 0 (satcv_scene_gather's double-then-round convention)
 *   origins, total, first, n, off, side: as for satcv_scene_gather, including the reflect-then-clamp rule for coordinates outside
 *            the (h, w_) plane: the kernel never reads outside the stack, whatever the table holds
 *   dst:     (steps, n, side, side, cpad) in the storage type `dtype` (SATCV_BF16 or SATCV_F32), 16-byte aligned; cpad % 8 == 0,
 *            cpad >= c; channels c .. cpad - 1 are written as zero.  The conversion to bf16 is that of satcv_ingest_seq: equal
 *            float32 values give equal bits */
typedef struct {
  const void* src; int32_t src_kind;
  int32_t t, c, h, w_, steps;
  double maxval;
  const int32_t* origins; int32_t total, first, n;
  int32_t off, side;
  void* dst; int32_t dtype, cpad;
} satcv_series_gather_desc;
int satcv_series_gather(const satcv_series_gather_desc* d, void* stream);

/* ------------------------------------------------------------------ median composite of an image time stack
 * Everything of run_local (utils/pc_tools.py:620-668; twin predict_pc_local, utils/prediction_tools.py:731-779) between "the
 * acquisitions are in memory" and the chip loop, in ONE launch:
 *   per sample      v > 0 ? v : NaN (:376; NaN stays NaN, negative i16 / f32 values are nodata), then for an acquisition whose
 *                   offset is > 0: max(v, offset) - offset (harmonize_to_old, :284-326; a valid value <= offset becomes 0 and
 *                   stays valid)
 *   per pixel, band median over time of the valid samples, the mean of the two middle ones for an even count, NaN for none
 *                   (DataArray.median(dim='time'), :642-643)
 *   per pixel       (median - mean) / (sd + 1e-6), mean and sd (ddof 0) over the bands that are not NaN; a NaN band stays NaN
 *                   (normalize_dataArray, :90-107)
 *   src:     (t, c, h, w_) planar, contiguous, of kind 1 u16, 2 f32 or 3 i16 (the kinds of satcv_tile_desc); c <= 16,
 *            t <= SATCV_COMPOSITE_MAX_T, h * w_ < 2^31
 *   offsets: t floats on the device (0 = none; 1000 for Sentinel-2 acquisitions on or after 2022-01-25), or NULL.  The 16-bit kinds
 *            take an offset rounded to the nearest integer and limited to 65535 (their harmonisation is integer arithmetic)
 *   median:  (h, w_, ld_med) fp32 written at channel offset coff_med, or NULL
 *   norm:    (h, w_, ld_norm) fp32 written at channel offset coff_norm, or NULL; use_fill: NaN in norm (only there) becomes `fill`.
 *            Both are the HWC layout satcv_scene_gather reads; with ld_norm = 2 c two launches put the before / after composites
 *            into the halves of one scene (the xr.concat over 'band' of :650)
 * Numerics: samples are held exactly (f32 stacks: max(v, offset) - offset is rounded to fp32); the selection is exact; the midpoint
 * of an even count and the whole normalisation are computed in double from the double medians and rounded once to fp32. */
#define SATCV_COMPOSITE_MAX_T 256
typedef struct satcv_composite_desc {
  const void* src; int32_t src_kind;
  int32_t t, c, h, w_;
  const float* offsets;
  float* median; int32_t ld_med, coff_med;
  float* norm; int32_t ld_norm, coff_norm;
  int32_t use_fill; float fill;
} satcv_composite_desc;
int satcv_median_composite(const satcv_composite_desc* d, void* stream);

/* ------------------------------------------------------------------ Sentinel-2 quality masks of a time stack
 * The per-sample masks of utils/ee_tools.py on a resident (t, cs, h, w_) planar stack, ONE launch: basicQA (:159-180),
 * sentinelCloudScore (:218-255) with the `cloudScore <= 15` of maskTOA (:288-306), waterScore (:115-157) with the `<= 0.25` and the
 * `B11 > 900` shadow test of mask (:257-268), and the scene classification of maskSR (:270-286).  The Cloud Displacement Index and
 * the JRC water history that mask also consults are external products and stay out, as maskTOA leaves them out.
 *   src:     (t, cs, h, w_) planar, contiguous, of kind 1 u16, 2 f32 or 3 i16; cs <= 16, t <= SATCV_COMPOSITE_MAX_T, h * w_ < 2^31
 *   offsets: as for the composite; applied to the REFLECTANCE roles only, before anything else, as max(v, off) - off
 *   band:    the plane of each role in the order B1, B2, B3, B4, B8, B10, B11, B12, QA60, SCL (SATCV_Q_ROLE_*); -1 = absent.  A rule
 *            or an output whose roles are absent is an error before any launch.  Only the planes of the selected rules are read
 *   rules:   a set of SATCV_Q_* bits; cloud_max (reference: 15) and shadow_min (reference: 900) are their thresholds
 *   clear:   uint32 bit-planes (ceil(t / 32), h, w_): bit j % 32 of word j / 32 is 1 when acquisition j passes every selected rule
 *            at that pixel; unused high bits are 0.  Or NULL
 *   cloud_score: (t, h, w_) uint8, 0 ... 100, 255 where a band the score reads is nodata; or NULL
 *   water_score: (t, h, w_) fp32 in [0, 1], NaN where a band the score reads is nodata; or NULL.  At least one output is non-null
 * Nodata: a sample passes a rule only if every reflectance band that rule reads is valid (> 0, not NaN) at that acquisition and
 * pixel -- in Earth Engine a masked input masks the result.  QA60 and SCL are codes: the nodata rule does not apply to them; in an
 * f32 stack a NaN code fails the rule and other values are truncated to integers.
 * Rules, on the harmonised DN x (the reference divides by 10000 in sentinel2toa :90; the constants are multiplied through):
 *   QA60    (qa & 1024) == 0 && (qa & 2048) == 0
 *   CLOUD   s100 = min(100, (B2 - 1000) / 40, (B1 - 1000) / 20, (B1 + B10 - 1500) / 5, (B2 + B3 + B4 - 2000) / 60,
 *                      500 (B8 - B11) / (B8 + B11) + 50, 400 - 500 (B3 - B11) / (B3 + B11));
 *           cloud_score = floor(s100) limited to 0 ... 100 (`.multiply(100).byte()`: saturating, truncating); clear when
 *           cloud_score <= cloud_max
 *   SHADOW  B11 > shadow_min
 *   WATER   w1 = clamp((3500 - (B8 + B11 + B12)) / 1500, 0, 1); w2 = clamp((B2 - sd) / mean, 0, 1), mean and sd (ddof 0: the
 *           population form is taken for ee.Reducer.stdDev) over B3, B4, B8, B11, B12; w3 = ((B3 - B11) / (B3 + B11) - 0.3) / 0.5;
 *           water_score = clamp(min(1, w1, w2, w3), 0, 1); the sample is water when all three terms exceed 1/4, and passes when
 *           it is not water
 *   SCL     the code is none of 0 (nodata), 2, 3, 8, 9, 10, 11
 *   A quotient whose denominator is 0 (both bands of a normalised difference 0 after the harmonisation, mean 0) is 0, Earth Engine's
 *   convention for a division by zero.
 * Numerics: decisions are exact on the stored sample values, not the result of a floating-point evaluation order.  The 16-bit kinds
 * use integer arithmetic (division-free cross-multiplied inequalities, 64-bit products for w2, floor divisions for the score); f32
 * stacks evaluate the same cross-multiplied inequalities in double, which is exact for integer-valued data below 2^22 -- fractional
 * f32 data are decided by those double expressions.  water_score is computed in double and rounded once to fp32. */
#define SATCV_Q_QA60 1
#define SATCV_Q_CLOUD 2
#define SATCV_Q_SHADOW 4
#define SATCV_Q_WATER 8
#define SATCV_Q_SCL 16
#define SATCV_Q_ROLES 10
typedef struct satcv_quality_desc {
  const void* src; int32_t src_kind;
  int32_t t, cs, h, w_;
  const float* offsets;
  int32_t band[SATCV_Q_ROLES];
  int32_t rules;
  int32_t cloud_max; float shadow_min;
  uint32_t* clear;
  uint8_t* cloud_score;
  float* water_score;
} satcv_quality_desc;
int satcv_quality_mask(const satcv_quality_desc* d, void* stream);

/* Median composite under a clear mask and a band selection (the composites the reference's models were trained on: every
 * acquisition masked by utils/ee_tools.py before the median).  Everything of satcv_median_composite holds, with
 *   base:     its descriptor; base.c is the number of OUTPUT bands (<= 16), base.src has cs planes per acquisition
 *   clear:    the bit-planes satcv_quality_mask writes, or NULL (every sample clear).  A sample is valid iff v > 0 and its bit is set
 *   cs:       planes per acquisition in base.src (<= 16)
 *   band_idx: the plane of output band b, 0 <= band_idx[b] < cs for b < base.c -- a 14-plane quality stack yields a 4-band composite
 *             without a copy
 * With clear = NULL and the identity table the results equal satcv_median_composite's bit for bit. */
typedef struct satcv_composite_masked_desc {
  satcv_composite_desc base;
  const uint32_t* clear;
  int32_t cs;
  int32_t band_idx[16];
} satcv_composite_masked_desc;
int satcv_median_composite_masked(const satcv_composite_masked_desc* d, void* stream);

/* ------------------------------------------------------------------ Cloud-Optimized GeoTIFF writer: the device half
 * What numpy_to_raster / arrays_to_cog (utils/raster_tools.py:367-461: rasterio's write, then GDAL's COG driver with COMPRESS=LZW
 * and nodata = 255) and write_geotiff_prediction(s) (utils/prediction_tools.py:447-536) do to the samples of a map, on a map that is
 * resident on the device.  The container (IFDs, GeoKeys) is host code in raster_tools.py.  Kinds: 0 u8, 1 u16, 2 f32, 3 i16, 5 i32
 * (those of satcv_tile_desc).  One descriptor serves the three per-sample entries; each reads the fields named for it.  Refused on
 * the host before any launch: c > 16, unknown kinds, a map beyond 2^31 pixels, and what each entry lists.
 *
 * satcv_raster_convert (rasterio's `astype(dtype)` of :399 / :472 with the `nodata` of :393):
 *   src (h, w_, ld) of src_kind read at channel offset coff, c bands -> dst contiguous (h, w_, c) of dst_kind
 *   to f32:                a plain cast; an f32 source is first multiplied by `scale` (one fp32 multiply; 0 = none, f32 sources only)
 *   f32 -> integer kind:   NaN -> nodata (0 without has_nodata), else rintf (half to even) of the fp32 product, saturated to the kind
 *   integer -> integer:    saturated
 * satcv_raster_overview (the overviews GDAL's COG driver adds, :405 / :455; the resampling rules are THIS library's, GDAL's default is cubic):
 *   src contiguous (h, w_, c) -> dst (ceil(h / 2), ceil(w_ / 2), c), same kind.  Per 2 x 2 block only samples inside the image count; a
 *   sample equal to nodata (with has_nodata) is invalid, and so is NaN.  resampling:
 *   0 nearest   src[2 y, 2 x]
 *   1 average   over the valid samples; none valid -> nodata, NaN for f32 without nodata.  Integers: floor((2 sum + n) / (2 n)) in 64
 *               bits; f32: the valid samples added in row-major order in fp32, one fp32 division
 *   2 mode      the most frequent valid value, ties to the smallest; none valid -> nodata.  Integer kinds only
 * satcv_raster_tiles (TILED=YES, BLOCKSIZE, PREDICTOR=2 of the COG driver):
 *   src contiguous (h, w_, c) -> dst (nty * ntx, blocksize, blocksize, c), tile-major (tiles row-major), pixel-interleaved, same kind;
 *   nty = ceil(h / blocksize), ntx = ceil(w_ / blocksize); blocksize a multiple of 16, tile bytes below 2^30.  Samples outside the image
 *   are nodata (0 without).  predictor != 0 (integer kinds only): every sample but those of the first pixel of a tile row becomes
 *   itself minus the same band of the pixel to its left, modulo 2^bits, both taken from the padded tile before any subtraction. */
typedef struct satcv_raster_desc {
  const void* src; int32_t src_kind;
  int32_t h, w_, c, ld, coff;
  void* dst; int32_t dst_kind;
  float scale;
  int32_t has_nodata; double nodata;
  int32_t resampling;
  int32_t blocksize, predictor;
} satcv_raster_desc;
int satcv_raster_convert(const satcv_raster_desc* d, void* stream);
int satcv_raster_overview(const satcv_raster_desc* d, void* stream);
int satcv_raster_tiles(const satcv_raster_desc* d, void* stream);
/* satcv_lzw_tiles (COMPRESS=LZW of :405 / :455): n tiles of tile_bytes each (contiguous, 16-byte aligned, tile_bytes a multiple of 16
 * below 2^30) -> tile i's stream at dst + i * (2 * tile_bytes + 16), its length in sizes[i]; bytes of a slot past sizes[i] are
 * unspecified.  The slot is enough for any input: a code is at most 12 bits and consumes at least one byte, plus one Clear per 3836
 * codes, the opening Clear and EOI.  One wavefront per tile, the dictionary in LDS.
 * The stream is TIFF 6.0 section 13 LZW, made unique by: MSB-first packing; Clear (256) first, at 9 bits; greedy longest match, first
 * free code 258; after an entry is added: next free code 4094 -> Clear at the current width and start over at 9 bits, 512 / 1024 / 2048
 * -> one bit wider (libtiff's "early change"); after the last data code the same counter step once more; then EOI (257), zero-padded
 * to a byte.  libtiff decodes it; libtiff's own encoder adds ratio-driven Clears, so its bytes differ.
 * satcv_lzw_encode_host: the same coder on a HOST buffer (n >= 0 bytes below 2^30).  *size receives the length of the stream; when it
 * exceeds cap the call fails and nothing is written past dst + cap. */
int satcv_lzw_tiles(const void* src, int32_t n, int64_t tile_bytes, void* dst, int32_t* sizes, void* stream);
int satcv_lzw_encode_host(const void* src, int64_t n, void* dst, int64_t cap, int64_t* size);
/* satcv_bytes_compact: the first sizes[i] bytes of slot i (slots + i * slot_bytes) -> dst + offsets[i], i < n; sizes and offsets are
 * device arrays, the offsets computed by the host from the sizes it read back (every tile of a TIFF starts on an even offset).  A byte
 * that would land outside [0, dst_bytes) is not written.  The result is the file's tile payload: one device-to-host copy. */
int satcv_bytes_compact(const void* slots, int64_t slot_bytes, const int32_t* sizes, const int64_t* offsets, int32_t n, void* dst,
                        int64_t dst_bytes, void* stream);

/* ------------------------------------------------------------------ GeoTIFF / COG reader: the device half
 * What rasterio's `open().read(window=)` and rioxarray's `open_rasterio` (utils/pc_tools.py:131-186, 328-386) do to the blocks of a
 * file, with the result resident on the device: the mirror image of the writer above.  The container is parsed on the host
 * (raster_tools.read_info), the compressed blocks go up in one copy.
 *
 * satcv_lzw_decode_tiles: n compressed slices payload[offsets[i], offsets[i] + sizes[i]) (offsets and sizes are device arrays; a slice
 * may start at any byte and is clipped to [0, payload_bytes)) -> block i at dst + i * dst_stride, at most block_bytes of it, the count
 * in lengths[i] (lengths may be NULL), and status[i]:
 *   0 ok          EOI was read, or block_bytes bytes are out (a stream need not end with EOI)
 *   1 truncated   the slice ended inside a code, or before either of the above
 *   2 bad code    a code above the next free one, or a non-literal first code after a Clear
 *   3 overlong    a code whose string would pass block_bytes
 * Bytes of a block past lengths[i] are not written, bytes outside a slice are not read.  Accepted: every TIFF 6.0 section 13 stream
 * libtiff accepts -- MSB-first codes; widths 9 -> 10 once the next free code is 511, then 1023, 2047 ("early change"); a Clear
 * anywhere; no Clear at the start; no EOI; a full table (no more entries, the width stays 12).  Not the LSB-first "old-style" variant.
 * One wavefront per block; no loop bound depends on the data.  dst_stride >= block_bytes; a 16-byte aligned slot is written 16 bytes
 * per lane.
 * satcv_lzw_decode_host: the same decoder on HOST buffers: n bytes of stream -> at most cap bytes at dst, the count in *size, the
 * status above in *status.  The return value is SATCV_OK whenever the arguments were usable, whatever the stream held. */
int satcv_lzw_decode_tiles(const void* payload, int64_t payload_bytes, const int64_t* offsets, const int32_t* sizes, int32_t n, int64_t block_bytes,
                           void* dst, int64_t dst_stride, int32_t* status, int32_t* lengths, void* stream);
int satcv_lzw_decode_host(const void* src, int64_t n, void* dst, int64_t cap, int64_t* size, int32_t* status);
/* satcv_raster_untile, the inverse of satcv_raster_tiles: decoded blocks -> the window (row0, col0, h, w_) of the image, resident.
 *   src         decoded block j (j < nblocks) at src + j * src_stride: (bh, bw, spp) samples for planar 1, (bh, bw) for planar 2; a strip
 *               is a block of the image's width and RowsPerStrip rows
 *   blocks      device array: blocks[j] is block j's index in the file's block list -- row-major with `across` blocks per row, and for
 *               planar 2 band after band, per_plane blocks each.  Only the blocks the window touches need to be there
 *   predictor   2 (integer kinds only): a running sum along every block row, per band, modulo 2^bits, from the block's first pixel on
 *               -- also when the window starts to its right.  One wavefront per block row; without a predictor one thread per sample
 *   dst         layout 0: (h, w_, ld), sample of band b at channel coff + band_map[b]; layout 1: (ld, h, w_), plane coff + band_map[b].
 *               band_map[b] = -1 drops band b.  Samples outside the window are dropped, those of edge blocks outside the image with them
 * Refused on the host before any launch: unknown kinds, spp > 16, a planar configuration other than 1 or 2, a predictor other than 0 or
 * 2 or on f32, blocks of 2^30 bytes and more, a window beyond 2^31 pixels, channels outside ld, misaligned pointers. */
typedef struct satcv_untile_desc {
  const void* src; int64_t src_stride;
  const int32_t* blocks; int32_t nblocks;
  int32_t bh, bw, across, per_plane;
  int32_t spp, planar, kind, predictor;
  int32_t row0, col0, h, w_;
  void* dst; int32_t layout, ld, coff;
  int32_t band_map[16];
} satcv_untile_desc;
int satcv_raster_untile(const satcv_untile_desc* d, void* stream);

/* ------------------------------------------------------------------ Raster alignment: resampling between two grids of one CRS
 * What stackstac.stack(resolution=), gdal.BuildVRT / rioxarray's merge_arrays and reproject_match do to the samples before any code of
 * the reference runs (utils/pc_tools.py:152-186, 251-282, 368-431): a resident raster is resampled onto another north-up or south-up
 * grid of the SAME coordinate system (scale and shift per axis; no rotation, no reprojection).  The grid arithmetic is host code in
 * raster_tools.py.  The rules below are THIS library's (GDAL's and stackstac's are not restated): tests/warp_oracle.py says them again
 * in float64 NumPy.
 *
 * Rasters: src is a window of the source grid, (sh, sw, src_ld) for src_layout 0 or (src_ld, sh, sw) for 1; src[0, 0] is pixel
 * (src_row0, src_col0) of the source grid.  dst likewise with (dh, dw, dst_ld), dst[0, 0] being pixel (dst_row0, dst_col0) of the
 * destination grid.  Bands src_coff .. src_coff + c - 1 go to dst_coff .. dst_coff + c - 1; no other channel of dst is written.  Kinds
 * as in the writer section (0 u8, 1 u16, 2 f32, 3 i16, 5 i32); dst_kind is src_kind or 2.
 * Coordinates: pixel k of a grid covers [k, k + 1).  Destination pixel (i, j) = (dst_row0 + local row, dst_col0 + local column) has the
 * source-grid coordinates u = su * (j + 0.5) + ou, v = sv * (i + 0.5) + ov, in float64 with the product and the sum rounded
 * separately (the kernel is compiled with floating-point contraction off: a fused multiply-add moves floor(u) on real grids).  From
 * two Affine transforms: su = a_d / a_s, ou = (c_d - c_s) / a_s, sv = e_d / e_s, ov = (f_d - f_s) / e_s; su or sv < 0 is a grid of
 * the opposite orientation.  The window origin is subtracted from floor(...) only, so a warp of a window equals the warp of the whole
 * raster bit for bit wherever the window holds the taps.
 * Validity: a source sample is valid when it lies inside the sh x sw window, is not NaN and (with has_src_nodata) differs from
 * src_nodata (compared as float64).
 * resampling (all arithmetic in float64; taps are added rows outer, columns inner):
 *   0 nearest    the sample at (floor(v), floor(u)); invalid when that sample is
 *   1 bilinear   x0 = floor(u - 0.5), t = u - 0.5 - x0, taps x0, x0 + 1 with the weights 1 - t, t; the same in v; a tap's weight is
 *                the product of its two.  The tap nearest picks (the pixel that contains the point) must be valid, otherwise the
 *                result is invalid.  Then: sum of weight * sample over the valid taps, divided by the sum of their weights -- a convex
 *                combination: nothing bleeds into a hole, nothing is amplified
 *   2 cubic      Catmull-Rom (a = -0.5): taps x0 - 1 .. x0 + 2 with the weights -t^3/2 + t^2 - t/2, 3t^3/2 - 5t^2/2 + 1,
 *                -3t^3/2 + 2t^2 + t/2, t^3/2 - t^2/2, evaluated as written from t, t * t and t * t * t; the sum of the 16
 *                products, not renormalised.  Only when all 16 taps are valid; otherwise the sample takes rule 1.  (A partial stencil
 *                is not renormalised: with the negative lobes alone beside the containing tap the weight sum falls to 0.035.)
 *   3 average    the footprint of the destination pixel is [min, max] of su * j + ou and su * (j + 1) + ou, likewise in v; a source
 *                pixel's weight is the area of its overlap with it (product of the overlaps per axis); sum of weight * sample over
 *                the valid samples of positive weight, divided by their weight sum; no such sample: invalid.  ceil(|s|) + 1 taps
 *                per axis, whatever the data.  |su| or |sv| above 64 is refused: read an overview instead
 * Result: f32 -- the float64 value rounded once; integer kinds -- rint (half to even), saturated to the kind.  An invalid result
 * leaves dst untouched with keep; otherwise it is dst_nodata (in the kind, as the writer's nodata), and without has_dst_nodata NaN
 * for f32 and 0 for integers.
 * One thread per destination pixel and all its bands, neighbouring lanes on neighbouring columns; bands travel in groups of 4 or 2
 * by one load and one store where c, ld, coff and the address allow.
 * Refused on the host before any launch: null or misaligned pointers, unknown kinds, layouts or methods, dst_kind neither src_kind
 * nor f32, c > 16, channels outside ld, a zero or non-finite scale or a non-finite offset, non-positive sizes, rasters beyond 2^31
 * pixels, src and dst overlapping. */
typedef struct satcv_warp_desc {
  const void* src; int32_t src_kind, src_layout;
  int32_t sh, sw, src_ld, src_coff;
  int32_t src_row0, src_col0;
  void* dst; int32_t dst_kind, dst_layout;
  int32_t dh, dw, dst_ld, dst_coff;
  int32_t dst_row0, dst_col0;
  int32_t c;
  double su, ou, sv, ov;
  int32_t resampling;
  int32_t has_src_nodata; double src_nodata;
  int32_t has_dst_nodata; double dst_nodata;
  int32_t keep;
} satcv_warp_desc;
int satcv_raster_warp(const satcv_warp_desc* d, void* stream);

/* ------------------------------------------------------------------ Reprojection between coordinate systems
 * What the reference leaves to PROJ behind gdal.Warp (utils/pc_tools.py:152-186, the two-UTM-zone NAIP case), stackstac.stack(epsg=)
 * (get_s2_stac / get_s1_stac / get_hag_stac) and rasterio's transform_bounds (utils/prediction_tools.py:560-600).  The projection rules
 * -- Krueger's n^6 series for the transverse Mercator, the spherical Mercator, longitude wrapping, the domain, no datum shift between
 * WGS84 and NAD83 -- are written in csrc/crs_core.hpp, the one source of the host loop and of the kernels; tests/crs_oracle.py says
 * them again in float64 NumPy.  csrc/reproject.hip is compiled with floating-point contraction off.
 *
 * satcv_crs: kind 0 geographic (x = longitude, y = latitude, degrees: the GeoTIFF axis order), 1 transverse Mercator, 2 spherical (web)
 * Mercator; a, inv_f the ellipsoid; lon0 the central meridian in degrees (0 for kinds 0 and 2); k0 the scale on it; fe, fn the false
 * easting and northing in metres.  The host table of EPSG codes is satellite_computervision_amd/crs.py.
 *
 * satcv_crs_transform: n points (x[k], y[k]) of `from` -> (xo[k], yo[k]) of `to`: crs_inverse(from), then crs_forward(to).  A point
 * outside either domain gets NaN and ok[k] = 0 (ok may be NULL).  on_device = 0: host pointers, the loop runs on the CPU (bounds and
 * windows of the Python host code); 1: device pointers, one thread per point.  xo / yo may be x / y.
 *
 * satcv_reproject_map: the destination grid (dst_crs; dst_a, dst_c, dst_e, dst_f of its Affine transform) and the source (src_crs; with
 * has_src_transform its src_a, src_c, src_e, src_f; without, "source CRS units": u, v are the coordinates themselves, e.g. the
 * longitude / latitude field of a UTM scene).  The chain of destination pixel (i, j), GLOBAL indices (so a strip equals the whole):
 *     X = dst_a * (j + 0.5) + dst_c,  Y = dst_e * (i + 0.5) + dst_f;  (lon, lat) = crs_inverse(dst_crs, X, Y);
 *     (Xs, Ys) = crs_forward(src_crs, lon, lat);  u = (Xs - src_c) / src_a,  v = (Ys - src_f) / src_e
 * each product, sum and quotient rounded on its own.  A pixel whose chain is not ok has u = v = NaN.
 * satcv_grid_coords: u and v (dh x dw float64 planes on the device) of the window (row0, col0, dh, dw) of the destination grid.
 * satcv_raster_reproject: satcv_raster_warp with u, v from the chain -- through the same inline device function as satcv_grid_coords,
 * so the two kernels' coordinates agree bit for bit -- in place of su * (j + 0.5) + ou; d->su / ou / sv / ov are ignored, every other
 * field and rule of the descriptor is unchanged (kinds, layouts, ld / coff, src_row0 / src_col0, dst_row0 / dst_col0, nodata, keep,
 * band packs; 0 nearest, 1 bilinear, 2 cubic).  A pixel whose chain is not ok is invalid.  Method 3 (average) is refused: the footprint
 * of a pixel is no axis-parallel rectangle any more.
 * Refused on the host before any launch: what satcv_raster_warp refuses except its scale checks, a null map, an unknown CRS kind,
 * non-positive a or inv_f, non-finite parameters, zero or non-finite transform scales, non-finite origins, method 3. */
typedef struct satcv_crs { int32_t kind; double a, inv_f, lon0, k0, fe, fn; } satcv_crs;
typedef struct satcv_reproject_map {
  satcv_crs dst_crs; double dst_a, dst_c, dst_e, dst_f;
  satcv_crs src_crs; int32_t has_src_transform; double src_a, src_c, src_e, src_f;
} satcv_reproject_map;
int satcv_crs_transform(const satcv_crs* from, const satcv_crs* to, const double* x, const double* y, double* xo, double* yo, uint8_t* ok,
                        int64_t n, int32_t on_device, void* stream);
int satcv_grid_coords(const satcv_reproject_map* m, int32_t dh, int32_t dw, int32_t row0, int32_t col0, double* u, double* v, void* stream);
int satcv_raster_reproject(const satcv_warp_desc* d, const satcv_reproject_map* m, void* stream);

/* ------------------------------------------------------------------ Radiometric calibration: histogram matching between scenes
 * utils/calibration.py on arrays: clamp_and_scale (:12-45), get_overlap (:64-76), hist_to_FC / make_FC (:78-134), equalize (:136-182)
 * and the chain of equalize_collection (:184-233).  The reference takes a 4096-bucket Earth Engine histogram and fits two 100-tree
 * random-forest regressors (DN -> cumulative probability -> DN), an approximation of CDF matching; this library computes the thing
 * it approximates, exactly and in integers, one bin per stored value.  Every decision is exact on the stored sample values.
 *
 * Kinds: 0 u8 (256 bins), 1 u16 (65536 bins), 3 i16 (65536 bins, bin = v + 32768).  f32 (2) and i32 (5) are refused: f32 needs a
 * binning rule whose rounding can be pinned.  Rasters are (c, h, w_) planar and contiguous, 1 <= c <= 16, h * w_ < 2^31.
 * Validity: a sample equal to nodata (with has_nodata) is invalid; a nodata that is no value of the kind matches no sample.
 *
 * satcv_calib_overlap (get_overlap :64-76 with the footprint geometry replaced by validity): region[y, x] = 1 where EVERY band of a
 *   and (b may be NULL: one raster alone) of b is valid and mask (uint8 (h, w_), may be NULL) is non-zero there, else 0.  A streaming
 *   kernel: a lane takes 16 bytes of every plane per step.
 * satcv_calib_histogram (make_FC :106-134, every stored value its own bucket): hist[band][k] = number of pixels with region != 0
 *   whose band has bin k; uint32 (c, bins), zeroed by the call.  One workgroup takes a strip of 2^18 samples of one plane, counts the
 *   values 0 ... split - 1 in an LDS-private histogram (LDS atomics) and the others straight in global memory, and adds its non-zero
 *   private bins to global memory at the end.  split: 0 the library's choice (16384); n > 0 that many private bins (at most 32768; u8
 *   privatises all 256 whatever n); negative none (global atomics only).  Integer counts: the result does not depend on the arrival order.
 * satcv_calib_match_lut (equalize :136-182): with cum1, cum2 the inclusive cumulative counts of hist1, hist2 and n1, n2 their totals,
 *   lut[band][v] = the value (in the kind) of the smallest bin u with cum1[u] * n2 >= cum2[v] * n1, compared in unsigned 64 bits (the
 *   products stay below 2^62); n1 == 0 or n2 == 0: the identity (the `ee.Algorithms.If(overlap.area(5).gt(0), ...)` of :225, decided
 *   on the device).  Below image 2's smallest occupied bin cum2[v] is 0 and the inequality would hold at bin 0, occupied or not: there
 *   cum2[v] counts as 1, so those bins map where image 2's smallest occupied bin maps at the least.  Every table value is therefore
 *   an occupied bin of image 1 -- never nodata: the validity of an equalized scene is that of the original.  lut is (c, bins) of the
 *   kind; counts (may be NULL) receives n1, n2 per band, int64 (c, 2).
 * satcv_calib_scale_lut (clamp_and_scale :12-45): upper[band] = the value of the smallest bin v with cum[v] * 100 >= p * n (nearest
 *   rank, p = 1 ... 100; the reference ignores its p and always asks for 99), -1 for an empty band; table[band][k] = (float)((double)
 *   min(value(k), upper) / (double)upper), NaN for every k when n == 0 or upper == 0.  table is float32 (c, bins), upper int32 (c).
 * satcv_calib_apply: dst = table[band][bin(src)] for every valid sample of the (c, h, w_) raster src.  table is (c, bins) of the source
 *   kind (dst_kind = src_kind; dst may be src itself: in place) or float32 (dst_kind = 2).  dst is addressed like the warp's
 *   destination: layout 0 (h, w_, ld), layout 1 (ld, h, w_), bands at channels coff ... coff + c - 1, no other channel is written.
 *   An invalid sample leaves dst untouched with keep (an equalized scene painted straight into a mosaic); otherwise it becomes nodata
 *   (source kind; 0 without has_nodata, where no sample is invalid) or NaN (float32).  The table is read through the L2.
 * Refused on the host before any launch: null pointers, unsupported kinds, c < 1 or c > 16, non-positive sizes, h * w_ >= 2^31, p
 * outside 1 ... 100, split above 32768, a dst_kind that is neither src_kind nor 2, an unknown layout, channels outside ld, dst
 * overlapping src other than exactly in place. */
typedef struct satcv_calib_apply_desc {
  const void* src; int32_t src_kind;
  int32_t c, h, w_;
  int32_t has_nodata; double nodata;
  const void* table;
  void* dst; int32_t dst_kind, dst_layout;
  int32_t dst_ld, dst_coff;
  int32_t keep;
} satcv_calib_apply_desc;
int satcv_calib_overlap(const void* a, const void* b, int32_t kind, int32_t c, int32_t h, int32_t w_, int32_t has_nodata, double nodata,
                        const uint8_t* mask, uint8_t* region, void* stream);
int satcv_calib_histogram(const void* src, int32_t kind, int32_t c, int32_t h, int32_t w_, const uint8_t* region, uint32_t* hist,
                          int32_t split, void* stream);
int satcv_calib_match_lut(const uint32_t* hist1, const uint32_t* hist2, int32_t kind, int32_t c, void* lut, int64_t* counts, void* stream);
int satcv_calib_scale_lut(const uint32_t* hist, int32_t kind, int32_t c, int32_t p, float* table, int32_t* upper, void* stream);
int satcv_calib_apply(const satcv_calib_apply_desc* d, void* stream);

/* ------------------------------------------------------------------ Polygon rasterization: clipping rasters to an area of interest
 * What the reference leaves to rioxarray: `rio.clip([aoi], crs)` on its composites (utils/pc_tools.py:595-606; the same call stands
 * commented out at :384, :439 and :493).  Polygons become a uint8 mask or a burned label raster on the device, and one mask is applied
 * to every plane of a raster or a stack.  The rule below is THIS library's, the pixel-centre scanline rule (all_touched = False); it
 * is modelled on GDAL's filled-polygon scanline but nothing pins it to GDAL.  tests/rasterize_oracle.py says it again in float64
 * NumPy; csrc/rasterize_core.hpp is the one source of the crossing column for the host loop and the kernels; csrc/rasterize.hip is
 * compiled with floating-point contraction off.
 *
 * Vertices are grid pixel coordinates in float64 (px = (X - c) / a, py = (Y - f) / e, each operation rounded on its own); a ring is
 * closed implicitly.  Every ring edge is ordered so that y0 < y1; edges with y0 == y1 are dropped.  The edge crosses row i iff
 * y0 <= i + 0.5 < y1, at x = x0 + ((i + 0.5) - y0) * (x1 - x0) / (y1 - y0), evaluated in that order and not fused; its crossing column
 * is col = floor(x + 0.5), clamped to [0, w_] before the integer conversion.  Pixel (i, j) belongs to a geometry iff the number of
 * that geometry's crossings of row i with col <= j is odd: even-odd over all rings of the geometry, so holes and the parts of a
 * MultiPolygon need no special case.  A mask is the union of the geometries; a burn takes the value of the LAST geometry in list
 * order that covers the pixel.
 *
 * The edge table is built on the host (polygons.edge_table): float64 rows {x0, y0, x1, y1, r0, r1, g}, [r0, r1) the rows the edge
 * crosses clipped to [0, h) -- found with the comparison above, not with a ceil -- g the geometry index; an edge of more than 64 rows
 * is split into work items of at most 64.  row_start (int32, h + 1) is the running sum of the per-row crossing counts, which follow
 * from the row ranges alone (a difference array): the workspace is sized without asking the device.  edges, row_start and values are
 * HOST pointers; the call copies them into the workspace on the stream.  They need to stay valid only until the call returns: they are
 * ordinary pageable memory, which the runtime reads (into its own staging buffers) before hipMemcpyAsync returns.  For the same reason
 * the call is refused while the stream is being captured into a graph: a replay would read host memory that is gone.
 * satcv_rasterize_workspace: the bytes satcv_rasterize needs for n_items table rows, h grid rows, n_keys = row_start[h] crossings and
 *   n_geoms values.
 * satcv_rasterize: on_device = 1 -- dst and workspace are device pointers.  Crossings kernel: one lane per (work item, row) appends
 *   key = g << 32 | col at row_start[i] + atomicAdd(cursor[i], 1).  Fill kernel: one workgroup per (row, strip of 8192 columns) sorts
 *   the row's keys in LDS (bitonic, padded to a power of two), walks the consecutive pairs of one g as spans and raises an LDS strip of
 *   int32 winners with atomicMax(g + 1) -- order-independent, so two runs give the same bytes -- then stores the strip.  mode 0 (mask):
 *   dst is u8, 1 inside and 0 outside, swapped by invert.  mode 1 (burn): values[g] (n_geoms samples of dst_kind) inside, fill (in the
 *   kind, as the writer's nodata) outside.  dst is addressed like the warp's destination: layout 0 (h, w_, ld) or 1 (ld, h, w_), the
 *   one channel coff; with keep a pixel no geometry covers is left untouched.  At most 4096 crossings per row (32 KiB of keys beside
 *   the 32 KiB strip: two workgroups per CU).  on_device = 0: dst is a host pointer and the same rule runs on the CPU; no workspace.
 * satcv_raster_mask_apply: where mask (u8 (h, w_)) is 0 -- with invert: is not 0 -- the samples of the channels coff ... coff + c - 1
 *   become nodata in the kind (without has_nodata NaN for f32, 0 for integers); every other sample is copied, or left alone when dst
 *   is src (in place).  layout 0 (h, w_, ld), 1 (ld, h, w_): a (T, C, H, W) stack is ld = T * C planes, a slot of it coff = t * C.  A
 *   streaming kernel: planar rasters (and layout 0 with ld = 1, which is the same memory) take 16 bytes of samples per lane and step; in place
 *   a vector wholly inside the mask is neither read nor written.  Pixel-interleaved rasters with ld > 1 take one pixel and its c channels per lane.
 * Refused on the host before any launch: null pointers, unknown kinds, layouts or modes, a mask that is not u8, non-positive sizes,
 * h * w_ >= 2^31, channels outside ld, non-finite vertices, an unordered edge, r0 / r1 outside [0, h] or not the rows the edge crosses,
 * a work item of more than 64 rows, g outside the values table, a row with more than 4096 crossings (the message names the row and the
 * count), row_start not matching the edge table, a workspace too small or misaligned, a stream that is being captured, dst overlapping the
 * workspace, the mask or (other than exactly in place) src. */
typedef struct satcv_rasterize_desc {
  const double* edges; int64_t n_items;
  const int32_t* row_start;
  int32_t h, w_;
  int32_t n_geoms;
  int32_t mode, invert;
  const void* values; double fill;
  void* dst; int32_t dst_kind, dst_layout;
  int32_t dst_ld, dst_coff;
  int32_t keep;
  int32_t on_device;
  void* workspace; int64_t workspace_bytes;
} satcv_rasterize_desc;
typedef struct satcv_mask_apply_desc {
  const uint8_t* mask; int32_t h, w_;
  int32_t invert;
  const void* src; void* dst;
  int32_t kind, layout;
  int32_t c, ld, coff;
  int32_t has_nodata; double nodata;
} satcv_mask_apply_desc;
int satcv_rasterize_workspace(int64_t n_items, int32_t h, int64_t n_keys, int32_t n_geoms, int64_t* bytes);
int satcv_rasterize(const satcv_rasterize_desc* d, void* stream);
int satcv_raster_mask_apply(const satcv_mask_apply_desc* d, void* stream);

/* ------------------------------------------------------------------ losses
 * Each writes loss_out[0] += mean loss contribution (caller zeroes) and
 * dlogits = dL/dlogits (through the head activation).
 * kind 0: weighted_categorical_crossentropy (utils/model_tools.py:25-40), weights[ncls]
 * kind 1: weighted_bce on probabilities (:96-112), weights[0] = pos_weight                 */
int satcv_loss_fwd_bwd(int32_t kind, const float* probs, const float* y_true,
                       const float* weights, int32_t ncls, int32_t activation, int64_t npix,
                       float grad_scale, float* loss_out, float* dlogits, void* stream);

/* Ratio-type losses that need global sums before the gradient exists (two passes inside):
 * kind 2: gen_dice (utils/model_tools.py:42-94; class_weights = global_weights or NULL for the
 *         per-image 1/count^2 weights with `eps` for empty classes), 3: iou_loss (:131-140),
 *         4: mse_4d (:142-166, mean over finite elements).
 * workspace: nimg*3*ncls floats (zeroed here).  Writes loss_out[0] += loss and dL/dlogits. */
int satcv_loss_global_fwd_bwd(int32_t kind, const float* probs, const float* y_true,
                              const float* class_weights, int32_t ncls, int32_t activation,
                              int32_t nimg, int64_t pix_per_img, float eps, float grad_scale,
                              float* workspace, float* loss_out, float* dlogits, void* stream);

/* confusion[t*ncls + p] += 1 over pixels (MeanIoU / accuracy; notebooks nb:275) */
int satcv_confusion(const int32_t* classes, const float* y_true, int32_t ncls, int64_t npix,
                    int64_t* confusion, void* stream);

/* --------------------------------------------------------------- optimizer
 * Keras Adam (epsilon outside the bias correction).  `state` is a device
 * float[4]: {lr, step_count, grad_scale, unused}; the kernel increments
 * step_count itself so that the launch is graph-replayable. */
int satcv_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float beta1,
                    float beta2, float eps, float* state, const float* lr_mul, void* stream);
/* The same update on a SUB-RANGE of the flat buffers (pointers already offset, n elements), with the step counter incremented only when
 * bump != 0: a step may be applied in several launches -- the part of the parameters whose gradients are final early in the backward pass
 * on a second stream, beside the rest of the backward pass (engine.Plan, round 6) -- as long as exactly ONE of them, the last to run,
 * bumps: every part then sees the same step number. */
int satcv_adam_step_part(float* p, const float* g, float* m, float* v, int64_t n, float beta1,
                         float beta2, float eps, float* state, const float* lr_mul, int32_t bump, void* stream);

/* tf.keras.optimizers.SGD(learning_rate, momentum, nesterov) -- the `optim=` / `OPTIMIZER` a caller hands to the reference's
 * builders (utils/model_tools.py:773-920) and notebooks.  Flat fp32 buffers as for Adam; lr = state[0] and grad_scale = state[2]
 * are read on the device (a replayed graph picks up a new rate), the step counter is not touched (no bias correction).
 *     momentum == 0 (v NULL):  p -= lr g
 *     momentum  > 0:           v = momentum v - lr g;   p += v          (nesterov: p += momentum v - lr g, with the new v)
 * `v` is passed exactly when momentum > 0.  lr_mul (optional, 0 / 1 per element): an element whose entry is 0 keeps its weight and
 * its slot bit for bit. */
int satcv_sgd_step(float* p, const float* g, float* v, int64_t n, float momentum, int32_t nesterov, float* state,
                   const float* lr_mul, void* stream);
/* tf.keras.optimizers.RMSprop(learning_rate, rho, momentum, epsilon, centered), the arithmetic TensorFlow documents for ApplyRMSProp /
 * ApplyCenteredRMSProp (epsilon INSIDE the root):
 *     ms = rho ms + (1 - rho) g^2;   centered (mg not NULL): mg = rho mg + (1 - rho) g
 *     denom = sqrt(ms - mg^2 + eps)  (mg = 0 when not centered)
 *     mom = momentum mom + lr g / denom;   p -= mom                     (momentum == 0, mom NULL: p -= lr g / denom)
 * `mom` is passed exactly when momentum > 0, `mg` exactly when centered.  state / lr_mul as for SGD. */
int satcv_rmsprop_step(float* p, const float* g, float* ms, float* mg, float* mom, int64_t n, float rho, float momentum, float eps,
                       float* state, const float* lr_mul, void* stream);
/* The `clipvalue` / `global_clipnorm` arguments of every tf.keras optimizer, applied to the flat gradient in place before the step.  Both
 * act on what the optimizer will see, g * grad_scale (state[2]; state NULL: 1).
 *   SATCV_CLIP_VALUE        every element clamped so that |g grad_scale| <= c (a NaN stays a NaN); no workspace.
 *   SATCV_CLIP_GLOBAL_NORM  g *= min(1, c / ||g grad_scale||_2).  The norm is a two-stage sum in double with a fixed partition and a
 *                           fixed order (1024 partials whatever n is, then one workgroup): no floating-point atomics, bit-identical
 *                           from run to run and from stream to stream.  The second stage and the scaling read it from `workspace`
 *                           (satcv_grad_clip_workspace(n) bytes, 8-byte aligned; afterwards double [1024] holds the SQUARED norm of
 *                           g): no host synchronisation.  A gradient at or below the threshold is not written at all.  A non-finite
 *                           norm (NaN or infinity) leaves the gradient as it is: the step is lost either way, as with
 *                           tf.clip_by_global_norm, which marks that case by setting every entry to NaN. */
#define SATCV_CLIP_VALUE 0
#define SATCV_CLIP_GLOBAL_NORM 1
int64_t satcv_grad_clip_workspace(int64_t n);
int satcv_grad_clip(float* g, int64_t n, int32_t mode, float c, const float* state, void* workspace, void* stream);

/* Clears the two buffers a training step accumulates into -- the flat gradient (bytes_a, a multiple of 16, 16-byte aligned) and a small
 * second one (the loss scalar; bytes_b a multiple of 4) -- in ONE launch of the library's own (the optimizer loop of Model.fit,
 * notebooks/UNET_G4G_2019_solar.ipynb:1267: Keras starts every step from zero gradients).  Either may be empty. */
int satcv_zero2(void* a, int64_t bytes_a, void* b, int64_t bytes_b, void* stream);

/* ---------------------------------------------------- data-parallel collectives
 * The reference has no multi-device code; this is the north-star's data-parallel `Model.fit`
 * (notebooks/UNET_G4G_2019_solar.ipynb:1267-1275 run on N replicas): one process per GPU, ONE exchange per step -- the
 * sum of the flat fp32 gradient over the replicas, RCCL over xGMI.  RCCL is bound at run time (dlopen of librccl.so.1, or the
 * path in SATCV_RCCL_LIB): SATCV_ERR_UNSUPPORTED from every entry point below when it cannot be loaded.
 *
 * satcv_comm_unique_id: rank 0 fills 128 bytes and hands them to every rank through any side channel.
 * satcv_comm_init:      collective over all ranks, on the calling thread's CURRENT device; the handle is owned by the
 *                       caller and released with satcv_comm_destroy (also collective).  One communicator per device/process.
 * satcv_allreduce_grads: sum of grads[lo, hi) over the ranks, in place, asynchronous on `stream`, sent in buckets of
 *                       `bucket_elems` floats cut from the END of the range (reverse-layer order: the layers nearest the loss are
 *                       final first) inside one RCCL group.  payload SATCV_F32, or SATCV_BF16: the range is rounded to bf16
 *                       into `scratch` (caller-owned, >= (hi - lo) * 2 bytes), summed in bf16 on the wire (half the bytes: 37 MB
 *                       instead of 74 MB for get_unet_model(2, 4)) and widened back.  The mean is the optimizer's business
 *                       (satcv_adam_step's grad_scale = 1 / world).
 * satcv_allreduce:      in-place sum (average != 0: mean) of `count` elements of SATCV_F32 / SATCV_BF16 / SATCV_F64 -- the
 *                       BatchNorm statistics rows under SyncBN, loss / confusion-matrix scalars at log points. */
#define SATCV_COMM_ID_BYTES 128
typedef struct satcv_comm satcv_comm;
int satcv_comm_unique_id(void* id128);
int satcv_comm_init(satcv_comm** comm_out, int32_t rank, int32_t world, const void* id128);
int satcv_comm_destroy(satcv_comm* comm);
int satcv_comm_info(const satcv_comm* comm, int32_t* rank, int32_t* world);
int satcv_allreduce_grads(satcv_comm* comm, float* grads, int64_t lo, int64_t hi, int64_t bucket_elems, int32_t payload,
                          void* scratch, void* stream);
int satcv_allreduce(satcv_comm* comm, void* buf, int64_t count, int32_t dtype, int32_t average, void* stream);

/* ------------------------------------------------------------ ConvLSTM2D family
 * The reference's LSTM builders (utils/model_tools.py:666-768 build_lstm_layers / build_lstm_layers2, :773-920 get_lstm_model /
 * get_lstm_autoencoder / get_hybrid_model, :1016-1060 get_hierarchical_model) call tf.keras.layers.ConvLSTM2D(filters, [3, 3],
 * padding 'same', activation None, optional dilation_rate on the INPUT convolution).  Per time step
 *     z = conv(x_t, kernel) + bias + conv(h_{t-1}, recurrent_kernel)          (gate order i, f, c, o along the 4 F channels)
 *     i, f, o = rec_act(z_i, z_f, z_o);  g = act(z_c);  c_t = f c_{t-1} + i g;  h_t = o act(c_t)
 * Both convolutions are satcv_conv2d_igemm launches (sequences are stored time-major, so the input convolution of ALL steps is
 * one launch over T * B images); these entry points are the cell arithmetic.
 *
 * satcv_ingest_seq: (B, T, H, W, C) float32 (the Keras input layout) -> (T, B, H, W, cpad) storage type. */
int satcv_ingest_seq(const float* src, void* dst, int32_t batch, int32_t steps, int32_t h, int32_t w_, int32_t c, int32_t cpad,
                     int32_t dtype, void* stream);
typedef struct satcv_lstm_gates_desc {
  /* forward inputs: the two convolution outputs of this step (storage type), (npix, 4 F) with leading dimensions ldx / ldh_g;
   * hg NULL at t = 0 (h_0 = 0); c_prev (npix, F) float32 or NULL (c_0 = 0) */
  const void* xg; int32_t ldx; const void* hg; int32_t ldh_g; const float* c_prev;
  float* c_out;                        /* c_t (npix, F) float32 (backward: c_t as an INPUT)                                       */
  void* h_out; int32_t ldh;            /* h_t (npix, ldh) storage type                                                            */
  void* gates_out;                     /* post-activation (i, f, g, o) (npix, 4 F) storage type: forward output (NULL at inference),
                                          backward input                                                                          */
  satcv_stat_t* stats; int32_t stats_ld;   /* optional BatchNorm statistics of the stored h_t, rows as in satcv_conv_desc           */
  /* backward: dL/dh_t from up to two producers (the layer above; the recurrent data gradient of step t + 1), dc_{t+1 -> t} or NULL */
  const void* dh_a; int32_t lddh_a; const void* dh_b; int32_t lddh_b; const float* dc_next;
  void* dz_out; int32_t lddz;          /* dL/dz_t (npix, lddz >= 4 F) storage type: the dy of both convolutions' gradients        */
  float* dc_prev_out;                  /* dc_{t -> t-1} (npix, F) float32                                                         */
  int64_t npix; int32_t filters;
  int32_t rec_act;                     /* 0 hard_sigmoid = clip(0.2 z + 0.5, 0, 1) (Keras 2.x ConvLSTM2D default), 1 sigmoid (Keras 3) */
  int32_t act;                         /* 0 linear (activation=None, as every reference call site), 1 tanh (the Keras default)    */
  int32_t dtype;
} satcv_lstm_gates_desc;
/* Both refuse filters outside 8, 16, 32, 64, 128, 256 and any leading dimension narrower than its tensor (ldx, ldh_g, lddz >= 4 F; ldh,
 * stats_ld, lddh_a, lddh_b >= F).  The backward takes the hard-sigmoid slope from the STORED gate: 0.2 strictly inside (0, 1), else 0. */
int satcv_convlstm_gates_fwd(const satcv_lstm_gates_desc* d, void* stream);
int satcv_convlstm_gates_bwd(const satcv_lstm_gates_desc* d, void* stream);

/* satcv_convlstm_step_fwd: one ConvLSTM2D INFERENCE step in one launch (utils/model_tools.py:685-720) -- the recurrent 3x3 'same'
 * convolution of h_{t-1} (never dilated: Keras dilates the input kernel only) with the gate arithmetic above as its epilogue:
 *     z = conv3x3(h_prev, w) + xg      (fp32 accumulators, never stored; xg = the input convolution's output, bias inside)
 *     i, f, g, o = ra(z_i), ra(z_f), act(z_c), ra(z_o);   c_t = f c_prev + i g (float32);   h_t = o act(c_t) (storage type)
 * with rec_act / act exactly as in satcv_lstm_gates_desc.  No BatchNorm statistics and no gate stash are produced.
 *
 * Gate-interleaved channel order.  xg (its 4 F channels) and the OUTPUT channels of w are in the order
 *     position  blk * 4 G + gate * G + j   holds natural channel  gate * F + blk * G + j,     G = min(F, 32), blk < F / G, j < G, gate = i, f, c, o
 * (lstm_infer.gate_order(F)): permute the recurrent kernel, the input kernel and the bias with it on the host, then pack as usual --
 * w is the forward image of satcv_pack_weights for the permuted (3, 3, F, 4 F) kernel with cin_pad = F.  h_prev, c_prev, c_out and
 * h_out are in NATURAL channel order.
 *
 * h_prev (n, h, w_, ldh_prev) storage type, NULL at t = 0 (no K loop: z = xg; w is then not read); c_prev (npix, F) float32 or NULL.
 * Refused (error code, satcv_last_error naming convlstm_step_fwd, nothing written): filters other than 16, 32, 64; h_out overlapping
 * h_prev or c_out overlapping c_prev (ping-pong the buffers); ldx < 4 F, ldh < F, ldh_prev < F or any of them not a multiple of 8. */
typedef struct satcv_lstm_step_desc {
  const void* h_prev; int32_t ldh_prev;
  const void* w;
  const void* xg; int32_t ldx;
  const float* c_prev;
  float* c_out;
  void* h_out; int32_t ldh;
  int32_t n, h, w_, filters;
  int32_t rec_act, act, dtype;
} satcv_lstm_step_desc;
int satcv_convlstm_step_fwd(const satcv_lstm_step_desc* d, void* stream);
/* 1 when satcv_convlstm_step_fwd was built for this filter count and storage type, else 0 (host query: a plan decides per layer, once) */
int satcv_convlstm_step_supported(int32_t filters, int32_t dtype);

/* Conv2D(cout <= 16, 1x1) over the channel concatenation of one or two sources -- the `dense` layers and fusion heads of the LSTM
 * family (utils/model_tools.py:797, 847-857, 902-910, 1050-1056).  A source is an NHWC tensor (float32 or bf16) with an optional
 * pending BatchNorm + ReLU and, if hs / ws are set, on a coarser grid that is read through tf.image.resize(..., 'nearest')
 * (half-pixel centres: source index min(floor((i + 0.5) in / out), in - 1)).  activation: 0 softmax (+ argmax classes), 1 sigmoid,
 * 2 linear, 3 ReLU clipped at max_value (max_value <= 0: plain ReLU; layers.ReLU(max_value=2.0) is the reference's default head).
 * Backward: `dout` is dL/d out for activations 2 / 3 (for softmax / sigmoid heads pass the loss kernel's dL/dlogits with activation 2);
 * dw (rows of every source in order, (sum cin, cout)) and db are ACCUMULATED (zero them first); src[i].dx receives the gradient of the
 * source's ACTIVATED values on the source's own grid. */
typedef struct satcv_dense_src {
  const void* x; int32_t ld, cin, dtype;
  const float* in_scale; const float* in_shift; int32_t in_relu;
  int32_t hs, ws;                      /* 0, 0: the output grid                                                                   */
  void* dx; int32_t lddx, dx_dtype;    /* backward output or NULL                                                                 */
} satcv_dense_src;
typedef struct satcv_dense_desc {
  satcv_dense_src src[2]; int32_t nsrc;
  const float* w; const float* b; int32_t cout;
  int32_t activation; float max_value;
  float* out; int32_t* classes; float* z_out;      /* (npix, cout) float32; classes (npix) for softmax or NULL; z_out optional     */
  int64_t npix; int32_t h, w_;                     /* output grid (npix = images * h * w_)                                         */
  const float* dout; float* dz_out; float* dw; float* db;
} satcv_dense_desc;
/* Both validate every source (x, cin > 0, ld >= cin, dtype, hs / ws both zero or both set, in_scale and in_shift together) and the grid
 * (h, w_ > 0, npix a whole number of images); the forward refuses an activation outside 0 .. 3, the backward a dx with lddx < cin or a
 * dx_dtype other than float32 / bf16.  The nearest index is evaluated in float32, floorf((i + 0.5f) * ((float) in / (float) out)). */
int satcv_dense_small_fwd(const satcv_dense_desc* d, void* stream);
int satcv_dense_small_bwd(const satcv_dense_desc* d, void* stream);
/* satcv_dense_scene_fwd: the fusion head of a scene prediction.  It is satcv_dense_small_fwd restricted to the centre crop of every
 * chip, storing straight into the prediction map: the last Conv2D(k, [1, 1]) of get_hybrid_model / get_hierarchical_model
 * (utils/model_tools.py:902-911, 1047-1049) together with the crop and placement of the chip loop of
 * utils/prediction_tools.py:133-156 -- bit-equal to satcv_dense_small_fwd followed by satcv_scene_scatter (accumulate 0), without
 * the (n, h, w_, cout) probability tensor in between and without the arithmetic of the pixels the crop throws away.
 *   head:  sources, w, b, cout, activation, max_value as for satcv_dense_small_fwd; h, w_ the CHIP grid and npix = n * h * w_ (n chips);
 *          out, classes, z_out and the backward fields (dout, dz_out, dw, db, src[i].dx) must be NULL
 *   crop_h x crop_w pixels starting at (crop_y, crop_x) of chip k go to map position origins[first + k] (origins, total, first as for
 *          satcv_scene_scatter), clipped to [0, map_h) x [0, map_w).  A resized source is read through the nearest index of the CHIP
 *          grid (h, w_ against hs, ws) at chip coordinates (crop_y + v, crop_x + u), exactly as satcv_dense_small_fwd reads it
 *   map:   float32 (map_h, map_w, ldm); output channels [c0, c0 + nc) are stored at map channels 0 .. nc - 1 (nc <= ldm)
 *   class_map: optional uint8 (map_h, map_w), the argmax (first of equals) of a softmax head (activation 0 only)
 * Contract: the placed windows of the chips of ONE launch are pairwise disjoint (plain stores, no accumulation).
 * Refused, naming the entry point and writing nothing: a NULL map or origin table, c0 + nc > cout, nc > ldm, a crop outside the chip
 * grid, class_map with a non-softmax activation, first + n > total, a non-NULL head.out / classes / z_out / backward field, and
 * everything satcv_dense_small_fwd refuses of the sources and the grid. */
typedef struct satcv_dense_scene_desc {
  satcv_dense_desc head;
  int32_t crop_y, crop_x, crop_h, crop_w;
  const int32_t* origins; int32_t total, first;
  float* map; int32_t map_h, map_w, ldm, c0, nc;
  uint8_t* class_map;
} satcv_dense_scene_desc;
int satcv_dense_scene_fwd(const satcv_dense_scene_desc* d, void* stream);

/* ------------------------------------------------------- stream utilities */
int satcv_graph_begin(void* stream);
int satcv_graph_end(void* stream, void** graph_exec_out);
int satcv_graph_launch(void* graph_exec, void* stream);
int satcv_graph_destroy(void* graph_exec);
/* event pairs recorded around every igemm launch while enabled; total ms + count returned.  kind (bit of kind_mask): 0 = 3x3 conv
 * forward / data gradient, 1 = 1x1 / transposed-conv GEMMs, 2 = weight gradients, 3 = fused thin-layer backward (data + weight gradient) */
int satcv_prof_enable(int32_t kind_mask);
int satcv_prof_collect(int32_t kind, double* total_ms, int64_t* launches, double* flops);
/* Runtime switches of the library (tests force a tile configuration on small shapes; probes A/B variants in one process).  One table,
 * csrc/options.hpp, declares every one of them; each value comes from its environment variable once, when the library is loaded.
 *   settable      satcv_set_option changes it (not thread-safe against concurrent launches)
 *   startup-only  the environment decides; satcv_set_option returns SATCV_ERR_INVALID (several size workspaces that plans cache)
 *   counter       launches a path has served in this process (tests check the path taken); satcv_set_option returns SATCV_ERR_INVALID
 * satcv_get_option reads any of them.  satcv_option_key(i) enumerates the keys in table order and returns NULL past the end.
 * An unknown key is SATCV_ERR_INVALID.  Keys:
 * "igemm_db"  SATCV_DB, default 1, settable:
 *     0 the single-buffered 128x128 tile (and 32-channel chunks for deep 1x1) only, 1 automatic, 2 the double-buffered
 *     256x128 tile wherever its shape limits allow (profiles/r03_db_vs_single.txt)
 * "igemm_sched"  SATCV_IGEMM_SCHED, default 0, settable:
 *     experiment bits handed to the deep tile (half-chunk stagger, no gain); none wired at present
 * "igemm_thin"  SATCV_THIN, default 1, settable:
 *     persistent weights-stationary kernel of the thin 3x3 layers (conv_igemm_ws.hip, conv_thin_roles.hip): 0 off, 1 / 2 on
 *     wherever the shape limits allow, whatever the batch size
 * "igemm_m16"  SATCV_M16, default 1, settable:
 *     the 16x16x32 deep 3x3 tiles (conv_igemm_m16.hip, conv_igemm_m16p.hip): 0 off, 1 launches that write statistics
 *     (training), 2 every eligible launch; a training plan's tile_policy raises 1 to 2 (profiles/r05_ab_m16_step.txt)
 * "splitk"  SATCV_SPLITK, default 0, settable:
 *     split-K of under-filled plain (halo-tile / 1x1) launches, opt-in because the K order then depends on the workgroup
 *     count: 1 every eligible launch, 2 launches of fewer than 64 workgroups (the DeepLab inference plans;
 *     profiles/r04_ab_splitk.txt)
 * "splitk_tl"  SATCV_SPLITK_TL, default 1, startup-only:
 *     split-K of under-filled tap-loop launches (dilated / strided convolutions); 0 off
 * "convt_wide"  SATCV_CONVT_WIDE, default 1, startup-only:
 *     transposed-conv tiles span several sub-pixel positions (input read once, whole-line stores); 0 one position per tile
 * "wdma"  SATCV_WDMA, default 1, startup-only:
 *     deep 3x3 tile: weights by LDS-DMA into a three-slot ring (profiles/r04_ab_weight_ring_dma.txt); 0 register-staged
 *     weights
 * "db64"  SATCV_DB64, default 1, startup-only:
 *     512-pixel x 64-channel double-buffered tile for 64 output channels with deep K (profiles/r03_ab_late_switches.txt): 0
 *     off, 2 also other multiples of 64, 3 also below 128 input channels
 * "db_tl"  SATCV_DB_TL, default 1, startup-only:
 *     double-buffered 256x128 tap-loop tile with 64-channel chunks (profiles/r04_deeplab_ab_double_buffered_taploop.txt): 0
 *     off, 1 from 96 tiles on, n > 1 from n tiles on
 * "db1x1"  SATCV_DB1X1, default 1, startup-only:
 *     deep 1x1 / transposed convolutions on the double-buffered 256x128 tile (profiles/r03_ab_late_switches.txt); 0 the
 *     single-buffered tile
 * "db1x1_small"  SATCV_DB1X1_SMALL, default 1, startup-only:
 *     ... also where even 128-pixel tiles leave CUs idle (profiles/r04_deeplab_ab_db1x1_small.txt); 0 off
 * "igemm_generic"  SATCV_IGEMM, default 0, startup-only:
 *     SATCV_IGEMM=generic: every convolution on the generic kernel of conv_igemm.hip (ablation; the value is 1 when the word
 *     starts with g)
 * "m16_ws"  SATCV_M16_WS, default 1, startup-only:
 *     wave roles in the one-tile 16x16x32 kernel: 0 never (symmetric kernel), 1 from 256 input channels on, 2 always
 *     (profiles/r05_ablation_m16.txt)
 * "m16p"  SATCV_M16P, default 1, settable:
 *     persistent 16x16x32 kernel: 0 off, 1 where a workgroup gets at least two tiles, 2 every eligible launch
 *     (profiles/r06_ab_m16p_step.txt)
 * "m16p_prio"  SATCV_M16P_PRIO, default 30, settable:
 *     s_setprio of its staging waves, decimal digits (plain launches)(launches with the fused input BatchNorm)(launches with
 *     the fused BatchNorm-backward sums), each 0 ... 3 (30: profiles/r06_ab_m16p_prio_step.txt)
 * "m16p_prio64"  SATCV_M16P_PRIO64, default -1, startup-only:
 *     the same digits for its 64-channel output block; negative: as m16p_prio
 * "m16p_bn64"  SATCV_M16P_BN64, default 1, startup-only:
 *     its 64-channel output block (profiles/r06_ab_m16p_bn64_step.txt); 0 the 64-filter layers stay on the one-tile kernels
 * "thin_roles"  SATCV_THIN_ROLES, default 1, settable:
 *     wave-role kernel of the thin 3x3 layers: 0 off, 1 the shapes it measured faster on, 2 every shape it serves
 *     (profiles/r05_ab_thin_roles_step.txt)
 * "convt_thin"  SATCV_CONVT_THIN, default 1, startup-only:
 *     streaming kernels of the thin transposed convolutions and their data gradient (profiles/r03_ab_convt_thin.txt): 0 off
 *     (tiled kernels), non-zero on, >= 2 also the 64 <- 4 x 32 data gradient, where the tiled kernel measured faster
 * "convt_wps"  SATCV_CONVT_WPS, default 3, startup-only:
 *     waves per SIMD of the 64 -> 4 x 32 forward: 2, anything else 3
 * "convt_mid"  SATCV_CONVT_MID, default 1, startup-only:
 *     256 -> 4 x 128 on the streaming kernel, one position per workgroup; 0 the tiled kernel
 * "wgrad_db"  SATCV_WGRAD_DB, default 1, settable:
 *     double-buffered weight-gradient kernel where its limits allow: 0 the single-buffered one, 2 the 64x128 block for 1x1 /
 *     transposed-conv gradients instead of 128x256
 * "wgrad_m16"  SATCV_WGRAD_M16, default 0, settable:
 *     wgrad_dma_kernel on v_mfma_f32_16x16x32_bf16: measured slower, off (profiles/r06_ab_wgrad_m16.txt)
 * "wgrad_pix256"  SATCV_WGRAD_PIX256, default 1, startup-only:
 *     thin layers stage 256 pixels per step; 0 always 128
 * "wgrad_dma"  SATCV_WGRAD_DMA, default 1, startup-only:
 *     deep 3x3 layers: the 64x128 block with dY by LDS-DMA (profiles/r04_ab_wgrad_dma.txt); 0 the 32x128 block
 * "wgrad_wgs"  SATCV_WGRAD_WGS, default 128, startup-only:
 *     workgroups of a double-buffered weight-gradient launch that shares the chip (profiles/r04_ab_wgrad_workgroups.txt);
 *     below 8 reads as 128
 * "ew_per_cu"  SATCV_EW_PER_CU, default 6, startup-only:
 *     workgroups per CU of the grid-stride elementwise kernels (3 ... 16 within 0.3 % of the step, elementwise.hip); below 1
 *     reads as 6
 * "bn_apply"  SATCV_BN_APPLY, default 1, startup-only:
 *     BatchNorm-backward apply on its own kernel; 0 the round-3 loop for every apply launch (a null in the step:
 *     profiles/r06_ab_env_switches.txt)
 * "bn_rev"  SATCV_BN_REV, default 1, startup-only:
 *     BatchNorm-backward apply walks the pixels in reversed order; 0 forward (ablation of a single kernel choice, DESIGN.md
 *     section 6)
 * "loss_fast"  SATCV_LOSS_FAST, default 1, startup-only:
 *     vectorised softmax cross-entropy kernel for 2 / 4 classes; 0 the general loss kernel
 * "igemm_thin_launches"  no variable, starts at 0, read-only counter:
 *     launches served by the persistent thin-layer kernels (conv_igemm_ws.hip and conv_thin_roles.hip)
 * "thin_roles_launches"  no variable, starts at 0, read-only counter:
 *     ... of them by conv_thin_roles.hip
 * "m16p_launches"  no variable, starts at 0, read-only counter:
 *     launches served by conv_igemm_m16p.hip
 */
int satcv_set_option(const char* key, int32_t value);
int satcv_get_option(const char* key, int32_t* value);
const char* satcv_option_key(int32_t index);

#ifdef __cplusplus
}
#endif
#endif
