/*
 * libpcuda_hip.so -- C ABI of the MI355X (gfx950) kernels behind the PointCloudUDA
 * adversarial train-step hot path.
 *
 * The reference (sulaimanvesal/PointCloudUDA) has no FFI: its "operators" are the ATen
 * ops issued by the modules under src/networks, src/utils/loss.py and the body of train_epoch
 * (src/train_mscmrseg.py:183-330).  Each entry point below names the reference call
 * site(s) it replaces.  The Python host (pointcloududa_amd/) binds these with ctypes and
 * keeps the reference's nn.Module / function signatures on top.
 *
 * Conventions
 *   - all tensors are device pointers owned by the caller; fp32 unless stated otherwise;
 *     image tensors are NCHW with dense HxW planes and explicit batch/channel strides
 *     (in ELEMENTS), so channel slices of concatenated buffers can be passed without copies;
 *   - every launch goes to the caller's hipStream_t (void* here); nothing allocates, frees
 *     or synchronises; scratch memory is passed in (query the size with *_workspace_size);
 *   - return value: 0 = ok, <0 = error (PCUDA_E_*); never throws;
 *   - precision modes for the MFMA convolutions (operands are split on the fly from fp32):
 *       PCUDA_PREC_BF16X3  a = a_hi + a_lo (two bf16), a*b ~= ah*bh + ah*bl + al*bh, fp32 accumulate
 *                          (~2^-17 relative per product: the parity mode, default)
 *       PCUDA_PREC_BF16    single bf16 MFMA per product, fp32 accumulate (throughput mode)
 */
#ifndef PCUDA_HIP_H
#define PCUDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCUDA_OK 0
#define PCUDA_E_BADARG (-1)
#define PCUDA_E_UNSUPPORTED (-2)
#define PCUDA_E_LAUNCH (-3)
#define PCUDA_E_WORKSPACE (-4)

#define PCUDA_PREC_BF16X3 0
#define PCUDA_PREC_BF16 1

typedef void* pcuda_stream_t; /* hipStream_t */

/* library / device ----------------------------------------------------------------- */
/* ABI version of this header.  Bumped whenever an entry point's signature, a struct layout or a workspace contract
 * changes (5, round 5: pcuda_src / pcuda_dst lost the record fields, the record-convolution entries left the library,
 * pcuda_nn_loss_workspace_floats / pcuda_abi_struct_size / pcuda_last_kernel were added).  A binding must refuse a library
 * whose pcuda_version() differs from the PCUDA_ABI_VERSION it was written against, and compare its own struct sizes
 * with pcuda_abi_struct_size: the library reads these structs from caller memory. */
#define PCUDA_ABI_VERSION 5
int pcuda_version(void);
/* sizeof() of an ABI struct as THIS library was compiled: 0 pcuda_conv_geom, 1 pcuda_src, 2 pcuda_dst, 3 pcuda_pooled,
 * 4 pcuda_reduce_job; 0 for an unknown index */
size_t pcuda_abi_struct_size(int which);
int pcuda_device_count(void);            /* hipGetDeviceCount, 0 when no GPU */
const char* pcuda_last_error(void);      /* text of the last failing call on this thread */
const char* pcuda_build_hash(void);      /* sha256[:16] of the kernel sources the loaded library was compiled from */
long long pcuda_launch_count(int reset); /* kernel launches issued by this library since the last reset (host-side count) */
/* convolution launches that ran on a generic fallback kernel because the geometry's specialised template instantiation is
 * not in this build (csrc/variants.h: the default build holds the variants of the benchmark configurations and tests) */
long long pcuda_fallback_count(void);
/* "<shape tag> | <kernel>" of the most recent convolution launch issued by the calling thread (the tag a profile row
 * carries, and which kernel family the dispatcher picked for it: igemm_pipe / igemm8 / igemm_generic / wgrad[+fallback] /
 * wgrad3 / wgrad3r / wgrad1 / direct ...): lets a kernel-level test assert WHICH kernel produced the result it checks */
const char* pcuda_last_kernel(void);
/* measurement aid (bench.py `clock_ghz_under_load`): 512 workgroups x 4 waves issue `iters` x 4 back-to-back 32x32x16 bf16
 * MFMAs; out2_dev[0] / out2_dev[1] receive the summed shader-clock (s_memtime) and 100-MHz reference-clock (s_memrealtime)
 * ticks of every workgroup's first wave: shader GHz = 0.1 * out2[0] / out2[1].  sink_dev: one float (never written). */
int pcuda_clock_probe(unsigned long long* out2_dev, float* sink_dev, int iters, pcuda_stream_t s);

/* kernel-family timing (HIP events recorded on the launch stream around every launch of
 * a family while enabled; used by bench.py for the live roofline figure) */
#define PCUDA_FAM_CONV_FWD 0   /* implicit-GEMM forward + dgrad launches */
#define PCUDA_FAM_CONV_WGRAD 1
#define PCUDA_FAM_POINTWISE 2
#define PCUDA_FAM_DENSE_F32 3 /* exact-fp32 MFMA k=1 Conv1d of PointNetCls (forward, dgrad, wgrad): fp32 matrix peak, not bf16 */
#define PCUDA_FAM_COUNT 4
int pcuda_prof_enable(int on);
int pcuda_prof_reset(void);
/* synchronises the recorded events; ms = summed kernel time, work = summed algorithmic
 * FLOPs (conv families) or bytes (pointwise), launches = number of launches */
int pcuda_prof_read(int family, double* ms, double* work, long long* launches);
/* writes one CSV row per recorded launch (family, work, ms, shape tag) */
int pcuda_prof_dump(const char* path);
/* timing experiments only (PCUDA_DBG bit 128): the eight per-phase cycle sums the pipelined forward/dgrad
 * kernel accumulates (barrier, X commit, issue, weight copy, barrier, MFMA, epilogue, loop tail); read + reset */
int pcuda_debug_read_clocks(unsigned long long* out8);

/* ------------------------------------------------------------------------------------
 * 2-D convolution: replaces nn.Conv2d forward/backward at
 *   unet.py:23,27,32 (encoder 3x3 / 1x1), :61 (dilated bottleneck), :85 (6x6 head),
 *   :112,116,122 (decoder), :178 (classifier); GAN.py:97-107 (4x4 s2 p2, 3x3 s2 p1).
 * cross-correlation, square kernel, symmetric padding, one dilation, groups = 1.
 * ---------------------------------------------------------------------------------- */
typedef struct pcuda_conv_geom {
  int n;            /* batch */
  int cin, cout;
  int in_h, in_w;   /* LOGICAL input plane (after the optional x2 upsample) */
  int out_h, out_w; /* = floor((in + 2*pad - dil*(k-1) - 1)/stride) + 1 */
  int k, stride, pad, dil;
  int in_up;        /* 1: the stored input is (in_h/2 x in_w/2) and is read through a nearest x2
                       upsample (folds nn.UpsamplingNearest2d, unet.py:111, into the conv) */
} pcuda_conv_geom;

/* source / destination that may be split across two tensors along channels
 * (zero-copy torch.cat(dim=1): unet.py:46,134).  c1 = channels taken from p1; the rest come
 * from p2 (p2 may be NULL when c1 == total).  scale/shift: optional per-channel affine
 * applied on load to in-bounds elements (fused BatchNorm apply), NULL = identity. */
typedef struct pcuda_src {
  const float* p1; long long sn1, sc1; const float* scale1; const float* shift1;
  const float* p2; long long sn2, sc2; const float* scale2; const float* shift2;
  int c1;
} pcuda_src;
typedef struct pcuda_dst {
  float* p1; long long sn1, sc1;
  float* p2; long long sn2, sc2;
  int c1;
} pcuda_dst;

/* packed-weight sizes (bytes) for a given geometry / precision */
size_t pcuda_conv2d_packed_fwd_bytes(const pcuda_conv_geom* g, int prec);
size_t pcuda_conv2d_packed_dgrad_bytes(const pcuda_conv_geom* g, int prec);
/* repack fp32 OIHW weights into the MFMA-fragment layout [co-tile][ci-chunk][tap][row][record]; record =
 * 32 hi | 32 lo | 8 pad bf16 (144 bytes) in PCUDA_PREC_BF16X3, 32 values + 8 pad (80 bytes) in PCUDA_PREC_BF16.
 * Opaque to the caller (sizes from the two queries above); call once per optimiser step */
int pcuda_conv2d_pack_fwd(const pcuda_conv_geom* g, int prec, const float* w, void* packed, pcuda_stream_t s);
int pcuda_conv2d_pack_dgrad(const pcuda_conv_geom* g, int prec, const float* w, void* packed, pcuda_stream_t s);
/* both repacks in ONE launch (forward layout + every dgrad parity class -- for k = 4 / stride 2 / pad 2 one image per ROW
 * parity with the two column classes interleaved row by row; the layout is the library's business: size it with
 * pcuda_conv2d_packed_dgrad_bytes and hand it back to pcuda_conv2d_dgrad); packed_dgrad may be NULL */
int pcuda_conv2d_pack_all(const pcuda_conv_geom* g, int prec, const float* w, void* packed_fwd, void* packed_dgrad,
                          pcuda_stream_t s);
/* Batched repack (one launch for all layers of a network after an optimiser step): fill the job records of a layer
 * (forward layout + every dgrad parity class; packed_dgrad may be NULL) into host memory -- returns the number of jobs
 * written (<= 1 + stride^2) or <0; job_blocks[j] = workgroups job j needs.  Keep the concatenated records in DEVICE
 * memory next to an int table first_block[j] (exclusive prefix sum of job_blocks over all jobs) and replay them with
 * pcuda_conv2d_pack_table (total_blocks = the sum).  The records hold the raw pointers given here. */
size_t pcuda_conv2d_pack_job_bytes(void);
int pcuda_conv2d_pack_jobs_fill(const pcuda_conv_geom* g, int prec, const float* w, void* packed_fwd, void* packed_dgrad,
                                void* host_jobs, int max_jobs, int* job_blocks);
int pcuda_conv2d_pack_table(const void* dev_jobs, const int* dev_first_block, int njobs, int total_blocks, pcuda_stream_t s);

/* 1: pcuda_conv2d_forward takes this geometry (the discriminators' first layer, GAN.py:97: k = 4, stride 2, pad 2, <= 5
 * input channels, 64 outputs) on the direct MFMA kernel that reads the 4x4 taps straight from the image -- the caller then
 * skips the unfold (pcuda_unfold_taps) + 1x1 form of the layer */
int pcuda_conv2d_d1_forward_ok(const pcuda_conv_geom* g);
/* y = lrelu(conv(x) + bias, slope)   (slope = 1 -> no activation; bias may be NULL)
 * bn_partials (optional): per-tile partial sums [ntiles][cout][2] (sum, sum of squares) of the
 * activated output, for the BatchNorm that follows (unet.py:26,30); ntiles from
 * pcuda_conv2d_fwd_tiles().  Deterministic (no atomics). */
int pcuda_conv2d_fwd_tiles(const pcuda_conv_geom* g, int prec);
int pcuda_conv2d_forward(const pcuda_conv_geom* g, int prec, const pcuda_src* x, const void* packed_w,
                         const float* bias, float slope, const pcuda_dst* y, float* bn_partials,
                         pcuda_stream_t s);
/* dx (+)= conv_transpose(dy): the data gradient; for stride 2 this is the transposed
 * convolution the adversarial gradient takes back through the discriminators.
 * dy: [n][cout][out_h][out_w] given as a pcuda_src (c1 = cout); dx may be split like a cat.
 * When g->in_up is set, dx is the gradient of the UPSAMPLED (logical) input. */
int pcuda_conv2d_dgrad(const pcuda_conv_geom* g, int prec, const pcuda_src* dy, const void* packed_w_dgrad,
                       const pcuda_dst* dx, int accumulate, pcuda_stream_t s);
/* The same data gradient with the BatchNorm-backward reduce of the layer in front of this convolution fused into its
 * epilogue (unet.py:23-30: conv -> LeakyReLU -> BN -> conv; the second convolution's dx IS the first BatchNorm's incoming
 * gradient): red_partials[tile][cin][2] = (sum g, sum g * (a - mean) * invstd) over the tile's stored gradient g, the
 * input of pcuda_bn_bwd_finalize with ntiles = pcuda_conv2d_dgrad_tiles().  Stride-1 layers whose rows are multiples of
 * 4 pixels; returns PCUDA_E_UNSUPPORTED otherwise (run pcuda_conv2d_dgrad + pcuda_bn_bwd_reduce instead). */
int pcuda_conv2d_dgrad_tiles(const pcuda_conv_geom* g, int prec);
int pcuda_conv2d_dgrad_bnred(const pcuda_conv_geom* g, int prec, const pcuda_src* dy, const void* packed_w_dgrad,
                             const pcuda_dst* dx, int accumulate, const float* a, long long a_sn, long long a_sc,
                             const float* mean, const float* invstd, float* red_partials, pcuda_stream_t s);
/* dx = pcuda_conv2d_dgrad(dy) * (a > 0 ? 1 : slope): the LeakyReLU backward of the layer in FRONT of this convolution
 * (GAN.py:97-108, conv -> LeakyReLU(0.2) -> conv going back) in the data-gradient kernel's epilogue; the gradient with respect
 * to the activation is never stored.  a: the saved activation [n][cin][in_h][in_w], plane stride a_sc == dx->sc1, one
 * destination.  PCUDA_E_UNSUPPORTED where a launch of the layer takes the transposed (16-byte store) epilogue: the caller runs
 * pcuda_conv2d_dgrad + pcuda_lrelu_bwd instead (a partly written dx is overwritten by them). */
int pcuda_conv2d_dgrad_lrelu(const pcuda_conv_geom* g, int prec, const pcuda_src* dy, const void* packed_w_dgrad,
                             const pcuda_dst* dx, const float* a, long long a_sn, long long a_sc, float slope,
                             pcuda_stream_t s);
/* The data gradient of a layer behind the nearest-x2 fold (g->in_up: the decoder's up-convolutions, unet.py:111-112) written at
 * the STORED, half resolution: dx_half[n][cin][in_h/2][in_w/2] = the 2x2 block sums of the logical gradient (what
 * pcuda_upsample2_bwd computes from pcuda_conv2d_dgrad's output, without that 4x larger tensor going through HBM).  a != NULL:
 * the BatchNorm-backward reduce of the layer that produced the stored tensor rides along as in pcuda_conv2d_dgrad_bnred
 * (red_partials[pcuda_conv2d_dgrad_tiles()][cin][2]).  PCUDA_E_UNSUPPORTED for plans off the 32 x 8-tile transposed epilogue. */
int pcuda_conv2d_dgrad_fold(const pcuda_conv_geom* g, int prec, const pcuda_src* dy, const void* packed_w_dgrad,
                            const pcuda_dst* dx_half, const float* a, long long a_sn, long long a_sc, const float* mean,
                            const float* invstd, float* red_partials, pcuda_stream_t s);
/* dw (+)= sum over batch and space of dy (x) x ; db (+)= sum dy (db may be NULL).
 * workspace: pcuda_conv2d_wgrad_workspace_size() bytes. */
size_t pcuda_conv2d_wgrad_workspace_size(const pcuda_conv_geom* g);
int pcuda_conv2d_wgrad(const pcuda_conv_geom* g, int prec, const pcuda_src* x, const float* dy,
                       long long dy_sn, long long dy_sc, float* dw, float* db, int accumulate,
                       void* workspace, size_t workspace_bytes, pcuda_stream_t s);

/* The same weight gradient with its split-K reduce DEFERRED: the partial sums stay in `workspace` (which must live
 * until the reduce has run) and *job describes the reduce; pcuda_wgrad_reduce_batch runs the reduces of many layers in
 * one launch (host array of jobs; same per-output arithmetic and order as pcuda_conv2d_wgrad, bit-identical results).
 * A backward pass issues one weight gradient per layer; no two jobs of one batch may name the same dw.
 * job->ksplit == 0 on return: the layer's kernel wrote dw itself, nothing to reduce. */
#define PCUDA_REDUCE_MAX_JOBS 56
typedef struct {
  const float* partial;      /* [ksplit][numel] */
  long long numel;
  float* dw;
  const float* db_partial;   /* [ksplit][nb] or NULL */
  long long nb;
  float* db;
  int ksplit, nkg, accumulate, ntaps;
} pcuda_reduce_job;
int pcuda_conv2d_wgrad_partial(const pcuda_conv_geom* g, int prec, const pcuda_src* x, const float* dy,
                               long long dy_sn, long long dy_sc, float* dw, float* db, int accumulate,
                               void* workspace, size_t workspace_bytes, pcuda_reduce_job* job, pcuda_stream_t s);
int pcuda_wgrad_reduce_batch(const pcuda_reduce_job* host_jobs, int njobs, pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * BatchNorm (training mode) around LeakyReLU: conv -> LeakyReLU -> BatchNorm2d
 * (unet.py:23-30,116-125); also BatchNorm1d of PointNetCls.py (hw = points or 1).
 * ---------------------------------------------------------------------------------- */
/* reduce per-tile partials -> mean, invstd, scale = gamma*invstd, shift = beta - mean*scale;
 * running stats updated with momentum (unbiased variance), torch semantics. count = n*h*w.
 * count == 1: var = 0 (unbiased = var), scale = 0 and shift = beta -- the output is the constant beta */
int pcuda_bn_finalize(const float* partials, int ntiles, int c, long long count, const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                      float* mean, float* invstd, float* scale, float* shift, pcuda_stream_t s);
/* partial sums of a tensor a[n][c][hw] (for layers whose producer is not a conv epilogue);
 * returns ntiles written through *ntiles (query with partials == NULL) */
int pcuda_bn_stats(const float* a, long long sn, long long sc, int n, int c, long long hw,
                   float* partials, int* ntiles, pcuda_stream_t s);
/* y = a*scale[c] + shift[c]; ``flags``: PCUDA_BN_APPLY_RELU then relu (PointNetCls.py:41-43); PCUDA_BN_APPLY_FMA
   rounds once, fmaf(a, scale, shift), as the convolutions apply a pending BatchNorm in their load (a sub-module that
   returns a block output computes what the next layer of the fused network would read); without it a*scale is
   rounded before the add */
#define PCUDA_BN_APPLY_RELU 1
#define PCUDA_BN_APPLY_FMA 2
int pcuda_bn_apply(const float* a, long long a_sn, long long a_sc, const float* scale, const float* shift,
                   int flags, float* y, long long y_sn, long long y_sc, int n, int c, long long hw,
                   pcuda_stream_t s);
/* backward of [z -> a = lrelu(z, slope) -> y = BN(a)] given dy (optionally dy + dy2):
 * pass 1: per-tile partials of (sum dy, sum dy*xhat) -> red[ntiles][c][2]
 * pass 2 (after pcuda_bn_bwd_finalize): dz = lrelu'(a) * scale*(dy - mean_dy - xhat*mean_dyxhat)
 * post_relu: the block is BN -> ReLU instead (PointNetCls): dy is first masked by (y > 0) and
 * `act_slope` applies to nothing (a is then the BN input). */
int pcuda_bn_bwd_reduce(const float* dy, long long dy_sn, long long dy_sc, const float* dy2, long long dy2_sn,
                        long long dy2_sc, const float* a, long long a_sn, long long a_sc, const float* mean,
                        const float* invstd, const float* scale, const float* shift, int post_relu, int n, int c,
                        long long hw, float* red, int* ntiles, pcuda_stream_t s);
/* count < 0: the statistics were FROZEN (eval-mode BatchNorm, nn.BatchNorm2d.eval() in a fine-tuning run: mean / invstd
 * from the running buffers): coef then describes the fixed affine (dz = m * c0 * dy), dgamma / dbeta are unchanged */
int pcuda_bn_bwd_finalize(const float* red, int ntiles, int c, long long count, const float* gamma,
                          const float* invstd, const float* mean, float* dgamma, float* dbeta, int accumulate,
                          float* coef /* [c][3]: dz = m*(c0*dy + c1*a + c2) */, pcuda_stream_t s);
int pcuda_bn_bwd_apply(const float* dy, long long dy_sn, long long dy_sc, const float* dy2, long long dy2_sn,
                       long long dy2_sc, const float* a, long long a_sn, long long a_sc, const float* coef,
                       const float* scale, const float* shift, int post_relu, float act_slope, float* dz,
                       long long dz_sn, long long dz_sc, int n, int c, long long hw, pcuda_stream_t s);
/* dz = dy * (a > 0 ? 1 : slope)   (LeakyReLU backward from the saved OUTPUT, as the in-place
 * nn.LeakyReLU of unet.py:24 / GAN.py:108 does); optional second addend dy2 */
int pcuda_lrelu_bwd(const float* dy, long long dy_sn, long long dy_sc, const float* dy2, long long dy2_sn,
                    long long dy2_sc, const float* a, long long a_sn, long long a_sc, float slope, float* dz,
                    long long dz_sn, long long dz_sc, int n, int c, long long hw, pcuda_stream_t s);
/* per-channel sum over batch and space (bias gradients) db (+)= sum dz */
int pcuda_channel_sum(const float* dz, long long sn, long long sc, int n, int c, long long hw, float* db,
                      int accumulate, float* workspace, size_t workspace_bytes, pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * pooling / resampling / adds (unet.py:48 MaxPool2d(2,2); :111 UpsamplingNearest2d backward)
 * ---------------------------------------------------------------------------------- */
/* y = maxpool2x2(x*scale + shift) with argmax code (0..3) saved as uint8 */
int pcuda_maxpool2_fwd(const float* x, long long x_sn, long long x_sc, const float* scale, const float* shift,
                       float* y, long long y_sn, long long y_sc, uint8_t* idx, int n, int c, int h, int w,
                       pcuda_stream_t s);
/* dx (+)= scatter(dy (+ dy2)) through idx; positions not selected get 0 (or keep when accumulate) */
int pcuda_maxpool2_bwd(const float* dy, long long dy_sn, long long dy_sc, const float* dy2, long long dy2_sn,
                       long long dy2_sc, const uint8_t* idx, float* dx, long long dx_sn, long long dx_sc,
                       int accumulate, int n, int c, int h, int w, pcuda_stream_t s);
/* The backward kernels behind a max-pool, with the pool's scatter read IN PLACE (round 4): the gradient of element (y, x) is
 * g[y/2][x/2] (+ g2) where idx[y/2][x/2] == 2 (y & 1) + (x & 1), else 0 -- what pcuda_maxpool2_bwd would have written into a
 * 4x larger tensor for these kernels to read back (unet.py:48 going back into :27-36 / the residual convolution).  `dy` is an
 * optional full-resolution addend (the skip connection's gradient); results equal the two-kernel form bit for bit. */
typedef struct pcuda_pooled {
  const float* g; long long g_sn, g_sc;     /* gradient at the pooled resolution [n][c][h/2][w/2] (strided planes) */
  const float* g2; long long g2_sn, g2_sc;  /* optional second share, summed (NULL: none) */
  const uint8_t* idx;                       /* dense [n][c][h/2][w/2], from pcuda_maxpool2_fwd */
  int h, w;                                 /* the FULL-resolution plane, both even */
} pcuda_pooled;
int pcuda_bn_bwd_reduce_pooled(const pcuda_pooled* pool, const float* dy, long long dy_sn, long long dy_sc, const float* a,
                               long long a_sn, long long a_sc, const float* mean, const float* invstd, int n, int c,
                               float* red, int* ntiles, pcuda_stream_t s);
int pcuda_bn_bwd_apply_pooled(const pcuda_pooled* pool, const float* dy, long long dy_sn, long long dy_sc, const float* a,
                              long long a_sn, long long a_sc, const float* coef, float act_slope, float* dz, long long dz_sn,
                              long long dz_sc, int n, int c, pcuda_stream_t s);
int pcuda_lrelu_bwd_pooled(const pcuda_pooled* pool, const float* dy, long long dy_sn, long long dy_sc, const float* a,
                           long long a_sn, long long a_sc, float slope, float* dz, long long dz_sn, long long dz_sc, int n,
                           int c, pcuda_stream_t s);
/* dx[h][w] (+)= sum of the 2x2 block of dy[2h][2w] (nearest-upsample backward) */
int pcuda_upsample2_bwd(const float* dy, long long dy_sn, long long dy_sc, float* dx, long long dx_sn,
                        long long dx_sc, int accumulate, int n, int c, int h, int w, pcuda_stream_t s);
/* ... with the BatchNorm-backward reduce of the layer that consumes dx fused in (the decoder's conv -> LeakyReLU -> BN
 * blocks, unet.py:116-125, going back): red[ntiles][c][2] = (sum g, sum g * (a - mean) * invstd) per workgroup, the input of
 * pcuda_bn_bwd_finalize; red == NULL only reports ntiles */
int pcuda_upsample2_bwd_bnred(const float* dy, long long dy_sn, long long dy_sc, float* dx, long long dx_sn,
                              long long dx_sc, int accumulate, const float* a, long long a_sn, long long a_sc,
                              const float* mean, const float* invstd, float* red, int* ntiles, int n, int c, int h, int w,
                              pcuda_stream_t s);
/* bilinear resize, align_corners = True (nn.UpsamplingBilinear2d(size=(224, 224)) in OutputDiscriminator, GAN.py:57,78):
 * y dense [n][c][oh][ow]; ATen's arithmetic (src = dst * (in-1)/(out-1)).  bwd: dx = J^T dy, gather form (deterministic) */
int pcuda_bilinear_fwd(const float* x, long long x_sn, long long x_sc, int n, int c, int h, int w, float* y, int oh,
                       int ow, pcuda_stream_t s);
int pcuda_bilinear_bwd(const float* dy, int n, int c, int oh, int ow, float* dx, long long dx_sn, long long dx_sc,
                       int h, int w, pcuda_stream_t s);
/* taps unfolded into channels (u: dense [n][c*k*k][oh][ow]); a k x k layer over few input channels becomes a 1x1
 * layer over c*k*k of them (the discriminators' first layer, GAN.py:96 / :120-124) */
int pcuda_unfold_taps(const float* x, long long x_sn, long long x_sc, int n, int c, int h, int w, int k, int stride,
                      int pad, int dil, float* u, int oh, int ow, pcuda_stream_t s);
/* y = a + b (+ c) (+ d), flat fp32 (bottleneck running sum, unet.py:68-73; gradient joins) */
int pcuda_add4(const float* a, const float* b, const float* c, const float* d, float* y, long long numel,
               pcuda_stream_t s);
/* y = a * b, flat fp32 (applies a precomputed nn.Dropout mask, PointNetCls.py:179,209) */
int pcuda_mul(const float* a, const float* b, float* y, long long numel, pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * losses / entropy (train_mscmrseg.py:202-203,222-226; train_mmwhs.py:212-224,242; loss.py)
 * ---------------------------------------------------------------------------------- */
#define PCUDA_ACT_SIGMOID 0
#define PCUDA_ACT_SOFTMAX 1
/* e = -p*log(p + 1e-7) * norm, p = sigmoid|softmax(logits); optionally also writes p */
int pcuda_entropy_fwd(const float* logits, int mode, float norm, float* ent, float* prob, int n, int c,
                      long long hw, pcuda_stream_t s);
/* dlogits (+)= d(ent)/dlogits . dent  (+ dprob through p when dprob != NULL) */
int pcuda_entropy_bwd(const float* logits, int mode, float norm, const float* dent, const float* dprob,
                      float* dlogits, int accumulate, int n, int c, long long hw, pcuda_stream_t s);
/* the same with the gradient of the map's mean on top: dmean (device scalar, may be NULL) is d/d[mean over n and pixels of
 * sum_c ent] -- the entropy terms of train_mmwhs.py:225-230 (-etpls) and :243-247 (-Tetpls); every element receives
 * dmean / (n * hw) in addition to its dent (which may then be NULL) */
int pcuda_entropy_bwd2(const float* logits, int mode, float norm, const float* dent, const float* dprob, const float* dmean,
                       float* dlogits, int accumulate, int n, int c, long long hw, pcuda_stream_t s);
/* out[0] = scale * sum(x[0..numel)), fixed summation order (deterministic): torch.mean(torch.sum(uncertainty_map, dim=1))
 * of train_mmwhs.py:225,243 with scale = 1 / (n * hw) */
size_t pcuda_sum_all_workspace_size(void);
int pcuda_sum_all(const float* x, long long numel, double scale, float* out, void* workspace, size_t workspace_bytes,
                  pcuda_stream_t s);
/* segmentation loss: mode SIGMOID: BCE(sigmoid(o), y) + jaccard(sigmoid(o), y)
 *                    mode SOFTMAX: cross_entropy(softmax(o), argmax y) ("double softmax") + jaccard(softmax(o), y)
 * y: one-hot uint8 [n][c][hw].  out[0] = bce|ce, out[1] = jaccard.  workspace from *_workspace_size.
 * c = 1..8 (PCUDA_E_UNSUPPORTED above).  pass 1 (fwd) leaves the per-class sums and the coefficient pairs 1 / U_c, I_c / U_c^2
 * in the workspace; bwd reads the pairs there.  (csrc/losses.hip: the overlap kernels of csrc/loss_device.h with the Jaccard
 * policy; csrc/dice_loss.hip runs the same kernels with the Dice policy) */
size_t pcuda_seg_loss_workspace_size(int n, int c, long long hw);
int pcuda_seg_loss_fwd(const float* logits, const uint8_t* onehot, int mode, int n, int c, long long hw,
                       float* out2, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* dlogits = g_main * d(bce|ce)/do + g_jac * d(jaccard)/do */
int pcuda_seg_loss_bwd(const float* logits, const uint8_t* onehot, int mode, int n, int c, long long hw,
                       const float* g_main, const float* g_jac, float* dlogits, const void* workspace,
                       pcuda_stream_t s);
/* mean BCE-with-logits against a constant label; acc (optional) = mean(sigmoid(x) >= .5)
 * (train_mscmrseg.py:224-226,270-273) */
int pcuda_bce_const_fwd(const float* x, long long numel, float label, float* loss, float* acc, pcuda_stream_t s);
int pcuda_bce_const_bwd(const float* x, long long numel, float label, const float* gout, float gscale, float* dx,
                        pcuda_stream_t s);
/* batch_NN_loss (loss.py:40-76): x,y [b][npts][3]; loss scalar; workspaces: idx_ws int32 [2][b][npts],
 * val_ws float [pcuda_nn_loss_workspace_floats(b, npts)] = [2][b][npts] + [2][b][ceil(npts / 64)] (partial sums of the
 * minima per block of 64 points; ABI 5: ask the library instead of sizing it by formula) */
size_t pcuda_nn_loss_workspace_floats(int b, int npts);
int pcuda_nn_loss_fwd(const float* x, const float* y, int b, int npts, float* loss, int* idx_ws, float* val_ws,
                      pcuda_stream_t s);
int pcuda_nn_loss_bwd(const float* x, const float* y, int b, int npts, const int* idx_ws, const float* val_ws,
                      const float* gout, float* dx, pcuda_stream_t s);
/* per-step host metric moved on-device (utils.py:32-40 + metric.py:5-36): hard = (o == max_c o);
 * dice = mean_{c>=1} (2*sum(y*hard)+1)/(sum y + sum hard + 1).  workspace: 3*c doubles. */
int pcuda_dice_metric(const float* logits, const uint8_t* onehot, int n, int c, long long hw, float* dice,
                      void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* loader-side batch assembly (data_generator_mmwhs.py:265-272, utils.py:7-29, crop_volume :134-137): centre crop
 * (crop = the generator's crop_size, 0 = none), channel-last -> channel-first and integer labels -> one-hot uint8
 * in one pass.  images_hwc [b][h][w][c] fp32, mask_labels [b][h][w] int32 (may be NULL together with onehot),
 * outputs images_chw [b][c][oh][ow], onehot [b][num_classes][oh][ow] */
int pcuda_assemble_batch(const float* images_hwc, const int* mask_labels, int b, int h, int w, int c, int crop,
                         int num_classes, float* images_chw, uint8_t* onehot, pcuda_stream_t s);
/* batch-global minimum and maximum of an fp32 buffer (data_generator_mmwhs.py:246-247) -> out2[0] = min, out2[1] = max,
 * device floats, no host read; NaNs are skipped.  workspace: pcuda_minmax_workspace_size() bytes */
size_t pcuda_minmax_workspace_size(void);
int pcuda_minmax(const float* x, long long numel, float* out2, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* fp32 -> uint8 with the device (min, max) pair pcuda_minmax wrote (data_generator_mmwhs.py:248-249), in fp32 with every
 * operation rounded on its own: q = trunc(((x - min) * 255) / (max - min)) clamped to [0, 255]; max == min gives 0
 * everywhere (0 / 0 in the reference), a NaN element gives 0.  The integers PCUDA_AUG_MINMAX below quantises each gathered
 * texel to, written out, so that the uint8 stages can run between the quantisation and the warp.  No host read, no
 * workspace; x and q 16-byte aligned take the wide path, anything else one element per lane. */
int pcuda_quantize_u8(const float* x, long long numel, const float* minmax, uint8_t* q, pcuda_stream_t s);
/* device-side light augmentation fused with the batch assembly above (light_aug data_generator_mmwhs.py:87-122 +
 * :245-274; simple_aug data_generator_mscmrseg.py:135-167 + :305-317): per sample one inverse 2x3 matrix
 * inv_mats[b][6] (float64, device; output pixel (x, y) of the FULL image -> source coordinate
 * sx = m0 x + m1 y + m2, sy = m3 x + m4 y + m5: flips and the affine composed on the host), order[b] (0 = nearest
 * floor(s + 0.5), anything else = bilinear in float64 with cval for a neighbour outside the image) and cval[b] (0..255),
 * all device arrays.  images_hwc [b][h][w][c] fp32, or uint8 when images_u8.  rescale:
 *   PCUDA_AUG_NONE    fp32: the values themselves are interpolated (no quantisation); uint8: float(q')
 *   PCUDA_AUG_MINMAX  fp32 only, minmax = device (min, max): q = trunc((x - min) * 255 / (max - min)) as uint8, warp,
 *                     out = min + float(q') * (max - min) / 255, all fp32; max == min gives q = 0, so every output = min
 *   PCUDA_AUG_DIV255  uint8 only: float(q') / 255
 * where q' = floor(v + 0.5) clipped to [0, 255].  Labels take order 0 and fill 0 whatever the image's order and cval.
 * Outputs (each may be NULL, not all): images_chw [b][c][oh][ow] fp32 and onehot [b][num_classes][oh][ow] over the centre
 * crop (crop as in pcuda_assemble_batch); over the full image full_mask [b][h][w] uint8 (label > 0: what the point-cloud
 * sampler reads), labels_full [b][h][w] int32 and images_u8_full [b][h][w][c] (uint8 input only).  With identity
 * matrices and PCUDA_AUG_NONE the cropped outputs are pcuda_assemble_batch's bit for bit. */
#define PCUDA_AUG_NONE 0
#define PCUDA_AUG_MINMAX 1
#define PCUDA_AUG_DIV255 2
int pcuda_augment_assemble(const void* images_hwc, int images_u8, const int* mask_labels, int b, int h, int w, int c, int crop,
                           int num_classes, const double* inv_mats, const int* order, const int* cval, int rescale,
                           const float* minmax, float* images_chw, uint8_t* onehot, uint8_t* full_mask, int* labels_full,
                           uint8_t* images_u8_full, pcuda_stream_t s);
/* the second half of the min-max round trip for images that are uint8 already (pcuda_quantize_u8, then any uint8 stages):
 * pcuda_augment_assemble on uint8 images with out = min + float(q') * (max - min) / 255 in fp32 (data_generator_mmwhs.py:254);
 * minmax = the device (min, max) pair, required.  Every other argument and output as above. */
int pcuda_augment_assemble_dequant(const uint8_t* images_hwc, const int* mask_labels, int b, int h, int w, int c, int crop,
                                   int num_classes, const double* inv_mats, const int* order, const int* cval,
                                   const float* minmax, float* images_chw, uint8_t* onehot, uint8_t* full_mask,
                                   int* labels_full, uint8_t* images_u8_full, pcuda_stream_t s);
/* device-side photometric augmentation: the photometric operators of ImageProcessor.augmentation2
 * (data_generator_mscmrseg.py:87-132; called at :305-309) on uint8 images [b][h][w][c], c = 1..4, as a per-sample program
 * of `slots` (0..8) slots in device memory: opcode [b][slots], iarg [b][slots][4], farg [b][slots][16] (float64),
 * seed [b][slots] (64-bit Philox key).  The value is uint8 between two slots; float64 arithmetic in a fixed order,
 * floor(v + 0.5) clipped to [0, 255]; reflect-101 borders, the median replicates.  Per opcode:
 *   PCUDA_PHOTO_NOP             copy (so does an unknown opcode: the host validates programs)
 *   PCUDA_PHOTO_GAUSSIAN_BLUR   iarg[0] = radius 0..12, farg[0..radius] = normalised weights w[|d|] (computed on the host);
 *                               rows, then columns on the unrounded values: t = x[0] w[0]; d = r..1: t += (x[-d] + x[d]) w[d]
 *   PCUDA_PHOTO_AVERAGE_BLUR    iarg[0] = k 2..7, offsets -(k / 2) .. k - k / 2 - 1, (2 S + k k) / (2 k k) in integers
 *   PCUDA_PHOTO_MEDIAN_BLUR     iarg[0] = odd k 3..11, replicated border
 *   PCUDA_PHOTO_CONV3X3         farg[0..8]: correlation, taps summed row-major from 0 (Sharpen, Emboss)
 *   PCUDA_PHOTO_GAUSSIAN_NOISE  farg[0] = scale, iarg[0] = per_channel: v + scale z, z = Box-Muller in float64 of the first
 *                               two words of Philox4x32-10(key = seed, counter = element index; pixel index if !per_channel)
 *   PCUDA_PHOTO_DROPOUT         iarg[0] = per_channel, iarg[1] = threshold (uint32 bits): 0 iff the first word < threshold
 *   PCUDA_PHOTO_COARSE_DROPOUT  the same on an iarg[2] x iarg[3] grid, cell ((y h') / h, (x w') / w)
 *   PCUDA_PHOTO_INVERT          iarg[0] = channel bit mask: 255 - v
 *   PCUDA_PHOTO_ADD             iarg[ch]: clipped integer add
 *   PCUDA_PHOTO_MULTIPLY        farg[ch]: floor(v m + 0.5) clipped
 *   PCUDA_PHOTO_GRAYSCALE       farg[0] = alpha, c = 3 (channel 0 = red): g = 0.299 c0 + 0.587 c1 + 0.114 c2,
 *                               (1 - alpha) v + alpha g; c = 1: copy
 * The result depends on (image, program) only, never on the launch geometry.  `in` is never written and in == out is
 * rejected; slots == 0 copies.  workspace: pcuda_photometric_workspace_size bytes, 16-byte aligned, needed for slots > 1. */
#define PCUDA_PHOTO_NOP 0
#define PCUDA_PHOTO_GAUSSIAN_BLUR 1
#define PCUDA_PHOTO_AVERAGE_BLUR 2
#define PCUDA_PHOTO_MEDIAN_BLUR 3
#define PCUDA_PHOTO_CONV3X3 4
#define PCUDA_PHOTO_GAUSSIAN_NOISE 5
#define PCUDA_PHOTO_DROPOUT 6
#define PCUDA_PHOTO_COARSE_DROPOUT 7
#define PCUDA_PHOTO_INVERT 8
#define PCUDA_PHOTO_ADD 9
#define PCUDA_PHOTO_MULTIPLY 10
#define PCUDA_PHOTO_GRAYSCALE 11
size_t pcuda_photometric_workspace_size(int b, int h, int w, int c);
int pcuda_photometric(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode,
                      const int* iarg, const double* farg, const unsigned long long* seed, void* workspace,
                      size_t workspace_bytes, pcuda_stream_t s);
/* device-side geometric augmentation: the warps of ImageProcessor.augmentation (data_generator_mscmrseg.py:20-84; called at
 * :305-309) on uint8 images [b][h][w][c], c = 1..4, h, w >= 2, and optional int32 labels [b][h][w], as a per-sample program
 * of `slots` (0..8) slots in device memory: opcode [b][slots], iarg [b][slots][4], farg [b][slots][32] (float64),
 * seed [b][slots] (64-bit Philox key).  Every slot is one resampling, one launch; the value is uint8 again between two slots.
 * A slot computes a source coordinate (sx, sy) per output pixel (x, y) in float64 and samples there:
 *   iarg[0]  order: 0 = the texel at floor(s + 0.5); anything else = bilinear over (floor(s), floor(s) + 1), summed as
 *            pcuda_augment_assemble sums, floor(v + 0.5) clipped to [0, 255]
 *   iarg[1]  border mode per neighbour index: PCUDA_GEO_CONSTANT (cval = iarg[2]), _EDGE, _REFLECT (no edge repeat),
 *            _SYMMETRIC, _WRAP; anything else behaves as constant
 * Labels take order 0 and constant 0 at the same coordinate.  A NaN coordinate or one with |s| > 2^30 takes cval (labels 0)
 * in every mode; indices are folded in integers before any load.  Per opcode:
 *   PCUDA_GEO_NOP               copy (so does an unknown opcode: the host validates programs)
 *   PCUDA_GEO_HOMOGRAPHY        farg[0..8] = inverse 3x3 map h, row-major: d = (h6 x + h7 y) + h8,
 *                               sx = ((h0 x + h1 y) + h2) / d, sy = ((h3 x + h4 y) + h5) / d
 *   PCUDA_GEO_ELASTIC           iarg[3] = radius r 0..4, farg[0] = alpha, farg[1..1+r] = one-sided normalised weights;
 *                               noise 2 u - 1, u = (word + 0.5) 2^-32 of words 0 (dx) and 1 (dy) of Philox4x32-10
 *                               (key = seed, counter = y w + x), reflect-101 outside the image; blurred along y, then
 *                               along x (t = n[0] w[0]; d = r..1: t += (n[-d] + n[d]) w[d]); sx = x + alpha bx, sy = y + alpha by
 *   PCUDA_GEO_PIECEWISE_AFFINE  iarg[3] = G 2..4, farg[i G + j] / farg[16 + i G + j] = source x / y of control point (i, j)
 *                               of the regular G x G grid over [0, w-1] x [0, h-1]; cells split along the TL-BR diagonal
 * The result depends on (image, program) only, never on the launch geometry.  `in` (labels_in) is never written and
 * in == out is rejected; labels_in and labels_out are both NULL or both given; slots == 0 copies.  workspace:
 * pcuda_geometric_workspace_size bytes, 16-byte aligned, needed for slots > 1. */
#define PCUDA_GEO_NOP 0
#define PCUDA_GEO_HOMOGRAPHY 1
#define PCUDA_GEO_ELASTIC 2
#define PCUDA_GEO_PIECEWISE_AFFINE 3
#define PCUDA_GEO_CONSTANT 0
#define PCUDA_GEO_EDGE 1
#define PCUDA_GEO_REFLECT 2
#define PCUDA_GEO_SYMMETRIC 3
#define PCUDA_GEO_WRAP 4
size_t pcuda_geometric_workspace_size(int b, int h, int w, int c, int with_labels);
int pcuda_geometric(const uint8_t* in, uint8_t* out, const int* labels_in, int* labels_out, int b, int h, int w, int c,
                    int slots, const int* opcode, const int* iarg, const double* farg, const unsigned long long* seed,
                    void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* pcuda_geometric with a third sampling order (f8b): the same arguments, rules and workspace, but iarg[0] == 3 is the Keys
 * cubic convolution with A = -0.75 over the 4 x 4 neighbours floor(s) - 1 .. floor(s) + 2 (0 stays nearest, anything else
 * bilinear).  For t = s - floor(s), u = t + 1, r = 1 - t, in float64, every operation rounded on its own:
 *   wm = ((A u - 5 A) u + 8 A) u - 4 A;  w0 = ((A + 2) t - (A + 3)) t t + 1;  w1 = ((A + 2) r - (A + 3)) r r + 1;
 *   w2 = ((1 - wm) - w0) - w1
 * The border mode folds each of the eight neighbour indices (constant: cval per tap); a row is
 * ((p[-1] wxm + p[0] wx0) + p[1] wx1) + p[2] wx2, the four rows are summed likewise with the y weights, floor(v + 0.5)
 * clipped to [0, 255].  A kernel instance of its own: pcuda_geometric keeps its registers and samples order 3 bilinearly. */
int pcuda_geometric_cubic(const uint8_t* in, uint8_t* out, const int* labels_in, int* labels_out, int b, int h, int w, int c,
                          int slots, const int* opcode, const int* iarg, const double* farg, const unsigned long long* seed,
                          void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* device-side stylize augmentation: the three entries of the reference's SomeOf lists that pcuda_photometric and
 * pcuda_geometric do not hold (data_generator_mscmrseg.py:46, 57-60, 69) on uint8 images [b][h][w][c], c = 1..4, as a per-sample
 * program of `slots` (0..8) slots in device memory: opcode [b][slots], iarg [b][slots][12], farg [b][slots][16] (float64),
 * table [b][slots][768] (float64: three coarse grids of up to 16 x 16 values, row-major, grid k at offset 256 k), seed
 * [b][slots] (64-bit Philox key).  The value is uint8 between two slots.  rdiv(a, b) = floor((2 a + b) / (2 b)).  Per opcode:
 *   PCUDA_STYLE_NOP                  copy (so does an unknown opcode: the host validates programs)
 *   PCUDA_STYLE_HUE_SATURATION       c = 3 (channel 0 = red; any other c copies), iarg[0] = dh, iarg[1] = ds, integers only:
 *                                    V = max, d = V - min, S = rdiv(255 d, V) (0 if V = 0), H = 0 if d = 0 else
 *                                    (base + rdiv(30 num, d)) mod 180, (base, num) = (0, g - b) if V == r, (60, b - r) if V == g,
 *                                    else (120, r - g); H' = (H + dh) mod 180 >= 0, S' = clip(S + ds, 0, 255); sec = H' / 30,
 *                                    F = H' % 30, p = rdiv(V (255 - S'), 255), q = rdiv(V (7650 - S' F), 7650),
 *                                    t = rdiv(V (7650 - S' (30 - F)), 7650); (r, g, b) by sector 0..5 = (V,t,p), (q,V,p),
 *                                    (p,V,t), (p,q,V), (t,p,V), (V,p,q)
 *   PCUDA_STYLE_NOISE_ALPHA_CONV3X3  iarg[0] = n 1..3 grids, iarg[1] = upscale (0 nearest: cell ((y h') / h, (x w') / w);
 *                                    1 bilinear: sy = (y + 0.5) h' / h - 0.5 clamped to [0, h' - 1], rows g00 (1 - fx) + g01 fx,
 *                                    then top (1 - fy) + bot fy; 3 cubic: the same sy, sx unclamped, the weights and the
 *                                    summation order of pcuda_geometric_cubic, every tap index clamped into the grid, the
 *                                    value clipped to [0, 1]; 2 is no upscale), iarg[2] = aggregation (0 min, 1 mean in grid order, 2 max),
 *                                    iarg[3] = sigmoid on: m = 1 / (1 + exp(-(20 (m - 0.5) - farg[9]))), iarg[4 + 2 k],
 *                                    iarg[5 + 2 k] = h', w' of grid k (2..16); farg[0..8] = 3x3 correlation as
 *                                    PCUDA_PHOTO_CONV3X3, e = its rounded result; out = floor((1 - m) x + m e + 0.5) clipped;
 *                                    float64 in this order, one m for all channels
 *   PCUDA_STYLE_SUPERPIXELS          iarg[0], iarg[1] = gy, gx (gy gx <= 256), iarg[2] = updates 0..10, iarg[3] = M2
 *                                    (compactness squared), iarg[4] = threshold (uint32 bits); integers only.  Centre
 *                                    k = j gx + i starts at (((2j+1) h) / (2 gy), ((2i+1) w) / (2 gx)) with that pixel's colour; a
 *                                    pixel takes, among the centres of the 3x3 grid cells around its cell ((y gy) / h,
 *                                    (x gx) / w) that exist, the smallest 64-bit D = dc2 S2 + M2 ds2 (S2 = max(1, (h w) / (gy gx))),
 *                                    ties to the lowest k; update: centre = rdiv(sum, n) of colour, y, x (n = 0: stays); after
 *                                    the updates and one last assignment segment k takes its mean colour rdiv(sum, n) iff the
 *                                    first word of Philox4x32-10(key = seed, counter = k) < threshold, else it is copied
 * The result depends on (image, program) only, never on the launch geometry.  `in` is never written and in == out is
 * rejected; slots == 0 copies.  workspace: pcuda_stylize_workspace_size bytes, 16-byte aligned, needed for slots > 0 (a
 * uint8 label plane and the second image of the ping-pong). */
#define PCUDA_STYLE_NOP 0
#define PCUDA_STYLE_HUE_SATURATION 1
#define PCUDA_STYLE_NOISE_ALPHA_CONV3X3 2
#define PCUDA_STYLE_SUPERPIXELS 3
size_t pcuda_stylize_workspace_size(int b, int h, int w, int c);
int pcuda_stylize(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode, const int* iarg,
                  const double* farg, const double* table, const unsigned long long* seed, void* workspace,
                  size_t workspace_bytes, pcuda_stream_t s);
/* connected superpixels (csrc/spx_connect.hip): pcuda_stylize with an opt-in connectivity pass behind SUPERPIXELS slots, the
 * counterpart of skimage's enforce_connectivity = True with min_size_factor = 0.5 under iaa.Superpixels.  Same parameters and
 * status codes as pcuda_stylize; a SUPERPIXELS slot additionally reads iarg[5] = min_size (pcuda_stylize never does):
 *   iarg[5] <= 0  the slot is pcuda_stylize's, bit for bit; so is every slot of another opcode
 *   iarg[5] >= 1  (values above h w act as h w) on the label plane of the last assignment: the 4-connected components of equal
 *                 labels (label 0 is an ordinary label) get as id the index r = y w + x of their raster-first pixel; a
 *                 component is small iff its own pixel count < min_size and r != 0; a small component's target is the
 *                 component of pixel r - 1 if x > 0, else of pixel r - w (another component, id below r); targets are followed
 *                 until a component that is not small: the final id of the pixels on the way (merged pixels count towards
 *                 nobody's size).  All pixels of one final id form a 4-connected segment; it takes rdiv(sum, n) of the slot's
 *                 input per channel iff the first word of Philox4x32-10(key = seed, counter = final id) < iarg[4], else its
 *                 pixels are copied.  min_size = 1 merges nothing and recolours per piece.  Integers only; this build's own
 *                 convention (parity with skimage's _enforce_label_connectivity_cython is unpinned; no max_size split, no
 *                 8-connectivity; the downscale to 128 pixels is pcuda_stylize_scaled's)
 * h w <= 2^24 (32-bit segment sums; PCUDA_E_BADARG above).  workspace: pcuda_stylize_connect_workspace_size bytes, 16-byte
 * aligned, needed for slots > 0, each part rounded up to 16 bytes: [pcuda_stylize_workspace_size bytes, laid out as
 * pcuda_stylize's] [parents int32 b h w] [component sizes uint32 b h w] [segment sums uint32 b h w (c + 1): colour sums, then the
 * pixel count, at the index of the final id]; 0 for non-positive dims. */
size_t pcuda_stylize_connect_workspace_size(int b, int h, int w, int c);
int pcuda_stylize_connect(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode,
                          const int* iarg, const double* farg, const double* table, const unsigned long long* seed,
                          void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* superpixels at a working size (csrc/spx_scale.hip): pcuda_stylize_connect with an opt-in max_size on SUPERPIXELS slots, the
 * counterpart of iaa.Superpixels' max_size = 128.  Same parameters and status codes as pcuda_stylize_connect (iarg[5] is
 * honoured on every SUPERPIXELS slot); a SUPERPIXELS slot additionally reads iarg[6] = max_size = m (pcuda_stylize and
 * pcuda_stylize_connect never do).  With L = max(h, w):
 *   m <= 0 or L <= m  the slot is pcuda_stylize_connect's, bit for bit; so is every slot of another opcode
 *   m >= 1 and L > m  (a SCALED slot) working size h' = max(1, (h m) / L), w' = max(1, (w m) / L) (integer division).  Linear
 *                     resize R(src[Sh x Sw x c] -> Dh x Dw), per axis with source size S, destination size D and destination
 *                     index d: a = clip((2 d + 1) S - D, 0, 2 D (S - 1)), i0 = a / (2 D), t = a - 2 D i0, i1 = min(i0 + 1, S - 1);
 *                     num = (2 Dh - ty) ((2 Dw - tx) p00 + tx p01) + ty ((2 Dw - tx) p10 + tx p11), den = 4 Dh Dw, value =
 *                     floor((2 num + den) / (2 den)) (64-bit integers).  small = R(slot input -> h' x w'); the grid SLIC of
 *                     pcuda_stylize runs on small with h', w' in place of h, w everywhere and, for iarg[5] >= 1, the
 *                     connectivity rule above on the working-size label plane (ids and counters r = y w' + x); the repaint
 *                     over the pixels of small gives painted; out = R(painted -> h x w), except that a sample none of whose
 *                     final segments that hold a pixel is replaced gets the slot's input, bit for bit.  Integers only; this
 *                     build's own convention (parity with imgaug, cv2 and skimage is unpinned)
 * h w <= 2^24 (PCUDA_E_BADARG above).  workspace: pcuda_stylize_scaled_workspace_size bytes, 16-byte aligned, needed for
 * slots > 0, each part rounded up to 16 bytes: [pcuda_stylize_connect_workspace_size bytes, laid out as
 * pcuda_stylize_connect's] [working images uint8 b h w c] [painted working images uint8 b h w c] [one int32 per sample: a
 * segment was replaced]; 0 for non-positive dims. */
size_t pcuda_stylize_scaled_workspace_size(int b, int h, int w, int c);
int pcuda_stylize_scaled(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode,
                         const int* iarg, const double* farg, const double* table, const unsigned long long* seed,
                         void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* device-side CropAndPad with every defined mode of numpy.pad: iaa.CropAndPad(percent=(-0.05, 0.1), pad_mode=ia.ALL,
 * pad_cval=(0, 255)) of both heavy recipes (data_generator_mscmrseg.py:28-32, 91-95; csrc/croppad.hip) on uint8 images
 * [b][h][w][c], c = 1..4, h, w >= 2, and optional int32 labels [b][h][w], as a per-sample program in device memory: opcode [b]
 * (0 copy, 1 crop-and-pad; anything else copies) and iarg [b][6] = (top, right, bottom, left, mode, cval): signed pixels per
 * side, positive pads (at most 64), negative crops; mode PCUDA_PAD_*; cval 0..255.  For a live sample
 *   xc = x[ct : h - cb, cl : w - cr] (the negative sides), I = numpy.pad(xc, ((pt, pb), (pl, pr), (0, 0)), mode), Hi x Wi, with
 *   constant_values = cval (constant), end_values = cval (linear_ramp), the statistics over the whole axis; bit for bit numpy's
 *   (tests/golden/croppad.npz): axis 0 is padded first and axis 1 on the padded array (a corner is a statistic of statistics,
 *   or a ramp whose edge value is a ramp); mean and median round half to even; a ramp is floor(end + k step), k = 0 outermost,
 *   step = (edge - end) / width, unless some edge value of that side (all columns and channels of the numpy call) equals end:
 *   then floor(end + (k / width) (edge - end)), numpy.linspace's any_step_zero branch
 *   out = I resized to h x w: ax = Wi / w, sx = (x + 0.5) ax - 0.5 (float64, every operation rounded on its own), x0 = floor(sx),
 *   wx1 = sx - x0, neighbour indices clamped into I, y likewise; v = 0; v += p00 wy0 wx0; v += p01 wy0 wx1; v += p10 wy1 wx0;
 *   v += p11 wy1 wx1; floor(v + 0.5) clipped to [0, 255].  Hi == h and Wi == w give I itself
 *   labels: the same crop, constant 0, the texel at floor(s + 0.5), whatever the image's mode is
 * I is never materialised.  Sides and modes are clamped on the device before any load (the host validates programs).  The
 * result depends on (image, program) only.  `in` (labels_in) is never written and in == out is rejected; labels_in and
 * labels_out are both NULL or both given.  workspace: pcuda_crop_pad_workspace_size bytes, 16-byte aligned, always needed (per
 * sample and channel the column and row statistics, per sample the four ramp flags); 0 for dims the entry point refuses.
 * Three launches; nothing allocates or synchronises. */
#define PCUDA_PAD_CONSTANT 0
#define PCUDA_PAD_EDGE 1
#define PCUDA_PAD_LINEAR_RAMP 2
#define PCUDA_PAD_MAXIMUM 3
#define PCUDA_PAD_MEAN 4
#define PCUDA_PAD_MEDIAN 5
#define PCUDA_PAD_MINIMUM 6
#define PCUDA_PAD_REFLECT 7
#define PCUDA_PAD_SYMMETRIC 8
#define PCUDA_PAD_WRAP 9
size_t pcuda_crop_pad_workspace_size(int b, int h, int w, int c);
int pcuda_crop_pad(const uint8_t* in, uint8_t* out, const int* labels_in, int* labels_out, int b, int h, int w, int c,
                   const int* opcode, const int* iarg, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* device-side histogram matching: match_histograms(img, reference_img, multichannel=True) of the MM-WHS generator
 * (data_generator_mmwhs.py:174-176, 236-237; train_mmwhs.py -mh) on images [b][h][w][c], c = 1..4, fp32 or uint8 (is_u8),
 * against a template that is fixed for the run and arrives as tables in device memory: tvalues / tquantiles [c][tstride]
 * (float64; per channel the template's sorted distinct values tv and tq = cumsum(counts) / M) and tlen[c] (1..tstride valid
 * entries; clamped into that range on the device).  Per plane (b, c) of N = h w values and per value s:
 *   cnt = #{s' in the plane : s' <= s} (-0.0 and +0.0 are one value), q = double(cnt) / double(N)
 *   j = the last index with tq[j] <= q;  j < 0: tv[0];  j == len - 1: tv[len - 1];  tq[j] == q: tv[j];  otherwise
 *   slope = (tv[j+1] - tv[j]) / (tq[j+1] - tq[j]), r = slope (q - tq[j]) + tv[j]
 * every operation rounded separately in float64 (np.unique / np.cumsum / np.interp; the library is built with
 * -ffp-contract=off).  fp32 images store float(r) (round to nearest even); uint8 images store uint8(trunc(r)) and want a
 * uint8 template (r stays in [0, 255]; the host checks that, the device clips).  NaN in an image is unsupported (the
 * reference's result is garbage there too); +-inf are ordinary values.  fp32: each plane's order-preserving 32-bit keys are
 * sorted in the workspace (one workgroup per plane: LSD radix sort, 8-bit digits, four passes) and every value finds cnt by
 * binary search; uint8: a 256-bin histogram and a 256-entry LUT per plane, no workspace.  Integer atomics only: the same
 * bits from run to run.  Never allocates, never synchronises; `in` is never written and in == out is rejected; b h w == 0 is
 * a no-op returning 0.  workspace: pcuda_match_hist_workspace_size bytes (8 per fp32 value; 0 for uint8), 16-byte aligned. */
size_t pcuda_match_hist_workspace_size(int b, int h, int w, int c, int is_u8);
int pcuda_match_hist(const void* in, void* out, int is_u8, int b, int h, int w, int c, const double* tvalues,
                     const double* tquantiles, const int* tlen, int tstride, void* workspace, size_t workspace_bytes,
                     pcuda_stream_t s);
/* histogram matching against a BANK of r references kept on the device (csrc/histmatch_bank.hip): sample i of the batch is
 * matched to reference ref_index[i] -- a source image against a target image drawn from a pool, or against this step's target
 * batch.  Same definition and the same bits as pcuda_match_hist with the tables of that reference; no host sort, no upload.
 *
 * pcuda_hist_bank_build: refs[r][rh][rw][c] (fp32, or uint8 when is_u8), c = 1..4 -> bank, pcuda_hist_bank_size bytes:
 *   fp32: per plane (r, c) of M = rh rw values its SORTED order-preserving 32-bit keys k[0..M) (4 bytes per value; one
 *   workgroup per plane, the sort of pcuda_match_hist; workspace: pcuda_hist_bank_workspace_size bytes, the second buffer of
 *   the sort's ping-pong, free after the call's kernels ran).  -0.0 is stored as +0.0.  uint8: per plane 256 uint32 counts, no
 *   workspace.  Non-finite reference values are unsupported: *flag (device int32) is set to 0 by the call and to 1 by the
 *   kernel when it meets one; the call never reads it.  A bank is rebuilt in place by calling again.
 * pcuda_match_hist_bank: in[b][h][w][c] -> out of the same dtype (is_u8: uint8 images AND a uint8 bank; else fp32 images and
 *   an fp32 bank); ref_index: device int32 [b], every entry clamped into [0, r) on the device.  rh rw need not equal h w.
 *   fp32, per value after its own rank search (cnt, q = double(cnt) / double(N) as above), with E(p) = double(p) / double(M)
 *   and val(key) = the float the key came from, widened to float64:
 *     e* = max{e in [0, M] : E(e) <= q} (decided by the division; trunc(q M) is only a first guess);
 *     p = e* if e* == 0, e* == M or k[e*-1] != k[e*], else lower_bound(k, k[e*]) (the last run end at or below e*);
 *     p == 0: r = val(k[0]);  p == M: r = val(k[M-1]);  otherwise q0 = E(p), v0 = val(k[p-1]); q0 == q: r = v0; else
 *     p1 = upper_bound(k, k[p]), q1 = E(p1), v1 = val(k[p]), slope = (v1 - v0) / (q1 - q0), r = slope (q - q0) + v0,
 *   every operation rounded separately in float64; the store is float(r), nearest even.  uint8: the image plane's histogram
 *   and scan as pcuda_match_hist; the 256 counts of the sample's reference are scanned and compacted into tq / tv in LDS, then
 *   the same interpolation, truncation into a 256-entry LUT, one gather.
 *   workspace: pcuda_match_hist_bank_workspace_size bytes (8 per fp32 image value; 0 for uint8), 16-byte aligned.
 * Both: integer atomics only, the same bits from run to run; never allocate, never synchronise; inputs are never written
 * (in == out, refs == bank are rejected); an empty batch (b h w == 0) or an empty set (r rh rw == 0 in the build) is a no-op
 * returning 0; a bank or workspace that is short or not 16-byte aligned is PCUDA_E_WORKSPACE. */
size_t pcuda_hist_bank_size(int r, int rh, int rw, int c, int is_u8);
size_t pcuda_hist_bank_workspace_size(int r, int rh, int rw, int c, int is_u8);
int pcuda_hist_bank_build(const void* refs, int is_u8, int r, int rh, int rw, int c, void* bank, size_t bank_bytes, int* flag,
                          void* workspace, size_t workspace_bytes, pcuda_stream_t s);
size_t pcuda_match_hist_bank_workspace_size(int b, int h, int w, int c, int is_u8);
int pcuda_match_hist_bank(const void* in, void* out, int is_u8, int b, int h, int w, int c, const void* bank, int r, int rh,
                          int rw, const int* ref_index, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* Fourier domain adaptation against a BANK of r target images kept on the device (csrc/fourier.hip): the low-frequency block of
 * every source plane's amplitude spectrum is replaced by the target's, the source phase is kept.  The rule is this build's own
 * statement of FDA, written with numpy's FFT; the public FDA code (its beta-to-radius convention, its torch variant) is not
 * vendored by the reference: parity with it is unpinned.  Per plane (sample, channel) of a source s[h][w] and the same channel
 * of a target t[h][w] of the SAME size, in float64:
 *   S = fft2(s), T = fft2(t); the block is the (2 radius + 1)^2 bins with frequencies -radius..radius on both axes (rows and
 *   columns floor(h/2) - radius .. floor(h/2) + radius, likewise w, of the fftshift-ed array); S' = S outside the block and
 *   S'[k] = |T[k]| exp(1j angle(S[k])) inside it (angle(0) = 0); v = real(ifft2(S')).
 * Computed as v = s + real(sum over block bins of D[k] e^{+2 pi i (ky y / h + kx x / w)}) / (h w) with D[k] = (|T[k]| - |S[k]|)
 * S[k] / |S[k]| (|T[k]| where S[k] == 0) by a partial DFT over kx = 0..radius, ky = -radius..radius (Hermitian symmetry: the
 * bins kx >= 1 count twice); all arithmetic float64, every operation rounded on its own, twiddles from sincospi of an
 * integer-reduced (k x) mod n.  It differs from the full-FFT form by summation order only (1e-9 on 0..255 images is generous).
 * fp32 images store float(v), nearest even, or float(min(max(v, clip_lo), clip_hi)) when clip; uint8 images store
 * uint8(min(max(rint(v), 0), 255)), rint half to even.  A bin whose |S[k]| is rounding noise (an image constant along one
 * axis) has an arbitrary phase here as in numpy: no floor is added.  NaN and inf are unsupported.
 *
 * pcuda_fourier_bank_build: refs[r][h][w][c] (fp32, or uint8 when is_u8), c = 1..4 interleaved -> bank, pcuda_fourier_bank_size
 *   bytes: per plane (r, c) the float64 amplitudes |T[ky][kx]|, ky = -radius..radius, kx = 0..radius (half of the block: t is
 *   real).  workspace: pcuda_fourier_bank_workspace_size bytes (per-band partial spectra), free after the call's kernels ran.
 *   A bank is rebuilt in place by calling again.  Two launches.
 * pcuda_fourier_adapt: in[b][h][w][c] -> out of the same dtype; bank as the build left it for r references of the same h, w, c
 *   and radius (either dtype).  ref_index: device int32 [b]; sample i is adapted to reference ref_index[i]; an entry >= r is
 *   clamped to r - 1; a NEGATIVE entry passes the sample through bit for bit (how a loader applies the stage with a
 *   probability).  sample_radius: device int32 [b] or NULL (the bank's radius for every sample); an entry is clamped into
 *   [0, radius]; radius 0 swaps the DC bin only.  workspace: pcuda_fourier_adapt_workspace_size bytes.  Three launches.
 * Both: no atomics, every sum in a fixed order: the same bits from run to run; never allocate, never synchronise; inputs are
 * never written (in == out, refs == bank are rejected, PCUDA_E_BADARG); b h w == 0 (r h w == 0) is a no-op returning 0; a bank
 * or workspace that is short or not 16-byte aligned is PCUDA_E_WORKSPACE; radius > 32, 2 radius + 1 > min(h, w) (the bins
 * would alias), c outside 1..4 and a side above 4096 are PCUDA_E_UNSUPPORTED.  The size queries return 0 for such dims. */
size_t pcuda_fourier_bank_size(int r, int c, int radius);
size_t pcuda_fourier_bank_workspace_size(int r, int h, int w, int c, int radius);
int pcuda_fourier_bank_build(const void* refs, int is_u8, int r, int h, int w, int c, int radius, void* bank, size_t bank_bytes,
                             void* workspace, size_t workspace_bytes, pcuda_stream_t s);
size_t pcuda_fourier_adapt_workspace_size(int b, int h, int w, int c, int radius);
int pcuda_fourier_adapt(const void* in, void* out, int is_u8, int b, int h, int w, int c, const void* bank, int r, int radius,
                        const int* ref_index, const int* sample_radius, int clip, double clip_lo, double clip_hi, void* workspace,
                        size_t workspace_bytes, pcuda_stream_t s);
/* device-side slice preparation of the MS-CMRSeg data (utils/read_nii_image.py:60-74 preprocess_volume, used at :100, 137,
 * 176 behind RescaleIntensity -> uint8, the nearest resize to 256 and the centre crop to 224; csrc/preprocess.hip).  Parity
 * with OpenCV / ITK is unpinned: the convention below is this build's own, written after OpenCV's clahe.cpp and ITK's
 * RescaleIntensityImageFilter, and pinned by two independent restatements in tests/golden/preprocess.npz.
 *
 * pcuda_clahe: cv2.createCLAHE(clipLimit, tileGridSize=(tiles_x, tiles_y)).apply on uint8 slices in[n][h][w].
 *   histSize = 256.  Extended size: w % tiles_x == 0 and h % tiles_y == 0: (eh, ew) = (h, w); otherwise eh = h + (tiles_y -
 *   h % tiles_y) and ew = w + (tiles_x - w % tiles_x) (OpenCV's quirk: a divisible axis still grows by a whole `tiles` when
 *   the other one is indivisible), BORDER_REFLECT_101 at the bottom / right (index reflection in the histogram kernel: no
 *   padded copy is written).  th = eh / tiles_y, tw = ew / tiles_x, T = th tw; clip = 0 if clip_limit <= 0 else
 *   max(int(clip_limit T / 256), 1) (double, on the host); lutScale = float(255) / float(T), inv_tw = 1.0f / float(tw),
 *   inv_th likewise (fp32, on the host).
 *   Per tile: the 256-bin histogram; if clip > 0: clipped = sum(max(hist[i] - clip, 0)), hist = min(hist, clip), batch =
 *   clipped / 256, residual = clipped - 256 batch (integers), every bin gains batch, and if residual != 0, step = max(256 /
 *   residual, 1) and bin i gains 1 iff i % step == 0 and i / step < residual (the closed form of OpenCV's loop);
 *   lut[i] = clamp(rint(float(cumsum_i) lutScale), 0, 255), rint to nearest even.
 *   Per pixel (y, x) of value v: txf = float(x) inv_tw - 0.5f, tx1 = floor(txf), xa = txf - float(tx1), xa1 = 1.0f - xa, then
 *   tx2 = min(tx1 + 1, tiles_x - 1), tx1 = max(tx1, 0); y likewise; res = (L[ty1][tx1][v] xa1 + L[ty1][tx2][v] xa) ya1 +
 *   (L[ty2][tx1][v] xa1 + L[ty2][tx2][v] xa) ya, every operation rounded separately in fp32 (-ffp-contract=off); the output
 *   is clamp(rint(res), 0, 255).
 *   out_mode PCUDA_CLAHE_U8: uint8 out[n][h][w]; PCUDA_CLAHE_F32X3: fp32 out[n][3][h][w] = float(u8) / 255.0f in all three
 *   channels (cv2.imread of a grey PNG, / 255., moveaxis: what the networks take).
 *   1 <= tiles <= 16 per axis, h, w >= 2 (up to 32768), every pad <= dim - 1 (the reflection is defined), T < 2^24, else
 *   PCUDA_E_BADARG.  workspace: pcuda_clahe_workspace_size bytes (the LUTs [n][tiles_y][tiles_x][256]), 16-byte aligned.
 *
 * pcuda_rescale_resize_crop_u8: the front of read_*_nii_save_png in one pass over the output: in[n][sh][sw] of in_dtype
 * (PCUDA_PRE_F32 / _I16 / _U8) -> uint8 out[n][oh][ow].  lo / hi = the volume's minimum / maximum, reduced on the device
 * (integer atomics on order-preserving keys, no host round trip).  Rescale after ITK, in double, every operation rounded
 * separately: scale = 255 / (hi - lo) if hi != lo, else 255 / hi if hi != 0, else 0; shift = -lo scale;
 * u8 = clamp(trunc(double(v) scale + shift), 0, 255).  Nearest resize after cv2.INTER_NEAREST: sy = min(int(floor(y ify)),
 * sh - 1), ify = 1.0 / (double(resize_h) / double(sh)), x likewise (the identity when resize == source size).  Centre crop
 * (crop_volume): rows resize_h / 2 - crop / 2 .. resize_h / 2 + crop / 2 of the resized slice, columns likewise, so
 * oh = ow = 2 (crop / 2); crop = 0: none, (oh, ow) = (resize_h, resize_w).  A crop window outside the resized slice is
 * PCUDA_E_BADARG.  NaN in the volume is unsupported.  PCUDA_PRE_U8_RAW: a uint8 volume whose values are kept as they are
 * (no rescale: resize_volume / crop_volume on their own).  workspace: pcuda_rescale_resize_crop_u8_workspace_size bytes.
 *
 * Both: never allocate, never synchronise; `in` is never written and in == out is rejected; n == 0 is a no-op returning 0;
 * integer atomics only: the same bits from run to run. */
#define PCUDA_CLAHE_U8 0
#define PCUDA_CLAHE_F32X3 1
#define PCUDA_PRE_F32 0
#define PCUDA_PRE_I16 1
#define PCUDA_PRE_U8 2
#define PCUDA_PRE_U8_RAW 3
size_t pcuda_clahe_workspace_size(int n, int tiles_x, int tiles_y);
int pcuda_clahe(const uint8_t* in, void* out, int n, int h, int w, double clip_limit, int tiles_x, int tiles_y, int out_mode,
                void* workspace, size_t workspace_bytes, pcuda_stream_t s);
size_t pcuda_rescale_resize_crop_u8_workspace_size(void);
int pcuda_rescale_resize_crop_u8(const void* in, int in_dtype, int n, int sh, int sw, int resize_h, int resize_w, int crop,
                                 uint8_t* out, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* device-side spacing resample of the MS-CMRSeg data: the .npy path of utils/read_nii_image.py (read_*_nii_save_npy :202-231,
 * read_*_nii_label_save_npy :234-271; csrc/resample.hip).  The arithmetic is scipy.ndimage.zoom(order=1)'s, pinned bit for bit:
 * the expected arrays of tests/golden/resample.npz are the outputs of scipy 1.15.3 / numpy themselves
 * (scripts/make_resample_golden.py), next to a plain restatement of the rule below.
 *
 * pcuda_zoom_linear_crop: ndimage.zoom(vol, [1, zh / sh, zw / sw], order=1) of in[n][sh][sw] (dtype PCUDA_PRE_F32 / _I16 / _U8;
 *   the caller passes the zoomed size (zh, zw) = round(dim factor)), then crop_volume -> out[n][oh][ow] of the same dtype.  Only
 *   the crop window is computed: rows zh / 2 - crop / 2 .. zh / 2 + crop / 2 of the zoomed slice, columns likewise, so
 *   oh = ow = 2 (crop / 2); crop = 0: none, (oh, ow) = (zh, zw).
 *   Per axis, in float64: z = (in - 1) / (out - 1) (1.0 when out == 1), cc = double(k) z for the output index k of the zoomed
 *   slice, i0 = floor(cc), t = cc - i0, w0 = 1 - t, w1 = t.  Per pixel: acc = (c00 wy0) wx0, += (c01 wy0) wx1, += (c10 wy1) wx0,
 *   += (c11 wy1) wx1 in that order, every operation rounded on its own (-ffp-contract=off); c01 = in[i0y][i0x + 1] and so on.
 *   mode='constant', cval=0: a tap whose index equals the input size is 0 (it is never read), and a pixel with cc > in - 1 on
 *   either axis -- the last coordinate of some (in, out) pairs, (8, 26) the smallest, overshoots by an ulp -- is 0 altogether
 *   (scipy does not interpolate beyond the last sample).  fp32: out = float(acc); integers: r = acc > 0 ? acc + 0.5 : acc - 0.5,
 *   clamped to the dtype's range, truncated toward zero (scipy's round half away from zero).  The slice axis has factor 1 and
 *   drops out (its second tap has weight 0).
 *   workspace: pcuda_zoom_linear_crop_workspace_size bytes: (i0, t) per output row and column, written by a small kernel.
 *
 * pcuda_zoom_standardize: the image chain in one call: the zoom and crop above, mean and std of the zoomed cropped values of
 *   the whole volume, then out = float((double(x) - mean) / std) (a true float64 division), fp32 out[n][channels][oh][ow] with
 *   channels 1 or 3 (3: the same value in all three channels, what predict_labels takes; compare PCUDA_CLAHE_F32X3).  The
 *   statistics stay on the device (no host round trip) and are left in stats[0] = mean, stats[1] = std (device, two doubles).
 *   Integer volumes, exact: Sx and Sxx in 64-bit integers (per-workgroup partials, then one workgroup; no atomics),
 *   mean = double(Sx) / double(n), std = sqrt(double(n Sxx - Sx Sx) / (double(n) double(n))) with the numerator in 128-bit
 *   integers, converted once (nearest even): mean equals numpy.mean bit for bit, std is within 2e-16 relative of numpy.std.
 *   fp32 volumes: THIS BUILD'S OWN convention: statistics of the fp32-rounded zoomed values accumulated in float64 in a fixed
 *   reduction order, in two passes (mean = S / n; std = sqrt(sum((x - mean)^2) / n)); numpy's float32 pairwise accumulation of
 *   a float32 array is not reproduced.  No float atomics.  std == 0 gives inf / NaN as numpy does; NaN in the input is
 *   unsupported.  workspace: pcuda_zoom_standardize_workspace_size bytes (the table, the partials, the zoomed values).
 *
 * pcuda_zoom_labels: the label chain fused, no one-hot tensor: raw codes in[n][sh][sw] (PCUDA_PRE_I16 or _U8); remap: num_remap
 *   <= 8 (from, to) pairs (host array of 2 num_remap ints), applied in order like the reference's chained np.where; for each
 *   class c < num_classes (2..8) the four taps above over [label == c] as 0.0 / 1.0, rounded as for uint8; the label is the
 *   first class whose rounded channel is largest (argmax; every channel 0: class 0) -> uint8 out[n][oh][ow].  A remapped
 *   value outside [0, num_classes) matches no class; the number of such values in the WHOLE input volume is left in the first
 *   8 bytes of the workspace (uint64; the reference asserts on it in to_categorical).
 *   workspace: pcuda_zoom_labels_workspace_size bytes (the counter, then the table).
 *
 * All three: never allocate, never synchronise; `in` is never written and in == out is rejected; n == 0 is a no-op returning
 * 0; sides 1..32768, zh, zw >= 1, a crop window inside the zoomed slice and fewer than 2^31 output values, else
 * PCUDA_E_BADARG before any launch; the same bits from run to run. */
size_t pcuda_zoom_linear_crop_workspace_size(int zh, int zw, int crop);
int pcuda_zoom_linear_crop(const void* in, int dtype, int n, int sh, int sw, int zh, int zw, int crop, void* out,
                           void* workspace, size_t workspace_bytes, pcuda_stream_t s);
size_t pcuda_zoom_standardize_workspace_size(int dtype, int n, int zh, int zw, int crop);
int pcuda_zoom_standardize(const void* in, int dtype, int n, int sh, int sw, int zh, int zw, int crop, int channels,
                           float* out, double* stats, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
size_t pcuda_zoom_labels_workspace_size(int zh, int zw, int crop);
int pcuda_zoom_labels(const void* in, int dtype, int n, int sh, int sw, int zh, int zw, int crop, int num_classes,
                      const int* remap, int num_remap, uint8_t* out, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* test volumes of the evaluate scripts on the device (csrc/evalprep.hip): read_img's
 * np.moveaxis(vol, 2, 0)[:, ::-1, ::-1], its 2.5-D stack and to_categorical (evaluate_mmwhs.py:19-29), the nimg.T of
 * evaluate_mscmrseg.py:147, and the way back from a prediction to the volume's own axis order.  Casts only: numpy pins every bit.
 *
 * One index map, in ELEMENTS of the caller's array, serves all three:
 *   src(z, r, c) = base + z sz + (flip_r ? r_size - 1 - r : r) sr + (flip_c ? c_size - 1 - c : c) sc
 * C order, Fortran order and any permuted view are strides only (nimg.T swaps strides; moveaxis(2, 0)[:, ::-1, ::-1] is strides
 * plus both flips).  base >= 0; a stride is positive on every axis longer than 1 (an axis of length 1 ignores its stride); the
 * caller guarantees that every address of the map lies inside its array.  z, r, c (the sizes) >= 0; an empty volume returns 0
 * without a launch.  All offsets are 64-bit.  The kernel form follows the strides: sc == 1: a pass along the rows, four
 * columns per lane where c % 4 == 0 and pointers and pitches are aligned to the group; sr == 1 or sz == 1: a 64 x 64 tile
 * through LDS, so that reads and writes both run along their own fastest axis; no unit stride: a plain gather / scatter.
 *
 * pcuda_volume_slices: in of PCUDA_VOL_F32 / _F64 / _I16 / _U8 -> contiguous fp32 out[z][window][r][c]; float64 rounds to
 *   nearest even (numpy's astype(float32)).  window 1: the reoriented slices.  window 3: channel k of sample i is slice
 *   (i + k - 1) mod z, wrapping at both ends (img[[i - 1, i, (i + 1) % D]]; z = 1 gives three copies of the slice).  Every
 *   source value is read once and stored `window` times.
 * pcuda_volume_labels: in of PCUDA_VOL_U8 / _I16 / _I32 / _F32 / _F64; remap: num_remap <= 8 (from, to) pairs (host array of
 *   2 num_remap ints) applied in order, like chained np.where; -> uint8 labels[z][r][c] and, if onehot is not null, uint8
 *   onehot[z][num_classes][r][c] in the same pass (num_classes 2..255).  A value that after the remap is not an integer in
 *   [0, num_classes) (NaN included) is written as label 0 with an all-zero one-hot pixel and counted: the count is left in the
 *   first 8 bytes of the workspace (uint64, integer atomics; the reference's to_categorical asserts there).
 *   workspace: pcuda_volume_labels_workspace_size bytes, 8-byte aligned (an empty volume leaves it as it is).  raw != 0: labels is int32 labels[z][r][c] holding
 *   int32(value) (truncation toward zero for floating point), no remap, no range check, no one-hot, no workspace needed (the
 *   MS-CMRSeg ground truth keeps its 200 / 500 / 600 codes).
 * pcuda_volume_restore: the inverse scatter: uint8 in[z][r][c] -> out (PCUDA_VOL_U8 or _I16) through the same map, so that
 *   labels(restore(x)) == x; lut: null, or 256 int16 values ON THE DEVICE looked up first (MS-CMRSeg's 1 / 2 / 3 -> 200 / 500 /
 *   600; cast to the output dtype).  Elements of out the map does not reach are left as they are.
 *
 * All three: never allocate, never synchronise, launch on s; in is never written and in == out is rejected; bad arguments are
 * PCUDA_E_BADARG before any launch; the same bits from run to run. */
#define PCUDA_VOL_F32 0
#define PCUDA_VOL_I16 1
#define PCUDA_VOL_U8 2
#define PCUDA_VOL_F64 4
#define PCUDA_VOL_I32 5
int pcuda_volume_slices(const void* in, int dtype, long long base, long long sz, long long sr, long long sc, int z, int r, int c,
                        int flip_r, int flip_c, int window, float* out, pcuda_stream_t s);
size_t pcuda_volume_labels_workspace_size(void);
int pcuda_volume_labels(const void* in, int dtype, long long base, long long sz, long long sr, long long sc, int z, int r, int c,
                        int flip_r, int flip_c, int num_classes, const int* remap, int num_remap, int raw, void* labels,
                        uint8_t* onehot, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
int pcuda_volume_restore(const uint8_t* in, int z, int r, int c, void* out, int out_dtype, long long base, long long sz,
                         long long sr, long long sc, int flip_r, int flip_c, const int16_t* lut, pcuda_stream_t s);
/* validation metrics (train_mscmrseg.py:85-92, metric.py:39-82): labels[n][i] = first channel holding the
 * per-pixel maximum of x[n][c][i] (fp32 logits, or a uint8 one-hot mask when x_is_u8); strides in elements */
int pcuda_argmax_labels(const void* x, int x_is_u8, long long sn, long long sc, int n, int c, long long hw,
                        uint8_t* labels, pcuda_stream_t s);
/* dice[k] = 2|pred==k & gt==k| / (|pred==k| + |gt==k|), 0 if both empty (medpy dc), k < c.
 * workspace: 3*c 64-bit counters */
int pcuda_label_dice(const uint8_t* pred, const uint8_t* gt, long long numel, int c, float* dice, void* workspace,
                     size_t workspace_bytes, pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * native-size evaluation of MS-CMRSeg (evaluate_mscmrseg.py:139-145; utils/utils.py:83-92 resize_volume =
 * cv2.resize(.., INTER_AREA) per fp32 plane).  The rule is this build's own, written after OpenCV's resize.cpp; its parity
 * with OpenCV is NOT pinned (DESIGN.md f15 states the rule).  Per axis, source size S, destination size D, scale = S / D and
 * inv = D / S in fp64; every fp32 operation rounded on its own.
 *   scale_x >= 1 and scale_y >= 1: the area table per axis (f1 = d * scale, f2 = f1 + scale, cell = min(scale, S - f1),
 *     s1 = ceil(f1), s2 = min(floor(f2), S - 1), s1 = min(s1, s2); tap s1 - 1 with (s1 - f1) / cell if s1 - f1 > 1e-3, taps
 *     s1 .. s2 - 1 with 1 / cell, tap s2 with min(min(f2 - s2, 1), cell) / cell if f2 - s2 > 1e-3; weights rounded to fp32);
 *     per source row in order the row sum h = w0 * v0, h += w * v over the taps in order, then out = wy0 * h0, out += wy * h.
 *   otherwise (an axis enlarges) two-tap linear on both axes: sx = floor(d * scale), fx = (d + 1) - (sx + 1) * inv, fx = 0 if
 *     fx <= 0 else fx - floor(fx); sx >= S - 1: sx = S - 1, fx = 0; h = v[sx] * (float)(1 - fx) + v[sx + 1] * (float)fx, h =
 *     v[sx] when fx == 0; the rows are combined the same way.
 * pcuda_area_resize: in[n] at in + n * sn, rows sr elements apart, unit column stride, [sh][sw] -> out[n][dh][dw] dense.
 * pcuda_reconstruct_resize_argmax: logits[n][c][h][w] (strides sn, sc, sr in elements, unit column stride; c 1..8, h = w =
 *   2 * crop) pasted at origin / 2 - crop of a zero origin x origin canvas that is never written, each class plane resized to
 *   [dh][dw] by the rule above, labels[n][dh][dw] = first class holding the maximum, 0 when any class is NaN (the rule of
 *   pcuda_argmax_labels); the resized planes are never written either.
 * Both: every size 1..16384, n <= 65535; never allocate, never synchronise, launch on s; bad arguments are PCUDA_E_BADARG
 * before any launch; the same bits from run to run. */
int pcuda_area_resize(const float* in, long long sn, long long sr, int n, int sh, int sw, float* out, int dh, int dw,
                      pcuda_stream_t s);
int pcuda_reconstruct_resize_argmax(const float* logits, long long sn, long long sc, long long sr, int n, int c, int h, int w,
                                    int crop, int origin, uint8_t* labels, int dh, int dw, pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * evaluation metrics (utils/metric.py evaluate / metrics2, evaluate_*.py; medpy.metric.binary dc / hd / asd and
 * utils.py keep_largest_connected_components) on integer label volumes [z][h][w] (ndim 2: z = 1, [h][w]), uint8 or
 * int32 (labels_i32); every dimension 1..16384, z*h*w < 2^31.
 * ---------------------------------------------------------------------------------- */
/* per class value classes[k] (ncls 1..8, host array), A = pred == c, B = gt == c:
 * out[k][8] (device fp64) = dice 2|A.B|/(|A|+|B|) (0 if both empty), hd, asd(pred->gt), asd(gt->pred), |A|, |B|, |A.B|,
 * flags (1: A empty, 2: B empty; hd / asd are NaN then).  border(X) = X & ~erode(X) with the footprint of connectivity
 * 1..ndim, outside = background; sd(X, Y) = Euclidean distance (spacing[ndim] per array axis, host, NULL = 1) from each
 * border(X) voxel to the nearest border(Y) voxel; hd = max over both directions, asd(X->Y) = mean sd(X, Y).  Exact
 * integer squared distances at unit spacing; results are the same bits from run to run. */
size_t pcuda_surface_metrics_workspace_size(int ndim, int z, int h, int w, int ncls, const double* spacing);
int pcuda_surface_metrics(const void* pred, const void* gt, int labels_i32, int ndim, int z, int h, int w, const int* classes,
                          int ncls, int connectivity, const double* spacing, double* out, void* workspace,
                          size_t workspace_bytes, pcuda_stream_t s);
/* pcuda_surface_metrics and four more columns: out[k][12] (device fp64) = the eight columns above (the same bits), then
 * the percentile-th percentile (0..100; 95: medpy's hd95) of the pooled distances sd(A, B) u sd(B, A) by numpy's linear
 * method (n values sorted ascending: v = (n - 1) * percentile / 100, lo = floor(v), hi = min(lo + 1, n - 1), t = v - lo,
 * s[lo] + (s[hi] - s[lo]) * t, or s[hi] - (s[hi] - s[lo]) * (1 - t) where t >= 0.5; fp64, one rounding per operation),
 * assd = (asd(pred->gt) + asd(gt->pred)) / 2 (medpy's assd), |border(A)|, |border(B)|.  Columns 8 and 9 are NaN when a
 * flag is set.  The two order statistics are selected exactly on the device (MSB-first radix select over the stored
 * squared distances, 8 bits per pass: 4 passes at unit spacing, 8 with spacing; integer atomics only): the same bits
 * from run to run, no host synchronisation.  Argument checks as pcuda_surface_metrics; a percentile outside [0, 100] or
 * NaN is PCUDA_E_BADARG.  Needs its own, larger workspace. */
size_t pcuda_surface_metrics_ext_workspace_size(int ndim, int z, int h, int w, int ncls, const double* spacing);
int pcuda_surface_metrics_ext(const void* pred, const void* gt, int labels_i32, int ndim, int z, int h, int w,
                              const int* classes, int ncls, int connectivity, const double* spacing, double percentile,
                              double* out, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* out (uint8) = for each label 1..min(nlabels, 255) of mask the largest face-connected component (among equal sizes
 * the one whose first voxel comes first in raster order), every other voxel 0 */
size_t pcuda_largest_components_workspace_size(int ndim, int z, int h, int w);
int pcuda_largest_components(const void* mask, int mask_i32, int ndim, int z, int h, int w, int nlabels, uint8_t* out,
                             void* workspace, size_t workspace_bytes, pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * small dense ops of PointNetCls / the point head (PointNetCls.py; unet.py:86,94-95)
 * ---------------------------------------------------------------------------------- */
/* y[m][n] = x[m][k] . w[n][k]^T + b[n]   (nn.Linear; also conv1d k=1 seen as [B*L][C]) */
int pcuda_linear_fwd(const float* x, const float* w, const float* b, float* y, int m, int k, int n, pcuda_stream_t s);
int pcuda_linear_bwd_x(const float* dy, const float* w, float* dx, int m, int k, int n, int accumulate, pcuda_stream_t s);
/* workspace (optional; pcuda_linear_bwd_w_workspace_size bytes) enables a deterministic split-K for
 * long reductions into a small output (the point head's Linear over 300*B rows) */
size_t pcuda_linear_bwd_w_workspace_size(int m, int k, int n);
int pcuda_linear_bwd_w(const float* dy, const float* x, float* dw, float* db, int m, int k, int n, int accumulate,
                       void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* torch.nn.Conv1d(cin, cout, 1) on dense [b][c][l] point clouds (PointNetCls.py:26-28 STN3d, :76-78 STNkd, :116-131
 * PointNetfeat) in EXACT fp32 on the matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma chain; no bf16
 * operand split).  w = [cout][cin] (the Conv1d weight with its unit kernel axis dropped), bias may be NULL.
 * fwd: y[b][co][l]; bn_partials (optional) = [pcuda_conv1d_k1_fwd_tiles(b, l)][cout][2] per-tile (sum, sum of squares)
 * of y for the BatchNorm1d that follows (pcuda_bn_finalize reduces them in a fixed order).
 * dgrad: dx[b][ci][l] = sum_co w[co][ci] dy[b][co][l].
 * wgrad: dw[co][ci] (+)= sum_{b,l} dy x, db[co] (+)= sum_{b,l} dy (db may be NULL); split-K slabs in the caller's
 * workspace, summed in a fixed order (deterministic). */
int pcuda_conv1d_k1_fwd_tiles(int b, int l);
int pcuda_conv1d_k1_fwd(const float* x, const float* w, const float* bias, float* y, int b, int cin, int cout, int l,
                        float* bn_partials, pcuda_stream_t s);
int pcuda_conv1d_k1_dgrad(const float* dy, const float* w, float* dx, int b, int cin, int cout, int l, pcuda_stream_t s);
size_t pcuda_conv1d_k1_wgrad_workspace_size(int b, int cin, int cout, int l);
int pcuda_conv1d_k1_wgrad(const float* x, const float* dy, float* dw, float* db, int b, int cin, int cout, int l,
                          int accumulate, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* max over the last axis of x[b][c][l] with argmax (PointNetCls.py:44,162) */
int pcuda_max_points_fwd(const float* x, int b, int c, int l, float* y, int* idx, pcuda_stream_t s);
int pcuda_max_points_bwd(const float* dy, const int* idx, int b, int c, int l, float* dx, pcuda_stream_t s);
/* Small-tensor forms of the point-cloud discriminator (csrc/pointnet_small.hip).  Each computes, bit for bit, what the
 * general entry points named with it compute: same association of every sum, another mapping to threads.
 * bn1d_fwd: training BatchNorm1d on a[b][c] (rows a_sn floats apart, channels contiguous; count = b) in one launch =
 *   pcuda_bn_stats + pcuda_bn_finalize + pcuda_bn_apply (flags = relu ? PCUDA_BN_APPLY_RELU : 0).
 * bn1d_bwd: = pcuda_bn_bwd_reduce + pcuda_bn_bwd_finalize(count = b) + pcuda_bn_bwd_apply with one gradient source.
 *   Both return PCUDA_E_UNSUPPORTED for b > 1024; a second gradient share (dy2) and frozen statistics (count < 0) have
 *   no fused form: use the three calls. */
int pcuda_bn1d_fwd(const float* a, long long a_sn, int b, int c, const float* gamma, const float* beta, float eps,
                   float momentum, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                   float* shift, int relu, float* y, long long y_sn, pcuda_stream_t s);
int pcuda_bn1d_bwd(const float* dy, long long dy_sn, const float* a, long long a_sn, int b, int c, const float* gamma,
                   const float* mean, const float* invstd, const float* scale, const float* shift, int post_relu,
                   float act_slope, float* dgamma, float* dbeta, int accumulate, float* dz, long long dz_sn,
                   pcuda_stream_t s);
/* The two passes of the BatchNorm backward whose incoming gradient is pcuda_max_points_bwd(g, idx), without that dense
 * [b][c][l] tensor: g, idx dense [b][c]; a, dz dense [b][c][l]; l <= 2048 (PCUDA_E_UNSUPPORTED above).
 * reduce_maxpts writes red[b][c][2] = what pcuda_bn_bwd_reduce writes for the dense gradient (ntiles = b), the input of
 * pcuda_bn_bwd_finalize; apply_maxpts = pcuda_bn_bwd_apply on the dense gradient. */
int pcuda_bn_bwd_reduce_maxpts(const float* g, const int* idx, const float* a, const float* mean, const float* invstd,
                               const float* scale, const float* shift, int post_relu, int b, int c, int l, float* red,
                               pcuda_stream_t s);
int pcuda_bn_bwd_apply_maxpts(const float* g, const int* idx, const float* a, const float* coef, const float* scale,
                              const float* shift, int post_relu, float act_slope, float* dz, int b, int c, int l,
                              pcuda_stream_t s);
/* batched small matmul C[b] = op(A[b]) . op(B[b]); A [m][k] (or [k][m] when ta), B [k][n] (or [n][k] when tb) */
int pcuda_bmm(const float* a, const float* bmat, float* c, int batch, int m, int k, int n, int ta, int tb,
              int accumulate, pcuda_stream_t s);

/* jaccard_loss(true, logits=probabilities, eps, activation=False) as a free-standing function (utils/loss.py:5-37 the way
 * train_mscmrseg.py:203 / train_mmwhs.py:218 call it): probs fp32 dense [n][c][hw]; truth one-hot, fp32 or uint8;
 * loss = 1 - mean_c I_c / (S_c - I_c + eps).  bwd: dprobs = gout * d loss / d probs (workspace of the forward call) */
size_t pcuda_jaccard_workspace_size(int c);
int pcuda_jaccard_fwd(const float* probs, const void* truth, int truth_is_u8, int n, int c, long long hw, float eps,
                      float* loss, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
int pcuda_jaccard_bwd(const void* truth, int truth_is_u8, int n, int c, long long hw, float eps, const float* gout,
                      float* dprobs, const void* workspace, pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * Dice loss (the -dice switch both training scripts parse and never read; csrc/dice_loss.hip: the per-class kernels are
 * the overlap family of csrc/loss_device.h with the Dice policy, the per-sample reduction and the label-map form are its own)
 * ---------------------------------------------------------------------------------- */
/* This build's own rule (the reference builds kornia.losses.DiceLoss() and never calls it; parity with any kornia version is
 * unpinned, and kornia's + eps on its one-hot tensor is not reproduced).  p: probabilities, y: one-hot truth,
 *   PCUDA_OV_DICE_CLASS   I_c = sum p y, S_c = sum (p + y) over (batch, pixels): loss = 1 - mean_c 2 I_c / (S_c + eps)
 *   PCUDA_OV_DICE_SAMPLE  I_n, S_n over (classes, pixels) of sample n:           loss = mean_n (1 - 2 I_n / (S_n + eps))
 *   d loss / d p = -(2 / M) (y / (S + eps) - I / (S + eps)^2) with the sums of the element's own class or sample, M = c or n.
 * All three families: a forward call leaves the coefficients 1 / (S + eps), I / (S + eps)^2 in its workspace and the
 * backward call reads them there (eps is an argument of the forward only; the same n, c, hw, overlap / reduce on both);
 * partial sums of different samples never share a row, the final reduce runs in a fixed order in double: the same bits
 * from run to run, any n (it is not laid on a grid's y axis).  Never allocate, never synchronise; arguments are checked
 * before any launch (PCUDA_E_BADARG, PCUDA_E_UNSUPPORTED above the class limit of the fused form, PCUDA_E_WORKSPACE). */
#define PCUDA_OV_DICE_CLASS 1
#define PCUDA_OV_DICE_SAMPLE 2
/* pcuda_seg_loss_fwd / _bwd with a Dice overlap term: out2 = [bce | double-softmax ce, dice], c = 1..8;
 * dlogits = g_main * d main / do + g_ov * d dice / do (a NULL seed is 1).  workspace_size: 0 for arguments the calls reject */
size_t pcuda_seg_loss_ov_workspace_size(int n, int c, long long hw, int overlap);
int pcuda_seg_loss_ov_fwd(const float* logits, const uint8_t* onehot, int mode, int overlap, double eps, int n, int c,
                          long long hw, float* out2, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
int pcuda_seg_loss_ov_bwd(const float* logits, const uint8_t* onehot, int mode, int overlap, int n, int c, long long hw,
                          const float* g_main, const float* g_ov, float* dlogits, const void* workspace,
                          size_t workspace_bytes, pcuda_stream_t s);
/* Dice on given probabilities, the twin of pcuda_jaccard_*: probs fp32 dense [n][c][hw]; truth fp32 or uint8, same shape;
 * reduce = PCUDA_OV_DICE_CLASS | PCUDA_OV_DICE_SAMPLE; c = 1..16.  bwd: dprobs = gout * d loss / d probs (gout NULL: 1) */
size_t pcuda_dice_workspace_size(int n, int c, long long hw, int reduce);
int pcuda_dice_fwd(const float* probs, const void* truth, int truth_is_u8, int n, int c, long long hw, int reduce, float eps,
                   float* loss, void* workspace, size_t workspace_bytes, pcuda_stream_t s);
int pcuda_dice_bwd(const void* truth, int truth_is_u8, int n, int c, long long hw, int reduce, const float* gout,
                   float* dprobs, const void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* Dice per sample on logits [n][c][hw] and a label map [n][hw] (uint8 or int64): p = softmax over the channels, computed
 * inside; the one-hot tensor is never written.  A label outside [0, c) belongs to no class (nothing to I, only p to S) and
 * is counted: bad_count (device, may be NULL) is zeroed and receives their number (an integer atomic).  c = 1..16.
 * bwd: dlogits = gout * d loss / d logits */
size_t pcuda_dice_labels_workspace_size(int n, int c, long long hw);
int pcuda_dice_labels_fwd(const float* logits, const void* labels, int labels_are_i64, int n, int c, long long hw, float eps,
                          float* loss, unsigned long long* bad_count, void* workspace, size_t workspace_bytes,
                          pcuda_stream_t s);
int pcuda_dice_labels_bwd(const float* logits, const void* labels, int labels_are_i64, int n, int c, long long hw,
                          const float* gout, float* dlogits, const void* workspace, size_t workspace_bytes,
                          pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * mask -> surface point cloud sampler (utils/npy2point.py:7-18,101-125)
 * ---------------------------------------------------------------------------------- */
/* canonical surface-vertex list of b binary masks [b][h][w] (uint8, >0 = foreground):
 * verts int32 [b][max_verts][3] rows (z,y,x) in lexicographic order, z in {0,1,2}; counts[b].
 * workspace: b*h*w*4 + 4096 bytes */
int pcuda_surface_vertices(const uint8_t* mask, int b, int h, int w, int* verts, int max_verts, int* counts,
                           void* workspace, size_t workspace_bytes, pcuda_stream_t s);
/* second vertex-list mode: marching-cubes traversal order on the 3-slice stack (cells nested slice / row / column, per
 * cell the edges 6,5,10,0,1,2,3,4,7,8,9,11, one vertex per crossing edge at its background end, duplicates included);
 * replaces mcubes.marching_cubes(vol, 0) at utils/npy2point.py:112,121 as far as the un-vendored library's published
 * algorithm pins it (parity unpinned, oracle/sampler.py).  verts int32 [b][max_verts][3] rows (slice,row,col); counts[b]
 * = vertices found (may exceed max_verts: only the first max_verts are written) */
int pcuda_surface_vertices_mc(const uint8_t* mask, int b, int h, int w, int* verts, int max_verts, int* counts,
                              pcuda_stream_t s);
/* farthest point sampling (graipher): pts float64 [b][npts_max][3] with counts[b] valid rows;
 * first[b] = start index; out idx int32 [b][k].  Bit-exact with numpy float64 (no FMA contraction,
 * first-occurrence argmax).  counts[b] == 0 -> idx all -1 */
int pcuda_fps(const double* pts, const int* counts, const int* first, int b, int npts_max, int k, int* idx,
              pcuda_stream_t s);

/* ------------------------------------------------------------------------------------
 * optimisers on flat fp32 buffers (train_mscmrseg.py:427-455: Adam(b=(.9,.99)); SGD(m, wd))
 * ---------------------------------------------------------------------------------- */
int pcuda_adam_step(float* p, const float* g, float* m, float* v, long long numel, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int step, float grad_scale, pcuda_stream_t s);
/* same update with the step count held in device memory: *step_dev is incremented on the stream first and then
 * used for the bias corrections, so a captured graph of the train step replays correctly */
int pcuda_adam_step_dev(float* p, const float* g, float* m, float* v, long long numel, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int* step_dev, float grad_scale,
                        pcuda_stream_t s);
int pcuda_sgd_step(float* p, const float* g, float* mom, long long numel, float lr, float momentum,
                   float weight_decay, int first_step, float grad_scale, pcuda_stream_t s);

/* guarded steps: gradient-norm clipping and non-finite skip decided on the device (no host round trip, so a captured
 * graph of the step replays the decision with the gradient it finds).
 *
 * The guard record is 8 four-byte words of device memory owned by the caller, zeroed once:
 *   [0] float norm     global L2 norm of g * grad_scale over the ranges
 *   [1] float coef     max_norm > 0 ? min(1, max_norm / (norm + 1e-6f)) : 1   (fp32; a NaN norm gives a NaN coef, as
 *                      torch.nn.utils.clip_grad_norm_ does)
 *   [2] int   finite   isfinite(norm): a sum that overflows fp32 counts as non-finite
 *   [3] int   skipped  cumulative: calls that decided "skip"   (skip_nonfinite != 0 and finite == 0)
 *   [4] int   applied  cumulative: all other calls
 *   [5] int   skip     this call's decision, 0 or 1
 *   [6..7]             reserved
 *
 * pcuda_grad_norm: `ranges` is HOST memory, nranges x (offset, numel) in elements of g, 1 <= nranges <=
 * PCUDA_GUARD_MAX_RANGES, numel >= 0; a range may start at any element, elements outside the ranges are never read.
 * x = g[i] * grad_scale in fp32, x * x accumulated in double in a fixed order (lane, wave, workgroup partial; a second
 * one-workgroup launch sums the partials per range in a fixed order and writes the record): no atomics, the same bits on
 * every call.  norm = (float)sqrt(total).  range_sumsq (device, nranges doubles; may be NULL) receives each range's sum.
 * workspace: PCUDA_GRAD_NORM_WORKSPACE_BYTES of device memory, 8-byte aligned. */
#define PCUDA_GUARD_MAX_RANGES 16
#define PCUDA_GUARD_RECORD_BYTES 32
#define PCUDA_GRAD_NORM_WORKSPACE_BYTES 16384
int pcuda_grad_norm(const float* g, const long long* ranges, int nranges, float grad_scale, float max_norm,
                    int skip_nonfinite, void* record, double* range_sumsq, void* workspace, size_t workspace_bytes,
                    pcuda_stream_t s);
/* pcuda_adam_step_dev / pcuda_sgd_step with gi = (g[i] * grad_scale) * record.coef (two rounded fp32 products; coef == 1
 * gives the unguarded kernels' bits).  With skip_nonfinite != 0 and record.finite == 0 nothing is stored: p, m, v, mom
 * keep their bits, *step_dev is not incremented (the conditional increment takes the place of the unconditional one),
 * *init_dev is not set.  With skip_nonfinite == 0 a non-finite norm propagates as clip_grad_norm_(error_if_nonfinite=
 * False) followed by the step does.
 * SGD: *init_dev (device int32) is "the momentum buffer is initialised" (torch.optim.SGD's first step copies the gradient
 * into it); with mark_init != 0 it is set behind this call's update when the step is applied -- pass 0 for all but the last
 * of the contiguous ranges of one step.  init_dev may be NULL when momentum == 0. */
int pcuda_adam_step_guarded(float* p, const float* g, float* m, float* v, long long numel, float lr, float beta1,
                            float beta2, float eps, float weight_decay, int* step_dev, float grad_scale,
                            const void* record, int skip_nonfinite, pcuda_stream_t s);
int pcuda_sgd_step_guarded(float* p, const float* g, float* mom, long long numel, float lr, float momentum,
                           float weight_decay, int* init_dev, int mark_init, float grad_scale, const void* record,
                           int skip_nonfinite, pcuda_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* PCUDA_HIP_H */
