// Dice loss on the device (the -dice switch of both training scripts; this build's own rule, include/pcuda_hip.h):
//   per class   I_c = sum p*y, S_c = sum (p + y) over (batch, pixels); loss = 1 - mean_c 2 I_c / (S_c + eps)
//   per sample  I_n, S_n over (classes, pixels);                      loss = mean_n (1 - 2 I_n / (S_n + eps))
//   d loss / d p = -(2 / M) (y / (S + eps) - I / (S + eps)^2), the sums of the element's own class or sample, M = C or N
// Three families: the fused segmentation loss with a Dice overlap term (pcuda_seg_loss_ov_*), Dice on given probabilities
// (pcuda_dice_*), Dice on logits + a label map (pcuda_dice_labels_*).
//
// Every forward is: block partial rows (fp32) -> a fixed-order reduce in double -> the scalars and the coefficients
// a = 1 / (S + eps), b = I / (S + eps)^2 per class or per sample, left in the workspace for the backward pass.  No floating
// point atomics: the same bits from run to run.  The per-class kernels are the overlap family's (loss_device.h) with the Dice
// policy, the ones losses.hip runs with the Jaccard policy; what is here is what only Dice has: the per-sample reduction and
// the label-map form.  A per-sample partial row belongs to ONE sample: the grid of a per-sample pass is (sample, chunk) pairs
// laid out on the x axis (n * bps blocks; n is not bounded by a grid's y limit).
#include "loss_device.h"

#define OV_BLOCKS 1024     // blocks a (sample, chunk) forward pass aims at (more only where n alone exceeds it)
#define DICE_BLOCKS 256    // block cap (per class) of the stand-alone per-class pass

// ---------------------------------------------------------------------------- per-sample reduce
// stage 1: one wave per sample over its bps partial rows of NACC floats: [main (NACC = 3)] [I] [S]
//   coef[2n], coef[2n+1] = a_n, b_n; samp[2n] = 2 I_n / (S_n + eps), samp[2n+1] = the sample's main sum
template <int NACC>
__global__ __launch_bounds__(256) void dice_sample_reduce_kernel(const float* __restrict__ part, int n, int bps, double eps,
                                                                float* __restrict__ coef, double* __restrict__ samp) {
  const int smp = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (smp >= n) return;      // (the whole wave)
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0;
  for (int j = lane; j < bps; j += 64) {
    const float* r = part + ((long long)smp * bps + j) * NACC;
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] += (double)r[k];
  }
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = wave_sum_d(acc[k]);
  if (lane == 0) {
    const double I = acc[NACC - 2], S = acc[NACC - 1];
    overlap_coef<DiceOv>(I, S, eps, coef[2ll * smp], coef[2ll * smp + 1]);
    samp[2ll * smp] = DiceOv::term(I, DiceOv::den(I, S, eps));
    samp[2ll * smp + 1] = NACC == 3 ? acc[0] : 0.0;
  }
}

// stage 2: out = [sum of the main sums / numel_main (has_main),] 1 - mean_n samp[2n]; samples in a fixed order
__global__ __launch_bounds__(256) void dice_sample_final_kernel(const double* __restrict__ samp, int n, int has_main,
                                                               double numel_main, double* __restrict__ sums,
                                                               float* __restrict__ out) {
  __shared__ double red[256];
  double t = 0, m = 0;
  for (int i = threadIdx.x; i < n; i += 256) { t += samp[2ll * i]; m += samp[2ll * i + 1]; }
  t = block_tree_sum(t, red);
  m = block_tree_sum(m, red);
  if (threadIdx.x == 0) {
    sums[0] = m; sums[1] = t;
    if (has_main) out[0] = (float)(m / numel_main);
    out[has_main] = (float)(1.0 - t / n);
  }
}

// ---------------------------------------------------------------------------- Dice on given probabilities, per sample
// a sample's c * hw values are contiguous (len of them); block = (sample, chunk), partial row [I, S]
__global__ __launch_bounds__(256) void dice_sample_partial_kernel(const float* __restrict__ p, const float* __restrict__ tf,
                                                                 const uint8_t* __restrict__ tu, long long len, int bps,
                                                                 float* __restrict__ part) {
  const long long n = blockIdx.x / (unsigned)bps;
  const int j = (int)(blockIdx.x - n * bps);
  float acc[2] = {0.f, 0.f};
  for (long long e = j * 256ll + threadIdx.x; e < len; e += 256ll * bps) {
    const long long o = n * len + e;
    const float pr = p[o], y = tf ? tf[o] : (float)tu[o];
    acc[0] += pr * y;
    acc[1] += pr + y;
  }
  block_store_row<2>(acc, part + (long long)blockIdx.x * 2);
}

// ---------------------------------------------------------------------------- Dice on logits + a label map (per sample)
// p = softmax over the c channels, y = one-hot of the label without ever being written; a label outside [0, c) belongs to no
// class (nothing to I, only p to S) and is counted (integer atomic: order independent)
__device__ __forceinline__ long long read_label(const uint8_t* __restrict__ l8, const long long* __restrict__ l64,
                                                long long i) {
  return l64 ? l64[i] : (long long)l8[i];
}

__global__ __launch_bounds__(256) void dice_labels_partial_kernel(const float* __restrict__ logits,
                                                                 const uint8_t* __restrict__ l8,
                                                                 const long long* __restrict__ l64, int c, long long hw,
                                                                 int bps, float* __restrict__ part,
                                                                 unsigned long long* __restrict__ bad_count) {
  const long long n = blockIdx.x / (unsigned)bps;
  const int j = (int)(blockIdx.x - n * bps);
  float acc[2] = {0.f, 0.f};
  unsigned int bad = 0;
  for (long long px = j * 256ll + threadIdx.x; px < hw; px += 256ll * bps) {
    const long long lab = read_label(l8, l64, n * hw + px);
    const bool valid = lab >= 0 && lab < c;
    float v[LOSS_MAXC];
    const float ssum = channel_softmax(logits + n * c * hw + px, hw, c, v);
    float pl = 0.f, psum = 0.f;
    for (int k = 0; k < c; ++k) {
      const float pr = v[k] / ssum;
      psum += pr;
      if (k == lab) pl = pr;
    }
    acc[0] += pl;
    acc[1] += psum + (valid ? 1.f : 0.f);
    bad += valid ? 0u : 1u;
  }
  block_store_row<2>(acc, part + (long long)blockIdx.x * 2);
  if (bad_count && bad) atomicAdd(bad_count, (unsigned long long)bad);
}

__global__ __launch_bounds__(256) void dice_labels_bwd_kernel(const float* __restrict__ logits,
                                                             const uint8_t* __restrict__ l8,
                                                             const long long* __restrict__ l64, int c, long long hw,
                                                             long long npix, int nsamp, const float* __restrict__ coef,
                                                             const float* __restrict__ gout, float* __restrict__ dlogits) {
  const float g = (gout ? *gout : 1.f) * DiceOv::gscale / (float)nsamp;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npix; i += 256ll * gridDim.x) {
    const long long n = i / hw, px = i - n * hw;
    const long long base = n * c * hw + px;
    const long long lab = read_label(l8, l64, i);
    const float sa = coef[2 * n], sb = coef[2 * n + 1];
    float v[LOSS_MAXC];
    const float ssum = channel_softmax(logits + base, hw, c, v);
    float dot = 0.f;
    for (int k = 0; k < c; ++k) {
      v[k] = v[k] / ssum;
      dot += -g * ((k == lab ? sa : 0.f) - sb) * v[k];
    }
    for (int k = 0; k < c; ++k) dlogits[base + k * hw] = v[k] * (-g * ((k == lab ? sa : 0.f) - sb) - dot);
  }
}

// ============================================================================ host wrappers
namespace {
// workspace: [WS_HEAD doubles: sums] then
//   per class : [coef float 2 * LOSS_MAXC] [partial rows float blocks * nacc]
//   per sample: [samp double 2 n] [coef float 2 n] [partial rows float n * bps * nacc]
struct Layout {
  size_t samp, coef, part, total;
};
inline Layout layout_class(int blocks, int nacc) {
  Layout l;
  l.samp = l.coef = WS_HEAD * sizeof(double);
  l.part = l.coef + 2 * LOSS_MAXC * sizeof(float);
  l.total = l.part + (size_t)blocks * nacc * sizeof(float);
  return l;
}
inline Layout layout_sample(int n, int bps, int nacc) {
  Layout l;
  l.samp = WS_HEAD * sizeof(double);
  l.coef = l.samp + (size_t)n * 2 * sizeof(double);
  l.part = l.coef + (size_t)n * 2 * sizeof(float);
  l.total = l.part + (size_t)n * bps * nacc * sizeof(float);
  return l;
}
inline bool ov_known(int overlap) { return overlap == PCUDA_OV_DICE_CLASS || overlap == PCUDA_OV_DICE_SAMPLE; }
inline Layout ov_layout(int n, int c, long long hw, int overlap) {
  const int bps = sample_bps(n, hw, OV_BLOCKS);
  return overlap == PCUDA_OV_DICE_SAMPLE ? layout_sample(n, bps, 3) : layout_class(n * bps, 2 * c + 1);
}
inline Layout dice_layout(int n, int c, long long hw, int reduce) {
  return reduce == PCUDA_OV_DICE_SAMPLE ? layout_sample(n, sample_bps(n, (long long)c * hw, OV_BLOCKS), 2)
                                        : layout_class(DICE_BLOCKS, 2 * c);
}
inline Layout labels_layout(int n, long long hw) { return layout_sample(n, sample_bps(n, hw, OV_BLOCKS), 2); }

// the checks every entry point of the fused Dice form makes before it launches
int ov_check(const char* what, const void* logits, const void* onehot, const void* out, int mode, int overlap, int n, int c,
             long long hw, const void* workspace, size_t workspace_bytes) {
  if (int rc = seg_check_args(what, logits, onehot, out, mode == PCUDA_ACT_SIGMOID || mode == PCUDA_ACT_SOFTMAX, n, c, hw))
    return rc;
  if (!ov_known(overlap)) PCUDA_FAIL(PCUDA_E_BADARG, "%s: unknown overlap term %d", what, overlap);
  if (!workspace || workspace_bytes < ov_layout(n, c, hw, overlap).total)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "%s: workspace too small", what);
  return PCUDA_OK;
}
// ... and of Dice on given probabilities
int dice_check(const char* what, const void* in, const void* truth, const void* out, int reduce, int n, int c, long long hw,
               const void* workspace, size_t workspace_bytes) {
  if (int rc = probs_check_args(what, in, truth, out, n, c, hw)) return rc;
  if (!ov_known(reduce)) PCUDA_FAIL(PCUDA_E_BADARG, "%s: unknown reduction %d", what, reduce);
  if (!workspace || workspace_bytes < dice_layout(n, c, hw, reduce).total)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "%s: workspace too small", what);
  return PCUDA_OK;
}

// the reduce of a per-class forward: sums, coefficient pairs and the scalars
int launch_class_final(void* workspace, const Layout& l, int blocks, int c, int off, double numel_main, double eps, float* out,
                       hipStream_t s) {
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, 4.0 * blocks * (2 * c + off), s);
    hipLaunchKernelGGL(overlap_class_final_kernel<DiceOv>, dim3(1), dim3(256), 0, s, (const float*)((char*)workspace + l.part),
                       blocks, c, off, numel_main, eps, (double*)workspace, (float*)((char*)workspace + l.coef), out);
  }
  PCUDA_CHECK_LAUNCH("overlap_class_final_kernel");
  return PCUDA_OK;
}

// the two reduce stages of a per-sample forward
template <int NACC>
int launch_sample_reduce(const char* what, void* workspace, const Layout& l, int n, int bps, double eps, double numel_main,
                         float* out, hipStream_t s) {
  double* sums = (double*)workspace;
  double* samp = (double*)((char*)workspace + l.samp);
  float* coef = (float*)((char*)workspace + l.coef);
  const float* part = (const float*)((char*)workspace + l.part);
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, 4.0 * n * bps * NACC + 24.0 * n, s);
    hipLaunchKernelGGL(dice_sample_reduce_kernel<NACC>, dim3((n + 3) / 4), dim3(256), 0, s, part, n, bps, eps, coef, samp);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) PCUDA_FAIL(PCUDA_E_LAUNCH, "%s: dice_sample_reduce_kernel: %s", what, hipGetErrorString(e));
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, 16.0 * n, s);
    hipLaunchKernelGGL(dice_sample_final_kernel, dim3(1), dim3(256), 0, s, (const double*)samp, n, NACC == 3 ? 1 : 0,
                       numel_main, sums, out);
  }
  e = hipGetLastError();
  if (e != hipSuccess) PCUDA_FAIL(PCUDA_E_LAUNCH, "%s: dice_sample_final_kernel: %s", what, hipGetErrorString(e));
  return PCUDA_OK;
}
}  // namespace

extern "C" size_t pcuda_seg_loss_ov_workspace_size(int n, int c, long long hw, int overlap) {
  if (n <= 0 || c <= 0 || c > OV_MAXC || hw <= 0 || !ov_known(overlap)) return 0;
  return ov_layout(n, c, hw, overlap).total;
}

extern "C" int pcuda_seg_loss_ov_fwd(const float* logits, const uint8_t* onehot, int mode, int overlap, double eps, int n,
                                     int c, long long hw, float* out2, void* workspace, size_t workspace_bytes,
                                     pcuda_stream_t s) {
  if (!(eps >= 0.0)) PCUDA_FAIL(PCUDA_E_BADARG, "seg_loss_ov_fwd: bad arguments");
  if (int rc = ov_check("seg_loss_ov_fwd", logits, onehot, out2, mode, overlap, n, c, hw, workspace, workspace_bytes)) return rc;
  const Layout l = ov_layout(n, c, hw, overlap);
  const long long npix = (long long)n * hw;
  const double numel_main = seg_numel_main(mode, n, c, hw);
  float* part = (float*)((char*)workspace + l.part);
  hipStream_t st = (hipStream_t)s;
  const int bps = sample_bps(n, hw, OV_BLOCKS);
  const unsigned blocks = (unsigned)n * bps;
  const bool sample = overlap == PCUDA_OV_DICE_SAMPLE;
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, 5.0 * npix * c, st);
#define OV_CASE(CC)                                                                                                           \
  case CC:                                                                                                                    \
    if (sample)                                                                                                               \
      hipLaunchKernelGGL((seg_partial_kernel<CC, true, true>), dim3(blocks), dim3(256), 0, st, logits, onehot, mode, hw, npix, bps, part); \
    else                                                                                                                      \
      hipLaunchKernelGGL((seg_partial_kernel<CC, true, false>), dim3(blocks), dim3(256), 0, st, logits, onehot, mode, hw, npix, bps, part); \
    break;
    switch (c) { OV_CASE(1) OV_CASE(2) OV_CASE(3) OV_CASE(4) OV_CASE(5) OV_CASE(6) OV_CASE(7) OV_CASE(8) }
#undef OV_CASE
  }
  PCUDA_CHECK_LAUNCH("seg_partial_kernel");
  if (sample) return launch_sample_reduce<3>("seg_loss_ov_fwd", workspace, l, n, bps, eps, numel_main, out2, st);
  return launch_class_final(workspace, l, (int)blocks, c, 1, numel_main, eps, out2, st);
}

extern "C" int pcuda_seg_loss_ov_bwd(const float* logits, const uint8_t* onehot, int mode, int overlap, int n, int c,
                                     long long hw, const float* g_main, const float* g_ov, float* dlogits,
                                     const void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (int rc = ov_check("seg_loss_ov_bwd", logits, onehot, dlogits, mode, overlap, n, c, hw, workspace, workspace_bytes)) return rc;
  const float* coef = (const float*)((const char*)workspace + ov_layout(n, c, hw, overlap).coef);
  const double numel_main = seg_numel_main(mode, n, c, hw);
  hipStream_t st = (hipStream_t)s;
  const int bps = sample_bps(n, hw, 4096);
  const unsigned blocks = (unsigned)n * bps;
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, 9.0 * n * hw * c, st);
    if (overlap == PCUDA_OV_DICE_CLASS)
      hipLaunchKernelGGL((seg_bwd_kernel<DiceOv, false>), dim3(blocks), dim3(256), 0, st, logits, onehot, mode, c, hw, bps,
                         numel_main, coef, c, g_main, g_ov, dlogits);
    else
      hipLaunchKernelGGL((seg_bwd_kernel<DiceOv, true>), dim3(blocks), dim3(256), 0, st, logits, onehot, mode, c, hw, bps,
                         numel_main, coef, n, g_main, g_ov, dlogits);
  }
  PCUDA_CHECK_LAUNCH("seg_bwd_kernel");
  return PCUDA_OK;
}

extern "C" size_t pcuda_dice_workspace_size(int n, int c, long long hw, int reduce) {
  if (n <= 0 || c <= 0 || c > LOSS_MAXC || hw <= 0 || !ov_known(reduce)) return 0;
  return dice_layout(n, c, hw, reduce).total;
}

extern "C" int pcuda_dice_fwd(const float* probs, const void* truth, int truth_is_u8, int n, int c, long long hw,
                              int reduce, float eps, float* loss, void* workspace, size_t workspace_bytes,
                              pcuda_stream_t s) {
  if (!(eps >= 0.f)) PCUDA_FAIL(PCUDA_E_BADARG, "dice_fwd: bad arguments");
  if (int rc = dice_check("dice_fwd", probs, truth, loss, reduce, n, c, hw, workspace, workspace_bytes)) return rc;
  const Layout l = dice_layout(n, c, hw, reduce);
  const long long npix = (long long)n * hw;
  const float* tf = truth_is_u8 ? nullptr : (const float*)truth;
  const uint8_t* tu = truth_is_u8 ? (const uint8_t*)truth : nullptr;
  const double bytes = (truth_is_u8 ? 5.0 : 8.0) * npix * c;
  float* part = (float*)((char*)workspace + l.part);
  hipStream_t st = (hipStream_t)s;
  if (reduce == PCUDA_OV_DICE_CLASS) {
    int blocks = grid_for(npix);
    if (blocks > DICE_BLOCKS) blocks = DICE_BLOCKS;
    {
      ProfScope prof(PCUDA_FAM_POINTWISE, bytes, st);
      hipLaunchKernelGGL(overlap_class_partial_kernel, dim3(blocks, c), dim3(256), 0, st, probs, tf, tu, c, hw, npix, part);
    }
    PCUDA_CHECK_LAUNCH("overlap_class_partial_kernel");
    return launch_class_final(workspace, l, blocks, c, 0, 1.0, (double)eps, loss, st);
  }
  const long long len = (long long)c * hw;
  const int bps = sample_bps(n, len, OV_BLOCKS);
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, bytes, st);
    hipLaunchKernelGGL(dice_sample_partial_kernel, dim3((unsigned)n * bps), dim3(256), 0, st, probs, tf, tu, len, bps, part);
  }
  PCUDA_CHECK_LAUNCH("dice_sample_partial_kernel");
  return launch_sample_reduce<2>("dice_fwd", workspace, l, n, bps, (double)eps, 1.0, loss, st);
}

extern "C" int pcuda_dice_bwd(const void* truth, int truth_is_u8, int n, int c, long long hw, int reduce,
                              const float* gout, float* dprobs, const void* workspace, size_t workspace_bytes,
                              pcuda_stream_t s) {
  if (int rc = dice_check("dice_bwd", truth, truth, dprobs, reduce, n, c, hw, workspace, workspace_bytes)) return rc;
  const long long numel = (long long)n * c * hw;
  const bool sample = reduce == PCUDA_OV_DICE_SAMPLE;
  ProfScope prof(PCUDA_FAM_POINTWISE, (truth_is_u8 ? 5.0 : 8.0) * numel, (hipStream_t)s);
  hipLaunchKernelGGL((overlap_bwd_kernel<DiceOv, false>), dim3(grid_for(numel)), dim3(256), 0, (hipStream_t)s,
                     truth_is_u8 ? nullptr : (const float*)truth, truth_is_u8 ? (const uint8_t*)truth : nullptr, numel,
                     sample ? (long long)c * hw : hw, sample ? n : c, sample ? n : c,
                     (const float*)((const char*)workspace + dice_layout(n, c, hw, reduce).coef), (const double*)nullptr, 0.0,
                     gout, dprobs);
  PCUDA_CHECK_LAUNCH("overlap_bwd_kernel");
  return PCUDA_OK;
}

extern "C" size_t pcuda_dice_labels_workspace_size(int n, int c, long long hw) {
  if (n <= 0 || c <= 0 || c > LOSS_MAXC || hw <= 0) return 0;
  return labels_layout(n, hw).total;
}

extern "C" int pcuda_dice_labels_fwd(const float* logits, const void* labels, int labels_are_i64, int n, int c,
                                     long long hw, float eps, float* loss, unsigned long long* bad_count, void* workspace,
                                     size_t workspace_bytes, pcuda_stream_t s) {
  if (!logits || !labels || !loss || n <= 0 || c <= 0 || c > LOSS_MAXC || hw <= 0 || !(eps >= 0.f))
    PCUDA_FAIL(PCUDA_E_BADARG, "dice_labels_fwd: bad arguments (1..%d classes)", LOSS_MAXC);
  const int bps = sample_bps(n, hw, OV_BLOCKS);
  const Layout l = labels_layout(n, hw);
  if (!workspace || workspace_bytes < l.total) PCUDA_FAIL(PCUDA_E_WORKSPACE, "dice_labels_fwd: workspace too small");
  hipStream_t st = (hipStream_t)s;
  if (bad_count && hipMemsetAsync(bad_count, 0, sizeof(unsigned long long), st) != hipSuccess)
    PCUDA_FAIL(PCUDA_E_LAUNCH, "dice_labels_fwd: memset failed");
  const long long npix = (long long)n * hw;
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, (4.0 * c + (labels_are_i64 ? 8.0 : 1.0)) * npix, st);
    hipLaunchKernelGGL(dice_labels_partial_kernel, dim3((unsigned)n * bps), dim3(256), 0, st, logits,
                       labels_are_i64 ? nullptr : (const uint8_t*)labels, labels_are_i64 ? (const long long*)labels : nullptr,
                       c, hw, bps, (float*)((char*)workspace + l.part), bad_count);
  }
  PCUDA_CHECK_LAUNCH("dice_labels_partial_kernel");
  return launch_sample_reduce<2>("dice_labels_fwd", workspace, l, n, bps, (double)eps, 1.0, loss, st);
}

extern "C" int pcuda_dice_labels_bwd(const float* logits, const void* labels, int labels_are_i64, int n, int c,
                                     long long hw, const float* gout, float* dlogits, const void* workspace,
                                     size_t workspace_bytes, pcuda_stream_t s) {
  if (!logits || !labels || !dlogits || n <= 0 || c <= 0 || c > LOSS_MAXC || hw <= 0)
    PCUDA_FAIL(PCUDA_E_BADARG, "dice_labels_bwd: bad arguments (1..%d classes)", LOSS_MAXC);
  const Layout l = labels_layout(n, hw);
  if (!workspace || workspace_bytes < l.total) PCUDA_FAIL(PCUDA_E_WORKSPACE, "dice_labels_bwd: workspace too small");
  const long long npix = (long long)n * hw;
  ProfScope prof(PCUDA_FAM_POINTWISE, (8.0 * c + (labels_are_i64 ? 8.0 : 1.0) + 8.0) * npix, (hipStream_t)s);
  hipLaunchKernelGGL(dice_labels_bwd_kernel, dim3(grid_for(npix)), dim3(256), 0, (hipStream_t)s, logits,
                     labels_are_i64 ? nullptr : (const uint8_t*)labels, labels_are_i64 ? (const long long*)labels : nullptr, c,
                     hw, npix, n, (const float*)((const char*)workspace + l.coef), gout, dlogits);
  PCUDA_CHECK_LAUNCH("dice_labels_bwd_kernel");
  return PCUDA_OK;
}
