// Dice loss on the device (the -dice switch of both training scripts; this build's own rule, include/pcuda_hip.h):
//   per class   I_c = sum p*y, S_c = sum (p + y) over (batch, pixels); loss = 1 - mean_c 2 I_c / (S_c + eps)
//   per sample  I_n, S_n over (classes, pixels);                      loss = mean_n (1 - 2 I_n / (S_n + eps))
//   d loss / d p = -(2 / M) (y / (S + eps) - I / (S + eps)^2), the sums of the element's own class or sample, M = C or N
// Three families: the fused segmentation loss with a Dice overlap term (pcuda_seg_loss_ov_*), Dice on given probabilities
// (pcuda_dice_*), Dice on logits + a label map (pcuda_dice_labels_*).
//
// Every forward is: block partial rows (fp32) -> a fixed-order reduce in double -> the scalars and the coefficients
// a = 1 / (S + eps), b = I / (S + eps)^2 per class or per sample, left in the workspace for the backward pass.  No floating
// point atomics: the same bits from run to run.  A per-sample partial row belongs to ONE sample: the grid of a per-sample
// pass is (sample, chunk) pairs laid out on the x axis (n * bps blocks; n is not bounded by a grid's y limit).
#include "loss_device.h"

#define DICE_MAXC 16       // classes of the stand-alone forms
#define OV_MAXC 8          // classes of the fused form (as seg_loss)
#define OV_BLOCKS 1024     // blocks a (sample, chunk) forward pass aims at (more only where n alone exceeds it)
#define DICE_BLOCKS 256    // block cap (per class) of the stand-alone per-class pass
#define WS_HEAD 64         // doubles in front of every workspace: the reduced sums

// ---------------------------------------------------------------------------- shared pieces
// the block's sum of every accumulator -> one partial row (waves in a fixed order)
template <int NACC>
__device__ __forceinline__ void block_store_row(const float (&acc)[NACC], float* __restrict__ row) {
  __shared__ float sh[4][NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) {
    const float s = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NACC)
    row[threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// sum over the 256 threads of a block, fixed order; every thread gets it
__device__ __forceinline__ double block_tree_sum(double s, double* red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// per-class reduce of `nblocks` partial rows of nacc = 2 c + off floats: [main (off = 1)] [I_0..I_{c-1}] [S_0..S_{c-1}]
//   sums[a] = every accumulator in double; coef[2k], coef[2k+1] = a_k, b_k; out = [main / numel_main,] 1 - mean_c 2I/(S+eps)
__global__ __launch_bounds__(256) void dice_class_final_kernel(const float* __restrict__ part, int nblocks, int c, int off,
                                                              double numel_main, double eps, double* __restrict__ sums,
                                                              float* __restrict__ coef, float* __restrict__ out) {
  __shared__ double sh[2 * DICE_MAXC + 1];
  __shared__ double red[256];
  const int nacc = 2 * c + off;
  for (int a = 0; a < nacc; ++a) {
    double s = 0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += (double)part[(long long)b * nacc + a];
    const double tot = block_tree_sum(s, red);
    if (threadIdx.x == 0) { sums[a] = tot; sh[a] = tot; }
  }
  __syncthreads();
  if ((int)threadIdx.x < c) {
    const double I = sh[off + threadIdx.x], d = sh[off + c + threadIdx.x] + eps;
    coef[2 * threadIdx.x] = (float)(1.0 / d);
    coef[2 * threadIdx.x + 1] = (float)(I / (d * d));
  }
  if (threadIdx.x == 0) {
    double t = 0;
    for (int k = 0; k < c; ++k) t += 2.0 * sh[off + k] / (sh[off + c + k] + eps);
    if (off) out[0] = (float)(sh[0] / numel_main);
    out[off] = (float)(1.0 - t / c);
  }
}

// per-sample reduce, stage 1: one wave per sample over its bps partial rows of NACC floats: [main (NACC = 3)] [I] [S]
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
    const double I = acc[NACC - 2], d = acc[NACC - 1] + eps;
    coef[2ll * smp] = (float)(1.0 / d);
    coef[2ll * smp + 1] = (float)(I / (d * d));
    samp[2ll * smp] = 2.0 * I / d;
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

// ---------------------------------------------------------------------------- fused segmentation loss, Dice overlap
// one pixel: the main term (BCE with the -100 clamp, or the double-softmax cross entropy: what seg_loss computes), and per
// class pi = p * y, ps = p + y
template <int C>
__device__ __forceinline__ float seg_pixel(const float* __restrict__ lp, const uint8_t* __restrict__ yp, long long hw,
                                           int mode, float (&pi)[C], float (&ps)[C]) {
  float main = 0.f;
  if (mode == PCUDA_ACT_SIGMOID) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float pr = sigmoidf_(lp[k * hw]);
      const float y = (float)yp[k * hw];
      const float l1 = fmaxf(logf(pr), -100.f), l0 = fmaxf(logf(1.f - pr), -100.f);   // torch BCELoss clamps each log
      main += -(y * l1 + (1.f - y) * l0);
      pi[k] = pr * y;
      ps[k] = pr + y;
    }
  } else {
    float v[C];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < C; ++k) { v[k] = lp[k * hw]; m = fmaxf(m, v[k]); }
    float ssum = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) { v[k] = expf(v[k] - m); ssum += v[k]; }
    uint8_t best = 0;
    float pm = -INFINITY, plabel = 0.f;
    bool first = true;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float pr = v[k] / ssum;
      v[k] = pr;
      const uint8_t yk = yp[k * hw];
      if (first || yk > best) { best = yk; plabel = pr; first = false; }   // first maximum = np.argmax
      pm = fmaxf(pm, pr);
      pi[k] = pr * (float)yk;
      ps[k] = pr + (float)yk;
    }
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) s2 += expf(v[k] - pm);
    main = -(plabel - pm - logf(s2));   // -log_softmax(p)[label]
  }
  return main;
}

// forward pass: block = (sample, chunk) = (blockIdx.x / bps, blockIdx.x % bps) walks its chunk of ITS sample's pixels (no
// division per pixel).  Partial row per block: per sample [main, I, S], per class [main, I_0.., S_0..] (rows of different
// samples are summed by the per-class reduce, which is what that reduction asks for)
template <int C, bool SAMPLE>
__global__ __launch_bounds__(256) void seg_ov_partial_kernel(const float* __restrict__ logits,
                                                            const uint8_t* __restrict__ onehot, int mode, long long hw,
                                                            int bps, float* __restrict__ part) {
  constexpr int NACC = SAMPLE ? 3 : 2 * C + 1;
  const long long n = blockIdx.x / (unsigned)bps;
  const int j = (int)(blockIdx.x - n * bps);
  float acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
  for (long long px = j * 256ll + threadIdx.x; px < hw; px += 256ll * bps) {
    const long long base = n * C * hw + px;
    float pi[C], ps[C];
    acc[0] += seg_pixel<C>(logits + base, onehot + base, hw, mode, pi, ps);
#pragma unroll
    for (int k = 0; k < C; ++k) {
      acc[SAMPLE ? 1 : 1 + k] += pi[k];
      acc[SAMPLE ? 2 : 1 + C + k] += ps[k];
    }
  }
  block_store_row<NACC>(acc, part + (long long)blockIdx.x * NACC);
}

// dlogits = (g_main * d main / d p + g_ov * d dice / d p) through the sigmoid / softmax Jacobian (seg_loss_bwd_kernel's).
// block = (sample, chunk) as in the forward pass.  coef: per class [c][2] (held in LDS) or per sample [n][2] (the block's own
// pair, read from the workspace: n is not bounded by LDS); m = c or n
template <bool SAMPLE>
__global__ __launch_bounds__(256) void seg_ov_bwd_kernel(const float* __restrict__ logits,
                                                         const uint8_t* __restrict__ onehot, int mode, int c, long long hw,
                                                         int bps, double numel_main, const float* __restrict__ coef, int m,
                                                         const float* __restrict__ g_main, const float* __restrict__ g_ov,
                                                         float* __restrict__ dlogits) {
  __shared__ float ca[OV_MAXC], cb[OV_MAXC];
  const long long n = blockIdx.x / (unsigned)bps;
  const int j = (int)(blockIdx.x - n * bps);
  if (!SAMPLE) {
    if ((int)threadIdx.x < c) { ca[threadIdx.x] = coef[2 * threadIdx.x]; cb[threadIdx.x] = coef[2 * threadIdx.x + 1]; }
    __syncthreads();
  }
  const float sa = SAMPLE ? coef[2 * n] : 0.f, sb = SAMPLE ? coef[2 * n + 1] : 0.f;
  const float gm = (g_main ? *g_main : 1.f) / (float)numel_main;
  const float gd = (g_ov ? *g_ov : 1.f) * 2.f / (float)m;
  for (long long px = j * 256ll + threadIdx.x; px < hw; px += 256ll * bps) {
    const long long base = n * c * hw + px;
    if (mode == PCUDA_ACT_SIGMOID) {
      for (int k = 0; k < c; ++k) {
        const float pr = sigmoidf_(logits[base + k * hw]);
        const float y = (float)onehot[base + k * hw];
        const float pq = pr * (1.f - pr);
        // torch: BCE backward divides by max(p(1-p), 1e-12), sigmoid backward multiplies by p(1-p)
        const float gb = gm * (pr - y) / fmaxf(pq, 1e-12f);
        const float gov = -gd * (y * (SAMPLE ? sa : ca[k]) - (SAMPLE ? sb : cb[k]));
        dlogits[base + k * hw] = (gb + gov) * pq;
      }
    } else {
      float v[OV_MAXC], gp[OV_MAXC];
      float mx = -INFINITY;
      for (int k = 0; k < c; ++k) { v[k] = logits[base + k * hw]; mx = fmaxf(mx, v[k]); }
      float ssum = 0.f;
      for (int k = 0; k < c; ++k) { v[k] = expf(v[k] - mx); ssum += v[k]; }
      int label = 0;
      uint8_t best = 0;
      float pm = -INFINITY;
      for (int k = 0; k < c; ++k) {
        v[k] = v[k] / ssum;
        const uint8_t yk = onehot[base + k * hw];
        if (yk > best) { best = yk; label = k; }
        pm = fmaxf(pm, v[k]);
      }
      float s2 = 0.f;
      for (int k = 0; k < c; ++k) s2 += expf(v[k] - pm);
      float dot = 0.f;
      for (int k = 0; k < c; ++k) {
        const float y = (float)onehot[base + k * hw];
        const float sm2 = expf(v[k] - pm) / s2;
        const float g = gm * (sm2 - (k == label ? 1.f : 0.f)) - gd * (y * (SAMPLE ? sa : ca[k]) - (SAMPLE ? sb : cb[k]));
        gp[k] = g;
        dot += g * v[k];
      }
      for (int k = 0; k < c; ++k) dlogits[base + k * hw] = v[k] * (gp[k] - dot);
    }
  }
}

// ---------------------------------------------------------------------------- Dice on given probabilities
// per class: as jaccard_partial_kernel (class on the grid's y axis); partial row [I_0..I_{c-1}, S_0..S_{c-1}] per x block
__global__ __launch_bounds__(256) void dice_class_partial_kernel(const float* __restrict__ p, const float* __restrict__ tf,
                                                                const uint8_t* __restrict__ tu, int c, long long hw,
                                                                long long npix, float* __restrict__ part) {
  __shared__ float sh[4][2];
  const int k = blockIdx.y;
  float a0 = 0.f, a1 = 0.f;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npix; i += 256ll * gridDim.x) {
    const long long n = i / hw, px = i - n * hw;
    const long long o = (n * c + k) * hw + px;
    const float pr = p[o], y = tf ? tf[o] : (float)tu[o];
    a0 += pr * y;
    a1 += pr + y;
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][0] = a0; sh[threadIdx.x >> 6][1] = a1; }
  __syncthreads();
  if (threadIdx.x < 2)
    part[(long long)blockIdx.x * 2 * c + threadIdx.x * c + k] =
        (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// per sample: a sample's c * hw values are contiguous (len of them); block = (sample, chunk), partial row [I, S]
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

// dp = -(gout * 2 / m) (y a - b); the element's coefficient pair is (o / seg) % mod: (hw, c) per class, (c hw, n) per sample
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ tf, const uint8_t* __restrict__ tu,
                                                       long long numel, long long seg, int mod, int m,
                                                       const float* __restrict__ coef, const float* __restrict__ gout,
                                                       float* __restrict__ dp) {
  const float g = (gout ? *gout : 1.f) * 2.f / (float)m;
  for (long long o = blockIdx.x * 256ll + threadIdx.x; o < numel; o += 256ll * gridDim.x) {
    const long long q = (o / seg) % mod;
    const float y = tf ? tf[o] : (float)tu[o];
    dp[o] = -g * (y * coef[2 * q] - coef[2 * q + 1]);
  }
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
    const float* lp = logits + n * c * hw + px;
    const long long lab = read_label(l8, l64, n * hw + px);
    const bool valid = lab >= 0 && lab < c;
    float v[DICE_MAXC];
    float m = -INFINITY;
    for (int k = 0; k < c; ++k) { v[k] = lp[k * hw]; m = fmaxf(m, v[k]); }
    float ssum = 0.f;
    for (int k = 0; k < c; ++k) { v[k] = expf(v[k] - m); ssum += v[k]; }
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
  const float g = (gout ? *gout : 1.f) * 2.f / (float)nsamp;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npix; i += 256ll * gridDim.x) {
    const long long n = i / hw, px = i - n * hw;
    const long long base = n * c * hw + px;
    const long long lab = read_label(l8, l64, i);
    const float sa = coef[2 * n], sb = coef[2 * n + 1];
    float v[DICE_MAXC];
    float m = -INFINITY;
    for (int k = 0; k < c; ++k) { v[k] = logits[base + k * hw]; m = fmaxf(m, v[k]); }
    float ssum = 0.f;
    for (int k = 0; k < c; ++k) { v[k] = expf(v[k] - m); ssum += v[k]; }
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
//   per class : [coef float 2 * DICE_MAXC] [partial rows float blocks * nacc]
//   per sample: [samp double 2 n] [coef float 2 n] [partial rows float n * bps * nacc]
struct Layout {
  size_t samp, coef, part, total;
};
inline Layout layout_class(int blocks, int nacc) {
  Layout l;
  l.samp = l.coef = WS_HEAD * sizeof(double);
  l.part = l.coef + 2 * DICE_MAXC * sizeof(float);
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
// chunks per sample of a (sample, chunk) pass over `len` values each: one block per 256 values, about `blocks` blocks in all
inline int sample_bps(int n, long long len, int blocks = OV_BLOCKS) {
  const long long want = (len + 255) / 256, cap = blocks / n > 1 ? blocks / n : 1;
  return (int)(want < cap ? want : cap);
}
inline bool ov_known(int overlap) { return overlap == PCUDA_OV_DICE_CLASS || overlap == PCUDA_OV_DICE_SAMPLE; }
inline Layout ov_layout(int n, int c, long long hw, int overlap) {
  const int bps = sample_bps(n, hw);
  return overlap == PCUDA_OV_DICE_SAMPLE ? layout_sample(n, bps, 3) : layout_class(n * bps, 2 * c + 1);
}
inline Layout dice_layout(int n, int c, long long hw, int reduce) {
  return reduce == PCUDA_OV_DICE_SAMPLE ? layout_sample(n, sample_bps(n, (long long)c * hw), 2)
                                        : layout_class(DICE_BLOCKS, 2 * c);
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
  if (!logits || !onehot || !out2 || n <= 0 || c <= 0 || hw <= 0 ||
      (mode != PCUDA_ACT_SIGMOID && mode != PCUDA_ACT_SOFTMAX) || !(eps >= 0.0))
    PCUDA_FAIL(PCUDA_E_BADARG, "seg_loss_ov_fwd: bad arguments");
  if (!ov_known(overlap)) PCUDA_FAIL(PCUDA_E_BADARG, "seg_loss_ov_fwd: unknown overlap term %d", overlap);
  if (c > OV_MAXC) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "seg_loss_ov: at most %d classes (got %d)", OV_MAXC, c);
  const Layout l = ov_layout(n, c, hw, overlap);
  if (!workspace || workspace_bytes < l.total) PCUDA_FAIL(PCUDA_E_WORKSPACE, "seg_loss_ov_fwd: workspace too small");
  const long long npix = (long long)n * hw;
  const double numel_main = mode == PCUDA_ACT_SIGMOID ? (double)npix * c : (double)npix;
  float* part = (float*)((char*)workspace + l.part);
  hipStream_t st = (hipStream_t)s;
  const int bps = sample_bps(n, hw);
  const unsigned blocks = (unsigned)n * bps;
  const bool sample = overlap == PCUDA_OV_DICE_SAMPLE;
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, 5.0 * npix * c, st);
#define OV_CASE(CC)                                                                                                           \
  case CC:                                                                                                                    \
    if (sample)                                                                                                               \
      hipLaunchKernelGGL((seg_ov_partial_kernel<CC, true>), dim3(blocks), dim3(256), 0, st, logits, onehot, mode, hw, bps, part); \
    else                                                                                                                      \
      hipLaunchKernelGGL((seg_ov_partial_kernel<CC, false>), dim3(blocks), dim3(256), 0, st, logits, onehot, mode, hw, bps, part); \
    break;
    switch (c) { OV_CASE(1) OV_CASE(2) OV_CASE(3) OV_CASE(4) OV_CASE(5) OV_CASE(6) OV_CASE(7) OV_CASE(8) }
#undef OV_CASE
  }
  PCUDA_CHECK_LAUNCH("seg_ov_partial_kernel");
  if (sample) return launch_sample_reduce<3>("seg_loss_ov_fwd", workspace, l, n, bps, eps, numel_main, out2, st);
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, 4.0 * blocks * (2 * c + 1), st);
    hipLaunchKernelGGL(dice_class_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (int)blocks, c, 1, numel_main,
                       eps, (double*)workspace, (float*)((char*)workspace + l.coef), out2);
  }
  PCUDA_CHECK_LAUNCH("dice_class_final_kernel");
  return PCUDA_OK;
}

extern "C" int pcuda_seg_loss_ov_bwd(const float* logits, const uint8_t* onehot, int mode, int overlap, int n, int c,
                                     long long hw, const float* g_main, const float* g_ov, float* dlogits,
                                     const void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (!logits || !onehot || !dlogits || n <= 0 || c <= 0 || hw <= 0 ||
      (mode != PCUDA_ACT_SIGMOID && mode != PCUDA_ACT_SOFTMAX))
    PCUDA_FAIL(PCUDA_E_BADARG, "seg_loss_ov_bwd: bad arguments");
  if (!ov_known(overlap)) PCUDA_FAIL(PCUDA_E_BADARG, "seg_loss_ov_bwd: unknown overlap term %d", overlap);
  if (c > OV_MAXC) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "seg_loss_ov: at most %d classes (got %d)", OV_MAXC, c);
  const Layout l = ov_layout(n, c, hw, overlap);
  if (!workspace || workspace_bytes < l.total) PCUDA_FAIL(PCUDA_E_WORKSPACE, "seg_loss_ov_bwd: workspace too small");
  const long long npix = (long long)n * hw;
  const double numel_main = mode == PCUDA_ACT_SIGMOID ? (double)npix * c : (double)npix;
  const float* coef = (const float*)((const char*)workspace + l.coef);
  hipStream_t st = (hipStream_t)s;
  const int bps = sample_bps(n, hw, 4096);
  const unsigned blocks = (unsigned)n * bps;
  {
    ProfScope prof(PCUDA_FAM_POINTWISE, 9.0 * npix * c, st);
    if (overlap == PCUDA_OV_DICE_CLASS)
      hipLaunchKernelGGL(seg_ov_bwd_kernel<false>, dim3(blocks), dim3(256), 0, st, logits, onehot, mode, c, hw, bps,
                         numel_main, coef, c, g_main, g_ov, dlogits);
    else
      hipLaunchKernelGGL(seg_ov_bwd_kernel<true>, dim3(blocks), dim3(256), 0, st, logits, onehot, mode, c, hw, bps,
                         numel_main, coef, n, g_main, g_ov, dlogits);
  }
  PCUDA_CHECK_LAUNCH("seg_ov_bwd_kernel");
  return PCUDA_OK;
}

extern "C" size_t pcuda_dice_workspace_size(int n, int c, long long hw, int reduce) {
  if (n <= 0 || c <= 0 || c > DICE_MAXC || hw <= 0 || !ov_known(reduce)) return 0;
  return dice_layout(n, c, hw, reduce).total;
}

extern "C" int pcuda_dice_fwd(const float* probs, const void* truth, int truth_is_u8, int n, int c, long long hw,
                              int reduce, float eps, float* loss, void* workspace, size_t workspace_bytes,
                              pcuda_stream_t s) {
  if (!probs || !truth || !loss || n <= 0 || c <= 0 || c > DICE_MAXC || hw <= 0 || !(eps >= 0.f))
    PCUDA_FAIL(PCUDA_E_BADARG, "dice_fwd: bad arguments (1..%d classes)", DICE_MAXC);
  if (!ov_known(reduce)) PCUDA_FAIL(PCUDA_E_BADARG, "dice_fwd: unknown reduction %d", reduce);
  const Layout l = dice_layout(n, c, hw, reduce);
  if (!workspace || workspace_bytes < l.total) PCUDA_FAIL(PCUDA_E_WORKSPACE, "dice_fwd: workspace too small");
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
      hipLaunchKernelGGL(dice_class_partial_kernel, dim3(blocks, c), dim3(256), 0, st, probs, tf, tu, c, hw, npix, part);
    }
    PCUDA_CHECK_LAUNCH("dice_class_partial_kernel");
    {
      ProfScope prof(PCUDA_FAM_POINTWISE, 4.0 * blocks * 2 * c, st);
      hipLaunchKernelGGL(dice_class_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, blocks, c, 0, 1.0,
                         (double)eps, (double*)workspace, (float*)((char*)workspace + l.coef), loss);
    }
    PCUDA_CHECK_LAUNCH("dice_class_final_kernel");
    return PCUDA_OK;
  }
  const long long len = (long long)c * hw;
  const int bps = sample_bps(n, len);
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
  if (!truth || !dprobs || n <= 0 || c <= 0 || c > DICE_MAXC || hw <= 0)
    PCUDA_FAIL(PCUDA_E_BADARG, "dice_bwd: bad arguments (1..%d classes)", DICE_MAXC);
  if (!ov_known(reduce)) PCUDA_FAIL(PCUDA_E_BADARG, "dice_bwd: unknown reduction %d", reduce);
  const Layout l = dice_layout(n, c, hw, reduce);
  if (!workspace || workspace_bytes < l.total) PCUDA_FAIL(PCUDA_E_WORKSPACE, "dice_bwd: workspace too small");
  const long long numel = (long long)n * c * hw;
  const bool sample = reduce == PCUDA_OV_DICE_SAMPLE;
  ProfScope prof(PCUDA_FAM_POINTWISE, (truth_is_u8 ? 5.0 : 8.0) * numel, (hipStream_t)s);
  hipLaunchKernelGGL(dice_bwd_kernel, dim3(grid_for(numel)), dim3(256), 0, (hipStream_t)s,
                     truth_is_u8 ? nullptr : (const float*)truth, truth_is_u8 ? (const uint8_t*)truth : nullptr, numel,
                     sample ? (long long)c * hw : hw, sample ? n : c, sample ? n : c,
                     (const float*)((const char*)workspace + l.coef), gout, dprobs);
  PCUDA_CHECK_LAUNCH("dice_bwd_kernel");
  return PCUDA_OK;
}

extern "C" size_t pcuda_dice_labels_workspace_size(int n, int c, long long hw) {
  if (n <= 0 || c <= 0 || c > DICE_MAXC || hw <= 0) return 0;
  return layout_sample(n, sample_bps(n, hw), 2).total;
}

extern "C" int pcuda_dice_labels_fwd(const float* logits, const void* labels, int labels_are_i64, int n, int c,
                                     long long hw, float eps, float* loss, unsigned long long* bad_count, void* workspace,
                                     size_t workspace_bytes, pcuda_stream_t s) {
  if (!logits || !labels || !loss || n <= 0 || c <= 0 || c > DICE_MAXC || hw <= 0 || !(eps >= 0.f))
    PCUDA_FAIL(PCUDA_E_BADARG, "dice_labels_fwd: bad arguments (1..%d classes)", DICE_MAXC);
  const int bps = sample_bps(n, hw);
  const Layout l = layout_sample(n, bps, 2);
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
  if (!logits || !labels || !dlogits || n <= 0 || c <= 0 || c > DICE_MAXC || hw <= 0)
    PCUDA_FAIL(PCUDA_E_BADARG, "dice_labels_bwd: bad arguments (1..%d classes)", DICE_MAXC);
  const Layout l = layout_sample(n, sample_bps(n, hw), 2);
  if (!workspace || workspace_bytes < l.total) PCUDA_FAIL(PCUDA_E_WORKSPACE, "dice_labels_bwd: workspace too small");
  const long long npix = (long long)n * hw;
  ProfScope prof(PCUDA_FAM_POINTWISE, (8.0 * c + (labels_are_i64 ? 8.0 : 1.0) + 8.0) * npix, (hipStream_t)s);
  hipLaunchKernelGGL(dice_labels_bwd_kernel, dim3(grid_for(npix)), dim3(256), 0, (hipStream_t)s, logits,
                     labels_are_i64 ? nullptr : (const uint8_t*)labels, labels_are_i64 ? (const long long*)labels : nullptr, c,
                     hw, npix, n, (const float*)((const char*)workspace + l.coef), gout, dlogits);
  PCUDA_CHECK_LAUNCH("dice_labels_bwd_kernel");
  return PCUDA_OK;
}
