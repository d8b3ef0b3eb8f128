// What the loss sources (losses.hip, dice_loss.hip) share: the per-pixel channel softmax, the block reductions, and the
// overlap-loss family.  Jaccard and Dice are one family: a ratio of the same two sums I = sum p y and S = sum (p + y), a
// coefficient pair (a, b) per class or per sample, and a gradient that is linear in y.  The policy structs below are the only
// place where the two differ; the kernels take one as a template argument.
//
//              term                a            b                d(y)               gradient scale
//   Jaccard    I / (S - I + eps)   1 / U        I / U^2          y a - (1 - y) b    1 / M          (U = S - I + eps)
//   Dice       2 I / (S + eps)     1 / (S+eps)  I / (S + eps)^2  y a - b            2 / M          (M = C or N)
//
// Every helper performs its operations in one fixed order and the library is compiled with -ffp-contract=off: the same bits
// wherever it is inlined (tests/test_loss_pin_gpu.py holds every entry point to the bits of the build before the merge).
#pragma once
#include "common.h"

#define LOSS_MAXC 16       // classes of the stand-alone forms and of the entropy maps
#define OV_MAXC 8          // classes of the fused forms
#define WS_HEAD 64         // doubles in front of every workspace: the reduced sums
#define WS_HEAD_COEF 32    // where in that head the fused Jaccard form keeps its coefficient pairs (2 * OV_MAXC floats)

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// grid of a grid-stride pointwise kernel: one 256-thread block per 256 elements, at most 4096 blocks
static inline int grid_for(long long n) { long long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }

// chunks per sample of a (sample, chunk) pass over `len` values each: one block per 256 values, about `blocks` blocks in all
static inline int sample_bps(int n, long long len, int blocks) {
  const long long want = (len + 255) / 256, cap = blocks / n > 1 ? blocks / n : 1;
  return (int)(want < cap ? want : cap);
}

// elements the main term of the fused forms is a mean over: BCE over every element, the cross entropy over pixels
static inline double seg_numel_main(int mode, int n, int c, long long hw) {
  const long long npix = (long long)n * hw;
  return mode == PCUDA_ACT_SIGMOID ? (double)npix * c : (double)npix;
}

// argument check of the fused forms (pcuda_seg_loss_*, pcuda_seg_loss_ov_*)
static inline int seg_check_args(const char* what, const void* logits, const void* onehot, const void* out, bool mode_ok, int n,
                                 int c, long long hw) {
  if (!logits || !onehot || !out || n <= 0 || c <= 0 || hw <= 0 || !mode_ok) PCUDA_FAIL(PCUDA_E_BADARG, "%s: bad arguments", what);
  if (c > OV_MAXC) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "%s: at most %d classes (got %d)", what, OV_MAXC, c);
  return PCUDA_OK;
}

// argument check of the forms on given probabilities (pcuda_jaccard_*, pcuda_dice_*); `in`: what the pass reads besides the
// truth (the forward's probabilities, the Jaccard backward's workspace; the Dice backward checks its workspace by size)
static inline int probs_check_args(const char* what, const void* in, const void* truth, const void* out, int n, int c,
                                   long long hw) {
  if (!in || !truth || !out || n <= 0 || c <= 0 || c > LOSS_MAXC || hw <= 0)
    PCUDA_FAIL(PCUDA_E_BADARG, "%s: bad arguments (1..%d classes)", what, LOSS_MAXC);
  return PCUDA_OK;
}

// ---------------------------------------------------------------------------- per pixel
// softmax over the c channels of one pixel (channels strided by hw): v[k] = expf(x_k - max), the return value their sum in
// channel order; the probability is v[k] / sum.  The division is the caller's, in the loop that uses the probability: a loop
// of its own over v costs the run-time-c kernels a second indexed pass over registers (measured: 2 us of the fused softmax
// forms' 57)
template <int N>
__device__ __forceinline__ float channel_softmax(const float* __restrict__ lp, long long hw, int c, float (&v)[N]) {
  float m = -INFINITY;
  for (int k = 0; k < c; ++k) { v[k] = lp[k * hw]; m = fmaxf(m, v[k]); }
  float ssum = 0.f;
  for (int k = 0; k < c; ++k) { v[k] = expf(v[k] - m); ssum += v[k]; }
  return ssum;
}

// ---------------------------------------------------------------------------- block reductions
// the block's sum of every accumulator -> one partial row, element k at row[k * stride] (waves in a fixed order)
template <int NACC>
__device__ __forceinline__ void block_store_row(const float (&acc)[NACC], float* __restrict__ row, int stride = 1) {
  __shared__ float sh[4][NACC];
  float s[NACC];      // (every wave sum before the first store: the shuffles of different accumulators overlap)
#pragma unroll
  for (int k = 0; k < NACC; ++k) s[k] = wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NACC; ++k) sh[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < NACC)
    row[threadIdx.x * stride] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
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

// ---------------------------------------------------------------------------- the overlap policy
struct JaccardOv {
  static constexpr float gscale = 1.f;
  __device__ static double den(double I, double S, double eps) { return S - I + eps; }
  __device__ static double term(double I, double d) { return I / d; }
  __device__ static float d(float y, float a, float b) { return y * a - b * (1.f - y); }
};
struct DiceOv {
  static constexpr float gscale = 2.f;
  __device__ static double den(double I, double S, double eps) { return S + eps; }
  __device__ static double term(double I, double d) { return 2.0 * I / d; }
  __device__ static float d(float y, float a, float b) { return y * a - b; }
};
// the coefficient pair of sums (I, S)
template <class OV>
__device__ __forceinline__ void overlap_coef(double I, double S, double eps, float& a, float& b) {
  const double d = OV::den(I, S, eps);
  a = (float)(1.0 / d);
  b = (float)(I / (d * d));
}

// ---------------------------------------------------------------------------- fused forms: main term + overlap term
// one pixel: the main term (BCE with the -100 clamp, or the double-softmax cross entropy) added to `main`, p * y and p + y
// added to the row's I and S accumulators ([main, I_0.., S_0..] per class, [main, I, S] per sample).  `main` may be acc[0]
// itself (every class's term goes straight into the running sum) or a zero of the caller's (the pixel's terms are summed
// first): two associations, and each form keeps the one it has always had.
template <int C, bool SAMPLE, int NACC>
__device__ __forceinline__ void seg_pixel(const float* __restrict__ lp, const uint8_t* __restrict__ yp, long long hw, int mode,
                                          float& main, float (&acc)[NACC]) {
  if (mode == PCUDA_ACT_SIGMOID) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const float pr = sigmoidf_(lp[k * hw]);
      const float y = (float)yp[k * hw];
      const float l1 = fmaxf(logf(pr), -100.f), l0 = fmaxf(logf(1.f - pr), -100.f);   // torch BCELoss clamps each log
      main += -(y * l1 + (1.f - y) * l0);
      acc[SAMPLE ? 1 : 1 + k] += pr * y;
      acc[SAMPLE ? 2 : 1 + C + k] += pr + y;
    }
  } else {
    float v[C];
    const float ssum = channel_softmax(lp, hw, C, v);
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
      acc[SAMPLE ? 1 : 1 + k] += pr * (float)yk;
      acc[SAMPLE ? 2 : 1 + C + k] += pr + (float)yk;
    }
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) s2 += expf(v[k] - pm);
    main += -(plabel - pm - logf(s2));   // -log_softmax(p)[label]
  }
}

// forward pass, one partial row per block.  The block partials are sums over the block's pixels, so the walk is part of the
// result and each form keeps its own: CHUNKS = false (Jaccard) walks grid-stride over all n * hw pixels; CHUNKS = true (Dice)
// gives block (sample, chunk) = (blockIdx.x / bps, blockIdx.x % bps) its chunk of ITS sample's pixels, which is what a
// per-sample row needs (rows of different samples are summed by the per-class reduce)
template <int C, bool CHUNKS, bool SAMPLE>
__global__ __launch_bounds__(256) void seg_partial_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ onehot,
                                                          int mode, long long hw, long long npix, int bps,
                                                          float* __restrict__ part) {
  constexpr int NACC = SAMPLE ? 3 : 2 * C + 1;
  float acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
  if (CHUNKS) {
    const long long n = blockIdx.x / (unsigned)bps;
    const int j = (int)(blockIdx.x - n * bps);
    for (long long px = j * 256ll + threadIdx.x; px < hw; px += 256ll * bps) {
      const long long base = n * C * hw + px;
      float main = 0.f;
      seg_pixel<C, SAMPLE>(logits + base, onehot + base, hw, mode, main, acc);
      acc[0] += main;
    }
  } else {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npix; i += 256ll * gridDim.x) {
      const long long n = i / hw, px = i - n * hw;
      const long long base = n * C * hw + px;
      seg_pixel<C, SAMPLE>(logits + base, onehot + base, hw, mode, acc[0], acc);
    }
  }
  block_store_row<NACC>(acc, part + (long long)blockIdx.x * NACC);
}

// per-class reduce of `nblocks` partial rows of nacc = 2 c + off floats: [main (off = 1)] [I_0..I_{c-1}] [S_0..S_{c-1}], a
// strided tree in double per accumulator (a single lane per accumulator walking thousands of partials took 110 us between the
// segmenter's forward and backward passes)
//   sums[a] = every accumulator; coef[2k], coef[2k+1] = a_k, b_k; out = [main / numel_main,] 1 - mean_c term_c
template <class OV>
__global__ __launch_bounds__(256) void overlap_class_final_kernel(const float* __restrict__ part, int nblocks, int c, int off,
                                                                  double numel_main, double eps, double* __restrict__ sums,
                                                                  float* __restrict__ coef, float* __restrict__ out) {
  __shared__ double sh[2 * LOSS_MAXC + 1];
  __shared__ double red[256];
  const int nacc = 2 * c + off;
  for (int a = 0; a < nacc; ++a) {
    double s = 0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += (double)part[(long long)b * nacc + a];
    const double tot = block_tree_sum(s, red);
    if (threadIdx.x == 0) { sums[a] = tot; sh[a] = tot; }
  }
  __syncthreads();
  if ((int)threadIdx.x < c)
    overlap_coef<OV>(sh[off + threadIdx.x], sh[off + c + threadIdx.x], eps, coef[2 * threadIdx.x], coef[2 * threadIdx.x + 1]);
  if (threadIdx.x == 0) {
    double t = 0;
    for (int k = 0; k < c; ++k) t += OV::term(sh[off + k], OV::den(sh[off + k], sh[off + c + k], eps));
    if (off) out[0] = (float)(sh[0] / numel_main);
    out[off] = (float)(1.0 - t / c);
  }
}

// dlogits = (g_main * d main / d p + g_ov * d overlap / d p) through the sigmoid / softmax Jacobian.  No reduction, so the
// walk does not touch the bits: block = (sample, chunk), no division per pixel.  coef: per class [c][2] (held in LDS) or per
// sample [n][2] (the block's own pair, read from the workspace: n is not bounded by LDS); m = c or n
template <class OV, bool SAMPLE>
__global__ __launch_bounds__(256) void seg_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ onehot,
                                                      int mode, int c, long long hw, int bps, double numel_main,
                                                      const float* __restrict__ coef, int m, const float* __restrict__ g_main,
                                                      const float* __restrict__ g_ov, float* __restrict__ dlogits) {
  __shared__ float ca[OV_MAXC], cb[OV_MAXC];
  const long long n = blockIdx.x / (unsigned)bps;
  const int j = (int)(blockIdx.x - n * bps);
  if (!SAMPLE) {
    if ((int)threadIdx.x < c) { ca[threadIdx.x] = coef[2 * threadIdx.x]; cb[threadIdx.x] = coef[2 * threadIdx.x + 1]; }
    __syncthreads();
  }
  const float sa = SAMPLE ? coef[2 * n] : 0.f, sb = SAMPLE ? coef[2 * n + 1] : 0.f;
  const float gm = (g_main ? *g_main : 1.f) / (float)numel_main;
  const float go = (g_ov ? *g_ov : 1.f) * OV::gscale / (float)m;
  for (long long px = j * 256ll + threadIdx.x; px < hw; px += 256ll * bps) {
    const long long base = n * c * hw + px;
    if (mode == PCUDA_ACT_SIGMOID) {
      for (int k = 0; k < c; ++k) {
        const float pr = sigmoidf_(logits[base + k * hw]);
        const float y = (float)onehot[base + k * hw];
        const float pq = pr * (1.f - pr);
        // torch: BCE backward divides by max(p(1-p), 1e-12), sigmoid backward multiplies by p(1-p)
        const float gb = gm * (pr - y) / fmaxf(pq, 1e-12f);
        const float gov = -go * OV::d(y, SAMPLE ? sa : ca[k], SAMPLE ? sb : cb[k]);
        dlogits[base + k * hw] = (gb + gov) * pq;
      }
    } else {
      float v[OV_MAXC], gp[OV_MAXC];
      const float ssum = channel_softmax(logits + base, hw, c, v);
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
        const float g = gm * (sm2 - (k == label ? 1.f : 0.f)) - go * OV::d(y, SAMPLE ? sa : ca[k], SAMPLE ? sb : cb[k]);
        gp[k] = g;
        dot += g * v[k];
      }
      for (int k = 0; k < c; ++k) dlogits[base + k * hw] = v[k] * (gp[k] - dot);
    }
  }
}

// ---------------------------------------------------------------------------- on given probabilities
// per class: class on the grid's y axis; partial row [I_0..I_{c-1}, S_0..S_{c-1}] per x block
static __global__ __launch_bounds__(256) void overlap_class_partial_kernel(const float* __restrict__ p,
                                                                           const float* __restrict__ tf,
                                                                           const uint8_t* __restrict__ tu, int c, long long hw,
                                                                           long long npix, float* __restrict__ part) {
  const int k = blockIdx.y;
  float acc[2] = {0.f, 0.f};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npix; i += 256ll * gridDim.x) {
    const long long n = i / hw, px = i - n * hw;
    const long long o = (n * c + k) * hw + px;
    const float pr = p[o], y = tf ? tf[o] : (float)tu[o];
    acc[0] += pr * y;
    acc[1] += pr + y;
  }
  block_store_row<2>(acc, part + (long long)blockIdx.x * 2 * c + k, c);
}

// dp = -(gout * gscale / m) d(y); the element's coefficient pair is q = (o / seg) % mod: (hw, c) per class, (c hw, n) per
// sample.  The pairs are read from the workspace (coef), or derived here from the reduced sums [I_0.., S_0..] with the eps
// of this call (SUMS: per class only, mod <= LOSS_MAXC)
template <class OV, bool SUMS>
__global__ __launch_bounds__(256) void overlap_bwd_kernel(const float* __restrict__ tf, const uint8_t* __restrict__ tu,
                                                          long long numel, long long seg, int mod, int m,
                                                          const float* __restrict__ coef, const double* __restrict__ sums,
                                                          double eps, const float* __restrict__ gout, float* __restrict__ dp) {
  __shared__ float ca[LOSS_MAXC], cb[LOSS_MAXC];
  if (SUMS) {
    if ((int)threadIdx.x < mod) overlap_coef<OV>(sums[threadIdx.x], sums[mod + threadIdx.x], eps, ca[threadIdx.x], cb[threadIdx.x]);
    __syncthreads();
  }
  const float g = (gout ? *gout : 1.f) * OV::gscale / (float)m;
  for (long long o = blockIdx.x * 256ll + threadIdx.x; o < numel; o += 256ll * gridDim.x) {
    const long long q = (o / seg) % mod;
    const float y = tf ? tf[o] : (float)tu[o];
    dp[o] = -g * OV::d(y, SUMS ? ca[q] : coef[2 * q], SUMS ? cb[q] : coef[2 * q + 1]);
  }
}
