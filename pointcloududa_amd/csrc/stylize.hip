// Device-side "stylize" augmentation of the loader path: the three entries of the reference's
// SomeOf lists (data_generator_mscmrseg.py:46, 57-60, 69 and :98, 108-111, 120) that f7 and f8 left on the CPU --
// AddToHueAndSaturation, SimplexNoiseAlpha(EdgeDetect | DirectedEdgeDetect) and Superpixels -- on uint8 [B,H,W,C] images, as a
// per-sample PROGRAM of up to eight slots that lives in device memory (the shape of pcuda_photometric).
//
// Convention (this build's own: imgaug / cv2 / skimage are not vendored by the reference, parity is unpinned; pinned by
// tests/golden/stylize.npz against two restatements):
//   * the value is uint8 again between two slots
//   * rdiv(a, b) = floor((2 a + b) / (2 b)), a true floor for negative a
//   * HUE_SATURATION (C = 3, channel 0 = red; integers only): V = max, m = min, d = V - m, S = rdiv(255 d, V) (0 when V = 0),
//     H = 0 when d = 0, else (base + rdiv(30 num, d)) mod 180 with (base, num) = (0, g - b) if V == r, (60, b - r) if V == g,
//     (120, r - g) otherwise; H' = (H + dh) mod 180 >= 0, S' = clip(S + ds, 0, 255); sec = H' / 30, F = H' % 30,
//     p = rdiv(V (255 - S'), 255), q = rdiv(V (7650 - S' F), 7650), t = rdiv(V (7650 - S' (30 - F)), 7650),
//     (r, g, b) by sector = (V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q)
//   * NOISE_ALPHA_CONV3X3 (float64 in the written order; the library is built with -ffp-contract=off): n = 1..3 coarse grids
//     h' x w' (2..16 each) of values in [0, 1] come from the host (table); each is upscaled to H x W -- nearest: cell
//     ((y h') / H, (x w') / W); bilinear: sy = (y + 0.5) h' / H - 0.5 clamped to [0, h' - 1], y0 = floor(sy), y1 = min(y0 + 1,
//     h' - 1), fy = sy - y0, top = g00 (1 - fx) + g01 fx, bot likewise, top (1 - fy) + bot fy; cubic (iarg[1] = 3, f8b): the
//     same sy, sx UNCLAMPED, Keys weights (A = -0.75, imgdev::cubic_weights) of sy - floor(sy) over the taps floor(sy) - 1 ..
//     floor(sy) + 2, each tap index clamped to [0, h' - 1], rows summed left to right, then the rows, the value clipped to
//     [0, 1] --, aggregated (min | mean in
//     iteration order | max), optionally m = 1 / (1 + exp(-(20 (m - 0.5) - t))); e = to_u8(3x3 correlation, f7's CONV3X3:
//     t = 0, nine taps row-major, reflect-101); out = to_u8((1 - m) x + m e), to_u8 = floor(v + 0.5) clipped
//   * SUPERPIXELS (integers only): a gy x gx grid SLIC.  Centre k = j gx + i starts at (((2j+1) H) / (2 gy), ((2i+1) W) / (2 gx))
//     with that pixel's colour.  A pixel looks at the centres of the 3x3 grid cells around its own cell ((y gy) / H, (x gx) / W)
//     (cells outside the grid are skipped) and takes the smallest 64-bit D = dc2 S2 + M2 ds2 (dc2 = sum over channels of
//     (v - centre)^2, ds2 = squared pixel distance, S2 = max(1, (H W) / (gy gx))), a tie goes to the lowest k.  Update: centre =
//     rdiv(sum, n) for colour, y and x; a centre with n = 0 stays.  After `iters` updates and one last assignment segment k
//     takes its mean colour rdiv(sum_ch, n) iff the first word of Philox4x32-10(key = seed, counter = (k, 0, 0, 0)) is below
//     the threshold, else its pixels are copied.  No connectivity pass (spx_connect.hip adds one behind this kernel for slots
//     that ask for it, through pcuda_stylize_connect; pcuda_stylize never reads iarg[5]).  imgaug's downscale to 128 pixels
//     is built in spx_scale.hip (f9c, opt-in: iarg[6] = max_size, read by pcuda_stylize_scaled alone, which launches this
//     kernel a second time for the scaled samples with their working size h' x w' in place of H x W; StyleArgs.scale).
//
// One slot = three launches, and each workgroup reads its sample's opcode with scalar loads and leaves at once when the
// slot belongs to another kernel (the branch on the opcode is wave-uniform):
//   * pointwise (NOP, unknown opcodes, HUE_SATURATION): 16 bytes per lane for the copy, four pixels (three dwords) per lane
//     for the hue
//   * noise-alpha: one pixel per lane; the grids and the weights are staged in LDS once per workgroup, the 3x3 window is
//     gathered through the cache
//   * superpixels: ONE workgroup of 1024 lanes per sample; centres and 64-bit integer sums live in LDS, __syncthreads between
//     assignment and update; lanes hold consecutive pixels, a wave first adds up each run of equal labels with shuffles and only
//     the run's first lane issues the LDS atomics (integer adds: any order gives the same bits); the uint8 label plane of
//     the last assignment lives in the workspace
// The slots ping-pong between the caller's output and the workspace.  Every gather index is mirrored or clamped into the image
// (or the table) BEFORE the load, an unknown opcode copies, and every in-flight load's address stays alive (PCUDA_KEEP, VMEM
// address rule, common.h).
#include "common.h"
#include "image_device.h"
#include "stylize_host.h"

namespace {

enum { OP_NOP = 0, OP_HUE_SATURATION = 1, OP_NOISE_ALPHA = 2, OP_SUPERPIXELS = 3 };
enum { UPSCALE_NEAREST = 0, UPSCALE_BILINEAR = 1, UPSCALE_CUBIC = 3 };      // (2 is not an upscale: the host rejects it)

constexpr int kMaxSlots = 8, kIArgs = 12, kFArgs = 16;
constexpr int kGrid = 256;                 // values of one coarse grid (16 x 16)
constexpr int kTable = 3 * kGrid;          // doubles per slot
constexpr int kMaxC = 4;
constexpr int kMaxSeg = 256;
constexpr int kSpxThreads = 1024;

struct StyleArgs {
  const uint8_t* in;         // [b][h][w][c]
  uint8_t* out;              // [b][h][w][c]
  const int* opcode;         // [b][slots]
  const int* iarg;           // [b][slots][12]
  const double* farg;        // [b][slots][16]
  const double* table;       // [b][slots][768]
  const uint32_t* seed;      // [b][slots][2] (low, high word)
  uint8_t* labels;           // [b][h][w] (workspace)
  int h, w, c, slots;
  int slot;                  // the slot this launch runs; < 0: copy
  int vec_in, vec_out;       // 16-byte loads / stores are aligned
  int word_in, word_out;     // 4-byte loads / stores of a group of four pixels are aligned (C = 3)
  // f9c, set by pcuda_stylize_scaled alone (0 from pcuda_stylize and pcuda_stylize_connect, which never read iarg[6]):
  // 1 = the superpixel kernel stands aside for the samples whose slot is scaled, 2 = it runs those samples alone, on
  // their working size (rows of w' pixels; a sample's planes stay h w apart) and leaves `flag`
  int scale;
  int* flag;                 // [b] (scale == 2): 1 iff a segment that holds a pixel is replaced
};

using imgdev::clampi;
using imgdev::reflect101;
using imgdev::round_u8;
using imgdev::philox_word0;
// floor((2 a + b) / (2 b)), b > 0
__device__ __forceinline__ int rdiv(int a, int b) {
  const int num = 2 * a + b, den = 2 * b;
  const int q = num / den;
  return (num % den != 0 && num < 0) ? q - 1 : q;
}
__device__ __forceinline__ long long rdiv64(long long a, long long b) { return (2 * a + b) / (2 * b); }      // a >= 0, b > 0

// one pixel through HUE_SATURATION; dh in 0..179, ds in -255..255
__device__ __forceinline__ void hue_pixel(int& r, int& g, int& b, int dh, int ds) {
  const int V = max(r, max(g, b)), m = min(r, min(g, b)), d = V - m;
  const int S = V == 0 ? 0 : rdiv(255 * d, V);
  int H = 0;
  if (d != 0) {
    int base, num;
    if (V == r) { base = 0; num = g - b; }
    else if (V == g) { base = 60; num = b - r; }
    else { base = 120; num = r - g; }
    H = (base + rdiv(30 * num, d)) % 180;
    if (H < 0) H += 180;
  }
  const int H2 = (H + dh) % 180, S2 = clampi(S + ds, 0, 255);
  const int sec = H2 / 30, F = H2 - 30 * sec;
  const int p = rdiv(V * (255 - S2), 255), q = rdiv(V * (7650 - S2 * F), 7650), t = rdiv(V * (7650 - S2 * (30 - F)), 7650);
  switch (sec) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// ------------------------------------------------------------------------------------------
// NOP / unknown opcodes (copy: 16 consecutive bytes per lane) and HUE_SATURATION (four pixels per lane)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stylize_pointwise_kernel(const StyleArgs a) {
  const int n = blockIdx.y;
  const int at = n * a.slots + (a.slot < 0 ? 0 : a.slot);
  const int op = a.slot < 0 ? (int)OP_NOP : a.opcode[at];
  if (op == OP_NOISE_ALPHA || op == OP_SUPERPIXELS) return;
  const int c = a.c, hw = a.h * a.w;
  const int numel = hw * c;
  const uint8_t* src = a.in + (long long)n * numel;
  uint8_t* dst = a.out + (long long)n * numel;
  const int t = blockIdx.x * 256 + threadIdx.x;

  if (op == OP_HUE_SATURATION && c == 3) {
    const int p0 = 4 * t;                                  // first pixel of the group
    if (p0 >= hw) return;
    const int* ia = a.iarg + at * kIArgs;
    int dh = ia[0] % 180;
    if (dh < 0) dh += 180;
    const int ds = clampi(ia[1], -255, 255);
    const bool full = p0 + 4 <= hw;
    uint8_t v[12];
    if (a.word_in && full) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(src + 3 * p0);
      const uint32_t wd[3] = {p[0], p[1], p[2]};
#pragma unroll
      for (int i = 0; i < 12; ++i) v[i] = (uint8_t)(wd[i >> 2] >> (8 * (i & 3)));
      PCUDA_KEEP(p);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        const uint8_t* p = src + (3 * p0 + i < numel ? 3 * p0 + i : numel - 1);
        v[i] = *p;
        PCUDA_KEEP(p);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int r = v[3 * k], g = v[3 * k + 1], b = v[3 * k + 2];
      hue_pixel(r, g, b, dh, ds);
      v[3 * k] = (uint8_t)r; v[3 * k + 1] = (uint8_t)g; v[3 * k + 2] = (uint8_t)b;
    }
    PCUDA_KEEP(ia);
    if (a.word_out && full) {
      uint32_t wd[3] = {0, 0, 0};
#pragma unroll
      for (int i = 0; i < 12; ++i) wd[i >> 2] |= (uint32_t)v[i] << (8 * (i & 3));
      uint32_t* q = reinterpret_cast<uint32_t*>(dst + 3 * p0);
      q[0] = wd[0]; q[1] = wd[1]; q[2] = wd[2];
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (3 * p0 + i < numel) dst[3 * p0 + i] = v[i];
    }
    return;
  }

  const int i0 = t * 16;
  if (i0 >= numel) return;
  const bool full = i0 + 16 <= numel;
  if (a.vec_in && a.vec_out && full) {
    const uint4* p = reinterpret_cast<const uint4*>(src + i0);
    const uint4 q = *p;
    *reinterpret_cast<uint4*>(dst + i0) = q;
    PCUDA_KEEP(p);
  } else {
    uint8_t v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint8_t* p = src + (i0 + i < numel ? i0 + i : numel - 1);
      v[i] = *p;
      PCUDA_KEEP(p);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i0 + i < numel) dst[i0 + i] = v[i];
  }
}

// ------------------------------------------------------------------------------------------
// NOISE_ALPHA_CONV3X3: one pixel per lane
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double upscaled(const double* g, int h2, int w2, int y, int x, int h, int w, int up) {
  if (up != UPSCALE_BILINEAR && up != UPSCALE_CUBIC) return g[(int)(((long long)y * h2) / h) * w2 + (int)(((long long)x * w2) / w)];
  double sy = ((double)y + 0.5) * (double)h2 / (double)h - 0.5;
  double sx = ((double)x + 0.5) * (double)w2 / (double)w - 0.5;
  if (up == UPSCALE_CUBIC) {      // the coordinate stays unclamped, each of the eight tap indices is clamped into the grid
    const double yf = floor(sy), xf = floor(sx);
    double wy[4], wx[4];
    imgdev::cubic_weights(sy - yf, wy);
    imgdev::cubic_weights(sx - xf, wx);
    const int ya = (int)yf - 1, xa = (int)xf - 1;
    int xi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xi[q] = clampi(xa + q, 0, w2 - 1);
    double rows[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double* r = g + clampi(ya + k, 0, h2 - 1) * w2;
      rows[k] = ((r[xi[0]] * wx[0] + r[xi[1]] * wx[1]) + r[xi[2]] * wx[2]) + r[xi[3]] * wx[3];
    }
    const double v = ((rows[0] * wy[0] + rows[1] * wy[1]) + rows[2] * wy[2]) + rows[3] * wy[3];
    return fmin(fmax(v, 0.0), 1.0);      // an alpha: the cubic overshoots
  }
  sy = fmin(fmax(sy, 0.0), (double)(h2 - 1));
  sx = fmin(fmax(sx, 0.0), (double)(w2 - 1));
  const int y0 = clampi((int)floor(sy), 0, h2 - 1), x0 = clampi((int)floor(sx), 0, w2 - 1);
  const int y1 = min(y0 + 1, h2 - 1), x1 = min(x0 + 1, w2 - 1);
  const double fy = sy - (double)y0, fx = sx - (double)x0;
  const double top = g[y0 * w2 + x0] * (1.0 - fx) + g[y0 * w2 + x1] * fx;
  const double bot = g[y1 * w2 + x0] * (1.0 - fx) + g[y1 * w2 + x1] * fx;
  return top * (1.0 - fy) + bot * fy;
}

__global__ __launch_bounds__(256) void stylize_noise_alpha_kernel(const StyleArgs a) {
  __shared__ double s_tab[kTable];      // 6144 B
  __shared__ double s_w[kFArgs];
  const int n = blockIdx.y;
  const int at = n * a.slots + a.slot;
  if (a.opcode[at] != OP_NOISE_ALPHA) return;
  const int tid = threadIdx.x;
  const int c = a.c, w = a.w, h = a.h;
  const int* ia = a.iarg + at * kIArgs;
  const int niter = clampi(ia[0], 1, 3);
  const int up = ia[1];
  const int aggregation = ia[2];
  const bool sigmoid = ia[3] != 0;
  int h2[3], w2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { h2[k] = clampi(ia[4 + 2 * k], 1, 16); w2[k] = clampi(ia[5 + 2 * k], 1, 16); }
  for (int i = tid; i < kTable; i += 256) {
    const double* p = a.table + (long long)at * kTable + i;
    s_tab[i] = *p;
    PCUDA_KEEP(p);
  }
  if (tid < kFArgs) {
    const double* p = a.farg + at * kFArgs + tid;
    s_w[tid] = *p;
    PCUDA_KEEP(p);
  }
  PCUDA_KEEP(ia);
  __syncthreads();
  const int pix = blockIdx.x * 256 + tid;
  if (pix >= h * w) return;
  const int y = pix / w, x = pix - y * w;

  double m = upscaled(s_tab, h2[0], w2[0], y, x, h, w, up);
  for (int k = 1; k < niter; ++k) {
    const double v = upscaled(s_tab + k * kGrid, h2[k], w2[k], y, x, h, w, up);
    if (aggregation == 0) m = fmin(m, v);
    else if (aggregation == 2) m = fmax(m, v);
    else m = m + v;
  }
  if (aggregation != 0 && aggregation != 2) m = m / (double)niter;
  if (sigmoid) m = 1.0 / (1.0 + exp(-(20.0 * (m - 0.5) - s_w[9])));

  const uint8_t* src = a.in + (long long)n * h * w * c;
  uint8_t* dst = a.out + (long long)n * h * w * c;
  const int ys[3] = {reflect101(y - 1, h), y, reflect101(y + 1, h)};
  const int xs[3] = {reflect101(x - 1, w), x, reflect101(x + 1, w)};
  for (int ch = 0; ch < c; ++ch) {
    const uint8_t* p[9];
    double v[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      p[i] = src + ((long long)ys[i / 3] * w + xs[i % 3]) * c + ch;
      v[i] = (double)*p[i];
    }
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) t += v[i] * s_w[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) PCUDA_KEEP(p[i]);
    const double e = (double)round_u8(t);
    dst[(long long)pix * c + ch] = round_u8((1.0 - m) * v[4] + m * e);
  }
}

// ------------------------------------------------------------------------------------------
// SUPERPIXELS: one workgroup per sample
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpxThreads) void stylize_superpixels_kernel(const StyleArgs a) {
  __shared__ int s_cy[kMaxSeg], s_cx[kMaxSeg], s_cc[kMaxSeg * kMaxC];
  __shared__ unsigned long long s_sum[kMaxSeg * 7];      // per centre: colour[4], y, x, n
  __shared__ int s_rep[kMaxSeg];
  const int n = blockIdx.x;
  const int at = n * a.slots + a.slot;
  if (a.opcode[at] != OP_SUPERPIXELS) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int* ia = a.iarg + at * kIArgs;
  int h = a.h, w = a.w;
  if (a.scale != 0) {      // (a kernel argument and scalar loads: workgroup-uniform)
    const bool scaled = imgdev::spx_working_size(a.h, a.w, ia[6], h, w);
    if (scaled != (a.scale == 2)) return;
  }
  const int c = a.c, hw = h * w;
  const long long plane = (long long)a.h * a.w;      // (a sample's stride, whatever size it works on)
  const int gy = clampi(ia[0], 1, min(h, kMaxSeg));
  const int gx = clampi(ia[1], 1, min(w, kMaxSeg / gy));
  const int iters = clampi(ia[2], 0, 10);
  const long long M2 = clampi(ia[3], 0, 1 << 20);
  const uint32_t thr = (uint32_t)ia[4];
  PCUDA_KEEP(ia);
  const int K = gy * gx;
  const long long S2 = max(1, hw / K);
  const uint8_t* src = a.in + n * plane * c;
  uint8_t* dst = a.out + n * plane * c;
  uint8_t* lab_plane = a.labels + n * plane;

  if (tid < K) {
    const int j = tid / gx, i = tid - j * gx;
    const int cy = (int)(((long long)(2 * j + 1) * h) / (2 * gy)), cx = (int)(((long long)(2 * i + 1) * w) / (2 * gx));
    s_cy[tid] = cy; s_cx[tid] = cx;
    const uint8_t* p = src + ((long long)cy * w + cx) * c;
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch) s_cc[tid * kMaxC + ch] = ch < c ? (int)p[ch] : 0;
    PCUDA_KEEP(p);
  }

  for (int pass = 0; pass <= iters; ++pass) {
    if (tid < K) {
#pragma unroll
      for (int q = 0; q < 7; ++q) s_sum[tid * 7 + q] = 0;
    }
    __syncthreads();
    const bool last = pass == iters;
    for (int base = 0; base < hw; base += kSpxThreads) {      // (the trip count is the same for every lane: shuffles below)
      const int pi = base + tid;
      const bool active = pi < hw;
      const int px = active ? pi : hw - 1;
      const int y = px / w, x = px - y * w;
      const uint8_t* p = src + (long long)px * c;
      int v[kMaxC];
#pragma unroll
      for (int ch = 0; ch < kMaxC; ++ch) v[ch] = ch < c ? (int)p[ch] : 0;
      PCUDA_KEEP(p);
      const int cj = (int)(((long long)y * gy) / h), ci = (int)(((long long)x * gx) / w);
      long long best = 0x7fffffffffffffffll;
      int lab = 0;
      for (int dj = -1; dj <= 1; ++dj) {
        const int jj = cj + dj;
        if (jj < 0 || jj >= gy) continue;
        for (int di = -1; di <= 1; ++di) {
          const int ii = ci + di;
          if (ii < 0 || ii >= gx) continue;
          const int k = jj * gx + ii;
          long long dc2 = 0;
#pragma unroll
          for (int ch = 0; ch < kMaxC; ++ch) { const int d = v[ch] - s_cc[k * kMaxC + ch]; dc2 += d * d; }
          const long long ddy = y - s_cy[k], ddx = x - s_cx[k];
          const long long D = dc2 * S2 + M2 * (ddy * ddy + ddx * ddx);
          if (D < best) { best = D; lab = k; }      // (k ascends: a tie keeps the lowest)
        }
      }
      if (!active) lab = -1;
      if (last && active) lab_plane[pi] = (uint8_t)lab;
      // runs of equal labels inside the wave are added up with shuffles; the first lane of a run issues the atomics
      const int prev = __shfl_up(lab, 1);
      const bool head_flag = lane == 0 || prev != lab;
      const unsigned long long heads = __ballot(head_flag);
      const int head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
      int s01 = active ? (v[0] | (v[1] << 16)) : 0, s23 = active ? (v[2] | (v[3] << 16)) : 0;
      int sy = active ? y : 0, sx = active ? x : 0, sn = active ? 1 : 0;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int oh = __shfl_down(head, off);
        const int o01 = __shfl_down(s01, off), o23 = __shfl_down(s23, off);
        const int oy = __shfl_down(sy, off), ox = __shfl_down(sx, off), on = __shfl_down(sn, off);
        if (lane + off < 64 && oh == head) { s01 += o01; s23 += o23; sy += oy; sx += ox; sn += on; }
      }
      if (head_flag && lab >= 0) {
        unsigned long long* q = s_sum + lab * 7;
        atomicAdd(q + 0, (unsigned long long)(s01 & 0xffff));
        atomicAdd(q + 1, (unsigned long long)((unsigned)s01 >> 16));
        atomicAdd(q + 2, (unsigned long long)(s23 & 0xffff));
        atomicAdd(q + 3, (unsigned long long)((unsigned)s23 >> 16));
        atomicAdd(q + 4, (unsigned long long)sy);
        atomicAdd(q + 5, (unsigned long long)sx);
        atomicAdd(q + 6, (unsigned long long)sn);
      }
    }
    __syncthreads();
    if (tid < K) {
      const long long cnt = (long long)s_sum[tid * 7 + 6];
      if (cnt > 0) {
#pragma unroll
        for (int ch = 0; ch < kMaxC; ++ch) s_cc[tid * kMaxC + ch] = (int)rdiv64((long long)s_sum[tid * 7 + ch], cnt);
        if (!last) {
          s_cy[tid] = (int)rdiv64((long long)s_sum[tid * 7 + 4], cnt);
          s_cx[tid] = (int)rdiv64((long long)s_sum[tid * 7 + 5], cnt);
        }
      }
      if (last) {
        const uint32_t* sd = a.seed + 2 * at;
        asm volatile("" : "+v"(sd));      // a vector address of its own, kept alive below (as photometric.hip)
        const uint32_t k0 = sd[0], k1 = sd[1];
        s_rep[tid] = philox_word0(k0, k1, (uint32_t)tid) < thr ? 1 : 0;
        PCUDA_KEEP(sd);
        if (a.scale == 2 && s_rep[tid] != 0 && cnt > 0) a.flag[n] = 1;      // (zeroed by the downscale; every writer stores 1)
      }
    }
    __syncthreads();      // (the next pass zeroes a centre's sums in the lane that read them)
  }

  // after the last pass s_cc holds the mean colour of every segment that has a pixel
  for (int pi = tid; pi < hw; pi += kSpxThreads) {
    const uint8_t* lp = lab_plane + pi;
    const int lab = *lp;
    const uint8_t* p = src + (long long)pi * c;
    uint8_t v[kMaxC];
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch) v[ch] = ch < c ? p[ch] : (uint8_t)0;
    PCUDA_KEEP(lp); PCUDA_KEEP(p);
    const bool rep = s_rep[lab] != 0;
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch)
      if (ch < c) dst[(long long)pi * c + ch] = rep ? (uint8_t)s_cc[lab * kMaxC + ch] : v[ch];
  }
}


}  // namespace

extern "C" size_t pcuda_stylize_workspace_size(int b, int h, int w, int c) {
  if (b <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  return round16((size_t)b * h * w) + round16((size_t)b * h * w * c);      // the label plane, then the ping-pong image
}

int stylize_run(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode, const int* iarg,
                const double* farg, const double* table, const unsigned long long* seed, void* workspace, size_t workspace_bytes,
                size_t workspace_need, pcuda_stream_t s, StyleSlotHook hook, void* ctx, int scale) {
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "stylize: null pointer");
  if (in == out) PCUDA_FAIL(PCUDA_E_BADARG, "stylize: in == out (the input is never written)");
  if (b <= 0 || b > 65535 || h <= 0 || w <= 0 || h > 32768 || w > 32768 || c <= 0 || c > kMaxC ||
      (long long)h * w * c >= (1ll << 31) - 8192)
    PCUDA_FAIL(PCUDA_E_BADARG, "stylize: bad dims (1..4 channels, sides up to 32768)");
  if (slots < 0 || slots > kMaxSlots) PCUDA_FAIL(PCUDA_E_BADARG, "stylize: slots outside 0..8");
  if (slots > 0 && (!opcode || !iarg || !farg || !table || !seed)) PCUDA_FAIL(PCUDA_E_BADARG, "stylize: null pointer (program)");
  const size_t bytes = (size_t)b * h * w * c;
  if (slots > 0 && (!workspace || workspace_bytes < workspace_need || workspace_bytes < pcuda_stylize_workspace_size(b, h, w, c)))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "stylize: workspace too small");
  StyleArgs a;
  memset(&a, 0, sizeof(a));
  a.opcode = opcode; a.iarg = iarg; a.farg = farg; a.table = table; a.seed = reinterpret_cast<const uint32_t*>(seed);
  a.h = h; a.w = w; a.c = c; a.slots = slots;
  a.labels = (uint8_t*)workspace;
  a.scale = scale;
  uint8_t* spare = slots > 0 ? (uint8_t*)workspace + round16((size_t)b * h * w) : nullptr;
  const long long per_sample = (long long)h * w * c, hw = (long long)h * w;
  const long long lanes = c == 3 ? (cdiv(per_sample, 16) > cdiv(hw, 4) ? cdiv(per_sample, 16) : cdiv(hw, 4)) : cdiv(per_sample, 16);
  const dim3 grid_p(cdiv(lanes, 256), b), grid_n(cdiv(hw, 256), b), grid_s(b);
  const int launches = slots > 0 ? slots : 1;
  ProfScope prof(PCUDA_FAM_POINTWISE, 2.0 * (double)bytes * launches, (hipStream_t)s);
  const uint8_t* cur = in;
  for (int i = 0; i < launches; ++i) {
    // the slots alternate between the output and the workspace so that the last one lands in the output
    uint8_t* dst = ((launches - 1 - i) & 1) ? spare : out;
    a.in = cur; a.out = dst; a.slot = slots > 0 ? i : -1;
    a.vec_in = ((uintptr_t)cur & 15) == 0 && (per_sample & 15) == 0;
    a.vec_out = ((uintptr_t)dst & 15) == 0 && (per_sample & 15) == 0;
    a.word_in = ((uintptr_t)cur & 3) == 0 && (per_sample & 3) == 0;
    a.word_out = ((uintptr_t)dst & 3) == 0 && (per_sample & 3) == 0;
    hipLaunchKernelGGL(stylize_pointwise_kernel, grid_p, dim3(256), 0, (hipStream_t)s, a);
    PCUDA_CHECK_LAUNCH("stylize_pointwise_kernel");
    if (slots > 0) {
      hipLaunchKernelGGL(stylize_noise_alpha_kernel, grid_n, dim3(256), 0, (hipStream_t)s, a);
      PCUDA_CHECK_LAUNCH("stylize_noise_alpha_kernel");
      hipLaunchKernelGGL(stylize_superpixels_kernel, grid_s, dim3(kSpxThreads), 0, (hipStream_t)s, a);
      PCUDA_CHECK_LAUNCH("stylize_superpixels_kernel");
      if (hook) {
        const int rc = hook(ctx, i, cur, dst, a.labels);
        if (rc != PCUDA_OK) return rc;
      }
    }
    cur = dst;
  }
  return PCUDA_OK;
}

extern "C" int pcuda_stylize(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode,
                             const int* iarg, const double* farg, const double* table, const unsigned long long* seed,
                             void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  return stylize_run(in, out, b, h, w, c, slots, opcode, iarg, farg, table, seed, workspace, workspace_bytes, 0, s, nullptr,
                     nullptr, 0);
}

int stylize_superpixels_scaled(const uint8_t* small, uint8_t* painted, uint8_t* labels, int* flag, int b, int h, int w, int c,
                               int slots, int slot, const int* opcode, const int* iarg, const unsigned long long* seed,
                               pcuda_stream_t s) {
  StyleArgs a;
  memset(&a, 0, sizeof(a));
  a.in = small; a.out = painted; a.labels = labels; a.flag = flag;
  a.opcode = opcode; a.iarg = iarg; a.seed = reinterpret_cast<const uint32_t*>(seed);
  a.h = h; a.w = w; a.c = c; a.slots = slots; a.slot = slot;
  a.scale = 2;
  hipLaunchKernelGGL(stylize_superpixels_kernel, dim3(b), dim3(kSpxThreads), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("stylize_superpixels_kernel");
  return PCUDA_OK;
}
