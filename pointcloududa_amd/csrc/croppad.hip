// Device-side CropAndPad with every defined mode of numpy.pad: the reference's
// iaa.CropAndPad(percent=(-0.05, 0.1), pad_mode=ia.ALL, pad_cval=(0, 255)) (data_generator_mscmrseg.py:28-32, 91-95) on uint8
// [B,H,W,C] images and int32 [B,H,W] labels, as a per-sample program in device memory: opcode[b] (0 copy, 1 crop-and-pad) and
// iarg[b][6] = (top, right, bottom, left, mode, cval); the sides are signed pixels, positive pads, negative crops.
//
// For a live sample: xc = x[ct : H - cb, cl : W - cr] (the negative sides), I = numpy.pad(xc, ((pt, pb), (pl, pr), (0, 0)), mode)
// (Hi x Wi; constant_values = cval for constant, end_values = cval for linear_ramp, the statistics over the whole axis), and the
// output is I resized back to H x W by this build's order-1 rule (float64, no contraction):
//   ax = Wi / W, sx = (x + 0.5) ax - 0.5, x0 = floor(sx), wx1 = sx - x0, the neighbour indices x0, x0 + 1 clamped into I (y
//   likewise); v = 0; v += p00 wy0 wx0; v += p01 wy0 wx1; v += p10 wy1 wx0; v += p11 wy1 wx1; floor(v + 0.5) clipped to 0..255
// Labels: the same crop, constant 0, the texel at floor(s + 0.5).  I is never materialised: a texel of I is
//   * inside the crop: the image texel
//   * constant: cval; edge / reflect / symmetric / wrap: the image texel at the folded index (per axis)
//   * maximum / mean / median / minimum: numpy pads axis 0 first and axis 1 on the padded array.  A top or bottom pad row holds
//     the column statistics over the cropped rows; a left or right pad value of row y of I (a pad row included) is the statistic
//     of that row of the axis-0-padded array, so a corner is a statistic of statistics.  mean and median are rounded half to
//     even (integer sum, one division, rint; median of an even count = the mean of the two middle values).  The statistics
//     pass writes them to the workspace: per sample and channel Wc column values and Hi row values
//   * linear_ramp: per side floor(end + k step), k = 0 outermost, step = (edge - end) / width -- unless some edge value of
//     that side (all columns and channels; for axis 1 all Hi rows, ramped pad rows included) equals end: numpy's linspace then
//     computes the whole side as floor(end + (k / width) (edge - end)).  Four flags per sample (statistics pass) select the
//     form; a corner is a ramp along x whose edge value is a ramp along y
//
// Three launches for the batch: the line statistics (one wave per cropped column or row and channel: max / min / integer sum by
// wave reduction, the median from a 256-bin LDS histogram per wave and a scan), the pad-row statistics and ramp flags (one
// workgroup per sample), the sampling pass (a tile is 16 rows x 64 pixels, a lane owns four consecutive pixels and stores their
// bytes as 32-bit words, labels as 16 bytes).  Samples that do not need a pass leave it at once.  The program is read by
// scalar loads, so every branch on it is wave-uniform.  Sides and modes are clamped on the device BEFORE any load (a garbage
// program reads wrong texels, never out of bounds; the host validates), and every in-flight load's address stays alive behind
// the code that consumes the data (PCUDA_KEEP, VMEM address rule, common.h).
#include "common.h"
#include "image_device.h"

namespace {

constexpr int kIArgs = 6, kMaxC = 4, kMaxPad = 64;
constexpr int kTileW = 64, kTileH = 16;
enum { F_TOP = 1, F_RIGHT = 2, F_BOTTOM = 4, F_LEFT = 8 };

struct CpArgs {
  const uint8_t* in;         // [b][h][w][c]
  uint8_t* out;              // [b][h][w][c]
  const int* lab_in;         // [b][h][w] (may be null together with lab_out)
  int* lab_out;
  const int* opcode;         // [b]
  const int* iarg;           // [b][6]
  uint8_t* tab;              // [b][c][stride]: Wc column statistics at 0, Hi row statistics at w
  int* flags;                // [b]: F_* of the sides that hold an edge value equal to cval
  int h, w, c, stride;
  int vec_out, vec_lab;      // 4-byte image stores / 16-byte label stores are aligned
};

// one sample's program, clamped so that every index derived from it stays inside the image and the table
struct Samp {
  int mode, cv;
  int ct, cl;                // first cropped row / column
  int pt, pb, pl, pr;        // pads, 0..64
  int hc, wc, hi, wi;        // the crop and the padded array I
};

using imgdev::clampi;
// imgdev::round_u8 in a 32-bit word, as the packed store takes it (the uint8_t form costs a mask here)
__device__ __forceinline__ uint32_t round_u8_word(double v) {
  const double r = fmin(fmax(floor(v + 0.5), 0.0), 255.0);
  return (uint32_t)(int)r;
}
__device__ __forceinline__ bool is_stat(int mode) { return mode >= PCUDA_PAD_MAXIMUM && mode <= PCUDA_PAD_MINIMUM; }

__device__ __forceinline__ Samp decode(const CpArgs& a, int n) {
  Samp s;
  const int* ia = a.iarg + n * kIArgs;
  int top = ia[0], right = ia[1], bottom = ia[2], left = ia[3];
  s.mode = ia[4];
  s.cv = clampi(ia[5], 0, 255);
  if (a.opcode[n] != 1) { top = right = bottom = left = 0; s.mode = PCUDA_PAD_CONSTANT; }      // copy
  if (s.mode < PCUDA_PAD_CONSTANT || s.mode > PCUDA_PAD_WRAP) s.mode = PCUDA_PAD_CONSTANT;
  s.ct = clampi(-top, 0, a.h - 1);
  s.cl = clampi(-left, 0, a.w - 1);
  s.hc = a.h - s.ct - clampi(-bottom, 0, a.h - 1 - s.ct);
  s.wc = a.w - s.cl - clampi(-right, 0, a.w - 1 - s.cl);
  s.pt = clampi(top, 0, kMaxPad); s.pb = clampi(bottom, 0, kMaxPad);
  s.pl = clampi(left, 0, kMaxPad); s.pr = clampi(right, 0, kMaxPad);
  s.hi = s.hc + s.pt + s.pb;
  s.wi = s.wc + s.pl + s.pr;
  return s;
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// numpy's statistic of the `len` bytes base[i step], as numpy.pad rounds it, by one wave; every lane returns it.  `mode` is
// uniform over the workgroup and EVERY wave of the workgroup calls this (the median's barriers); len == 0 returns garbage
// that the caller does not store.  hist: 256 counters of this wave
__device__ __forceinline__ int line_stat(int mode, const uint8_t* base, int step, int len, unsigned* hist, int lane) {
  if (mode == PCUDA_PAD_MEDIAN) {
#pragma unroll
    for (int k = 0; k < 4; ++k) hist[lane + 64 * k] = 0u;
    __syncthreads();
    for (int i = lane; i < len; i += 64) {
      const uint8_t* p = base + i * step;
      const uint8_t t = *p;
      atomicAdd(&hist[t], 1u);
      PCUDA_KEEP(p);
    }
    __syncthreads();
    // lane l owns the values 4 l .. 4 l + 3; an inclusive scan over the lanes gives the rank of each value
    int cnt[4], tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { cnt[k] = (int)hist[4 * lane + k]; tot += cnt[k]; }
    int inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    const int lo = (len - 1) >> 1, hi = len >> 1;      // the two middle ranks (equal for an odd count)
    int cum = inc - tot, va = 0, vb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int prev = cum;
      cum += cnt[k];
      if (prev <= lo && lo < cum) va = 4 * lane + k;
      if (prev <= hi && hi < cum) vb = 4 * lane + k;
    }
    const int sum = wave_max_i(va) + wave_max_i(vb);
    int r = sum >> 1;
    if (sum & 1) r += r & 1;                           // k + 0.5 rounds to the even neighbour
    return r;
  }
  int acc = mode == PCUDA_PAD_MINIMUM ? 255 : 0;
  for (int i = lane; i < len; i += 64) {
    const uint8_t* p = base + i * step;
    const int t = *p;
    if (mode == PCUDA_PAD_MAXIMUM) acc = max(acc, t);
    else if (mode == PCUDA_PAD_MINIMUM) acc = min(acc, t);
    else acc += t;
    PCUDA_KEEP(p);
  }
  if (mode == PCUDA_PAD_MAXIMUM) return wave_max_i(acc);
  if (mode == PCUDA_PAD_MINIMUM) return wave_min_i(acc);
  return (int)rint((double)wave_sum_i(acc) / (double)(len > 0 ? len : 1));      // (half to even, as numpy.round)
}

// grid (lines / 4, channel, sample): wave k of a workgroup owns cropped column or row 4 blockIdx.x + k
__global__ __launch_bounds__(256) void croppad_line_stats_kernel(const CpArgs a) {
  __shared__ unsigned s_hist[4][256];
  const int n = blockIdx.z, ch = blockIdx.y;
  const Samp s = decode(a, n);
  if (!is_stat(s.mode)) return;
  if ((int)blockIdx.x * 4 >= s.wc + s.hc) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int line = blockIdx.x * 4 + wave;
  const bool live = line < s.wc + s.hc, col = line < s.wc;
  const int yy = col ? 0 : min(line - s.wc, s.hc - 1);
  const uint8_t* src = a.in + (long long)n * a.h * a.w * a.c;
  const uint8_t* base = src + ((s.ct + yy) * a.w + s.cl + (col ? line : 0)) * a.c + ch;
  const int r = line_stat(s.mode, base, col ? a.w * a.c : a.c, live ? (col ? s.hc : s.wc) : 0, s_hist[wave], lane);
  if (live && lane == 0) a.tab[((long long)n * a.c + ch) * a.stride + (col ? line : a.w + s.pt + yy)] = (uint8_t)r;
}

// grid (sample): the statistic of the pad rows (over the column statistics, wave k = channel k) and the ramp flags
__global__ __launch_bounds__(256) void croppad_pad_stats_kernel(const CpArgs a) {
  __shared__ unsigned s_hist[4][256];
  __shared__ int s_flags;
  const int n = blockIdx.x;
  const Samp s = decode(a, n);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (is_stat(s.mode)) {
    if (s.pt + s.pb == 0) return;
    const bool live = wave < a.c;
    uint8_t* tab = a.tab + ((long long)n * a.c + (live ? wave : 0)) * a.stride;
    const int r = line_stat(s.mode, tab, 1, live ? s.wc : 0, s_hist[wave], lane);
    if (live)
      for (int y = lane; y < s.pt + s.pb; y += 64) tab[a.w + (y < s.pt ? y : s.hc + y)] = (uint8_t)r;
    return;
  }
  if (s.mode != PCUDA_PAD_LINEAR_RAMP) return;
  if (tid == 0) s_flags = (s.pt + s.pb) > 0 ? (F_LEFT | F_RIGHT) : 0;      // (the outermost pad row is cval itself)
  __syncthreads();
  const uint8_t* src = a.in + (long long)n * a.h * a.w * a.c;
  int f = 0;
  for (int i = tid; i < s.wc * a.c; i += 256) {
    const uint8_t* p0 = src + (s.ct * a.w + s.cl) * a.c + i;
    const uint8_t* p1 = src + ((s.ct + s.hc - 1) * a.w + s.cl) * a.c + i;
    const int t0 = *p0, t1 = *p1;
    if (t0 == s.cv) f |= F_TOP;
    if (t1 == s.cv) f |= F_BOTTOM;
    PCUDA_KEEP(p0); PCUDA_KEEP(p1);
  }
  for (int i = tid; i < s.hc * a.c; i += 256) {
    const int r = i / a.c, k = i - r * a.c;
    const uint8_t* p0 = src + ((s.ct + r) * a.w + s.cl) * a.c + k;
    const uint8_t* p1 = src + ((s.ct + r) * a.w + s.cl + s.wc - 1) * a.c + k;
    const int t0 = *p0, t1 = *p1;
    if (t0 == s.cv) f |= F_LEFT;
    if (t1 == s.cv) f |= F_RIGHT;
    PCUDA_KEEP(p0); PCUDA_KEEP(p1);
  }
  if (f) atomicOr(&s_flags, f);
  __syncthreads();
  if (tid == 0) a.flags[n] = s_flags;
}

// the index of the crop that an index i outside [0, n) folds to (edge and the ramp's edge texel: the nearest)
__device__ __forceinline__ int fold(int i, int n, int mode) {
  if ((unsigned)i < (unsigned)n) return i;
  if (mode == PCUDA_PAD_REFLECT && n > 1) {
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
  }
  if (mode == PCUDA_PAD_SYMMETRIC) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
  }
  if (mode == PCUDA_PAD_WRAP) {
    i %= n;
    return i < 0 ? i + n : i;
  }
  return i < 0 ? 0 : n - 1;
}

// one side of numpy's linear_ramp: position k (0 outermost) of `width` between end and the edge value e
__device__ __forceinline__ double ramp(double e, int k, int width, double end, bool any_step_zero) {
  const double delta = e - end;
  const double t = any_step_zero ? ((double)k / (double)width) * delta : (double)k * (delta / (double)width);
  return floor(end + t);
}

// texel (yi, xi) of I, both inside I: where its byte of channel 0 lives (`step` bytes between channels) and what turns the
// loaded byte into the value
struct Texel {
  const uint8_t* p;
  int step;
  int ky, kx;                // ramp positions, < 0: no ramp on that axis
  bool use_cval;
};

__device__ __forceinline__ Texel texel_of(const CpArgs& a, const Samp& s, const uint8_t* src, const uint8_t* tab, int yi, int xi) {
  Texel t;
  const int yy = yi - s.pt, xx = xi - s.pl;
  const bool iny = (unsigned)yy < (unsigned)s.hc, inx = (unsigned)xx < (unsigned)s.wc;
  t.ky = -1; t.kx = -1; t.use_cval = false; t.step = 1;
  if (is_stat(s.mode) && !(iny && inx)) {
    t.p = tab + (inx ? xx : a.w + yi);
    t.step = a.stride;
    return t;
  }
  const int fy = fold(yy, s.hc, s.mode), fx = fold(xx, s.wc, s.mode);
  t.p = src + ((s.ct + fy) * a.w + s.cl + fx) * a.c;
  if (s.mode == PCUDA_PAD_CONSTANT) t.use_cval = !(iny && inx);
  if (s.mode == PCUDA_PAD_LINEAR_RAMP) {
    if (!iny) t.ky = yy < 0 ? yy + s.pt : s.hc + s.pb - 1 - yy;
    if (!inx) t.kx = xx < 0 ? xx + s.pl : s.wc + s.pr - 1 - xx;
  }
  return t;
}

__device__ __forceinline__ double texel_value(const Samp& s, const Texel& t, int yi, int xi, int flags, uint8_t byte) {
  double v = t.use_cval ? (double)s.cv : (double)byte;
  if (t.ky >= 0) {
    const bool top = yi < s.pt;
    v = ramp(v, t.ky, top ? s.pt : s.pb, (double)s.cv, (flags & (top ? F_TOP : F_BOTTOM)) != 0);
  }
  if (t.kx >= 0) {
    const bool left = xi < s.pl;
    v = ramp(v, t.kx, left ? s.pl : s.pr, (double)s.cv, (flags & (left ? F_LEFT : F_RIGHT)) != 0);
  }
  return v;
}

__global__ __launch_bounds__(256) void croppad_sample_kernel(const CpArgs a) {
  const int n = blockIdx.y, tid = threadIdx.x;
  const int h = a.h, w = a.w, c = a.c;
  const int tiles_x = (w + kTileW - 1) / kTileW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const Samp s = decode(a, n);
  const int flags = s.mode == PCUDA_PAD_LINEAR_RAMP ? a.flags[n] : 0;
  const int xg = tx * kTileW + (tid & 15) * 4, y = ty * kTileH + (tid >> 4);
  if (xg >= w || y >= h) return;
  const uint8_t* src = a.in + (long long)n * h * w * c;
  const uint8_t* tab = a.tab + (long long)n * c * a.stride;
  const int* labn = a.lab_in ? a.lab_in + (long long)n * h * w : nullptr;
  const double ax = (double)s.wi / (double)w, ay = (double)s.hi / (double)h;
  const double sy = ((double)y + 0.5) * ay - 0.5;
  const double yf = floor(sy), wy1 = sy - yf, wy0 = 1.0 - wy1;
  const int ya = (int)yf, yn = (int)floor(sy + 0.5);
  const int yi[2] = {clampi(ya, 0, s.hi - 1), clampi(ya + 1, 0, s.hi - 1)};
  uint32_t words[4] = {0u, 0u, 0u, 0u};
  int labv[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (xg + j >= w) continue;
    const double sx = ((double)(xg + j) + 0.5) * ax - 0.5;
    const double xf = floor(sx), wx1 = sx - xf, wx0 = 1.0 - wx1;
    const int xa = (int)xf, xn = (int)floor(sx + 0.5);
    if (labn) {
      const int ly = yn - s.pt, lx = xn - s.pl;
      const bool lin = (unsigned)ly < (unsigned)s.hc && (unsigned)lx < (unsigned)s.wc;
      const int* pl = labn + ((s.ct + clampi(ly, 0, s.hc - 1)) * w + s.cl + clampi(lx, 0, s.wc - 1));
      const int l = *pl;
      labv[j] = lin ? l : 0;
      PCUDA_KEEP(pl);
    }
    const int xi[2] = {clampi(xa, 0, s.wi - 1), clampi(xa + 1, 0, s.wi - 1)};
    Texel t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = texel_of(a, s, src, tab, yi[q >> 1], xi[q & 1]);
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch) {
      if (ch >= c) break;
      const uint8_t* pc[4];
      double p[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pc[q] = t[q].p + ch * t[q].step;
        const uint8_t byte = *pc[q];
        p[q] = texel_value(s, t[q], yi[q >> 1], xi[q & 1], flags, byte);
      }
      double v = 0.0;
      v += p[0] * wy0 * wx0;
      v += p[1] * wy0 * wx1;
      v += p[2] * wy1 * wx0;
      v += p[3] * wy1 * wx1;
      const uint32_t res = round_u8_word(v);
      const int e = j * c + ch;
      words[e >> 2] |= res << (8 * (e & 3));
#pragma unroll
      for (int q = 0; q < 4; ++q) PCUDA_KEEP(pc[q]);      // (VMEM address rule, common.h)
    }
  }
  const long long pix = ((long long)n * h + y) * w + xg;
  uint8_t* dst = a.out + pix * c;
  if (a.vec_out && xg + 4 <= w) {
    uint32_t* po = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int k = 0; k < kMaxC; ++k)
      if (k < c) po[k] = words[k];
  } else {
#pragma unroll
    for (int e = 0; e < 4 * kMaxC; ++e)
      if (e < 4 * c && xg + e / c < w) dst[e] = (uint8_t)(words[e >> 2] >> (8 * (e & 3)));
  }
  if (a.lab_out) {
    int* pl = a.lab_out + pix;
    if (a.vec_lab && xg + 4 <= w) {
      *reinterpret_cast<int4*>(pl) = int4{labv[0], labv[1], labv[2], labv[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xg + j < w) pl[j] = labv[j];
    }
  }
}

inline int table_stride(int h, int w) { return (w + h + 2 * kMaxPad + 3) & ~3; }
inline bool dims_ok(int b, int h, int w, int c) {
  return b > 0 && b <= 65535 && c > 0 && c <= kMaxC && h >= 2 && w >= 2 && (long long)h * w * c < (1ll << 31) - 8192;
}

}  // namespace

extern "C" size_t pcuda_crop_pad_workspace_size(int b, int h, int w, int c) {
  if (!dims_ok(b, h, w, c)) return 0;
  return round16((size_t)b * c * table_stride(h, w)) + round16((size_t)b * sizeof(int));
}

extern "C" int pcuda_crop_pad(const uint8_t* in, uint8_t* out, const int* labels_in, int* labels_out, int b, int h, int w, int c,
                              const int* opcode, const int* iarg, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (!in || !out || !opcode || !iarg) PCUDA_FAIL(PCUDA_E_BADARG, "crop_pad: null pointer");
  if (in == out || (labels_in && labels_in == labels_out))
    PCUDA_FAIL(PCUDA_E_BADARG, "crop_pad: in == out (the input is never written)");
  if ((labels_in == nullptr) != (labels_out == nullptr))
    PCUDA_FAIL(PCUDA_E_BADARG, "crop_pad: labels come with an input and an output, or not at all");
  if (!dims_ok(b, h, w, c)) PCUDA_FAIL(PCUDA_E_BADARG, "crop_pad: bad dims (1..4 channels, H and W at least 2)");
  if (!workspace || workspace_bytes < pcuda_crop_pad_workspace_size(b, h, w, c))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "crop_pad: workspace too small");
  CpArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.lab_in = labels_in; a.lab_out = labels_out; a.opcode = opcode; a.iarg = iarg;
  a.h = h; a.w = w; a.c = c; a.stride = table_stride(h, w);
  a.tab = (uint8_t*)workspace;
  a.flags = reinterpret_cast<int*>((uint8_t*)workspace + round16((size_t)b * c * a.stride));
  a.vec_out = ((uintptr_t)out & 3) == 0 && (((long long)w * c) & 3) == 0;
  a.vec_lab = ((uintptr_t)labels_out & 15) == 0 && (w & 3) == 0;
  const size_t px = (size_t)b * h * w;
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)px * (2.0 * c + (labels_in ? 8.0 : 0.0)), (hipStream_t)s);
  hipLaunchKernelGGL(croppad_line_stats_kernel, dim3(cdiv(w + h, 4), c, b), dim3(256), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("croppad_line_stats_kernel");
  hipLaunchKernelGGL(croppad_pad_stats_kernel, dim3(b), dim3(256), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("croppad_pad_stats_kernel");
  hipLaunchKernelGGL(croppad_sample_kernel, dim3(cdiv(w, kTileW) * cdiv(h, kTileH), b), dim3(256), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("croppad_sample_kernel");
  return PCUDA_OK;
}
