// Fourier domain adaptation on the device: the low-frequency block of every source plane's
// amplitude spectrum is replaced by a target plane's, the source phase is kept.  The definition is this build's own, written
// with numpy's FFT (include/pcuda_hip.h, tests/fourier_refs.py); parity with the public FDA code is unpinned.
//
// No full FFT: the block is the (2 radius + 1)^2 bins with frequencies -radius..radius on both axes, so
//   v = s + real(sum over block bins of D[k] e^{+2 pi i (ky y / H + kx x / W)}) / (H W),   D[k] = (|T[k]| - |S[k]|) S[k] / |S[k]|
// (D[k] = |T[k]| where S[k] == 0), and only kx = 0..radius is kept: s and t are real, D[-k] = conj(D[k]), the bins kx >= 1
// count twice.  Three launches per call, all float64, every operation rounded on its own (-ffp-contract=off):
//   1. fourier_spectrum_kernel, one workgroup per (plane, band of rows): per group of rows the row DFT onto kx = 0..radius
//      (one lane per (row, column segment, kx), the pixels staged in LDS as float -- uint8 and fp32 values are exact there),
//      then the group's contribution to the (2 radius + 1) x (radius + 1) bins, accumulated in LDS; per-band partials go to the
//      workspace
//   2. fourier_amplitude_kernel (bank build) / fourier_delta_kernel (adapt): the bands summed in their order; |T| = hypot into
//      the bank, or D (times its weight 1 or 2, over H W, zero outside the sample's own radius) into the workspace
//   3. fourier_apply_kernel, one workgroup per (plane, band of rows): D in LDS, per row A[y, kx] = sum_ky D[ky, kx]
//      e^{2 pi i ky y / H} once, per pixel the radius + 1 terms.
// Twiddles come from sincospi(2 m / N) with m = (k x) mod N reduced in integers: a per-workgroup table over x for the W axis,
// per (row, ky) for the H axis; never from a growing product.  No atomics at all, no workgroup waits on another, every sum in
// a fixed order that depends on the shapes only: the same bits from run to run.
//
// ref_index entries >= r are clamped on the device; a NEGATIVE entry passes the sample through bit for bit (its planes skip
// the first two launches).  A sample radius is clamped into [0, radius].  Every load's address stays alive until its data has
// been consumed (PCUDA_KEEP, VMEM address rule, common.h).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxRadius = 32;
constexpr int kMaxSide = 4096;       // the W table is 16 W bytes of LDS
constexpr int kMaxC = 4;
constexpr int kChunk = 256;          // columns staged at a time
constexpr int kMaxGroup = 16;        // rows per group of the spectrum pass
constexpr int kBandRows = 32;        // rows per workgroup of the spectrum pass, about (whole groups, one at the least)
constexpr int kApplyRows = 16;       // rows per group of the apply pass
constexpr int kApplyGroups = 1;      // groups per workgroup of the apply pass
constexpr int kLdsHard = 160 * 1024;

struct alignas(16) cplx {
  double re, im;
};

// how the spectrum pass cuts a plane: g rows per group, seg column segments per row (g seg (radius + 1) <= 256 lanes),
// gp groups per band
struct Plan {
  int nb, nky, bins, g, seg, gp, band, nbands;
  size_t lds_spectrum, lds_apply;
};

inline Plan make_plan(int h, int w, int radius) {
  Plan p;
  p.nb = radius + 1; p.nky = 2 * radius + 1; p.bins = p.nky * p.nb;
  p.g = kThreads / p.nb;
  p.g = p.g > kMaxGroup ? kMaxGroup : p.g;
  p.g = p.g > h ? h : p.g;
  p.g = p.g < 1 ? 1 : p.g;
  p.seg = kThreads / (p.g * p.nb);
  const int cols = w < kChunk ? w : kChunk;
  p.seg = p.seg > cols ? cols : p.seg;
  p.seg = p.seg < 1 ? 1 : p.seg;
  p.gp = kBandRows / p.g;
  p.gp = p.gp < 1 ? 1 : p.gp;
  p.band = p.g * p.gp;
  p.nbands = h > 0 ? cdiv(h, p.band) : 0;
  p.lds_spectrum = sizeof(cplx) * ((size_t)w + p.bins + (size_t)p.g * p.nky + kThreads + (size_t)p.g * p.nb) +
                   sizeof(float) * (size_t)p.g * kChunk;
  p.lds_apply = sizeof(cplx) * ((size_t)w + p.bins + (size_t)kApplyRows * p.nky + (size_t)kApplyRows * p.nb);
  return p;
}

struct SpectrumArgs {
  const void* img;            // [n][h][w][c] fp32 or uint8
  const int* ref_index;       // [n] or null: planes of a sample with a negative entry are skipped
  cplx* partial;              // [n c][nbands][bins]
  int is_u8, h, w, c, radius;
  int g, seg, gp, nbands;
};

struct ReduceArgs {
  const cplx* partial;        // [planes][nbands][bins]
  double* amplitude;          // bank build: [planes][bins]
  const double* bank;         // adapt: [r c][bins]
  const int* ref_index;       // adapt: [n]
  const int* sample_radius;   // adapt: [n] or null
  cplx* delta;                // adapt: [planes][bins]
  double hw;                  // adapt: double(h) double(w)
  int planes, nbands, bins, nb, radius, c, r;
};

struct ApplyArgs {
  const void* in;             // [n][h][w][c]
  void* out;
  const cplx* delta;          // [n c][bins]
  const int* ref_index;       // [n]
  double lo, hi;
  int is_u8, h, w, c, radius, clip, nbands;
};

__device__ __forceinline__ cplx unit(long long m, int n, double sign) {   // e^{sign 2 pi i m / n}, 0 <= m < n
  double s, c;
  sincospi(2.0 * (double)m / (double)n, &s, &c);
  return cplx{c, sign * s};
}

__device__ __forceinline__ int sample_index(const int* ref_index, int smp) {
  const int* p = ref_index + smp;
  const int ri = *p;
  PCUDA_KEEP(p);
  return ri;
}

__device__ __forceinline__ float load_pixel(const void* img, long long e, int is_u8) {
  float v;
  if (is_u8) {
    const uint8_t* p = static_cast<const uint8_t*>(img) + e;
    v = (float)*p;
    PCUDA_KEEP(p);
  } else {
    const float* p = static_cast<const float*>(img) + e;
    v = *p;
    PCUDA_KEEP(p);
  }
  return v;
}

// ------------------------------------------------------------------------------------------
// 1. the band's contribution to S[ky, kx] = sum_y sum_x s[y, x] e^{-2 pi i (ky y / H + kx x / W)}, ky = -radius..radius,
//    kx = 0..radius
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fourier_spectrum_kernel(const SpectrumArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int h = a.h, w = a.w, c = a.c, rad = a.radius, nb = rad + 1, nky = 2 * rad + 1, bins = nky * nb;
  const int g = a.g, seg = a.seg;
  const int plane = blockIdx.x / a.nbands, band = blockIdx.x - plane * a.nbands;
  const int smp = plane / c, ch = plane - smp * c;
  if (a.ref_index && sample_index(a.ref_index, smp) < 0) return;   // (the whole workgroup: before any barrier)

  cplx* s_tw = reinterpret_cast<cplx*>(smem);          // [w]       e^{+2 pi i x / W}
  cplx* s_acc = s_tw + w;                              // [bins]    the band's bins
  cplx* s_e = s_acc + bins;                            // [g][nky]  e^{-2 pi i ky y / H} of the group's rows
  cplx* s_rp = s_e + g * nky;                          // [256]     the lanes' row sums
  cplx* s_rs = s_rp + kThreads;                        // [g][nb]   the rows' DFT
  float* s_px = reinterpret_cast<float*>(s_rs + g * nb);   // [g][kChunk]

  for (int i = tid; i < w; i += kThreads) s_tw[i] = unit(i, w, 1.0);
  for (int i = tid; i < bins; i += kThreads) s_acc[i] = cplx{0.0, 0.0};

  const int kx = tid % nb, rsg = tid / nb, sg = rsg % seg, row = rsg / seg;    // this lane's share of the row DFT
  const int band_y0 = band * g * a.gp;
  for (int gi = 0; gi < a.gp; ++gi) {
    const int y0 = band_y0 + gi * g;
    if (y0 >= h) break;
    const int gn = h - y0 < g ? h - y0 : g;
    __syncthreads();                                   // (the tables; the group before is done with s_e)
    for (int i = tid; i < gn * nky; i += kThreads) {
      const int rr = i / nky, ky = i - rr * nky - rad;
      long long m = ((long long)ky * (y0 + rr)) % h;
      m = m < 0 ? m + h : m;
      s_e[rr * nky + (ky + rad)] = unit(m, h, -1.0);
    }
    cplx acc = cplx{0.0, 0.0};
    for (int c0 = 0; c0 < w; c0 += kChunk) {
      const int cn = w - c0 < kChunk ? w - c0 : kChunk;
      __syncthreads();                                 // (the chunk before has been consumed)
      for (int i = tid; i < gn * cn; i += kThreads) {
        const int rr = i / cn, xx = i - rr * cn;
        s_px[rr * kChunk + xx] = load_pixel(a.img, (((long long)smp * h + (y0 + rr)) * w + (c0 + xx)) * c + ch, a.is_u8);
      }
      __syncthreads();
      if (row < gn) {
        const int len = (cn + seg - 1) / seg, xs = sg * len, xe = xs + len < cn ? xs + len : cn;
        if (xs < xe) {
          int idx = (int)(((long long)kx * (c0 + xs)) % w);
#pragma unroll 4
          for (int xx = xs; xx < xe; ++xx) {                       // (unrolled: four pairs of LDS reads in flight)
            const double v = (double)s_px[row * kChunk + xx];
            const cplx t = s_tw[idx];
            acc.re += v * t.re;
            acc.im -= v * t.im;
            idx += kx;
            idx = idx >= w ? idx - w : idx;
          }
        }
      }
    }
    s_rp[tid] = acc;
    __syncthreads();
    for (int i = tid; i < gn * nb; i += kThreads) {    // the segments of a row in their order
      const int rr = i / nb, k = i - rr * nb;
      cplx sum = cplx{0.0, 0.0};
      for (int s = 0; s < seg; ++s) {
        const cplx v = s_rp[(rr * seg + s) * nb + k];
        sum.re += v.re;
        sum.im += v.im;
      }
      s_rs[rr * nb + k] = sum;
    }
    __syncthreads();
    for (int it = tid; it < bins; it += kThreads) {    // (every bin belongs to one lane for the whole kernel)
      const int kyi = it / nb, k = it - kyi * nb;
      cplx sum = s_acc[it];
#pragma unroll 4
      for (int rr = 0; rr < gn; ++rr) {
        const cplx v = s_rs[rr * nb + k], e = s_e[rr * nky + kyi];
        sum.re += v.re * e.re - v.im * e.im;
        sum.im += v.re * e.im + v.im * e.re;
      }
      s_acc[it] = sum;
    }
  }
  cplx* dst = a.partial + ((long long)plane * a.nbands + band) * bins;
  for (int it = tid; it < bins; it += kThreads) dst[it] = s_acc[it];
}

// ------------------------------------------------------------------------------------------
// 2. the bands in their order
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ cplx sum_bands(const ReduceArgs& a, int plane, int bin) {
  cplx sum = cplx{0.0, 0.0};
  for (int k = 0; k < a.nbands; ++k) {
    const cplx* p = a.partial + ((long long)plane * a.nbands + k) * a.bins + bin;
    const cplx v = *p;
    PCUDA_KEEP(p);
    sum.re += v.re;
    sum.im += v.im;
  }
  return sum;
}

__global__ __launch_bounds__(kThreads) void fourier_amplitude_kernel(const ReduceArgs a) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= (long long)a.planes * a.bins) return;
  const int plane = (int)(gid / a.bins), bin = (int)(gid - (long long)plane * a.bins);
  const cplx s = sum_bands(a, plane, bin);
  a.amplitude[gid] = hypot(s.re, s.im);
}

__global__ __launch_bounds__(kThreads) void fourier_delta_kernel(const ReduceArgs a) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= (long long)a.planes * a.bins) return;
  const int plane = (int)(gid / a.bins), bin = (int)(gid - (long long)plane * a.bins);
  const int smp = plane / a.c, ch = plane - smp * a.c;
  int ri = sample_index(a.ref_index, smp);
  if (ri < 0) return;                                  // passed through: the apply pass never reads this plane's bins
  ri = ri > a.r - 1 ? a.r - 1 : ri;
  int rs = a.radius;
  if (a.sample_radius) {
    rs = sample_index(a.sample_radius, smp);
    rs = rs < 0 ? 0 : (rs > a.radius ? a.radius : rs);
  }
  const int kyi = bin / a.nb, kx = bin - kyi * a.nb, ky = kyi - a.radius;
  cplx d = cplx{0.0, 0.0};
  if (ky >= -rs && ky <= rs && kx <= rs) {
    const cplx s = sum_bands(a, plane, bin);
    const double* pt = a.bank + ((long long)ri * a.c + ch) * a.bins + bin;
    const double t = *pt;
    PCUDA_KEEP(pt);
    const double amp = hypot(s.re, s.im);
    if (amp == 0.0) {
      d = cplx{t, 0.0};
    } else {
      const double f = t - amp;
      d = cplx{f * (s.re / amp), f * (s.im / amp)};
    }
    const double wgt = kx == 0 ? 1.0 : 2.0;            // the bins kx >= 1 stand for their conjugates at -kx too
    d.re = d.re * wgt / a.hw;
    d.im = d.im * wgt / a.hw;
  }
  a.delta[gid] = d;
}

// ------------------------------------------------------------------------------------------
// 3. v = s + sum_kx real(A[y, kx] e^{2 pi i kx x / W}),  A[y, kx] = sum_ky D[ky, kx] e^{2 pi i ky y / H}
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_pixel(const ApplyArgs& a, long long e, double v) {
  if (a.is_u8) {
    const double q = fmin(fmax(rint(v), 0.0), 255.0);  // rint: half to even
    static_cast<uint8_t*>(a.out)[e] = (uint8_t)(int)q;
  } else {
    if (a.clip) v = fmin(fmax(v, a.lo), a.hi);
    static_cast<float*>(a.out)[e] = (float)v;          // nearest even
  }
}

__global__ __launch_bounds__(kThreads) void fourier_apply_kernel(const ApplyArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int h = a.h, w = a.w, c = a.c, rad = a.radius, nb = rad + 1, nky = 2 * rad + 1, bins = nky * nb;
  const int plane = blockIdx.x / a.nbands, band = blockIdx.x - plane * a.nbands;
  const int smp = plane / c, ch = plane - smp * c;
  const int band_y0 = band * kApplyRows * kApplyGroups;
  const int band_y1 = band_y0 + kApplyRows * kApplyGroups < h ? band_y0 + kApplyRows * kApplyGroups : h;

  if (sample_index(a.ref_index, smp) < 0) {            // passed through bit for bit (the whole workgroup: before any barrier)
    const int n = (band_y1 - band_y0) * w;
    for (int i = tid; i < n; i += kThreads) {
      const long long e = (((long long)smp * h + band_y0) * w + i) * c + ch;
      if (a.is_u8) {
        const uint8_t* p = static_cast<const uint8_t*>(a.in) + e;
        const uint8_t v = *p;
        PCUDA_KEEP(p);
        static_cast<uint8_t*>(a.out)[e] = v;
      } else {
        const uint32_t* p = static_cast<const uint32_t*>(a.in) + e;
        const uint32_t v = *p;
        PCUDA_KEEP(p);
        static_cast<uint32_t*>(a.out)[e] = v;
      }
    }
    return;
  }

  cplx* s_tw = reinterpret_cast<cplx*>(smem);          // [w]                e^{+2 pi i x / W}
  cplx* s_d = s_tw + w;                                // [nky][nb]          D
  cplx* s_e = s_d + bins;                              // [kApplyRows][nky]  e^{+2 pi i ky y / H}
  cplx* s_a = s_e + kApplyRows * nky;                  // [kApplyRows][nb]   A

  for (int i = tid; i < w; i += kThreads) s_tw[i] = unit(i, w, 1.0);
  for (int i = tid; i < bins; i += kThreads) {
    const cplx* p = a.delta + (long long)plane * bins + i;
    const double re = p->re, im = p->im;
    PCUDA_KEEP(p);
    s_d[i] = cplx{re, im};
  }
  for (int y0 = band_y0; y0 < band_y1; y0 += kApplyRows) {
    const int gn = band_y1 - y0 < kApplyRows ? band_y1 - y0 : kApplyRows;
    __syncthreads();                                   // (the tables; the group before is done with s_e and s_a)
    for (int i = tid; i < gn * nky; i += kThreads) {
      const int rr = i / nky, ky = i - rr * nky - rad;
      long long m = ((long long)ky * (y0 + rr)) % h;
      m = m < 0 ? m + h : m;
      s_e[i] = unit(m, h, 1.0);
    }
    __syncthreads();
    for (int i = tid; i < gn * nb; i += kThreads) {
      const int rr = i / nb, k = i - rr * nb;
      cplx sum = cplx{0.0, 0.0};
#pragma unroll 4
      for (int kyi = 0; kyi < nky; ++kyi) {
        const cplx d = s_d[kyi * nb + k], e = s_e[rr * nky + kyi];
        sum.re += d.re * e.re - d.im * e.im;
        sum.im += d.re * e.im + d.im * e.re;
      }
      s_a[i] = sum;
    }
    __syncthreads();
    for (int i = tid; i < gn * w; i += kThreads) {
      const int rr = i / w, x = i - rr * w;
      const long long e = (((long long)smp * h + (y0 + rr)) * w + x) * c + ch;
      const double s = (double)load_pixel(a.in, e, a.is_u8);
      const cplx* arow = s_a + rr * nb;
      double corr = arow[0].re;
      int idx = 0;
#pragma unroll 4
      for (int k = 1; k < nb; ++k) {
        idx += x;
        idx = idx >= w ? idx - w : idx;
        const cplx t = s_tw[idx], av = arow[k];
        corr += av.re * t.re - av.im * t.im;
      }
      store_pixel(a, e, s + corr);
    }
  }
}

// nonzero: the status the entry points return for these dims
inline int bad_dims(const char* who, int n, int h, int w, int c, int radius) {
  if (c < 1 || c > kMaxC) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "%s: 1..4 interleaved channels, got %d", who, c);
  if (radius > kMaxRadius) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "%s: radius %d is above %d", who, radius, kMaxRadius);
  if (n < 0 || h < 0 || w < 0 || radius < 0 || n > 65535 || h > 32768 || w > 32768 || (long long)n * h * w * c >= (1ll << 31) - 8192)
    PCUDA_FAIL(PCUDA_E_BADARG, "%s: bad dims (up to 65535 images of less than 2^31 values, radius >= 0)", who);
  return PCUDA_OK;
}

inline int bad_block(const char* who, int h, int w, int radius) {
  if (2 * radius + 1 > (h < w ? h : w))
    PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "%s: the block of radius %d (%d bins a side) does not fit %d x %d images: the bins would alias",
               who, radius, 2 * radius + 1, h, w);
  if (h > kMaxSide || w > kMaxSide) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "%s: sides up to %d, got %d x %d", who, kMaxSide, h, w);
  return PCUDA_OK;
}

inline bool dims_ok(int n, int h, int w, int c, int radius) {
  return n > 0 && h > 0 && w > 0 && c >= 1 && c <= kMaxC && radius >= 0 && radius <= kMaxRadius && n <= 65535 && h <= kMaxSide &&
         w <= kMaxSide && (long long)n * h * w * c < (1ll << 31) - 8192 && 2 * radius + 1 <= (h < w ? h : w);
}

template <typename K>
int raise_lds(K kern, size_t lds, DeviceOnce& once, const char* name) {
  if (lds > (size_t)kLdsHard) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "%s: %zu bytes of LDS", name, lds);
  if (const unsigned long long bit = lds > 32 * 1024 ? once.pending() : 0ull) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsHard) != hipSuccess)
      PCUDA_FAIL(PCUDA_E_LAUNCH, "%s: cannot opt in to %d bytes of LDS", name, kLdsHard);
    once.mark(bit);
  }
  return PCUDA_OK;
}

int launch_spectrum(const void* img, int is_u8, int n, int h, int w, int c, int radius, const int* ref_index, cplx* partial,
                    const Plan& p, hipStream_t s) {
  static DeviceOnce once;
  if (int rc = raise_lds(fourier_spectrum_kernel, p.lds_spectrum, once, "fourier_spectrum_kernel")) return rc;
  SpectrumArgs a;
  memset(&a, 0, sizeof(a));
  a.img = img; a.ref_index = ref_index; a.partial = partial;
  a.is_u8 = is_u8; a.h = h; a.w = w; a.c = c; a.radius = radius;
  a.g = p.g; a.seg = p.seg; a.gp = p.gp; a.nbands = p.nbands;
  hipLaunchKernelGGL(fourier_spectrum_kernel, dim3(n * c * p.nbands), dim3(kThreads), p.lds_spectrum, s, a);
  PCUDA_CHECK_LAUNCH("fourier_spectrum_kernel");
  return PCUDA_OK;
}

inline size_t partial_bytes(int n, int c, const Plan& p) { return round16((size_t)n * c * p.nbands * p.bins * sizeof(cplx)); }

}  // namespace

extern "C" size_t pcuda_fourier_bank_size(int r, int c, int radius) {
  if (r <= 0 || c < 1 || c > kMaxC || radius < 0 || radius > kMaxRadius) return 0;
  return round16((size_t)r * c * (2 * radius + 1) * (radius + 1) * sizeof(double));
}

extern "C" size_t pcuda_fourier_bank_workspace_size(int r, int h, int w, int c, int radius) {
  if (!dims_ok(r, h, w, c, radius)) return 0;
  return partial_bytes(r, c, make_plan(h, w, radius));
}

extern "C" int pcuda_fourier_bank_build(const void* refs, int is_u8, int r, int h, int w, int c, int radius, void* bank,
                                        size_t bank_bytes, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (int rc = bad_dims("fourier_bank_build", r, h, w, c, radius)) return rc;
  if (r == 0 || h == 0 || w == 0) return PCUDA_OK;
  if (int rc = bad_block("fourier_bank_build", h, w, radius)) return rc;
  if (!refs || !bank) PCUDA_FAIL(PCUDA_E_BADARG, "fourier_bank_build: null pointer");
  if (refs == bank) PCUDA_FAIL(PCUDA_E_BADARG, "fourier_bank_build: refs == bank (the references are never written)");
  if (bank_bytes < pcuda_fourier_bank_size(r, c, radius) || ((uintptr_t)bank & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "fourier_bank_build: bank too small (or not 16-byte aligned)");
  const Plan p = make_plan(h, w, radius);
  const size_t need = partial_bytes(r, c, p);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "fourier_bank_build: workspace too small (or not 16-byte aligned)");
  const size_t elems = (size_t)r * h * w * c;
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)elems * (is_u8 ? 1.0 : 4.0), (hipStream_t)s);
  if (int rc = launch_spectrum(refs, is_u8, r, h, w, c, radius, nullptr, static_cast<cplx*>(workspace), p, (hipStream_t)s)) return rc;
  ReduceArgs a;
  memset(&a, 0, sizeof(a));
  a.partial = static_cast<const cplx*>(workspace); a.amplitude = static_cast<double*>(bank);
  a.planes = r * c; a.nbands = p.nbands; a.bins = p.bins; a.nb = p.nb; a.radius = radius; a.c = c; a.r = r;
  hipLaunchKernelGGL(fourier_amplitude_kernel, dim3(cdiv((long long)a.planes * a.bins, kThreads)), dim3(kThreads), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("fourier_amplitude_kernel");
  return PCUDA_OK;
}

extern "C" size_t pcuda_fourier_adapt_workspace_size(int b, int h, int w, int c, int radius) {
  if (!dims_ok(b, h, w, c, radius)) return 0;
  const Plan p = make_plan(h, w, radius);
  return partial_bytes(b, c, p) + round16((size_t)b * c * p.bins * sizeof(cplx));
}

extern "C" int pcuda_fourier_adapt(const void* in, void* out, int is_u8, int b, int h, int w, int c, const void* bank, int r,
                                   int radius, const int* ref_index, const int* sample_radius, int clip, double clip_lo,
                                   double clip_hi, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (int rc = bad_dims("fourier_adapt", b, h, w, c, radius)) return rc;
  if (b == 0 || h == 0 || w == 0) return PCUDA_OK;
  if (int rc = bad_block("fourier_adapt", h, w, radius)) return rc;
  if (r < 1 || r > 65535) PCUDA_FAIL(PCUDA_E_BADARG, "fourier_adapt: a bank of 1..65535 references, got %d", r);
  if (clip && !(clip_lo <= clip_hi)) PCUDA_FAIL(PCUDA_E_BADARG, "fourier_adapt: clip needs lo <= hi");
  if (!in || !out || !bank || !ref_index) PCUDA_FAIL(PCUDA_E_BADARG, "fourier_adapt: null pointer");
  if (in == out) PCUDA_FAIL(PCUDA_E_BADARG, "fourier_adapt: in == out (the input is never written)");
  if (((uintptr_t)bank & 15) != 0) PCUDA_FAIL(PCUDA_E_WORKSPACE, "fourier_adapt: bank not 16-byte aligned");
  const Plan p = make_plan(h, w, radius);
  const size_t part = partial_bytes(b, c, p), need = part + round16((size_t)b * c * p.bins * sizeof(cplx));
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "fourier_adapt: workspace too small (or not 16-byte aligned)");
  cplx* partial = static_cast<cplx*>(workspace);
  cplx* delta = reinterpret_cast<cplx*>(static_cast<unsigned char*>(workspace) + part);
  static DeviceOnce once;
  if (int rc = raise_lds(fourier_apply_kernel, p.lds_apply, once, "fourier_apply_kernel")) return rc;
  const size_t elems = (size_t)b * h * w * c;
  // bytes: the source read twice, the output written once
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)elems * (is_u8 ? 1.0 : 4.0) * 3.0, (hipStream_t)s);
  if (int rc = launch_spectrum(in, is_u8, b, h, w, c, radius, ref_index, partial, p, (hipStream_t)s)) return rc;
  ReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.partial = partial; ra.bank = static_cast<const double*>(bank); ra.ref_index = ref_index; ra.sample_radius = sample_radius;
  ra.delta = delta; ra.hw = (double)h * (double)w;
  ra.planes = b * c; ra.nbands = p.nbands; ra.bins = p.bins; ra.nb = p.nb; ra.radius = radius; ra.c = c; ra.r = r;
  hipLaunchKernelGGL(fourier_delta_kernel, dim3(cdiv((long long)ra.planes * ra.bins, kThreads)), dim3(kThreads), 0, (hipStream_t)s, ra);
  PCUDA_CHECK_LAUNCH("fourier_delta_kernel");
  ApplyArgs aa;
  memset(&aa, 0, sizeof(aa));
  aa.in = in; aa.out = out; aa.delta = delta; aa.ref_index = ref_index; aa.lo = clip_lo; aa.hi = clip_hi;
  aa.is_u8 = is_u8; aa.h = h; aa.w = w; aa.c = c; aa.radius = radius; aa.clip = clip;
  aa.nbands = cdiv(h, kApplyRows * kApplyGroups);
  hipLaunchKernelGGL(fourier_apply_kernel, dim3(b * c * aa.nbands), dim3(kThreads), p.lds_apply, (hipStream_t)s, aa);
  PCUDA_CHECK_LAUNCH("fourier_apply_kernel");
  return PCUDA_OK;
}
