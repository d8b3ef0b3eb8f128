// Device-side spacing resample of the MS-CMRSeg data: the .npy path of the reference's
// utils/read_nii_image.py (read_*_nii_save_npy :202-231, read_*_nii_label_save_npy :234-271): scipy.ndimage.zoom(order=1) of
// every slice to the new in-plane spacing, crop_volume, then (image - image.mean()) / image.std() over the volume; for labels
// the np.where remap, to_categorical, the zoom of the one-hot tensor, argmax and the crop -- fused, no one-hot tensor.
//
// The arithmetic is scipy's, in float64, and pinned bit for bit by tests/golden/resample.npz, whose expected arrays are the
// outputs of scipy.ndimage.zoom / numpy themselves (scripts/make_resample_golden.py); the convention is written out in
// include/pcuda_hip.h (pcuda_zoom_linear_crop).  Nothing here is contracted (-ffp-contract=off).
//
// zoom_table_kernel (tiny): per output row and column of the crop window the first tap's index i0 and the weight t, once per
// call, into the workspace; i0 = -1 marks a coordinate beyond the last sample (the pixel is 0) and pads each axis to a
// multiple of four entries.  zoom_kernel: a workgroup owns a band of rows of one slice; a lane owns four neighbouring output
// columns -- their table entries come in three 16-byte loads (the indices, two pairs of weights), once -- and walks down the
// band; neighbouring lanes read neighbouring elements of the two source rows; one 4 / 8 / 16-byte store per lane and row where
// the pitch allows it.  With STATS the workgroup also leaves the sums of its values (int64 sum and sum of squares, exact; or a float64 sum in a
// fixed order) as one partial per workgroup: no atomics.  stats_finalize_kernel reduces the partials in a fixed order (one
// workgroup) and leaves mean / std in the caller's two doubles: integers by the exact route (the numerator n Sxx - Sx Sx in
// 128-bit integers, converted once), fp32 in two passes (sqdev_partial_kernel: the squared deviations from the mean).
// standardize_kernel reads the two doubles and maps (x - mean) / std in float64 -> fp32, one or three channels.
// label_scan_kernel counts the input values whose remapped code is no class (an integer atomic); zoom_labels_kernel weighs the
// (at most four) classes under a pixel's taps.
// Every source index is clamped into the slice before it is used as an address, and a tap beyond the slice is replaced by 0
// after the load; every in-flight load's address stays alive (PCUDA_KEEP, VMEM address rule, common.h).
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBandRows = 32;                  // rows of one slice a workgroup of the zoom kernels owns
constexpr int kMaxRemap = 8;
constexpr int kMaxClasses = 8;
constexpr int kReduceBlocks = 1024;            // workgroups of sqdev_partial_kernel, at most

inline int round4(int v) { return (v + 3) & ~3; }

struct Geom {
  int sh, sw, zh, zw, oh, ow, y0, x0, ohp, owp;     // ohp / owp: oh / ow rounded up to a multiple of four (the table's pitch)
};

// the table: double t[ohp + owp] (rows, then columns), then int i0[ohp + owp]
struct Table {
  const double* ty;
  const double* tx;
  const int* iy;
  const int* ix;
};
inline size_t table_bytes(const Geom& g) { return (size_t)(g.ohp + g.owp) * 12; }   // (a multiple of 48)
inline Table table_at(void* ws, const Geom& g) {
  double* t = static_cast<double*>(ws);
  int* i = reinterpret_cast<int*>(t + g.ohp + g.owp);
  return Table{t, t + g.ohp, i, i + g.ohp};
}

__global__ __launch_bounds__(kThreads) void zoom_table_kernel(double* __restrict__ t, int* __restrict__ i0, const Geom g) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= g.ohp + g.owp) return;
  const bool is_y = e < g.ohp;
  const int k = is_y ? e : e - g.ohp;
  const int n_in = is_y ? g.sh : g.sw, n_out = is_y ? g.zh : g.zw, valid = is_y ? g.oh : g.ow, off = is_y ? g.y0 : g.x0;
  double tt = 0.0;
  int ii = -1;
  if (k < valid) {
    const double z = n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 1.0;
    const double cc = (double)(k + off) * z;
    const double fl = floor(cc);
    if (!(cc > (double)(n_in - 1))) {                    // beyond the last sample: no interpolation under mode='constant'
      ii = (int)fl;
      tt = cc - fl;
    }
  }
  t[e] = tt;
  i0[e] = ii;
}

// ------------------------------------------------------------------------------------------ values
template <int DT> struct Elem;
template <> struct Elem<PCUDA_PRE_F32> { using type = float; };
template <> struct Elem<PCUDA_PRE_I16> { using type = int16_t; };
template <> struct Elem<PCUDA_PRE_U8> { using type = uint8_t; };

template <int DT>
__device__ __forceinline__ double load_value(const void* base, long long i) {
  const typename Elem<DT>::type* p = static_cast<const typename Elem<DT>::type*>(base) + i;
  const typename Elem<DT>::type v = *p;
  PCUDA_KEEP(p);
  return (double)v;
}
__device__ __forceinline__ int load_code(const void* base, long long i, int is_u8) {
  if (is_u8) {
    const uint8_t* p = static_cast<const uint8_t*>(base) + i;
    const int v = *p;
    PCUDA_KEEP(p);
    return v;
  }
  const int16_t* p = static_cast<const int16_t*>(base) + i;
  const int v = *p;
  PCUDA_KEEP(p);
  return v;
}

// scipy's rounding of an interpolated value into an integer dtype: half away from zero, clamped, truncated
template <int DT>
__device__ __forceinline__ int round_int(double acc) {
  double r = acc > 0.0 ? acc + 0.5 : acc - 0.5;
  const double lo = DT == PCUDA_PRE_I16 ? -32768.0 : 0.0, hi = DT == PCUDA_PRE_I16 ? 32767.0 : 255.0;
  r = fmin(fmax(r, lo), hi);
  return (int)r;
}

// the table entries of a lane's four columns
struct Cols {
  int i0[4];
  double t[4];
};
__device__ __forceinline__ Cols load_cols(const Table& tb, int x) {      // x: a multiple of four below owp
  Cols c;
  const int4* pi = reinterpret_cast<const int4*>(tb.ix + x);
  const double2* pt = reinterpret_cast<const double2*>(tb.tx + x);
  const int4 i = *pi;
  const double2 a = pt[0], b = pt[1];
  c.i0[0] = i.x; c.i0[1] = i.y; c.i0[2] = i.z; c.i0[3] = i.w;
  c.t[0] = a.x; c.t[1] = a.y; c.t[2] = b.x; c.t[3] = b.y;
  PCUDA_KEEP(pi);
  PCUDA_KEEP(pt);
  return c;
}

struct ZoomArgs {
  const void* in;             // [n][sh][sw]
  void* out;                  // [n][oh][ow] of the same dtype
  void* partials;             // STATS: [gridDim.x][2] of int64 (integers) or double (fp32: [0] only)
  Table tb;
  Geom g;
  int bands;
};

template <int DT, bool VEC, bool STATS>
__global__ __launch_bounds__(kThreads) void zoom_kernel(const ZoomArgs a) {
  using T = typename Elem<DT>::type;
  const Geom& g = a.g;
  const int tid = threadIdx.x;
  const int img = blockIdx.x / a.bands, band = blockIdx.x - img * a.bands;
  const int groups = g.owp >> 2;
  const int gpb = groups < kThreads ? groups : kThreads;
  const int rows_per_pass = kThreads / gpb;
  const int gx = tid % gpb, ry = tid / gpb;
  const int row0 = band * kBandRows, row1 = row0 + kBandRows < g.oh ? row0 + kBandRows : g.oh;
  const long long slice = (long long)img * g.sh * g.sw;
  T* dst_img = static_cast<T*>(a.out) + (long long)img * g.oh * g.ow;
  long long s1 = 0, s2 = 0;                               // (integers)
  double fs = 0.0;                                        // (fp32)
  if (ry < rows_per_pass) {
    for (int grp = gx; grp < groups; grp += gpb) {
      const int ox0 = grp * 4;
      const Cols c = load_cols(a.tb, ox0);
      int xa[4], xb[4];
      double wx0[4];
      bool in_x[4], right[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        in_x[j] = c.i0[j] >= 0;
        xa[j] = in_x[j] ? c.i0[j] : 0;
        right[j] = xa[j] + 1 < g.sw;                      // a tap whose index equals the size is 0
        xb[j] = right[j] ? xa[j] + 1 : xa[j];
        wx0[j] = 1.0 - c.t[j];
      }
      for (int oy = row0 + ry; oy < row1; oy += rows_per_pass) {
        const int* piy = a.tb.iy + oy;
        const double* pty = a.tb.ty + oy;
        const int iy = *piy;
        const double t_y = *pty;
        PCUDA_KEEP(piy);
        PCUDA_KEEP(pty);
        const bool in_y = iy >= 0;
        const int ya = in_y ? iy : 0;
        const bool below = ya + 1 < g.sh;
        const long long ra = slice + (long long)ya * g.sw, rb = slice + (long long)(below ? ya + 1 : ya) * g.sw;
        const double wy0 = 1.0 - t_y, wy1 = t_y;
        double acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double c00 = load_value<DT>(a.in, ra + xa[j]);
          double c01 = load_value<DT>(a.in, ra + xb[j]);
          double c10 = load_value<DT>(a.in, rb + xa[j]);
          double c11 = load_value<DT>(a.in, rb + xb[j]);
          c01 = right[j] ? c01 : 0.0;
          c10 = below ? c10 : 0.0;
          c11 = right[j] && below ? c11 : 0.0;
          double v = (c00 * wy0) * wx0[j];
          v = v + (c01 * wy0) * c.t[j];
          v = v + (c10 * wy1) * wx0[j];
          v = v + (c11 * wy1) * c.t[j];
          acc[j] = in_x[j] && in_y ? v : 0.0;
        }
        T r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (DT == PCUDA_PRE_F32) r[j] = (T)acc[j];
          else r[j] = (T)round_int<DT>(acc[j]);
          if (STATS && ox0 + j < g.ow) {
            if (DT == PCUDA_PRE_F32) {
              fs += (double)r[j];
            } else {
              const long long q = (long long)r[j];
              s1 += q;
              s2 += q * q;
            }
          }
        }
        T* dst = dst_img + (long long)oy * g.ow + ox0;
        if (VEC) {
          if (DT == PCUDA_PRE_F32) {
            *reinterpret_cast<f32x4*>(dst) = f32x4{(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
          } else if (DT == PCUDA_PRE_I16) {
            uint2 w;
            w.x = ((uint32_t)(uint16_t)r[0]) | ((uint32_t)(uint16_t)r[1] << 16);
            w.y = ((uint32_t)(uint16_t)r[2]) | ((uint32_t)(uint16_t)r[3] << 16);
            *reinterpret_cast<uint2*>(dst) = w;
          } else {
            *reinterpret_cast<uint32_t*>(dst) = (uint32_t)(uint8_t)r[0] | ((uint32_t)(uint8_t)r[1] << 8) |
                                                ((uint32_t)(uint8_t)r[2] << 16) | ((uint32_t)(uint8_t)r[3] << 24);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (ox0 + j < g.ow) dst[j] = r[j];
        }
      }
    }
  }
  if (STATS) {
    // the workgroup's sums in a fixed order: the butterfly over a wave, then the four waves one after the other
    __shared__ long long s_i[4][2];
    __shared__ double s_f[4];
    const int lane = tid & 63, wave = tid >> 6;
    if (DT == PCUDA_PRE_F32) {
      fs = wave_sum_d(fs);
      if (lane == 0) s_f[wave] = fs;
    } else {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
      }
      if (lane == 0) {
        s_i[wave][0] = s1;
        s_i[wave][1] = s2;
      }
    }
    __syncthreads();
    if (tid == 0) {
      if (DT == PCUDA_PRE_F32) {
        double* p = static_cast<double*>(a.partials) + (long long)blockIdx.x * 2;
        p[0] = ((s_f[0] + s_f[1]) + s_f[2]) + s_f[3];
        p[1] = 0.0;
      } else {
        long long* p = static_cast<long long*>(a.partials) + (long long)blockIdx.x * 2;
        p[0] = s_i[0][0] + s_i[1][0] + s_i[2][0] + s_i[3][0];
        p[1] = s_i[0][1] + s_i[1][1] + s_i[2][1] + s_i[3][1];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ statistics
// an unsigned 128-bit integer to the nearest double (ties to even): the top 64 bits with the rest folded into a sticky bit
__device__ __forceinline__ double u128_to_double(unsigned __int128 v) {
  const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
  if (hi == 0) return (double)lo;
  const int shift = 64 - __clzll((long long)hi);
  unsigned long long top = (unsigned long long)(v >> shift);
  const unsigned long long rest = shift == 64 ? lo : lo & ((1ull << shift) - 1ull);
  top |= rest != 0 ? 1ull : 0ull;
  return ldexp((double)top, shift);
}

// the sum over a workgroup, in a fixed order; every thread of the (one) workgroup calls it; valid in thread 0
template <typename V>
__device__ __forceinline__ V block_sum(V v, V* s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// mode 0: integer partials -> stats[0] = mean, stats[1] = std; mode 1: fp32, the sums -> stats[0] = mean;
// mode 2: fp32, the sums of the squared deviations -> stats[1] = std.  One workgroup.
__global__ __launch_bounds__(kThreads) void stats_finalize_kernel(const void* __restrict__ partials, int count, long long n,
                                                                  double* __restrict__ stats, int mode) {
  __shared__ long long s_i[2][4];
  __shared__ double s_f[4];
  const int tid = threadIdx.x;
  if (mode == 0) {
    const long long* p = static_cast<const long long*>(partials);
    long long s1 = 0, s2 = 0;
    for (int i = tid; i < count; i += kThreads) {
      s1 += p[2 * i];
      s2 += p[2 * i + 1];
    }
    s1 = block_sum(s1, s_i[0]);
    s2 = block_sum(s2, s_i[1]);
    if (tid == 0) {
      const double dn = (double)n;
      const unsigned __int128 a = (unsigned __int128)(unsigned long long)n * (unsigned __int128)(unsigned long long)s2;
      const unsigned long long m = (unsigned long long)(s1 < 0 ? -s1 : s1);
      const unsigned __int128 b = (unsigned __int128)m * (unsigned __int128)m;
      stats[0] = (double)s1 / dn;
      stats[1] = sqrt(u128_to_double(a - b) / (dn * dn));          // (n Sxx >= Sx Sx: Cauchy-Schwarz)
    }
  } else {
    const double* p = static_cast<const double*>(partials);
    double s = 0.0;
    for (int i = tid; i < count; i += kThreads) s += p[2 * i];
    s = block_sum(s, s_f);
    if (tid == 0) {
      if (mode == 1) stats[0] = s / (double)n;
      else stats[1] = sqrt(s / (double)n);
    }
  }
}

// fp32, second pass: the squared deviations of the zoomed values from the mean, one partial per workgroup
__global__ __launch_bounds__(kThreads) void sqdev_partial_kernel(const float* __restrict__ z, long long total,
                                                                 const double* __restrict__ stats, double* __restrict__ partials) {
  __shared__ double s_f[4];
  const double mean = stats[0];
  const long long stride = (long long)gridDim.x * kThreads;
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
    const float* p = z + i;
    const double d = (double)*p - mean;
    s += d * d;
    PCUDA_KEEP(p);
  }
  s = block_sum(s, s_f);
  if (threadIdx.x == 0) {
    partials[2 * (long long)blockIdx.x] = s;
    partials[2 * (long long)blockIdx.x + 1] = 0.0;
  }
}

// (x - mean) / std in float64 -> fp32 out[n][channels][plane]; a lane owns four neighbouring values (VEC: plane % 4 == 0 and
// the pointers allow one load and one 16-byte store per channel)
template <int DT, bool VEC>
__global__ __launch_bounds__(kThreads) void standardize_kernel(const void* __restrict__ z, float* __restrict__ out,
                                                               const double* __restrict__ stats, long long total, long long plane,
                                                               int channels) {
  const long long e0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (e0 >= total) return;
  const double mean = stats[0], sd = stats[1];           // (uniform)
  double v[4];
  if (VEC) {
    if (DT == PCUDA_PRE_F32) {
      const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(z) + e0);
      const f32x4 q = *p;
      v[0] = (double)q[0]; v[1] = (double)q[1]; v[2] = (double)q[2]; v[3] = (double)q[3];
      PCUDA_KEEP(p);
    } else if (DT == PCUDA_PRE_I16) {
      const uint2* p = reinterpret_cast<const uint2*>(static_cast<const int16_t*>(z) + e0);
      const uint2 q = *p;
      v[0] = (double)(int16_t)(q.x & 0xffffu); v[1] = (double)(int16_t)(q.x >> 16);
      v[2] = (double)(int16_t)(q.y & 0xffffu); v[3] = (double)(int16_t)(q.y >> 16);
      PCUDA_KEEP(p);
    } else {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(z) + e0);
      const uint32_t q = *p;
      v[0] = (double)(q & 255u); v[1] = (double)((q >> 8) & 255u); v[2] = (double)((q >> 16) & 255u); v[3] = (double)(q >> 24);
      PCUDA_KEEP(p);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = load_value<DT>(z, e0 + j < total ? e0 + j : total - 1);
  }
  float r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = (float)((v[j] - mean) / sd);
  if (VEC) {
    const long long img = e0 / plane, rem = e0 - img * plane;
    float* d = out + img * channels * plane + rem;
    for (int ch = 0; ch < channels; ++ch) *reinterpret_cast<f32x4*>(d + ch * plane) = f32x4{r[0], r[1], r[2], r[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = e0 + j;
      if (e < total) {
        const long long img = e / plane, rem = e - img * plane;
        float* d = out + img * channels * plane + rem;
        for (int ch = 0; ch < channels; ++ch) d[ch * plane] = r[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ labels
struct LabelArgs {
  const void* in;             // [n][sh][sw] of int16 or uint8 raw codes
  uint8_t* out;               // [n][oh][ow]
  unsigned long long* stray;  // workspace: the number of input values whose remapped code is no class
  Table tb;
  Geom g;
  long long total;            // n sh sw
  int bands, is_u8, num_classes, num_remap;
  int from[kMaxRemap], to[kMaxRemap];
};

// the pairs in order, like the reference's chained np.where; no class: -1
__device__ __forceinline__ int remap_code(const LabelArgs& a, int v) {
#pragma unroll
  for (int k = 0; k < kMaxRemap; ++k)
    if (k < a.num_remap) v = v == a.from[k] ? a.to[k] : v;
  return v >= 0 && v < a.num_classes ? v : -1;
}

__global__ __launch_bounds__(kThreads) void label_scan_kernel(const LabelArgs a) {
  const long long stride = (long long)gridDim.x * kThreads;
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < a.total; i += stride)
    bad += remap_code(a, load_code(a.in, i, a.is_u8)) < 0 ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  if ((threadIdx.x & 63) == 0 && bad != 0) atomicAdd(a.stray, (unsigned long long)bad);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void zoom_labels_kernel(const LabelArgs a) {
  const Geom& g = a.g;
  const int tid = threadIdx.x;
  const int img = blockIdx.x / a.bands, band = blockIdx.x - img * a.bands;
  const int groups = g.owp >> 2;
  const int gpb = groups < kThreads ? groups : kThreads;
  const int rows_per_pass = kThreads / gpb;
  const int gx = tid % gpb, ry = tid / gpb;
  if (ry >= rows_per_pass) return;                       // (no barrier below)
  const int row0 = band * kBandRows, row1 = row0 + kBandRows < g.oh ? row0 + kBandRows : g.oh;
  const long long slice = (long long)img * g.sh * g.sw;
  uint8_t* dst_img = a.out + (long long)img * g.oh * g.ow;
  for (int grp = gx; grp < groups; grp += gpb) {
    const int ox0 = grp * 4;
    const Cols c = load_cols(a.tb, ox0);
    int xa[4], xb[4];
    double wx0[4];
    bool in_x[4], right[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      in_x[j] = c.i0[j] >= 0;
      xa[j] = in_x[j] ? c.i0[j] : 0;
      right[j] = xa[j] + 1 < g.sw;
      xb[j] = right[j] ? xa[j] + 1 : xa[j];
      wx0[j] = 1.0 - c.t[j];
    }
    for (int oy = row0 + ry; oy < row1; oy += rows_per_pass) {
      const int* piy = a.tb.iy + oy;
      const double* pty = a.tb.ty + oy;
      const int iy = *piy;
      const double t_y = *pty;
      PCUDA_KEEP(piy);
      PCUDA_KEEP(pty);
      const bool in_y = iy >= 0;
      const int ya = in_y ? iy : 0;
      const bool below = ya + 1 < g.sh;
      const long long ra = slice + (long long)ya * g.sw, rb = slice + (long long)(below ? ya + 1 : ya) * g.sw;
      const double wy0 = 1.0 - t_y, wy1 = t_y;
      unsigned r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // the classes under the four taps (-1: no class, or a tap beyond the slice: 0 in every channel) and the weight
        // each tap gives the channel of its class: (1.0 wy) wx
        int cls[4];
        cls[0] = remap_code(a, load_code(a.in, ra + xa[j], a.is_u8));
        cls[1] = remap_code(a, load_code(a.in, ra + xb[j], a.is_u8));
        cls[2] = remap_code(a, load_code(a.in, rb + xa[j], a.is_u8));
        cls[3] = remap_code(a, load_code(a.in, rb + xb[j], a.is_u8));
        cls[1] = right[j] ? cls[1] : -1;
        cls[2] = below ? cls[2] : -1;
        cls[3] = right[j] && below ? cls[3] : -1;
        const double w[4] = {wy0 * wx0[j], wy0 * c.t[j], wy1 * wx0[j], wy1 * c.t[j]};
        int best = kMaxClasses;                           // the first class whose channel rounds to 1
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          double acc = cls[0] == cls[k] ? w[0] : 0.0;
          acc = acc + (cls[1] == cls[k] ? w[1] : 0.0);
          acc = acc + (cls[2] == cls[k] ? w[2] : 0.0);
          acc = acc + (cls[3] == cls[k] ? w[3] : 0.0);
          const bool one = acc + 0.5 >= 1.0;             // uint8(trunc(acc + 0.5)) of a value in 0 .. 1
          best = cls[k] >= 0 && one && cls[k] < best ? cls[k] : best;
        }
        r[j] = in_x[j] && in_y && best < kMaxClasses ? (unsigned)best : 0u;   // every channel 0: argmax gives class 0
      }
      uint8_t* dst = dst_img + (long long)oy * g.ow + ox0;
      if (VEC) {
        *reinterpret_cast<uint32_t*>(dst) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ox0 + j < g.ow) dst[j] = (uint8_t)r[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ host
// the shared argument checks -> the geometry; 0 on success
int make_geom(const char* who, int n, int sh, int sw, int zh, int zw, int crop, Geom& g) {
  if (n < 0 || sh < 1 || sw < 1 || zh < 1 || zw < 1 || sh > 32768 || sw > 32768 || zh > 32768 || zw > 32768 || crop < 0)
    PCUDA_FAIL(PCUDA_E_BADARG, "%s: bad dims (sides 1..32768, a zoomed size of at least 1, crop >= 0)", who);
  memset(&g, 0, sizeof(g));
  g.sh = sh; g.sw = sw; g.zh = zh; g.zw = zw; g.oh = zh; g.ow = zw;
  if (crop > 0) {
    const int half = crop / 2;
    g.y0 = zh / 2 - half; g.x0 = zw / 2 - half;
    g.oh = g.ow = 2 * half;
    if (half < 1 || g.y0 < 0 || g.x0 < 0 || g.y0 + g.oh > zh || g.x0 + g.ow > zw)
      PCUDA_FAIL(PCUDA_E_BADARG, "%s: the crop window leaves the zoomed slice", who);
  }
  g.ohp = round4(g.oh); g.owp = round4(g.ow);
  if ((long long)n * sh * sw >= (1ll << 40) || (long long)n * g.oh * g.ow >= (1ll << 31) ||
      (long long)n * ((g.oh + kBandRows - 1) / kBandRows) >= (1ll << 31))
    PCUDA_FAIL(PCUDA_E_BADARG, "%s: volume too large (fewer than 2^31 output values)", who);
  return PCUDA_OK;
}
inline bool known_dtype(int dt) { return dt == PCUDA_PRE_F32 || dt == PCUDA_PRE_I16 || dt == PCUDA_PRE_U8; }
inline size_t elem_size(int dt) { return dt == PCUDA_PRE_F32 ? 4 : dt == PCUDA_PRE_I16 ? 2 : 1; }
inline int bands_of(const Geom& g) { return (g.oh + kBandRows - 1) / kBandRows; }

int launch_table(const Table& tb, const Geom& g, hipStream_t s) {
  hipLaunchKernelGGL(zoom_table_kernel, dim3(cdiv(g.ohp + g.owp, kThreads)), dim3(kThreads), 0, s, const_cast<double*>(tb.ty),
                     const_cast<int*>(tb.iy), g);
  PCUDA_CHECK_LAUNCH("zoom_table_kernel");
  return PCUDA_OK;
}

template <int DT, bool STATS>
int launch_zoom(const ZoomArgs& a, int n, hipStream_t s) {
  const size_t es = elem_size(DT);
  const bool vec = a.g.ow % 4 == 0 && ((uintptr_t)a.out & (4 * es - 1)) == 0;
  const dim3 grid(n * a.bands), block(kThreads);
  if (vec) hipLaunchKernelGGL((zoom_kernel<DT, true, STATS>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((zoom_kernel<DT, false, STATS>), grid, block, 0, s, a);
  PCUDA_CHECK_LAUNCH("zoom_kernel");
  return PCUDA_OK;
}

template <int DT>
int launch_standardize(const ZoomArgs& a, int n, int channels, float* out, double* stats, hipStream_t s) {
  const long long plane = (long long)a.g.oh * a.g.ow, total = plane * n;
  const int blocks = n * a.bands;
  int rc = launch_zoom<DT, true>(a, n, s);
  if (rc != PCUDA_OK) return rc;
  if (DT == PCUDA_PRE_F32) {
    double* partials = static_cast<double*>(a.partials);
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(kThreads), 0, s, (const void*)partials, blocks, total, stats, 1);
    PCUDA_CHECK_LAUNCH("stats_finalize_kernel");
    const long long want = (total + kThreads * 8 - 1) / (kThreads * 8);
    const int rblocks = (int)(want > kReduceBlocks ? kReduceBlocks : want);
    hipLaunchKernelGGL(sqdev_partial_kernel, dim3(rblocks), dim3(kThreads), 0, s, static_cast<const float*>(a.out), total,
                       (const double*)stats, partials);
    PCUDA_CHECK_LAUNCH("sqdev_partial_kernel");
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(kThreads), 0, s, (const void*)partials, rblocks, total, stats, 2);
    PCUDA_CHECK_LAUNCH("stats_finalize_kernel");
  } else {
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(kThreads), 0, s, (const void*)a.partials, blocks, total, stats, 0);
    PCUDA_CHECK_LAUNCH("stats_finalize_kernel");
  }
  const bool vec = plane % 4 == 0 && ((uintptr_t)out & 15) == 0;       // (the zoomed values start a 16-byte aligned block)
  const dim3 grid(cdiv((total + 3) / 4, kThreads)), block(kThreads);
  if (vec) hipLaunchKernelGGL((standardize_kernel<DT, true>), grid, block, 0, s, (const void*)a.out, out, (const double*)stats, total, plane, channels);
  else hipLaunchKernelGGL((standardize_kernel<DT, false>), grid, block, 0, s, (const void*)a.out, out, (const double*)stats, total, plane, channels);
  PCUDA_CHECK_LAUNCH("standardize_kernel");
  return PCUDA_OK;
}

// the workspace of pcuda_zoom_standardize: the table | the partials [max(n bands, kReduceBlocks)][2] of 8 bytes | the zoomed values
inline size_t partial_bytes(int n, const Geom& g) {
  const long long blocks = (long long)n * bands_of(g);
  return round16((size_t)(blocks > kReduceBlocks ? blocks : kReduceBlocks) * 16);
}

}  // namespace

extern "C" size_t pcuda_zoom_linear_crop_workspace_size(int zh, int zw, int crop) {
  Geom g;
  if (make_geom("zoom_linear_crop_workspace_size", 1, 1, 1, zh, zw, crop, g) != PCUDA_OK) return 0;
  return round16(table_bytes(g));
}

extern "C" int pcuda_zoom_linear_crop(const void* in, int dtype, int n, int sh, int sw, int zh, int zw, int crop, void* out,
                                      void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (!known_dtype(dtype)) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_linear_crop: dtype is fp32, int16 or uint8");
  Geom g;
  int rc = make_geom("zoom_linear_crop", n, sh, sw, zh, zw, crop, g);
  if (rc != PCUDA_OK) return rc;
  if (n == 0) return PCUDA_OK;
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_linear_crop: null pointer");
  if (in == (const void*)out) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_linear_crop: in == out (the input is never written)");
  if (!workspace || workspace_bytes < round16(table_bytes(g)) || ((uintptr_t)workspace & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "zoom_linear_crop: workspace too small (or not 16-byte aligned)");
  hipStream_t st = (hipStream_t)s;
  ZoomArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.tb = table_at(workspace, g); a.g = g; a.bands = bands_of(g);
  const double bytes = ((double)n * sh * sw + (double)n * g.oh * g.ow) * (double)elem_size(dtype);
  ProfScope prof(PCUDA_FAM_POINTWISE, bytes, st);
  rc = launch_table(a.tb, g, st);
  if (rc != PCUDA_OK) return rc;
  if (dtype == PCUDA_PRE_F32) return launch_zoom<PCUDA_PRE_F32, false>(a, n, st);
  if (dtype == PCUDA_PRE_I16) return launch_zoom<PCUDA_PRE_I16, false>(a, n, st);
  return launch_zoom<PCUDA_PRE_U8, false>(a, n, st);
}

extern "C" size_t pcuda_zoom_standardize_workspace_size(int dtype, int n, int zh, int zw, int crop) {
  Geom g;
  if (!known_dtype(dtype) || n <= 0 || make_geom("zoom_standardize_workspace_size", n, 1, 1, zh, zw, crop, g) != PCUDA_OK) return 0;
  return round16(table_bytes(g)) + partial_bytes(n, g) + round16((size_t)n * g.oh * g.ow * elem_size(dtype));
}

extern "C" int pcuda_zoom_standardize(const void* in, int dtype, int n, int sh, int sw, int zh, int zw, int crop, int channels,
                                      float* out, double* stats, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (!known_dtype(dtype)) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_standardize: dtype is fp32, int16 or uint8");
  if (channels != 1 && channels != 3) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_standardize: channels is 1 or 3");
  Geom g;
  int rc = make_geom("zoom_standardize", n, sh, sw, zh, zw, crop, g);
  if (rc != PCUDA_OK) return rc;
  if (n == 0) return PCUDA_OK;
  if (!in || !out || !stats) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_standardize: null pointer");
  if (in == (const void*)out) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_standardize: in == out (the input is never written)");
  if (((uintptr_t)stats & 7) != 0) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_standardize: stats is two doubles (8-byte aligned)");
  if (!workspace || workspace_bytes < pcuda_zoom_standardize_workspace_size(dtype, n, zh, zw, crop) || ((uintptr_t)workspace & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "zoom_standardize: workspace too small (or not 16-byte aligned)");
  hipStream_t st = (hipStream_t)s;
  char* ws = static_cast<char*>(workspace);
  ZoomArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.tb = table_at(ws, g); a.g = g; a.bands = bands_of(g);
  a.partials = ws + round16(table_bytes(g));
  a.out = ws + round16(table_bytes(g)) + partial_bytes(n, g);          // the zoomed values, in the volume's dtype
  const double px = (double)n * g.oh * g.ow;
  const double bytes = (double)n * sh * sw * (double)elem_size(dtype) + px * (2.0 * (double)elem_size(dtype) + 4.0 * channels);
  ProfScope prof(PCUDA_FAM_POINTWISE, bytes, st);
  rc = launch_table(a.tb, g, st);
  if (rc != PCUDA_OK) return rc;
  if (dtype == PCUDA_PRE_F32) return launch_standardize<PCUDA_PRE_F32>(a, n, channels, out, stats, st);
  if (dtype == PCUDA_PRE_I16) return launch_standardize<PCUDA_PRE_I16>(a, n, channels, out, stats, st);
  return launch_standardize<PCUDA_PRE_U8>(a, n, channels, out, stats, st);
}

extern "C" size_t pcuda_zoom_labels_workspace_size(int zh, int zw, int crop) {
  Geom g;
  if (make_geom("zoom_labels_workspace_size", 1, 1, 1, zh, zw, crop, g) != PCUDA_OK) return 0;
  return 16 + round16(table_bytes(g));                                  // the counter of stray codes | the table
}

extern "C" int pcuda_zoom_labels(const void* in, int dtype, int n, int sh, int sw, int zh, int zw, int crop, int num_classes,
                                 const int* remap, int num_remap, uint8_t* out, void* workspace, size_t workspace_bytes,
                                 pcuda_stream_t s) {
  if (dtype != PCUDA_PRE_I16 && dtype != PCUDA_PRE_U8) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_labels: dtype is int16 or uint8");
  if (num_classes < 2 || num_classes > kMaxClasses) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_labels: 2..8 classes");
  if (num_remap < 0 || num_remap > kMaxRemap || (num_remap > 0 && !remap))
    PCUDA_FAIL(PCUDA_E_BADARG, "zoom_labels: a remap table of at most 8 (from, to) pairs");
  Geom g;
  int rc = make_geom("zoom_labels", n, sh, sw, zh, zw, crop, g);
  if (rc != PCUDA_OK) return rc;
  if (n == 0) return PCUDA_OK;
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_labels: null pointer");
  if (in == (const void*)out) PCUDA_FAIL(PCUDA_E_BADARG, "zoom_labels: in == out (the input is never written)");
  if (!workspace || workspace_bytes < 16 + round16(table_bytes(g)) || ((uintptr_t)workspace & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "zoom_labels: workspace too small (or not 16-byte aligned)");
  hipStream_t st = (hipStream_t)s;
  LabelArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.stray = static_cast<unsigned long long*>(workspace);
  a.tb = table_at(static_cast<char*>(workspace) + 16, g); a.g = g; a.bands = bands_of(g);
  a.total = (long long)n * sh * sw;
  a.is_u8 = dtype == PCUDA_PRE_U8; a.num_classes = num_classes; a.num_remap = num_remap;
  for (int k = 0; k < num_remap; ++k) {
    a.from[k] = remap[2 * k];
    a.to[k] = remap[2 * k + 1];
  }
  const double bytes = (double)a.total * (double)elem_size(dtype) * 2.0 + (double)n * g.oh * g.ow;
  ProfScope prof(PCUDA_FAM_POINTWISE, bytes, st);
  if (hipMemsetAsync(workspace, 0, 16, st) != hipSuccess) PCUDA_FAIL(PCUDA_E_LAUNCH, "zoom_labels: hipMemsetAsync failed");
  rc = launch_table(a.tb, g, st);
  if (rc != PCUDA_OK) return rc;
  const long long want = (a.total + kThreads * 8 - 1) / (kThreads * 8);
  hipLaunchKernelGGL(label_scan_kernel, dim3((unsigned)(want > 2048 ? 2048 : want)), dim3(kThreads), 0, st, a);
  PCUDA_CHECK_LAUNCH("label_scan_kernel");
  const bool vec = g.ow % 4 == 0 && ((uintptr_t)out & 3) == 0;
  const dim3 grid(n * a.bands), block(kThreads);
  if (vec) hipLaunchKernelGGL((zoom_labels_kernel<true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((zoom_labels_kernel<false>), grid, block, 0, st, a);
  PCUDA_CHECK_LAUNCH("zoom_labels_kernel");
  return PCUDA_OK;
}
