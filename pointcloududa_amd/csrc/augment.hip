// Device-side light augmentation of the loader path: horizontal / vertical flips and one affine
// warp per sample (data_generator_mmwhs.py:87-122 light_aug, data_generator_mscmrseg.py:135-167 simple_aug), fused with the
// batch assembly of pointwise.hip (centre crop, channel-last -> channel-first, labels -> one-hot) and with the MM-WHS
// batch-global min-max rescale to uint8 and back (data_generator_mmwhs.py:246-254).  The two halves of that round trip also
// stand alone (f6b: pcuda_quantize_u8, pcuda_augment_assemble_dequant), so that uint8 stages can run between them.
//
// Convention (this build's own: imgaug / cv2 are not vendored by the reference, parity of the sub-pixel rule is unpinned;
// pinned against scipy.ndimage.affine_transform(mode="grid-constant") by tests/golden/augment.npz):
//   * the host composes flips and the affine in float64 and hands over the INVERSE 2x3 matrix per sample
//     (output pixel -> source coordinate); no trigonometry here
//   * source coordinates and the interpolation run in float64 (the library is built with -ffp-contract=off)
//   * order 0: the texel at floor(coord + 0.5); order 1: bilinear over four neighbours, a neighbour outside the image
//     contributes cval; the sum runs in scipy's order ((p * wy) * wx, rows outer, columns inner, accumulated from 0)
//   * quantised modes round floor(v + 0.5) and clip to [0, 255]; labels always take order 0 and fill 0
//
// The kernels have next to no LDS footprint (a 1 KB table at most), so they can share a compute unit with another process's workgroups: every gather goes
// through an address that stays alive behind the code that consumes the data (PCUDA_KEEP, VMEM address rule, common.h), and
// every gather address is clamped into the image, so a garbage matrix reads wrong texels, never out of bounds.
#include "common.h"

#include <float.h>

namespace {

// ------------------------------------------------------------------------------------------
// batch-global min / max of an fp32 buffer -> two device floats (no host read)
// ------------------------------------------------------------------------------------------
constexpr int kMinMaxBlocks = 1024;

__device__ __forceinline__ void wave_minmax(float& lo, float& hi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
}

// one partial (min, max) per workgroup; fminf / fmaxf skip NaNs, and any order of min / max gives the same bits
__global__ __launch_bounds__(256) void minmax_kernel(const float* __restrict__ x, long long numel, int vec,
                                                     float* __restrict__ partial) {
  __shared__ float slo[4], shi[4];
  float lo = FLT_MAX, hi = -FLT_MAX;
  const long long tid = blockIdx.x * 256ll + threadIdx.x, nthr = 256ll * gridDim.x;
  if (vec) {
    const long long n4 = numel >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    for (long long i = tid; i < n4; i += nthr) {
      const f32x4* p = x4 + i;
      const f32x4 v = *p;
      lo = fminf(fminf(lo, fminf(v.x, v.y)), fminf(v.z, v.w));
      hi = fmaxf(fmaxf(hi, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
      PCUDA_KEEP(p);
    }
    for (long long i = (n4 << 2) + tid; i < numel; i += nthr) {
      const float* p = x + i;
      const float v = *p;
      lo = fminf(lo, v); hi = fmaxf(hi, v);
      PCUDA_KEEP(p);
    }
  } else {
    for (long long i = tid; i < numel; i += nthr) {
      const float* p = x + i;
      const float v = *p;
      lo = fminf(lo, v); hi = fmaxf(hi, v);
      PCUDA_KEEP(p);
    }
  }
  wave_minmax(lo, hi);
  if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = fminf(fminf(slo[0], slo[1]), fminf(slo[2], slo[3]));
    partial[2 * blockIdx.x + 1] = fmaxf(fmaxf(shi[0], shi[1]), fmaxf(shi[2], shi[3]));
  }
}

// second, tiny launch: one wave folds the partials
__global__ __launch_bounds__(64) void minmax_final_kernel(const float* __restrict__ partial, int n, float* __restrict__ out2) {
  float lo = FLT_MAX, hi = -FLT_MAX;
  for (int i = threadIdx.x; i < n; i += 64) {
    const float* p = partial + 2 * i;
    const float a = p[0], b = p[1];
    lo = fminf(lo, a); hi = fmaxf(hi, b);
    PCUDA_KEEP(p);
  }
  wave_minmax(lo, hi);
  if (threadIdx.x == 0) { out2[0] = lo; out2[1] = hi; }
}

// ------------------------------------------------------------------------------------------
// fp32 -> uint8 with the (min, max) pair above: the joint in front of the uint8 stages (data_generator_mmwhs.py:248-249)
// ------------------------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kQuantBlocks = 4096;
constexpr int kQuantPerLane = 16;      // four float4 loads -> one 16-byte store

// images = (images - img_min) * 255. / (img_max - img_min); np.array(images, dtype=np.uint8): fp32, every operation rounded
// on its own, truncation.  The kernel moves 5 bytes per element, so the true division costs nothing that shows (the warp's
// texel_value runs it per gathered texel and therefore multiplies by a reciprocal outside a band; same integers).
// max == min (0 / 0 in the reference): 0; a NaN element: 0 (fmaxf returns the other operand)
__device__ __forceinline__ uint32_t quantize_one(float x, float mn, float range) {
  float q = ((x - mn) * 255.f) / range;
  q = range != 0.f ? q : 0.f;
  return (uint32_t)(int)fminf(fmaxf(q, 0.f), 255.f);
}

__device__ __forceinline__ uint32_t quantize_four(f32x4 v, float mn, float range) {
  return quantize_one(v.x, mn, range) | (quantize_one(v.y, mn, range) << 8) | (quantize_one(v.z, mn, range) << 16) |
         (quantize_one(v.w, mn, range) << 24);
}

// vec (x and q 16-byte aligned): a lane owns 16 consecutive elements; the last numel % 16 elements, and everything when a
// pointer is misaligned, go one element per lane
__global__ __launch_bounds__(256) void quantize_u8_kernel(const float* __restrict__ x, long long numel, int vec,
                                                          const float* __restrict__ minmax, uint8_t* __restrict__ q) {
  const float mn = minmax[0], range = minmax[1] - mn;
  const long long tid = blockIdx.x * 256ll + threadIdx.x, nthr = 256ll * gridDim.x;
  long long done = 0;
  if (vec) {
    const long long n16 = numel / kQuantPerLane;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    u32x4* q16 = reinterpret_cast<u32x4*>(q);
    for (long long i = tid; i < n16; i += nthr) {
      const f32x4* p = x4 + 4 * i;
      const f32x4 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
      q16[i] = u32x4{quantize_four(v0, mn, range), quantize_four(v1, mn, range), quantize_four(v2, mn, range),
                     quantize_four(v3, mn, range)};
      PCUDA_KEEP(p);
    }
    done = n16 * kQuantPerLane;
  }
  for (long long i = done + tid; i < numel; i += nthr) {
    const float* p = x + i;
    const float v = *p;
    q[i] = (uint8_t)quantize_one(v, mn, range);
    PCUDA_KEEP(p);
  }
}

// ------------------------------------------------------------------------------------------
// flips + affine + rescale + batch assembly
// ------------------------------------------------------------------------------------------
struct AugArgs {
  const void* img;          // [b][h][w][c] fp32 or uint8
  const int* lab;           // [b][h][w] (may be null)
  const double* inv;        // [b][6]: sx = m0 x + m1 y + m2, sy = m3 x + m4 y + m5
  const int* order;         // [b]: 0 nearest, anything else bilinear
  const int* cval;          // [b]: fill value of the image, 0..255
  const float* minmax;      // [2] (PCUDA_AUG_MINMAX)
  float* img_out;           // [b][c][oh][ow] (may be null)
  uint8_t* onehot;          // [b][k][oh][ow] (may be null)
  uint8_t* fullmask;        // [b][h][w] label > 0 (may be null)
  int* lab_full;            // [b][h][w] warped labels (may be null)
  uint8_t* img_u8_full;     // [b][h][w][c] warped uint8 image (may be null; uint8 input only)
  int b, h, w, c, k;
  int y0, x0, oh, ow;       // the centre crop inside the image
  int rx0, ry0, rx1, ry1;   // the region this launch walks (image coordinates; rx0 may be -3..0 so that the groups of
                            // four pixels start at multiples of four of the CROPPED row)
  int vec_img, vec_oh, vec_mask;
};

constexpr int kTileW = 64, kTileH = 16;      // 16 lanes x 4 consecutive x, 16 rows: one wave covers 64 x 4 pixels

template <bool IN_U8>
struct Texel;
template <>
struct Texel<false> { typedef float type; };
template <>
struct Texel<true> { typedef uint8_t type; };

// the value a texel contributes to the warp, as the (possibly quantised) number that is interpolated
template <bool IN_U8, int MODE>
__device__ __forceinline__ double texel_value(typename Texel<IN_U8>::type t, float mn, float range, float rinv) {
  if (IN_U8) return (double)t;
  if (MODE == PCUDA_AUG_MINMAX) {
    // images = (images - img_min) * 255. / (img_max - img_min); np.array(images, dtype=np.uint8): fp32, truncation.
    // Only trunc(q) is needed, and a true division per gathered texel made the kernel ALU-bound: q' = s * fl(1 / range)
    // lies within 1.5 ulp (4.6e-5 at 255) of the divided q, so it truncates to the same integer unless it lies that close
    // to one; inside a five times wider band the true division runs.  max == min (0 / 0 in the reference): q = 0
    const float s = ((float)t - mn) * 255.f;
    float q = s * rinv;
    if (fabsf(q - rintf(q)) < 2.5e-4f) q = s / range;
    q = range != 0.f ? q : 0.f;
    return (double)(int)fminf(fmaxf(q, 0.f), 255.f);
  }
  return (double)t;
}

// lut[r] = the fp32 value of grey level r (one true division per workgroup thread instead of one per output value)
template <bool IN_U8, int MODE>
__device__ __forceinline__ float finish(double v, bool exact, const float* lut) {
  if (!IN_U8 && MODE == PCUDA_AUG_NONE) return (float)v;      // fp32 pass-through: no quantisation
  double r = exact ? v : floor(v + 0.5);
  r = fmin(fmax(r, 0.0), 255.0);
  if (MODE == PCUDA_AUG_NONE) return (float)r;
  return lut[(int)r];
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool IN_U8, int MODE, int ORD>
__device__ __forceinline__ void augment_body(const AugArgs& a, int n, int xg, int y, double m0, double m1, double m2,
                                             double m3, double m4, double m5, int cv, float mn, float range, float rinv,
                                             const float* lut) {
  typedef typename Texel<IN_U8>::type T;
  constexpr int NB = ORD ? 4 : 1;
  const int h = a.h, w = a.w, c = a.c;
  const T* img = reinterpret_cast<const T*>(a.img) + (long long)n * h * w * c;
  const bool row_in_crop = y >= a.y0 && y < a.y0 + a.oh;

  bool valid[4], in_crop[4];
  int loff[4];                 // nearest source pixel (labels), clamped
  bool lin[4];
  const T* pt[4][NB];          // clamped texel addresses (channel 0)
  bool tin[4][NB];
  double wx1[4], wy1[4];
  bool any_crop = false, all_crop = true, all_valid = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = xg + j;
    valid[j] = x >= 0 && x < w;
    in_crop[j] = row_in_crop && x >= a.x0 && x < a.x0 + a.ow;
    any_crop |= in_crop[j]; all_crop &= in_crop[j]; all_valid &= valid[j];
    double sx = m0 * (double)x + m1 * (double)y + m2;
    double sy = m3 * (double)x + m4 * (double)y + m5;
    // beyond one pixel outside every neighbour is outside anyway; NaN -> -2 (fmax returns the other operand)
    sx = fmin(fmax(sx, -2.0), (double)w + 1.0);
    sy = fmin(fmax(sy, -2.0), (double)h + 1.0);
    const int xn = (int)floor(sx + 0.5), yn = (int)floor(sy + 0.5);
    lin[j] = xn >= 0 && xn < w && yn >= 0 && yn < h;
    loff[j] = clampi(yn, h - 1) * w + clampi(xn, w - 1);
    if (ORD == 0) {
      pt[j][0] = img + (long long)loff[j] * c;
      tin[j][0] = lin[j];
      wx1[j] = wy1[j] = 0.0;
    } else {
      const double xf = floor(sx), yf = floor(sy);
      wx1[j] = sx - xf; wy1[j] = sy - yf;
      const int xa = (int)xf, ya = (int)yf;
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const int xx = xa + (q & 1), yy = ya + (q >> 1);
        tin[j][q] = xx >= 0 && xx < w && yy >= 0 && yy < h;
        pt[j][q] = img + (long long)(clampi(yy, h - 1) * w + clampi(xx, w - 1)) * c;
      }
    }
  }

  const bool want_img = any_crop && a.img_out;
  const bool want_u8 = IN_U8 && a.img_u8_full;
  if (want_img || want_u8) {
    const long long plane = (long long)a.oh * a.ow;
    const long long dst = (long long)(y - a.y0) * a.ow + (xg - a.x0);
    for (int ch = 0; ch < c; ++ch) {
      float o[4];
      double rq[4];
      const T* pc[4][NB];      // this channel's addresses: kept alive behind the code that consumes the data
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        T t[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) { pc[j][q] = pt[j][q] + ch; t[q] = *pc[j][q]; }
        double p[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) p[q] = tin[j][q] ? texel_value<IN_U8, MODE>(t[q], mn, range, rinv) : (double)cv;
        double v;
        if (ORD == 0) {
          v = p[0];
        } else {
          const double wx0 = 1.0 - wx1[j], wy0 = 1.0 - wy1[j];
          v = 0.0;
          v += p[0] * wy0 * wx0;
          v += p[1] * wy0 * wx1[j];
          v += p[ORD ? 2 : 0] * wy1[j] * wx0;
          v += p[ORD ? 3 : 0] * wy1[j] * wx1[j];
        }
        o[j] = finish<IN_U8, MODE>(v, ORD == 0, lut);
        rq[j] = fmin(fmax(ORD == 0 ? v : floor(v + 0.5), 0.0), 255.0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < NB; ++q) PCUDA_KEEP(pc[j][q]);      // (VMEM address rule, common.h)
      if (want_img) {
        float* po = a.img_out + ((long long)n * c + ch) * plane + dst;
        if (all_crop && a.vec_img) {
          *reinterpret_cast<f32x4*>(po) = f32x4{o[0], o[1], o[2], o[3]};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (in_crop[j]) po[j] = o[j];
        }
      }
      if (want_u8) {
        uint8_t* pu = a.img_u8_full + (((long long)n * h + y) * w + xg) * c + ch;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (valid[j]) pu[(long long)j * c] = (uint8_t)(int)rq[j];
      }
    }
  }

  const bool want_oh = any_crop && a.onehot;
  const bool want_full = a.fullmask || a.lab_full;
  if (a.lab && (want_oh || want_full)) {
    const int* labn = a.lab + (long long)n * h * w;
    const int* pl[4];
    int l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { pl[j] = labn + loff[j]; l[j] = *pl[j]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) l[j] = lin[j] ? l[j] : 0;
    if (want_oh) {
      const long long plane = (long long)a.oh * a.ow;
      uint8_t* po = a.onehot + (long long)n * a.k * plane + (long long)(y - a.y0) * a.ow + (xg - a.x0);
      for (int kk = 0; kk < a.k; ++kk, po += plane) {
        if (all_crop && a.vec_oh) {
          const uint32_t word = (uint32_t)(l[0] == kk) | ((uint32_t)(l[1] == kk) << 8) | ((uint32_t)(l[2] == kk) << 16) |
                                ((uint32_t)(l[3] == kk) << 24);
          *reinterpret_cast<uint32_t*>(po) = word;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (in_crop[j]) po[j] = (uint8_t)(l[j] == kk);
        }
      }
    }
    if (want_full) {
      const long long at = ((long long)n * h + y) * w + xg;
      if (a.fullmask) {
        if (all_valid && a.vec_mask && (at & 3) == 0) {
          const uint32_t word = (uint32_t)(l[0] > 0) | ((uint32_t)(l[1] > 0) << 8) | ((uint32_t)(l[2] > 0) << 16) |
                                ((uint32_t)(l[3] > 0) << 24);
          *reinterpret_cast<uint32_t*>(a.fullmask + at) = word;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (valid[j]) a.fullmask[at + j] = (uint8_t)(l[j] > 0);
        }
      }
      if (a.lab_full) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (valid[j]) a.lab_full[at + j] = l[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) PCUDA_KEEP(pl[j]);      // (VMEM address rule, common.h)
  }
}

// grid (tiles in x, tiles in y, sample): the inverse matrix, order and cval of the sample are wave-uniform (scalar loads,
// once per workgroup), and the branch on the order is wave-uniform too
template <bool IN_U8, int MODE>
__global__ __launch_bounds__(256) void augment_assemble_kernel(const AugArgs a) {
  const int n = blockIdx.z;
  float mn = 0.f, range = 0.f, rinv = 0.f;
  if (MODE == PCUDA_AUG_MINMAX) { mn = a.minmax[0]; range = a.minmax[1] - mn; rinv = 1.f / range; }
  // images = img_min + images.astype(np.float32) * (img_max - img_min) / 255.  |  np.array(x_batch, np.float32) / 255.
  __shared__ float lut[MODE == PCUDA_AUG_NONE ? 1 : 256];
  if (MODE != PCUDA_AUG_NONE) {
    const float r = (float)threadIdx.x;
    lut[threadIdx.x] = MODE == PCUDA_AUG_MINMAX ? mn + r * range / 255.f : r / 255.f;
    __syncthreads();
  }
  const int xg = a.rx0 + (blockIdx.x * (kTileW / 4) + (threadIdx.x & 15)) * 4;
  const int y = a.ry0 + blockIdx.y * kTileH + (threadIdx.x >> 4);
  if (xg >= a.rx1 || y >= a.ry1) return;
  const double* m = a.inv + 6 * n;
  const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  const int ord = a.order[n];
  int cv = a.cval[n];
  cv = cv < 0 ? 0 : (cv > 255 ? 255 : cv);
  if (ord != 0) augment_body<IN_U8, MODE, 1>(a, n, xg, y, m0, m1, m2, m3, m4, m5, cv, mn, range, rinv, lut);
  else augment_body<IN_U8, MODE, 0>(a, n, xg, y, m0, m1, m2, m3, m4, m5, cv, mn, range, rinv, lut);
}

}  // namespace

extern "C" size_t pcuda_minmax_workspace_size(void) { return (size_t)kMinMaxBlocks * 2 * sizeof(float); }

extern "C" int pcuda_minmax(const float* x, long long numel, float* out2, void* workspace, size_t workspace_bytes,
                            pcuda_stream_t s) {
  if (!x || !out2 || !workspace || numel <= 0) PCUDA_FAIL(PCUDA_E_BADARG, "minmax: bad arguments");
  if (workspace_bytes < pcuda_minmax_workspace_size()) PCUDA_FAIL(PCUDA_E_WORKSPACE, "minmax: workspace too small");
  const int vec = ((uintptr_t)x & 15) == 0;
  const long long per = vec ? 256ll * 4 * 4 : 256ll * 4;      // a few loads per lane before a block is worth launching
  const int blocks = (int)(cdiv(numel, per) > kMinMaxBlocks ? kMinMaxBlocks : cdiv(numel, per));
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)numel * 4.0, (hipStream_t)s);
  hipLaunchKernelGGL(minmax_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, x, numel, vec, (float*)workspace);
  PCUDA_CHECK_LAUNCH("minmax_kernel");
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (const float*)workspace, blocks, out2);
  PCUDA_CHECK_LAUNCH("minmax_final_kernel");
  return PCUDA_OK;
}

extern "C" int pcuda_quantize_u8(const float* x, long long numel, const float* minmax, uint8_t* q, pcuda_stream_t s) {
  if (!x || !minmax || !q || numel <= 0) PCUDA_FAIL(PCUDA_E_BADARG, "quantize_u8: bad arguments");
  const int vec = (((uintptr_t)x | (uintptr_t)q) & 15) == 0;
  const long long per = vec ? 256ll * kQuantPerLane : 256ll * 4;
  const long long want = (numel + per - 1) / per;
  const int blocks = (int)(want > kQuantBlocks ? kQuantBlocks : want);
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)numel * 5.0, (hipStream_t)s);
  hipLaunchKernelGGL(quantize_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, x, numel, vec, minmax, q);
  PCUDA_CHECK_LAUNCH("quantize_u8_kernel");
  return PCUDA_OK;
}

// the host side of both assemble entries: dequant = uint8 images through augment_assemble_kernel<true, PCUDA_AUG_MINMAX>
static int augment_assemble_run(const char* who, bool dequant, const void* images_hwc, int images_u8, const int* mask_labels,
                                int b, int h, int w, int c, int crop, int num_classes, const double* inv_mats, const int* order,
                                const int* cval, int rescale, const float* minmax, float* images_chw, uint8_t* onehot,
                                uint8_t* full_mask, int* labels_full, uint8_t* images_u8_full, pcuda_stream_t s) {
  if (!images_hwc || !inv_mats || !order || !cval) PCUDA_FAIL(PCUDA_E_BADARG, "%s: null pointer", who);
  if (!images_chw && !onehot && !full_mask && !labels_full && !images_u8_full)
    PCUDA_FAIL(PCUDA_E_BADARG, "%s: null pointer (no output)", who);
  if (b <= 0 || b > 65535 || h <= 0 || w <= 0 || c <= 0 || (long long)h * w * c >= (1ll << 31))
    PCUDA_FAIL(PCUDA_E_BADARG, "%s: bad dims", who);
  if ((onehot || full_mask || labels_full) && !mask_labels) PCUDA_FAIL(PCUDA_E_BADARG, "%s: null pointer (mask_labels)", who);
  if (onehot && num_classes < 2) PCUDA_FAIL(PCUDA_E_BADARG, "%s: num_classes < 2 with a one-hot output", who);
  if (dequant) {
    if (!minmax) PCUDA_FAIL(PCUDA_E_BADARG, "%s: null pointer (minmax)", who);
  } else {
    if (rescale != PCUDA_AUG_NONE && rescale != PCUDA_AUG_MINMAX && rescale != PCUDA_AUG_DIV255)
      PCUDA_FAIL(PCUDA_E_BADARG, "%s: bad rescale mode", who);
    if (rescale == PCUDA_AUG_MINMAX && (images_u8 || !minmax))
      PCUDA_FAIL(PCUDA_E_BADARG, "%s: the min-max rescale takes fp32 images and a device (min, max) pair", who);
  }
  if (rescale == PCUDA_AUG_DIV255 && !images_u8) PCUDA_FAIL(PCUDA_E_BADARG, "%s: the /255 rescale takes uint8 images", who);
  if (images_u8_full && !images_u8) PCUDA_FAIL(PCUDA_E_BADARG, "%s: a uint8 image output takes uint8 images", who);
  AugArgs a;
  memset(&a, 0, sizeof(a));
  a.y0 = 0; a.x0 = 0; a.oh = h; a.ow = w;
  if (crop > 0) {      // ImageProcessor.crop_volume(vol, crop_size = crop // 2), as pcuda_assemble_batch
    const int hc = crop / 2;
    a.y0 = h / 2 - hc; a.x0 = w / 2 - hc; a.oh = 2 * hc; a.ow = 2 * hc;
    if (a.y0 < 0 || a.x0 < 0 || a.y0 + a.oh > h || a.x0 + a.ow > w || hc <= 0)
      PCUDA_FAIL(PCUDA_E_BADARG, "%s: crop larger than the image", who);
  }
  a.img = images_hwc; a.lab = mask_labels; a.inv = inv_mats; a.order = order; a.cval = cval; a.minmax = minmax;
  a.img_out = images_chw; a.onehot = onehot; a.fullmask = full_mask; a.lab_full = labels_full; a.img_u8_full = images_u8_full;
  a.b = b; a.h = h; a.w = w; a.c = c; a.k = num_classes;
  const bool full = full_mask || labels_full || images_u8_full;
  if (full) {      // the whole image, in groups of four that start at multiples of four of the cropped row
    a.rx0 = a.x0 - 4 * ((a.x0 + 3) / 4); a.ry0 = 0; a.rx1 = w; a.ry1 = h;
  } else {
    a.rx0 = a.x0; a.ry0 = a.y0; a.rx1 = a.x0 + a.ow; a.ry1 = a.y0 + a.oh;
  }
  a.vec_img = (a.ow & 3) == 0 && ((uintptr_t)images_chw & 15) == 0;
  a.vec_oh = (a.ow & 3) == 0 && ((uintptr_t)onehot & 3) == 0;
  a.vec_mask = ((uintptr_t)full_mask & 3) == 0;
  const dim3 grid(cdiv(a.rx1 - a.rx0, kTileW), cdiv(a.ry1 - a.ry0, kTileH), b);
  const double out_pix = (double)b * a.oh * a.ow, all_pix = (double)b * (a.ry1 - a.ry0) * (a.rx1 - a.rx0);
  ProfScope prof(PCUDA_FAM_POINTWISE, out_pix * ((images_chw ? (images_u8 ? 5.0 : 8.0) * c : 0.0) + (onehot ? num_classes : 0.0)) +
                 all_pix * (mask_labels ? 4.0 : 0.0) + (full ? all_pix : 0.0), (hipStream_t)s);
#define PCUDA_AUG_LAUNCH(U8, MODE)                                                                                     \
  hipLaunchKernelGGL((augment_assemble_kernel<U8, MODE>), grid, dim3(256), 0, (hipStream_t)s, a)
  if (dequant) {
    PCUDA_AUG_LAUNCH(true, PCUDA_AUG_MINMAX);
  } else if (images_u8) {
    if (rescale == PCUDA_AUG_DIV255) PCUDA_AUG_LAUNCH(true, PCUDA_AUG_DIV255);
    else PCUDA_AUG_LAUNCH(true, PCUDA_AUG_NONE);
  } else {
    if (rescale == PCUDA_AUG_MINMAX) PCUDA_AUG_LAUNCH(false, PCUDA_AUG_MINMAX);
    else PCUDA_AUG_LAUNCH(false, PCUDA_AUG_NONE);
  }
#undef PCUDA_AUG_LAUNCH
  PCUDA_CHECK_LAUNCH("augment_assemble_kernel");
  return PCUDA_OK;
}

extern "C" int pcuda_augment_assemble(const void* images_hwc, int images_u8, const int* mask_labels, int b, int h, int w, int c,
                                      int crop, int num_classes, const double* inv_mats, const int* order, const int* cval,
                                      int rescale, const float* minmax, float* images_chw, uint8_t* onehot,
                                      uint8_t* full_mask, int* labels_full, uint8_t* images_u8_full, pcuda_stream_t s) {
  return augment_assemble_run("augment_assemble", false, images_hwc, images_u8, mask_labels, b, h, w, c, crop, num_classes, inv_mats,
                              order, cval, rescale, minmax, images_chw, onehot, full_mask, labels_full, images_u8_full, s);
}

// uint8 images that pcuda_quantize_u8 made (and the uint8 stages changed) back to fp32 behind the warp:
// images = img_min + images.astype(np.float32) * (img_max - img_min) / 255. (data_generator_mmwhs.py:254)
extern "C" int pcuda_augment_assemble_dequant(const uint8_t* images_hwc, const int* mask_labels, int b, int h, int w, int c, int crop,
                                              int num_classes, const double* inv_mats, const int* order, const int* cval,
                                              const float* minmax, float* images_chw, uint8_t* onehot, uint8_t* full_mask,
                                              int* labels_full, uint8_t* images_u8_full, pcuda_stream_t s) {
  return augment_assemble_run("augment_assemble_dequant", true, images_hwc, 1, mask_labels, b, h, w, c, crop, num_classes, inv_mats,
                              order, cval, PCUDA_AUG_MINMAX, minmax, images_chw, onehot, full_mask, labels_full, images_u8_full, s);
}
