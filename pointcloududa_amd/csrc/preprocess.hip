// Device-side slice preparation of the MS-CMRSeg data: the reference's preprocess_volume
// (utils/read_nii_image.py:60-74: cv2.createCLAHE(clipLimit=2.0, tileGridSize=(4, 4)) on every uint8 slice) and the front of
// read_*_nii_save_png (:94-99: RescaleIntensity -> uint8, the nearest resize to 256, the centre crop to 224).
//
// Parity with OpenCV / ITK is unpinned: the convention (include/pcuda_hip.h, pcuda_clahe / pcuda_rescale_resize_crop_u8) is
// this build's own, written after OpenCV's clahe.cpp and ITK's RescaleIntensityImageFilter, and pinned by two independent
// restatements in tests/golden/preprocess.npz (scripts/make_preprocess_golden.py).
//
// CLAHE is two kernels.  clahe_lut_kernel: one workgroup of 256 lanes per (image, tile); the tile's pixels -- reflected
// (BORDER_REFLECT_101) by index where the extended image overhangs, no padded copy -- go into a 256-bin LDS histogram by
// integer atomics; lane i owns bin i from there on: the clip, the clipped total by wave reductions, the redistribution in
// closed form, an inclusive scan over the four waves, and one LUT byte to the workspace [n][ty][tx][256].
// clahe_apply_kernel: a workgroup stages its image's LUTs in LDS (tiles_x tiles_y 256 bytes, at most 64 KB) and blends a band
// of rows; a lane owns four neighbouring columns (one dword load, one dword store or three float4 stores when the width
// allows it), whose tile indices and weights it computes once, and walks down the band.  The blend is never contracted
// (-ffp-contract=off): the bits are those of the fp32 restatement.
// The rescale is three small kernels: the reduction cells are set, every lane reduces order-preserving 32-bit keys of its
// values (16 bytes per lane and load), every workgroup issues one integer atomic min and max, and a lane maps the source
// values of four neighbouring output pixels in double (one dword store where the row pitch allows it;
// PCUDA_PRE_U8_RAW: the map kernel alone, values as they are -- the reference's resize_volume / crop_volume on their own).
// Every LUT index is a byte value below 256 and every tile index is clamped into the grid before it is used; every
// in-flight load's address stays alive (PCUDA_KEEP, VMEM address rule, common.h).
#include <math.h>

#include "common.h"

namespace {

constexpr int kLutThreads = 256;
constexpr int kApplyThreads = 256;
constexpr int kApplyRows = 32;                 // rows of one image a workgroup of the apply kernel blends
constexpr int kMaxTiles = 16;

struct ClaheArgs {
  const uint8_t* in;          // [n][h][w]
  void* out;                  // uint8 [n][h][w] or fp32 [n][3][h][w]
  uint8_t* lut;               // [n][tiles_y][tiles_x][256] (workspace)
  int h, w, tiles_x, tiles_y, th, tw, clip;
  float lut_scale, inv_tw, inv_th;
};

__global__ __launch_bounds__(kLutThreads) void clahe_lut_kernel(const ClaheArgs a) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_tot[4], s_clipped[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = a.tiles_x * a.tiles_y;
  const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int h = a.h, w = a.w, th = a.th, tw = a.tw;
  const uint8_t* src = a.in + (long long)img * h * w;
  s_hist[tid] = 0;
  __syncthreads();
  const int npix = th * tw;
  for (int i = tid; i < npix; i += kLutThreads) {
    const int r = i / tw, c = i - r * tw;
    int y = ty * th + r, x = tx * tw + c;
    y = y < h ? y : 2 * h - 2 - y;                      // BORDER_REFLECT_101 (the host checked pad <= dim - 1)
    x = x < w ? x : 2 * w - 2 - x;
    y = y < 0 ? 0 : y;
    x = x < 0 ? 0 : x;
    const uint8_t* p = src + (long long)y * w + x;
    const unsigned v = *p;
    atomicAdd(&s_hist[v], 1u);
    PCUDA_KEEP(p);
  }
  __syncthreads();
  unsigned mine = s_hist[tid];
  if (a.clip > 0) {                                      // (uniform)
    const unsigned clip = (unsigned)a.clip;
    unsigned excess = mine > clip ? mine - clip : 0u;
    mine = mine > clip ? clip : mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) excess += __shfl_xor(excess, o, 64);
    if (lane == 0) s_clipped[wave] = excess;
    __syncthreads();
    const unsigned clipped = s_clipped[0] + s_clipped[1] + s_clipped[2] + s_clipped[3];
    const unsigned batch = clipped >> 8, residual = clipped - (batch << 8);
    mine += batch;
    if (residual != 0) {
      const unsigned step = 256u / residual;             // residual <= 255: step >= 1
      const unsigned k = (unsigned)tid / step;
      if (k * step == (unsigned)tid && k < residual) mine += 1u;
    }
  }
  unsigned incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_tot[wave] = incl;
  __syncthreads();
  for (int k = 0; k < wave; ++k) incl += s_tot[k];
  float f = rintf((float)incl * a.lut_scale);
  f = fminf(fmaxf(f, 0.0f), 255.0f);
  a.lut[((long long)img * tiles + tile) * 256 + tid] = (uint8_t)(int)f;
}

// tile indices (as LUT offsets) and weights of one coordinate
__device__ __forceinline__ void axis_terms(int x, float inv_t, int tiles, int& t1, int& t2, float& wa, float& wa1) {
  const float tf = (float)x * inv_t - 0.5f;
  const float fl = floorf(tf);
  int i1 = (int)fl;
  wa = tf - fl;
  wa1 = 1.0f - wa;
  int i2 = i1 + 1;
  i2 = i2 > tiles - 1 ? tiles - 1 : i2;
  i2 = i2 < 0 ? 0 : i2;
  i1 = i1 < 0 ? 0 : i1;
  i1 = i1 > tiles - 1 ? tiles - 1 : i1;
  t1 = i1;
  t2 = i2;
}

template <bool VEC, int OUT_MODE>
__global__ __launch_bounds__(kApplyThreads) void clahe_apply_kernel(const ClaheArgs a, const int bands) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lut[];   // [tiles_y][tiles_x][256]
  const int tid = threadIdx.x;
  const int tiles = a.tiles_x * a.tiles_y;
  const int img = blockIdx.x / bands, band = blockIdx.x - img * bands;
  const int h = a.h, w = a.w;
  {
    const uint32_t* g = reinterpret_cast<const uint32_t*>(a.lut + (long long)img * tiles * 256);   // (16-byte aligned workspace)
    uint32_t* l = reinterpret_cast<uint32_t*>(s_lut);
    for (int i = tid; i < tiles * 64; i += kApplyThreads) {
      const uint32_t* p = g + i;
      const uint32_t v = *p;
      l[i] = v;
      PCUDA_KEEP(p);
    }
  }
  __syncthreads();
  const int groups = (w + 3) >> 2;                       // four columns each
  const int gpb = groups < kApplyThreads ? groups : kApplyThreads;
  const int rows_per_pass = kApplyThreads / gpb;
  const int gx = tid % gpb, ry = tid / gpb;
  if (ry >= rows_per_pass) return;                       // (no barrier below)
  const int row0 = band * kApplyRows, row1 = row0 + kApplyRows < h ? row0 + kApplyRows : h;
  const uint8_t* src = a.in + (long long)img * h * w;
  for (int g = gx; g < groups; g += gpb) {
    const int x0 = g * 4;
    int o1[4], o2[4];
    float xa[4], xa1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int t1, t2;
      axis_terms(x0 + j, a.inv_tw, a.tiles_x, t1, t2, xa[j], xa1[j]);
      o1[j] = t1 * 256;
      o2[j] = t2 * 256;
    }
    for (int y = row0 + ry; y < row1; y += rows_per_pass) {
      int t1, t2;
      float ya, ya1;
      axis_terms(y, a.inv_th, a.tiles_y, t1, t2, ya, ya1);
      const uint8_t* lut1 = s_lut + t1 * a.tiles_x * 256;
      const uint8_t* lut2 = s_lut + t2 * a.tiles_x * 256;
      const long long at = (long long)y * w + x0;
      unsigned v[4];
      if (VEC) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(src + at);
        const uint32_t word = *p;
        v[0] = word & 255u; v[1] = (word >> 8) & 255u; v[2] = (word >> 16) & 255u; v[3] = word >> 24;
        PCUDA_KEEP(p);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint8_t* p = src + at + (x0 + j < w ? j : 0);
          v[j] = *p;
          PCUDA_KEEP(p);
        }
      }
      unsigned r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float l11 = (float)lut1[o1[j] + v[j]], l12 = (float)lut1[o2[j] + v[j]];
        const float l21 = (float)lut2[o1[j] + v[j]], l22 = (float)lut2[o2[j] + v[j]];
        const float top = l11 * xa1[j] + l12 * xa[j];
        const float bot = l21 * xa1[j] + l22 * xa[j];
        float res = top * ya1 + bot * ya;
        res = fminf(fmaxf(rintf(res), 0.0f), 255.0f);
        r[j] = (unsigned)(int)res;
      }
      if (OUT_MODE == PCUDA_CLAHE_U8) {
        uint8_t* dst = static_cast<uint8_t*>(a.out) + (long long)img * h * w + at;
        if (VEC) {
          *reinterpret_cast<uint32_t*>(dst) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x0 + j < w) dst[j] = (uint8_t)r[j];
        }
      } else {
        float* dst = static_cast<float*>(a.out) + (long long)img * 3 * h * w + at;
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = (float)r[j] / 255.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          float* d = dst + (long long)ch * h * w;
          if (VEC) {
            *reinterpret_cast<f32x4*>(d) = f32x4{f[0], f[1], f[2], f[3]};
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (x0 + j < w) d[j] = f[j];
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// rescale -> nearest resize -> centre crop
// ------------------------------------------------------------------------------------------
struct RescaleArgs {
  const void* in;             // [n][sh][sw] of in_dtype
  uint8_t* out;               // [n][oh][ow]
  uint32_t* cells;            // workspace: [0] the smallest key, [1] the largest
  long long total;            // n sh sw
  int dtype, n, sh, sw, oh, ow, y0, x0;
  double ify, ifx;
};

// an order-preserving 32-bit key of a value (fp32: -0.0 -> +0.0, then as the sort keys of histmatch.hip) and its inverse
__device__ __forceinline__ uint32_t f32_key(uint32_t u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
template <int DT>
__device__ __forceinline__ uint32_t load_key(const void* base, long long i) {
  if (DT == PCUDA_PRE_F32) {
    const uint32_t* p = static_cast<const uint32_t*>(base) + i;
    const uint32_t u = *p;
    PCUDA_KEEP(p);
    return f32_key(u);
  } else if (DT == PCUDA_PRE_I16) {
    const int16_t* p = static_cast<const int16_t*>(base) + i;
    const int v = *p;
    PCUDA_KEEP(p);
    return (uint32_t)(v + 32768);
  } else {
    const uint8_t* p = static_cast<const uint8_t*>(base) + i;
    const uint32_t v = *p;
    PCUDA_KEEP(p);
    return v;
  }
}
template <int DT>
__device__ __forceinline__ double key_value(uint32_t key) {
  if (DT == PCUDA_PRE_F32) {
    const uint32_t u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    return (double)__builtin_bit_cast(float, u);
  } else if (DT == PCUDA_PRE_I16) {
    return (double)((int)key - 32768);
  } else {
    return (double)key;
  }
}
__device__ __forceinline__ void fold(uint32_t k, uint32_t& lo, uint32_t& hi) {
  lo = k < lo ? k : lo;
  hi = k > hi ? k : hi;
}
// the keys of the one, two or four values of a 32-bit word
template <int DT>
__device__ __forceinline__ void fold_word(uint32_t w, uint32_t& lo, uint32_t& hi) {
  if (DT == PCUDA_PRE_F32) {
    fold(f32_key(w), lo, hi);
  } else if (DT == PCUDA_PRE_I16) {
    fold((uint32_t)((int)(int16_t)(w & 0xffffu) + 32768), lo, hi);
    fold((uint32_t)((int)(int16_t)(w >> 16) + 32768), lo, hi);
  } else {
    fold(w & 255u, lo, hi); fold((w >> 8) & 255u, lo, hi); fold((w >> 16) & 255u, lo, hi); fold(w >> 24, lo, hi);
  }
}

__global__ void rescale_init_kernel(uint32_t* cells) {
  if (threadIdx.x == 0) {
    cells[0] = 0xffffffffu;
    cells[1] = 0u;
  }
}

// `wide`: the volume starts on a 16-byte boundary: 16 bytes per lane and load, the tail value by value
template <int DT>
__global__ __launch_bounds__(256) void rescale_minmax_kernel(const RescaleArgs a, const int wide) {
  constexpr int kPer = DT == PCUDA_PRE_F32 ? 4 : DT == PCUDA_PRE_I16 ? 8 : 16;      // values in 16 bytes
  const long long stride = (long long)gridDim.x * 256;
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nvec = wide ? a.total / kPer : 0;
  uint32_t lo = 0xffffffffu, hi = 0u;
  const uint4* vbase = static_cast<const uint4*>(a.in);
  for (long long i = first; i < nvec; i += stride) {
    const uint4* p = vbase + i;
    const uint4 q = *p;
    fold_word<DT>(q.x, lo, hi); fold_word<DT>(q.y, lo, hi); fold_word<DT>(q.z, lo, hi); fold_word<DT>(q.w, lo, hi);
    PCUDA_KEEP(p);
  }
  for (long long i = nvec * kPer + first; i < a.total; i += stride) fold(load_key<DT>(a.in, i), lo, hi);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  // one pair of atomics per workgroup: they all land on the same two cells and are served one after the other
  __shared__ uint32_t s_lo[4], s_hi[4];
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      lo = s_lo[k] < lo ? s_lo[k] : lo;
      hi = s_hi[k] > hi ? s_hi[k] : hi;
    }
    if (lo <= hi) {                                      // (a workgroup that saw no value has lo > hi)
      atomicMin(a.cells, lo);
      atomicMax(a.cells + 1, hi);
    }
  }
}

// a lane owns four neighbouring output pixels of a row: four gathered source values, one dword store where the row
// pitch and the pointer allow it (VEC)
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void rescale_map_kernel(const RescaleArgs a, const uint32_t* __restrict__ cells) {
  const int groups = (a.ow + 3) >> 2;
  const long long per = (long long)a.oh * groups;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= per * a.n) return;
  const int img = (int)(e / per);
  const int rem = (int)(e - (long long)img * per);
  const int oy = rem / groups, ox0 = (rem - oy * groups) * 4;
  int sy = (int)floor((double)(oy + a.y0) * a.ify);
  sy = sy > a.sh - 1 ? a.sh - 1 : sy;
  sy = sy < 0 ? 0 : sy;
  const long long row = ((long long)img * a.sh + sy) * a.sw;
  uint32_t key[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = ox0 + j < a.ow ? ox0 + j : a.ow - 1;  // (a ragged last group reads its last pixel again)
    int sx = (int)floor((double)(ox + a.x0) * a.ifx);
    sx = sx > a.sw - 1 ? a.sw - 1 : sx;
    sx = sx < 0 ? 0 : sx;
    key[j] = load_key<DT>(a.in, row + sx);
  }
  uint32_t r[4];
  if (DT == PCUDA_PRE_U8_RAW) {                          // the values as they are: no rescale, the cells are not read
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = key[j];
  } else {
    const uint32_t klo = cells[0], khi = cells[1];       // (uniform: the compiler reads them with one scalar load)
    const double lo = key_value<DT>(klo), hi = key_value<DT>(khi);
    double scale;
    if (hi != lo) scale = 255.0 / (hi - lo);
    else if (hi != 0.0) scale = 255.0 / hi;
    else scale = 0.0;
    const double shift = -lo * scale;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = trunc(key_value<DT>(key[j]) * scale + shift);
      v = fmin(fmax(v, 0.0), 255.0);
      r[j] = (uint32_t)(int)v;
    }
  }
  uint8_t* dst = a.out + ((long long)img * a.oh + oy) * a.ow + ox0;
  if (VEC) {
    *reinterpret_cast<uint32_t*>(dst) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ox0 + j < a.ow) dst[j] = (uint8_t)r[j];
  }
}


template <int DT>
int launch_rescale(const RescaleArgs& a, hipStream_t s) {
  if constexpr (DT != PCUDA_PRE_U8_RAW) {
    hipLaunchKernelGGL(rescale_init_kernel, dim3(1), dim3(64), 0, s, a.cells);
    PCUDA_CHECK_LAUNCH("rescale_init_kernel");
    const int wide = ((uintptr_t)a.in & 15) == 0;
    const double bytes = (double)a.total * (DT == PCUDA_PRE_F32 ? 4.0 : DT == PCUDA_PRE_I16 ? 2.0 : 1.0);
    const long long want = (long long)(bytes / (256.0 * 16.0 * 4.0)) + 1;      // four 16-byte loads per lane, at least
    hipLaunchKernelGGL(rescale_minmax_kernel<DT>, dim3((unsigned)(want > 512 ? 512 : want)), dim3(256), 0, s, a, wide);
    PCUDA_CHECK_LAUNCH("rescale_minmax_kernel");
  }
  const dim3 grid(cdiv((long long)a.n * a.oh * ((a.ow + 3) >> 2), 256));
  const uint32_t* cells = a.cells;
  if (a.ow % 4 == 0 && ((uintptr_t)a.out & 3) == 0) hipLaunchKernelGGL((rescale_map_kernel<DT, true>), grid, dim3(256), 0, s, a, cells);
  else hipLaunchKernelGGL((rescale_map_kernel<DT, false>), grid, dim3(256), 0, s, a, cells);
  PCUDA_CHECK_LAUNCH("rescale_map_kernel");
  return PCUDA_OK;
}

}  // namespace

extern "C" size_t pcuda_clahe_workspace_size(int n, int tiles_x, int tiles_y) {
  if (n <= 0 || tiles_x < 1 || tiles_y < 1 || tiles_x > kMaxTiles || tiles_y > kMaxTiles) return 0;
  return round16((size_t)n * tiles_x * tiles_y * 256);
}

extern "C" int pcuda_clahe(const uint8_t* in, void* out, int n, int h, int w, double clip_limit, int tiles_x, int tiles_y,
                           int out_mode, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (tiles_x < 1 || tiles_y < 1 || tiles_x > kMaxTiles || tiles_y > kMaxTiles)
    PCUDA_FAIL(PCUDA_E_BADARG, "clahe: 1..16 tiles per axis");
  if (n < 0 || h < 2 || w < 2 || h > 32768 || w > 32768) PCUDA_FAIL(PCUDA_E_BADARG, "clahe: bad dims (sides 2..32768)");
  if (out_mode != PCUDA_CLAHE_U8 && out_mode != PCUDA_CLAHE_F32X3) PCUDA_FAIL(PCUDA_E_BADARG, "clahe: unknown out_mode");
  if (!(clip_limit == clip_limit)) PCUDA_FAIL(PCUDA_E_BADARG, "clahe: clip_limit is NaN");
  int eh = h, ew = w;
  if (w % tiles_x != 0 || h % tiles_y != 0) {              // (OpenCV's quirk: both axes grow)
    eh = h + (tiles_y - h % tiles_y);
    ew = w + (tiles_x - w % tiles_x);
  }
  if (eh - h > h - 1 || ew - w > w - 1) PCUDA_FAIL(PCUDA_E_BADARG, "clahe: the reflected border is wider than the image");
  const int th = eh / tiles_y, tw = ew / tiles_x;
  const long long T = (long long)th * tw;
  if (T >= (1ll << 24)) PCUDA_FAIL(PCUDA_E_BADARG, "clahe: a tile of 2^24 pixels or more");
  if (n == 0) return PCUDA_OK;
  const int tiles = tiles_x * tiles_y;
  const int bands = (h + kApplyRows - 1) / kApplyRows;
  if ((long long)n * tiles >= (1ll << 31) || (long long)n * bands >= (1ll << 31)) PCUDA_FAIL(PCUDA_E_BADARG, "clahe: batch too large");
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "clahe: null pointer");
  if ((const void*)in == (const void*)out) PCUDA_FAIL(PCUDA_E_BADARG, "clahe: in == out (the input is never written)");
  const size_t need = pcuda_clahe_workspace_size(n, tiles_x, tiles_y);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "clahe: workspace too small (or not 16-byte aligned)");
  ClaheArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.lut = static_cast<uint8_t*>(workspace);
  a.h = h; a.w = w; a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.th = th; a.tw = tw;
  if (clip_limit > 0.0) {
    const double c = clip_limit * (double)T / 256.0;
    a.clip = c >= 2147483647.0 ? 2147483647 : (int)c;
    if (a.clip < 1) a.clip = 1;
  }
  a.lut_scale = 255.0f / (float)T;
  a.inv_tw = 1.0f / (float)tw;
  a.inv_th = 1.0f / (float)th;
  hipStream_t st = (hipStream_t)s;
  const size_t pixels = (size_t)n * h * w;
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)pixels * (out_mode == PCUDA_CLAHE_U8 ? 3.0 : 14.0), st);
  hipLaunchKernelGGL(clahe_lut_kernel, dim3(n * tiles), dim3(kLutThreads), 0, st, a);
  PCUDA_CHECK_LAUNCH("clahe_lut_kernel");
  const bool vec = (w % 4 == 0) && ((uintptr_t)in & 3) == 0 && ((uintptr_t)out & 15) == 0;
  const dim3 grid(n * bands), block(kApplyThreads);
  const size_t lds = (size_t)tiles * 256;
  if (out_mode == PCUDA_CLAHE_U8) {
    if (vec) hipLaunchKernelGGL((clahe_apply_kernel<true, PCUDA_CLAHE_U8>), grid, block, lds, st, a, bands);
    else hipLaunchKernelGGL((clahe_apply_kernel<false, PCUDA_CLAHE_U8>), grid, block, lds, st, a, bands);
  } else {
    if (vec) hipLaunchKernelGGL((clahe_apply_kernel<true, PCUDA_CLAHE_F32X3>), grid, block, lds, st, a, bands);
    else hipLaunchKernelGGL((clahe_apply_kernel<false, PCUDA_CLAHE_F32X3>), grid, block, lds, st, a, bands);
  }
  PCUDA_CHECK_LAUNCH("clahe_apply_kernel");
  return PCUDA_OK;
}

extern "C" size_t pcuda_rescale_resize_crop_u8_workspace_size(void) { return 16; }

extern "C" int pcuda_rescale_resize_crop_u8(const void* in, int in_dtype, int n, int sh, int sw, int resize_h, int resize_w,
                                            int crop, uint8_t* out, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (in_dtype != PCUDA_PRE_F32 && in_dtype != PCUDA_PRE_I16 && in_dtype != PCUDA_PRE_U8 && in_dtype != PCUDA_PRE_U8_RAW)
    PCUDA_FAIL(PCUDA_E_BADARG, "rescale_resize_crop_u8: in_dtype is fp32, int16, uint8 or raw uint8");
  if (n < 0 || sh < 1 || sw < 1 || resize_h < 1 || resize_w < 1 || sh > 32768 || sw > 32768 || resize_h > 32768 ||
      resize_w > 32768 || crop < 0)
    PCUDA_FAIL(PCUDA_E_BADARG, "rescale_resize_crop_u8: bad dims (sides 1..32768, crop >= 0)");
  const int half = crop / 2;
  int oh = resize_h, ow = resize_w, y0 = 0, x0 = 0;
  if (crop > 0) {
    y0 = resize_h / 2 - half; x0 = resize_w / 2 - half;
    oh = ow = 2 * half;
    if (half < 1 || y0 < 0 || x0 < 0 || y0 + oh > resize_h || x0 + ow > resize_w)
      PCUDA_FAIL(PCUDA_E_BADARG, "rescale_resize_crop_u8: the crop window leaves the resized slice");
  }
  if (n == 0) return PCUDA_OK;
  if ((long long)n * sh * sw >= (1ll << 40) || (long long)n * oh * ow >= (1ll << 31) * 256)
    PCUDA_FAIL(PCUDA_E_BADARG, "rescale_resize_crop_u8: volume too large");
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "rescale_resize_crop_u8: null pointer");
  if (in == (const void*)out) PCUDA_FAIL(PCUDA_E_BADARG, "rescale_resize_crop_u8: in == out (the input is never written)");
  if (!workspace || workspace_bytes < pcuda_rescale_resize_crop_u8_workspace_size() || ((uintptr_t)workspace & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "rescale_resize_crop_u8: workspace too small (or not 16-byte aligned)");
  RescaleArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.cells = static_cast<uint32_t*>(workspace);
  a.total = (long long)n * sh * sw;
  a.dtype = in_dtype; a.n = n; a.sh = sh; a.sw = sw; a.oh = oh; a.ow = ow; a.y0 = y0; a.x0 = x0;
  a.ify = 1.0 / ((double)resize_h / (double)sh);
  a.ifx = 1.0 / ((double)resize_w / (double)sw);
  hipStream_t st = (hipStream_t)s;
  const double bytes = (double)a.total * (in_dtype == PCUDA_PRE_F32 ? 4.0 : in_dtype == PCUDA_PRE_I16 ? 2.0 : 1.0) + (double)n * oh * ow * 2.0;
  ProfScope prof(PCUDA_FAM_POINTWISE, bytes, st);
  if (in_dtype == PCUDA_PRE_F32) return launch_rescale<PCUDA_PRE_F32>(a, st);
  if (in_dtype == PCUDA_PRE_I16) return launch_rescale<PCUDA_PRE_I16>(a, st);
  if (in_dtype == PCUDA_PRE_U8) return launch_rescale<PCUDA_PRE_U8>(a, st);
  return launch_rescale<PCUDA_PRE_U8_RAW>(a, st);
}
