// Native-size evaluation of MS-CMRSeg (evaluate_mscmrseg.py:139-145): resize_volume (utils/utils.py:83-92, cv2.resize INTER_AREA
// per fp32 plane) as pcuda_area_resize, and reconstuct_volume + the per-class resize + argmax in one pass as
// pcuda_reconstruct_resize_argmax.  The rule is stated in include/pcuda_hip.h and DESIGN.md f15; it is this build's own
// convention written after OpenCV's resize.cpp and its parity with OpenCV is not pinned.
//
// One kernel serves both entries and both regimes.  Per axis every output index has a run of source taps (start, count) and three
// fp32 weights (first, middle, last): the area table when both axes shrink, (sx, sx + 1) with (1 - fx, fx) otherwise, one tap
// of weight 1 where fx == 0.  out = sum over the rows in order of wy * (sum over the taps in order of wx * v), the first term
// of each sum assigned, every operation rounded on its own (-ffp-contract=off): 1 * v keeps v's bits, so equal sizes and
// integer enlargements copy.
//
// A block of 256 lanes makes a tile of 8 output rows x 256 output columns: lane l of wave w makes columns 4l .. 4l + 3 of rows
// w and w + 4.  The block builds the two tables for its tile in fp64 and keeps them in LDS (5.3 KB).  Where an axis enlarges,
// neighbouring outputs read the same source texels: the tile's source patch (at most 258 x 10 texels when both axes enlarge)
// is staged through LDS once per class, the zero canvas of the fused entry materialising there only, and read without tap loops
// (both rows and both columns at clamped addresses, the second term selected by the tap count: the same sums); a patch above PATCH_CAP
// texels (the linear rule with one axis shrinking hard) and the area regime, where a texel feeds at most two outputs per
// axis, read global memory through the window test instead.  The fused entry keeps the running maximum of its 8 pixels in
// registers over the classes and stores one dword of four labels per row; the planes and the canvas never reach memory.
#include <math.h>

#include "common.h"

namespace {

constexpr int TW = 256, TH = 8, NT = 256, PATCH_CAP = 4096, MAX_SIDE = 16384;

struct ResizeArgs {
  const float* in;
  long long sn, sc, sr;      // strides of the source in elements: image, class, row
  int c;                     // classes (1 for the plain resize)
  int x0, y0, w, h;          // the window of the virtual sh x sw source that the memory at `in` covers; zero outside
  int sh, sw, dh, dw;
  int area;                  // both axes shrink or stay: the area tables
  int vec;                   // rows of the output are aligned for the 4-pixel store
  void* out;
};

struct Plane {
  const float* p;
  long long sr;
  int x0, y0, w, h;
};

__device__ __forceinline__ float fetch(const Plane& P, int sy, int sx) {
  const unsigned ux = (unsigned)(sx - P.x0), uy = (unsigned)(sy - P.y0);
  if (ux >= (unsigned)P.w || uy >= (unsigned)P.h) return 0.f;
  const float* q = P.p + (long long)uy * P.sr + ux;
  const float v = *q;
  PCUDA_KEEP(q);      // VMEM address rule (common.h): the address outlives the load
  return v;
}

// the taps of output index d of an axis S -> D (d < D)
__device__ void build_taps(int d, int S, int D, int area, int& start, int& n, float& w0, float& wm, float& wl) {
  const double scale = (double)S / (double)D;
  if (area) {
    const double f1 = (double)d * scale, f2 = f1 + scale, cell = fmin(scale, (double)S - f1);
    int s1 = (int)ceil(f1);
    const int s2 = min((int)floor(f2), S - 1);
    s1 = min(s1, s2);
    const bool lead = ((double)s1 - f1) > 1e-3, trail = (f2 - (double)s2) > 1e-3;
    const float wlead = (float)(((double)s1 - f1) / cell), wfull = (float)(1.0 / cell),
                wtrail = (float)(fmin(fmin(f2 - (double)s2, 1.0), cell) / cell);
    const int full = s2 - s1;
    start = lead ? s1 - 1 : s1;
    n = (lead ? 1 : 0) + full + (trail ? 1 : 0);
    w0 = lead ? wlead : (full > 0 ? wfull : wtrail);
    wm = wfull;
    wl = trail ? wtrail : wfull;
  } else {
    const double inv = (double)D / (double)S;
    int sx = (int)floor((double)d * scale);
    double fx = (double)(d + 1) - (double)(sx + 1) * inv;
    fx = fx <= 0.0 ? 0.0 : fx - floor(fx);
    if (sx >= S - 1) { sx = S - 1; fx = 0.0; }
    start = sx;
    n = fx == 0.0 ? 1 : 2;
    w0 = (float)(1.0 - fx);
    wm = 0.f;
    wl = (float)fx;
  }
}

template <bool FUSED>
__global__ __launch_bounds__(NT) void area_resize_kernel(const ResizeArgs a) {
  __shared__ int xs[TW], xn[TW], ys[TH], yn[TH];
  __shared__ float xw0[TW], xwm[TW], xwl[TW], yw0[TH], ywm[TH], ywl[TH];
  __shared__ float patch[PATCH_CAP];
  const int tid = threadIdx.x, ox = blockIdx.x * TW, oy = blockIdx.y * TH, img = blockIdx.z;
  for (int i = tid; i < TW + TH; i += NT) {
    int start = 0, n = 0;
    float w0 = 0.f, wm = 0.f, wl = 0.f;
    if (i < TW) {
      if (ox + i < a.dw) build_taps(ox + i, a.sw, a.dw, a.area, start, n, w0, wm, wl);
      xs[i] = start; xn[i] = n; xw0[i] = w0; xwm[i] = wm; xwl[i] = wl;
    } else {
      const int r = i - TW;
      if (oy + r < a.dh) build_taps(oy + r, a.sh, a.dh, a.area, start, n, w0, wm, wl);
      ys[r] = start; yn[r] = n; yw0[r] = w0; ywm[r] = wm; ywl[r] = wl;
    }
  }
  __syncthreads();
  // the source patch of the tile under the linear rule: starts are monotone in d and a second tap exists below S - 1 only
  const int lastx = min(TW, a.dw - ox) - 1, lasty = min(TH, a.dh - oy) - 1;
  const int px0 = xs[0], py0 = ys[0];
  const int pw = min(xs[lastx] + 1, a.sw - 1) - px0 + 1, ph = min(ys[lasty] + 1, a.sh - 1) - py0 + 1;
  const bool staged = !a.area && (long long)pw * ph <= PATCH_CAP;

  const int wave = tid >> 6, col = (tid & 63) * 4;
  int cs[4], cn[4];
  float cw0[4], cwm[4], cwl[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cs[j] = xs[col + j]; cn[j] = xn[col + j]; cw0[j] = xw0[col + j]; cwm[j] = xwm[col + j]; cwl[j] = xwl[col + j];
  }
  float best[2][4];
  int bi[2][4];
  bool bad[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) { best[r][j] = 0.f; bi[r][j] = 0; bad[r][j] = false; }

  for (int k = 0; k < a.c; ++k) {
    Plane P = {a.in + (long long)img * a.sn + (long long)k * a.sc, a.sr, a.x0, a.y0, a.w, a.h};
    if (staged) {
      if (k) __syncthreads();                    // the last class's patch has been read
      for (int i = tid; i < pw * ph; i += NT) {
        const int py = i / pw, px = i - py * pw;
        patch[i] = fetch(P, py0 + py, px0 + px);
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int row = wave + 4 * r, ny = yn[row], sy0 = ys[row];
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      if (staged) {
        // at most two taps per axis: both rows and both columns are read, the second at a clamped patch address, and the
        // second term is selected by the tap count -- the sums of the general loop below without its trip counts
        const int y0 = min(max(sy0 - py0, 0), ph - 1), y1 = min(y0 + 1, ph - 1);
        const float b0 = yw0[row], b1 = ywl[row];
        const float *p0 = patch + y0 * pw, *p1 = patch + y1 * pw;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x0 = min(max(cs[j] - px0, 0), pw - 1), x1 = min(x0 + 1, pw - 1);
          const float t0 = cw0[j] * p0[x0], u0 = cwl[j] * p0[x1], t1 = cw0[j] * p1[x0], u1 = cwl[j] * p1[x1];
          const float h0 = cn[j] == 2 ? t0 + u0 : t0, h1 = cn[j] == 2 ? t1 + u1 : t1;
          const float q0 = b0 * h0, q1 = b1 * h1;
          acc[j] = ny == 2 ? q0 + q1 : q0;
        }
      } else {
        for (int ty = 0; ty < ny; ++ty) {
          const int sy = sy0 + ty;
          const float wy = ty == 0 ? yw0[row] : (ty == ny - 1 ? ywl[row] : ywm[row]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float h = 0.f;
            for (int tx = 0; tx < cn[j]; ++tx) {
              const float wx = tx == 0 ? cw0[j] : (tx == cn[j] - 1 ? cwl[j] : cwm[j]);
              const float t = wx * fetch(P, sy, cs[j] + tx);
              h = tx == 0 ? t : h + t;
            }
            const float q = wy * h;
            acc[j] = ty == 0 ? q : acc[j] + q;
          }
        }
      }
      if (FUSED) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = acc[j];
          bad[r][j] |= v != v;
          if (k == 0 || v > best[r][j]) { best[r][j] = v; bi[r][j] = k; }
        }
      } else if (ny > 0) {
        float* o = (float*)a.out + ((long long)img * a.dh + (oy + row)) * a.dw + ox + col;
        if (a.vec && cn[3] > 0) {
          *(f32x4*)o = f32x4{acc[0], acc[1], acc[2], acc[3]};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (cn[j] > 0) o[j] = acc[j];
        }
      }
    }
  }
  if (FUSED) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int row = wave + 4 * r;
      if (yn[row] <= 0) continue;
      uint8_t* o = (uint8_t*)a.out + ((long long)img * a.dh + (oy + row)) * a.dw + ox + col;
      uint32_t lab[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) lab[j] = bad[r][j] ? 0u : (uint32_t)bi[r][j];
      if (a.vec && cn[3] > 0) {
        *(uint32_t*)o = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (cn[j] > 0) o[j] = (uint8_t)lab[j];
      }
    }
  }
}

template <bool FUSED>
int launch(const ResizeArgs& a, int n, hipStream_t s, const char* name) {
  const dim3 grid(cdiv(a.dw, TW), cdiv(a.dh, TH), n);
  // the bytes the task must move: the source once, the output once
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)n * ((double)a.c * a.w * a.h * 4.0 + (double)a.dh * a.dw * (FUSED ? 1.0 : 4.0)), s);
  hipLaunchKernelGGL(area_resize_kernel<FUSED>, grid, dim3(NT), 0, s, a);
  PCUDA_CHECK_LAUNCH(name);
  return PCUDA_OK;
}

bool side_ok(int v) { return v >= 1 && v <= MAX_SIDE; }

}  // namespace

extern "C" int pcuda_area_resize(const float* in, long long sn, long long sr, int n, int sh, int sw, float* out, int dh, int dw,
                                 pcuda_stream_t s) {
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "area_resize: null pointer");
  if ((const void*)in == (const void*)out) PCUDA_FAIL(PCUDA_E_BADARG, "area_resize: in == out");
  if (!side_ok(sh) || !side_ok(sw) || !side_ok(dh) || !side_ok(dw))
    PCUDA_FAIL(PCUDA_E_BADARG, "area_resize: sizes %dx%d -> %dx%d outside 1..%d", sh, sw, dh, dw, MAX_SIDE);
  if (n < 0 || n > 65535) PCUDA_FAIL(PCUDA_E_BADARG, "area_resize: n = %d outside 0..65535", n);
  if (sr < sw || sn < 0 || (n > 1 && sn == 0)) PCUDA_FAIL(PCUDA_E_BADARG, "area_resize: strides sn = %lld, sr = %lld", sn, sr);
  if (n == 0) return PCUDA_OK;
  ResizeArgs a = {in, sn, 0, sr, 1, 0, 0, sw, sh, sh, sw, dh, dw, (sw >= dw && sh >= dh) ? 1 : 0,
                  (dw % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0, out};
  return launch<false>(a, n, (hipStream_t)s, "area_resize_kernel");
}

extern "C" int pcuda_reconstruct_resize_argmax(const float* logits, long long sn, long long sc, long long sr, int n, int c, int h,
                                               int w, int crop, int origin, uint8_t* labels, int dh, int dw, pcuda_stream_t s) {
  if (!logits || !labels) PCUDA_FAIL(PCUDA_E_BADARG, "reconstruct_resize_argmax: null pointer");
  if (c < 1 || c > 8) PCUDA_FAIL(PCUDA_E_BADARG, "reconstruct_resize_argmax: %d classes outside 1..8", c);
  if (!side_ok(origin) || !side_ok(dh) || !side_ok(dw))
    PCUDA_FAIL(PCUDA_E_BADARG, "reconstruct_resize_argmax: sizes %d -> %dx%d outside 1..%d", origin, dh, dw, MAX_SIDE);
  if (crop < 1 || origin / 2 - crop < 0 || origin / 2 + crop > origin)
    PCUDA_FAIL(PCUDA_E_BADARG, "reconstruct_resize_argmax: the window %d +- %d does not fit a canvas of %d", origin / 2, crop, origin);
  if (h != 2 * crop || w != 2 * crop)
    PCUDA_FAIL(PCUDA_E_BADARG, "reconstruct_resize_argmax: logits of %dx%d, the window is %dx%d", h, w, 2 * crop, 2 * crop);
  if (n < 0 || n > 65535) PCUDA_FAIL(PCUDA_E_BADARG, "reconstruct_resize_argmax: n = %d outside 0..65535", n);
  if (sr < w || sc < 0 || sn < 0 || (c > 1 && sc == 0) || (n > 1 && sn == 0))
    PCUDA_FAIL(PCUDA_E_BADARG, "reconstruct_resize_argmax: strides sn = %lld, sc = %lld, sr = %lld", sn, sc, sr);
  if (n == 0) return PCUDA_OK;
  const int o0 = origin / 2 - crop;
  ResizeArgs a = {logits, sn, sc, sr, c, o0, o0, w, h, origin, origin, dh, dw, (origin >= dw && origin >= dh) ? 1 : 0,
                  (dw % 4 == 0 && ((uintptr_t)labels & 3) == 0) ? 1 : 0, labels};
  return launch<true>(a, n, (hipStream_t)s, "reconstruct_resize_argmax_kernel");
}
