// Device-side geometric augmentation of the loader path: the warps of the reference's default
// recipe ImageProcessor.augmentation (data_generator_mscmrseg.py:20-84: Fliplr, Flipud, CropAndPad, Affine over the heavy
// ranges with every border mode, ElasticTransformation, PiecewiseAffine, PerspectiveTransform) on uint8 [B,H,W,C] images
// and int32 [B,H,W] labels, as a per-sample PROGRAM of up to eight slots that lives in device memory (f7's shape, with
// 32 float64 arguments per slot).
//
// Convention (this build's own: imgaug / skimage / cv2 are not vendored by the reference, parity is unpinned; pinned
// against a scipy map_coordinates and a plain-numpy restatement by tests/golden/geometric.npz):
//   * every slot is one resampling: a source coordinate (sx, sy) per output pixel (x, y) in float64 (the library is built
//     with -ffp-contract=off), then one sample; the value is uint8 again between two slots
//   * order 0 takes the texel at floor(s + 0.5); order 1 is bilinear over (floor(s), floor(s) + 1) in f6's order
//     (v = 0; v += ((p * wy) * wx) for the neighbours row-major), floor(v + 0.5) clipped to [0, 255]
//   * order 3 (pcuda_geometric_cubic only; pcuda_geometric samples it as order 1): Keys cubic convolution, A = -0.75, over
//     floor(s) - 1 .. floor(s) + 2 per axis with imgdev::cubic_weights of s - floor(s); a row is summed left to right
//     (((p0 wx0 + p1 wx1) + p2 wx2) + p3 wx3), then the rows top to bottom likewise, floor(v + 0.5) clipped to [0, 255]
//   * border mode per neighbour INDEX, folded in integers: 0 constant (cval), 1 edge, 2 reflect without repeating the edge
//     (period 2 (n - 1)), 3 symmetric (period 2 n), 4 wrap (period n); anything else behaves as 0
//   * labels take order 0 and constant 0 at the same coordinate whatever the image's order, mode and cval are
//   * a NaN coordinate or one with |s| > 2^30 takes cval (labels: 0) in every mode
//   * HOMOGRAPHY   farg[0..8] = h: d = (h6 x + h7 y) + h8, sx = ((h0 x + h1 y) + h2) / d, sy = ((h3 x + h4 y) + h5) / d
//   * ELASTIC      iarg[3] = r in 0..4, farg[0] = alpha, farg[1..1+r] = one-sided weights w[0..r]; noise n_k(p) = 2 u - 1,
//                  u = (word_k + 0.5) 2^-32 of f7's Philox4x32-10 (key = the slot's seed, counter = y W + x; word 0: dx,
//                  word 1: dy), outside the image the noise of the reflect-101 pixel; blur along y, then along x on the
//                  unrounded values (t = n[0] w[0]; d = r..1: t += (n[-d] + n[+d]) w[d]); sx = x + alpha bx, sy = y + alpha by
//   * PIECEWISE_AFFINE  iarg[3] = G in 2..4, farg[i G + j] / farg[16 + i G + j] = source x / y of control point (i, j);
//                  cell j = min((x (G-1)) / (W-1), G-2) in integers, u = (x (G-1) - j (W-1)) / (W-1) (one division, the
//                  numerator is an integer), i and v likewise from y and H; u >= v:
//                  (P_TL + u (P_TR - P_TL)) + v (P_BR - P_TR), otherwise (P_TL + u (P_BR - P_BL)) + v (P_BL - P_TL)
//
// One launch per slot over (tile, sample); a tile is 16 rows x 64 pixels, a lane owns four consecutive pixels and stores
// their bytes as 32-bit words.  The sample's opcode and arguments are read once per workgroup (scalar loads and a 32-entry
// LDS table), so every branch on them is wave-uniform.  The elastic slot stages the Philox words of its tile plus an
// r-pixel halo in LDS once.  The slots ping-pong between the caller's output and the caller's workspace.  Every gather
// index is folded or clamped into the image in integers BEFORE the load (a garbage program reads wrong texels, never out
// of bounds), an unknown opcode copies, and every in-flight load's address stays alive behind the code that consumes the
// data (PCUDA_KEEP, VMEM address rule, common.h).
#include "common.h"
#include "image_device.h"

namespace {

enum { OP_NOP = 0, OP_HOMOGRAPHY = 1, OP_ELASTIC = 2, OP_PIECEWISE = 3 };
enum { M_CONSTANT = 0, M_EDGE = 1, M_REFLECT = 2, M_SYMMETRIC = 3, M_WRAP = 4 };

constexpr int kMaxSlots = 8, kIArgs = 4, kFArgs = 32, kMaxC = 4;
constexpr int kTileW = 64, kTileH = 16;
constexpr int kMaxR = 4;                                  // the elastic blur's largest radius
constexpr int kStageW = kTileW + 2 * kMaxR, kStageH = kTileH + 2 * kMaxR;
constexpr double kCoordLimit = 1073741824.0;              // 2^30

struct GeoArgs {
  const uint8_t* in;         // [b][h][w][c]
  uint8_t* out;              // [b][h][w][c]
  const int* lab_in;         // [b][h][w] (may be null together with lab_out)
  int* lab_out;
  const int* opcode;         // [b][slots]
  const int* iarg;           // [b][slots][4]
  const double* farg;        // [b][slots][32]
  const uint32_t* seed;      // [b][slots][2] (low, high word)
  int h, w, c, slots;
  int slot;                  // the slot this launch runs; < 0: copy
  int vec_out, vec_lab;      // 4-byte image stores / 16-byte label stores are aligned
};

using imgdev::clampi;
// imgdev::round_u8 in a 32-bit word, as the packed store takes it (the uint8_t form costs a mask here)
__device__ __forceinline__ uint32_t round_u8_word(double v) {
  const double r = fmin(fmax(floor(v + 0.5), 0.0), 255.0);      // (fmax returns the other operand for a NaN: 0)
  return (uint32_t)(int)r;
}

// the texel index a neighbour index reads in a border mode, always inside [0, n); n >= 2.  Constant (and any unknown
// mode): `inside` tells whether the neighbour contributes its texel or cval
__device__ __forceinline__ int fold(int i, int n, int mode, bool& inside) {
  inside = true;
  if ((unsigned)i < (unsigned)n) return i;
  if (mode == M_EDGE) return i < 0 ? 0 : n - 1;
  if (mode == M_REFLECT) {
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
  }
  if (mode == M_SYMMETRIC) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
  }
  if (mode == M_WRAP) {
    i %= n;
    return i < 0 ? i + n : i;
  }
  inside = false;
  return i < 0 ? 0 : n - 1;
}

// Philox4x32-10 as photometric.hip implements it: ten rounds, the key bumped between rounds; words 0 and 1
__device__ __forceinline__ void philox2(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t& w0, uint32_t& w1) {
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w0 = c0; w1 = c1;
}
__device__ __forceinline__ double noise_of(uint32_t word) { return 2.0 * (((double)word + 0.5) * 0x1p-32) - 1.0; }
__device__ __forceinline__ int reflect101(int i, int n) {      // np.pad "reflect" for any i; n >= 2
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// four consecutive pixels (xg .. xg + 3, row y) of sample n sampled at (sx[j], sy[j]) and stored
template <int ORD>
__device__ __forceinline__ void sample_store(const GeoArgs& a, int n, int xg, int y, const double (&sx)[4], const double (&sy)[4],
                                             int mode, int cv) {
  constexpr int NB = ORD ? 4 : 1;
  const int h = a.h, w = a.w, c = a.c;
  const uint8_t* src = a.in + (long long)n * h * w * c;
  const int* labn = a.lab_in ? a.lab_in + (long long)n * h * w : nullptr;
  uint32_t words[4] = {0u, 0u, 0u, 0u};
  int labv[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (xg + j >= w) continue;
    double cx = sx[j], cy = sy[j];
    const bool bad = !(fabs(cx) <= kCoordLimit) || !(fabs(cy) <= kCoordLimit);      // (a NaN is bad too)
    if (bad) { cx = 0.0; cy = 0.0; }
    const int xn = (int)floor(cx + 0.5), yn = (int)floor(cy + 0.5);
    if (labn) {
      const bool lin = !bad && xn >= 0 && xn < w && yn >= 0 && yn < h;
      const int* pl = labn + (clampi(yn, 0, h - 1) * w + clampi(xn, 0, w - 1));
      const int l = *pl;
      labv[j] = lin ? l : 0;
      PCUDA_KEEP(pl);
    }
    if constexpr (ORD == 3) {
      // Keys cubic over the 4 x 4 neighbours (floor(s) - 1 .. floor(s) + 2 per axis): the border mode folds each of the
      // eight indices, a row is summed left to right, then the four rows top to bottom
      const double xf = floor(cx), yf = floor(cy);
      double wx[4], wy[4];
      imgdev::cubic_weights(cx - xf, wx);
      imgdev::cubic_weights(cy - yf, wy);
      const int xa = (int)xf - 1, ya = (int)yf - 1;
      int fx[4], fy[4];
      bool ix[4], iy[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        fx[q] = fold(xa + q, w, mode, ix[q]) * c;
        fy[q] = fold(ya + q, h, mode, iy[q]) * w * c;
        ix[q] = ix[q] && !bad;
      }
#pragma unroll
      for (int ch = 0; ch < kMaxC; ++ch) {
        if (ch >= c) break;
        double rows[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint8_t* pc[4];
          double p[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            pc[q] = src + (fy[k] + fx[q] + ch);
            const uint8_t t = *pc[q];
            p[q] = (ix[q] && iy[k]) ? (double)t : (double)cv;
          }
          rows[k] = ((p[0] * wx[0] + p[1] * wx[1]) + p[2] * wx[2]) + p[3] * wx[3];
#pragma unroll
          for (int q = 0; q < 4; ++q) PCUDA_KEEP(pc[q]);      // (VMEM address rule, common.h)
        }
        const double v = ((rows[0] * wy[0] + rows[1] * wy[1]) + rows[2] * wy[2]) + rows[3] * wy[3];
        const int e = j * c + ch;
        words[e >> 2] |= round_u8_word(v) << (8 * (e & 3));
      }
      continue;
    }
    const uint8_t* pt[NB];
    bool tin[NB];
    double wx1 = 0.0, wy1 = 0.0;
    if (ORD == 0) {
      bool ix, iy;
      const int fx = fold(xn, w, mode, ix), fy = fold(yn, h, mode, iy);
      tin[0] = ix && iy && !bad;
      pt[0] = src + (long long)(fy * w + fx) * c;
    } else {
      const double xf = floor(cx), yf = floor(cy);
      wx1 = cx - xf; wy1 = cy - yf;
      const int xa = (int)xf, ya = (int)yf;
      bool ix[2], iy[2];
      const int fx[2] = {fold(xa, w, mode, ix[0]), fold(xa + 1, w, mode, ix[1])};
      const int fy[2] = {fold(ya, h, mode, iy[0]), fold(ya + 1, h, mode, iy[1])};
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        tin[q] = ix[q & 1] && iy[q >> 1] && !bad;
        pt[q] = src + (long long)(fy[q >> 1] * w + fx[q & 1]) * c;
      }
    }
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch) {
      if (ch >= c) break;
      const uint8_t* pc[NB];
      double p[NB];
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        pc[q] = pt[q] + ch;
        const uint8_t t = *pc[q];
        p[q] = tin[q] ? (double)t : (double)cv;
      }
      uint32_t res;
      if (ORD == 0) {
        res = (uint32_t)(int)p[0];
      } else {
        const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
        double v = 0.0;
        v += p[0] * wy0 * wx0;
        v += p[ORD ? 1 : 0] * wy0 * wx1;
        v += p[ORD ? 2 : 0] * wy1 * wx0;
        v += p[ORD ? 3 : 0] * wy1 * wx1;
        res = round_u8_word(v);
      }
      const int e = j * c + ch;
      words[e >> 2] |= res << (8 * (e & 3));
#pragma unroll
      for (int q = 0; q < NB; ++q) PCUDA_KEEP(pc[q]);      // (VMEM address rule, common.h)
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

// CUBIC: order 3 samples cubically (the instance behind pcuda_geometric_cubic); without it order 3 samples as order 1 and
// the kernel is the one pcuda_geometric has always launched, register for register
template <bool CUBIC>
__global__ __launch_bounds__(256) void geometric_kernel(const GeoArgs a) {
  __shared__ double s_f[kFArgs];
  __shared__ uint32_t s_seed[2];
  __shared__ uint32_t s_noise[2][kStageH * kStageW];      // 13824 B: the Philox words, dx and dy
  __shared__ double s_mid[2][kTileH * kStageW];           // 18432 B: the blur along y, unrounded

  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const int h = a.h, w = a.w;
  const int tiles_x = (w + kTileW - 1) / kTileW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int at = a.slot < 0 ? 0 : n * a.slots + a.slot;
  int op = OP_NOP, order = 0, mode = M_CONSTANT, cv = 0, ia3 = 0;
  if (a.slot >= 0) {
    op = a.opcode[at];
    const int* ia = a.iarg + at * kIArgs;
    order = ia[0]; mode = ia[1]; cv = clampi(ia[2], 0, 255); ia3 = ia[3];
    if (tid < kFArgs) {
      const double* p = a.farg + at * kFArgs + tid;
      s_f[tid] = *p;
      PCUDA_KEEP(p);
    } else if (tid < kFArgs + 2) {
      const uint32_t* p = a.seed + 2 * at + (tid - kFArgs);
      s_seed[tid - kFArgs] = *p;
      PCUDA_KEEP(p);
    }
    __syncthreads();
  }
  if (op < OP_HOMOGRAPHY || op > OP_PIECEWISE) { op = OP_NOP; order = 0; mode = M_CONSTANT; }      // copy

  const int r = clampi(ia3, 0, kMaxR);
  const int sw = kTileW + 2 * r;
  if (op == OP_ELASTIC) {      // (wave-uniform: the barriers inside are reached by every lane of the workgroup)
    const uint32_t k0 = s_seed[0], k1 = s_seed[1];
    const int nstage = (kTileH + 2 * r) * sw;
    for (int s = tid; s < nstage; s += 256) {
      const int sy = s / sw, sx = s - sy * sw;
      const int gy = reflect101(y0 - r + sy, h), gx = reflect101(x0 - r + sx, w);
      uint32_t w0, w1;
      philox2(k0, k1, (uint32_t)(gy * w + gx), w0, w1);
      s_noise[0][s] = w0; s_noise[1][s] = w1;
    }
    __syncthreads();
    const double wt0 = s_f[1];
    for (int e = tid; e < kTileH * sw; e += 256) {
      const int row = e / sw, col = e - row * sw;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const uint32_t* q = &s_noise[k][(row + r) * sw + col];
        double t = noise_of(q[0]) * wt0;
        for (int d = r; d >= 1; --d) t += (noise_of(q[-d * sw]) + noise_of(q[d * sw])) * s_f[1 + d];
        s_mid[k][e] = t;
      }
    }
    __syncthreads();
  }

  const int lane_x = (tid & 15) * 4, row = tid >> 4;
  const int xg = x0 + lane_x, y = y0 + row;
  if (xg >= w || y >= h) return;
  double sx[4], sy[4];
  const double Y = (double)y;
  if (op == OP_HOMOGRAPHY) {
    const double h0 = s_f[0], h1 = s_f[1], h2 = s_f[2], h3 = s_f[3], h4 = s_f[4], h5 = s_f[5], h6 = s_f[6], h7 = s_f[7], h8 = s_f[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double X = (double)(xg + j);
      const double d = (h6 * X + h7 * Y) + h8;
      sx[j] = ((h0 * X + h1 * Y) + h2) / d;
      sy[j] = ((h3 * X + h4 * Y) + h5) / d;
    }
  } else if (op == OP_ELASTIC) {
    const double alpha = s_f[0], wt0 = s_f[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double b[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double* q = &s_mid[k][row * sw + lane_x + j + r];
        double t = q[0] * wt0;
        for (int d = r; d >= 1; --d) t += (q[-d] + q[d]) * s_f[1 + d];
        b[k] = t;
      }
      sx[j] = (double)(xg + j) + alpha * b[0];
      sy[j] = Y + alpha * b[1];
    }
  } else if (op == OP_PIECEWISE) {
    const int g = clampi(ia3, 2, 4);
    const int ci = min((y * (g - 1)) / (h - 1), g - 2);
    const double v = (double)(y * (g - 1) - ci * (h - 1)) / (double)(h - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xg + j;
      const int cj = min((x * (g - 1)) / (w - 1), g - 2);
      const double u = (double)(x * (g - 1) - cj * (w - 1)) / (double)(w - 1);
      const int tl = ci * g + cj, bl = tl + g;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double* P = s_f + 16 * k;
        const double ptl = P[tl], ptr = P[tl + 1], pbl = P[bl], pbr = P[bl + 1];
        const double val = u >= v ? (ptl + u * (ptr - ptl)) + v * (pbr - ptr) : (ptl + u * (pbr - pbl)) + v * (pbl - ptl);
        if (k == 0) sx[j] = val; else sy[j] = val;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { sx[j] = (double)(xg + j); sy[j] = Y; }
  }
  if (CUBIC && order == 3) sample_store<3>(a, n, xg, y, sx, sy, mode, cv);
  else if (order != 0) sample_store<1>(a, n, xg, y, sx, sy, mode, cv);
  else sample_store<0>(a, n, xg, y, sx, sy, mode, cv);
}


}  // namespace

extern "C" size_t pcuda_geometric_workspace_size(int b, int h, int w, int c, int with_labels) {
  if (b <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  const size_t px = (size_t)b * h * w;
  return round16(px * c) + (with_labels ? round16(px * sizeof(int)) : 0);
}

static int geometric_run(bool cubic, const uint8_t* in, uint8_t* out, const int* labels_in, int* labels_out, int b, int h, int w,
                         int c, int slots, const int* opcode, const int* iarg, const double* farg,
                         const unsigned long long* seed, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "geometric: null pointer");
  if (in == out || (labels_in && labels_in == labels_out))
    PCUDA_FAIL(PCUDA_E_BADARG, "geometric: in == out (the input is never written)");
  if ((labels_in == nullptr) != (labels_out == nullptr))
    PCUDA_FAIL(PCUDA_E_BADARG, "geometric: labels come with an input and an output, or not at all");
  if (b <= 0 || b > 65535 || c <= 0 || c > kMaxC) PCUDA_FAIL(PCUDA_E_BADARG, "geometric: bad dims (1..4 channels)");
  if (h < 2 || w < 2 || (long long)h * w * c >= (1ll << 31) - 8192)
    PCUDA_FAIL(PCUDA_E_BADARG, "geometric: bad dims (H and W at least 2)");
  if (slots < 0 || slots > kMaxSlots) PCUDA_FAIL(PCUDA_E_BADARG, "geometric: slots outside 0..8");
  if (slots > 0 && (!opcode || !iarg || !farg || !seed)) PCUDA_FAIL(PCUDA_E_BADARG, "geometric: null pointer (program)");
  if (slots > 1 && (!workspace || workspace_bytes < pcuda_geometric_workspace_size(b, h, w, c, labels_in != nullptr)))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "geometric: workspace too small");
  GeoArgs a;
  memset(&a, 0, sizeof(a));
  a.opcode = opcode; a.iarg = iarg; a.farg = farg; a.seed = reinterpret_cast<const uint32_t*>(seed);
  a.h = h; a.w = w; a.c = c; a.slots = slots;
  const size_t px = (size_t)b * h * w;
  uint8_t* ws_img = (uint8_t*)workspace;
  int* ws_lab = labels_in ? reinterpret_cast<int*>((uint8_t*)workspace + round16(px * c)) : nullptr;
  const dim3 grid(cdiv(w, kTileW) * cdiv(h, kTileH), b);
  const int launches = slots > 0 ? slots : 1;
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)px * launches * (2.0 * c + (labels_in ? 8.0 : 0.0)), (hipStream_t)s);
  const uint8_t* cur = in;
  const int* cur_lab = labels_in;
  for (int i = 0; i < launches; ++i) {
    // the slots alternate between the output and the workspace so that the last one lands in the output
    const bool to_ws = ((launches - 1 - i) & 1) != 0;
    uint8_t* dst = to_ws ? ws_img : out;
    int* dst_lab = labels_in ? (to_ws ? ws_lab : labels_out) : nullptr;
    a.in = cur; a.out = dst; a.lab_in = cur_lab; a.lab_out = dst_lab; a.slot = slots > 0 ? i : -1;
    a.vec_out = ((uintptr_t)dst & 3) == 0 && (((long long)w * c) & 3) == 0;
    a.vec_lab = ((uintptr_t)dst_lab & 15) == 0 && (w & 3) == 0;
    if (cubic) {
      hipLaunchKernelGGL(geometric_kernel<true>, grid, dim3(256), 0, (hipStream_t)s, a);
      PCUDA_CHECK_LAUNCH("geometric_kernel<cubic>");
    } else {
      hipLaunchKernelGGL(geometric_kernel<false>, grid, dim3(256), 0, (hipStream_t)s, a);
      PCUDA_CHECK_LAUNCH("geometric_kernel");
    }
    cur = dst; cur_lab = dst_lab;
  }
  return PCUDA_OK;
}

extern "C" int pcuda_geometric(const uint8_t* in, uint8_t* out, const int* labels_in, int* labels_out, int b, int h, int w,
                               int c, int slots, const int* opcode, const int* iarg, const double* farg,
                               const unsigned long long* seed, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  return geometric_run(false, in, out, labels_in, labels_out, b, h, w, c, slots, opcode, iarg, farg, seed, workspace,
                       workspace_bytes, s);
}

// the same arguments and workspace; order 3 is cubic here (order 0 nearest, anything else bilinear)
extern "C" int pcuda_geometric_cubic(const uint8_t* in, uint8_t* out, const int* labels_in, int* labels_out, int b, int h, int w,
                                     int c, int slots, const int* opcode, const int* iarg, const double* farg,
                                     const unsigned long long* seed, void* workspace, size_t workspace_bytes,
                                     pcuda_stream_t s) {
  return geometric_run(true, in, out, labels_in, labels_out, b, h, w, c, slots, opcode, iarg, farg, seed, workspace,
                       workspace_bytes, s);
}
