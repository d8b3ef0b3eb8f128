// Device-side photometric augmentation of the loader path: the photometric operator set of
// ImageProcessor.augmentation2 (data_generator_mscmrseg.py:87-132): Gaussian / average / median blur, sharpen and emboss
// (one 3x3 correlation), additive Gaussian noise, dropout and coarse dropout, invert, add, multiply, grayscale -- on uint8
// [B,H,W,C] images, as a per-sample PROGRAM of up to eight slots that lives in device memory.
//
// Convention (this build's own: imgaug / cv2 are not vendored by the reference, parity is unpinned; pinned against a
// scipy and a plain-numpy restatement by tests/golden/photometric.npz):
//   * the value is uint8 again between two slots; non-integer arithmetic is float64 in the order written below (the library
//     is built with -ffp-contract=off), rounded floor(v + 0.5) and clipped to [0, 255]
//   * borders: reflect-101 (np.pad "reflect"), the median replicates (cv2.medianBlur)
//   * GAUSSIAN_BLUR: the host passes radius r and the normalised weights w[0..r] (no exp here); rows first
//     (t = x[0] w[0]; for d = r..1: t += (x[-d] + x[+d]) w[d], scipy's symmetric correlate1d), then the same along x on the
//     unrounded float64
//   * AVERAGE_BLUR: offsets -(k / 2) .. k - k / 2 - 1, (2 S + k k) / (2 k k) in integers;  MEDIAN_BLUR: rank (k k - 1) / 2
//   * CONV3X3: t = 0; t += x[i] w[i] for the nine taps row-major
//   * random operators: Philox4x32-10 as implemented here (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
//     0xBB67AE85), key = the slot's seed, counter = (element index inside the sample, 0, 0, 0): the value depends on
//     (seed, element index) only.  Noise: u = (x + 0.5) 2^-32 of the first two words, z = sqrt(-2 log u1) cos(2 pi u2),
//     v + scale z.  Dropouts: element -> 0 iff the first word < the host's threshold
//
// One slot = two launches over (tile, sample): a pointwise kernel (no LDS; 16 bytes per lane) and a neighbourhood kernel
// (tile + halo staged in LDS once, results collected in LDS and stored 16 bytes per lane); each workgroup reads its sample's
// opcode with scalar loads and leaves at once when the slot belongs to the other kernel, so the branch on the opcode is
// wave-uniform.  The slots ping-pong between the caller's output and the caller's workspace.  Every gather address is
// mirrored or clamped into the image BEFORE the load (a garbage program gives wrong pixels, never an access out of
// bounds), an unknown opcode copies, and every in-flight load's address stays alive (PCUDA_KEEP, VMEM address rule,
// common.h).
#include "common.h"
#include "image_device.h"

namespace {

enum {
  OP_NOP = 0, OP_GAUSSIAN_BLUR = 1, OP_AVERAGE_BLUR = 2, OP_MEDIAN_BLUR = 3, OP_CONV3X3 = 4, OP_GAUSSIAN_NOISE = 5,
  OP_DROPOUT = 6, OP_COARSE_DROPOUT = 7, OP_INVERT = 8, OP_ADD = 9, OP_MULTIPLY = 10, OP_GRAYSCALE = 11
};

constexpr int kMaxSlots = 8, kIArgs = 4, kFArgs = 16;
constexpr int kRows = 16;            // rows of a neighbourhood tile
constexpr int kMaxR = 12;            // largest halo: the Gaussian at sigma = 3
constexpr int kMaxC = 4;
constexpr int kMaxStageRow = 352;    // bytes of a staged row: (64 + 24) pixels x 4 channels (C = 1: 280, 2: 304, 3: 264)
constexpr int kMaxTileRow = 256;     // bytes of an output row of a tile

struct PhotoArgs {
  const uint8_t* in;         // [b][h][w][c]
  uint8_t* out;              // [b][h][w][c]
  const int* opcode;         // [b][slots]
  const int* iarg;           // [b][slots][4]
  const double* farg;        // [b][slots][16]
  const uint32_t* seed;      // [b][slots][2] (low, high word)
  int h, w, c, slots;
  int slot;                  // the slot this launch runs; < 0: copy
  int twpx;                  // pixels per tile row: 64 (C = 3: 192 bytes) or 256 / C (256 bytes)
  int vec_in, vec_out;       // 16-byte loads / stores are aligned
};

__device__ __forceinline__ bool is_neighbourhood(int op) { return op >= OP_GAUSSIAN_BLUR && op <= OP_CONV3X3; }
using imgdev::clampi;
using imgdev::reflect101;
using imgdev::round_u8;

// Philox4x32-10 as implemented here: ten rounds, the key bumped between rounds
struct Philox4 { uint32_t x0, x1, x2, x3; };
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0) {
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

struct PointArgs {
  int ia0, ia1, ia2, ia3;
  double fa0, fa1, fa2, fa3;
  uint32_t k0, k1;
  int h, w, c, i0;
  const uint8_t* src;
};

// sixteen consecutive elements of one sample through one pointwise opcode
template <int OP>
__device__ __forceinline__ void pointwise_slot(uint8_t (&v)[16], const PointArgs& q) {
  const int c = q.c, w = q.w, h = q.h;
  const int gh = clampi(q.ia2, 1, 4096), gw = clampi(q.ia3, 1, 4096);      // coarse dropout grid
  int pix = q.i0 / c, ch = q.i0 - pix * c;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = q.i0 + i;
    const int x = v[i];
    if (OP == OP_GAUSSIAN_NOISE) {
      const Philox4 r = philox4x32_10(q.k0, q.k1, (uint32_t)(q.ia0 ? e : pix));
      const double u1 = ((double)r.x0 + 0.5) * 0x1p-32, u2 = ((double)r.x1 + 0.5) * 0x1p-32;
      const double rad = sqrt(-2.0 * log(u1));
      const double z = rad * cos(6.283185307179586 * u2);
      v[i] = round_u8((double)x + q.fa0 * z);
    } else if (OP == OP_DROPOUT) {
      const Philox4 r = philox4x32_10(q.k0, q.k1, (uint32_t)(q.ia0 ? e : pix));
      if (r.x0 < (uint32_t)q.ia1) v[i] = 0;
    } else if (OP == OP_COARSE_DROPOUT) {
      const int py = pix / w, px = pix - py * w;
      const int cell = (int)(((long long)py * gh) / h) * gw + (int)(((long long)px * gw) / w);
      const Philox4 r = philox4x32_10(q.k0, q.k1, (uint32_t)(q.ia0 ? cell * c + ch : cell));
      if (r.x0 < (uint32_t)q.ia1) v[i] = 0;
    } else if (OP == OP_INVERT) {
      if ((q.ia0 >> ch) & 1) v[i] = (uint8_t)(255 - x);
    } else if (OP == OP_ADD) {
      const int add = ch == 0 ? q.ia0 : (ch == 1 ? q.ia1 : (ch == 2 ? q.ia2 : q.ia3));
      v[i] = (uint8_t)clampi(x + add, 0, 255);
    } else if (OP == OP_MULTIPLY) {
      const double m = ch == 0 ? q.fa0 : (ch == 1 ? q.fa1 : (ch == 2 ? q.fa2 : q.fa3));
      v[i] = round_u8((double)x * m);
    } else if (c == 3) {      // OP_GRAYSCALE (C = 1: copy; the host rejects every other C)
      const uint8_t* p = q.src + 3 * (pix < h * w ? pix : h * w - 1);
      const double c0 = (double)p[0], c1 = (double)p[1], c2 = (double)p[2];
      PCUDA_KEEP(p);
      const double g = 0.299 * c0 + 0.587 * c1 + 0.114 * c2;
      v[i] = round_u8((1.0 - q.fa0) * (double)x + q.fa0 * g);
    }
    if (++ch == c) { ch = 0; ++pix; }
  }
}

// ------------------------------------------------------------------------------------------
// pointwise slots (and NOP / unknown opcodes: copy): 16 consecutive bytes of the sample per lane
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void photometric_pointwise_kernel(const PhotoArgs a) {
  const int n = blockIdx.y;
  const int at = n * a.slots + a.slot;
  const int op = a.slot < 0 ? (int)OP_NOP : a.opcode[at];
  if (is_neighbourhood(op)) return;
  const int c = a.c, w = a.w, h = a.h;
  const int numel = h * w * c;
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 16;
  if (i0 >= numel) return;
  const uint8_t* src = a.in + (long long)n * numel;
  uint8_t* dst = a.out + (long long)n * numel;
  const bool full = i0 + 16 <= numel;
  uint8_t v[16];
  if (a.vec_in && full) {
    const uint4* p = reinterpret_cast<const uint4*>(src + i0);
    const uint4 q = *p;
    const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = (uint8_t)(wd[i >> 2] >> (8 * (i & 3)));
    PCUDA_KEEP(p);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint8_t* p = src + (i0 + i < numel ? i0 + i : numel - 1);
      v[i] = *p;
      PCUDA_KEEP(p);
    }
  }
  if (op >= OP_GAUSSIAN_NOISE && op <= OP_GRAYSCALE) {
    PointArgs q;
    const int* ia = a.iarg + at * kIArgs;
    const double* fa = a.farg + at * kFArgs;
    q.ia0 = ia[0]; q.ia1 = ia[1]; q.ia2 = ia[2]; q.ia3 = ia[3];
    q.fa0 = fa[0]; q.fa1 = fa[1]; q.fa2 = fa[2]; q.fa3 = fa[3];
    const uint32_t* sd = a.seed + 2 * at;
    asm volatile("" : "+v"(sd));      // a vector address of its own, kept alive below (the compiler loads the pair through a
                                      // zero offset register that its data overwrites otherwise)
    q.k0 = sd[0]; q.k1 = sd[1];
    q.h = h; q.w = w; q.c = c; q.i0 = i0; q.src = src;
    // one loop per opcode (the branch is wave-uniform): with the switch inside the loop the sixteen unrolled copies of all
    // seven bodies did not fit the instruction cache, and INVERT took 25 us where the copy takes 6
    switch (op) {
      case OP_GAUSSIAN_NOISE: pointwise_slot<OP_GAUSSIAN_NOISE>(v, q); break;
      case OP_DROPOUT: pointwise_slot<OP_DROPOUT>(v, q); break;
      case OP_COARSE_DROPOUT: pointwise_slot<OP_COARSE_DROPOUT>(v, q); break;
      case OP_INVERT: pointwise_slot<OP_INVERT>(v, q); break;
      case OP_ADD: pointwise_slot<OP_ADD>(v, q); break;
      case OP_MULTIPLY: pointwise_slot<OP_MULTIPLY>(v, q); break;
      default: pointwise_slot<OP_GRAYSCALE>(v, q); break;
    }
    PCUDA_KEEP(ia); PCUDA_KEEP(fa); PCUDA_KEEP(sd);      // (VMEM address rule, common.h)
  }
  if (a.vec_out && full) {
    uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) wd[i >> 2] |= (uint32_t)v[i] << (8 * (i & 3));
    *reinterpret_cast<uint4*>(dst + i0) = uint4{wd[0], wd[1], wd[2], wd[3]};
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i0 + i < numel) dst[i0 + i] = v[i];
  }
}

// ------------------------------------------------------------------------------------------
// neighbourhood slots: 16 rows x (192 or 256 bytes) of output per workgroup, tile + halo staged in LDS once
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void photometric_neighbourhood_kernel(const PhotoArgs a) {
  __shared__ uint8_t s_in[(kRows + 2 * kMaxR) * kMaxStageRow];      // 14080 B
  __shared__ double s_mid[kRows * kMaxStageRow];                    // 45056 B: the Gaussian's row pass, unrounded
  __shared__ uint4 s_out4[kRows * kMaxTileRow / 16];                //  4096 B
  __shared__ double s_w[kFArgs];
  uint8_t* s_out = reinterpret_cast<uint8_t*>(s_out4);

  const int n = blockIdx.y;
  const int at = n * a.slots + a.slot;
  const int op = a.opcode[at];
  if (!is_neighbourhood(op)) return;
  const int tid = threadIdx.x;
  const int c = a.c, w = a.w, h = a.h, twpx = a.twpx;
  const int tb = twpx * c;                                 // bytes of an output row of the tile: 192 or 256
  const int tiles_x = (w + twpx - 1) / twpx;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * twpx, y0 = ty * kRows;
  int k = a.iarg[at * kIArgs];
  int r;                                                   // halo
  if (op == OP_GAUSSIAN_BLUR) { r = clampi(k, 0, kMaxR); }
  else if (op == OP_AVERAGE_BLUR) { k = clampi(k, 1, 7); r = k / 2; }
  else if (op == OP_MEDIAN_BLUR) { k = clampi(k, 1, 11) | 1; r = k / 2; }
  else { r = 1; }
  const bool replicate = op == OP_MEDIAN_BLUR;
  const int swpx = twpx + 2 * r, srow = swpx * c;          // staged row: pixels, bytes
  const int nstage = (kRows + 2 * r) * srow;
  const uint8_t* src = a.in + (long long)n * h * w * c;

  if (tid < kFArgs) {
    const double* p = a.farg + at * kFArgs + tid;
    s_w[tid] = *p;
    PCUDA_KEEP(p);
  }
  for (int s = tid; s < nstage; s += 256) {
    const int sy = s / srow, rem = s - sy * srow;
    const int sx = rem / c, ch = rem - sx * c;
    int gy = y0 - r + sy, gx = x0 - r + sx;
    gy = replicate ? clampi(gy, 0, h - 1) : reflect101(gy, h);
    gx = replicate ? clampi(gx, 0, w - 1) : reflect101(gx, w);
    const uint8_t* p = src + ((long long)gy * w + gx) * c + ch;
    s_in[s] = *p;
    PCUDA_KEEP(p);
  }
  __syncthreads();

  if (op == OP_GAUSSIAN_BLUR) {      // rows first (scipy filters axis 0 first): kRows x srow unrounded values
    const double w0 = s_w[0];
    for (int e = tid; e < kRows * srow; e += 256) {
      const int row = e / srow, j = e - row * srow;
      const uint8_t* q = s_in + (row + r) * srow + j;
      double t = (double)q[0] * w0;
      for (int d = r; d >= 1; --d) t += ((double)q[-d * srow] + (double)q[d * srow]) * s_w[d];
      s_mid[e] = t;
    }
    __syncthreads();
  }

  for (int e = tid; e < kRows * tb; e += 256) {
    const int row = e / tb, jb = e - row * tb;
    const int px = jb / c, ch = jb - px * c;
    uint8_t res = 0;
    if (y0 + row < h && x0 + px < w) {
      const int centre = (row + r) * srow + (px + r) * c + ch;      // in s_in
      if (op == OP_GAUSSIAN_BLUR) {
        const double* q = s_mid + row * srow + (px + r) * c + ch;
        double t = q[0] * s_w[0];
        for (int d = r; d >= 1; --d) t += (q[-d * c] + q[d * c]) * s_w[d];
        res = round_u8(t);
      } else if (op == OP_AVERAGE_BLUR) {
        const int lo = -(k / 2), hi = k - k / 2 - 1;
        int sum = 0;
        for (int dy = lo; dy <= hi; ++dy)
          for (int dx = lo; dx <= hi; ++dx) sum += s_in[centre + dy * srow + dx * c];
        res = (uint8_t)((2 * sum + k * k) / (2 * k * k));
      } else if (op == OP_MEDIAN_BLUR) {
        // the smallest value m with #(window <= m) >= (k k + 1) / 2: eight halvings of [0, 255]
        const int need = (k * k + 1) / 2;
        int lo = 0, hi = 255;
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {
          const int mid = (lo + hi) >> 1;
          int cnt = 0;
          for (int dy = -r; dy <= r; ++dy) {
            const uint8_t* q = s_in + centre + dy * srow;
            for (int dx = -r; dx <= r; ++dx) cnt += q[dx * c] <= mid;
          }
          if (cnt >= need) hi = mid; else lo = mid + 1;
        }
        res = (uint8_t)lo;
      } else {      // OP_CONV3X3
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) t += (double)s_in[centre + (i / 3 - 1) * srow + (i % 3 - 1) * c] * s_w[i];
        res = round_u8(t);
      }
    }
    s_out[row * tb + jb] = res;
  }
  __syncthreads();

  const int row_bytes = w * c, chunks_per_row = tb / 16;
  uint8_t* dst = a.out + (long long)n * h * row_bytes;
  for (int q = tid; q < kRows * chunks_per_row; q += 256) {
    const int row = q / chunks_per_row, cb = (q - row * chunks_per_row) * 16;
    const int gy = y0 + row, gb = x0 * c + cb;
    if (gy >= h || gb >= row_bytes) continue;
    uint8_t* p = dst + (long long)gy * row_bytes + gb;
    if (a.vec_out && gb + 16 <= row_bytes) {
      *reinterpret_cast<uint4*>(p) = s_out4[(row * tb + cb) >> 4];
    } else {
      for (int i = 0; i < 16 && gb + i < row_bytes; ++i) p[i] = s_out[row * tb + cb + i];
    }
  }
}


}  // namespace

extern "C" size_t pcuda_photometric_workspace_size(int b, int h, int w, int c) {
  if (b <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  return round16((size_t)b * h * w * c);
}

extern "C" int pcuda_photometric(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode,
                                 const int* iarg, const double* farg, const unsigned long long* seed, void* workspace,
                                 size_t workspace_bytes, pcuda_stream_t s) {
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "photometric: null pointer");
  if (in == out) PCUDA_FAIL(PCUDA_E_BADARG, "photometric: in == out (the input is never written)");
  if (b <= 0 || b > 65535 || h <= 0 || w <= 0 || c <= 0 || c > kMaxC || (long long)h * w * c >= (1ll << 31) - 8192)
    PCUDA_FAIL(PCUDA_E_BADARG, "photometric: bad dims (1..4 channels)");
  if (slots < 0 || slots > kMaxSlots) PCUDA_FAIL(PCUDA_E_BADARG, "photometric: slots outside 0..8");
  if (slots > 0 && (!opcode || !iarg || !farg || !seed)) PCUDA_FAIL(PCUDA_E_BADARG, "photometric: null pointer (program)");
  const size_t bytes = (size_t)b * h * w * c;
  if (slots > 1 && (!workspace || workspace_bytes < pcuda_photometric_workspace_size(b, h, w, c)))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "photometric: workspace too small");
  PhotoArgs a;
  memset(&a, 0, sizeof(a));
  a.opcode = opcode; a.iarg = iarg; a.farg = farg; a.seed = reinterpret_cast<const uint32_t*>(seed);
  a.h = h; a.w = w; a.c = c; a.slots = slots;
  a.twpx = c == 3 ? 64 : kMaxTileRow / c;
  const long long per_sample = (long long)h * w * c;
  const dim3 grid_p(cdiv(cdiv(per_sample, 16), 256), b), grid_n(cdiv(w, a.twpx) * cdiv(h, kRows), b);
  const int launches = slots > 0 ? slots : 1;
  ProfScope prof(PCUDA_FAM_POINTWISE, 2.0 * (double)bytes * launches, (hipStream_t)s);
  const uint8_t* cur = in;
  for (int i = 0; i < launches; ++i) {
    // the slots alternate between the output and the workspace so that the last one lands in the output
    uint8_t* dst = ((launches - 1 - i) & 1) ? (uint8_t*)workspace : out;
    a.in = cur; a.out = dst; a.slot = slots > 0 ? i : -1;
    a.vec_in = ((uintptr_t)cur & 15) == 0 && (per_sample & 15) == 0;
    a.vec_out = ((uintptr_t)dst & 15) == 0 && (per_sample & 15) == 0;
    hipLaunchKernelGGL(photometric_pointwise_kernel, grid_p, dim3(256), 0, (hipStream_t)s, a);
    PCUDA_CHECK_LAUNCH("photometric_pointwise_kernel");
    if (slots > 0) {
      a.vec_out = ((uintptr_t)dst & 15) == 0 && (((long long)w * c) & 15) == 0;
      hipLaunchKernelGGL(photometric_neighbourhood_kernel, grid_n, dim3(256), 0, (hipStream_t)s, a);
      PCUDA_CHECK_LAUNCH("photometric_neighbourhood_kernel");
    }
    cur = dst;
  }
  return PCUDA_OK;
}
