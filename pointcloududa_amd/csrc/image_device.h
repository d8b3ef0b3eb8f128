// Device helpers the image kernels share (photometric, geometric, stylize, spx_connect, croppad): defined once, pulled into
// a source's unnamed namespace with using-declarations, so a source keeps a local variant under the same name where it
// needs one (geometric.hip's reflect101 takes n >= 2; geometric.hip and croppad.hip round into a 32-bit word).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace imgdev {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// np.pad(mode="reflect") index for any i; n >= 1
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  i %= period;
  if (i < 0) i += period;
  return i < n ? i : period - i;
}
__device__ __forceinline__ uint8_t round_u8(double v) {
  const double r = fmin(fmax(floor(v + 0.5), 0.0), 255.0);      // (fmax returns the other operand for a NaN: 0)
  return (uint8_t)(int)r;
}

// Keys cubic convolution, A = -0.75 (the constant OpenCV documents for INTER_CUBIC), for the fraction t in [0, 1) of a
// source coordinate: the weights of the taps i0 - 1, i0, i0 + 1, i0 + 2.  Float64, every operation rounded on
// its own (-ffp-contract=off), in exactly this order; t = 0 gives (0, 1, 0, 0) exactly
constexpr double kCubicA = -0.75;
__device__ __forceinline__ void cubic_weights(double t, double (&wt)[4]) {
  const double u = t + 1.0;
  wt[0] = ((kCubicA * u - 5.0 * kCubicA) * u + 8.0 * kCubicA) * u - 4.0 * kCubicA;
  wt[1] = ((kCubicA + 2.0) * t - (kCubicA + 3.0)) * t * t + 1.0;
  const double r = 1.0 - t;
  wt[2] = ((kCubicA + 2.0) * r - (kCubicA + 3.0)) * r * r + 1.0;
  wt[3] = ((1.0 - wt[0]) - wt[1]) - wt[2];
}

// first word of Philox4x32-10 as photometric.hip implements it: ten rounds, the key bumped between rounds
__device__ __forceinline__ uint32_t philox_word0(uint32_t k0, uint32_t k1, uint32_t c0) {
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// Working size of a SUPERPIXELS slot whose max_size (iarg[6]) is m, for h x w images: the slot is SCALED iff
// m >= 1 and L = max(h, w) > m, and then runs on h2 x w2 = max(1, (h m) / L) x max(1, (w m) / L) (the longer side is exactly
// m); else h2 x w2 = h x w and the return value is false
__device__ __forceinline__ bool spx_working_size(int h, int w, int m, int& h2, int& w2) {
  const int L = h > w ? h : w;
  h2 = h; w2 = w;
  if (m < 1 || L <= m) return false;
  const int hs = (int)(((long long)h * m) / L), ws = (int)(((long long)w * m) / L);
  h2 = hs < 1 ? 1 : hs; w2 = ws < 1 ? 1 : ws;
  return true;
}

}  // namespace imgdev
