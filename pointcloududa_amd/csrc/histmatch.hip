// Device-side histogram matching of the loader path: the reference's `-mh` switch,
// match_histograms(img, reference_img, multichannel=True) (data_generator_mmwhs.py:174-176, 236-237), on [B,H,W,C] images.
//
// Definition (skimage.exposure.match_histograms 0.16-0.18, restated in plain numpy by scripts/make_match_hist_golden.py and
// pinned by tests/golden/match_hist.npz).  Per plane (b, c) of N = H W values and the template's table of channel c
// (tv = its sorted distinct values, tq = cumsum(counts) / M, both float64, built once on the host):
//   cnt = #{s' in the plane : s' <= s} (-0.0 and +0.0 are one value), q = double(cnt) / double(N)
//   j = the last index with tq[j] <= q;  j < 0: tv[0];  j == len - 1: tv[len - 1];  tq[j] == q: tv[j];  otherwise
//   slope = (tv[j+1] - tv[j]) / (tq[j+1] - tq[j]), r = slope (q - tq[j]) + tv[j], every operation rounded separately in float64
//   (the library is built with -ffp-contract=off); fp32 images store float(r) (nearest even), uint8 images uint8(trunc(r)).
// NaN in an image is unsupported (the reference's result is garbage there too); +-inf are ordinary values.
//
// fp32: the hot part is a sort of each plane's keys (the library's first sort).  A value maps to an order-preserving 32-bit
// key (-0.0 -> +0.0, then the sign bit flipped for non-negatives and all bits for negatives).  ONE workgroup of 1024 lanes
// owns a plane: a first sweep writes the keys to the workspace and counts all four 8-bit digit histograms in LDS (a digit's
// histogram does not depend on the order of the keys), then four LSD passes ping-pong through the plane's two key buffers.
// A pass walks the plane in tiles of 4096 keys in order; a wave takes 256 consecutive keys of the tile in four rounds of 64:
// a lane finds the lanes of its wave that hold the same digit with eight ballots (its rank among them is a popcount), the
// first of them adds their number to the wave's counter of that digit in LDS and hands the counter's old value -- the keys
// of the earlier rounds -- to the others, 256 lanes turn the sixteen counters of each digit into offsets behind the digit's
// running base, and every lane stores its keys at offset + rank -- the tile order, the wave order, the round order and the
// lane order carry the stability.  No workgroup waits on another, only integer LDS atomics, the same bits from run to run.
// A second kernel, one lane per value, finds cnt as the upper bound of its key in the sorted plane (a binary search that
// hits the L2), then q, the table search and the interpolation.
// uint8: one workgroup per plane, a 256-bin LDS histogram, an inclusive scan, a 256-entry LUT through the same
// interpolation, one gather pass.
// Every table index is clamped into [0, tstride) and every scatter position is checked against N before the store; every
// in-flight load's address stays alive (PCUDA_KEEP, VMEM address rule, common.h).
#include "common.h"

namespace {

#include "histmatch_device.h"      // float_key, digit_peers, sort_plane_keys, interp_table and the launch constants

struct HistArgs {
  const void* in;             // [b][n][c] fp32 or uint8
  void* out;                  // [b][n][c], the dtype of `in`
  uint32_t* keys;             // [b c][2][n] (workspace, fp32 path): the sorted plane ends in [.][0]
  const double* tvalues;      // [c][tstride]
  const double* tquantiles;   // [c][tstride]
  const int* tlen;            // [c]
  int n, c, tstride;
};

__device__ __forceinline__ int table_len(const HistArgs& a, int ch) {
  const int* p = a.tlen + ch;
  int len = *p;
  PCUDA_KEEP(p);
  len = len < 1 ? 1 : len;
  return len > a.tstride ? a.tstride : len;
}

// ------------------------------------------------------------------------------------------
// fp32: keys + four LSD radix passes, one workgroup per plane
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSortThreads) void histmatch_sort_kernel(const HistArgs a) {
  const int n = a.n, c = a.c;
  const int plane = blockIdx.x, b = plane / c, ch = plane - b * c;
  const float* src = static_cast<const float*>(a.in) + (long long)b * n * c + ch;
  uint32_t* buf0 = a.keys + (long long)plane * 2 * n;
  sort_plane_keys(src, c, n, buf0, buf0 + n);
}

// one lane per value: rank by binary search in the sorted plane, then the table
__global__ __launch_bounds__(256) void histmatch_lookup_kernel(const HistArgs a) {
  const int n = a.n, c = a.c;
  const int b = blockIdx.y;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;   // element of the sample: pixel * c + channel
  if (e >= (long long)n * c) return;
  const int ch = (int)(e % c);
  const float* src = static_cast<const float*>(a.in) + (long long)b * n * c + e;
  const uint32_t key = float_key(*src);
  PCUDA_KEEP(src);
  const uint32_t* sorted = a.keys + ((long long)b * c + ch) * 2 * n;
  int lo = 0, hi = n;                                              // upper bound of the key
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const uint32_t* p = sorted + mid;
    const uint32_t v = *p;
    if (v <= key) lo = mid + 1; else hi = mid;
    PCUDA_KEEP(p);
  }
  const double q = (double)lo / (double)n;
  const double r = interp_table(q, a.tquantiles + (long long)ch * a.tstride, a.tvalues + (long long)ch * a.tstride, table_len(a, ch));
  static_cast<float*>(a.out)[(long long)b * n * c + e] = (float)r;
}

// ------------------------------------------------------------------------------------------
// uint8: histogram, scan, LUT, gather; one workgroup per plane
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kU8Threads) void histmatch_u8_kernel(const HistArgs a) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_tot[4];
  __shared__ uint8_t s_lut[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, c = a.c;
  const int plane = blockIdx.x, b = plane / c, ch = plane - b * c;
  const uint8_t* src = static_cast<const uint8_t*>(a.in) + (long long)b * n * c + ch;
  uint8_t* dst = static_cast<uint8_t*>(a.out) + (long long)b * n * c + ch;
  if (tid < 256) s_hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += kU8Threads) {
    const uint8_t* p = src + (long long)i * c;
    const unsigned v = *p;
    PCUDA_KEEP(p);
    atomicAdd(&s_hist[v], 1u);
  }
  __syncthreads();
  unsigned incl = 0;
  if (tid < 256) {                                     // (waves 0..3, whole)
    incl = s_hist[tid];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (lane == 63) s_tot[wave] = incl;
  }
  __syncthreads();
  if (tid < 256) {
    unsigned cnt = incl;
    for (int k = 0; k < wave; ++k) cnt += s_tot[k];
    const double q = (double)cnt / (double)n;
    double r = interp_table(q, a.tquantiles + (long long)ch * a.tstride, a.tvalues + (long long)ch * a.tstride, table_len(a, ch));
    r = fmin(fmax(r, 0.0), 255.0);                     // (a uint8 template keeps r in [0, 255]: the cast never wraps)
    s_lut[tid] = (uint8_t)(int)r;                      // truncation toward zero
  }
  __syncthreads();
  for (int i = tid; i < n; i += kU8Threads) {
    const uint8_t* p = src + (long long)i * c;
    const unsigned v = *p;
    PCUDA_KEEP(p);
    dst[(long long)i * c] = s_lut[v];
  }
}


}  // namespace

extern "C" size_t pcuda_match_hist_workspace_size(int b, int h, int w, int c, int is_u8) {
  if (b <= 0 || h <= 0 || w <= 0 || c <= 0 || is_u8) return 0;
  return round16((size_t)b * c * 2 * (size_t)h * w * sizeof(uint32_t));      // per plane: the two key buffers of the ping-pong
}

extern "C" int pcuda_match_hist(const void* in, void* out, int is_u8, int b, int h, int w, int c, const double* tvalues,
                                const double* tquantiles, const int* tlen, int tstride, void* workspace, size_t workspace_bytes,
                                pcuda_stream_t s) {
  if (b < 0 || h < 0 || w < 0 || c <= 0 || c > kMaxC || b > 65535 || h > 32768 || w > 32768 ||
      (long long)h * w * c >= (1ll << 31) - 8192)
    PCUDA_FAIL(PCUDA_E_BADARG, "match_hist: bad dims (1..4 channels, sides up to 32768)");
  if (!tvalues || !tquantiles || !tlen || tstride < 1) PCUDA_FAIL(PCUDA_E_BADARG, "match_hist: null table or tstride < 1");
  if (b == 0 || h == 0 || w == 0) return PCUDA_OK;
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "match_hist: null pointer");
  if (in == out) PCUDA_FAIL(PCUDA_E_BADARG, "match_hist: in == out (the input is never written)");
  const size_t need = pcuda_match_hist_workspace_size(b, h, w, c, is_u8);
  if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "match_hist: workspace too small (or not 16-byte aligned)");
  HistArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.keys = static_cast<uint32_t*>(workspace);
  a.tvalues = tvalues; a.tquantiles = tquantiles; a.tlen = tlen;
  a.n = h * w; a.c = c; a.tstride = tstride;
  const size_t elems = (size_t)b * h * w * c;
  if (is_u8) {
    ProfScope prof(PCUDA_FAM_POINTWISE, 3.0 * (double)elems, (hipStream_t)s);
    hipLaunchKernelGGL(histmatch_u8_kernel, dim3(b * c), dim3(kU8Threads), 0, (hipStream_t)s, a);
    PCUDA_CHECK_LAUNCH("histmatch_u8_kernel");
    return PCUDA_OK;
  }
  // bytes: the keys written once and moved by four passes (a load and a store each), the input read twice, the output
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)elems * 4.0 * 12.0, (hipStream_t)s);
  hipLaunchKernelGGL(histmatch_sort_kernel, dim3(b * c), dim3(kSortThreads), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("histmatch_sort_kernel");
  hipLaunchKernelGGL(histmatch_lookup_kernel, dim3(cdiv((long long)a.n * c, 256), b), dim3(256), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("histmatch_lookup_kernel");
  return PCUDA_OK;
}
