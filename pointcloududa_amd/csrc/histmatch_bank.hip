// Histogram matching against a BANK of references held on the device: every sample of a batch is
// matched to the reference its entry of ref_index names -- the unsupervised-domain-adaptation form (a source image against a
// target image drawn from a pool, or against this step's target batch), where histmatch.hip matches every image to one
// template whose tables were sorted on the host.  Same definition (skimage.exposure.match_histograms 0.16-0.18 per plane,
// scripts/make_match_hist_golden.py), same bits.
//
// fp32 bank: per reference plane (r, c) of M = RH RW values its SORTED order-preserving keys k[0..M), 4 bytes per value (the
// sort of histmatch_device.h, one workgroup per plane; its second ping-pong buffer is the build's workspace).  No (values,
// quantiles) table exists: the sorted plane is the table -- the distinct values are the run ends, a run end e has the quantile
// E(e) = double(e) / double(M).  Per image value, after its own rank search (cnt, q = double(cnt) / double(N), as in
// histmatch.hip), with val(key) = the float the key came from, widened to float64:
//   1. e* = max{e in [0, M] : E(e) <= q}, decided by the division itself (trunc(q M) is the first guess, its neighbours are
//      tested with E)
//   2. p = the last run end at or below e*: p = e* if e* == 0, e* == M or k[e*-1] != k[e*], else lower_bound(k, k[e*])
//   3. p == 0: r = val(k[0])          4. p == M: r = val(k[M-1])
//   5. q0 = E(p), v0 = val(k[p-1]); q0 == q: r = v0; else p1 = upper_bound(k, k[p]), q1 = E(p1), v1 = val(k[p]),
//      slope = (v1 - v0) / (q1 - q0), r = slope (q - q0) + v0, every operation rounded on its own (-ffp-contract=off)
//   6. the store is float(r), nearest even
// which is np.interp(cumsum(sc) / N, cumsum(tc) / M, tv) with tv, tc read off the sorted plane.  A reference's -0.0 is read as
// +0.0 (the keys canonicalise it).  Non-finite reference values are unsupported: the build raises a device-side flag.
//
// uint8 bank: per reference plane 256 uint32 counts (an LDS histogram, one workgroup per plane).  The match runs one workgroup
// per image plane: its own histogram and scan as histmatch_u8_kernel, then the 256 counts of its sample's reference are
// scanned and compacted into tq / tv (up to 256 float64 each, in LDS), the same interp_table, a 256-entry LUT, one gather.
//
// ref_index entries are clamped into [0, R) on the device; every search index stays inside its plane; every in-flight load's
// address stays alive (PCUDA_KEEP, VMEM address rule, common.h).  Integer LDS atomics only, no workgroup waits on another, the
// same bits from run to run.
#include "common.h"

namespace {

#include "histmatch_device.h"      // float_key, digit_peers, sort_plane_keys, interp_table and the launch constants

struct BankBuildArgs {
  const void* refs;           // [r][m][c] fp32 or uint8
  uint32_t* bank;             // fp32: [r c][m] sorted keys; uint8: [r c][256] counts
  uint32_t* other;            // fp32: [r c][m], the second buffer of the ping-pong (workspace)
  int* flag;                  // set to 1 when a reference value is not finite
  int m, c;
};

struct BankMatchArgs {
  const void* in;             // [b][n][c] fp32 or uint8
  void* out;                  // [b][n][c], the dtype of `in`
  uint32_t* keys;             // [b c][2][n] (workspace, fp32 path): the sorted image plane ends in [.][0]
  const uint32_t* bank;       // as BankBuildArgs::bank
  const int* ref_index;       // [b]
  int n, c, m, r;
};

__device__ __forceinline__ double key_value(uint32_t k) {        // the inverse of float_key, widened
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return (double)__builtin_bit_cast(float, u);
}

__device__ __forceinline__ int sample_reference(const BankMatchArgs& a, int b) {
  const int* p = a.ref_index + b;
  int ri = *p;
  PCUDA_KEEP(p);
  ri = ri < 0 ? 0 : ri;
  return ri > a.r - 1 ? a.r - 1 : ri;
}

// ------------------------------------------------------------------------------------------
// fp32 build: the sorted keys of every reference plane
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSortThreads) void histbank_sort_kernel(const BankBuildArgs a) {
  const int m = a.m, c = a.c;
  const int plane = blockIdx.x, r = plane / c, ch = plane - r * c;
  const float* src = static_cast<const float*>(a.refs) + (long long)r * m * c + ch;
  const bool bad = sort_plane_keys(src, c, m, a.bank + (long long)plane * m, a.other + (long long)plane * m);
  if (bad) *a.flag = 1;                                            // (every writer stores the same value)
}

// image planes: as histmatch_sort_kernel
__global__ __launch_bounds__(kSortThreads) void histbank_image_sort_kernel(const BankMatchArgs a) {
  const int n = a.n, c = a.c;
  const int plane = blockIdx.x, b = plane / c, ch = plane - b * c;
  const float* src = static_cast<const float*>(a.in) + (long long)b * n * c + ch;
  uint32_t* buf0 = a.keys + (long long)plane * 2 * n;
  sort_plane_keys(src, c, n, buf0, buf0 + n);
}

// one lane per value: its rank in its own sorted plane, then steps 1 to 6 on the sorted plane of its sample's reference
__global__ __launch_bounds__(256) void histbank_lookup_kernel(const BankMatchArgs a) {
  const int n = a.n, c = a.c, m = a.m;
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
  const uint32_t* k = a.bank + ((long long)sample_reference(a, b) * c + ch) * m;
  const double dm = (double)m;

  // 1. e* by the division: the product is a guess that is off by one at the most
  int es = (int)(q * dm);
  es = es < 0 ? 0 : (es > m ? m : es);
#pragma unroll 1
  for (int t = 0; t < 2 && es < m && (double)(es + 1) / dm <= q; ++t) ++es;
#pragma unroll 1
  for (int t = 0; t < 2 && es > 0 && (double)es / dm > q; ++t) --es;

  // 2. the last run end at or below e*
  const uint32_t *pa = k + (es > 0 ? es - 1 : 0), *pb = k + (es < m ? es : m - 1);
  const uint32_t ka = *pa, kb = *pb;
  PCUDA_KEEP(pa); PCUDA_KEEP(pb);
  int p = es;
  if (es > 0 && es < m && ka == kb) {                              // inside a run: its first index (k[es - 1] == kb: below es)
    lo = 0; hi = es;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const uint32_t* pm = k + mid;
      const uint32_t v = *pm;
      if (v < kb) lo = mid + 1; else hi = mid;
      PCUDA_KEEP(pm);
    }
    p = lo;
  }

  // 3. to 5.
  const uint32_t *p0 = k + (p > 0 ? p - 1 : 0), *p1 = k + (p < m ? p : m - 1);
  const uint32_t k0 = *p0, k1 = *p1;
  PCUDA_KEEP(p0); PCUDA_KEEP(p1);
  const double v0 = key_value(k0), v1 = key_value(k1), q0 = (double)p / dm;
  double r;
  if (p == 0) {
    r = v1;                                                        // (k[0])
  } else if (p == m || q0 == q) {
    r = v0;                                                        // (p == m: k[m - 1])
  } else {
    lo = p + 1; hi = m;                                            // upper bound of k[p] (k[p] itself is not above it)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const uint32_t* pm = k + mid;
      const uint32_t v = *pm;
      if (v <= k1) lo = mid + 1; else hi = mid;
      PCUDA_KEEP(pm);
    }
    const double q1 = (double)lo / dm;
    const double slope = (v1 - v0) / (q1 - q0);
    r = slope * (q - q0) + v0;
  }
  static_cast<float*>(a.out)[(long long)b * n * c + e] = (float)r;
}

// ------------------------------------------------------------------------------------------
// uint8
// ------------------------------------------------------------------------------------------
// inclusive scan over the lanes tid < 256 (waves 0..3, whole); every lane of the workgroup calls it (two barriers)
__device__ __forceinline__ unsigned scan256(unsigned v, unsigned* s_tot, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  unsigned incl = v;
  if (tid < 256) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (lane == 63) s_tot[wave] = incl;
  }
  __syncthreads();
  if (tid < 256)
    for (int w = 0; w < wave; ++w) incl += s_tot[w];
  __syncthreads();                                     // (s_tot is free again)
  return incl;
}

__global__ __launch_bounds__(kU8Threads) void histbank_count_u8_kernel(const BankBuildArgs a) {
  __shared__ unsigned s_hist[256];
  const int tid = threadIdx.x;
  const int m = a.m, c = a.c;
  const int plane = blockIdx.x, r = plane / c, ch = plane - r * c;
  const uint8_t* src = static_cast<const uint8_t*>(a.refs) + (long long)r * m * c + ch;
  if (tid < 256) s_hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < m; i += kU8Threads) {
    const uint8_t* p = src + (long long)i * c;
    const unsigned v = *p;
    PCUDA_KEEP(p);
    atomicAdd(&s_hist[v], 1u);
  }
  __syncthreads();
  if (tid < 256) a.bank[(long long)plane * 256 + tid] = s_hist[tid];
}

__global__ __launch_bounds__(kU8Threads) void histbank_match_u8_kernel(const BankMatchArgs a) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_tot[4];
  __shared__ double s_tq[256], s_tv[256];
  __shared__ int s_len;
  __shared__ uint8_t s_lut[256];
  const int tid = threadIdx.x;
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
  const unsigned cnt = scan256(tid < 256 ? s_hist[tid] : 0u, s_tot, tid);
  // the reference's table: its distinct values are the bins that are not empty
  const uint32_t* pc = a.bank + ((long long)sample_reference(a, b) * c + ch) * 256 + (tid & 255);
  const unsigned tc = *pc;
  PCUDA_KEEP(pc);
  const unsigned cum = scan256(tc, s_tot, tid);
  const unsigned pos = scan256(tc != 0u ? 1u : 0u, s_tot, tid);     // 1-based among the bins that are not empty
  if (tid < 256 && tc != 0u) {
    s_tq[pos - 1] = (double)cum / (double)a.m;
    s_tv[pos - 1] = (double)tid;
  }
  if (tid == 255) s_len = (int)pos;
  __syncthreads();
  if (tid < 256) {
    int len = s_len;
    len = len < 1 ? 1 : len;                           // (an empty table only comes from a bank that was never built)
    const double q = (double)cnt / (double)n;
    double r = interp_table(q, s_tq, s_tv, len);
    r = fmin(fmax(r, 0.0), 255.0);                     // (a uint8 reference keeps r in [0, 255]: the cast never wraps)
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


inline bool bad_plane_dims(int count, int h, int w, int c) {
  return count < 0 || h < 0 || w < 0 || c <= 0 || c > kMaxC || count > 65535 || h > 32768 || w > 32768 ||
         (long long)h * w * c >= (1ll << 31) - 8192;
}

}  // namespace

extern "C" size_t pcuda_hist_bank_size(int r, int rh, int rw, int c, int is_u8) {
  if (r <= 0 || rh <= 0 || rw <= 0 || c <= 0) return 0;
  if (is_u8) return (size_t)r * c * 256 * sizeof(uint32_t);
  return round16((size_t)r * c * (size_t)rh * rw * sizeof(uint32_t));         // per plane: its sorted keys
}

extern "C" size_t pcuda_hist_bank_workspace_size(int r, int rh, int rw, int c, int is_u8) {
  if (r <= 0 || rh <= 0 || rw <= 0 || c <= 0 || is_u8) return 0;
  return round16((size_t)r * c * (size_t)rh * rw * sizeof(uint32_t));         // per plane: the other buffer of the ping-pong
}

extern "C" int pcuda_hist_bank_build(const void* refs, int is_u8, int r, int rh, int rw, int c, void* bank, size_t bank_bytes,
                                     int* flag, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (bad_plane_dims(r, rh, rw, c)) PCUDA_FAIL(PCUDA_E_BADARG, "hist_bank_build: bad dims (1..4 channels, sides up to 32768)");
  if (r == 0 || rh == 0 || rw == 0) return PCUDA_OK;
  if (!refs || !bank || !flag) PCUDA_FAIL(PCUDA_E_BADARG, "hist_bank_build: null pointer");
  if (refs == bank) PCUDA_FAIL(PCUDA_E_BADARG, "hist_bank_build: refs == bank (the references are never written)");
  if (bank_bytes < pcuda_hist_bank_size(r, rh, rw, c, is_u8) || ((uintptr_t)bank & 15) != 0)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "hist_bank_build: bank too small (or not 16-byte aligned)");
  const size_t need = pcuda_hist_bank_workspace_size(r, rh, rw, c, is_u8);
  if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "hist_bank_build: workspace too small (or not 16-byte aligned)");
  BankBuildArgs a;
  memset(&a, 0, sizeof(a));
  a.refs = refs; a.bank = static_cast<uint32_t*>(bank); a.other = static_cast<uint32_t*>(workspace); a.flag = flag;
  a.m = rh * rw; a.c = c;
  const size_t elems = (size_t)r * rh * rw * c;
  if (hipMemsetAsync(flag, 0, sizeof(int), (hipStream_t)s) != hipSuccess) PCUDA_FAIL(PCUDA_E_LAUNCH, "hist_bank_build: memset failed");
  if (is_u8) {
    ProfScope prof(PCUDA_FAM_POINTWISE, (double)elems, (hipStream_t)s);
    hipLaunchKernelGGL(histbank_count_u8_kernel, dim3(r * c), dim3(kU8Threads), 0, (hipStream_t)s, a);
    PCUDA_CHECK_LAUNCH("histbank_count_u8_kernel");
    return PCUDA_OK;
  }
  // bytes: the references read once, the keys written once and moved by four passes (a load and a store each)
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)elems * 4.0 * 10.0, (hipStream_t)s);
  hipLaunchKernelGGL(histbank_sort_kernel, dim3(r * c), dim3(kSortThreads), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("histbank_sort_kernel");
  return PCUDA_OK;
}

extern "C" size_t pcuda_match_hist_bank_workspace_size(int b, int h, int w, int c, int is_u8) {
  if (b <= 0 || h <= 0 || w <= 0 || c <= 0 || is_u8) return 0;
  return round16((size_t)b * c * 2 * (size_t)h * w * sizeof(uint32_t));      // per image plane: the two key buffers of the ping-pong
}

extern "C" int pcuda_match_hist_bank(const void* in, void* out, int is_u8, int b, int h, int w, int c, const void* bank, int r,
                                     int rh, int rw, const int* ref_index, void* workspace, size_t workspace_bytes,
                                     pcuda_stream_t s) {
  if (bad_plane_dims(b, h, w, c)) PCUDA_FAIL(PCUDA_E_BADARG, "match_hist_bank: bad dims (1..4 channels, sides up to 32768)");
  if (bad_plane_dims(r, rh, rw, c) || r < 1 || rh < 1 || rw < 1)
    PCUDA_FAIL(PCUDA_E_BADARG, "match_hist_bank: bad bank dims (at least one reference, sides 1..32768)");
  if (!bank || !ref_index) PCUDA_FAIL(PCUDA_E_BADARG, "match_hist_bank: null bank or ref_index");
  if (((uintptr_t)bank & 15) != 0) PCUDA_FAIL(PCUDA_E_WORKSPACE, "match_hist_bank: bank not 16-byte aligned");
  if (b == 0 || h == 0 || w == 0) return PCUDA_OK;
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "match_hist_bank: null pointer");
  if (in == out) PCUDA_FAIL(PCUDA_E_BADARG, "match_hist_bank: in == out (the input is never written)");
  const size_t need = pcuda_match_hist_bank_workspace_size(b, h, w, c, is_u8);
  if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "match_hist_bank: workspace too small (or not 16-byte aligned)");
  BankMatchArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.keys = static_cast<uint32_t*>(workspace);
  a.bank = static_cast<const uint32_t*>(bank); a.ref_index = ref_index;
  a.n = h * w; a.c = c; a.m = rh * rw; a.r = r;
  const size_t elems = (size_t)b * h * w * c;
  if (is_u8) {
    ProfScope prof(PCUDA_FAM_POINTWISE, 3.0 * (double)elems, (hipStream_t)s);
    hipLaunchKernelGGL(histbank_match_u8_kernel, dim3(b * c), dim3(kU8Threads), 0, (hipStream_t)s, a);
    PCUDA_CHECK_LAUNCH("histbank_match_u8_kernel");
    return PCUDA_OK;
  }
  // bytes: the keys written once and moved by four passes (a load and a store each), the input read twice, the output
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)elems * 4.0 * 12.0, (hipStream_t)s);
  hipLaunchKernelGGL(histbank_image_sort_kernel, dim3(b * c), dim3(kSortThreads), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("histbank_image_sort_kernel");
  hipLaunchKernelGGL(histbank_lookup_kernel, dim3(cdiv((long long)a.n * c, 256), b), dim3(256), 0, (hipStream_t)s, a);
  PCUDA_CHECK_LAUNCH("histbank_lookup_kernel");
  return PCUDA_OK;
}
