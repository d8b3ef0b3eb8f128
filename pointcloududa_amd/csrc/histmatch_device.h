// Device code shared by histmatch.hip (one fixed template, f10) and histmatch_bank.hip (a bank of references on the device):
// the order-preserving key of an fp32 value, the wave's digit peers, the one-workgroup LSD radix sort of a plane's keys and
// np.interp for one quantile.  Include after common.h, inside the including file's anonymous namespace.
#pragma once

constexpr int kMaxC = 4;
constexpr int kSortThreads = 1024;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kKeysPerLane = 4;                // a wave takes 64 * kKeysPerLane consecutive keys of a tile
constexpr int kSortTile = kSortThreads * kKeysPerLane;
constexpr int kU8Threads = 1024;

__device__ __forceinline__ uint32_t float_key(float v) {
  uint32_t u = __builtin_bit_cast(uint32_t, v);
  if (u == 0x80000000u) u = 0u;                                  // -0.0 == +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the lanes of this wave that are active and hold the same 8-bit digit (eight ballots); every lane of the wave calls it
__device__ __forceinline__ unsigned long long digit_peers(unsigned d, bool active) {
  unsigned long long peers = __ballot(active);
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const bool set = (d >> bit) & 1u;
    const unsigned long long m = __ballot(set);
    peers &= set ? m : ~m;
  }
  return peers;
}

// np.interp(q, tq[0..len), tv[0..len)) for one q; len >= 1
__device__ __forceinline__ double interp_table(double q, const double* tq, const double* tv, int len) {
  int lo = 0, hi = len;                                          // upper bound of q in tq
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double* p = tq + mid;
    const double v = *p;
    if (v <= q) lo = mid + 1; else hi = mid;
    PCUDA_KEEP(p);
  }
  const int j = lo - 1;
  const int j0 = j < 0 ? 0 : j, j1 = j0 + 1 < len ? j0 + 1 : len - 1;
  const double *pq0 = tq + j0, *pq1 = tq + j1, *pv0 = tv + j0, *pv1 = tv + j1;
  const double q0 = *pq0, q1 = *pq1, v0 = *pv0, v1 = *pv1;
  double r;
  if (j < 0 || j >= len - 1 || q0 == q) {
    r = v0;                                                      // (j == len - 1: j0 = len - 1)
  } else {
    const double slope = (v1 - v0) / (q1 - q0);
    r = slope * (q - q0) + v0;
  }
  PCUDA_KEEP(pq0); PCUDA_KEEP(pq1); PCUDA_KEEP(pv0); PCUDA_KEEP(pv1);
  return r;
}

// The keys of one plane (n values of stride c behind src), sorted: a workgroup of kSortThreads lanes, all of them calling.  A
// first sweep writes the keys to buf0 and counts all four 8-bit digit histograms in LDS, then four LSD passes ping-pong buf0 ->
// buf1 -> buf0 -> buf1 -> buf0: the sorted plane ends in buf0.  Returns whether THIS lane read a non-finite value.
__device__ __forceinline__ bool sort_plane_keys(const float* src, int c, int n, uint32_t* buf0, uint32_t* buf1) {
  __shared__ unsigned s_hist[4 * 256];                 // the four digit histograms of the plane
  __shared__ unsigned s_wcnt[kSortWaves * 256];        // per wave and digit: keys of the tile (zero between two tiles)
  __shared__ unsigned s_woff[kSortWaves * 256];        // per wave and digit: where the wave's first such key goes
  __shared__ unsigned s_base[256];                     // per digit: where the next tile's first such key goes
  __shared__ unsigned s_tot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool nonfinite = false;

  for (int i = tid; i < 4 * 256; i += kSortThreads) s_hist[i] = 0;
  for (int i = tid; i < kSortWaves * 256; i += kSortThreads) s_wcnt[i] = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kSortThreads) {            // (the trip count is the same for every lane: ballots)
    const int i = base + tid;
    const bool active = i < n;
    const float* p = src + (long long)(active ? i : n - 1) * c;
    const float v = *p;
    PCUDA_KEEP(p);
    const uint32_t key = float_key(v);
    nonfinite |= (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) == 0x7F800000u;   // (unused by a caller: no code)
    // sign and exponent: a few digits hold a whole image, so a wave adds each of them up first (one atomic per digit and wave)
    const unsigned long long peers = digit_peers(key >> 24, active);
    if (active) {
      buf0[i] = key;
      atomicAdd(&s_hist[key & 255u], 1u);
      atomicAdd(&s_hist[256 + ((key >> 8) & 255u)], 1u);
      atomicAdd(&s_hist[512 + ((key >> 16) & 255u)], 1u);
      if ((peers & ((1ull << lane) - 1ull)) == 0) atomicAdd(&s_hist[768 + (key >> 24)], (unsigned)__popcll(peers));
    }
  }
  __syncthreads();      // (the keys are read back by other lanes of this workgroup: the barrier orders its global stores)

  for (int pass = 0; pass < 4; ++pass) {
    const uint32_t* from = (pass & 1) ? buf1 : buf0;
    uint32_t* to = (pass & 1) ? buf0 : buf1;
    const int shift = 8 * pass;
    // exclusive scan of the pass's histogram: the digit bases
    unsigned mine = 0, incl = 0;
    if (tid < 256) {                                   // (waves 0..3, whole)
      mine = s_hist[pass * 256 + tid];
      incl = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
      }
      if (lane == 63) s_tot[wave] = incl;
    }
    __syncthreads();
    if (tid < 256) {
      unsigned before = 0;
      for (int k = 0; k < wave; ++k) before += s_tot[k];
      s_base[tid] = before + incl - mine;
    }
    __syncthreads();

    for (int base = 0; base < n; base += kSortTile) {               // (the trip count is the same for every lane)
      uint32_t key[kKeysPerLane];
      unsigned rank[kKeysPerLane];                                  // among the wave's keys of the same digit; ~0u: no key
#pragma unroll
      for (int r = 0; r < kKeysPerLane; ++r) {
        const int i = base + (wave * kKeysPerLane + r) * 64 + lane;
        const bool active = i < n;
        const uint32_t* p = from + (active ? i : n - 1);
        key[r] = *p;
        PCUDA_KEEP(p);
        const unsigned d = (key[r] >> shift) & 255u;
        const unsigned long long peers = digit_peers(d, active);
        const unsigned below = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
        unsigned seen = 0;                                          // keys of this digit in the wave's earlier rounds
        if (active && below == 0) seen = atomicAdd(&s_wcnt[wave * 256 + d], (unsigned)__popcll(peers));   // (this wave's own counter)
        const int leader = active ? __ffsll((long long)peers) - 1 : lane;
        seen = __shfl(seen, leader);
        rank[r] = active ? seen + below : ~0u;
        __builtin_amdgcn_wave_barrier();                            // (rounds stay in order: the next one reads these counters)
      }
      __syncthreads();
      if (tid < 256) {
        unsigned cnt[kSortWaves];
#pragma unroll
        for (int k = 0; k < kSortWaves; ++k) cnt[k] = s_wcnt[k * 256 + tid];
        unsigned run = s_base[tid];
#pragma unroll
        for (int k = 0; k < kSortWaves; ++k) {
          s_woff[k * 256 + tid] = run;
          s_wcnt[k * 256 + tid] = 0;
          run += cnt[k];
        }
        s_base[tid] = run;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kKeysPerLane; ++r) {
        if (rank[r] != ~0u) {
          const unsigned pos = s_woff[wave * 256 + ((key[r] >> shift) & 255u)] + rank[r];
          if (pos < (unsigned)n) to[pos] = key[r];                  // (always true for a consistent histogram)
        }
      }
      // the next tile writes s_wcnt only (read above, before the barrier) until its own first barrier
    }
    __syncthreads();      // the pass's stores before the next pass's loads
  }
  return nonfinite;
}
