// Evaluation metrics of the reference's evaluate scripts (medpy.metric.binary dc / hd / asd, utils.py's
// keep_largest_connected_components) on integer label volumes [Z][H][W] (2-D inputs: Z = 1).
//
// Surface metrics, per class value c (A = pred == c, B = gt == c), five launches for every class at once:
//   1. border pass: border(X) = X & ~erode(X) (footprint of the connectivity, outside = background) for pred and gt,
//      one 16-bit mask per voxel (bit k: border of pred class k, bit 8 + k: of gt class k), and the Dice counts
//      |A|, |B|, |A.B| as integer per-block partials;
//   2. exact separable EDT (Felzenszwalb-Huttenlocher lower envelope of parabolas), one pass per axis W, H, Z; field
//      2k is the transform of ~border(A_k), field 2k+1 of ~border(B_k); every field's lines ride in the same launch;
//   3. the last axis pass evaluates each field only at the other mask's border voxels: max d^2 (64-bit integer atomic
//      max, order-free), sum of d and count as per-block partials;
//   4. a one-block kernel sums the partials in a fixed order and writes out[k][8].
// Unit spacing keeps squared distances in int32 end to end and takes the sqrt in fp64 (what scipy computes from its
// integer feature offsets); anisotropic spacing carries fp64 squared distances.
//
// Extended rows (pcuda_surface_metrics_ext: + percentile Hausdorff distance, assd, border counts).  The last axis pass
// (MODE 3) also stores d^2 at every border voxel of the eval mask: T itself is the key (int32, or the fp64 whose bit
// pattern orders like its value).  Two order statistics per class (ranks lo and hi of numpy's linear percentile) over
// the union of the class's two fields are then selected exactly, MSB first, 8 bits per pass: a histogram kernel (LDS
// histogram per block and query, flushed with integer atomic adds: the bins do not depend on block scheduling) and a
// one-wave-per-query kernel that finds the rank's bin, extends the query's key prefix and narrows its rank.  The two
// queries are tracked apart (they may part at any digit).  sizeof(T) passes: 4 (int) or 8 (double), every class and both
// queries in the same launches, no host round trip.  Launches: border, ndim axis passes, 2 * sizeof(T) select, final
// = 13 / 21 for a 3-D volume at unit / other spacing (12 / 20 in 2-D), after two memsets.
//
// Largest connected components: union-find on equal labels with face connectivity; the atomicMin hook makes every
// root its component's minimum linear index (= the raster-first voxel), so a 64-bit atomic max on
// (size << 32) | (0xFFFFFFFF - root) picks, per label, the largest component and among equal sizes the raster-first.
//
// Only vector stores and integer atomics; every in-flight load's address stays alive (PCUDA_KEEP, VMEM address rule,
// common.h): these are small-LDS kernels that share CUs.
#include "common.h"

#include <math.h>

namespace {

constexpr int EM_MAXCLS = 8;
constexpr int EM_MAXDIM = 16384;          // every dimension; d^2 <= 3 * 16383^2 < 2^31
constexpr int EM_BORDER_BLOCKS = 1024;    // grid of the border pass (its partials: [blocks][ncls][3])
constexpr int EM_LINE_THREADS = 64;       // one wave per block in the axis passes (wave-level partial reduction)
constexpr int EM_CCL_RUN = 16;            // consecutive voxels per thread in the size histogram

struct EmClasses {
  int c[EM_MAXCLS];
  int n;
};

struct EmLines {             // the lines of one axis: line l starts at (l / inner) * outer_stride + l % inner
  int n;                     // line length
  long long stride;          // element stride along the line
  long long inner, outer_stride, nlines;
};

size_t em_align(size_t b) { return (b + 255) & ~(size_t)255; }

template <typename T>
__device__ __forceinline__ unsigned em_eq_bits(T v, const EmClasses& cls) {
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < EM_MAXCLS; ++k)
    if (k < cls.n && (long long)v == (long long)cls.c[k]) m |= 1u << k;
  return m;
}

// ------------------------------------------------------------------------------------------------ border pass
template <typename T>
__global__ __launch_bounds__(256) void em_border_kernel(const T* __restrict__ pred, const T* __restrict__ gt, int Z, int H,
                                                        int W, int ndim, int conn, EmClasses cls,
                                                        uint16_t* __restrict__ bmask, unsigned* __restrict__ cnt_part) {
  __shared__ unsigned h[EM_MAXCLS * 3];
  if (threadIdx.x < EM_MAXCLS * 3) h[threadIdx.x] = 0;
  __syncthreads();
  const long long numel = (long long)Z * H * W, hw = (long long)H * W;
  unsigned ca[EM_MAXCLS] = {}, cb[EM_MAXCLS] = {}, cab[EM_MAXCLS] = {};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < numel; i += 256ll * gridDim.x) {
    const T* pp = pred + i;
    const T* pg = gt + i;
    const unsigned ma = em_eq_bits(*pp, cls), mb = em_eq_bits(*pg, cls);
    PCUDA_KEEP(pp); PCUDA_KEEP(pg);
    unsigned alla = ma, allb = mb;
    if (ma | mb) {
      const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / hw);
      const int dz0 = ndim == 3 ? -1 : 0, dz1 = ndim == 3 ? 1 : 0;
      for (int dz = dz0; dz <= dz1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int nz = (dz != 0) + (dy != 0) + (dx != 0);
            if (nz == 0 || nz > conn) continue;
            const int qx = x + dx, qy = y + dy, qz = z + dz;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H || qz < 0 || qz >= Z) {
              alla = 0; allb = 0;                       // outside the array: background (border_value = 0)
              continue;
            }
            const long long q = (long long)qz * hw + (long long)qy * W + qx;
            const T* qa = pred + q;
            const T* qb = gt + q;
            alla &= em_eq_bits(*qa, cls);
            allb &= em_eq_bits(*qb, cls);
            PCUDA_KEEP(qa); PCUDA_KEEP(qb);
          }
    }
    bmask[i] = (uint16_t)((ma & ~alla) | ((mb & ~allb) << 8));
#pragma unroll
    for (int k = 0; k < EM_MAXCLS; ++k) {
      ca[k] += (ma >> k) & 1u;
      cb[k] += (mb >> k) & 1u;
      cab[k] += (ma & mb) >> k & 1u;
    }
  }
#pragma unroll
  for (int k = 0; k < EM_MAXCLS; ++k)
    if (k < cls.n) {
      if (ca[k]) atomicAdd(&h[3 * k + 0], ca[k]);
      if (cb[k]) atomicAdd(&h[3 * k + 1], cb[k]);
      if (cab[k]) atomicAdd(&h[3 * k + 2], cab[k]);
    }
  __syncthreads();
  if (threadIdx.x < 3 * cls.n) cnt_part[(long long)blockIdx.x * 3 * cls.n + threadIdx.x] = h[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ EDT axis passes
// T = int (unit spacing: exact integer squared distances) or double (anisotropic spacing).
template <typename T> struct EmVal;
template <> struct EmVal<int> {
  static __device__ __forceinline__ int inf() { return 0x7fffffff; }
  static __device__ __forceinline__ int term(int d, double) { return d * d; }
  // abscissa where the parabola of q (> p) starts to lie at or below the one of p
  static __device__ __forceinline__ double isect(int p, int fp, int q, int fq, double) {
    return (double)(((long long)fq + (long long)q * q) - ((long long)fp + (long long)p * p)) / (2.0 * (q - p));
  }
  static __device__ __forceinline__ unsigned long long key(int d) { return (unsigned long long)d; }
};
template <> struct EmVal<double> {
  static __device__ __forceinline__ double inf() { return __builtin_huge_val(); }
  static __device__ __forceinline__ double term(int d, double sp) {
    const double t = (double)d * sp;
    return t * t;
  }
  static __device__ __forceinline__ double isect(int p, double fp, int q, double fq, double sp) {
    const double w = sp * sp;
    return ((fq + w * ((double)q * q)) - (fp + w * ((double)p * p))) / (2.0 * w * (q - p));
  }
  // non-negative doubles order like their bit patterns
  static __device__ __forceinline__ unsigned long long key(double d) { return __builtin_bit_cast(unsigned long long, d); }
};

// field f: the transform of ~border(target) evaluated at border(eval); fields 2k / 2k+1 target pred / gt of class k
__device__ __forceinline__ int em_target_bit(int f) { return (f & 1) ? 8 + (f >> 1) : (f >> 1); }
__device__ __forceinline__ int em_eval_bit(int f) { return (f & 1) ? (f >> 1) : 8 + (f >> 1); }

// MODE 0: first axis, input = the border masks (0 on the target's border, inf elsewhere), writes fout
// MODE 1: middle axis, fin -> fout
// MODE 2: last axis, fin -> (max d^2, sum d, count) at the eval mask's border voxels, no field written
// MODE 3: MODE 2, and d^2 stored to fout at those voxels only (the select's keys; the other entries are never read).
//         A field whose target is empty (all inf; its class is flagged) stores inf there and still counts them, so
//         that the counts are the border voxel counts for every class
template <typename T, int MODE>
__global__ __launch_bounds__(EM_LINE_THREADS) void em_edt_pass_kernel(
    const uint16_t* __restrict__ bmask, const T* __restrict__ fin, T* __restrict__ fout, int* __restrict__ vbuf,
    long long numel, EmLines ln, double sp, unsigned long long* __restrict__ maxkey, double* __restrict__ psum,
    unsigned* __restrict__ pcnt) {
  typedef EmVal<T> V;
  const int f = blockIdx.y;
  const long long l = blockIdx.x * (long long)EM_LINE_THREADS + threadIdx.x;
  const int tb = em_target_bit(f), eb = em_eval_bit(f);
  const T* in = fin + (long long)f * numel;
  T* out = fout + (long long)f * numel;
  int* vb = vbuf + (long long)f * numel;      // stack of the line's envelope: vb[k * nlines + l] (lanes coalesce)
  unsigned long long mx = 0;
  double sum = 0.0;
  unsigned cnt = 0;
  if (l < ln.nlines) {
    const long long base = (l / ln.inner) * ln.outer_stride + l % ln.inner;
    const int n = ln.n;
    auto load = [&](int q) -> T {
      const long long o = base + q * ln.stride;
      if constexpr (MODE == 0) {
        const uint16_t* pm = bmask + o;
        const unsigned b = *pm;
        PCUDA_KEEP(pm);
        return ((b >> tb) & 1u) ? (T)0 : V::inf();
      } else {
        const T* pi = in + o;
        const T v = *pi;
        PCUDA_KEEP(pi);
        return v;
      }
    };
    auto vload = [&](int k) -> int {
      const int* pv = vb + (long long)k * ln.nlines + l;
      const int v = *pv;
      PCUDA_KEEP(pv);
      return v;
    };
    // lower envelope of the parabolas y = f(p) + (x - p)^2 over the finite f(p)
    int k = -1, vk = 0;
    T fk = 0;
    double zk = -__builtin_huge_val();       // where the top parabola starts to be the envelope
    for (int q = 0; q < n; ++q) {
      const T fq = load(q);
      if (fq == V::inf()) continue;
      if (k >= 0) {
        double s = V::isect(vk, fk, q, fq, sp);
        while (s <= zk) {                    // the top parabola is nowhere strictly below: pop it (zk = -inf at k = 0)
          --k;
          vk = vload(k);
          fk = load(vk);
          if (k > 0) {
            const int vp = vload(k - 1);
            zk = V::isect(vp, load(vp), vk, fk, sp);
          } else {
            zk = -__builtin_huge_val();
          }
          s = V::isect(vk, fk, q, fq, sp);
        }
        zk = s;
      }
      ++k;
      vb[(long long)k * ln.nlines + l] = q;
      vk = q;
      fk = fq;
    }
    // read the envelope back along the line
    if (k >= 0) {
      int j = 0, vj = vload(0), vn = 0;
      T fj = load(vj), fn = 0;
      double zn = __builtin_huge_val();
      if (k > 0) { vn = vload(1); fn = load(vn); zn = V::isect(vj, fj, vn, fn, sp); }
      for (int q = 0; q < n; ++q) {
        while (zn < q) {
          ++j; vj = vn; fj = fn;
          if (j < k) { vn = vload(j + 1); fn = load(vn); zn = V::isect(vj, fj, vn, fn, sp); }
          else zn = __builtin_huge_val();
        }
        const T d = fj + V::term(q - vj, sp);
        const long long o = base + q * ln.stride;
        if constexpr (MODE < 2) {
          out[o] = d;
        } else {
          const uint16_t* pm = bmask + o;
          const unsigned b = *pm;
          PCUDA_KEEP(pm);
          if ((b >> eb) & 1u) {
            const unsigned long long kk = V::key(d);
            mx = kk > mx ? kk : mx;
            sum += sqrt((double)d);
            ++cnt;
            if constexpr (MODE == 3) out[o] = d;
          }
        }
      }
    } else if (MODE < 2) {
      for (int q = 0; q < n; ++q) out[base + q * ln.stride] = V::inf();
    } else if (MODE == 3) {
      for (int q = 0; q < n; ++q) {
        const long long o = base + q * ln.stride;
        const uint16_t* pm = bmask + o;
        const unsigned b = *pm;
        PCUDA_KEEP(pm);
        if ((b >> eb) & 1u) {
          out[o] = V::inf();
          ++cnt;
        }
      }
    }
  }
  if constexpr (MODE >= 2) {                 // one wave per block: fixed-order shuffle tree, one partial per block
    sum = wave_sum_d(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long om = __shfl_xor(mx, o, 64);
      mx = om > mx ? om : mx;
      cnt += __shfl_xor(cnt, o, 64);
    }
    if (threadIdx.x == 0) {
      psum[(long long)f * gridDim.x + blockIdx.x] = sum;
      pcnt[(long long)f * gridDim.x + blockIdx.x] = cnt;
      if (mx) atomicMax(&maxkey[f], mx);
    }
  }
}

// out[k][8] = dice, hd, asd(pred->gt), asd(gt->pred), |A|, |B|, |A.B|, flags (1: A empty, 2: B empty); hd / asd NaN
// when a flag is set
struct EmRow {                 // what the extended row needs beyond the eight columns
  double s[2];
  unsigned long long c[2];
  int flags;
};

// the eight columns of class k to o[0..7]: one thread, every sum in index order
template <typename T>
__device__ __forceinline__ EmRow em_final_row(const unsigned* __restrict__ cnt_part, int nbb,
                                              const unsigned long long* __restrict__ maxkey, const double* __restrict__ psum,
                                              const unsigned* __restrict__ pcnt, int nb2, int ncls, int k, double* o) {
  unsigned long long a = 0, b = 0, ab = 0;
  for (int i = 0; i < nbb; ++i) {
    const unsigned* p = cnt_part + (long long)i * 3 * ncls + 3 * k;
    a += p[0]; b += p[1]; ab += p[2];
    PCUDA_KEEP(p);
  }
  double s[2] = {0.0, 0.0};
  unsigned long long c[2] = {0, 0};
  for (int d = 0; d < 2; ++d) {              // d = 0: field 2k+1 (pred border -> gt), d = 1: field 2k (gt -> pred)
    const int f = 2 * k + 1 - d;
    for (int i = 0; i < nb2; ++i) {
      const double* ps = psum + (long long)f * nb2 + i;
      const unsigned* pc = pcnt + (long long)f * nb2 + i;
      s[d] += *ps; c[d] += *pc;
      PCUDA_KEEP(ps); PCUDA_KEEP(pc);
    }
  }
  const double dsum = (double)a + (double)b;
  const int flags = (a == 0 ? 1 : 0) | (b == 0 ? 2 : 0);
  const unsigned long long m0 = maxkey[2 * k], m1 = maxkey[2 * k + 1];
  const unsigned long long mk = m0 > m1 ? m0 : m1;
  const double d2 = sizeof(T) == sizeof(int) ? (double)mk : __builtin_bit_cast(double, mk);
  const double nan = __builtin_nan("");
  o[0] = dsum > 0.0 ? 2.0 * (double)ab / dsum : 0.0;
  o[1] = flags ? nan : sqrt(d2);
  o[2] = flags ? nan : s[0] / (double)c[0];
  o[3] = flags ? nan : s[1] / (double)c[1];
  o[4] = (double)a;
  o[5] = (double)b;
  o[6] = (double)ab;
  o[7] = (double)flags;
  return EmRow{{s[0], s[1]}, {c[0], c[1]}, flags};
}

template <typename T>
__global__ void em_final_kernel(const unsigned* __restrict__ cnt_part, int nbb, const unsigned long long* __restrict__ maxkey,
                                const double* __restrict__ psum, const unsigned* __restrict__ pcnt, int nb2, int ncls,
                                double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= ncls) return;
  em_final_row<T>(cnt_part, nbb, maxkey, psum, pcnt, nb2, ncls, k, out + 8 * k);
}

// ------------------------------------------------------------------------------------------------ percentile select
constexpr int EM_SEL_BITS = 8;                       // digit width: 256 bins, 2 KiB of LDS for a block's two histograms
constexpr int EM_SEL_BINS = 1 << EM_SEL_BITS;
constexpr int EM_SEL_BLOCKS = 256;                   // grid.x of the histogram kernel (grid-stride over the voxels)

struct EmSel {                                       // one query: class k, q = 0 (rank lo) / 1 (rank hi)
  unsigned long long prefix;                         // the digits found so far, in place; after the last pass: the key
  unsigned long long rank;                           // rank among the keys that share the prefix
};

// numpy.percentile's 'linear' method on n sorted values: v = (n - 1) * quant, lo = floor(v), hi = min(lo + 1, n - 1),
// t = v - lo, one fp64 rounding per operation
__device__ __forceinline__ void em_ranks(unsigned long long n, double quant, unsigned long long* lo, unsigned long long* hi,
                                         double* t) {
#pragma clang fp contract(off)
  if (n == 0) {
    *lo = 0; *hi = 0; *t = 0.0;
    return;
  }
  const double v = (double)(n - 1) * quant;
  const double fl = floor(v);
  const unsigned long long l = (unsigned long long)fl;       // quant <= 1: l <= n - 1
  *lo = l;
  *hi = l + 1 < n ? l + 1 : n - 1;
  *t = v - fl;
}

// numpy's _lerp: a + (b - a) * t, and b - (b - a) * (1 - t) where t >= 0.5; no FMA (the products are rounded first)
__device__ __forceinline__ double em_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
  const double diff = b - a;
  double p = diff * t;
  asm volatile("" : "+v"(p));
  double r = a + p;
  if (t >= 0.5) {
    double p2 = diff * (1.0 - t);
    asm volatile("" : "+v"(p2));
    r = b - p2;
  }
  return r;
}

// pass with digit shift `shift`: hist[k][q][bin] += the live keys of class k (fields 2k and 2k + 1 at their eval masks'
// border voxels) that share query q's prefix above the digit.  grid (EM_SEL_BLOCKS, ncls)
template <typename T>
__global__ __launch_bounds__(256) void em_sel_hist_kernel(const uint16_t* __restrict__ bmask, const T* __restrict__ keys,
                                                          long long numel, int shift, const EmSel* __restrict__ sel,
                                                          unsigned* __restrict__ hist) {
  typedef EmVal<T> V;
  __shared__ unsigned h[2 * EM_SEL_BINS];
  for (int i = threadIdx.x; i < 2 * EM_SEL_BINS; i += 256) h[i] = 0;
  __syncthreads();
  const int k = blockIdx.y;
  const EmSel* ps = sel + 2 * k;
  const unsigned long long p0 = ps[0].prefix, p1 = ps[1].prefix;
  PCUDA_KEEP(ps);
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < numel; i += 256ll * gridDim.x) {
    const uint16_t* pm = bmask + i;
    const unsigned b = *pm;
    PCUDA_KEEP(pm);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int f = 2 * k + d;
      if ((b >> em_eval_bit(f)) & 1u) {
        const T* pk = keys + (long long)f * numel + i;
        const unsigned long long key = V::key(*pk);
        PCUDA_KEEP(pk);
        const unsigned bin = (unsigned)(key >> shift) & (EM_SEL_BINS - 1);
        // (two shifts: shift + EM_SEL_BITS is the key's width in the first pass)
        if ((((key ^ p0) >> shift) >> EM_SEL_BITS) == 0) atomicAdd(&h[bin], 1u);
        if ((((key ^ p1) >> shift) >> EM_SEL_BITS) == 0) atomicAdd(&h[EM_SEL_BINS + bin], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* g = hist + (long long)k * 2 * EM_SEL_BINS;
  for (int i = threadIdx.x; i < 2 * EM_SEL_BINS; i += 256)
    if (h[i]) atomicAdd(g + i, h[i]);
}

// one wave per query (grid 2 * ncls): the bin that holds the query's rank becomes its next digit.  first: the ranks
// come from the per-block counts (n = c0 + c1, integer sums)
__global__ __launch_bounds__(64) void em_sel_narrow_kernel(const unsigned* __restrict__ hist, int shift, int first,
                                                           const unsigned* __restrict__ pcnt, int nb2, double quant,
                                                           EmSel* __restrict__ sel) {
  const int k = blockIdx.x >> 1, q = blockIdx.x & 1, lane = threadIdx.x;
  EmSel* ps = sel + blockIdx.x;
  unsigned long long rank;
  if (first) {
    unsigned long long n = 0;
    for (int f = 2 * k + 1; f >= 2 * k; --f)
      for (int i = lane; i < nb2; i += 64) {
        const unsigned* pc = pcnt + (long long)f * nb2 + i;
        n += *pc;
        PCUDA_KEEP(pc);
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    unsigned long long lo, hi;
    double t;
    em_ranks(n, quant, &lo, &hi, &t);
    rank = q ? hi : lo;
  } else {
    rank = ps->rank;
  }
  const unsigned long long prefix = ps->prefix;
  PCUDA_KEEP(ps);
  // lane j: bins 4j .. 4j + 3; exclusive prefix sums across the wave
  const unsigned* ph = hist + (long long)blockIdx.x * EM_SEL_BINS + 4 * lane;
  unsigned long long c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = ph[j];
  PCUDA_KEEP(ph);
  const unsigned long long mine = c[0] + c[1] + c[2] + c[3];
  unsigned long long incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  unsigned long long excl = incl - mine;
  if (rank >= excl && rank < incl) {             // exactly one lane (none when the class has no live key)
    int j = 0;
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (j == u && rank >= excl + c[u]) { excl += c[u]; j = u + 1; }
    EmSel r;
    r.prefix = prefix | ((unsigned long long)(4 * lane + j) << shift);
    r.rank = rank - excl;
    *ps = r;
  }
}

// out[k][12]: the eight columns of em_final_kernel, the percentile of the pooled distances (em_ranks / em_lerp on the
// sqrt of the two selected keys), assd = (asd(pred->gt) + asd(gt->pred)) / 2, and the border voxel counts of pred and gt;
// columns 8 and 9 NaN when a flag is set
template <typename T>
__global__ void em_final_ext_kernel(const unsigned* __restrict__ cnt_part, int nbb, const unsigned long long* __restrict__ maxkey,
                                    const double* __restrict__ psum, const unsigned* __restrict__ pcnt, int nb2, int ncls,
                                    const EmSel* __restrict__ sel, double quant, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= ncls) return;
  double* o = out + 12 * k;
  const EmRow r = em_final_row<T>(cnt_part, nbb, maxkey, psum, pcnt, nb2, ncls, k, o);
  unsigned long long lo, hi;
  double t;
  em_ranks(r.c[0] + r.c[1], quant, &lo, &hi, &t);
  const EmSel* ps = sel + 2 * k;
  const unsigned long long k0 = ps[0].prefix, k1 = ps[1].prefix;
  PCUDA_KEEP(ps);
  const double d0 = sizeof(T) == sizeof(int) ? (double)k0 : __builtin_bit_cast(double, k0);
  const double d1 = sizeof(T) == sizeof(int) ? (double)k1 : __builtin_bit_cast(double, k1);
  const double nan = __builtin_nan("");
  o[8] = r.flags ? nan : em_lerp(sqrt(d0), sqrt(d1), t);
  o[9] = r.flags ? nan : (o[2] + o[3]) / 2.0;
  o[10] = (double)r.c[0];
  o[11] = (double)r.c[1];
}

// ------------------------------------------------------------------------------------------------ connected components
template <typename T>
__device__ __forceinline__ int em_label(const T* mask, long long i, int nl) {
  const T* p = mask + i;
  const long long v = (long long)*p;
  PCUDA_KEEP(p);
  return (v >= 1 && v <= nl) ? (int)v : 0;
}

__device__ __forceinline__ int em_parent(int* par, int x) {      // agent-scope load: sees the other blocks' hooks
  int* p = par + x;
  const int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  PCUDA_KEEP(p);
  return v;
}
__device__ __forceinline__ int em_find(int* par, int x) {
  int p = em_parent(par, x);
  while (p != x) { x = p; p = em_parent(par, x); }
  return x;
}
// hook the larger root under the smaller one: a component's root ends as its minimum linear index
__device__ __forceinline__ void em_unite(int* par, int a, int b) {
  a = em_find(par, a);
  b = em_find(par, b);
  while (a != b) {
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + b, a);
    if (old == b) break;
    a = em_find(par, a);
    b = em_find(par, old);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void em_ccl_init_kernel(const T* __restrict__ mask, long long numel, int nl,
                                                          int* __restrict__ par) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i < numel) par[i] = em_label(mask, i, nl) ? (int)i : -1;
}

template <typename T>
__global__ __launch_bounds__(256) void em_ccl_merge_kernel(const T* __restrict__ mask, int Z, int H, int W, int nl,
                                                           int* par) {
  const long long numel = (long long)Z * H * W, hw = (long long)H * W;
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= numel) return;
  const int v = em_label(mask, i, nl);
  if (!v) return;
  const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / hw);
  if (x + 1 < W && em_label(mask, i + 1, nl) == v) em_unite(par, (int)i, (int)(i + 1));
  if (y + 1 < H && em_label(mask, i + W, nl) == v) em_unite(par, (int)i, (int)(i + W));
  if (z + 1 < Z && em_label(mask, i + hw, nl) == v) em_unite(par, (int)i, (int)(i + hw));
}

__global__ __launch_bounds__(256) void em_ccl_compress_kernel(long long numel, int* par) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= numel) return;
  int* pi = par + i;
  const int p = *pi;
  PCUDA_KEEP(pi);
  if (p >= 0 && p != (int)i) {
    int r = p, q;
    for (;;) {
      const int* pr = par + r;
      q = *pr;
      PCUDA_KEEP(pr);
      if (q == r) break;
      r = q;
    }
    *pi = r;
  }
}

// size[root] += voxels; runs of one root along memory share one atomic
__global__ __launch_bounds__(256) void em_ccl_size_kernel(const int* __restrict__ par, long long numel,
                                                          unsigned* __restrict__ size) {
  const long long i0 = (blockIdx.x * 256ll + threadIdx.x) * EM_CCL_RUN;
  if (i0 >= numel) return;
  const long long i1 = i0 + EM_CCL_RUN < numel ? i0 + EM_CCL_RUN : numel;
  int cur = -1;
  unsigned c = 0;
  for (long long i = i0; i < i1; ++i) {
    const int* pi = par + i;
    const int r = *pi;
    PCUDA_KEEP(pi);
    if (r != cur) {
      if (cur >= 0) atomicAdd(size + cur, c);
      cur = r;
      c = 0;
    }
    ++c;
  }
  if (cur >= 0) atomicAdd(size + cur, c);
}

template <typename T>
__global__ __launch_bounds__(256) void em_ccl_best_kernel(const T* __restrict__ mask, const int* __restrict__ par,
                                                          const unsigned* __restrict__ size, long long numel, int nl,
                                                          unsigned long long* __restrict__ best) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= numel) return;
  const int* pi = par + i;
  const int r = *pi;
  PCUDA_KEEP(pi);
  if (r != (int)i) return;
  const unsigned* ps = size + i;
  const unsigned long long key = ((unsigned long long)*ps << 32) | (0xFFFFFFFFull - (unsigned)i);
  PCUDA_KEEP(ps);
  atomicMax(best + em_label(mask, i, nl), key);
}

template <typename T>
__global__ __launch_bounds__(256) void em_ccl_write_kernel(const T* __restrict__ mask, const int* __restrict__ par,
                                                           const unsigned long long* __restrict__ best, long long numel,
                                                           int nl, uint8_t* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= numel) return;
  const int* pi = par + i;
  const int r = *pi;
  PCUDA_KEEP(pi);
  int o = 0;
  if (r >= 0) {
    const int v = em_label(mask, i, nl);
    const unsigned long long* pb = best + v;
    const unsigned root = 0xFFFFFFFFu - (unsigned)(*pb & 0xFFFFFFFFull);
    PCUDA_KEEP(pb);
    if ((unsigned)r == root) o = v;
  }
  out[i] = (uint8_t)o;
}

// ------------------------------------------------------------------------------------------------ host side
int em_check_shape(const char* who, int ndim, int z, int h, int w) {
  if (ndim != 2 && ndim != 3) PCUDA_FAIL(PCUDA_E_BADARG, "%s: ndim must be 2 or 3 (got %d)", who, ndim);
  if ((ndim == 2 && z != 1) || z < 1 || h < 1 || w < 1 || z > EM_MAXDIM || h > EM_MAXDIM || w > EM_MAXDIM)
    PCUDA_FAIL(PCUDA_E_BADARG, "%s: dims %d x %d x %d outside 1..%d (ndim 2: z = 1)", who, z, h, w, EM_MAXDIM);
  if ((long long)z * h * w >= (1ll << 31)) PCUDA_FAIL(PCUDA_E_BADARG, "%s: %d x %d x %d voxels >= 2^31", who, z, h, w);
  return PCUDA_OK;
}

bool em_anisotropic(int ndim, const double* spacing) {
  if (!spacing) return false;
  for (int a = 0; a < ndim; ++a)
    if (spacing[a] != 1.0) return true;
  return false;
}

EmLines em_lines(int axis, int z, int h, int w) {       // axis 0 = W, 1 = H, 2 = Z
  const long long hw = (long long)h * w, numel = hw * z;
  EmLines l;
  if (axis == 0) { l.n = w; l.stride = 1; l.inner = 1; l.outer_stride = w; }
  else if (axis == 1) { l.n = h; l.stride = w; l.inner = w; l.outer_stride = hw; }
  else { l.n = z; l.stride = hw; l.inner = hw; l.outer_stride = numel; }
  l.nlines = numel / l.n;
  return l;
}

struct EmLayout {
  size_t bmask, cntp, fa, fb, vb, maxkey, psum, pcnt, total;
  int nbb, nb2;
};
EmLayout em_layout(int ndim, int z, int h, int w, int ncls, bool aniso) {
  const long long numel = (long long)z * h * w;
  const int nf = 2 * ncls;
  const size_t tsz = aniso ? sizeof(double) : sizeof(int);
  EmLayout L;
  L.nbb = (int)(cdiv(numel, 256) < EM_BORDER_BLOCKS ? cdiv(numel, 256) : EM_BORDER_BLOCKS);
  L.nb2 = cdiv(em_lines(ndim == 3 ? 2 : 1, z, h, w).nlines, EM_LINE_THREADS);
  size_t o = 0;
  L.bmask = o; o += em_align((size_t)numel * sizeof(uint16_t));
  L.cntp = o; o += em_align((size_t)L.nbb * 3 * ncls * sizeof(unsigned));
  L.fa = o; o += em_align((size_t)nf * numel * tsz);
  L.fb = o; o += ndim == 3 ? em_align((size_t)nf * numel * tsz) : 0;
  L.vb = o; o += em_align((size_t)nf * numel * sizeof(int));
  L.maxkey = o; o += em_align((size_t)nf * sizeof(unsigned long long));
  L.psum = o; o += em_align((size_t)nf * L.nb2 * sizeof(double));
  L.pcnt = o; o += em_align((size_t)nf * L.nb2 * sizeof(unsigned));
  L.total = o;
  return L;
}

// the extended call's workspace: the plain layout, then the select's keys (in 3-D the first axis pass's field buffer is
// free again by the last pass and serves), its per-pass histograms [passes][ncls][2][bins] and its queries [ncls][2]
struct EmExtLayout {
  EmLayout base;
  size_t keys, hist, sel, zero_bytes, total;
  int passes;
};
EmExtLayout em_ext_layout(int ndim, int z, int h, int w, int ncls, bool aniso) {
  const long long numel = (long long)z * h * w;
  const size_t tsz = aniso ? sizeof(double) : sizeof(int);
  EmExtLayout X;
  X.base = em_layout(ndim, z, h, w, ncls, aniso);
  X.passes = (int)tsz * 8 / EM_SEL_BITS;
  size_t o = X.base.total;
  if (ndim == 3) X.keys = X.base.fa;
  else { X.keys = o; o += em_align((size_t)2 * ncls * numel * tsz); }
  X.hist = o; o += em_align((size_t)X.passes * ncls * 2 * EM_SEL_BINS * sizeof(unsigned));
  X.sel = o; o += em_align((size_t)ncls * 2 * sizeof(EmSel));
  X.zero_bytes = o - X.hist;                 // histograms and queries: one memset
  X.total = o;
  return X;
}

// ext: null for the plain rows out[ncls][8]; else the extended rows out[ncls][12] at percentile 100 * quant
template <typename T>
int em_surface_run(const void* pred, const void* gt, int labels_i32, int ndim, int z, int h, int w, const EmClasses& cls,
                   int conn, const double* spacing, double* out, char* ws, const EmLayout& L, hipStream_t s,
                   const EmExtLayout* ext = nullptr, double quant = 0.0) {
  const long long numel = (long long)z * h * w;
  const int nf = 2 * cls.n;
  uint16_t* bmask = (uint16_t*)(ws + L.bmask);
  unsigned* cntp = (unsigned*)(ws + L.cntp);
  T* fa = (T*)(ws + L.fa);
  T* fb = (T*)(ws + L.fb);
  int* vb = (int*)(ws + L.vb);
  unsigned long long* maxkey = (unsigned long long*)(ws + L.maxkey);
  double* psum = (double*)(ws + L.psum);
  unsigned* pcnt = (unsigned*)(ws + L.pcnt);
  if (hipMemsetAsync(maxkey, 0, nf * sizeof(unsigned long long), s) != hipSuccess)
    PCUDA_FAIL(PCUDA_E_LAUNCH, "surface_metrics: memset failed");
  if (ext && hipMemsetAsync(ws + ext->hist, 0, ext->zero_bytes, s) != hipSuccess)
    PCUDA_FAIL(PCUDA_E_LAUNCH, "surface_metrics_ext: memset failed");
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)numel * (2.0 * (labels_i32 ? 4 : 1) + 2.0 * nf * ndim * (2 * sizeof(T) + 4)), s);
  if (labels_i32)
    hipLaunchKernelGGL(em_border_kernel<int>, dim3(L.nbb), dim3(256), 0, s, (const int*)pred, (const int*)gt, z, h, w, ndim,
                       conn, cls, bmask, cntp);
  else
    hipLaunchKernelGGL(em_border_kernel<uint8_t>, dim3(L.nbb), dim3(256), 0, s, (const uint8_t*)pred, (const uint8_t*)gt,
                       z, h, w, ndim, conn, cls, bmask, cntp);
  PCUDA_CHECK_LAUNCH("em_border_kernel");
  // spacing[] is in array-axis order: (z,) y, x
  const double spw = spacing ? spacing[ndim - 1] : 1.0, sph = spacing ? spacing[ndim - 2] : 1.0,
               spz = (spacing && ndim == 3) ? spacing[0] : 1.0;
  const EmLines lw = em_lines(0, z, h, w), lh = em_lines(1, z, h, w), lz = em_lines(2, z, h, w);
  hipLaunchKernelGGL((em_edt_pass_kernel<T, 0>), dim3(cdiv(lw.nlines, EM_LINE_THREADS), nf), dim3(EM_LINE_THREADS), 0, s,
                     bmask, (const T*)nullptr, fa, vb, numel, lw, spw, maxkey, psum, pcnt);
  PCUDA_CHECK_LAUNCH("em_edt_pass_kernel<W>");
  if (ext) {
    T* keys = (T*)(ws + ext->keys);
    if (ndim == 3) {
      hipLaunchKernelGGL((em_edt_pass_kernel<T, 1>), dim3(cdiv(lh.nlines, EM_LINE_THREADS), nf), dim3(EM_LINE_THREADS), 0,
                         s, bmask, (const T*)fa, fb, vb, numel, lh, sph, maxkey, psum, pcnt);
      PCUDA_CHECK_LAUNCH("em_edt_pass_kernel<H>");
      hipLaunchKernelGGL((em_edt_pass_kernel<T, 3>), dim3(L.nb2, nf), dim3(EM_LINE_THREADS), 0, s, bmask, (const T*)fb, keys,
                         vb, numel, lz, spz, maxkey, psum, pcnt);
      PCUDA_CHECK_LAUNCH("em_edt_pass_kernel<Z, keys>");
    } else {
      hipLaunchKernelGGL((em_edt_pass_kernel<T, 3>), dim3(L.nb2, nf), dim3(EM_LINE_THREADS), 0, s, bmask, (const T*)fa, keys,
                         vb, numel, lh, sph, maxkey, psum, pcnt);
      PCUDA_CHECK_LAUNCH("em_edt_pass_kernel<H, keys>");
    }
    unsigned* hist = (unsigned*)(ws + ext->hist);
    EmSel* sel = (EmSel*)(ws + ext->sel);
    const int nbx = (int)(cdiv(numel, 256) < EM_SEL_BLOCKS ? cdiv(numel, 256) : EM_SEL_BLOCKS);
    for (int p = 0; p < ext->passes; ++p) {
      const int shift = (ext->passes - 1 - p) * EM_SEL_BITS;
      unsigned* hp = hist + (size_t)p * cls.n * 2 * EM_SEL_BINS;
      hipLaunchKernelGGL(em_sel_hist_kernel<T>, dim3(nbx, cls.n), dim3(256), 0, s, (const uint16_t*)bmask, (const T*)keys,
                         numel, shift, (const EmSel*)sel, hp);
      PCUDA_CHECK_LAUNCH("em_sel_hist_kernel");
      hipLaunchKernelGGL(em_sel_narrow_kernel, dim3(2 * cls.n), dim3(64), 0, s, (const unsigned*)hp, shift, p == 0 ? 1 : 0,
                         (const unsigned*)pcnt, L.nb2, quant, sel);
      PCUDA_CHECK_LAUNCH("em_sel_narrow_kernel");
    }
    hipLaunchKernelGGL(em_final_ext_kernel<T>, dim3(1), dim3(64), 0, s, (const unsigned*)cntp, L.nbb,
                       (const unsigned long long*)maxkey, (const double*)psum, (const unsigned*)pcnt, L.nb2, cls.n,
                       (const EmSel*)sel, quant, out);
    PCUDA_CHECK_LAUNCH("em_final_ext_kernel");
    return PCUDA_OK;
  }
  if (ndim == 3) {
    hipLaunchKernelGGL((em_edt_pass_kernel<T, 1>), dim3(cdiv(lh.nlines, EM_LINE_THREADS), nf), dim3(EM_LINE_THREADS), 0, s,
                       bmask, (const T*)fa, fb, vb, numel, lh, sph, maxkey, psum, pcnt);
    PCUDA_CHECK_LAUNCH("em_edt_pass_kernel<H>");
    hipLaunchKernelGGL((em_edt_pass_kernel<T, 2>), dim3(L.nb2, nf), dim3(EM_LINE_THREADS), 0, s, bmask, (const T*)fb,
                       (T*)nullptr, vb, numel, lz, spz, maxkey, psum, pcnt);
    PCUDA_CHECK_LAUNCH("em_edt_pass_kernel<Z>");
  } else {
    hipLaunchKernelGGL((em_edt_pass_kernel<T, 2>), dim3(L.nb2, nf), dim3(EM_LINE_THREADS), 0, s, bmask, (const T*)fa,
                       (T*)nullptr, vb, numel, lh, sph, maxkey, psum, pcnt);
    PCUDA_CHECK_LAUNCH("em_edt_pass_kernel<H>");
  }
  hipLaunchKernelGGL(em_final_kernel<T>, dim3(1), dim3(64), 0, s, (const unsigned*)cntp, L.nbb,
                     (const unsigned long long*)maxkey, (const double*)psum, (const unsigned*)pcnt, L.nb2, cls.n, out);
  PCUDA_CHECK_LAUNCH("em_final_kernel");
  return PCUDA_OK;
}

template <typename T>
int em_ccl_run(const T* mask, int z, int h, int w, int nl, uint8_t* out, char* ws, hipStream_t s) {
  const long long numel = (long long)z * h * w;
  int* par = (int*)ws;
  unsigned* size = (unsigned*)(ws + em_align((size_t)numel * sizeof(int)));
  unsigned long long* best = (unsigned long long*)(ws + 2 * em_align((size_t)numel * sizeof(int)));
  if (hipMemsetAsync(size, 0, (size_t)numel * sizeof(unsigned), s) != hipSuccess ||
      hipMemsetAsync(best, 0, 256 * sizeof(unsigned long long), s) != hipSuccess)
    PCUDA_FAIL(PCUDA_E_LAUNCH, "largest_components: memset failed");
  ProfScope prof(PCUDA_FAM_POINTWISE, (double)numel * (4.0 * sizeof(T) + 24.0), s);
  const int nb = cdiv(numel, 256);
  hipLaunchKernelGGL(em_ccl_init_kernel<T>, dim3(nb), dim3(256), 0, s, mask, numel, nl, par);
  PCUDA_CHECK_LAUNCH("em_ccl_init_kernel");
  hipLaunchKernelGGL(em_ccl_merge_kernel<T>, dim3(nb), dim3(256), 0, s, mask, z, h, w, nl, par);
  PCUDA_CHECK_LAUNCH("em_ccl_merge_kernel");
  hipLaunchKernelGGL(em_ccl_compress_kernel, dim3(nb), dim3(256), 0, s, numel, par);
  PCUDA_CHECK_LAUNCH("em_ccl_compress_kernel");
  hipLaunchKernelGGL(em_ccl_size_kernel, dim3(cdiv(cdiv(numel, EM_CCL_RUN), 256)), dim3(256), 0, s, (const int*)par, numel,
                     size);
  PCUDA_CHECK_LAUNCH("em_ccl_size_kernel");
  hipLaunchKernelGGL(em_ccl_best_kernel<T>, dim3(nb), dim3(256), 0, s, mask, (const int*)par, (const unsigned*)size, numel,
                     nl, best);
  PCUDA_CHECK_LAUNCH("em_ccl_best_kernel");
  hipLaunchKernelGGL(em_ccl_write_kernel<T>, dim3(nb), dim3(256), 0, s, mask, (const int*)par,
                     (const unsigned long long*)best, numel, nl, out);
  PCUDA_CHECK_LAUNCH("em_ccl_write_kernel");
  return PCUDA_OK;
}

}  // namespace

extern "C" size_t pcuda_surface_metrics_workspace_size(int ndim, int z, int h, int w, int ncls, const double* spacing) {
  if (em_check_shape("surface_metrics_workspace_size", ndim, z, h, w) != PCUDA_OK || ncls < 1 || ncls > EM_MAXCLS) return 0;
  return em_layout(ndim, z, h, w, ncls, em_anisotropic(ndim, spacing)).total;
}

extern "C" size_t pcuda_surface_metrics_ext_workspace_size(int ndim, int z, int h, int w, int ncls, const double* spacing) {
  if (em_check_shape("surface_metrics_ext_workspace_size", ndim, z, h, w) != PCUDA_OK || ncls < 1 || ncls > EM_MAXCLS)
    return 0;
  return em_ext_layout(ndim, z, h, w, ncls, em_anisotropic(ndim, spacing)).total;
}

extern "C" int pcuda_surface_metrics_ext(const void* pred, const void* gt, int labels_i32, int ndim, int z, int h, int w,
                                         const int* classes, int ncls, int connectivity, const double* spacing,
                                         double percentile, double* out, void* workspace, size_t workspace_bytes,
                                         pcuda_stream_t s) {
  const int rc = em_check_shape("surface_metrics_ext", ndim, z, h, w);
  if (rc != PCUDA_OK) return rc;
  if (!pred || !gt || !out || !classes) PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics_ext: null pointer");
  if (ncls < 1 || ncls > EM_MAXCLS) PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics_ext: %d classes (1..%d)", ncls, EM_MAXCLS);
  if (connectivity < 1 || connectivity > ndim)
    PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics_ext: connectivity %d outside 1..%d", connectivity, ndim);
  if (spacing)
    for (int a = 0; a < ndim; ++a)
      if (!(spacing[a] > 0.0) || !isfinite(spacing[a]))
        PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics_ext: spacing[%d] = %g is not a positive finite number", a, spacing[a]);
  if (!(percentile >= 0.0 && percentile <= 100.0))
    PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics_ext: percentile %g outside 0..100", percentile);
  const bool aniso = em_anisotropic(ndim, spacing);
  const EmExtLayout X = em_ext_layout(ndim, z, h, w, ncls, aniso);
  if (!workspace || workspace_bytes < X.total)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "surface_metrics_ext: workspace %zu bytes, needs %zu", workspace_bytes, X.total);
  EmClasses cls = {};
  for (int k = 0; k < ncls; ++k) cls.c[k] = classes[k];
  cls.n = ncls;
  const double quant = percentile / 100.0;
  if (aniso)
    return em_surface_run<double>(pred, gt, labels_i32, ndim, z, h, w, cls, connectivity, spacing, out, (char*)workspace,
                                  X.base, (hipStream_t)s, &X, quant);
  return em_surface_run<int>(pred, gt, labels_i32, ndim, z, h, w, cls, connectivity, nullptr, out, (char*)workspace, X.base,
                             (hipStream_t)s, &X, quant);
}

extern "C" int pcuda_surface_metrics(const void* pred, const void* gt, int labels_i32, int ndim, int z, int h, int w,
                                     const int* classes, int ncls, int connectivity, const double* spacing, double* out,
                                     void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  const int rc = em_check_shape("surface_metrics", ndim, z, h, w);
  if (rc != PCUDA_OK) return rc;
  if (!pred || !gt || !out || !classes) PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics: null pointer");
  if (ncls < 1 || ncls > EM_MAXCLS) PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics: %d classes (1..%d)", ncls, EM_MAXCLS);
  if (connectivity < 1 || connectivity > ndim)
    PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics: connectivity %d outside 1..%d", connectivity, ndim);
  if (spacing)
    for (int a = 0; a < ndim; ++a)
      if (!(spacing[a] > 0.0) || !isfinite(spacing[a]))
        PCUDA_FAIL(PCUDA_E_BADARG, "surface_metrics: spacing[%d] = %g is not a positive finite number", a, spacing[a]);
  const bool aniso = em_anisotropic(ndim, spacing);
  const EmLayout L = em_layout(ndim, z, h, w, ncls, aniso);
  if (!workspace || workspace_bytes < L.total)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "surface_metrics: workspace %zu bytes, needs %zu", workspace_bytes, L.total);
  EmClasses cls = {};
  for (int k = 0; k < ncls; ++k) cls.c[k] = classes[k];
  cls.n = ncls;
  if (aniso)
    return em_surface_run<double>(pred, gt, labels_i32, ndim, z, h, w, cls, connectivity, spacing, out, (char*)workspace, L,
                                  (hipStream_t)s);
  return em_surface_run<int>(pred, gt, labels_i32, ndim, z, h, w, cls, connectivity, nullptr, out, (char*)workspace, L,
                             (hipStream_t)s);
}

extern "C" size_t pcuda_largest_components_workspace_size(int ndim, int z, int h, int w) {
  if (em_check_shape("largest_components_workspace_size", ndim, z, h, w) != PCUDA_OK) return 0;
  return 2 * em_align((size_t)z * h * w * sizeof(int)) + 256 * sizeof(unsigned long long);
}

extern "C" int pcuda_largest_components(const void* mask, int mask_i32, int ndim, int z, int h, int w, int nlabels,
                                        uint8_t* out, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  const int rc = em_check_shape("largest_components", ndim, z, h, w);
  if (rc != PCUDA_OK) return rc;
  if (!mask || !out) PCUDA_FAIL(PCUDA_E_BADARG, "largest_components: null pointer");
  if (nlabels < 0) PCUDA_FAIL(PCUDA_E_BADARG, "largest_components: nlabels %d < 0", nlabels);
  const size_t need = pcuda_largest_components_workspace_size(ndim, z, h, w);
  if (!workspace || workspace_bytes < need)
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "largest_components: workspace %zu bytes, needs %zu", workspace_bytes, need);
  const int nl = nlabels < 255 ? nlabels : 255;       // labels 1..min(nlabels, 255); the caller rejects larger ones
  if (mask_i32) return em_ccl_run<int>((const int*)mask, z, h, w, nl, out, (char*)workspace, (hipStream_t)s);
  return em_ccl_run<uint8_t>((const uint8_t*)mask, z, h, w, nl, out, (char*)workspace, (hipStream_t)s);
}
