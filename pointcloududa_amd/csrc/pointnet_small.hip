// Small kernels of the point-cloud discriminator (PointNetCls): BatchNorm1d on [B][C] in one launch per direction, and the
// BatchNorm backward behind the max over points reading (g, idx) in place instead of the dense [B][C][L] gradient.
//
// Every kernel here computes, BIT FOR BIT, what the general kernels of pointwise.hip / dense.hip compute for the same
// tensors: the association of every floating-point sum is kept, only the mapping to threads and the memory access change.
// The BatchNorm arithmetic itself -- both finalisations, the gate, the reduce terms, the dz expression -- is bn_device.h's,
// the one statement both files compile.
// (A file of its own: tests/test_isa_rules.py keeps an allow-list of loads in pointwise.s / dense.s that this code must not
// add to.  The VMEM address rule of common.h is followed here all the same: PCUDA_KEEP after the data is consumed.)
#include "common.h"
#include "bn_device.h"      // the BatchNorm arithmetic, shared with pointwise.hip

#ifndef PCH
#define PCH 2048   // plane elements per workgroup of the general kernels (pointwise.hip)
#endif

namespace {

constexpr int B1_CH = 16;      // channels per workgroup (lanes along C, the contiguous axis)
constexpr int B1_RG = 16;      // row groups per workgroup
constexpr int B1_SLOTS = 16;   // 256 / B1_RG: the slots of bn_finalize_kernel's 256-slot tree one thread owns
constexpr int B1_MAXB = 1024;  // up to 4 samples per slot
constexpr int B1_MAXSN = 1 << 20;   // largest row stride (32-bit element offsets)

// Sum of per-sample fp32 pairs in fp64 in the order the general path takes for hw == 1, where every sample is a tile of
// its own: tile_pair_sum gives sample i to slot i % 256 (i ascending within the slot), then the 256-slot tree pairs slot t
// with slot t + o for o = 128 ... 1.  Thread (cx, ry) owns slots ry + 16 j, j = 0..15: the levels o = 128 ... 16 pair
// slots of ONE thread (t and t + o agree modulo 16) and run in registers; o = 8 ... 1 pair threads ry and ry + o through
// LDS.  Slots without a sample hold +0.0 as they do there.  The total lands in sh[.][0][cx].
template <bool TWO, class F>
__device__ __forceinline__ void slot_tree_sum(const float* __restrict__ pa, int a_sn, const float* __restrict__ pd,
                                              int d_sn, int b, bool live, F&& part, double (&sh)[2][B1_RG][B1_CH]) {
  const int cx = threadIdx.x & (B1_CH - 1), ry = threadIdx.x >> 4;
  double s1[B1_SLOTS], s2[B1_SLOTS];
#pragma unroll
  for (int j = 0; j < B1_SLOTS; ++j) { s1[j] = 0; s2[j] = 0; }
#pragma unroll
  for (int q = 0; q < B1_MAXB / 256; ++q) {
    if (q * 256 >= b) break;
    // all of a trip's loads first (one round trip, not sixteen), then the sums in slot order
    float av[B1_SLOTS], gv[B1_SLOTS];
    const float* qa[B1_SLOTS];
    const float* qd[B1_SLOTS];
#pragma unroll
    for (int j = 0; j < B1_SLOTS; ++j) {
      const int i = q * 256 + B1_RG * j + ry;
      const bool on = live && i < b;
      qa[j] = pa + i * a_sn;      // (rows below B1_MAXB, strides below 2^20: 32-bit offsets)
      qd[j] = TWO ? pd + i * d_sn : nullptr;
      av[j] = on ? *qa[j] : 0.f;
      gv[j] = (TWO && on) ? *qd[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < B1_SLOTS; ++j) {
      const int i = q * 256 + B1_RG * j + ry;
      float p1, p2;
      part(av[j], gv[j], p1, p2);
      if (i < b) { s1[j] += (double)p1; s2[j] += (double)p2; }
    }
#pragma unroll
    for (int j = 0; j < B1_SLOTS; ++j) {      // (VMEM address rule, common.h)
      PCUDA_KEEP(qa[j]);
      if (TWO) PCUDA_KEEP(qd[j]);
    }
  }
#pragma unroll
  for (int o = B1_SLOTS / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < o; ++j) { s1[j] += s1[j + o]; s2[j] += s2[j + o]; }
  }
  sh[0][ry][cx] = s1[0];
  sh[1][ry][cx] = s2[0];
  __syncthreads();
  for (int o = B1_RG / 2; o > 0; o >>= 1) {
    if (ry < o) {
      sh[0][ry][cx] += sh[0][ry + o][cx];
      sh[1][ry][cx] += sh[1][ry + o][cx];
    }
    __syncthreads();
  }
}

// bn_stats_kernel + bn_finalize_kernel + bn_apply_kernel<1, false> on a[b][c] (row stride a_sn, channels contiguous)
__global__ __launch_bounds__(256) void bn1d_fwd_kernel(const float* __restrict__ a, int a_sn, int b, int c, double count,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float eps, float momentum, float* running_mean, float* running_var,
                                                       float* __restrict__ mean, float* __restrict__ invstd,
                                                       float* __restrict__ scale, float* __restrict__ shift, int relu,
                                                       float* __restrict__ y, int y_sn) {
  __shared__ double sh[2][B1_RG][B1_CH];
  __shared__ float shc[2][B1_CH];
  const int cx = threadIdx.x & (B1_CH - 1), ry = threadIdx.x >> 4;
  const int ch = blockIdx.x * B1_CH + cx;
  const bool live = ch < c;
  const float* pa = a + ch;
  // one sample's partial as bn_stats_kernel leaves it for a one-element tile: block_sum adds the value to zeros
  slot_tree_sum<false>(pa, a_sn, nullptr, 0, b, live, [&](float v, float, float& p1, float& p2) {
    p1 = 0.f + v;
    p2 = 0.f + v * v;
  }, sh);
  if (ry == 0 && live) {      // bn_finalize_kernel's thread 0: the same bn_fwd_finalize (bn_device.h)
    const float* pgm = gamma ? gamma + ch : nullptr;
    const float* pbt = beta ? beta + ch : nullptr;
    const BnFwd r = bn_fwd_finalize(sh[0][0][cx], sh[1][0][cx], count, pgm ? *pgm : 1.f, pbt ? *pbt : 0.f, eps);
    mean[ch] = r.mean;
    invstd[ch] = r.invstd;
    scale[ch] = r.scale;
    shift[ch] = r.shift;
    shc[0][cx] = r.scale;
    shc[1][cx] = r.shift;
    if (running_mean) {
      float* prm = running_mean + ch;
      float* prv = running_var + ch;
      const float rm = *prm, rv = *prv;
      *prm = bn_running(rm, momentum, r.mean);
      *prv = bn_running(rv, momentum, bn_unbiased(r.var, count));
      PCUDA_KEEP(prm); PCUDA_KEEP(prv);
    }
    PCUDA_KEEP(pgm); PCUDA_KEEP(pbt);      // (VMEM address rule, common.h)
  }
  __syncthreads();
  if (!live) return;
  const float sc = shc[0][cx], sf = shc[1][cx];
  float* py = y + ch;
  for (int i = ry; i < b; i += B1_RG) {
    const float* q = pa + i * a_sn;
    float v = *q;
    v = v * sc + sf;      // multiply, then add: -ffp-contract=off, as bn_apply_kernel<.., false>
    if (relu) v = v > 0.f ? v : 0.f;
    py[i * y_sn] = v;
    PCUDA_KEEP(q);
  }
}

// bn_bwd_reduce_kernel<1> + bn_bwd_finalize_kernel + bn_bwd_apply_kernel<1> on [b][c], one gradient source, training
// statistics (count > 0)
__global__ __launch_bounds__(256) void bn1d_bwd_kernel(const float* __restrict__ dy, int dy_sn,
                                                       const float* __restrict__ a, int a_sn, int b, int c,
                                                       double count, const float* __restrict__ gamma,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       int post_relu, float act_slope, float* dgamma, float* dbeta,
                                                       int accumulate, float* __restrict__ dz, int dz_sn) {
  __shared__ double sh[2][B1_RG][B1_CH];
  __shared__ float shc[3][B1_CH];
  const int cx = threadIdx.x & (B1_CH - 1), ry = threadIdx.x >> 4;
  const int ch = blockIdx.x * B1_CH + cx;
  const bool live = ch < c;
  const float* pa = a + ch;
  const float* pd = dy + ch;
  float m = 0.f, is = 0.f, sc = 0.f, sf = 0.f;
  if (live) {
    const float* pm = mean + ch;
    const float* pis = invstd + ch;
    m = *pm; is = *pis;
    if (post_relu) {
      const float* psc = scale + ch;
      const float* psf = shift + ch;
      sc = *psc; sf = *psf;
      PCUDA_KEEP(psc); PCUDA_KEEP(psf);
    }
    PCUDA_KEEP(pm); PCUDA_KEEP(pis);      // (VMEM address rule, common.h)
  }
  // one sample's partial as bn_bwd_reduce_kernel leaves it for a one-element tile
  slot_tree_sum<true>(pa, a_sn, pd, dy_sn, b, live, [&](float av, float gg, float& p1, float& p2) {
    p1 = 0.f; p2 = 0.f;
    bn_reduce_terms(bn_gate(gg, av, sc, sf, post_relu), av, m, is, p1, p2);
  }, sh);
  if (ry == 0 && live) {      // bn_bwd_finalize_kernel's thread 0: the same bn_bwd_finalize (count > 0: never the frozen form)
    double g = 1.0;
    if (gamma) {
      const float* pgm = gamma + ch;
      g = (double)*pgm;
      PCUDA_KEEP(pgm);
    }
    const BnBwd r = bn_bwd_finalize(sh[0][0][cx], sh[1][0][cx], count, g, is, m);
    if (dgamma) {
      float* p = dgamma + ch;
      const float old = accumulate ? *p : 0.f;
      *p = accumulate ? old + r.dgamma : r.dgamma;
      PCUDA_KEEP(p);
    }
    if (dbeta) {
      float* p = dbeta + ch;
      const float old = accumulate ? *p : 0.f;
      *p = accumulate ? old + r.dbeta : r.dbeta;
      PCUDA_KEEP(p);
    }
    for (int k = 0; k < 3; ++k) shc[k][cx] = r.coef[k];
  }
  __syncthreads();
  if (!live) return;
  const float c0 = shc[0][cx], c1 = shc[1][cx], c2 = shc[2][cx];
  float* pz = dz + ch;
  for (int i = ry; i < b; i += B1_RG) {
    const float* qa = pa + i * a_sn;
    const float* qd = pd + i * dy_sn;
    const float av = *qa, gg = *qd;
    pz[i * dz_sn] = bn_dz(bn_gate(gg, av, sc, sf, post_relu), av, c0, c1, c2, post_relu, act_slope);
    PCUDA_KEEP(qa); PCUDA_KEEP(qd);
  }
}

// ---------------------------------------------------------------------------- gradient of the max over points, in place
// The dense gradient max_points_bwd_kernel writes holds, in row (n, ch) of l <= PCH elements, g[n][ch] at idx[n][ch] and
// 0.f elsewhere: bn_bwd_reduce_kernel's tile of that row sums one value with zeros, (0.f + gg, 0.f + gg * xhat).
__global__ __launch_bounds__(256) void bn_bwd_reduce_maxpts_kernel(const float* __restrict__ g, const int* __restrict__ idx,
                                                                   const float* __restrict__ a, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd,
                                                                   const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, int post_relu, int rows,
                                                                   int c, int l, float* __restrict__ red) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int ch = row % c;
  const int* pi = idx + row;
  const float* pg = g + row;
  const int k = *pi;
  float s1 = 0.f, s2 = 0.f;
  if (k >= 0 && k < l) {      // (a row without a maximum, all NaN, keeps idx = INT_MAX: the dense gradient is all zero)
    const float* qa = a + (long long)row * l + k;
    const float* pm = mean + ch;
    const float* ps = invstd + ch;
    const float av = *qa, m = *pm, is = *ps;
    float gg = *pg;
    if (post_relu) {
      const float* psc = scale + ch;
      const float* psf = shift + ch;
      gg = bn_gate(gg, av, *psc, *psf, 1);
      PCUDA_KEEP(psc); PCUDA_KEEP(psf);
    }
    bn_reduce_terms(gg, av, m, is, s1, s2);      // (onto 0.f: one value and the tile's zeros)
    PCUDA_KEEP(qa); PCUDA_KEEP(pm); PCUDA_KEEP(ps);
  }
  *(float2*)(red + 2ll * row) = make_float2(s1, s2);      // tile n, channel ch: red[(n * c + ch) * 2]
  PCUDA_KEEP(pi); PCUDA_KEEP(pg);
}

// bn_bwd_apply_kernel's expression with gg = (i == idx) ? g : 0.f; the rows of a / dz are dense, so the tensor is one flat
// run of rows * l elements: MP_CH elements per workgroup, VEC at a time (VEC = 4: l % 4 == 0, a vector stays in its row)
constexpr int MP_CH = 4096;
template <int VEC>
__global__ __launch_bounds__(256) void bn_bwd_apply_maxpts_kernel(const float* __restrict__ g, const int* __restrict__ idx,
                                                                  const float* __restrict__ a, const float* __restrict__ coef,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, int post_relu,
                                                                  float act_slope, long long total, int c, int l,
                                                                  float* __restrict__ dz) {
  const long long e0 = (long long)blockIdx.x * MP_CH;
  const long long row0 = e0 / l;
  const unsigned rem0 = (unsigned)(e0 - row0 * l);
  const int n_here = (int)(total - e0 < MP_CH ? total - e0 : MP_CH);
  for (int o = threadIdx.x * VEC; o < n_here; o += 256 * VEC) {
    const unsigned t = rem0 + (unsigned)o, dr = t / (unsigned)l;
    const int i0 = (int)(t - dr * (unsigned)l);
    const int row = (int)(row0 + dr), ch = row % c;
    const float* qa = a + e0 + o;
    const int* pi = idx + row;
    const float* pg = g + row;
    const float* pc = coef + ch * 3;
    float av[VEC], out[VEC];
    if (VEC == 4) {
      const float4 t4 = *(const float4*)qa;
      av[0] = t4.x; av[1 % VEC] = t4.y; av[2 % VEC] = t4.z; av[3 % VEC] = t4.w;
    } else {
      av[0] = *qa;
    }
    const int k = *pi;
    const float gv = *pg;
    const float c0 = pc[0], c1 = pc[1], c2 = pc[2];
    float sc = 0.f, sf = 0.f;
    if (post_relu) {
      const float* psc = scale + ch;
      const float* psf = shift + ch;
      sc = *psc; sf = *psf;
      PCUDA_KEEP(psc); PCUDA_KEEP(psf);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      out[e] = bn_dz(bn_gate((i0 + e == k) ? gv : 0.f, av[e], sc, sf, post_relu), av[e], c0, c1, c2, post_relu, act_slope);
    if (VEC == 4) *(float4*)(dz + e0 + o) = make_float4(out[0], out[1 % VEC], out[2 % VEC], out[3 % VEC]);
    else dz[e0 + o] = out[0];
    PCUDA_KEEP(qa); PCUDA_KEEP(pi); PCUDA_KEEP(pg); PCUDA_KEEP(pc);
  }
}

}  // namespace

// ---------------------------------------------------------------------------- host
// Training-mode BatchNorm1d on a[b][c] (rows a_sn apart, channels contiguous), b <= 1024: pcuda_bn_stats +
// pcuda_bn_finalize + pcuda_bn_apply (without PCUDA_BN_APPLY_FMA) in one launch, same bits.
extern "C" int pcuda_bn1d_fwd(const float* a, long long a_sn, int b, int c, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                              float* scale, float* shift, int relu, float* y, long long y_sn, pcuda_stream_t s) {
  if (!a || !y || !mean || !invstd || !scale || !shift || b <= 0 || c <= 0 || (running_mean == nullptr) != (running_var == nullptr))
    PCUDA_FAIL(PCUDA_E_BADARG, "bn1d_fwd: bad arguments");
  if (b > B1_MAXB || a_sn < c || y_sn < c || a_sn > B1_MAXSN || y_sn > B1_MAXSN)
    PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "bn1d_fwd: b > 1024 or row stride < c or > 2^20 (use pcuda_bn_stats / _finalize / _apply)");
  hipLaunchKernelGGL(bn1d_fwd_kernel, dim3(cdiv(c, B1_CH)), dim3(256), 0, (hipStream_t)s, a, (int)a_sn, b, c, (double)b, gamma, beta,
                     eps, momentum, running_mean, running_var, mean, invstd, scale, shift, relu, y, (int)y_sn);
  PCUDA_CHECK_LAUNCH("bn1d_fwd_kernel");
  return PCUDA_OK;
}

// pcuda_bn_bwd_reduce + pcuda_bn_bwd_finalize (count = b) + pcuda_bn_bwd_apply in one launch for [b][c] tensors.  Not
// taken here (callers use the three-launch path): a second gradient share (dy2), frozen statistics (count < 0), b > 1024,
// rows whose channels are not contiguous.
extern "C" int pcuda_bn1d_bwd(const float* dy, long long dy_sn, const float* a, long long a_sn, int b, int c,
                              const float* gamma, const float* mean, const float* invstd, const float* scale,
                              const float* shift, int post_relu, float act_slope, float* dgamma, float* dbeta,
                              int accumulate, float* dz, long long dz_sn, pcuda_stream_t s) {
  if (!dy || !a || !dz || !mean || !invstd || b <= 0 || c <= 0 || (post_relu && (!scale || !shift)))
    PCUDA_FAIL(PCUDA_E_BADARG, "bn1d_bwd: bad arguments");
  if (b > B1_MAXB || a_sn < c || dy_sn < c || dz_sn < c || a_sn > B1_MAXSN || dy_sn > B1_MAXSN || dz_sn > B1_MAXSN)
    PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "bn1d_bwd: b > 1024 or row stride < c or > 2^20 (use pcuda_bn_bwd_reduce / _finalize / _apply)");
  hipLaunchKernelGGL(bn1d_bwd_kernel, dim3(cdiv(c, B1_CH)), dim3(256), 0, (hipStream_t)s, dy, (int)dy_sn, a, (int)a_sn, b, c, (double)b,
                     gamma, mean, invstd, scale, shift, post_relu, act_slope, dgamma, dbeta, accumulate, dz, (int)dz_sn);
  PCUDA_CHECK_LAUNCH("bn1d_bwd_kernel");
  return PCUDA_OK;
}

// The two passes of the BatchNorm backward whose incoming gradient is pcuda_max_points_bwd(g, idx): dense g[b][c],
// idx[b][c], a / dz[b][c][l], l <= 2048 (one tile of the general kernels per row).  red[b][c][2] is what
// pcuda_bn_bwd_reduce would write for the dense gradient (ntiles = b); pcuda_bn_bwd_finalize consumes it unchanged.
extern "C" int pcuda_bn_bwd_reduce_maxpts(const float* g, const int* idx, const float* a, const float* mean,
                                          const float* invstd, const float* scale, const float* shift, int post_relu, int b,
                                          int c, int l, float* red, pcuda_stream_t s) {
  if (!g || !idx || !a || !mean || !invstd || !red || b <= 0 || c <= 0 || l <= 0 || (post_relu && (!scale || !shift)) ||
      (long long)b * c > 0x7fffffffll)
    PCUDA_FAIL(PCUDA_E_BADARG, "bn_bwd_reduce_maxpts: bad arguments");
  if (l > PCH) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "bn_bwd_reduce_maxpts: l > 2048 (use pcuda_max_points_bwd + pcuda_bn_bwd_reduce)");
  const int rows = b * c;
  hipLaunchKernelGGL(bn_bwd_reduce_maxpts_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, (hipStream_t)s, g, idx, a, mean, invstd,
                     scale, shift, post_relu, rows, c, l, red);
  PCUDA_CHECK_LAUNCH("bn_bwd_reduce_maxpts_kernel");
  return PCUDA_OK;
}

extern "C" int pcuda_bn_bwd_apply_maxpts(const float* g, const int* idx, const float* a, const float* coef,
                                         const float* scale, const float* shift, int post_relu, float act_slope, float* dz,
                                         int b, int c, int l, pcuda_stream_t s) {
  if (!g || !idx || !a || !coef || !dz || b <= 0 || c <= 0 || l <= 0 || (post_relu && (!scale || !shift)) ||
      (long long)b * c > 0x7fffffffll)
    PCUDA_FAIL(PCUDA_E_BADARG, "bn_bwd_apply_maxpts: bad arguments");
  if (l > PCH) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "bn_bwd_apply_maxpts: l > 2048 (use pcuda_max_points_bwd + pcuda_bn_bwd_apply)");
  const long long total = (long long)b * c * l;
  const bool vec = (l & 3) == 0 && ((((uintptr_t)a) | ((uintptr_t)dz)) & 15) == 0;
  const dim3 grid((unsigned)cdiv(total, MP_CH));
  if (vec)
    hipLaunchKernelGGL(bn_bwd_apply_maxpts_kernel<4>, grid, dim3(256), 0, (hipStream_t)s, g, idx, a, coef, scale, shift, post_relu,
                       act_slope, total, c, l, dz);
  else
    hipLaunchKernelGGL(bn_bwd_apply_maxpts_kernel<1>, grid, dim3(256), 0, (hipStream_t)s, g, idx, a, coef, scale, shift, post_relu,
                       act_slope, total, c, l, dz);
  PCUDA_CHECK_LAUNCH("bn_bwd_apply_maxpts_kernel");
  return PCUDA_OK;
}
