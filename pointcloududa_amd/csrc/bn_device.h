// The arithmetic of training BatchNorm and of its backward pass behind a LeakyReLU / in front of a ReLU, stated ONCE:
// pointwise.hip (planes [n][c][hw]) and pointnet_small.hip ([b][c] in one launch, the gradient of the max over points read
// in place) both compute with these functions, which is what keeps the two files bit for bit alike.  Pure functions of
// values: every load and store stays with the caller (the files address memory differently, and pointnet_small.hip holds
// its addresses with PCUDA_KEEP).  The order of the operations is part of the result (-ffp-contract=off).
#pragma once

// ---------------------------------------------------------------------------- forward finalisation
struct BnFwd { float mean, invstd, scale, shift; double var; };

// sums (s1 = sum a, s2 = sum a * a, in fp64) over `count` values -> the statistics and the affine y = a * scale + shift
__device__ __forceinline__ BnFwd bn_fwd_finalize(double s1, double s2, double count, float gamma, float beta, float eps) {
  const double m = s1 / count;
  double var = s2 / count - m * m;
  // count == 1: the variance of one value is 0 by definition, not the rounding residue of the float32 a * a next to
  // eps; the normalised value is then 0 and the output the constant beta, which scale = 0 states exactly
  if (var < 0 || count <= 1) var = 0;
  BnFwd r;
  r.mean = (float)m;
  r.invstd = (float)(1.0 / sqrt(var + (double)eps));
  r.scale = count > 1 ? gamma * r.invstd : 0.f;
  r.shift = beta - (float)m * r.scale;
  r.var = var;
  return r;
}
// running_mean / running_var after this batch: `now` is BnFwd::mean / the unbiased variance
__device__ __forceinline__ float bn_unbiased(double var, double count) {
  return (float)(count > 1 ? var * count / (count - 1.0) : var);
}
__device__ __forceinline__ float bn_running(float old, float momentum, float now) {
  return (1.f - momentum) * old + momentum * now;
}

// ---------------------------------------------------------------------------- backward finalisation
struct BnBwd { float dgamma, dbeta, coef[3]; };      // dz = coef[0] * g + coef[1] * a + coef[2] (bn_dz)

// S1 = sum g, S2 = sum g * xhat (fp64) over |count| values -> the increments of dgamma / dbeta and the coefficients
__device__ __forceinline__ BnBwd bn_bwd_finalize(double S1, double S2, double count, double gamma, double is, double m) {
  BnBwd r;
  r.dgamma = (float)S2;
  r.dbeta = (float)S1;
  // count == 1: the output of a training BatchNorm over one value is the constant beta, its input gradient exactly 0
  // (the three terms below would leave the rounding residue of sc * S1 instead)
  const double sc = count == 1 ? 0.0 : gamma * is;
  r.coef[0] = (float)sc;
  // count < 0: FROZEN statistics (eval-mode BatchNorm, mean / invstd from the running buffers): the layer is a fixed
  // per-channel affine, the batch-mean terms of the training formula vanish; dgamma / dbeta are the same sums
  r.coef[1] = count < 0 ? 0.f : (float)(-sc * is * S2 / count);
  r.coef[2] = count < 0 ? 0.f : (float)(-sc * S1 / count + sc * is * (S2 / count) * m);
  return r;
}

// ---------------------------------------------------------------------------- per element
// a -> BN -> ReLU (post_relu): the gradient passes where the BatchNorm's output a * sc + sf was positive
__device__ __forceinline__ float bn_gate(float g, float a, float sc, float sf, int post_relu) {
  if (post_relu && !(a * sc + sf > 0.f)) g = 0.f;
  return g;
}
// the reduce's two terms of one (gated) element
__device__ __forceinline__ void bn_reduce_terms(float g, float a, float m, float is, float& s1, float& s2) {
  s1 += g;
  s2 += g * ((a - m) * is);
}
// the gradient in front of the layer: w.r.t. a (post_relu) or through a = lrelu(z, act_slope) w.r.t. z; g is gated
__device__ __forceinline__ float bn_dz(float g, float a, float c0, float c1, float c2, int post_relu, float act_slope) {
  const float d = c0 * g + c1 * a + c2;
  return post_relu ? d : d * (a > 0.f ? 1.f : act_slope);
}

// ---------------------------------------------------------------------------- the 256-slot fp64 tree
// N sums at once over a 256-thread workgroup: slot t pairs with slot t + o for o = 128 ... 1 (the pairing order is part of
// the result; slot_tree_sum of pointnet_small.hip maps the same association to registers).  The totals land in sh[.][0].
template <int N>
__device__ __forceinline__ void tree_sum_256(double (&sh)[N][256], const double (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) sh[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < N; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
    }
    __syncthreads();
  }
}
