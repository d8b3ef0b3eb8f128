// Fused optimiser steps on flat fp32 parameter / gradient buffers.
// Adam(betas=(0.9,0.99)) for the segmenter, SGD(momentum, weight_decay=5e-4) for the
// discriminators (train_mscmrseg.py:427-455).  Arithmetic follows torch.optim's single-tensor
// path so one step from identical state matches to rounding.
#include "common.h"

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long numel,
                                                   float lr_over_bc1, float beta1, float beta2, float eps,
                                                   float weight_decay, float inv_sqrt_bc2, float grad_scale) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < numel; i += 256ll * gridDim.x) {
    float gi = g[i] * grad_scale;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;        // exp_avg.lerp_(grad, 1-beta1)
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;   // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] = pi - lr_over_bc1 * (mi / denom);
  }
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ mom, long long numel, float lr, float momentum,
                                                  float weight_decay, int first_step, float grad_scale) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < numel; i += 256ll * gridDim.x) {
    const float pi = p[i];
    float gi = g[i] * grad_scale + weight_decay * pi;
    if (momentum != 0.f) {
      const float b = first_step ? gi : momentum * mom[i] + gi;
      mom[i] = b;
      gi = b;
    }
    p[i] = pi - lr * gi;
  }
}

extern "C" int pcuda_adam_step(float* p, const float* g, float* m, float* v, long long numel, float lr, float beta1,
                               float beta2, float eps, float weight_decay, int step, float grad_scale,
                               pcuda_stream_t s) {
  if (!p || !g || !m || !v || numel <= 0 || step < 1) PCUDA_FAIL(PCUDA_E_BADARG, "adam_step: bad arguments");
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float lr_over_bc1 = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const int blocks = (int)(cdiv(numel, 256) > 8192 ? 8192 : cdiv(numel, 256));
  ProfScope prof(PCUDA_FAM_POINTWISE, 28.0 * (double)numel, (hipStream_t)s);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, p, g, m, v, numel, lr_over_bc1, beta1,
                     beta2, eps, weight_decay, inv_sqrt_bc2, grad_scale);
  PCUDA_CHECK_LAUNCH("adam_kernel");
  return PCUDA_OK;
}

// Adam with the step count in device memory (incremented here, ahead of the update): a captured hipGraph of the
// train step replays correctly, which a host-side count baked into the kernel arguments would not.
__global__ void inc_i32_kernel(int* p) { *p += 1; }
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, long long numel,
                                                       float lr, float beta1, float beta2, float eps, float weight_decay,
                                                       const int* __restrict__ step_dev, float grad_scale) {
  const int step = *step_dev;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float lr_over_bc1 = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < numel; i += 256ll * gridDim.x) {
    float gi = g[i] * grad_scale;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] = pi - lr_over_bc1 * (mi / denom);
  }
}

extern "C" int pcuda_adam_step_dev(float* p, const float* g, float* m, float* v, long long numel, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, int* step_dev, float grad_scale,
                                   pcuda_stream_t s) {
  if (!p || !g || !m || !v || !step_dev || numel <= 0) PCUDA_FAIL(PCUDA_E_BADARG, "adam_step_dev: bad arguments");
  const int blocks = (int)(cdiv(numel, 256) > 8192 ? 8192 : cdiv(numel, 256));
  ProfScope prof(PCUDA_FAM_POINTWISE, 28.0 * (double)numel, (hipStream_t)s);
  hipLaunchKernelGGL(inc_i32_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, step_dev);
  hipLaunchKernelGGL(adam_dev_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, p, g, m, v, numel, lr, beta1, beta2,
                     eps, weight_decay, (const int*)step_dev, grad_scale);
  PCUDA_CHECK_LAUNCH("adam_dev_kernel");
  return PCUDA_OK;
}

extern "C" int pcuda_sgd_step(float* p, const float* g, float* mom, long long numel, float lr, float momentum,
                              float weight_decay, int first_step, float grad_scale, pcuda_stream_t s) {
  if (!p || !g || (momentum != 0.f && !mom) || numel <= 0) PCUDA_FAIL(PCUDA_E_BADARG, "sgd_step: bad arguments");
  const int blocks = (int)(cdiv(numel, 256) > 8192 ? 8192 : cdiv(numel, 256));
  ProfScope prof(PCUDA_FAM_POINTWISE, 20.0 * (double)numel, (hipStream_t)s);
  hipLaunchKernelGGL(sgd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, p, g, mom, numel, lr, momentum,
                     weight_decay, first_step, grad_scale);
  PCUDA_CHECK_LAUNCH("sgd_kernel");
  return PCUDA_OK;
}

// ---------------------------------------------------------------- guarded steps
// Global L2 norm of a flat gradient on the device, and update kernels that take "clip by how much" and "skip this step"
// from the record that norm leaves in device memory: no host round trip, so a captured graph replays the decision with
// the gradient it finds (a host-computed factor would be baked into the capture as a by-value argument).
struct GuardRecord {   // include/pcuda_hip.h: 8 words
  float norm, coef;
  int finite, skipped, applied, skip, pad0, pad1;
};
static_assert(sizeof(GuardRecord) == PCUDA_GUARD_RECORD_BYTES, "guard record layout");

// workgroups of the norm's first pass: 8 per CU on 256 CUs.  (The update kernels cap at 8192 workgroups of one element per
// lane; this one reads 16 bytes per lane and every workgroup leaves one partial for a single workgroup to sum.)
#define NORM_MAX_BLOCKS 2048
static_assert(NORM_MAX_BLOCKS * sizeof(double) == PCUDA_GRAD_NORM_WORKSPACE_BYTES, "norm workspace");

struct NormRanges {
  long long off[PCUDA_GUARD_MAX_RANGES];
  long long numel[PCUDA_GUARD_MAX_RANGES];
  int blk0[PCUDA_GUARD_MAX_RANGES + 1];   // range r owns workgroups [blk0[r], blk0[r + 1])
  int n;
};

// sum over the workgroup in a fixed order: lanes (xor butterfly), then the four waves in wave order; valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return t;
}

__device__ __forceinline__ double sq_d(float g, float grad_scale) {
  const double x = (double)(g * grad_scale);   // the very fp32 product the update kernels form
  return x * x;                                // exact: 24 x 24 significant bits
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, NormRanges R, float grad_scale,
                                                         double* __restrict__ partial) {
  __shared__ double sh[4];
  int r = 0;
  while (r + 1 < R.n && (int)blockIdx.x >= R.blk0[r + 1]) ++r;
  const int lb = (int)blockIdx.x - R.blk0[r], nb = R.blk0[r + 1] - R.blk0[r];
  const float* __restrict__ x = g + R.off[r];
  const long long numel = R.numel[r];
  // scalar head up to the first 16-byte boundary, float4 body, scalar tail
  long long head = (long long)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2);
  if (head > numel) head = numel;
  const long long nvec = (numel - head) >> 2;
  const long long tail0 = head + (nvec << 2);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (lb == 0) {
    if ((long long)threadIdx.x < head) a0 = sq_d(x[threadIdx.x], grad_scale);
    if (tail0 + (long long)threadIdx.x < numel) a1 = sq_d(x[tail0 + threadIdx.x], grad_scale);
  }
  const f32x4* __restrict__ xv = reinterpret_cast<const f32x4*>(x + head);
  for (long long i = lb * 256ll + threadIdx.x; i < nvec; i += 256ll * nb) {
    const f32x4* ptr = xv + i;
    const f32x4 q = *ptr;
    a0 += sq_d(q[0], grad_scale);
    a1 += sq_d(q[1], grad_scale);
    a2 += sq_d(q[2], grad_scale);
    a3 += sq_d(q[3], grad_scale);
    PCUDA_KEEP(ptr);
  }
  const double t = block_sum_d((a0 + a1) + (a2 + a3), sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, NormRanges R,
                                                               float max_norm, int skip_nonfinite,
                                                               GuardRecord* __restrict__ rec,
                                                               double* __restrict__ range_sumsq) {
  __shared__ double sh[4];
  double total = 0.0;
  for (int r = 0; r < R.n; ++r) {
    double a = 0.0;
    for (int i = R.blk0[r] + (int)threadIdx.x; i < R.blk0[r + 1]; i += 256) a += partial[i];
    const double t = block_sum_d(a, sh);
    if (threadIdx.x == 0 && range_sumsq) range_sumsq[r] = t;
    total += t;
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);
    float coef = 1.0f;
    if (max_norm > 0.f) {
      const float c = max_norm / (norm + 1e-6f);
      coef = c > 1.0f ? 1.0f : c;   // a NaN norm stays a NaN coefficient (torch.clamp(max=1))
    }
    const int finite = isfinite(norm) ? 1 : 0;
    const int skip = (skip_nonfinite && !finite) ? 1 : 0;
    rec->norm = norm;
    rec->coef = coef;
    rec->finite = finite;
    rec->skip = skip;
    if (skip) rec->skipped += 1;
    else rec->applied += 1;
  }
}

extern "C" int pcuda_grad_norm(const float* g, const long long* ranges, int nranges, float grad_scale, float max_norm,
                               int skip_nonfinite, void* record, double* range_sumsq, void* workspace,
                               size_t workspace_bytes, pcuda_stream_t s) {
  if (!g || !ranges || !record || !workspace || nranges < 1 || nranges > PCUDA_GUARD_MAX_RANGES)
    PCUDA_FAIL(PCUDA_E_BADARG, "grad_norm: bad arguments");
  if (workspace_bytes < PCUDA_GRAD_NORM_WORKSPACE_BYTES || ((uintptr_t)workspace & 7) || ((uintptr_t)g & 3) ||
      ((uintptr_t)record & 3) || ((uintptr_t)range_sumsq & 7))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "grad_norm: workspace too small or a misaligned pointer");
  NormRanges R;
  memset(&R, 0, sizeof(R));
  R.n = nranges;
  long long need[PCUDA_GUARD_MAX_RANGES], need_all = 0, numel_all = 0;
  for (int r = 0; r < nranges; ++r) {
    R.off[r] = ranges[2 * r];
    R.numel[r] = ranges[2 * r + 1];
    if (R.off[r] < 0 || R.numel[r] < 0) PCUDA_FAIL(PCUDA_E_BADARG, "grad_norm: range %d is negative", r);
    need[r] = (R.numel[r] + 1023) / 1024;   // 256 lanes x 4 elements
    need_all += need[r];
    numel_all += R.numel[r];
  }
  for (int r = 0; r < nranges; ++r) {
    long long nb = need[r];
    if (need_all > NORM_MAX_BLOCKS) {   // share the capped grid by size; a non-empty range keeps one workgroup
      nb = need[r] * (NORM_MAX_BLOCKS - nranges) / need_all;
      if (nb < 1 && need[r] > 0) nb = 1;
    }
    R.blk0[r + 1] = R.blk0[r] + (int)nb;
  }
  const int blocks = R.blk0[nranges];
  ProfScope prof(PCUDA_FAM_POINTWISE, 4.0 * (double)numel_all, (hipStream_t)s);
  if (blocks > 0) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, g, R, grad_scale,
                       (double*)workspace);
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const double*)workspace, R,
                     max_norm, skip_nonfinite, (GuardRecord*)record, range_sumsq);
  PCUDA_CHECK_LAUNCH("grad_norm");
  return PCUDA_OK;
}

// the step count moves only when the step is applied (in place of inc_i32_kernel)
__global__ void guard_inc_i32_kernel(int* p, const GuardRecord* __restrict__ rec, int skip_nonfinite) {
  if (!(skip_nonfinite && rec->finite == 0)) *p += 1;
}
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           long long numel, float lr, float beta1, float beta2, float eps,
                                                           float weight_decay, const int* __restrict__ step_dev,
                                                           float grad_scale, const GuardRecord* __restrict__ rec,
                                                           int skip_nonfinite) {
  if (skip_nonfinite && rec->finite == 0) return;
  const float coef = rec->coef;
  const int step = *step_dev;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float lr_over_bc1 = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < numel; i += 256ll * gridDim.x) {
    float gi = (g[i] * grad_scale) * coef;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] = pi - lr_over_bc1 * (mi / denom);
  }
}

extern "C" int pcuda_adam_step_guarded(float* p, const float* g, float* m, float* v, long long numel, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, int* step_dev,
                                       float grad_scale, const void* record, int skip_nonfinite, pcuda_stream_t s) {
  if (!p || !g || !m || !v || !step_dev || !record || numel <= 0)
    PCUDA_FAIL(PCUDA_E_BADARG, "adam_step_guarded: bad arguments");
  const int blocks = (int)(cdiv(numel, 256) > 8192 ? 8192 : cdiv(numel, 256));
  ProfScope prof(PCUDA_FAM_POINTWISE, 28.0 * (double)numel, (hipStream_t)s);
  hipLaunchKernelGGL(guard_inc_i32_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, step_dev, (const GuardRecord*)record,
                     skip_nonfinite);
  hipLaunchKernelGGL(adam_guarded_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, p, g, m, v, numel, lr, beta1,
                     beta2, eps, weight_decay, (const int*)step_dev, grad_scale, (const GuardRecord*)record,
                     skip_nonfinite);
  PCUDA_CHECK_LAUNCH("adam_guarded_kernel");
  return PCUDA_OK;
}

// "the momentum buffer is initialised" in device memory: a skipped first step must not consume the initialisation, and a
// replayed graph cannot re-read a host flag
__global__ void guard_set_i32_kernel(int* p, const GuardRecord* __restrict__ rec, int skip_nonfinite) {
  if (!(skip_nonfinite && rec->finite == 0)) *p = 1;
}
__global__ __launch_bounds__(256) void sgd_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ mom, long long numel, float lr,
                                                          float momentum, float weight_decay,
                                                          const int* __restrict__ init_dev, float grad_scale,
                                                          const GuardRecord* __restrict__ rec, int skip_nonfinite) {
  if (skip_nonfinite && rec->finite == 0) return;
  const float coef = rec->coef;
  const int first_step = (momentum != 0.f) ? (*init_dev == 0) : 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < numel; i += 256ll * gridDim.x) {
    const float pi = p[i];
    float gi = (g[i] * grad_scale) * coef + weight_decay * pi;
    if (momentum != 0.f) {
      const float b = first_step ? gi : momentum * mom[i] + gi;
      mom[i] = b;
      gi = b;
    }
    p[i] = pi - lr * gi;
  }
}

extern "C" int pcuda_sgd_step_guarded(float* p, const float* g, float* mom, long long numel, float lr, float momentum,
                                      float weight_decay, int* init_dev, int mark_init, float grad_scale,
                                      const void* record, int skip_nonfinite, pcuda_stream_t s) {
  if (!p || !g || !record || (momentum != 0.f && (!mom || !init_dev)) || numel <= 0)
    PCUDA_FAIL(PCUDA_E_BADARG, "sgd_step_guarded: bad arguments");
  const int blocks = (int)(cdiv(numel, 256) > 8192 ? 8192 : cdiv(numel, 256));
  ProfScope prof(PCUDA_FAM_POINTWISE, 20.0 * (double)numel, (hipStream_t)s);
  hipLaunchKernelGGL(sgd_guarded_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, p, g, mom, numel, lr, momentum,
                     weight_decay, (const int*)init_dev, grad_scale, (const GuardRecord*)record, skip_nonfinite);
  if (mark_init && init_dev) {
    hipLaunchKernelGGL(guard_set_i32_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, init_dev, (const GuardRecord*)record,
                       skip_nonfinite);
  }
  PCUDA_CHECK_LAUNCH("sgd_guarded_kernel");
  return PCUDA_OK;
}
