// Superpixels at a working size: the opt-in max_size of a SUPERPIXELS slot of the stylize program
// (stylize.hip, f9; spx_connect.hip, f9b), the device-side counterpart of iaa.Superpixels' max_size = 128
// (data_generator_mscmrseg.py:46, :98, data_generator_mmwhs.py:41): an image whose longer side exceeds max_size is resized
// down linearly, segmented and painted there, and the painted image is resized back linearly.
//
// Rule (this build's own, integers only; imgaug, cv2 and skimage are not vendored by the reference, parity with them is
// unpinned; pinned by tests/golden/spx_scaled.npz against two restatements).  iarg[6] = m is the slot's max_size; the slot is
// SCALED iff m >= 1 and L = max(H, W) > m, else it is f9's / f9b's slot bit for bit.  For a scaled slot:
//   1. working size  h' = max(1, (H m) / L), w' = max(1, (W m) / L) (integer division: the longer side is exactly m)
//   2. linear resize R(src[Sh x Sw x C] -> Dh x Dw), per axis with source size S and destination size D:
//      a = clip((2 d + 1) S - D, 0, 2 D (S - 1)) (the coordinate (d + 0.5) S / D - 0.5 times 2 D, clamped into the image),
//      i0 = a / (2 D), t = a - 2 D i0, i1 = min(i0 + 1, S - 1); num = (2 Dh - ty) ((2 Dw - tx) p00 + tx p01) + ty ((2 Dw - tx) p10
//      + tx p11), den = 4 Dh Dw, value = floor((2 num + den) / (2 den)): two taps per axis, half-pixel centres, round half
//      up, 64-bit integers, no float
//   3. small = R(slot input -> h' x w'); f9's grid SLIC runs on small with h', w' in place of H, W everywhere; iarg[5] >= 1
//      runs f9b's rule on the working-size label plane (ids and Philox counters r = y w' + x); the repaint with rdiv(sum, n)
//      over the pixels of small gives painted
//   4. out = R(painted -> H x W) -- unless no final segment that holds a pixel is replaced: then the sample's output is the
//      slot's input bit for bit, not the blurred round trip (recalled as imgaug's own shortcut, not checkable here: this
//      build's choice)
//
// pcuda_stylize_scaled runs pcuda_stylize's launches (stylize_run with scale = 1: the superpixel kernel stands aside for
// the scaled samples) and, behind every slot: the connectivity pass for the samples that are not scaled (spx_connect_scaled,
// scale = 1: pcuda_stylize_connect's launches), the downscale below, the superpixel kernel and the connectivity pass on the
// scaled samples alone (scale = 2: per-sample h', w'), and the upscale below into the slot's output.  Each workgroup reads
// its sample's opcode and iarg[6] with scalar loads and leaves at once unless the slot is a scaled SUPERPIXELS slot
// (workgroup-uniform); one lane per destination pixel; every tap index is clamped into its plane BEFORE the load (the clip of
// a, the min of i1) and every in-flight load's address stays alive (PCUDA_KEEP, VMEM address rule, common.h); no atomics (one
// writer per byte; the flag's writers all store 1).  A sample's working image sits at the sample's full-size offset.
//
// Workspace (pcuda_stylize_scaled_workspace_size), each part rounded up to 16 bytes:
//   [pcuda_stylize_connect_workspace_size bytes, laid out as pcuda_stylize_connect's] [small uint8 b h w c]
//   [painted uint8 b h w c] [flag int32 b]
#include "common.h"
#include "image_device.h"
#include "stylize_host.h"

namespace {

enum { OP_SUPERPIXELS = 3 };
constexpr int kIArgs = 12, kMaxC = 4;
constexpr long long kMaxPixels = 1ll << 24;      // (pcuda_stylize_connect's limit: the pass serves connected slots too)

struct ScaleArgs {
  const uint8_t* src;        // [b][h][w][c]: down: the slot's input; up: painted
  uint8_t* dst;              // [b][h][w][c]: down: small; up: the slot's output
  const uint8_t* keep;       // [b][h][w][c] (up): the slot's input, copied where nothing is replaced
  const int* opcode;         // [b][slots]
  const int* iarg;           // [b][slots][12]
  int* flag;                 // [b]: zeroed by the downscale, read by the upscale
  int h, w, c, slots, slot;
};

// the working size of sample n's slot; false unless it is a scaled SUPERPIXELS slot (blockIdx-uniform: scalar loads)
__device__ __forceinline__ bool scale_dims(const ScaleArgs& a, int n, int& h2, int& w2) {
  const int at = n * a.slots + a.slot;
  h2 = a.h; w2 = a.w;
  if (a.opcode[at] != OP_SUPERPIXELS) return false;
  return imgdev::spx_working_size(a.h, a.w, a.iarg[at * kIArgs + 6], h2, w2);
}

// the two taps of destination index d on an axis resized from S to D, and the weight t (of 2 D) of the second
__device__ __forceinline__ void lin_taps(int d, int S, int D, int& i0, int& i1, long long& t) {
  const long long hi = 2ll * D * (S - 1);
  long long a = (2ll * d + 1) * S - D;
  a = a < 0 ? 0 : (a > hi ? hi : a);
  i0 = (int)(a / (2ll * D));
  t = a - 2ll * D * i0;
  i1 = min(i0 + 1, S - 1);
}

// pixel (y, x) of R(src[sh x sw x c] -> dh x dw), all channels
__device__ __forceinline__ void resize_pixel(const uint8_t* src, int sh, int sw, int dh, int dw, int c, int y, int x,
                                             uint8_t (&v)[kMaxC]) {
  int y0, y1, x0, x1;
  long long ty, tx;
  lin_taps(y, sh, dh, y0, y1, ty);
  lin_taps(x, sw, dw, x0, x1, tx);
  const uint8_t* p00 = src + ((long long)y0 * sw + x0) * c;
  const uint8_t* p01 = src + ((long long)y0 * sw + x1) * c;
  const uint8_t* p10 = src + ((long long)y1 * sw + x0) * c;
  const uint8_t* p11 = src + ((long long)y1 * sw + x1) * c;
  long long q[4][kMaxC];
#pragma unroll
  for (int ch = 0; ch < kMaxC; ++ch) {
    q[0][ch] = ch < c ? p00[ch] : 0; q[1][ch] = ch < c ? p01[ch] : 0;
    q[2][ch] = ch < c ? p10[ch] : 0; q[3][ch] = ch < c ? p11[ch] : 0;
  }
  PCUDA_KEEP(p00); PCUDA_KEEP(p01); PCUDA_KEEP(p10); PCUDA_KEEP(p11);
  const long long wy = 2ll * dh, wx = 2ll * dw, den = wy * wx;
#pragma unroll
  for (int ch = 0; ch < kMaxC; ++ch) {
    const long long num = (wy - ty) * ((wx - tx) * q[0][ch] + tx * q[1][ch]) + ty * ((wx - tx) * q[2][ch] + tx * q[3][ch]);
    v[ch] = (uint8_t)((2 * num + den) / (2 * den));      // (operands >= 0; a convex mix of bytes rounds into 0..255)
  }
}

// small = R(slot input -> h' x w'); lane 0 of the sample's first block zeroes the sample's flag
__global__ __launch_bounds__(256) void spx_scale_down_kernel(const ScaleArgs a) {
  const int n = blockIdx.y;
  int h2, w2;
  if (!scale_dims(a, n, h2, w2)) return;
  const int c = a.c;
  const long long plane = (long long)a.h * a.w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) a.flag[n] = 0;
  if (i >= h2 * w2) return;
  const int y = i / w2, x = i - y * w2;
  uint8_t v[kMaxC];
  resize_pixel(a.src + n * plane * c, a.h, a.w, h2, w2, c, y, x, v);
  uint8_t* dst = a.dst + (n * plane + i) * c;
#pragma unroll
  for (int ch = 0; ch < kMaxC; ++ch)
    if (ch < c) dst[ch] = v[ch];
}

// out = flag ? R(painted -> H x W) : the slot's input
__global__ __launch_bounds__(256) void spx_scale_up_kernel(const ScaleArgs a) {
  const int n = blockIdx.y;
  int h2, w2;
  if (!scale_dims(a, n, h2, w2)) return;
  const int c = a.c, w = a.w;
  const long long plane = (long long)a.h * w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  const int* pf = a.flag + n;
  const int replaced = *pf;
  PCUDA_KEEP(pf);
  uint8_t v[kMaxC];
  if (replaced != 0) {      // (one value per sample: workgroup-uniform)
    const int y = i / w, x = i - y * w;
    resize_pixel(a.src + n * plane * c, h2, w2, a.h, w, c, y, x, v);
  } else {
    const uint8_t* p = a.keep + (n * plane + i) * c;
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch) v[ch] = ch < c ? p[ch] : (uint8_t)0;
    PCUDA_KEEP(p);
  }
  uint8_t* dst = a.dst + (n * plane + i) * c;
#pragma unroll
  for (int ch = 0; ch < kMaxC; ++ch)
    if (ch < c) dst[ch] = v[ch];
}

struct ScaleCtx {
  ScaleArgs a;
  const unsigned long long* seed;
  void* conn_workspace;
  uint8_t* small;
  uint8_t* painted;
  int b;
  pcuda_stream_t s;
};

int scale_slot(void* ctx, int slot, const uint8_t* slot_in, uint8_t* slot_out, const uint8_t* labels) {
  ScaleCtx* k = (ScaleCtx*)ctx;
  ScaleArgs a = k->a;
  a.slot = slot;
  const long long hw = (long long)a.h * a.w;
  const dim3 grid(cdiv(hw, 256), k->b);
  // the samples whose slot is not scaled: pcuda_stylize_connect's pass behind the launches stylize_run just made
  int rc = spx_connect_scaled(slot_in, slot_out, labels, k->conn_workspace, a.flag, 1, k->b, a.h, a.w, a.c, a.slots, slot, a.opcode,
                              a.iarg, k->seed, k->s);
  if (rc != PCUDA_OK) return rc;
  a.src = slot_in; a.dst = k->small; a.keep = nullptr;
  hipLaunchKernelGGL(spx_scale_down_kernel, grid, dim3(256), 0, (hipStream_t)k->s, a);
  PCUDA_CHECK_LAUNCH("spx_scale_down_kernel");
  // (the label plane is the workspace's: the scaled samples' part was left alone by stylize_run's launch)
  rc = stylize_superpixels_scaled(k->small, k->painted, const_cast<uint8_t*>(labels), a.flag, k->b, a.h, a.w, a.c, a.slots, slot,
                                  a.opcode, a.iarg, k->seed, k->s);
  if (rc != PCUDA_OK) return rc;
  rc = spx_connect_scaled(k->small, k->painted, labels, k->conn_workspace, a.flag, 2, k->b, a.h, a.w, a.c, a.slots, slot, a.opcode,
                          a.iarg, k->seed, k->s);
  if (rc != PCUDA_OK) return rc;
  a.src = k->painted; a.dst = slot_out; a.keep = slot_in;
  hipLaunchKernelGGL(spx_scale_up_kernel, grid, dim3(256), 0, (hipStream_t)k->s, a);
  PCUDA_CHECK_LAUNCH("spx_scale_up_kernel");
  return PCUDA_OK;
}

}  // namespace

extern "C" size_t pcuda_stylize_scaled_workspace_size(int b, int h, int w, int c) {
  if (b <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  return pcuda_stylize_connect_workspace_size(b, h, w, c) + 2 * round16((size_t)b * h * w * c) + round16(4 * (size_t)b);
}

extern "C" int pcuda_stylize_scaled(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode,
                                    const int* iarg, const double* farg, const double* table, const unsigned long long* seed,
                                    void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (h > 0 && w > 0 && (long long)h * w > kMaxPixels)
    PCUDA_FAIL(PCUDA_E_BADARG, "stylize_scaled: h w above 2^24 (the segment sums of connected slots are 32-bit)");
  ScaleCtx k;
  memset(&k, 0, sizeof(k));
  k.b = b; k.s = s; k.seed = seed;
  k.a.opcode = opcode; k.a.iarg = iarg;
  k.a.h = h; k.a.w = w; k.a.c = c; k.a.slots = slots;
  if (workspace && b > 0 && h > 0 && w > 0 && c > 0) {
    const size_t img = round16((size_t)b * h * w * c);
    uint8_t* p = (uint8_t*)workspace;
    k.conn_workspace = p + pcuda_stylize_workspace_size(b, h, w, c);
    p += pcuda_stylize_connect_workspace_size(b, h, w, c);
    k.small = p;
    k.painted = p + img;
    k.a.flag = (int*)(p + 2 * img);
  }
  return stylize_run(in, out, b, h, w, c, slots, opcode, iarg, farg, table, seed, workspace, workspace_bytes,
                     pcuda_stylize_scaled_workspace_size(b, h, w, c), s, scale_slot, &k, 1);
}
