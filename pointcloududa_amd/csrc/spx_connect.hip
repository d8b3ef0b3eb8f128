// Connected superpixels: the opt-in connectivity pass behind a SUPERPIXELS slot of the stylize
// program (stylize.hip, f9), the device-side counterpart of skimage's enforce_connectivity = True with min_size_factor = 0.5
// that iaa.Superpixels runs with (data_generator_mscmrseg.py:46, :98, data_generator_mmwhs.py:41).
//
// Rule (this build's own, integers only; skimage is not vendored by the reference, parity with
// _enforce_label_connectivity_cython is unpinned; pinned by tests/golden/spx_connect.npz against two restatements).  Input: the
// label plane lab[h][w] the superpixel kernel leaves after its last assignment, the slot's input image, min_size = iarg[5] >= 1:
//   1. components: 4-connected components of equal labels (label 0 is a label like any other); a component's id is its
//      raster-first pixel's index r = y w + x, its size its own pixel count
//   2. a component is SMALL iff size < min_size and r != 0; its target is the component of pixel r - 1 if x > 0, else of pixel
//      r - w (always another component, with an id below r); targets are followed until a component that is not small: the
//      FINAL id of every pixel of the chain.  Merged pixels count towards nobody's size
//   3. a final segment (all pixels of one final id, 4-connected by induction) takes the colour rdiv(sum_ch, n) over its pixels of
//      the slot's input iff the first word of Philox4x32-10(key = seed, counter = final id) < iarg[4]; else its pixels are copied
//   iarg[5] == 0: no pass, the slot is f9's (counter = label k), bit for bit.  min_size == 1 merges nothing and recolours per piece.
// Not built: skimage's max_size_factor split, 8-connectivity.  imgaug's downscale to 128 pixels is built in spx_scale.hip
// (f9c, opt-in: iarg[6] = max_size, read by pcuda_stylize_scaled alone, which runs this pass on the working-size label plane
// of the scaled samples -- per-sample h' x w', ids r = y w' + x -- through spx_connect_scaled; ConnArgs.scale).
//
// pcuda_stylize_connect runs pcuda_stylize's launches unchanged (stylize_run: the superpixel kernel writes its label plane to
// the workspace and the unconnected image to the slot's output) and, behind every slot, the eight launches below over grids of
// (tiles, b).  Each workgroup reads its sample's opcode and iarg[5] with scalar loads and leaves at once unless the slot is a
// connected SUPERPIXELS slot (wave-uniform, as f9's kernels); the last launch overwrites the slot's output for those samples.
// The union-find is em_ccl_*'s (eval_metrics.hip): the larger root is hooked under the smaller with atomicMin, so a component's
// root is its minimum index, which is its raster-first pixel.
//   init      par[i] = i, size[i] = 0, sums[i][0..c] = 0
//   merge     unite(i, i + 1), unite(i, i + w) where the labels are equal
//   compress  par[i] = root
//   size      size[root] += pixels; a run of one root along memory shares one atomic
//   link      a small root takes its left (x > 0) or upper neighbour's parent as its own: that is the neighbour's component or,
//             if that component is small and has linked already, a component further up the same chain; ids only decrease, so
//             the parents form a forest whose roots are exactly the components that are not small
//   compress  again: every pixel walks to its forest root, however long the chain (no iteration count), par[i] = final id
//   sum       sums[final id][ch] += value, sums[final id][c] += 1; runs along memory share the atomics, inside a lane and,
//             with shuffles, across the lanes of a wave
//   write     out = replaced ? rdiv(sum, n) : in
// Integer atomics only (any order gives the same bits), 32-bit sums (h w <= 2^24, the entry point refuses more), no LDS, no
// scratch; every gather index is clamped into the plane BEFORE the load and every in-flight load's address stays alive
// (PCUDA_KEEP, VMEM address rule, common.h).
//
// Workspace (pcuda_stylize_connect_workspace_size), each part rounded up to 16 bytes:
//   [pcuda_stylize_workspace_size bytes: f9's label plane and ping-pong image] [par int32 b h w] [size uint32 b h w]
//   [sums uint32 b h w (c + 1)]
#include "common.h"
#include "image_device.h"
#include "stylize_host.h"

namespace {

enum { OP_SUPERPIXELS = 3 };
constexpr int kIArgs = 12, kMaxC = 4;
constexpr int kRun = 8;                     // consecutive pixels of one lane in the size and the sum kernel
constexpr long long kMaxPixels = 1ll << 24;

struct ConnArgs {
  const uint8_t* in;         // [b][h][w][c]: the slot's input
  uint8_t* out;              // [b][h][w][c]: the slot's output
  const uint8_t* labels;     // [b][h][w]
  const int* opcode;         // [b][slots]
  const int* iarg;           // [b][slots][12]
  const uint32_t* seed;      // [b][slots][2] (low, high word)
  int* par;                  // [b][h w]
  unsigned* size;            // [b][h w]
  unsigned* sums;            // [b][h w][c + 1]: colour sums, then the pixel count
  int h, w, c, slots, slot;
  // f9c, set by pcuda_stylize_scaled alone (0 from pcuda_stylize_connect, which never reads iarg[6]): 1 = the kernels stand
  // aside for the samples whose slot is scaled, 2 = they run those samples alone, on their working size (rows of w' pixels;
  // a sample's planes stay h w apart), and the write kernel leaves `flag`
  int scale;
  int* flag;                 // [b] (scale == 2): 1 iff a final segment is replaced
};

// min_size of sample n's slot, 0 when it is not a connected SUPERPIXELS slot or belongs to the other launch of a scaled
// run (blockIdx-uniform: scalar loads); h x w = the size the sample's planes are walked at
__device__ __forceinline__ int conn_min_size(const ConnArgs& a, int n, int& h, int& w) {
  h = a.h; w = a.w;
  const int at = n * a.slots + a.slot;
  if (a.opcode[at] != OP_SUPERPIXELS) return 0;
  const int m = a.iarg[at * kIArgs + 5];
  if (a.scale != 0) {
    const bool scaled = imgdev::spx_working_size(a.h, a.w, a.iarg[at * kIArgs + 6], h, w);
    if (scaled != (a.scale == 2)) return 0;
  }
  return m <= 0 ? 0 : min(m, h * w);
}

using imgdev::philox_word0;

__device__ __forceinline__ int conn_parent(int* par, int x) {      // agent-scope load: sees the other blocks' hooks
  int* p = par + x;
  const int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  PCUDA_KEEP(p);
  return v;
}
__device__ __forceinline__ int conn_find(int* par, int x) {
  int p = conn_parent(par, x);
  while (p != x) { x = p; p = conn_parent(par, x); }
  return x;
}
// hook the larger root under the smaller one: a component's root ends as its minimum linear index
__device__ __forceinline__ void conn_unite(int* par, int a, int b) {
  a = conn_find(par, a);
  b = conn_find(par, b);
  while (a != b) {
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + b, a);
    if (old == b) break;
    a = conn_find(par, a);
    b = conn_find(par, old);
  }
}

__global__ __launch_bounds__(256) void spx_connect_init_kernel(const ConnArgs a) {
  const int n = blockIdx.y;
  int h, w;
  if (conn_min_size(a, n, h, w) == 0) return;
  const int hw = h * w, c1 = a.c + 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  if (a.scale == 2 && i == 0) a.flag[n] = 0;      // (the superpixel kernel left its own answer: the write kernel's replaces it)
  const long long at = (long long)n * a.h * a.w + i;
  a.par[at] = i;
  a.size[at] = 0;
  unsigned* q = a.sums + at * c1;
#pragma unroll
  for (int ch = 0; ch <= kMaxC; ++ch)
    if (ch < c1) q[ch] = 0;
}

__global__ __launch_bounds__(256) void spx_connect_merge_kernel(const ConnArgs a) {
  const int n = blockIdx.y;
  int h, w;
  if (conn_min_size(a, n, h, w) == 0) return;
  const int hw = h * w;
  const long long plane = (long long)a.h * a.w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int y = i / w, x = i - y * w;
  const bool right = x + 1 < w, down = y + 1 < h;
  const uint8_t* lab = a.labels + n * plane;
  const uint8_t* p0 = lab + i;
  const uint8_t* p1 = lab + (right ? i + 1 : i);
  const uint8_t* p2 = lab + (down ? i + w : i);
  const int v0 = *p0, v1 = *p1, v2 = *p2;
  PCUDA_KEEP(p0); PCUDA_KEEP(p1); PCUDA_KEEP(p2);
  int* par = a.par + n * plane;
  if (right && v1 == v0) conn_unite(par, i, i + 1);
  if (down && v2 == v0) conn_unite(par, i, i + w);
}

// par[i] = the root of i's tree; a concurrent lane's write replaces a parent by one further up the same tree
__global__ __launch_bounds__(256) void spx_connect_compress_kernel(const ConnArgs a) {
  const int n = blockIdx.y;
  int h, w;
  if (conn_min_size(a, n, h, w) == 0) return;
  const int hw = h * w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  int* par = a.par + (long long)n * a.h * a.w;
  int r = conn_parent(par, i);
  if (r == i) return;
  for (;;) {
    const int q = conn_parent(par, r);
    if (q == r) break;
    r = q;
  }
  __hip_atomic_store(par + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// size[root] += pixels; runs of one root along memory share one atomic
__global__ __launch_bounds__(256) void spx_connect_size_kernel(const ConnArgs a) {
  const int n = blockIdx.y;
  int h, w;
  if (conn_min_size(a, n, h, w) == 0) return;
  const int hw = h * w;
  const long long plane = (long long)a.h * a.w;
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * kRun;
  if (i0 >= hw) return;
  const int i1 = min(i0 + kRun, hw);
  const int* par = a.par + n * plane;
  unsigned* size = a.size + n * plane;
  int cur = -1;
  unsigned cnt = 0;
  for (int i = i0; i < i1; ++i) {
    const int* pi = par + i;
    const int r = *pi;
    PCUDA_KEEP(pi);
    if (r != cur) {
      if (cur >= 0) atomicAdd(size + cur, cnt);
      cur = r;
      cnt = 0;
    }
    ++cnt;
  }
  if (cur >= 0) atomicAdd(size + cur, cnt);
}

// a small root (size < min_size, not pixel 0) hangs itself under its left or upper neighbour's parent
__global__ __launch_bounds__(256) void spx_connect_link_kernel(const ConnArgs a) {
  const int n = blockIdx.y;
  int h, w;
  const int min_size = conn_min_size(a, n, h, w);
  if (min_size == 0) return;
  const int hw = h * w;
  const long long plane = (long long)a.h * a.w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw || i == 0) return;
  int* par = a.par + n * plane;
  if (conn_parent(par, i) != i) return;
  const unsigned* ps = a.size + n * plane + i;
  const unsigned sz = *ps;
  PCUDA_KEEP(ps);
  if (sz >= (unsigned)min_size) return;
  const int x = i % w;
  const int nb = max(x > 0 ? i - 1 : i - w, 0);      // (i > 0 and x == 0 is a row below the first)
  const int t = conn_parent(par, nb);                // below i: nb < i is in another component and ids only decrease
  __hip_atomic_store(par + i, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sums[final id] += (colour, 1).  A lane walks kRun consecutive pixels and issues atomics of its own only where the id changes
// inside its run; the lanes' last runs are consecutive along memory, so a wave adds up each stretch of lanes with one id with
// shuffles (stylize.hip's segmented sum) and only the stretch's first lane issues the atomics
__global__ __launch_bounds__(256) void spx_connect_sum_kernel(const ConnArgs a) {
  const int n = blockIdx.y;
  int h, w;
  if (conn_min_size(a, n, h, w) == 0) return;
  const int hw = h * w, c = a.c, c1 = c + 1;
  const long long plane = (long long)a.h * a.w;
  const int lane = threadIdx.x & 63;
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * kRun;      // (a lane past the plane walks nothing and keeps cur = -1)
  const int i1 = min(i0 + kRun, hw);
  const int* par = a.par + n * plane;
  const uint8_t* src = a.in + n * plane * c;
  unsigned* sums = a.sums + n * plane * c1;
  int cur = -1;
  int acc[kMaxC] = {0, 0, 0, 0}, cnt = 0;
  for (int i = i0; i < i1; ++i) {
    const int* pi = par + i;
    const uint8_t* p = src + (long long)i * c;
    const int r = *pi;
    int v[kMaxC];
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch) v[ch] = ch < c ? (int)p[ch] : 0;
    PCUDA_KEEP(pi); PCUDA_KEEP(p);
    if (r != cur) {
      if (cur >= 0) {
        unsigned* q = sums + (long long)cur * c1;
#pragma unroll
        for (int ch = 0; ch < kMaxC; ++ch)
          if (ch < c) atomicAdd(q + ch, (unsigned)acc[ch]);
        atomicAdd(q + c, (unsigned)cnt);
      }
      cur = r;
      cnt = 0;
#pragma unroll
      for (int ch = 0; ch < kMaxC; ++ch) acc[ch] = 0;
    }
    ++cnt;
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch) acc[ch] += v[ch];
  }
  // every lane of the wave is here (no lane has left): stretches of lanes whose last run has one id
  const int prev = __shfl_up(cur, 1);
  const bool head_flag = lane == 0 || prev != cur;
  const unsigned long long heads = __ballot(head_flag);
  const int head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int oh = __shfl_down(head, off), on = __shfl_down(cnt, off);
    int oa[kMaxC];
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch) oa[ch] = __shfl_down(acc[ch], off);
    if (lane + off < 64 && oh == head) {
      cnt += on;
#pragma unroll
      for (int ch = 0; ch < kMaxC; ++ch) acc[ch] += oa[ch];
    }
  }
  if (head_flag && cur >= 0) {
    unsigned* q = sums + (long long)cur * c1;
#pragma unroll
    for (int ch = 0; ch < kMaxC; ++ch)
      if (ch < c) atomicAdd(q + ch, (unsigned)acc[ch]);
    atomicAdd(q + c, (unsigned)cnt);
  }
}

__global__ __launch_bounds__(256) void spx_connect_write_kernel(const ConnArgs a) {
  const int n = blockIdx.y;
  int h, w;
  if (conn_min_size(a, n, h, w) == 0) return;
  const int hw = h * w, c = a.c, c1 = c + 1;
  const long long plane = (long long)a.h * a.w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int at = n * a.slots + a.slot;
  const uint32_t thr = (uint32_t)a.iarg[at * kIArgs + 4];
  const uint32_t* sd = a.seed + 2 * at;
  asm volatile("" : "+v"(sd));      // a vector address of its own, kept alive below (as stylize.hip)
  const uint32_t k0 = sd[0], k1 = sd[1];
  const int* pi = a.par + n * plane + i;
  const int id = min(max(*pi, 0), hw - 1);
  const unsigned* q = a.sums + (n * plane + id) * c1;
  const uint8_t* p = a.in + (n * plane + i) * c;
  unsigned sum[kMaxC + 1];
  uint8_t v[kMaxC];
#pragma unroll
  for (int ch = 0; ch <= kMaxC; ++ch) sum[ch] = ch < c1 ? q[ch] : 0u;
#pragma unroll
  for (int ch = 0; ch < kMaxC; ++ch) v[ch] = ch < c ? p[ch] : (uint8_t)0;
  const bool rep = philox_word0(k0, k1, (uint32_t)id) < thr;
  PCUDA_KEEP(sd); PCUDA_KEEP(pi); PCUDA_KEEP(q); PCUDA_KEEP(p);
  unsigned cnt = 1;
#pragma unroll
  for (int ch = 0; ch <= kMaxC; ++ch)
    if (ch == c) cnt = max(sum[ch], 1u);
  if (a.scale == 2 && rep) a.flag[n] = 1;      // (zeroed by the init kernel; every writer stores 1)
  uint8_t* dst = a.out + (n * plane + i) * c;
#pragma unroll
  for (int ch = 0; ch < kMaxC; ++ch)
    if (ch < c) {
      const unsigned long long mean = (2ull * sum[ch] + cnt) / (2ull * cnt);      // rdiv, operands >= 0
      dst[ch] = rep ? (uint8_t)mean : v[ch];
    }
}


struct ConnCtx {
  ConnArgs a;
  int b;
  hipStream_t s;
};

int connect_slot(void* ctx, int slot, const uint8_t* slot_in, uint8_t* slot_out, const uint8_t* labels) {
  ConnCtx* k = (ConnCtx*)ctx;
  ConnArgs a = k->a;
  a.in = slot_in; a.out = slot_out; a.labels = labels; a.slot = slot;
  const long long hw = (long long)a.h * a.w;
  const dim3 grid(cdiv(hw, 256), k->b), grid_run(cdiv(hw, 256 * kRun), k->b);
  hipLaunchKernelGGL(spx_connect_init_kernel, grid, dim3(256), 0, k->s, a);
  PCUDA_CHECK_LAUNCH("spx_connect_init_kernel");
  hipLaunchKernelGGL(spx_connect_merge_kernel, grid, dim3(256), 0, k->s, a);
  PCUDA_CHECK_LAUNCH("spx_connect_merge_kernel");
  hipLaunchKernelGGL(spx_connect_compress_kernel, grid, dim3(256), 0, k->s, a);
  PCUDA_CHECK_LAUNCH("spx_connect_compress_kernel");
  hipLaunchKernelGGL(spx_connect_size_kernel, grid_run, dim3(256), 0, k->s, a);
  PCUDA_CHECK_LAUNCH("spx_connect_size_kernel");
  hipLaunchKernelGGL(spx_connect_link_kernel, grid, dim3(256), 0, k->s, a);
  PCUDA_CHECK_LAUNCH("spx_connect_link_kernel");
  hipLaunchKernelGGL(spx_connect_compress_kernel, grid, dim3(256), 0, k->s, a);
  PCUDA_CHECK_LAUNCH("spx_connect_compress_kernel");
  hipLaunchKernelGGL(spx_connect_sum_kernel, grid_run, dim3(256), 0, k->s, a);
  PCUDA_CHECK_LAUNCH("spx_connect_sum_kernel");
  hipLaunchKernelGGL(spx_connect_write_kernel, grid, dim3(256), 0, k->s, a);
  PCUDA_CHECK_LAUNCH("spx_connect_write_kernel");
  return PCUDA_OK;
}

// par, size and sums behind `base` (the connect workspace less pcuda_stylize's own part)
void conn_layout(ConnArgs& a, void* base, int b, int h, int w, int c) {
  const size_t px = (size_t)b * h * w;
  uint8_t* p = (uint8_t*)base;
  a.par = (int*)p;
  a.size = (unsigned*)(p + round16(4 * px));
  a.sums = (unsigned*)(p + 2 * round16(4 * px));
}

}  // namespace

int spx_connect_scaled(const uint8_t* slot_in, uint8_t* slot_out, const uint8_t* labels, void* conn_workspace, int* flag, int scale,
                       int b, int h, int w, int c, int slots, int slot, const int* opcode, const int* iarg,
                       const unsigned long long* seed, pcuda_stream_t s) {
  ConnCtx k;
  memset(&k, 0, sizeof(k));
  k.b = b; k.s = (hipStream_t)s;
  k.a.opcode = opcode; k.a.iarg = iarg; k.a.seed = reinterpret_cast<const uint32_t*>(seed);
  k.a.h = h; k.a.w = w; k.a.c = c; k.a.slots = slots;
  k.a.scale = scale; k.a.flag = flag;
  conn_layout(k.a, conn_workspace, b, h, w, c);
  return connect_slot(&k, slot, slot_in, slot_out, labels);
}

extern "C" size_t pcuda_stylize_connect_workspace_size(int b, int h, int w, int c) {
  if (b <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  const size_t px = (size_t)b * h * w;
  return pcuda_stylize_workspace_size(b, h, w, c) + 2 * round16(4 * px) + round16(4 * px * ((size_t)c + 1));
}

extern "C" int pcuda_stylize_connect(const uint8_t* in, uint8_t* out, int b, int h, int w, int c, int slots, const int* opcode,
                                     const int* iarg, const double* farg, const double* table, const unsigned long long* seed,
                                     void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (h > 0 && w > 0 && (long long)h * w > kMaxPixels)
    PCUDA_FAIL(PCUDA_E_BADARG, "stylize_connect: h w above 2^24 (the segment sums are 32-bit)");
  ConnCtx k;
  memset(&k, 0, sizeof(k));
  k.b = b; k.s = (hipStream_t)s;
  k.a.opcode = opcode; k.a.iarg = iarg; k.a.seed = reinterpret_cast<const uint32_t*>(seed);
  k.a.h = h; k.a.w = w; k.a.c = c; k.a.slots = slots;
  if (workspace && b > 0 && h > 0 && w > 0 && c > 0)
    conn_layout(k.a, (uint8_t*)workspace + pcuda_stylize_workspace_size(b, h, w, c), b, h, w, c);
  return stylize_run(in, out, b, h, w, c, slots, opcode, iarg, farg, table, seed, workspace, workspace_bytes,
                     pcuda_stylize_connect_workspace_size(b, h, w, c), s, connect_slot, &k, 0);
}
