// MM-WHS / MS-CMRSeg test volumes on the device: the plumbing of the reference's evaluate scripts
// around the network -- read_img's np.moveaxis(vol, 2, 0)[:, ::-1, ::-1], its 2.5-D stack img[[i - 1, i, (i + 1) % D]] and
// to_categorical (evaluate_mmwhs.py:19-29), the nimg.T of evaluate_mscmrseg.py:147 -- and the way back from a prediction
// [D][H][W] to the volume's own axis order.  No arithmetic but the casts: everything is pinned bit for bit by numpy.
//
// One index map serves the three entry points:
//   src(z, r, c) = base + z sz + (flip_r ? R - 1 - r : r) sr + (flip_c ? C - 1 - c : c) sc        (elements)
// C order, Fortran order and any permuted view are strides only.  The host folds the flips into the pointer and into SIGNED
// strides (View), so the kernels see  p + z sz + r sr + c sc  and pick their form from the strides' magnitudes:
//   row_kernel    lanes along c, one value each: |sc| == 1 (both sides then run along their fastest axis) and, with no unit
//                 stride at all, the plain gather / scatter
//   row4_kernel   the same with four neighbouring columns per lane: one 4 / 8 / 16-byte access per side (two for float64) where
//                 pointers, pitches and C allow it; a flipped row is read as the mirrored group and reversed in registers
//   tile_kernel   |sr| == 1 or |sz| == 1: a 64 x 64 tile of (c, f), f the unit-stride axis, through LDS padded to 65 words:
//                 lanes run along f on the caller's side and along c on the contiguous side, so that global reads and writes
//                 both go along their own fastest axis; the flips are in the addresses, that is, inside the tile
// Every source value is read ONCE.  The window of the 2.5-D stack is made on the write side: slice z goes to channel 1 of
// sample z, channel 0 of sample (z + 1) mod Z and channel 2 of sample (z - 1) mod Z (three stores along c), which is the
// reference's gather transposed; Z = 1 and Z = 2 need no special case.
// All offsets are 64-bit.  Every in-flight load's address stays alive (PCUDA_KEEP, VMEM address rule, common.h).
#include <math.h>

#include <type_traits>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;
constexpr int kMaxRemap = 8;
constexpr long long kMaxGridX = 1 << 20;
constexpr int kMaxGridY = 65535;

// the caller's array behind the map, flips folded in: element (z, r, c) lies at p[z sz + r sr + c sc], strides signed
template <typename T>
struct View {
  T* p;
  long long sz, sr, sc;
  __device__ __forceinline__ long long at(int z, int r, int c) const { return z * sz + r * sr + c * sc; }
};

template <typename T>
struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) Pack4 {
  T v[4];
};

template <typename T>
__device__ __forceinline__ T load1(const View<const T>& s, int z, int r, int c) {
  const T* q = s.p + s.at(z, r, c);
  const T v = *q;
  PCUDA_KEEP(q);
  return v;
}
// columns c .. c + 3 of a row with |sc| == 1, as one aligned group (the host has checked the alignment)
template <typename T>
__device__ __forceinline__ void load4(const View<const T>& s, int z, int r, int c, T (&v)[4]) {
  const bool rev = s.sc < 0;
  const T* q = s.p + s.at(z, r, c) - (rev ? 3 : 0);
  const Pack4<T> k = *reinterpret_cast<const Pack4<T>*>(q);
  PCUDA_KEEP(q);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = rev ? k.v[3 - j] : k.v[j];
}
template <typename T>
__device__ __forceinline__ void store4(const View<T>& d, int z, int r, int c, const T (&v)[4]) {
  const bool rev = d.sc < 0;
  Pack4<T> k;
#pragma unroll
  for (int j = 0; j < 4; ++j) k.v[j] = rev ? v[3 - j] : v[j];
  *reinterpret_cast<Pack4<T>*>(d.p + d.at(z, r, c) - (rev ? 3 : 0)) = k;
}

// r = p / n, c = p - r n: 32-bit where the plane allows it
__device__ __forceinline__ void split(long long p, int n, int& r, int& c) {
  if (p < (1ll << 32)) {
    const unsigned q = (unsigned)p / (unsigned)n;
    r = (int)q;
    c = (int)((unsigned)p - q * (unsigned)n);
  } else {
    const long long q = p / n;
    r = (int)q;
    c = (int)(p - q * n);
  }
}

// ------------------------------------------------------------------------------------------ the three operations
// An Op moves one value (z, r, c) from its source to its destination(s): load() -> a 32-bit staged word, store() takes it;
// move4() is both for four neighbouring columns; store() and move4() return a count that finish() takes once per lane at the end.

// slices: T -> fp32 (float64 rounds to nearest even like numpy's astype), out [Z][window][R][C]
template <typename T>
struct SliceOp {
  View<const T> src;
  float* out;
  int Z, R, C, window;
  __device__ __forceinline__ uint32_t load(int z, int r, int c) const { return __builtin_bit_cast(uint32_t, (float)load1(src, z, r, c)); }
  template <typename V>
  __device__ __forceinline__ void put(int z, int r, int c, V v) const {
    const long long plane = (long long)R * C, px = (long long)r * C + c;
    if (window == 1) {
      *reinterpret_cast<V*>(out + z * plane + px) = v;
    } else {
      const int zn = z + 1 == Z ? 0 : z + 1, zp = z == 0 ? Z - 1 : z - 1;
      *reinterpret_cast<V*>(out + (3ll * z + 1) * plane + px) = v;
      *reinterpret_cast<V*>(out + (3ll * zn + 0) * plane + px) = v;
      *reinterpret_cast<V*>(out + (3ll * zp + 2) * plane + px) = v;
    }
  }
  __device__ __forceinline__ int store(int z, int r, int c, uint32_t w) const {
    put(z, r, c, __builtin_bit_cast(float, w));
    return 0;
  }
  __device__ __forceinline__ int move4(int z, int r, int c) const {
    T v[4];
    load4(src, z, r, c, v);
    put(z, r, c, make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]));
    return 0;
  }
  __device__ __forceinline__ void finish(int) const {}
};

constexpr uint32_t kStray = 0xffffffffu;

// labels: the remap, then uint8 labels [Z][R][C] (and the one-hot [Z][K][R][C]) with the count of values that are no class; or,
// raw, the value cast to int32 as it is
struct LabelArgs {
  uint8_t* lab;                     // !raw
  uint8_t* onehot;                  // !raw, may be null
  int* rawout;                      // raw
  unsigned long long* counter;      // !raw
  int K, raw, nremap;
  int from[kMaxRemap], to[kMaxRemap];
};
template <typename T>
struct LabelOp {
  View<const T> src;
  LabelArgs a;
  int Z, R, C;
  __device__ __forceinline__ uint32_t code(T v) const {
    if (a.raw) return (uint32_t)(int)v;
    if constexpr (std::is_floating_point<T>::value) {
      double d = (double)v;
      for (int k = 0; k < a.nremap; ++k)
        if (d == (double)a.from[k]) d = (double)a.to[k];
      const bool ok = d >= 0.0 && d < (double)a.K && d == floor(d);              // NaN fails every comparison
      return ok ? (uint32_t)(int)d : kStray;
    } else {
      int d = (int)v;
      for (int k = 0; k < a.nremap; ++k)
        if (d == a.from[k]) d = a.to[k];
      return d >= 0 && d < a.K ? (uint32_t)d : kStray;
    }
  }
  __device__ __forceinline__ uint32_t load(int z, int r, int c) const { return code(load1(src, z, r, c)); }
  // -> the number of values that are no class (written as background, with an all-zero one-hot pixel)
  __device__ __forceinline__ int store(int z, int r, int c, uint32_t w) const {
    const long long plane = (long long)R * C, px = (long long)r * C + c;
    if (a.raw) {
      a.rawout[z * plane + px] = (int)w;
      return 0;
    }
    const bool bad = w == kStray;
    a.lab[z * plane + px] = bad ? (uint8_t)0 : (uint8_t)w;
    if (a.onehot)
      for (int k = 0; k < a.K; ++k) a.onehot[((long long)z * a.K + k) * plane + px] = (uint8_t)(w == (uint32_t)k);
    return bad ? 1 : 0;
  }
  __device__ __forceinline__ int move4(int z, int r, int c) const {
    T v[4];
    load4(src, z, r, c, v);
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = code(v[j]);
    const long long plane = (long long)R * C, px = (long long)r * C + c;
    if (a.raw) {
      *reinterpret_cast<int4*>(a.rawout + z * plane + px) = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
      return 0;
    }
    uint32_t word = 0;
    int stray = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool bad = w[j] == kStray;
      stray += bad ? 1 : 0;
      word |= (bad ? 0u : w[j]) << (8 * j);
    }
    *reinterpret_cast<uint32_t*>(a.lab + z * plane + px) = word;
    if (a.onehot)
      for (int k = 0; k < a.K; ++k) {
        uint32_t hot = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) hot |= (uint32_t)(w[j] == (uint32_t)k) << (8 * j);
        *reinterpret_cast<uint32_t*>(a.onehot + ((long long)z * a.K + k) * plane + px) = hot;
      }
    return stray;
  }
  __device__ __forceinline__ void finish(int stray) const {
    if (a.raw) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) stray += __shfl_xor(stray, o, 64);
    if ((threadIdx.x & 63) == 0 && stray) atomicAdd(a.counter, (unsigned long long)stray);   // an integer atomic: the same count every run
  }
};

// restore: uint8 [Z][R][C] -> the caller's strided array (uint8 or int16), through the optional 256-entry table
template <typename TO>
struct RestoreOp {
  View<const uint8_t> src;          // the contiguous prediction: sz = R C, sr = C, sc = 1
  View<TO> dst;
  const int16_t* lut;               // device, may be null
  int Z, R, C;
  __device__ __forceinline__ TO map(uint32_t w) const {
    if (!lut) return (TO)w;
    const int16_t* q = lut + w;
    const int16_t v = *q;
    PCUDA_KEEP(q);
    return (TO)v;
  }
  __device__ __forceinline__ uint32_t load(int z, int r, int c) const { return load1(src, z, r, c); }
  __device__ __forceinline__ int store(int z, int r, int c, uint32_t w) const {
    dst.p[dst.at(z, r, c)] = map(w);
    return 0;
  }
  __device__ __forceinline__ int move4(int z, int r, int c) const {
    uint8_t v[4];
    load4(src, z, r, c, v);
    const TO o[4] = {map(v[0]), map(v[1]), map(v[2]), map(v[3])};
    store4(dst, z, r, c, o);
    return 0;
  }
  __device__ __forceinline__ void finish(int) const {}
};

// ------------------------------------------------------------------------------------------ the three kernel forms
template <class Op>
__global__ __launch_bounds__(kThreads) void row_kernel(Op op) {
  const long long plane = (long long)op.R * op.C;
  int count = 0;
  for (int z = blockIdx.y; z < op.Z; z += gridDim.y)
    for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < plane; p += (long long)gridDim.x * kThreads) {
      int r, c;
      split(p, op.C, r, c);
      count += op.store(z, r, c, op.load(z, r, c));
    }
  op.finish(count);
}

template <class Op>
__global__ __launch_bounds__(kThreads) void row4_kernel(Op op) {      // C is a multiple of four
  const int c4 = op.C >> 2;
  const long long groups = (long long)op.R * c4;
  int count = 0;
  for (int z = blockIdx.y; z < op.Z; z += gridDim.y)
    for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < groups; p += (long long)gridDim.x * kThreads) {
      int r, g;
      split(p, c4, r, g);
      count += op.move4(z, r, 4 * g);
    }
  op.finish(count);
}

// f: the caller's unit-stride axis (z if f_is_z, else r), g: the other one.  CALLER_FIRST: the caller's array is the source
// (lanes along f while loading, along c while storing); else it is the destination (restore).
template <class Op, bool CALLER_FIRST>
__global__ __launch_bounds__(kThreads) void tile_kernel(Op op, int f_is_z) {
  __shared__ uint32_t tile[kTile][kTile + 1];                          // [c][f]
  const int F = f_is_z ? op.Z : op.R, G = f_is_z ? op.R : op.Z, C = op.C;
  const int tf = (F + kTile - 1) / kTile, tc = (C + kTile - 1) / kTile;
  const long long ntiles = (long long)tf * tc;
  const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x >> 6;     // 64 lanes along the fast axis, four rows at a time
  int count = 0;
  for (int g = blockIdx.y; g < G; g += gridDim.y)
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
      const long long tcol = t / tf;
      const int f0 = (int)(t - tcol * tf) * kTile, c0 = (int)tcol * kTile;
      // lanes along f
      const int f = f0 + tx;
      const int zf = f_is_z ? f : g, rf = f_is_z ? g : f;
      // lanes along c
      const int c = c0 + tx;
      if (CALLER_FIRST) {
        if (f < F)
          for (int j = ty; j < kTile && c0 + j < C; j += kThreads / kTile) tile[j][tx] = op.load(zf, rf, c0 + j);
      } else {
        if (c < C)
          for (int j = ty; j < kTile && f0 + j < F; j += kThreads / kTile)
            tile[tx][j] = op.load(f_is_z ? f0 + j : g, f_is_z ? g : f0 + j, c);
      }
      __syncthreads();
      if (CALLER_FIRST) {
        if (c < C)
          for (int j = ty; j < kTile && f0 + j < F; j += kThreads / kTile)
            count += op.store(f_is_z ? f0 + j : g, f_is_z ? g : f0 + j, c, tile[tx][j]);
      } else {
        if (f < F)
          for (int j = ty; j < kTile && c0 + j < C; j += kThreads / kTile) count += op.store(zf, rf, c0 + j, tile[j][tx]);
      }
      __syncthreads();
    }
  op.finish(count);
}

// ------------------------------------------------------------------------------------------ host side
struct Map {
  long long base, sz, sr, sc;      // as the caller gave them
  int Z, R, C, flip_r, flip_c;
};

int check_map(const char* who, const Map& m) {
  if (m.Z < 0 || m.R < 0 || m.C < 0) PCUDA_FAIL(PCUDA_E_BADARG, "%s: negative size (%d, %d, %d)", who, m.Z, m.R, m.C);
  if (m.base < 0) PCUDA_FAIL(PCUDA_E_BADARG, "%s: negative base offset", who);
  if (m.Z == 0 || m.R == 0 || m.C == 0) return PCUDA_OK;              // nothing is addressed
  if ((m.Z > 1 && m.sz <= 0) || (m.R > 1 && m.sr <= 0) || (m.C > 1 && m.sc <= 0))
    PCUDA_FAIL(PCUDA_E_BADARG, "%s: a positive stride on every axis longer than 1 (got %lld, %lld, %lld)", who, m.sz, m.sr, m.sc);
  return PCUDA_OK;
}
inline bool empty(const Map& m) { return m.Z == 0 || m.R == 0 || m.C == 0; }

// flips folded in; an axis of length 1 gets stride 0 (it is never stepped along)
template <typename T>
View<T> make_view(T* p, const Map& m) {
  View<T> v;
  const long long sz = m.Z > 1 ? m.sz : 0, sr = m.R > 1 ? m.sr : 0, sc = m.C > 1 ? m.sc : 0;
  v.p = p + m.base + (m.flip_r ? (m.R - 1) * sr : 0) + (m.flip_c ? (m.C - 1) * sc : 0);
  v.sz = sz;
  v.sr = m.flip_r ? -sr : sr;
  v.sc = m.flip_c ? -sc : sc;
  return v;
}

enum Form { kRow, kRow4, kTileR, kTileZ };

inline long long mag(long long v) { return v < 0 ? -v : v; }
// four neighbouring columns of the caller's array as one aligned group of `es`-byte elements?
template <typename T>
bool groups_aligned(const View<T>& v, int C) {
  const size_t es = sizeof(T), a = es * 4 > 16 ? 16 : es * 4;
  if (C % 4 != 0 || mag(v.sc) != 1) return false;
  const uintptr_t first = (uintptr_t)(v.p - (v.sc < 0 ? 3 : 0));
  return first % a == 0 && (size_t)(mag(v.sz) * (long long)es) % a == 0 && (size_t)(mag(v.sr) * (long long)es) % a == 0;
}
template <typename T>
Form pick_form(const View<T>& v, const Map& m, bool other_side_aligned) {
  if (mag(v.sc) == 1 || m.C == 1) return groups_aligned(v, m.C) && other_side_aligned ? kRow4 : kRow;
  if (mag(v.sr) == 1) return kTileR;
  if (mag(v.sz) == 1) return kTileZ;
  return kRow;
}

template <class Op, bool CALLER_FIRST>
int launch(const char* who, Op op, Form form, hipStream_t s) {
  const dim3 block(kThreads);
  if (form == kRow || form == kRow4) {
    const long long items = (long long)op.R * (form == kRow4 ? op.C / 4 : op.C);
    long long gx = (items + kThreads - 1) / kThreads;
    gx = gx > kMaxGridX ? kMaxGridX : gx;
    const dim3 grid((unsigned)gx, (unsigned)(op.Z > kMaxGridY ? kMaxGridY : op.Z));
    if (form == kRow4) hipLaunchKernelGGL((row4_kernel<Op>), grid, block, 0, s, op);
    else hipLaunchKernelGGL((row_kernel<Op>), grid, block, 0, s, op);
  } else {
    const int f_is_z = form == kTileZ;
    const int F = f_is_z ? op.Z : op.R, G = f_is_z ? op.R : op.Z;
    long long gx = (long long)((F + kTile - 1) / kTile) * ((op.C + kTile - 1) / kTile);
    gx = gx > kMaxGridX ? kMaxGridX : gx;
    const dim3 grid((unsigned)gx, (unsigned)(G > kMaxGridY ? kMaxGridY : G));
    hipLaunchKernelGGL((tile_kernel<Op, CALLER_FIRST>), grid, block, 0, s, op, f_is_z);
  }
  PCUDA_CHECK_LAUNCH(who);
  return PCUDA_OK;
}

inline size_t vol_elem_size(int dt) {
  return dt == PCUDA_VOL_F64 ? 8 : (dt == PCUDA_VOL_F32 || dt == PCUDA_VOL_I32) ? 4 : dt == PCUDA_VOL_I16 ? 2 : dt == PCUDA_VOL_U8 ? 1 : 0;
}

template <typename T>
int run_slices(const void* in, const Map& m, int window, float* out, hipStream_t s) {
  SliceOp<T> op;
  op.src = make_view(static_cast<const T*>(in), m);
  op.out = out; op.Z = m.Z; op.R = m.R; op.C = m.C; op.window = window;
  const bool out_ok = m.C % 4 == 0 && ((uintptr_t)out & 15) == 0;
  return launch<SliceOp<T>, true>("volume_slices", op, pick_form(op.src, m, out_ok), s);
}

template <typename T>
int run_labels(const void* in, const Map& m, const LabelArgs& a, hipStream_t s) {
  LabelOp<T> op;
  op.src = make_view(static_cast<const T*>(in), m);
  op.a = a; op.Z = m.Z; op.R = m.R; op.C = m.C;
  const bool out_ok = m.C % 4 == 0 && (a.raw ? ((uintptr_t)a.rawout & 15) == 0
                                             : ((uintptr_t)a.lab & 3) == 0 && ((uintptr_t)a.onehot & 3) == 0);
  return launch<LabelOp<T>, true>("volume_labels", op, pick_form(op.src, m, out_ok), s);
}

template <typename TO>
int run_restore(const uint8_t* in, const Map& m, void* out, const int16_t* lut, hipStream_t s) {
  RestoreOp<TO> op;
  Map cm = m;                       // the contiguous prediction
  cm.base = 0; cm.sz = (long long)m.R * m.C; cm.sr = m.C; cm.sc = 1; cm.flip_r = cm.flip_c = 0;
  op.src = make_view(in, cm);
  op.dst = make_view(static_cast<TO*>(out), m);
  op.lut = lut; op.Z = m.Z; op.R = m.R; op.C = m.C;
  const bool in_ok = m.C % 4 == 0 && ((uintptr_t)in & 3) == 0;
  return launch<RestoreOp<TO>, false>("volume_restore", op, pick_form(op.dst, m, in_ok), s);
}

}  // namespace

extern "C" int pcuda_volume_slices(const void* in, int dtype, long long base, long long sz, long long sr, long long sc, int z,
                                   int r, int c, int flip_r, int flip_c, int window, float* out, pcuda_stream_t s) {
  if (dtype != PCUDA_VOL_F32 && dtype != PCUDA_VOL_F64 && dtype != PCUDA_VOL_I16 && dtype != PCUDA_VOL_U8)
    PCUDA_FAIL(PCUDA_E_BADARG, "volume_slices: dtype is fp32, float64, int16 or uint8");
  if (window != 1 && window != 3) PCUDA_FAIL(PCUDA_E_BADARG, "volume_slices: window is 1 or 3, got %d", window);
  const Map m{base, sz, sr, sc, z, r, c, flip_r != 0, flip_c != 0};
  const int rc = check_map("volume_slices", m);
  if (rc != PCUDA_OK) return rc;
  if (empty(m)) return PCUDA_OK;
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "volume_slices: null pointer");
  if (in == (const void*)out) PCUDA_FAIL(PCUDA_E_BADARG, "volume_slices: in == out (the input is never written)");
  hipStream_t st = (hipStream_t)s;
  const double n = (double)z * r * c;
  ProfScope prof(PCUDA_FAM_POINTWISE, n * ((double)vol_elem_size(dtype) + 4.0 * window), st);
  if (dtype == PCUDA_VOL_F32) return run_slices<float>(in, m, window, out, st);
  if (dtype == PCUDA_VOL_F64) return run_slices<double>(in, m, window, out, st);
  if (dtype == PCUDA_VOL_I16) return run_slices<int16_t>(in, m, window, out, st);
  return run_slices<uint8_t>(in, m, window, out, st);
}

extern "C" size_t pcuda_volume_labels_workspace_size(void) { return 16; }      // the counter of values that are no class

extern "C" int pcuda_volume_labels(const void* in, int dtype, long long base, long long sz, long long sr, long long sc, int z,
                                   int r, int c, int flip_r, int flip_c, int num_classes, const int* remap, int num_remap, int raw,
                                   void* labels, uint8_t* onehot, void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  if (vol_elem_size(dtype) == 0) PCUDA_FAIL(PCUDA_E_BADARG, "volume_labels: dtype is uint8, int16, int32, fp32 or float64");
  if (!raw) {
    if (num_classes < 2 || num_classes > 255) PCUDA_FAIL(PCUDA_E_BADARG, "volume_labels: 2..255 classes, got %d", num_classes);
    if (num_remap < 0 || num_remap > kMaxRemap || (num_remap > 0 && !remap))
      PCUDA_FAIL(PCUDA_E_BADARG, "volume_labels: a remap table of at most 8 (from, to) pairs");
  }
  const Map m{base, sz, sr, sc, z, r, c, flip_r != 0, flip_c != 0};
  const int rc = check_map("volume_labels", m);
  if (rc != PCUDA_OK) return rc;
  if (!raw && (!workspace || workspace_bytes < 16 || ((uintptr_t)workspace & 7) != 0))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "volume_labels: workspace too small (or not 8-byte aligned)");
  hipStream_t st = (hipStream_t)s;
  if (empty(m)) return PCUDA_OK;                                        // (the workspace is left as it is)
  if (!in || !labels) PCUDA_FAIL(PCUDA_E_BADARG, "volume_labels: null pointer");
  if (in == (const void*)labels || (onehot && in == (const void*)onehot))
    PCUDA_FAIL(PCUDA_E_BADARG, "volume_labels: in == out (the input is never written)");
  if (raw && onehot) PCUDA_FAIL(PCUDA_E_BADARG, "volume_labels: raw output has no one-hot form");
  if (!raw && hipMemsetAsync(workspace, 0, 16, st) != hipSuccess) PCUDA_FAIL(PCUDA_E_LAUNCH, "volume_labels: hipMemsetAsync failed");
  LabelArgs a;
  memset(&a, 0, sizeof(a));
  a.lab = raw ? nullptr : static_cast<uint8_t*>(labels);
  a.rawout = raw ? static_cast<int*>(labels) : nullptr;
  a.onehot = onehot;
  a.counter = static_cast<unsigned long long*>(workspace);
  a.K = num_classes; a.raw = raw != 0; a.nremap = raw ? 0 : num_remap;
  for (int k = 0; k < a.nremap; ++k) {
    a.from[k] = remap[2 * k];
    a.to[k] = remap[2 * k + 1];
  }
  const double n = (double)z * r * c;
  ProfScope prof(PCUDA_FAM_POINTWISE, n * ((double)vol_elem_size(dtype) + (raw ? 4.0 : 1.0 + (onehot ? num_classes : 0))), st);
  if (dtype == PCUDA_VOL_U8) return run_labels<uint8_t>(in, m, a, st);
  if (dtype == PCUDA_VOL_I16) return run_labels<int16_t>(in, m, a, st);
  if (dtype == PCUDA_VOL_I32) return run_labels<int32_t>(in, m, a, st);
  if (dtype == PCUDA_VOL_F32) return run_labels<float>(in, m, a, st);
  return run_labels<double>(in, m, a, st);
}

extern "C" int pcuda_volume_restore(const uint8_t* in, int z, int r, int c, void* out, int out_dtype, long long base, long long sz,
                                    long long sr, long long sc, int flip_r, int flip_c, const int16_t* lut, pcuda_stream_t s) {
  if (out_dtype != PCUDA_VOL_U8 && out_dtype != PCUDA_VOL_I16) PCUDA_FAIL(PCUDA_E_BADARG, "volume_restore: the output is uint8 or int16");
  const Map m{base, sz, sr, sc, z, r, c, flip_r != 0, flip_c != 0};
  const int rc = check_map("volume_restore", m);
  if (rc != PCUDA_OK) return rc;
  if (empty(m)) return PCUDA_OK;
  if (!in || !out) PCUDA_FAIL(PCUDA_E_BADARG, "volume_restore: null pointer");
  if ((const void*)in == out) PCUDA_FAIL(PCUDA_E_BADARG, "volume_restore: in == out (the input is never written)");
  if (lut && ((uintptr_t)lut & 1) != 0) PCUDA_FAIL(PCUDA_E_BADARG, "volume_restore: the table is 256 int16 values (2-byte aligned)");
  hipStream_t st = (hipStream_t)s;
  const double n = (double)z * r * c;
  ProfScope prof(PCUDA_FAM_POINTWISE, n * (1.0 + (double)vol_elem_size(out_dtype)), st);
  if (out_dtype == PCUDA_VOL_U8) return run_restore<uint8_t>(in, m, out, lut, st);
  return run_restore<int16_t>(in, m, out, lut, st);
}
