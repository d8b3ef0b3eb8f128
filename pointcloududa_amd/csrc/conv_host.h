// Host-side geometry helpers shared by conv_igemm.hip and conv_wgrad.hip.
#pragma once
#include <stdlib.h>
#include <string.h>
#include "conv_igemm.h"

static const int LDS_HARD = 160 * 1024;

static inline bool geom_ok(const pcuda_conv_geom* g) {
  if (!g || g->n <= 0 || g->cin <= 0 || g->cout <= 0 || g->k <= 0 || g->stride <= 0 || g->dil <= 0 || g->pad < 0)
    return false;
  if (g->k * g->k > IG_MAX_TAPS) return false;
  const int oh = (g->in_h + 2 * g->pad - g->dil * (g->k - 1) - 1) / g->stride + 1;
  const int ow = (g->in_w + 2 * g->pad - g->dil * (g->k - 1) - 1) / g->stride + 1;
  if (oh != g->out_h || ow != g->out_w || oh <= 0 || ow <= 0) return false;
  if (g->in_up && ((g->in_h & 1) || (g->in_w & 1))) return false;
  return true;
}

static inline bool src_ok(const pcuda_src* s, int c) {
  if (!s || !s->p1 || s->c1 <= 0 || s->c1 > c) return false;
  if (s->c1 < c && !s->p2) return false;
  return true;
}
static inline bool dst_ok(const pcuda_dst* d, int c) {
  if (!d || !d->p1 || d->c1 <= 0 || d->c1 > c) return false;
  if (d->c1 < c && !d->p2) return false;
  return true;
}

struct TapSet {
  int n;
  signed char dy[IG_MAX_TAPS], dx[IG_MAX_TAPS], src[IG_MAX_TAPS];
  int dy_min, dy_max, dx_min, dx_max;
  void finish() {
    dy_min = dx_min = 127; dy_max = dx_max = -127;
    for (int i = 0; i < n; ++i) {
      if (dy[i] < dy_min) dy_min = dy[i];
      if (dy[i] > dy_max) dy_max = dy[i];
      if (dx[i] < dx_min) dx_min = dx[i];
      if (dx[i] > dx_max) dx_max = dx[i];
    }
    if (n == 0) dy_min = dy_max = dx_min = dx_max = 0;
  }
};

// (zero-initialised: src travels whole into kernel arguments and the device-resident job table, conv_igemm.hip fill_pack)
static inline TapSet fwd_taps(const pcuda_conv_geom* g) {
  TapSet t = {};
  for (int ky = 0; ky < g->k; ++ky)
    for (int kx = 0; kx < g->k; ++kx) {
      t.dy[t.n] = (signed char)(ky * g->dil - g->pad);
      t.dx[t.n] = (signed char)(kx * g->dil - g->pad);
      t.src[t.n] = (signed char)(ky * g->k + kx);
      ++t.n;
    }
  t.finish();
  return t;
}

static inline int posmod(int a, int m) { return ((a % m) + m) % m; }

// taps of the dgrad parity class (ry, rx): dX[s*m + ry] = sum_ky dY[m + (ry + pad - ky*dil)/s] w[ky]
static inline TapSet dgrad_taps(const pcuda_conv_geom* g, int ry, int rx) {
  TapSet t = {};
  const int s = g->stride;
  for (int ky = 0; ky < g->k; ++ky) {
    const int vy = ry + g->pad - ky * g->dil;
    if (posmod(vy, s) != 0) continue;
    for (int kx = 0; kx < g->k; ++kx) {
      const int vx = rx + g->pad - kx * g->dil;
      if (posmod(vx, s) != 0) continue;
      t.dy[t.n] = (signed char)(vy / s);
      t.dx[t.n] = (signed char)(vx / s);
      t.src[t.n] = (signed char)(ky * g->k + kx);
      ++t.n;
    }
  }
  t.finish();
  return t;
}

// Stride-2 layers whose two COLUMN parity classes reach the same gradient pixels (k = 4, pad = 2, the discriminators'
// layers, GAN.py:97-105: both classes have the tap offsets {0,1} x {0,1}): the two classes run as ONE launch with rows
// (channel, column parity), so that a wave writes both halves of every 8 bytes of a destination line (a class on its own
// stores every other dword: the lines reach HBM half-written twice, WRITE_SIZE 2x the tensor) and the gradient tile is
// staged twice per layer instead of four times.  A property of (k, stride, pad, dil, cin) only: the packed image of a
// layer and its launches agree.  (cin <= 5 stays on the four-class image: the direct kernels of the first layer read it.)
static inline bool dgrad_pair_enabled() {
  static int on = -1;
  if (on < 0) { const char* e = getenv("PCUDA_DGRAD_PAIR"); on = (e && !atoi(e)) ? 0 : 1; }
  return on != 0;
}
static inline bool dgrad_pair_ok(const pcuda_conv_geom* g) {
  if (g->stride != 2 || g->in_up || g->cin <= 5 || !dgrad_pair_enabled()) return false;
  for (int ry = 0; ry < 2; ++ry) {
    const TapSet a = dgrad_taps(g, ry, 0), b = dgrad_taps(g, ry, 1);
    if (a.n < 1 || a.n != b.n || 2 * a.n > IG_MAX_TAPS) return false;
    for (int i = 0; i < a.n; ++i)
      if (a.dy[i] != b.dy[i] || a.dx[i] != b.dx[i]) return false;
  }
  return true;
}
// taps of row class ry for both column classes: offsets once, src[0..n) for rx = 0 and src[n..2n) for rx = 1
static inline TapSet dgrad_pair_taps(const pcuda_conv_geom* g, int ry) {
  TapSet t = dgrad_taps(g, ry, 0);
  const TapSet b = dgrad_taps(g, ry, 1);
  for (int i = 0; i < b.n; ++i) t.src[t.n + i] = b.src[i];
  return t;
}

// candidate output-tile widths: powers of two plus even splits of the row (so a 17- or 33-wide map is
// not padded to 32 / 64)
static inline int tile_width_candidates(int lw, int tile_px, int* out) {
  int n = 0;
  for (int t = 8; t <= 256 && t <= tile_px; t <<= 1) out[n++] = t;
  for (int parts = 1; parts <= 4; ++parts) {
    const int t = (lw + parts - 1) / parts;
    if (t >= 4 && t <= 256 && t <= tile_px) {
      bool dup = false;
      for (int i = 0; i < n; ++i) dup |= out[i] == t;
      if (!dup) out[n++] = t;
    }
  }
  return n;
}


// fast (buffer-load) staging preconditions of the software-pipelined kernels: a 32-channel chunk lies
// in ONE source and every source image spans < 2^30 bytes (32-bit offsets, out-of-bounds marker)
static inline bool fast_src_ok(const pcuda_src* x, int cin) {
  const long long lim = 1ll << 30;
  const int c1 = x->c1 < cin ? x->c1 : cin;
  if (c1 < cin && (c1 & 31)) return false;
  if ((long long)(c1 + 32) * x->sc1 * 4 >= lim) return false;
  if (c1 < cin && (long long)(cin - c1 + 32) * x->sc2 * 4 >= lim) return false;
  return true;
}

// 16-byte rows: the base pointer and both strides (in floats) of an [n][c][plane] view
static inline bool aligned16(const void* p, long long sn, long long sc) { return (((uintptr_t)p) & 15) == 0 && (sn & 3) == 0 && (sc & 3) == 0; }

// fast epilogue (buffer stores): an 8-row register group never straddles the two destinations and every
// destination image spans < 2^30 bytes
static inline bool fast_dst_ok(const pcuda_dst* y, int cout) {
  const long long lim = 1ll << 30;
  const int c1 = y->c1 < cout ? y->c1 : cout;
  if (c1 < cout && (c1 & 7)) return false;
  if ((long long)(c1 + 64) * y->sc1 * 4 >= lim) return false;
  if (c1 < cout && (long long)(cout - c1 + 64) * y->sc2 * 4 >= lim) return false;
  return true;
}

// tile / LDS plan of one forward or dgrad launch (conv_igemm.hip plans, conv_igemm_impl.h launches)
struct IgemmPlan {
  int npb, tw, th, tiles_x, tiles_y, ih_t, iw_t, clamp, x_cap, tg;
  size_t lds;
  int fat;   // one workgroup per CU, every (or many) taps of weights resident
  int w8;    // eight-wave kernel (one 512-thread workgroup per CU)
  int te;    // transposed epilogue (16-byte row stores through a wave-local LDS transposition)
};

// transposed epilogue preconditions: unit x stride, rows and tiles of 4k pixels, 16-byte aligned planes
static inline bool te_dst_ok(const pcuda_dst* y, int cout, int out_w, int lw, int tw, int ox_mul, int ox_off) {
  if (ox_mul != 1 || ox_off != 0 || (tw & 3) || (out_w & 3) || (lw & 3)) return false;
  if (((uintptr_t)y->p1 & 15) || (y->sc1 & 3) || (y->sn1 & 3)) return false;
  if (y->c1 < cout && (((uintptr_t)y->p2 & 15) || (y->sc2 & 3) || (y->sn2 & 3))) return false;
  return true;
}


// anti-phase 3x3 kernel (conv_ap.hip): layer property, packed image, launcher (returns 1 when it took the launch)
struct IgemmParams;
struct PackParams;
bool ap_layer_ok(const pcuda_conv_geom* g, int rows, int red, int prec);
size_t ap_layer_packed_bytes(int rows, int red);
bool ap_fill_pack(PackParams& p, const float* w, unsigned char* out, int rows, int red, long long s_row, long long s_red,
                  const TapSet& taps);
int ap_launch_pack(const float* w, unsigned char* out, int rows, int red, long long s_row, long long s_red, const TapSet& taps,
                   hipStream_t s);
bool ap_map_ok(int n, int h, int w, int rows);
int ap_tiles(int n, int h, int w);
int ap_try_launch(const IgemmParams& p, const TapSet& taps, const unsigned char* image, hipStream_t s, int* rc);

// row-streaming 3x3 kernel of the 32 -> 32-channel layers (conv_rs.hip): reads the ORDINARY packed layout
bool rs_layer_ok(const pcuda_conv_geom* g, int rows, int red, int prec);
bool rs_map_ok(int n, int h, int w);
int rs_tiles(int n, int h, int w);
int rs_try_launch(const IgemmParams& p, int prec, const TapSet& taps, hipStream_t s, int* rc);

// ------------------------------------------------------------------------------------------
// What lies where in a layer's packed weight buffers: THE place that knows (sizes, packers and launches all walk this).
// Forward buffer: the ordinary image, then the anti-phase image behind it.  Data-gradient buffer: the two paired row-class
// images, or one image per stride-parity class (ry-major) followed by the anti-phase image -- which only a stride-1 layer
// has, behind its single class.  A class without taps has no image.  Depends on the LAYER only (kernel, stride, padding,
// dilation, channels, precision): a packed buffer is valid for whatever map the layer later runs on.
// ------------------------------------------------------------------------------------------
static inline size_t packed_elems(int rows, int red, int ntaps, int prec) {   // bf16 elements of one ordinary / pair image
  const int co_tile = 32 * ig_co_blks(rows);
  const int n_co_tiles = cdiv(rows, co_tile), nchunks = cdiv(red, 32);
  return (size_t)n_co_tiles * nchunks * ntaps * co_tile * (ig_rec_bytes(prec == PCUDA_PREC_BF16X3) / 2);
}

enum { SIDE_FWD = 0, SIDE_DGRAD = 1 };
enum { IMG_ORDINARY = 0, IMG_PAIR = 1, IMG_AP = 2 };
struct PackedImage {
  int kind;
  int rows, red;            // rows and reduction channels of the launch that reads it (pair: 2 x cin rows)
  long long s_row, s_red;   // element strides of a row / a reduction index in the fp32 weights [cout][cin][k][k]
  int ry, rx;               // data gradient: the parity class (pair: the row class)
  size_t off, bytes;        // inside the side's buffer
  TapSet taps;              // (anti-phase image: the taps of the ordinary image in front of it)
};
struct PackedLayout {
  int n;
  size_t bytes;                          // of the whole buffer
  PackedImage img[IG_MAX_TAPS + 1];      // every class with an image owns a tap, + the anti-phase image
  const PackedImage* ap() const { return n > 0 && img[n - 1].kind == IMG_AP ? &img[n - 1] : nullptr; }
  const PackedImage* cls(int ry, int rx) const {       // the image of a parity class, or NULL (no taps)
    for (int i = 0; i < n; ++i)
      if (img[i].kind != IMG_AP && img[i].ry == ry && img[i].rx == rx) return &img[i];
    return nullptr;
  }
};
static inline void packed_layout(const pcuda_conv_geom* g, int prec, int side, PackedLayout* L) {
  const int kk = g->k * g->k;
  const bool fwd = side == SIDE_FWD;
  const int rows = fwd ? g->cout : g->cin, red = fwd ? g->cin : g->cout;
  const long long s_row = fwd ? (long long)g->cin * kk : kk, s_red = fwd ? kk : (long long)g->cin * kk;
  L->n = 0; L->bytes = 0;
  auto add = [&](int kind, int r, const TapSet& t, int ry, int rx) {
    PackedImage& im = L->img[L->n++];
    im.kind = kind; im.rows = r; im.red = red; im.s_row = s_row; im.s_red = s_red; im.ry = ry; im.rx = rx; im.taps = t;
    im.off = L->bytes;
    im.bytes = kind == IMG_AP ? ap_layer_packed_bytes(r, red) : packed_elems(r, red, t.n, prec) * 2;
    L->bytes += im.bytes;
  };
  if (fwd) {
    add(IMG_ORDINARY, rows, fwd_taps(g), 0, 0);
  } else if (dgrad_pair_ok(g)) {          // (no anti-phase image: stride 2)
    for (int ry = 0; ry < 2; ++ry) add(IMG_PAIR, 2 * rows, dgrad_pair_taps(g, ry), ry, 0);
    return;
  } else {
    for (int ry = 0; ry < g->stride; ++ry)
      for (int rx = 0; rx < g->stride; ++rx) {
        const TapSet t = dgrad_taps(g, ry, rx);
        if (t.n) add(IMG_ORDINARY, rows, t, ry, rx);
      }
  }
  if (ap_layer_ok(g, rows, red, prec)) add(IMG_AP, rows, L->img[0].taps, 0, 0);
}

// direct (vector-ALU) kernels of the degenerate layers (conv_direct.hip); each returns 1 when it took the launch
int direct_fwd_tiles(const pcuda_conv_geom* g);
int direct_forward(const pcuda_conv_geom* g, int prec, const pcuda_src* x, const void* packed_w, long long w_lo_off,
                   const float* bias, float slope, const pcuda_dst* y, float* bn_partials, hipStream_t s, int* rc);
int direct_dgrad_tiles(const pcuda_conv_geom* g);
int direct_dgrad(const pcuda_conv_geom* g, int prec, const pcuda_src* dy, const void* packed_w_dgrad, const pcuda_dst* dx,
                 int accumulate, hipStream_t s, int* rc, const float* red_a = nullptr, long long red_sn = 0,
                 long long red_sc = 0, const float* red_mean = nullptr, const float* red_invstd = nullptr,
                 float* red = nullptr);
int direct_d1_dgrad(const pcuda_conv_geom* g, int prec, const pcuda_src* dy, const void* packed_w_dgrad, const pcuda_dst* dx,
                    int accumulate, size_t cls_elems, hipStream_t s, int* rc);
int direct_d1_forward(const pcuda_conv_geom* g, int prec, const pcuda_src* x, const void* packed_w, const float* bias,
                      float slope, const pcuda_dst* y, float* bn_partials, hipStream_t s, int* rc);
int direct_d5_forward(const pcuda_conv_geom* g, int prec, const pcuda_src* x, const void* packed_w, const float* bias,
                      float slope, const pcuda_dst* y, float* bn_partials, hipStream_t s, int* rc);

// ------------------------------------------------------------------------------------------
// Weight gradient.  One call record goes to every route of the table in conv_wgrad.hip (WGRAD_ROUTES: THE place that knows
// the route order); a route returns WGRAD_NOT_TAKEN or the PCUDA_* result of the launch it made.  Split-K slabs of every
// route but direct d1: [slices][welems] partial weights, then [slices][cout] partial biases, + 256 bytes.
// ------------------------------------------------------------------------------------------
struct WgradCall {
  const pcuda_conv_geom* g;
  int prec;
  const pcuda_src* x;
  const float* dy;
  long long dy_sn, dy_sc;
  float* dw;
  float* db;                  // or NULL
  int accumulate;
  void* workspace;            // pcuda_conv2d_wgrad_workspace_size(g) bytes
  hipStream_t s;
  pcuda_reduce_job* defer;    // not NULL: the route fills it instead of launching the reduce (pcuda_conv2d_wgrad_partial)
};
enum { WGRAD_NOT_TAKEN = 1 };   // (every PCUDA_* code is <= 0)

struct WgradSlabs {
  float* partial;
  float* db_partial;          // NULL without a bias gradient
  long long welems;
  int slices, ntaps;          // ntaps > 1: the slabs are [slice][tap][cout * cin], the reduce transposes into OIHW
};
static inline size_t wgrad_slab_bytes(const pcuda_conv_geom* g, int slices) {
  return ((size_t)slices * g->cout * g->cin * g->k * g->k + (size_t)slices * g->cout) * sizeof(float) + 256;
}
WgradSlabs wgrad_slabs(const WgradCall& c, int slices, int ntaps);
// the tail of every route: fills *c.defer, or launches the reduce of the slabs into dw / db
int wgrad_finish(const WgradCall& c, const WgradSlabs& sl);
int launch_wgrad_reduce(const float* partial, long long numel, int ksplit, float* dw, int accumulate, int ntaps,
                        const float* db_partial, long long nb, float* db, hipStream_t s);

int direct_wgrad_slices(const pcuda_conv_geom* g);
int direct_wgrad(const WgradCall& c);
size_t direct_d1_wgrad_bytes(const pcuda_conv_geom* g);
int direct_d1_wgrad(const WgradCall& c);
int wgrad3r_slices(const pcuda_conv_geom* g);
int wgrad3r_wgrad(const WgradCall& c);
int wgrad3_slices(const pcuda_conv_geom* g);
int wgrad3_wgrad(const WgradCall& c);
int wgrad1_slices(const pcuda_conv_geom* g);
int wgrad1_wgrad(const WgradCall& c);
