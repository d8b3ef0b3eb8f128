// Weight-gradient kernels of the implicit-GEMM convolution (see conv_igemm.hip for the layout).
#include "conv_igemm.h"
#include "conv_host.h"

// dw[i] (+)= sum_k partial[k][i], deterministic.  A workgroup owns 64 consecutive outputs; its
// blockDim/64 k-groups each sum a strided subset of the slices (8 loads in flight per lane), and the
// k-group partials are combined in a fixed order through LDS.  (One thread per output with a serial
// loop over up to 1024 slices was latency-bound: 0.5 ms for a 9K-weight layer.)
// ntaps > 1: partial is [k][tap][co*cin] and dw is [co*cin][tap] (OIHW): coalesced reads, the
// transpose costs one scattered write per weight.
// The bias gradient rides in the same launch: workgroups past the weight slab's reduce db's [k][cout] slab.
// One kernel serves both forms: a layer's own reduce is a table of one job launched with 64 x nkg threads, a backward pass's
// reduces are a table of up to PCUDA_REDUCE_MAX_JOBS jobs launched with 1024 (a backward pass issues one per layer: 80
// launches of ~15 us per step, most of it launch and drain).  Jobs travel as kernel arguments; a workgroup finds its job in
// the prefix of 64-output blocks.  The number of k-groups is the JOB's own (nkg, k-groups past it add nothing), so that the
// sums of the two forms are bit-identical.
struct ReduceJobs {
  int n;
  int first_block[PCUDA_REDUCE_MAX_JOBS + 1];
  pcuda_reduce_job j[PCUDA_REDUCE_MAX_JOBS];
};

__global__ __launch_bounds__(1024) void wgrad_reduce_batch_kernel(const ReduceJobs jobs) {
  __shared__ float sh[16][64];
  int lo = 0, hi = jobs.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const pcuda_reduce_job& jb = jobs.j[lo];
  const float* partial = jb.partial;
  long long numel = jb.numel;
  float* dw = jb.dw;
  int ntaps = jb.ntaps;
  const int ksplit = jb.ksplit, nkg = jb.nkg;
  const int lane = threadIdx.x & 63, kg = threadIdx.x >> 6;
  const long long nblk_w = (numel + 63) / 64;
  long long blk = (int)blockIdx.x - jobs.first_block[lo];
  if (blk >= nblk_w) { blk -= nblk_w; partial = jb.db_partial; numel = jb.nb; dw = jb.db; ntaps = 1; }
  const long long i = blk * 64 + lane;
  float s = 0.f;
  if (i < numel && kg < nkg) {
    int k = kg;
    for (; k + 7 * nkg < ksplit; k += 8 * nkg) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partial[(long long)(k + u * nkg) * numel + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < ksplit; k += nkg) s += partial[(long long)k * numel + i];
  }
  sh[kg][lane] = s;
  __syncthreads();
  if (kg == 0 && i < numel) {
    float t = 0.f;
    for (int q = 0; q < nkg; ++q) t += sh[q][lane];
    long long o = i;
    if (ntaps > 1) {
      const long long cc = numel / ntaps;
      const long long tt = i / cc, r = i - tt * cc;
      o = r * ntaps + tt;
    }
    dw[o] = jb.accumulate ? dw[o] + t : t;
  }
}

static int reduce_blocks(const pcuda_reduce_job& jb) { return cdiv(jb.numel, 64) + (jb.db ? cdiv(jb.nb, 64) : 0); }

// (first_block[n] = the grid; threads = 64 x the largest nkg of the table)
static int launch_reduce_jobs(const ReduceJobs& jobs, int threads, hipStream_t s) {
  hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(jobs.first_block[jobs.n]), dim3(threads), 0, s, jobs);
  PCUDA_CHECK_LAUNCH("wgrad_reduce_batch_kernel");
  return PCUDA_OK;
}

// the job of one split-K reduce: partial = [ksplit][numel], db_partial = [ksplit][nb] or NULL.  THE place that chooses the
// number of k-groups (the summation order): the largest power of two <= min(ksplit, 16)
static pcuda_reduce_job reduce_job(const float* partial, long long numel, int ksplit, float* dw, int accumulate, int ntaps,
                                   const float* db_partial, long long nb, float* db) {
  pcuda_reduce_job jb;
  memset(&jb, 0, sizeof(jb));
  jb.partial = partial; jb.numel = numel; jb.ksplit = ksplit; jb.dw = dw; jb.accumulate = accumulate; jb.ntaps = ntaps;
  jb.db_partial = db_partial; jb.nb = db ? nb : 0; jb.db = db;
  jb.nkg = 1;
  while (jb.nkg < 16 && jb.nkg * 2 <= ksplit) jb.nkg <<= 1;
  return jb;
}

// a layer's own reduce: a table of one job, 64 x nkg threads
static int launch_reduce_job(const pcuda_reduce_job& jb, hipStream_t s) {
  ReduceJobs jobs;
  jobs.n = 1;
  jobs.j[0] = jb;
  jobs.first_block[0] = 0;
  jobs.first_block[1] = reduce_blocks(jb);
  return launch_reduce_jobs(jobs, 64 * jb.nkg, s);
}
// (for other translation units: conv1d_f32.hip)
int launch_wgrad_reduce(const float* partial, long long numel, int ksplit, float* dw, int accumulate, int ntaps,
                        const float* db_partial, long long nb, float* db, hipStream_t s) {
  return launch_reduce_job(reduce_job(partial, numel, ksplit, dw, accumulate, ntaps, db_partial, nb, db), s);
}

WgradSlabs wgrad_slabs(const WgradCall& c, int slices, int ntaps) {
  WgradSlabs sl;
  sl.welems = (long long)c.g->cout * c.g->cin * c.g->k * c.g->k;
  sl.partial = (float*)c.workspace;
  sl.db_partial = c.db ? sl.partial + (size_t)slices * sl.welems : nullptr;
  sl.slices = slices; sl.ntaps = ntaps;
  return sl;
}

int wgrad_finish(const WgradCall& c, const WgradSlabs& sl) {
  const pcuda_reduce_job jb = reduce_job(sl.partial, sl.welems, sl.slices, c.dw, c.accumulate, sl.ntaps, sl.db_partial, c.g->cout, c.db);
  if (!c.defer) return launch_reduce_job(jb, c.s);
  *c.defer = jb;      // the caller batches the reduce (pcuda_wgrad_reduce_batch); the workspace must live until then
  return PCUDA_OK;
}

extern "C" int pcuda_wgrad_reduce_batch(const pcuda_reduce_job* host_jobs, int njobs, pcuda_stream_t s) {
  if (!host_jobs || njobs < 0) PCUDA_FAIL(PCUDA_E_BADARG, "wgrad_reduce_batch: bad arguments");
  int done = 0;
  while (done < njobs) {
    ReduceJobs jobs;
    jobs.n = 0;
    int blocks = 0;
    for (; done < njobs && jobs.n < PCUDA_REDUCE_MAX_JOBS; ++done) {
      const pcuda_reduce_job& jb = host_jobs[done];
      if (jb.ksplit <= 0) continue;      // (the layer's own kernel already wrote dw)
      if (!jb.partial || !jb.dw || jb.numel <= 0 || jb.nkg < 1 || jb.nkg > 16 || (jb.db && !jb.db_partial))
        PCUDA_FAIL(PCUDA_E_BADARG, "wgrad_reduce_batch: bad job %d", done);
      jobs.first_block[jobs.n] = blocks;
      jobs.j[jobs.n++] = jb;
      blocks += reduce_blocks(jb);
    }
    if (jobs.n == 0) break;
    jobs.first_block[jobs.n] = blocks;
    ProfScope prof(PCUDA_FAM_POINTWISE, 0.0, (hipStream_t)s, "wgrad reduce batch");
    const int rc = launch_reduce_jobs(jobs, 1024, (hipStream_t)s);
    if (rc) return rc;
  }
  return PCUDA_OK;
}

namespace {

struct WgradPlan {
  int co_blks, co_tile, n_co_tiles, n_chunks, tap_groups, taps_per_group, tw, th, tiles_x, tiles_y, ksplit;
  int ih_t, iw_t;
};

// pixels of the input tile behind an ih x iw window: the whole halo, and the window clipped to the image (+ 1: the zero pixel)
struct TileSpan {
  long long halo, clipped;
};
TileSpan tile_span(const pcuda_conv_geom* g, long long ih, long long iw) {
  return {ih * iw, (ih < g->in_h ? ih : g->in_h) * (iw < g->in_w ? iw : g->in_w) + 1};
}
// LDS of a launch that stages x_pixels input records and the dZ rows of one co tile; mul = 2 in bf16x3 (hi + lo planes), 1 in bf16
size_t stage_lds(long long x_pixels, int co_tile, size_t mul) {
  return (size_t)x_pixels * IG_REC_BYTES * mul + (size_t)co_tile * WG_ZROW * mul;
}

// The staging footprint of a plan: the tile is clipped to the image where that halves it, or where the whole halo does not
// fit.  mul = 2 wherever the PLAN must not depend on the precision (the workspace query has no precision argument): the
// slab count and its one-per-CU test; the launch passes its own multiplier.
struct WgradStage {
  bool clamp;
  int x_cap;
  size_t lds;
};
WgradStage wgrad_stage(const WgradPlan& w, const pcuda_conv_geom* g, size_t mul) {
  const TileSpan t = tile_span(g, w.ih_t, w.iw_t);
  WgradStage st;
  st.clamp = t.clipped * 2 <= t.halo || stage_lds(t.halo, w.co_tile, mul) > (size_t)LDS_HARD;
  st.x_cap = (int)(st.clamp ? t.clipped : t.halo);
  st.lds = stage_lds(st.x_cap, w.co_tile, mul);
  return st;
}

WgradPlan plan_wgrad(const pcuda_conv_geom* g) {
  WgradPlan w;
  w.co_blks = ig_co_blks(g->cout);
  w.co_tile = 32 * w.co_blks;
  w.n_co_tiles = cdiv(g->cout, w.co_tile);
  w.n_chunks = cdiv(g->cin, 32);
  const int ntaps = g->k * g->k;
  w.tap_groups = ntaps <= 16 ? 1 : cdiv(ntaps, 9);   // 4x4 kernels keep all 16 taps in one block: X and dZ staged once
  w.taps_per_group = cdiv(ntaps, w.tap_groups);
  const int span = (g->k - 1) * g->dil;
  {   // 128-slot tile with the fewest tiles; ties prefer widths that keep the float4 dZ path (TW % 8 == 0)
    int cand[16];
    const int nc = tile_width_candidates(g->out_w, 128, cand);
    long long best_key = -1;
    w.tw = 32; w.th = 4;
    for (int ci = 0; ci < nc; ++ci) {
      const int tw = cand[ci], th = 128 / tw;
      if (th < 1) continue;
      // The candidates' own clipped-tile rule (not wgrad_stage's: no LDS clause).  Filter: the smaller of halo and clipped
      // tile + the dZ rows must fit LDS in bf16x3.  Rank: the tile counts as clipped where that halves it.
      const TileSpan t = tile_span(g, (th - 1) * g->stride + span + 1, (tw - 1) * g->stride + span + 1);
      const long long cap = t.halo < t.clipped ? t.halo : t.clipped;
      if (stage_lds(cap, w.co_tile, 2) > (size_t)LDS_HARD) continue;
      // (a staged tile of more than 768 pixels runs unpipelined -- no register prefetch, four waves: the 16-tap layers of the
      // 224x224 network's 57-wide maps took tw = 64 over tw = 57 for its aligned rows and ran at half the rate)
      const long long staged = (t.clipped * 2 <= t.halo) ? t.clipped : t.halo;
      const long long key = ((long long)cdiv(g->out_w, tw) * cdiv(g->out_h, th) << 24) + (staged > 768 ? (1ll << 22) : 0) +
                            ((tw & 31) ? (1ll << 20) : 0) + t.halo;
      if (best_key < 0 || key < best_key) { best_key = key; w.tw = tw; w.th = th; }
    }
  }
  const int TW = w.tw, TH = w.th;
  w.tiles_x = cdiv(g->out_w, TW);
  w.tiles_y = cdiv(g->out_h, TH);
  w.ih_t = (TH - 1) * g->stride + span + 1;
  w.iw_t = (TW - 1) * g->stride + span + 1;
  const long long ntiles = (long long)g->n * w.tiles_x * w.tiles_y;
  const int base = w.n_co_tiles * w.n_chunks * w.tap_groups;
  // blocks in flight: 32-row blocks (160 VGPRs, 50 KB of LDS) are resident three per CU, 64-row blocks two per CU --
  // 768 / 1024 blocks are one / two balanced rounds (1024 32-row blocks were one full round plus a third of one)
  static const int tgt32 = env_knob("PCUDA_WG_BLOCKS32", 768);
  static const int tgt64 = env_knob("PCUDA_WG_BLOCKS64", 1024);
  // plans whose LDS footprint leaves room for ONE workgroup per CU (the 16-tap stride-2 layers of the discriminators on the
  // eight-wave kernel, the dilated bottleneck layers): one round of 256 blocks -- two rounds only doubled their split-K slabs
  // (round 5, scripts/conv_micro.py: d2 / d3 / d4 0.220 / 0.219 / 0.278 -> 0.205 / 0.204 / 0.258 ms, 512->512 at 16x16 dilation 4
  // 0.253 -> 0.241; the two-per-CU plans lose 20-30 % at 256).  Sized on the bf16x3 footprint so that the slab count does
  // not depend on the precision.
  static const int tgt1 = env_knob("PCUDA_WG_BLOCKS1", 256);
  const bool one_per_cu = wgrad_stage(w, g, 2).lds > (size_t)LDS_HARD / 2;
  long long ks = (one_per_cu ? tgt1 : (w.co_blks == 1 ? tgt32 : tgt64)) / base;
  if (ks < 1) ks = 1;
  if (ks > ntiles) ks = ntiles;
  // keep the partial slabs (written once, re-read once by the reduce kernel) below ~64 MB (measured:
  // 32 MB costs the wgrad kernels more parallelism than the reduce kernel saves)
  const long long welems = (long long)g->cout * g->cin * ntaps;
  while (ks > 1 && ks * welems * 4 > (64ll << 20)) ks >>= 1;
  if (ks >= 8) ks &= ~7ll;      // multiples of 8: an XCD's slices interleave over its eighth of the tiles (wgrad_kernel)
  w.ksplit = (int)ks;
  return w;
}

// register prefetch depth of the launch (0: unpipelined; 100 + depth: the eight-wave kernel)
int wgrad_prefetch(const WgradCall& c, const WgradPlan& w, int x_cap) {
  // software-pipelined variants hold the next tile's loads in registers: input tiles <= 256*PF pixels
  static const bool nopipe = env_knob("PCUDA_NOPIPE", 0) != 0;
  int pf = (nopipe || !fast_src_ok(c.x, c.g->cin)) ? 0 : (x_cap <= 256 ? 1 : (x_cap <= 768 ? 3 : 0));
  // 16-tap groups (4x4 kernels): LDS leaves room for one workgroup per CU, so make it eight waves
  static const bool now8 = env_knob("PCUDA_WG_NO8", 0) != 0;
  if (!now8 && pf > 0 && w.taps_per_group > 9 && x_cap <= 1024) pf = 100 + (x_cap <= 512 ? 1 : 2);
  return pf;
}

WgradParams wgrad_params(const WgradCall& c, const WgradPlan& w, const TapSet& t, const WgradStage& st, int pf, const dim3& grid) {
  const pcuda_conv_geom* g = c.g;
  WgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = *c.x; p.cin = g->cin;
  p.in_h = g->in_h; p.in_w = g->in_w; p.in_shift = g->in_up ? 1 : 0; p.in_row = g->in_w >> p.in_shift;
  p.dz = c.dy; p.dz_sn = c.dy_sn; p.dz_sc = c.dy_sc;
  p.cout = g->cout; p.out_h = g->out_h; p.out_w = g->out_w;
  p.stride = g->stride;
  p.ntaps = w.taps_per_group; p.ntaps_total = t.n; p.tap_groups = w.tap_groups;
  memcpy(p.dy, t.dy, sizeof(p.dy));
  memcpy(p.dx, t.dx, sizeof(p.dx));
  p.dy_min = t.dy_min; p.dx_min = t.dx_min;
  p.ih_t = w.ih_t; p.iw_t = w.iw_t;
  p.tw = w.tw; p.th = w.th; p.tmagic = 65536 / w.tw + 1; p.tiles_x = w.tiles_x; p.tiles_y = w.tiles_y; p.n = g->n;
  p.ksplit = w.ksplit; p.n_co_tiles = w.n_co_tiles; p.n_chunks = w.n_chunks;
  p.partial = (float*)c.workspace;
  static const int dbg = env_knob("PCUDA_DBG", 0);
  p.dbg = dbg;
  p.tw16 = ((w.tw & 15) == 0 && w.tw * w.th == 128) ? 1 : 0;
  p.aligned4 = ((g->out_w & 7) == 0 && (w.tw & 7) == 0 && aligned16(c.dy, c.dy_sn, c.dy_sc) &&
                ((long long)g->cout * c.dy_sc + (long long)g->out_h * g->out_w) * 4 < (1ll << 30)) ? 1 : 0;
  static const bool noxcd = env_knob("PCUDA_WG_NOXCD", 0) != 0;
  static const bool nointer = env_knob("PCUDA_WG_NOINTER", 0) != 0;
  const long long nblk = (long long)grid.x * grid.y;
  p.xcd_items = (!noxcd && nblk >= 16 && (nblk & 7) == 0) ? (int)(nblk / 8) : 0;
  p.xcd_slices = (p.xcd_items && !nointer && (w.ksplit & 7) == 0) ? w.ksplit / 8 : 0;
  {   // quad staging where the (row, quad) items of a tile fit the staging slots of this variant
    static const bool noxq = env_knob("PCUDA_NOXQ", 0) != 0;
    const int slots = pf >= 100 ? pf - 100 : pf, per = pf >= 100 ? 128 : 64;
    const int ih = st.clamp ? (w.ih_t < g->in_h ? w.ih_t : g->in_h) : w.ih_t;
    const int in_w_phys = g->in_up ? g->in_w / 2 : g->in_w;
    p.xq = (!noxq && slots > 0 && !g->in_up && (in_w_phys & 3) == 0 && (ih * ((w.iw_t + 6) / 4) + per - 1) / per <= slots) ? 1 : 0;
  }
  return p;
}

}  // namespace

int wgrad_dispatch_x3(const WgradParams& p, int co_blks, bool clamp, int taps_max, int pf, int x_cap, size_t lds,
                      float* dbp, dim3 grid, hipStream_t s);
int wgrad_dispatch_bf16(const WgradParams& p, int co_blks, bool clamp, int taps_max, int pf, int x_cap, size_t lds,
                        float* dbp, dim3 grid, hipStream_t s);

// the generic plan: takes every layer
static int generic_slices(const pcuda_conv_geom* g) { return plan_wgrad(g).ksplit; }
static int generic_wgrad(const WgradCall& c) {
  const pcuda_conv_geom* g = c.g;
  const bool x3 = c.prec == PCUDA_PREC_BF16X3;
  const WgradPlan w = plan_wgrad(g);
  const TapSet t = fwd_taps(g);
  const WgradSlabs sl = wgrad_slabs(c, w.ksplit, t.n);
  const WgradStage st = wgrad_stage(w, g, x3 ? 2 : 1);
  if (st.lds > (size_t)LDS_HARD) PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "conv2d_wgrad: tile %dx%d does not fit LDS", w.ih_t, w.iw_t);
  const dim3 grid(w.n_co_tiles * w.n_chunks * w.tap_groups, w.ksplit);
  const int pf = wgrad_prefetch(c, w, st.x_cap);
  const WgradParams p = wgrad_params(c, w, t, st, pf, grid);
  {
    const double flops = 2.0 * g->n * (double)g->out_h * g->out_w * g->cout * (double)g->cin * t.n;
    char tag[160];
    snprintf(tag, sizeof(tag), "wgrad n%d cin%d cout%d %dx%d k%d s%d d%d ksplit%d clamp%d pf%d lds%zu", g->n, g->cin,
             g->cout, g->out_h, g->out_w, g->k, g->stride, g->dil, w.ksplit, st.clamp ? 1 : 0, pf, st.lds);
    ProfScope prof(PCUDA_FAM_CONV_WGRAD, flops, c.s, tag);
    const int taps_max = w.taps_per_group <= 1 ? 1 : w.taps_per_group <= 9 ? 9 : 16;
    const int rc = x3 ? wgrad_dispatch_x3(p, w.co_blks, st.clamp, taps_max, pf, st.x_cap, st.lds, sl.db_partial, grid, c.s)
                      : wgrad_dispatch_bf16(p, w.co_blks, st.clamp, taps_max, pf, st.x_cap, st.lds, sl.db_partial, grid, c.s);
    if (rc) return rc;
  }
  return wgrad_finish(c, sl);
}

// THE route order: the first route that takes a call runs it, and the workspace is the largest any route may ask for (a
// route's own eligibility also depends on the tensors, which the size query does not see).  slices: the route's slab count
// in the common layout (wgrad_slab_bytes), 0 where the geometry is not the route's; bytes: a layout of its own.
struct WgradRoute {
  const char* name;
  int (*slices)(const pcuda_conv_geom* g);
  size_t (*bytes)(const pcuda_conv_geom* g);
  int (*run)(const WgradCall& c);
};
static const WgradRoute WGRAD_ROUTES[] = {
    {"direct c1", direct_wgrad_slices, nullptr, direct_wgrad},          // 1 -> cout channels, 3x3 (conv_direct.hip)
    {"direct d1", nullptr, direct_d1_wgrad_bytes, direct_d1_wgrad},     // cin <= 4, 4x4 / stride 2, no bias (conv_direct_d1.hip)
    {"wgrad3r", wgrad3r_slices, nullptr, wgrad3r_wgrad},                // 3x3 layers without LDS staging (conv_wgrad3r.hip)
    {"wgrad3", wgrad3_slices, nullptr, wgrad3_wgrad},                   // aligned 3x3 / stride-1 layers (conv_wgrad3.hip)
    {"wgrad1", wgrad1_slices, nullptr, wgrad1_wgrad},                   // 1x1 / stride-1 layers on whole 16-pixel steps (conv_wgrad1.hip)
    {"generic", generic_slices, nullptr, generic_wgrad},
};

extern "C" size_t pcuda_conv2d_wgrad_workspace_size(const pcuda_conv_geom* g) {
  if (!geom_ok(g)) return 0;
  size_t need = 0;
  for (const WgradRoute& r : WGRAD_ROUTES) {
    size_t b = 0;
    if (r.bytes) b = r.bytes(g);
    else if (const int slices = r.slices(g)) b = wgrad_slab_bytes(g, slices);
    if (b > need) need = b;
  }
  return need;
}

static int wgrad_impl(const WgradCall& c, size_t workspace_bytes) {
  const pcuda_conv_geom* g = c.g;
  if (!geom_ok(g)) PCUDA_FAIL(PCUDA_E_BADARG, "conv2d_wgrad: inconsistent geometry");
  if (!src_ok(c.x, g->cin) || !c.dy || !c.dw) PCUDA_FAIL(PCUDA_E_BADARG, "conv2d_wgrad: bad tensors");
  if (c.prec != PCUDA_PREC_BF16X3 && c.prec != PCUDA_PREC_BF16) PCUDA_FAIL(PCUDA_E_BADARG, "conv2d_wgrad: bad precision");
  if (!c.workspace || workspace_bytes < pcuda_conv2d_wgrad_workspace_size(g))
    PCUDA_FAIL(PCUDA_E_WORKSPACE, "conv2d_wgrad: workspace too small (%zu < %zu)", workspace_bytes,
               pcuda_conv2d_wgrad_workspace_size(g));
  for (const WgradRoute& r : WGRAD_ROUTES) {
    const int rc = r.run(c);
    if (rc != WGRAD_NOT_TAKEN) return rc;
  }
  PCUDA_FAIL(PCUDA_E_UNSUPPORTED, "conv2d_wgrad: no route took the layer");      // (not reached: the generic plan takes every layer)
}

extern "C" int pcuda_conv2d_wgrad(const pcuda_conv_geom* g, int prec, const pcuda_src* x, const float* dy,
                                  long long dy_sn, long long dy_sc, float* dw, float* db, int accumulate,
                                  void* workspace, size_t workspace_bytes, pcuda_stream_t s) {
  return wgrad_impl({g, prec, x, dy, dy_sn, dy_sc, dw, db, accumulate, workspace, (hipStream_t)s, nullptr}, workspace_bytes);
}

extern "C" int pcuda_conv2d_wgrad_partial(const pcuda_conv_geom* g, int prec, const pcuda_src* x, const float* dy,
                                          long long dy_sn, long long dy_sc, float* dw, float* db, int accumulate,
                                          void* workspace, size_t workspace_bytes, pcuda_reduce_job* job, pcuda_stream_t s) {
  if (!job) PCUDA_FAIL(PCUDA_E_BADARG, "conv2d_wgrad_partial: job is NULL");
  memset(job, 0, sizeof(*job));
  return wgrad_impl({g, prec, x, dy, dy_sn, dy_sc, dw, db, accumulate, workspace, (hipStream_t)s, job}, workspace_bytes);
}
