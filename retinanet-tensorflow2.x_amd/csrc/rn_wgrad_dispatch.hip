// rn_wgrad_dispatch.hip — host-only: which kernel, split-K plan, grid and workspace a weight-gradient call gets.
//
// wgrad_plan() is the one place that policy lives.  It fills a WgradPlan from the descriptors of a call (one layer, or the n
// layers of rn_conv2d_nhwc_wgrad_group) and rn_num_cus(); the two launch functions set the workspace and output pointers and
// launch what the plan names, and the four queries read one field of it each — a query cannot disagree with the launch.
// The kernels and a launch function each stay with their files (rn_wgrad.hip, rn_wgrad_big.hip, rn_wgrad_halo.hip).
// Precedence, one layer: wgrad_halo_kernel, then wgrad_big_kernel, then the 128-tile wgrad_kernel.  A group: one
// wgrad_halo_kernel launch, then the layers as SEGMENTS of one merged problem on the per-tap kernels, then layer by layer.
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "rn_wgrad_dev.h"

enum WgradPath {      // HALO: wgrad_halo_kernel, one layer or a group of identical layers; BIG / T128: one layer on
  WG_PATH_HALO,       // wgrad_big_kernel / wgrad_kernel; SEGMENTS: a group as the segments of one merged problem on either
  WG_PATH_BIG, WG_PATH_128, WG_PATH_SEGMENTS,   // of those two (kid tells which); LAYERS: a group issued layer by layer,
  WG_PATH_LAYERS      // every layer with a plan of its own
};

struct WgradPlan {
  bool valid = false;  // every layer passed validation
  WgradPath path = WG_PATH_LAYERS;
  int kid = -1;        // partial-tile kernel: 0 wgrad_kernel, 1 wgrad_big_kernel, 2 wgrad_halo_kernel; -1: layer by layer
  int fused = 0;       // a group of two or more layers that runs as one launch
  int ngroups = 1;     // layers the launch covers
  WgArgs g;            // kid 0 / 1: the kernel's arguments but ws
  WhArgs h;            // kid 2
  bool linear;         // kid 0 / 1: the LINEAR instantiation
  unsigned grid;       // workgroups of the partial-tile kernel
  long long n4;        // ordered reduction: float4 columns of one layer's dw, partial tiles per layer, blocks per layer
  int chunks, red_blocks;
  size_t launch_bytes = 0;   // partial tiles the launch writes
  size_t ws_bytes = 0;       // the workspace queries' answer: the launch AND, for a group, every layer issued on its own fit
};

// ---- validation: what every kernel requires of a problem -------------------------------------------------------------
static bool wg_valid(const rn_wgrad_problem* p) {
  if (!p || p->num_segments < 1 || p->num_segments > RN_CONV_MAX_SEGMENTS) return false;
  if (p->R < 1 || p->S < 1 || p->stride_h < 1 || p->stride_w < 1) return false;
  if (rn_validate_launch_opts(p->opts, "rn_conv2d_nhwc_wgrad")) return false;
  const int Cin = p->seg[0].Cin, Cout = p->seg[0].Cout;
  if (Cin % 8 || Cout % 4 || Cin <= 0 || Cout <= 0) return false;
  for (int i = 0; i < p->num_segments; ++i) {
    const rn_wgrad_segment& s = p->seg[i];
    if (!s.x || !s.dy || s.Cin != Cin || s.Cout != Cout) return false;
    const long long P = (long long)s.N * s.Ho * s.Wo;
    if (P <= 0 || P >= (1ll << 24)) return false;
    const long long dyS = s.dy_pix_stride > 0 ? s.dy_pix_stride : s.Cout;
    if (dyS < s.Cout || (dyS % 4)) return false;
    const long long xS = s.x_pix_stride > 0 ? s.x_pix_stride : s.Cin;
    if (xS % 4) return false;
    if ((long long)s.N * s.H * s.W * xS * 2 >= (1ll << 31) || P * dyS * 2 >= (1ll << 31)) return false;
    if ((long long)s.N * s.H * s.W >= (1ll << 24) || xS >= (1 << 24) || dyS >= (1 << 24)) return false;   // 24-bit multiplies
  }
  return true;
}

// the one comparison of group geometry: filter, options and every segment's shape and strides (the tensors differ)
static bool wg_same_geometry(const rn_wgrad_problem& p, const rn_wgrad_problem& q) {
  if (q.R != p.R || q.S != p.S || q.stride_h != p.stride_h || q.stride_w != p.stride_w || q.pad_top != p.pad_top ||
      q.pad_left != p.pad_left || q.num_segments != p.num_segments || memcmp(&q.opts, &p.opts, sizeof(p.opts)) != 0)
    return false;
  for (int i = 0; i < p.num_segments; ++i) {
    const rn_wgrad_segment &s = p.seg[i], &t = q.seg[i];
    if (t.N != s.N || t.H != s.H || t.W != s.W || t.Cin != s.Cin || t.Ho != s.Ho || t.Wo != s.Wo || t.Cout != s.Cout ||
        t.dy_pix_stride != s.dy_pix_stride || t.x_pix_stride != s.x_pix_stride)
      return false;
  }
  return true;
}

static long long wg_pixels(const rn_wgrad_problem* p) {
  long long P = 0;
  for (int i = 0; i < p->num_segments; ++i) P += (long long)p->seg[i].N * p->seg[i].Ho * p->seg[i].Wo;
  return P;
}

// ---- wgrad_halo_kernel -----------------------------------------------------------------------------------------------
// Layers it serves: 3x3 / stride 1 / pad 1, same-size output, Cin a multiple of 64, Cout a multiple of 8 and at least 64.
// Auto-selected when the launch holds at least 16 384 output pixels (rn_launch_opts.wgrad_kernel = 2: whatever the pixel
// count; = 3: keep the per-tap wgrad_big_kernel for A/B timing).  ps[0..ngroups): layers of IDENTICAL geometry (the caller
// compared them): tiles = groups x co x ci, so the split-K plan needs 1/ngroups of the pixel chunks per layer — every
// workgroup writes its 288 KB accumulator once, 75 MB per launch however small the layer (measured: eight head-tower
// layers as one launch 2.12 ms against 8 x 0.346 ms, tools/bench_wgrad.py presets tower8 / tower).
static bool wg_halo_fill(const rn_wgrad_problem* const* ps, int ngroups, WhArgs& a) {
  const rn_wgrad_problem* p = ps[0];
  if (p->num_segments < 1 || p->num_segments > RN_CONV_MAX_SEGMENTS) return false;
  if (p->R != 3 || p->S != 3 || p->stride_h != 1 || p->stride_w != 1 || p->pad_top != 1 || p->pad_left != 1) return false;
  if (p->opts.wgrad_kernel == 1 || p->opts.wgrad_kernel == 3) return false;
  const int Cin = p->seg[0].Cin, Cout = p->seg[0].Cout;
  if (Cin % 64 != 0 || Cout % 8 != 0 || Cout < 64) return false;
  long long steps = 0;
  a.nseg = p->num_segments; a.ngroups = ngroups; a.pad_ = 0;
  for (int i = 0; i < p->num_segments; ++i) {
    const rn_wgrad_segment& s = p->seg[i];
    if (s.Ho != s.H || s.Wo != s.W) return false;
    WhSeg& d = a.seg[i];
    d.N = s.N; d.H = s.H; d.W = s.W;
    d.dyS = s.dy_pix_stride > 0 ? s.dy_pix_stride : s.Cout;
    d.xS = s.x_pix_stride > 0 ? s.x_pix_stride : s.Cin;
    d.ctiles = (int)rn_cdiv(s.W, WH_STRIP);
    // padded rows G = 1 .. N*(H+1) - 1 carry products; step t >= 1 of a strip covers WH_STEP_ROWS of them, step 0 is load-only
    d.L = (int)rn_cdiv((long long)s.N * (s.H + 1) - 1, WH_STEP_ROWS) + 1;
    d.step_begin = (int)steps;
    d.pad_ = 0;
    steps += (long long)d.ctiles * d.L;
    if ((long long)s.N * s.H * s.W * (d.xS > d.dyS ? d.xS : d.dyS) * 2 >= (1ll << 31) - (1ll << 24)) return false;
    for (int g = 0; g < ngroups; ++g) {      // the other layers: the same geometry, their own tensors
      const rn_wgrad_segment& t = ps[g]->seg[i];
      if (!t.x || !t.dy) return false;
      a.ptr[g][i].x = (const uint16_t*)t.x;
      a.ptr[g][i].dy = (const uint16_t*)t.dy;
    }
  }
  if (wg_pixels(p) < 16384 && p->opts.wgrad_kernel != 2) return false;
  if (steps >= (1ll << 30)) return false;
  a.Cin = Cin; a.Cout = Cout;
  a.co_tiles = (int)rn_cdiv(Cout, 128);
  a.ci_tiles = Cin / 64;
  a.total_steps = (int)steps;
  const int tiles = a.co_tiles * a.ci_tiles * ngroups;
  // one round of the CUs the kernel may use: fewest split-K partials; a chunk is at least 24 steps long — every chunk
  // writes a 288 KB partial tile — unless the caller asks for MORE workgroups than the chip has (the tests of the chunk
  // seams do: short chunks on purpose).  The two-stream engine's CU cap (wgrad_target_blocks = 176) keeps 24.
  long long blocks = p->opts.wgrad_target_blocks > 0 ? p->opts.wgrad_target_blocks : rn_num_cus() - p->opts.reserved_cus;
  const long long min_steps = p->opts.wgrad_target_blocks > rn_num_cus() ? 2 : 24;
  long long chunks = blocks / tiles;
  if (chunks < 1) chunks = 1;
  if (chunks > rn_cdiv(steps, min_steps)) chunks = rn_cdiv(steps, min_steps);
  a.CHs = (int)rn_cdiv(steps, chunks);
  a.total_chunks = (int)rn_cdiv(steps, a.CHs);
  return true;
}

// ---- the per-tap kernels ---------------------------------------------------------------------------------------------
// arguments of a validated problem with the 128 x 128 tiles and split-K chunks of wgrad_kernel
static void wg_fill_128(const rn_wgrad_problem* p, WgArgs& a) {
  a.R = p->R; a.S = p->S; a.sh = p->stride_h; a.sw = p->stride_w; a.pt = p->pad_top; a.pl = p->pad_left;
  a.nseg = p->num_segments; a.Cin = p->seg[0].Cin; a.Cout = p->seg[0].Cout;
  a.co_tiles = (int)rn_cdiv(a.Cout, 128); a.ci_tiles = (int)rn_cdiv(a.Cin, 128);
  const int tiles = a.co_tiles * a.ci_tiles * a.R * a.S;
  a.co_groups = (int)rn_cdiv(tiles, 64);
  if (a.co_groups > a.co_tiles) a.co_groups = a.co_tiles;
  a.gco = (int)rn_cdiv(a.co_tiles, a.co_groups);
  a.co_groups = (int)rn_cdiv(a.co_tiles, a.gco);
  // 512 = one round of two workgroups per CU: measured (tools/bench_wgrad.py, same process) 58 vs 75 us on the 128 <-> 512
  // 1x1 layers of ResNet stage 2 and 41 vs 55 us on 2048 -> 512 against the former 1024 — these layers are HBM-bound and
  // every extra pixel chunk is another |W| x 4 bytes of partial tile written and read back
  long long target = rn_cdiv(p->opts.wgrad_target_blocks > 0 ? p->opts.wgrad_target_blocks : 512, tiles);
  if (target < 1) target = 1;
  if (target > 256) target = 256;
  long long CH = rn_cdiv(rn_cdiv(wg_pixels(p), target), WG_BK) * WG_BK;
  if (CH < WG_BK) CH = WG_BK;
  a.CH = (int)CH;
  int chunks = 0;
  for (int i = 0; i < p->num_segments; ++i) {
    const rn_wgrad_segment& s = p->seg[i];
    WgSegDev& d = a.seg[i];
    d.x = (const uint16_t*)s.x; d.dy = (const uint16_t*)s.dy;
    d.N = s.N; d.H = s.H; d.W = s.W; d.Ho = s.Ho; d.Wo = s.Wo;
    d.P = s.N * s.Ho * s.Wo;
    d.chunk_begin = chunks;
    d.dyS = s.dy_pix_stride > 0 ? s.dy_pix_stride : s.Cout;
    d.xS = s.x_pix_stride > 0 ? s.x_pix_stride : s.Cin;
    d.pad_ = 0;
    chunks += (int)rn_cdiv(d.P, CH);
  }
  a.total_chunks = chunks; a.pad_ = 0;
}

// Pixel chunk length of a wgrad_big_kernel launch.  One workgroup per CU (128 KB of LDS).  Candidates: chunk lengths that
// give about 1, 1.5, 2 and 3 rounds of the CUs the kernel may use (opts.wgrad_target_blocks: that many workgroups, no
// candidate search); segments (pyramid levels) are chunked separately, so each candidate grows its chunk until the
// workgroup count fits.  The kernel hands XCD x a contiguous range of (chunk, tile) ids, and a launch whose tile count does
// not divide the 32 CUs of an XCD (27 tiles for 256 -> 720) leaves one round badly filled: the candidates are priced with
// a greedy simulation of that mapping (per-workgroup cost = K steps + a fixed prologue / epilogue / partial-tile cost) and
// the cheapest wins.  Cached per shape: planning a layer again (every training step) is one map lookup.
static long long wg_big_chunk(const rn_wgrad_problem* p, const WgArgs& a, int tiles) {
  const long long Ptot = wg_pixels(p);
  const bool target_user = p->opts.wgrad_target_blocks > 0;
  const long long target_blocks = target_user ? p->opts.wgrad_target_blocks : rn_num_cus() - p->opts.reserved_cus;
  static std::mutex mu;
  static std::unordered_map<std::string, long long> cache;
  std::string key((const char*)&target_blocks, sizeof(target_blocks));
  key.push_back(target_user ? 1 : 0);
  const int dims[4] = {a.R * 16 + a.S, a.Cin, a.Cout, p->num_segments};
  key.append((const char*)dims, sizeof(dims));
  for (int i = 0; i < p->num_segments; ++i) key.append((const char*)&a.seg[i].P, sizeof(a.seg[i].P));
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  long long CH = 0;
  const int mult_x2[4] = {2, 3, 4, 6};
  const int ncand = target_user ? 1 : 4;
  double best = 0;
  for (int c = 0; c < ncand; ++c) {
    const long long blocks = (long long)target_blocks * mult_x2[c] / 2;
    long long target = blocks / tiles;
    if (target < 1) target = 1;
    long long ch = rn_cdiv(rn_cdiv(Ptot, target), WGB_BK) * WGB_BK;
    if (ch < 4 * WGB_BK) ch = 4 * WGB_BK;
    int chunks = 0;
    for (int it2 = 0; it2 < 16; ++it2) {
      chunks = 0;
      for (int i = 0; i < p->num_segments; ++i) chunks += (int)rn_cdiv(a.seg[i].P, ch);
      if ((long long)chunks * tiles <= blocks || chunks <= 1) break;
      ch += WGB_BK * rn_cdiv(ch / WGB_BK, 16);    // +6 % per iteration
    }
    // greedy schedule of the kernel's XCD mapping: workgroup `logical` = chunk * tiles + tile
    const long long total = (long long)chunks * tiles;
    std::vector<int> steps;   // K steps of every chunk
    for (int i = 0; i < p->num_segments; ++i)
      for (long long b = 0; b < a.seg[i].P; b += ch)
        steps.push_back((int)rn_cdiv(std::min<long long>(ch, a.seg[i].P - b), WGB_BK));
    const double fixed = 30.0;   // prologue + epilogue + partial tile write, in K steps
    double makespan = 0;
    const long long q = total >> 3, rr = total & 7;
    long long begin = 0;
    for (int x = 0; x < 8; ++x) {
      const long long n = q + (x < rr ? 1 : 0);
      double cu[32];
      for (int k = 0; k < 32; ++k) cu[k] = 0;
      for (long long l = begin; l < begin + n; ++l) {
        int k0 = 0;
        for (int k = 1; k < 32; ++k) if (cu[k] < cu[k0]) k0 = k;
        cu[k0] += steps[(size_t)(l / tiles)] + fixed;
      }
      for (int k = 0; k < 32; ++k) makespan = std::max(makespan, cu[k]);
      begin += n;
    }
    if (c == 0 || makespan < best * 0.97) {   // more workgroups only for a clear gain
      best = makespan;
      CH = ch;
    }
  }
  cache.emplace(key, CH);
  return CH;
}

// Layers worth the 256 x 256 tile: both channel counts >= 256, enough pixels to split K over the CUs and at most 512
// tiles.  Turns the 128-tile arguments `a` of `p` into wgrad_big_kernel's (same workspace layout).
static bool wg_fill_big(const rn_wgrad_problem* p, WgArgs& a) {
  if (p->opts.wgrad_kernel == 1 || a.Cin < 256 || a.Cout < 256) return false;
  const int co_tiles = (int)rn_cdiv(a.Cout, 256), ci_tiles = (int)rn_cdiv(a.Cin, 256);
  const int tiles = co_tiles * ci_tiles * a.R * a.S;
  if ((wg_pixels(p) < 16384 && p->opts.wgrad_kernel < 2) || tiles > 512) return false;
  a.co_tiles = co_tiles; a.ci_tiles = ci_tiles; a.co_groups = 1; a.gco = co_tiles;
  a.CH = (int)wg_big_chunk(p, a, tiles);
  int chunks = 0;
  for (int i = 0; i < p->num_segments; ++i) {
    a.seg[i].chunk_begin = chunks;
    chunks += (int)rn_cdiv(a.seg[i].P, a.CH);
  }
  a.total_chunks = chunks;
  return true;
}

// ---- launch and reduction geometry of the chosen kernel --------------------------------------------------------------
static unsigned wg_persistent_grid(int items, const rn_launch_opts& opts) {
  rn_launch_opts o = opts;
  o.max_workgroups = 0;   // the cap is for the persistent convolution grids
  return (unsigned)(opts.reserved_cus > 0 ? rn_persistent_grid(items, rn_num_cus(), o) : items);
}

// the ordered reduction of a launch over pl.ngroups layers: pl.chunks partial tiles of weight_elems floats per layer
static void wg_plan_reduction(WgradPlan& pl, long long weight_elems) {
  pl.n4 = weight_elems / 4;
  pl.red_blocks = (int)(rn_cdiv(pl.n4, 64) < 4096 ? rn_cdiv(pl.n4, 64) : 4096);
  if (pl.red_blocks * pl.ngroups > 8192) pl.red_blocks = 8192 / pl.ngroups;
  pl.launch_bytes = (size_t)pl.ngroups * pl.chunks * weight_elems * sizeof(float);
}

static size_t wg_halo_bytes(const WhArgs& h) { return (size_t)h.ngroups * h.total_chunks * h.Cout * 9 * h.Cin * sizeof(float); }

static void wg_plan_halo(const rn_launch_opts& opts, WgradPlan& pl) {   // pl.h is filled
  const WhArgs& h = pl.h;
  pl.path = WG_PATH_HALO; pl.kid = 2; pl.ngroups = h.ngroups; pl.linear = false;
  pl.grid = wg_persistent_grid(h.ngroups * h.co_tiles * h.ci_tiles * h.total_chunks, opts);
  pl.chunks = h.total_chunks;
  wg_plan_reduction(pl, (long long)h.Cout * 9 * h.Cin);
}

// `p` on the per-tap kernels.  ngroups > 1: p's segments are the LAYERS of a group (one segment each): segment g's partial
// tiles are the chunks [g * total_chunks / ngroups, ...) of the workspace (layers of identical geometry: equal chunk counts).
static void wg_plan_taps(const rn_wgrad_problem* p, int ngroups, WgradPlan& pl) {
  WgArgs& a = pl.g;
  wg_fill_128(p, a);
  const bool big = wg_fill_big(p, a);
  pl.path = big ? WG_PATH_BIG : WG_PATH_128; pl.kid = big ? 1 : 0; pl.ngroups = ngroups;
  // LINEAR: stride 1, same-size output, symmetric padding, 31-bit offsets with room for the last K step
  pl.linear = a.sh == 1 && a.sw == 1 && a.pt == (a.R - 1) / 2 && a.pl == (a.S - 1) / 2 && (a.R & 1) && (a.S & 1);
  for (int i = 0; i < a.nseg; ++i) {
    const WgSegDev& s = a.seg[i];
    pl.linear = pl.linear && s.Ho == s.H && s.Wo == s.W &&
                (long long)s.N * s.H * s.W * (s.xS > s.dyS ? s.xS : s.dyS) * 2 < (1ll << 31) - (1ll << 24);
  }
  const int tiles = a.gco * a.ci_tiles * a.R * a.S * a.co_groups;   // big: co_groups = 1, gco = co_tiles
  pl.grid = big ? wg_persistent_grid(tiles * a.total_chunks, p->opts) : (unsigned)(tiles * a.total_chunks);
  pl.chunks = a.total_chunks / ngroups;
  wg_plan_reduction(pl, (long long)a.Cout * a.R * a.S * a.Cin);
}

// one validated problem: halo, then big, then 128
static void wg_plan_layer(const rn_wgrad_problem* p, WgradPlan& pl) {
  if (wg_halo_fill(&p, 1, pl.h)) wg_plan_halo(p->opts, pl);
  else wg_plan_taps(p, 1, pl);
  pl.ws_bytes = pl.launch_bytes;
}

// ---- the plan of a call: a pure function of the descriptors and rn_num_cus(); tensor pointers are read as "null or not" --
// A group (n >= 2) is equivalent to n single calls.  Identical layers that wgrad_halo_kernel serves (the eight head-tower
// layers, the 3x3 layers of a ResNet stage) run as ONE launch over (layer, co tile, ci tile) tiles.  Identical one-segment
// layers it does not serve (the 1x1 layers of a ResNet stage) group WITHOUT another kernel, as the SEGMENTS of a merged
// problem: the per-tap kernels already walk per-segment pointers and chunk ranges, and equal segments get equal chunk
// counts, so segment g's partial tiles are the [chunks / n] slice g of the workspace — the [group][chunk] layout the grouped
// reduction reads.  Either way the plan aims for the same number of workgroups over n layers' pixels, i.e. 1/n of the
// partial tiles per layer, and one reduction launch sums all layers.  Anything else is issued layer by layer.
static WgradPlan wgrad_plan(const rn_wgrad_problem* const* ps, int n) {
  WgradPlan pl;
  if (!ps || n < 1) return pl;
  bool valid = true;
  for (int i = 0; i < n; ++i) {
    if (!ps[i]) return pl;
    valid = valid && wg_valid(ps[i]);
  }
  if (n == 1) {
    if (valid) wg_plan_layer(ps[0], pl);
    pl.valid = valid;
    return pl;
  }
  bool same = n <= RN_WGRAD_MAX_GROUP && n <= RN_CONV_MAX_SEGMENTS && ps[0]->num_segments >= 1 &&
              ps[0]->num_segments <= RN_CONV_MAX_SEGMENTS;
  for (int i = 1; same && i < n; ++i) same = wg_same_geometry(*ps[0], *ps[i]);
  size_t need = 0;
  if (same && wg_halo_fill(ps, n, pl.h)) {
    // (decided before the validation result is read: rn_wgrad_group_fused has always answered 1 for such a group even
    // when its options are out of range; the workspace query then answers 0 and the launch rejects it)
    wg_plan_halo(ps[0]->opts, pl);
    pl.fused = 1;
    need = pl.launch_bytes;
  } else if (same && valid && ps[0]->num_segments == 1) {
    rn_wgrad_problem m = *ps[0];
    m.num_segments = n;
    for (int i = 0; i < n; ++i) m.seg[i] = ps[i]->seg[0];
    wg_plan_taps(&m, n, pl);
    pl.path = WG_PATH_SEGMENTS;
    pl.fused = 1;
    // The workspace query has always answered the merged problem's need AS A SINGLE CALL, and a single call of 3x3 layers
    // whose pixels only reach 16 384 together goes to wgrad_halo_kernel, which a group of segments never runs on.  Kept so
    // that the answers stay what they were; the launch checks launch_bytes as well.
    WhArgs single;
    const rn_wgrad_problem* mp = &m;
    need = wg_halo_fill(&mp, 1, single) ? wg_halo_bytes(single) : pl.launch_bytes;
  }
  if (!valid) return pl;
  pl.valid = true;
  // the workspace also fits every layer issued on its own (identical layers: one plan tells all)
  for (int i = 0; i < (same ? 1 : n); ++i) {
    WgradPlan layer;
    wg_plan_layer(ps[i], layer);
    need = std::max(need, layer.ws_bytes);
  }
  pl.ws_bytes = need;
  return pl;
}

// ---- the queries: one field of the plan each (rnet_hip.h) -----------------------------------------------------------
extern "C" int rn_wgrad_kernel_id(const rn_wgrad_problem* p) { return wgrad_plan(&p, 1).kid; }   // -1: malformed
extern "C" size_t rn_wgrad_workspace_bytes(const rn_wgrad_problem* p) { return wgrad_plan(&p, 1).ws_bytes; }
extern "C" size_t rn_wgrad_group_workspace_bytes(const rn_wgrad_problem* const* ps, int n) { return wgrad_plan(ps, n).ws_bytes; }
// 1: one grouped launch, 0: per-layer calls
extern "C" int rn_wgrad_group_fused(const rn_wgrad_problem* const* ps, int n) { return wgrad_plan(ps, n).fused; }

// ---- the launches: plan, check the caller's buffers against the plan, launch what it names ---------------------------
static int wgrad_check_workspace(const char* who, const WgradPlan& pl, const void* workspace, size_t workspace_bytes) {
  const size_t need = std::max(pl.ws_bytes, pl.launch_bytes);
  if (!workspace || workspace_bytes < need) {
    rn_set_error("%s: workspace %zu < %zu", who, workspace_bytes, need);
    return RN_ENOMEM;
  }
  return RN_OK;
}

// the partial-tile kernel of the plan, then the ordered reduction into dws[0 .. pl.ngroups)
static int wgrad_launch(WgradPlan& pl, int variant, void* workspace, float* const* dws, float beta, hipStream_t st) {
  WgDwPtrs d;
  for (int i = 0; i < pl.ngroups; ++i) d.p[i] = (float4*)dws[i];
  int rc;
  if (pl.kid == 2) {
    pl.h.ws = (float*)workspace;
    rc = rn_launch_wgrad_halo(pl.h, variant, pl.grid, st);
  } else {
    pl.g.ws = (float*)workspace;
    rc = pl.kid == 1 ? rn_launch_wgrad_big(pl.g, pl.linear, pl.grid, st) : rn_launch_wgrad128(pl.g, pl.linear, pl.grid, st);
  }
  if (rc != RN_OK) return rc;
  return rn_launch_wgrad_reduce(workspace, pl.n4, pl.chunks, d, pl.red_blocks, pl.ngroups, beta, st);
}

extern "C" int rn_conv2d_nhwc_wgrad(const rn_wgrad_problem* p, float* dw, float beta, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  WgradPlan pl = wgrad_plan(&p, 1);
  RN_CHECK_ARG(pl.valid, "rn_conv2d_nhwc_wgrad: bad problem (Cin %% 8, Cout %% 4, < 2^24 pixels, < 2 GiB tensors)");
  RN_CHECK_ARG(dw != nullptr, "rn_conv2d_nhwc_wgrad: null dw");
  if (const int rc = wgrad_check_workspace("rn_conv2d_nhwc_wgrad", pl, workspace, workspace_bytes)) return rc;
  return wgrad_launch(pl, p->opts.ablate, workspace, &dw, beta, (hipStream_t)stream);
}

extern "C" int rn_conv2d_nhwc_wgrad_group(const rn_wgrad_problem* const* ps, int n, float* const* dws, float beta,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  RN_CHECK_ARG(ps && dws && n >= 1, "rn_conv2d_nhwc_wgrad_group: bad argument");
  for (int i = 0; i < n; ++i) RN_CHECK_ARG(ps[i] && dws[i], "rn_conv2d_nhwc_wgrad_group: null problem / output %d", i);
  WgradPlan pl = wgrad_plan(ps, n);
  RN_CHECK_ARG(pl.valid, "rn_conv2d_nhwc_wgrad_group: bad problem");
  if (const int rc = wgrad_check_workspace("rn_conv2d_nhwc_wgrad_group", pl, workspace, workspace_bytes)) return rc;
  if (pl.path == WG_PATH_LAYERS) {   // every layer plans itself as it is issued
    for (int i = 0; i < n; ++i) {
      const int rc = rn_conv2d_nhwc_wgrad(ps[i], dws[i], beta, workspace, workspace_bytes, stream);
      if (rc != RN_OK) return rc;
    }
    return RN_OK;
  }
  return wgrad_launch(pl, ps[0]->opts.ablate, workspace, dws, beta, (hipStream_t)stream);
}
