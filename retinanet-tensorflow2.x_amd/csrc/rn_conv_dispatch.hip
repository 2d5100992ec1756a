// rn_conv_dispatch.hip — host-only: which kernel, tile shape and split plan a forward-convolution launch gets.
//
// conv_plan() is the one place that policy lives.  It fills a ConvPlan from the problem descriptor and rn_num_cus();
// rn_conv2d_nhwc_fwd builds its ConvArgs from that plan, and the four queries the engines size their buffers with
// (rn_conv_kernel_id, rn_conv_tile_rows, rn_conv_bn_row_blocks, rn_conv_splitk_workspace_bytes) read one field of it each —
// a query cannot disagree with the launch.  The kernels and their launch_* templates stay with their files
// (rn_conv.hip, rn_conv_big.hip, rn_conv_halo.hip; declared in rn_conv_dev.h).
#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

#include "rn_conv_dev.h"

extern "C" int rn_conv_cout_pad(int Cout) { return Cout <= 64 ? 64 : (int)rn_align_up((size_t)Cout, 128); }
// packed-weight channel count: Cin rounded up to the K step (32 below 64 channels, 64 above)
extern "C" int rn_conv_cin_pad(int Cin) { return Cin <= 32 ? 32 : (int)rn_align_up((size_t)Cin, 64); }
// GEMM columns of a w_pair segment (two weight planes along Cout): the packed rows
extern "C" int rn_conv_pair_rows(int Cout) { return Cout > 0 ? 128 * ((Cout + 63) / 64) : 0; }

struct ConvPlanSeg {
  int cols, cols_pad;      // GEMM columns (Cout, or for w_pair the packed rows) and rn_conv_cout_pad() of them
  int terms, cin_pad;      // weight planes along Cin (w_terms, at least 1); Cin rounded up to the K step
  long long M;             // output pixels N * Ho * Wo
  int n_tiles, tile_begin; // column tiles; first tile in the launch's numbering
  int bn_row_blocks;       // 128-pixel row blocks of fused BatchNorm partial sums the launch writes
};

struct ConvPlan {
  int kid;                 // 0 = 128-row conv_fwd_kernel, 1 = conv_big_kernel, 2 = conv_halo_kernel with 256 x 256 tiles,
                           // 3 = conv_halo_kernel with 512 x 128 tiles
  int BM, BN;              // tile rows and columns
  int BK;                  // K step of the 128-row kernel for segment 0's channels (validation uses it whichever kernel runs)
  int bal_rows;            // conv_big_kernel: pixels a balanced tile covers, 0 = whole tiles
  bool deal;               // conv_big_kernel: tiles numbered deepest segment first and dealt round-robin
  bool fast_div;           // every M < 2^22: the kernels' float-reciprocal index arithmetic is valid
  int order[RN_CONV_MAX_SEGMENTS];   // launch position -> segment
  long long total_tiles;
  int min_depth;           // K extent per tap (terms * cin_pad) of the shallowest segment
  int split_parts;         // 128-row kernel: parts every tile is cut into along K (1: whole tiles)
  long long ws_bytes;      // split-K workspace the launch can use (0: it would not split)
  ConvPlanSeg seg[RN_CONV_MAX_SEGMENTS];
};

// the one tile count: tiles of `rows` pixels x `width` columns that cover a segment
static long long seg_tiles(const ConvPlanSeg& s, int rows, int width) { return rn_cdiv(s.M, rows) * rn_cdiv(s.cols_pad, width); }
static long long conv_tiles(const ConvPlan& pl, int nseg, int rows, int width) {
  long long t = 0;
  for (int i = 0; i < nseg; ++i) t += seg_tiles(pl.seg[i], rows, width);
  return t;
}

// 3x3 / stride 1 / pad 1 launches can run on the halo kernel (rn_conv_halo.hip) when every segment's worst tile of BM
// pixels (256, or 512 for the narrow form) fits its patch buffer.
static bool conv_halo_fits(const rn_conv_problem* p, int BM) {
  if (p->opts.conv_no_halo) return false;
  if (p->R != 3 || p->S != 3 || p->stride_h != 1 || p->stride_w != 1 || p->pad_top != 1 || p->pad_left != 1)
    return false;
  static std::mutex mu;
  static std::map<std::tuple<int, int, int, int>, int> patch_px;   // (N, H, W, BM) -> worst patch, computed once (O(M / BM))
  for (int i = 0; i < p->num_segments; ++i) {
    const rn_conv_segment& s = p->seg[i];
    if (s.Ho != s.H || s.Wo != s.W || s.Cin % 32 != 0) return false;
    if ((long long)s.N * s.H * s.W >= (1ll << 22)) return false;   // the kernel's float-reciprocal divisions
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple(s.N, s.H, s.W, BM);
    auto it = patch_px.find(key);
    if (it == patch_px.end()) it = patch_px.emplace(key, rn_conv_halo_patch_pixels(s.N, s.H, s.W, rn_conv_halo_pitch(s.W), BM)).first;
    if (it->second > rn_conv_halo_capacity(BM)) return false;
  }
  return true;
}

// Last-round split of a persistent launch (rnet_hip.h: rn_conv_problem.splitk_ws).  G0 workgroups walk `total` tiles in
// rounds; the L = total mod G0 tiles of the last round are each cut into S = min(G0 / L, chunks / 4, 4) parts along K, so
// that round keeps L * S workgroups busy for 1/S of a tile (+ the exchange of L * (S - 1) accumulator tiles through the
// workspace) instead of L workgroups for a whole one.
static int splitk_parts(int total, int min_chunks, int G0, long long* bytes) {
  const int L = total % G0;
  if (bytes) *bytes = 0;
  if (L == 0 || L > 511 || min_chunks < 8) return 1;   // 8 arrival counters per leftover tile in a 4096-word header
  // every part costs its tile one more 256 KB slot to write and part 0 one more to read (~4 us each): at least 4 chunks
  // (36 K steps, ~20 us) per part, at most 4 parts
  int S = G0 / L;
  if (S > min_chunks / 4) S = min_chunks / 4;
  if (S > 4) S = 4;
  if (S < 2) return 1;
  if (bytes) *bytes = RN_SPLITK_HEADER_BYTES + (long long)L * S * RN_SPLITK_SLOT_BYTES;   // one slot per part
  return S;
}

// that plan for a launch of a.total_tiles tiles whose shortest tile has `min_chunks` K chunks: fills a.split_f / split_s /
// vtotal / ws (no split when ws is null or too small)
static void rn_splitk_plan(ConvArgs& a, int min_chunks, void* ws, long long ws_bytes, const rn_launch_opts& opts) {
  const int total = a.total_tiles;
  a.split_f = total; a.split_s = 1; a.vtotal = total; a.pad2_ = 0; a.ws = nullptr;
  const int G0 = rn_persistent_grid(0x7fffffff, rn_num_cus(), opts);
  const int L = total % G0;
  int S = ws ? splitk_parts(total, min_chunks, G0, nullptr) : 1;
  while (S >= 2 && RN_SPLITK_HEADER_BYTES + (long long)L * S * RN_SPLITK_SLOT_BYTES > ws_bytes) --S;
  if (S < 2) return;
  a.split_f = total - L; a.split_s = S; a.vtotal = L * S; a.ws = (float*)ws;   // vtotal: units of the SPLIT launch
}

// what any problem can use on any grid: 16 KB header + 256 accumulator slots (one per part: L * S <= 256 workgroups)
extern "C" size_t rn_conv_splitk_workspace_max_bytes(void) { return RN_SPLITK_HEADER_BYTES + 256ull * RN_SPLITK_SLOT_BYTES; }

// Balanced tiles for conv_big_kernel's HBM-bound 1x1 launches.  The persistent grid walks its 256-row tiles in rounds of one
// per workgroup; a launch of 3.1 rounds runs as 4 with most of the chip idle in the last one (ResNet stage 3 `*_out` at
// B = 32: 800 tiles on 256 workgroups), and a tile's time there is set by its bytes, not by its MFMAs (four to sixteen K
// steps between a pipeline refill and a 128 KB epilogue).  A 1x1 tile's rows are independent, so the SAME number of rounds
// can be cut finer: rows = ceil(M / floor(rounds * grid / column tiles)) pixels per tile instead of 256 — every workgroup
// then walks `rounds` tiles of rows/256 of the bytes each (the rows a tile does not cover are masked: zero-filled by the
// DMA, never stored; their MFMAs run on zeros).  The busiest workgroup of the 256-row plan keeps its tile count and moves
// fewer bytes; nobody moves more.  Single-segment 1x1 / stride 1 launches only, shallow enough that bytes set the pace
// (K <= 512), and only when it shortens the tiles by 8 % or more; opts.conv_tile / conv_big_min_tiles / max_workgroups
// (tests, A/B) and an attached split-K workspace keep whole tiles.  Results are the same values: a tile's accumulation
// order does not depend on its rows.  Returns the rows per tile, 0 = whole 256-row tiles.  The fused BatchNorm partial sums
// are still written per (tile, half): two row blocks per tile (ConvPlanSeg::bn_row_blocks).
static int conv_big_balanced_rows(const rn_conv_problem* p, const ConvPlanSeg& s) {
  if (p->num_segments != 1 || p->R != 1 || p->S != 1 || p->stride_h != 1 || p->stride_w != 1) return 0;
  if (p->opts.conv_tile || p->opts.conv_big_min_tiles || p->opts.max_workgroups || p->splitk_ws) return 0;
  if (s.terms * s.cin_pad > 512) return 0;
  const int n_tiles = (int)rn_cdiv(s.cols_pad, 256);
  const int G = rn_persistent_grid(0x7fffffff, rn_num_cus(), p->opts);
  const long long T = seg_tiles(s, 256, 256);
  if (T <= 0 || G <= 0) return 0;
  const long long rounds = rn_cdiv(T, G);
  const long long m_tiles = rounds * G / n_tiles;   // row blocks that fit `rounds` rounds
  if (m_tiles < 1) return 0;
  long long rows = rn_cdiv(s.M, m_tiles);
  rows = (rows + 3) / 4 * 4;
  if (rows < 64 || rows > 236) return 0;            // (236 = 0.92 * 256)
  return (int)rows;
}

// Parts every tile of a 128-row launch of `tiles` tiles with `ksteps` K steps is cut into along K (1: whole tiles): small
// launches of deep layers (fewer tiles than the chip has compute units: batch-1 / batch-8 inference, ResNet stage 3 / 4, the
// FPN laterals).  Enough parts to put about one workgroup on three of every four compute units (opts.splitk_target_blocks
// moves the target), at least RN_SPLIT128_MIN_STEPS K steps per part (a part costs a 32 - 64 KB partial tile written and
// read back and a ~2 us hand-off), at most 8 parts (the last arriver keeps one 16-byte load per part in flight), the slots
// must fit the workspace and the tiles its 4096 counters.
#define RN_SPLIT128_MIN_STEPS 4
static int conv128_split_parts(const rn_launch_opts& opts, long long tiles, int ksteps, int BN, long long ws_bytes) {
  if (opts.conv_tile == 1 || tiles < 1 || tiles > 4096) return 1;
  // default target: three quarters of the compute units.  Same-box sweep with the counted-wait K loop, three rounds
  // (tools/bench_infer.py --split-target): batch-1 serving 1.357 / 1.360 / 1.353 ms at 256 workgroups, 1.322 / 1.310 / 1.318 at
  // 192, 1.323 / 1.323 / 1.315 at 160; batch 8 within +-0.4 % of each other (fewer, longer parts: less exchange traffic).
  const int target = opts.splitk_target_blocks > 0 ? opts.splitk_target_blocks : rn_num_cus() * 3 / 4;
  int S = target / (int)tiles;
  if (S > ksteps / RN_SPLIT128_MIN_STEPS) S = ksteps / RN_SPLIT128_MIN_STEPS;
  if (S > 8) S = 8;
  const long long slot = 128ll * BN * 4;
  while (S >= 2 && RN_SPLITK_HEADER_BYTES + tiles * S * slot > ws_bytes) --S;
  return S >= 2 ? S : 1;
}

// The plan of a launch: a pure function of the descriptor and rn_num_cus() that reads pointers only as "null or not"
// (bias, residual, splitk_ws).  assume_ws: plan the split as if a workspace of the largest useful size were attached when
// none is (rn_conv_splitk_workspace_bytes).  False on a descriptor without a valid segment count.
static bool conv_plan(const rn_conv_problem* p, bool assume_ws, ConvPlan& pl) {
  if (!p || p->num_segments < 1 || p->num_segments > RN_CONV_MAX_SEGMENTS) return false;
  const int nseg = p->num_segments;
  const rn_launch_opts& o = p->opts;

  // ---- per segment: every derived quantity, once -------------------------------------------------------------------
  bool all_wide = true, all_128 = true, all_128s_or_64 = true, one_col = true;   // padded columns: >= 256 / == 128 / n * 128 or 64 / <= 256
  bool epi_ok = true;        // the 256- / 512-row epilogues take every segment
  long long dmin = 1ll << 60, dmax = 0;   // K depth (all taps), shallowest and deepest segment
  pl.min_depth = 0x7fffffff;
  pl.fast_div = true;
  for (int i = 0; i < nseg; ++i) {
    const rn_conv_segment& s = p->seg[i];
    ConvPlanSeg& d = pl.seg[i];
    d.cols = s.w_pair ? rn_conv_pair_rows(s.Cout) : s.Cout;
    d.cols_pad = rn_conv_cout_pad(d.cols);
    d.terms = s.w_terms > 1 ? s.w_terms : 1;
    d.cin_pad = rn_conv_cin_pad(s.Cin);
    d.M = (long long)s.N * s.Ho * s.Wo;
    all_wide = all_wide && d.cols_pad >= 256;
    all_128 = all_128 && d.cols_pad == 128;
    all_128s_or_64 = all_128s_or_64 && (d.cols_pad % 128 == 0 || d.cols_pad == 64);
    one_col = one_col && d.cols_pad <= 256;
    // channel granularity of those epilogues: 16-byte rows of bf16, or of f32 (float4 stores); their residual variants
    // carry no bias path
    epi_ok = epi_ok && s.Cout % (p->out_dtype == RN_DT_F32 && s.w_pair ? 4 : 8) == 0 && !(s.bias && s.residual);
    const int depth = d.terms * d.cin_pad;
    pl.min_depth = depth < pl.min_depth ? depth : pl.min_depth;
    const long long depth_all = (long long)p->R * p->S * d.cin_pad * d.terms;
    dmin = depth_all < dmin ? depth_all : dmin;
    dmax = depth_all > dmax ? depth_all : dmax;
    pl.fast_div = pl.fast_div && d.M < (1 << 22);
  }
  // K step of the 128-row kernel: 64, or 32 when the padded channel count is not a multiple of 64 — and for the shallow
  // layers (K = R S Cin <= 256: ResNet stage 1's 256 -> 64, the first 1x1 of stage 2), which are HBM-bound: four stages of half
  // the size stream better than two or three (profiles/r05_ab/summary.tsv: 256 -> 64 at 160 x 160, batch 32, 133.9 -> 119.3 us;
  // 256 -> 128 194.0 -> 183.0) while every deeper layer loses 10 - 15 % to the second barrier per 16 MFMAs.  Cin need only be
  // a multiple of 8: the tail of the last K step reads past the pixel's channels (or out of range -> zeros) and meets the
  // zero-padded weight columns, so it contributes nothing.
  const int cin0 = pl.seg[0].cin_pad;
  pl.BK = (cin0 % 64 != 0 || (long long)p->R * p->S * cin0 <= 256) ? 32 : 64;

  // ---- kernel family -----------------------------------------------------------------------------------------------
  // 256 x 256 x 32 tiles (rn_conv_big.hip, rn_conv_halo.hip) for the MFMA-bound layers: every segment at least 256 output
  // channels wide, and enough tiles to fill the 256 CUs (one workgroup per CU) a few times over.  (rn_launch_opts: conv_tile
  // forces either family, conv_big_min_tiles moves the threshold.)
  // A launch of fewer tiles than compute units (batch-8 inference, ResNet stage 3 / 4) stays on the 128-row kernel.  Round 4
  // sent it to the halo kernel's 256 x 256 tiles, every tile cut along K, when a split-K workspace was attached; with the
  // counted-wait K loop of the 128-row kernel (and its own split-K) that choice loses: stage-3 3x3 at batch 8 43.7 vs 36.0 us,
  // batch 16 53.2 vs 46.1; stage-4 3x3 45.3 vs 42.6 at batch 8, 59.4 vs 61.4 at batch 16 (tools/probes/ab_small_3x3.sh); the
  // five-level head / FPN launches at batch 1: 46.6 vs 43.9, 63.9 vs 47.0, 41.8 vs 32.9 (tools/probes/ab_b1_heads.sh).
  // rn_launch_opts.conv_tile = 2 still takes a small launch to the halo kernel, split when a workspace is attached.
  const bool use_big = o.conv_tile != 1 && o.conv_tile != 3 && all_wide && epi_ok &&
                       (o.conv_tile == 2 || conv_tiles(pl, nseg, 256, 256) >= (o.conv_big_min_tiles > 0 ? o.conv_big_min_tiles : 192));
  if (use_big) {
    // A 3x3 / stride 1 launch that qualifies for the 256 x 256 halo tiles runs as 512 x 128 tiles instead when the longer
    // patches fit (its channel counts are multiples of 128): the same number of tiles and MACs per tile, but a K chunk
    // stages ~117 KB instead of ~171 KB per workgroup (one 8 KB weight piece per tap instead of 16 KB; the patch of 512
    // consecutive pixels has relatively fewer halo rows).  Measured inside the step on one box (round 4): head-tower launches
    // 564 -> 511 us, class prediction 1460 -> 1333, ResNet stage-3 3x3 (200 tiles) 59.8 -> 56.8, batch-8 towers 157 -> 152.
    // conv_tile = 2 and conv_big_min_tiles keep the 256 x 256 form (tests, A/B).
    if (!conv_halo_fits(p, 256)) pl.kid = 1;
    else pl.kid = (o.conv_tile == 0 && o.conv_big_min_tiles == 0 && conv_halo_fits(p, 512)) ? 3 : 2;
  } else {
    // 3x3 / stride 1 / pad 1 layers with 64 < Cout <= 128 (ResNet stage 2: 128 -> 128 at 80 x 80, forward and data gradient):
    // the halo kernel with 512 x 128 tiles (rn_conv_halo.hip, HaloGeo<4>: 4 x 2 waves of 128 pixels x 64 channels).  On the
    // 128-row kernel such a layer staged its pixels once per tap (the LDS-DMA path bound it at ~550 TFLOP/s); in a 256-wide
    // tile of the halo kernel half the waves multiply zero rows.  conv_tile = 3: any width that is a multiple of 128, also
    // <= 64 channels (half of the tile's columns are then zero weights).  Enough tiles to fill the chip once; conv_tile >= 2
    // forces the form (tests at small sizes).
    const bool halo512 = o.conv_tile != 1 && !o.conv_no_halo && (o.conv_tile == 3 ? all_128s_or_64 : all_128) && epi_ok &&
                         (o.conv_tile >= 2 || conv_tiles(pl, nseg, 512, 128) >= (o.conv_big_min_tiles > 0 ? o.conv_big_min_tiles : 128)) &&
                         conv_halo_fits(p, 512);
    pl.kid = halo512 ? 3 : 0;
  }

  // ---- tile shape --------------------------------------------------------------------------------------------------
  pl.bal_rows = 0;
  if (pl.kid == 0) {
    // 128 x 128, or 128 x 64 for Cout <= 64 and for small launches (batch-8 inference, ResNet stage 4: 100 tiles of 128 x 128
    // on 256 CUs): the narrower tiles put the work on twice as many CUs and read 12 KB instead of 16 KB of LDS fragments per
    // wave and K step — the 128-row kernel is bound by fragment bandwidth at one workgroup per CU (DESIGN.md section 4,
    // round-3 probes).  Only while they still fit one per CU: at two per CU they share that bandwidth again.  conv_tile = 1
    // keeps 128 x 128 (tests).
    pl.BM = 128;
    pl.BN = pl.seg[0].cols_pad <= 64 ? 64 : 128;
    if (pl.BN == 128 && o.conv_tile != 1 && 2 * conv_tiles(pl, nseg, 128, 128) <= rn_num_cus()) pl.BN = 64;
  } else if (pl.kid == 3) {
    pl.BM = 512; pl.BN = 128;
  } else {
    pl.BM = 256; pl.BN = 256;
    if (pl.kid == 1) pl.bal_rows = conv_big_balanced_rows(p, pl.seg[0]);
  }

  // ---- segment order and tile numbering ----------------------------------------------------------------------------
  // conv_big_kernel launch whose segments are all one column tile wide but differ 2x or more in K depth (the FPN lateral 1x1
  // convs: 512 / 1024 / 2048 input channels): tiles numbered deepest segment first and dealt to the workgroups round-robin
  // (identity numbering) instead of in the XCD-contiguous ranges that keep neighbouring column tiles on one L2 — there are
  // no neighbouring column tiles here, and a contiguous range hands one XCD all of the 64-step tiles (181 K steps per CU
  // there against 87 on average).  The order is internal to the launch: every tile's result is what it was.
  for (int i = 0; i < nseg; ++i) pl.order[i] = i;
  pl.deal = pl.kid == 1 && nseg > 1 && one_col && dmax >= 2 * dmin;
  if (pl.deal)
    std::stable_sort(pl.order, pl.order + nseg, [&](int x, int y) {
      return pl.seg[x].cin_pad * pl.seg[x].terms > pl.seg[y].cin_pad * pl.seg[y].terms;
    });
  const int rows = pl.bal_rows ? pl.bal_rows : pl.BM;
  pl.total_tiles = 0;
  for (int ii = 0; ii < nseg; ++ii) {
    ConvPlanSeg& d = pl.seg[pl.order[ii]];
    d.n_tiles = (int)rn_cdiv(d.cols_pad, pl.BN);
    d.tile_begin = (int)pl.total_tiles;
    // a balanced tile writes two row blocks, the second one short
    d.bn_row_blocks = (int)(pl.bal_rows ? 2 * rn_cdiv(d.M, rows) : (rows / 128) * rn_cdiv(d.M, rows));
    pl.total_tiles += seg_tiles(d, rows, pl.BN);
  }

  // ---- split along K -----------------------------------------------------------------------------------------------
  pl.split_parts = 1;
  pl.ws_bytes = 0;
  if (pl.kid == 0) {          // every tile cut into split_parts parts of one [128][BN] fp32 slot each
    if (p->splitk_ws || assume_ws) {
      const long long avail = p->splitk_ws ? p->splitk_ws_bytes : (long long)rn_conv_splitk_workspace_max_bytes();
      pl.split_parts = conv128_split_parts(o, pl.total_tiles, p->R * p->S * (pl.min_depth / pl.BK), pl.BN, avail);
    }
    if (pl.split_parts >= 2) pl.ws_bytes = RN_SPLITK_HEADER_BYTES + pl.total_tiles * pl.split_parts * 128 * pl.BN * 4;
  } else if (pl.kid == 2) {   // the tiles of the last round, in K chunks of 32 channels x all taps (rn_splitk_plan at launch)
    splitk_parts((int)pl.total_tiles, pl.min_depth / 32, rn_persistent_grid(0x7fffffff, rn_num_cus(), o), &pl.ws_bytes);
  }                           // conv_big_kernel and the 512 x 128 form run whole tiles only (the 1x1 layers are HBM-bound)
  return true;
}

// ---- the queries: one field of the plan each -----------------------------------------------------------------------
extern "C" size_t rn_conv_splitk_workspace_bytes(const rn_conv_problem* p) {
  ConvPlan pl;
  return conv_plan(p, true, pl) ? (size_t)pl.ws_bytes : 0;
}

/* 0: 128-row conv_fwd_kernel, 1: conv_big_kernel, 2: conv_halo_kernel (256 x 256 tiles), 3: conv_halo_kernel (512 x 128 tiles) */
extern "C" int rn_conv_kernel_id(const rn_conv_problem* p) {
  ConvPlan pl;
  return conv_plan(p, false, pl) ? pl.kid : -1;
}

extern "C" int rn_conv_bn_row_blocks(const rn_conv_problem* p, int segment) {
  ConvPlan pl;
  if (!conv_plan(p, false, pl) || segment < 0 || segment >= p->num_segments) return 0;
  return pl.seg[segment].bn_row_blocks;
}

extern "C" int rn_conv_tile_rows(const rn_conv_problem* p) {
  ConvPlan pl;
  return conv_plan(p, false, pl) ? pl.BM : 0;
}

// ---- the launch: validate, plan, fill ConvArgs from the plan, launch -----------------------------------------------
// what the kernels the plan picked require of the descriptor (the w_pair and K-step checks read the plan)
static int conv_validate(const rn_conv_problem* p, const ConvPlan& pl) {
  RN_CHECK_ARG(p->R >= 1 && p->S >= 1 && p->R * p->S <= 32, "rn_conv2d_nhwc_fwd: R*S=%d > 32", p->R * p->S);
  RN_CHECK_ARG(p->stride_h >= 1 && p->stride_w >= 1, "rn_conv2d_nhwc_fwd: bad stride");
  RN_CHECK_ARG(p->out_dtype == RN_DT_BF16 || p->out_dtype == RN_DT_F32, "rn_conv2d_nhwc_fwd: bad out_dtype");
  if (const int orc = rn_validate_launch_opts(p->opts, "rn_conv2d_nhwc_fwd")) return orc;
  for (int ii = 0; ii < p->num_segments; ++ii) {
    const int i = pl.order[ii];
    const rn_conv_segment& s = p->seg[i];
    RN_CHECK_ARG(s.x && s.w && s.y, "rn_conv2d_nhwc_fwd: segment %d has a null tensor", i);
    RN_CHECK_ARG(s.N > 0 && s.H > 0 && s.W > 0 && s.Ho > 0 && s.Wo > 0 && s.Cout > 0 && s.Cin > 0,
                 "rn_conv2d_nhwc_fwd: segment %d bad shape", i);
    RN_CHECK_ARG(s.Cin % 8 == 0 && pl.seg[i].cin_pad % pl.BK == 0,
                 "rn_conv2d_nhwc_fwd: segment %d Cin=%d must be a multiple of 8 (K step %d)", i, s.Cin, pl.BK);
    RN_CHECK_ARG(s.pix_stride % 4 == 0 && s.pix_stride > 0,
                 "rn_conv2d_nhwc_fwd: segment %d pix_stride=%d must be a positive multiple of 4", i, s.pix_stride);
    RN_CHECK_ARG(s.Cout % 4 == 0, "rn_conv2d_nhwc_fwd: segment %d Cout=%d not a multiple of 4", i, s.Cout);
    RN_CHECK_ARG((pl.seg[i].cols_pad <= 64) == (pl.seg[0].cols_pad <= 64), "rn_conv2d_nhwc_fwd: segments mix Cout tile widths");
    RN_CHECK_ARG(!s.w_pair || (pl.kid != 0 && p->out_dtype == RN_DT_F32 && s.w_terms <= 1 && !s.scale && !s.shift &&
                               !s.residual && !s.bn_partial),
                 "rn_conv2d_nhwc_fwd: segment %d: w_pair needs an f32 launch without scale / shift / residual that the 256- / "
                 "512-row kernels take (rn_conv_kernel_id() != 0)", i);
    RN_CHECK_ARG(((uintptr_t)s.x | (uintptr_t)s.w | (uintptr_t)s.y | (uintptr_t)s.residual) % 16 == 0,
                 "rn_conv2d_nhwc_fwd: segment %d tensors must be 16-byte aligned", i);
    RN_CHECK_ARG(pl.seg[i].M < (1ll << 31) && (long long)s.N * s.H * s.W * s.pix_stride * 2 < (1ll << 31),
                 "rn_conv2d_nhwc_fwd: segment %d input exceeds the 2 GiB buffer-addressing limit", i);
    if (s.bn_bwd_y) {
      RN_CHECK_ARG(s.bn_partial && s.bn_bwd_fwd && p->out_dtype == RN_DT_BF16 && !s.scale && !s.shift && !s.bias &&
                       !s.residual && p->act == RN_ACT_NONE && s.Cout % 8 == 0 && (uintptr_t)s.bn_bwd_y % 16 == 0,
                   "rn_conv2d_nhwc_fwd: segment %d: bn_bwd_y needs bn_partial + bn_bwd_fwd on a plain bf16 launch", i);
    }
    RN_CHECK_ARG((s.bn_bwd_y != nullptr) == (p->seg[0].bn_bwd_y != nullptr),
                 "rn_conv2d_nhwc_fwd: bn_bwd_y must be set on all segments or none");
    RN_CHECK_ARG(pl.seg[i].terms <= 3, "rn_conv2d_nhwc_fwd: segment %d w_terms=%d (1..3)", i, s.w_terms);
  }
  RN_CHECK_ARG(p->splitk_ws == nullptr || ((uintptr_t)p->splitk_ws % 16 == 0 && p->splitk_ws_bytes >= 0),
               "rn_conv2d_nhwc_fwd: splitk_ws must be 16-byte aligned");
  return RN_OK;
}

extern "C" int rn_conv2d_nhwc_fwd(const rn_conv_problem* p, void* stream) {
  RN_CHECK_ARG(p != nullptr, "rn_conv2d_nhwc_fwd: null problem");
  RN_CHECK_ARG(p->num_segments >= 1 && p->num_segments <= RN_CONV_MAX_SEGMENTS,
               "rn_conv2d_nhwc_fwd: num_segments=%d", p->num_segments);
  ConvPlan pl;
  conv_plan(p, false, pl);
  if (const int rc = conv_validate(p, pl)) return rc;

  ConvArgs a;
  a.R = p->R; a.S = p->S; a.sh = p->stride_h; a.sw = p->stride_w; a.pt = p->pad_top; a.pl = p->pad_left;
  a.act = p->act; a.nseg = p->num_segments;
  a.total_tiles = (int)pl.total_tiles;
  // pad_ bit 0: float-reciprocal index arithmetic in the tile set-up (128-row kernel, conv_big_kernel; the halo kernel is
  // only picked where it holds); bit 1: conv_big_kernel deals its tiles round-robin
  a.pad_ = pl.kid <= 1 ? (pl.fast_div ? 1 : 0) | (pl.deal ? 2 : 0) : 0;
  a.split_f = a.vtotal = a.total_tiles; a.split_s = 1; a.pad2_ = 0; a.ws = nullptr;
  for (int ii = 0; ii < p->num_segments; ++ii) {
    const rn_conv_segment& s = p->seg[pl.order[ii]];
    const ConvPlanSeg& ps = pl.seg[pl.order[ii]];
    ConvSegDev& d = a.seg[ii];
    d.x = (const uint16_t*)s.x; d.w = (const uint16_t*)s.w; d.y = s.y;
    d.scale = s.scale; d.shift = s.shift; d.residual = (const uint16_t*)s.residual;
    d.bn_partial = s.bn_partial;
    d.bn_y = (const uint16_t*)s.bn_bwd_y;
    d.bn_fwd = s.bn_bwd_fwd;
    d.bias = s.bias;
    d.N = s.N; d.H = s.H; d.W = s.W; d.Cin = s.Cin; d.pix_stride = s.pix_stride;
    d.Ho = s.Ho; d.Wo = s.Wo; d.Cout = ps.cols;
    d.pair_cout = s.w_pair ? s.Cout : 0;
    d.rows = pl.bal_rows;
    d.M = (int)ps.M;
    d.tile_begin = ps.tile_begin;
    d.n_tiles = ps.n_tiles;
    d.cwrap = ps.cin_pad;
    d.CinP = ps.terms * ps.cin_pad;
    d.halo_pitch = s.W + 1;   // rn_conv_halo_pitch: the one pitch there is
  }

  hipStream_t st = (hipStream_t)stream;
  const bool f32 = p->out_dtype == RN_DT_F32;
  switch (pl.kid) {
    case 3: return rn_launch_conv_halo(a, f32, p->opts, st, 4);
    case 2:
      rn_splitk_plan(a, pl.min_depth / 32, p->splitk_ws, p->splitk_ws_bytes, p->opts);
      return rn_launch_conv_halo(a, f32, p->opts, st);
    case 1: return rn_launch_conv_big(a, f32, p->opts, st);
  }
  if (pl.split_parts >= 2) {
    a.split_s = pl.split_parts; a.vtotal = a.total_tiles * pl.split_parts; a.ws = (float*)p->splitk_ws;
  }
  return rn_launch_conv128(a, pl.BN, pl.BK, f32, pl.split_parts >= 2, st);
}
