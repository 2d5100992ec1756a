// rn_conv.hip — K1/K2: grouped implicit-GEMM NHWC convolution on gfx950 MFMA.
// Replaces tf.keras.layers.Conv2D as used by the reference's ResNet
// (retinanet/model/backbone/resnet.py:118-144), FPN (model/neck/fpn_base.py:44-50,
// model/neck/fpn.py:47-66) and detection heads (model/head/detection_head.py:56-88).
//
// GEMM view: M = N*Ho*Wo output pixels, N = Cout, K = R*S*Cin; A[m][k] is gathered on the fly
// from the NHWC input (for one filter tap the Cin slice of a pixel is contiguous), B is the
// prepacked weight [Cout_pad][R*S*Cin] (k contiguous), accumulation fp32 on
// v_mfma_f32_32x32x16_bf16.
//
// This file: weight / image packing, and the 128-row kernel — workgroup = 256 threads =
// 4 wavefronts (2x2), tile BM x BN x BK = 128 x {128,64} x {64,32} — that serves the narrow layers and the
// small launches; layers with Cout >= 256 and enough tiles go to the persistent 256 x 256 x 32 kernel in
// rn_conv_big.hip.  Which launch gets which kernel: rn_conv_dispatch.hip (conv_plan).
//   * staging by `buffer_load ... lds` DMA (16 B per lane, no VGPR round trip) into a ring of three or four LDS
//     stages — as many as leave two workgroups per CU (launch_conv) — with counted waits and ONE s_barrier per
//     K step: the DMA of step t + STAGES - 1 is issued before the MFMAs of step t.
//   * LDS tiles are [rows][BK] bf16 with the 16-byte slot index XOR-swizzled by
//     (row / rows_per_256B) — applied to the DMA's per-lane source chunk and to the ds_read_b128
//     fragment address — so the fragment reads (one row per lane, same k slot) hit 16 distinct
//     16-byte slots of the 256-byte bank row: conflict free.
//   * padding / image borders / M tail: per-row tap-validity bitmask computed once per tile;
//     invalid pieces get an out-of-range buffer offset, which the hardware zero-fills.
//   * epilogue: acc*scale[c]+shift[c] staged through LDS as fp32 [BM][BN] (reusing the A/B
//     buffers), then read back row-contiguous: + residual, activation, convert, 8/16-byte
//     coalesced stores.  BN(+bias) folding makes Conv+BN+ReLU(+add) one kernel at inference.
//   * grouped launch: up to 10 independent segments (pyramid levels / both heads) share one
//     grid, so the small P5-P7 problems ride along with P3 instead of under-filling 256 CUs.
//   * blockIdx -> tile map is XCD aware: consecutive tiles (same A rows, neighbouring n tiles)
//     land on the same XCD's L2 (blocks are dispatched round-robin over the 8 XCDs).
// Roofline: MFMA-bound for K >= ~512; the small-K 1x1 convs of ResNet stage 1-2 are HBM-bound.
#include "rn_conv_dev.h"

// 2 x 2 wavefronts (64 x (BN/2) wave tiles): 128 x {128,64} x {64,32} for the narrow / small launches; the wide layers
// go to rn_conv_big.hip.  STAGES (launch_conv picks it from the tile's bytes): 3 or 4 = that many whole LDS stages,
// 32 = three stages of pixels and two of weights (128 x 128 x 64); 48 - 80 KB of LDS, two workgroups per CU.
// SPLIT (rnet_hip.h: rn_conv_problem.splitk_ws; small launches of deep layers — batch-1 / batch-8 inference): every tile is
// cut along K into args.split_s parts, one workgroup each (grid = total_tiles * split_s, the parts of a tile neighbours in
// the XCD-aware numbering).  A part writes its raw fp32 accumulators — in the [BM][BN] row layout the epilogue's second
// stage reads — to its slot of the workspace with write-through (sc1) stores, drains them, and counts itself in on the
// tile's counter with a returning agent-scope atomic; the part that arrives LAST (whichever it is: nobody waits) reads
// all slots back with sc1 loads, adds them IN PART ORDER (the same bits on every run), zeroes the counter and runs the
// epilogue arithmetic (bias, rounding points, BatchNorm affine, residual, activation) on the sums.
template <int BM, int BN, int BK, bool OUT_F32, int STAGES, bool SPLIT>
__global__ void __launch_bounds__(CONV_THREADS, 2) conv_fwd_kernel(const ConvArgs args) {
  static_assert((STAGES >= 3 && STAGES <= 8) || STAGES == 32, "no K loop for this stage count");
  constexpr int WM = 2, WN = 2;                     // wavefronts along M / N
  constexpr int NWAVES = WM * WN;
  constexpr int NTHREADS = 64 * NWAVES;
  constexpr int SLOTS = BK / 8;
  constexpr int RPI = 64 / SLOTS;                   // rows per wave DMA instruction (1 KiB)
  constexpr int A_INSTR = BM / RPI / NWAVES;        // DMA instructions per wave for the A tile
  constexpr int B_INSTR = BN / RPI / NWAVES;
  constexpr int WTM = BM / WM, WTN = BN / WN;       // wave tile
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int KSUB = BK / 16;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  static_assert(A_INSTR >= 1 && B_INSTR >= 1, "tile too small for the wave count");

  extern __shared__ __attribute__((aligned(16))) char smem[];

  // ---- tile lookup (XCD-aware remap of the linear block id) ---------------------------------
  int tile, part = 0;
  {
    const int total = SPLIT ? args.vtotal : args.total_tiles;   // work units: tiles, or (tile, part) pairs
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int q = total >> 3, r = total & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    if (SPLIT) {
      const int v = tile;
      tile = v / args.split_s;
      part = v - tile * args.split_s;
    }
  }
  int si = 0;
#pragma unroll 1
  for (int i = 1; i < args.nseg; ++i)
    if (tile >= args.seg[i].tile_begin) si = i;
  const ConvSegDev& sg = args.seg[si];
  const int lt = tile - sg.tile_begin;
  const int m_tile = lt / sg.n_tiles, n_tile = lt - m_tile * sg.n_tiles;
  const int m0 = m_tile * BM, n0 = n_tile * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / WN, wave_n = wave % WN;

  const int R = args.R, S = args.S;
  const int H = sg.H, W = sg.W, Cin = sg.CinP, PS = sg.pix_stride;
  const int M = sg.M;
  const int Ktot = R * S * Cin;
  const int cwrap = sg.cwrap;   // split-bf16 weight planes: the input channels repeat every cwrap

  const __amdgpu_buffer_rsrc_t rs_x =
      __builtin_amdgcn_make_buffer_rsrc((void*)sg.x, 0, (int)((long long)sg.N * H * W * PS * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc((void*)sg.w, 0, (int)((long long)sg.n_tiles * BN * Ktot * 2), 0x00020000);

  // ---- per-lane DMA bookkeeping: instruction j of this wave fills rows (j*4 + wave)*RPI .. ----
  const int d_row = lane / SLOTS, d_pos = lane % SLOTS;
  unsigned a_off[A_INSTR];   // byte offset of (row's first tap pixel, its k chunk) or RN_OOB
  unsigned a_mask[A_INSTR];
#pragma unroll
  for (int j = 0; j < A_INSTR; ++j) {
    const int row = (j * NWAVES + wave) * RPI + d_row;
    const int chunk = d_pos ^ lds_swz<BK>(row);
    const int m = m0 + row;
    const int mm = m < M ? m : 0;
    int ox, oy, n;
    if (args.pad_ & 1) {   // every M < 2^22: float-reciprocal divisions (~8 VALU instead of ~45 each; four rows x two per thread
                           // were ~1 us of every launch's prologue — a tenth of a batch-1 layer)
      const int t2 = rn_fdiv(mm, sg.Wo, rn_rcp((float)sg.Wo));
      ox = mm - t2 * sg.Wo;
      n = rn_fdiv(t2, sg.Ho, rn_rcp((float)sg.Ho));
      oy = t2 - n * sg.Ho;
    } else {
      ox = mm % sg.Wo;
      const int t2 = mm / sg.Wo;
      oy = t2 % sg.Ho;
      n = t2 / sg.Ho;
    }
    const int iy0 = oy * args.sh - args.pt, ix0 = ox * args.sw - args.pl;
    a_off[j] = (unsigned)(((((long long)n * H + iy0) * W + ix0) * PS + chunk * 8) * 2);
    unsigned mask = 0;
    if (m < M) {
      for (int r = 0; r < R; ++r)
        for (int s = 0; s < S; ++s) {
          const bool ok = (unsigned)(iy0 + r) < (unsigned)H && (unsigned)(ix0 + s) < (unsigned)W;
          mask |= (ok ? 1u : 0u) << (r * S + s);
        }
    }
    a_mask[j] = mask;
  }
  unsigned b_off[B_INSTR];
#pragma unroll
  for (int j = 0; j < B_INSTR; ++j) {
    const int row = (j * NWAVES + wave) * RPI + d_row;
    const int chunk = d_pos ^ lds_swz<BK>(row);
    b_off[j] = (unsigned)(((long long)(n0 + row) * Ktot + chunk * 8) * 2);
  }

  // fragment read offsets (row = lane&31 of a 32-row tile, k slot = 2*kk + (lane>>5))
  const int frag_row = lane & 31, frag_half = lane >> 5;
  int rd_a[TM][KSUB], rd_b[TN][KSUB];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int kk = 0; kk < KSUB; ++kk)
      rd_a[i][kk] = lds_slot_off<BK>(wave_m * WTM + i * 32 + frag_row, kk * 2 + frag_half);
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int kk = 0; kk < KSUB; ++kk)
      rd_b[j][kk] = A_BYTES + lds_slot_off<BK>(wave_n * WTN + j * 32 + frag_row, kk * 2 + frag_half);

  f32x16_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int ksteps_all = R * S * (Cin / BK);
  // K steps [kbeg, ksteps) of this workgroup: all of them, or the part's share
  const int kbeg = SPLIT ? (int)((long long)part * ksteps_all / args.split_s) : 0;
  const int ksteps = SPLIT ? (int)((long long)(part + 1) * ksteps_all / args.split_s) : ksteps_all;

#define RN_ISSUE_TILE(buf, tap_, c0_)                                                         \
  do {                                                                                        \
    const int r__ = (tap_) / S, s__ = (tap_) - r__ * S;                                       \
    const int cw__ = (c0_) < cwrap ? (c0_) : ((c0_) < 2 * cwrap ? (c0_) - cwrap : (c0_) - 2 * cwrap);   \
    const unsigned tap_off__ = (unsigned)((((long long)r__ * W + s__) * PS + cw__) * 2);      \
    char* st__ = smem + (buf) * STAGE_BYTES;                                                  \
    _Pragma("unroll") for (int j = 0; j < A_INSTR; ++j) {                                     \
      const unsigned v__ = ((a_mask[j] >> (tap_)) & 1u) ? a_off[j] + tap_off__ : RN_OOB;      \
      dma16(rs_x, st__ + (j * NWAVES + wave) * 1024, v__);                                    \
    }                                                                                         \
    const unsigned koff__ = (unsigned)(((long long)(tap_) * Cin + (c0_)) * 2);                \
    _Pragma("unroll") for (int j = 0; j < B_INSTR; ++j)                                       \
      dma16(rs_w, st__ + A_BYTES + (j * NWAVES + wave) * 1024, b_off[j] + koff__);            \
  } while (0)

  int tap = 0, c0 = 0;   // coordinates of the NEXT tile to issue
  if (SPLIT) {
    const int cpk = Cin / BK;
    tap = kbeg / cpk;
    c0 = (kbeg - tap * cpk) * BK;
  }
#define RN_ADVANCE()  \
  do {                \
    c0 += BK;         \
    if (c0 >= Cin) {  \
      c0 = 0;         \
      ++tap;          \
    }                 \
  } while (0)

  if (STAGES <= 8) {
    // STAGES LDS stages, counted waits: the DMA of step kt + STAGES - 1 is issued while step kt is multiplied, so a tile's
    // bytes have STAGES - 1 steps to arrive instead of one (a two-stage loop that waits for ALL outstanding pieces — i.e. for
    // the round trip of the tile it issued at the top of the same step — before every barrier cost ~1.2 us per K step
    // whatever the step computed).  One s_barrier per step (no fence: __syncthreads() would put s_waitcnt vmcnt(0) in front of it):
    // behind it every wave's pieces of step kt have landed and every wave has finished reading step kt - 1, whose stage
    // the next issue overwrites.
    constexpr int PIECES = A_INSTR + B_INSTR;   // DMA instructions per wave and K step
    constexpr int AHEAD = STAGES - 1;
#pragma unroll
    for (int q = 0; q < AHEAD; ++q)
      if (kbeg + q < ksteps) {
        RN_ISSUE_TILE(q, tap, c0);
        RN_ADVANCE();
      }
    int cur = 0;
#pragma unroll 1
    for (int kt = kbeg; kt < ksteps; ++kt) {
      // everything but the pieces of the AHEAD - 1 newest steps has landed (at the tail, where fewer are in flight: all)
      if (kt + AHEAD - 1 < ksteps) asm volatile("s_waitcnt vmcnt(%0)" ::"i"((AHEAD - 1) * PIECES) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (kt + AHEAD < ksteps) {
        const int nxt = cur >= 1 ? cur - 1 : STAGES - 1;   // (cur + STAGES - 1) % STAGES
        RN_ISSUE_TILE(nxt, tap, c0);
        RN_ADVANCE();
      }
      const char* base = smem + cur * STAGE_BYTES;
#pragma unroll
      for (int kk = 0; kk < KSUB; ++kk) {
        bf16x8_t fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = *(const bf16x8_t*)(base + rd_a[i][kk]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = *(const bf16x8_t*)(base + rd_b[j][kk]);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = RN_MFMA_32x32x16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
      cur = cur == STAGES - 1 ? 0 : cur + 1;
    }
    __syncthreads();   // the epilogue reuses the stages
  } else {
    // 128 x 128 x 64 (32 KB per K step; three whole stages would leave one workgroup per CU): THREE stages of pixels, TWO of
    // weights, 80 KB — two workgroups per CU.  The pixels come from HBM (or another XCD's L2) and get two steps to arrive; the
    // weights are L2-resident and get one.  Issue order per step: weights of step kt + 1, THEN pixels of step kt + 2, so that
    // "everything but the last A_INSTR pieces" (loads retire in order) = pixels and weights of step kt + 1.
    constexpr int B0 = 3 * A_BYTES;   // the weight stages sit behind the three pixel stages
    int tap_a = tap, c0_a = c0, tap_b = tap, c0_b = c0;   // the pixel stream runs one step ahead of the weight stream
#define RN_ISSUE_A(buf, tap_, c0_)                                                            \
  do {                                                                                        \
    const int r__ = (tap_) / S, s__ = (tap_) - r__ * S;                                       \
    const int cw__ = (c0_) < cwrap ? (c0_) : ((c0_) < 2 * cwrap ? (c0_) - cwrap : (c0_) - 2 * cwrap);   \
    const unsigned tap_off__ = (unsigned)((((long long)r__ * W + s__) * PS + cw__) * 2);      \
    _Pragma("unroll") for (int j = 0; j < A_INSTR; ++j) {                                     \
      const unsigned v__ = ((a_mask[j] >> (tap_)) & 1u) ? a_off[j] + tap_off__ : RN_OOB;      \
      dma16(rs_x, smem + (buf) * A_BYTES + (j * NWAVES + wave) * 1024, v__);                   \
    }                                                                                         \
  } while (0)
#define RN_ISSUE_B(buf, tap_, c0_)                                                            \
  do {                                                                                        \
    const unsigned koff__ = (unsigned)(((long long)(tap_) * Cin + (c0_)) * 2);                \
    _Pragma("unroll") for (int j = 0; j < B_INSTR; ++j)                                       \
      dma16(rs_w, smem + B0 + (buf) * B_BYTES + (j * NWAVES + wave) * 1024, b_off[j] + koff__); \
  } while (0)
#define RN_ADV(tap_, c0_) do { c0_ += BK; if (c0_ >= Cin) { c0_ = 0; ++tap_; } } while (0)
    // prologue: pixels of steps 0 and 1, weights of step 0 (weights first where both are issued)
    RN_ISSUE_B(0, tap_b, c0_b); RN_ADV(tap_b, c0_b);
    RN_ISSUE_A(0, tap_a, c0_a); RN_ADV(tap_a, c0_a);
    if (kbeg + 1 < ksteps) { RN_ISSUE_A(1, tap_a, c0_a); RN_ADV(tap_a, c0_a); }
    int cur_a = 0, cur_b = 0;
#pragma unroll 1
    for (int kt = kbeg; kt < ksteps; ++kt) {
      // pixels and weights of step kt have landed: everything but the pixel pieces of step kt + 1 (the newest issue)
      if (kt + 1 < ksteps) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(A_INSTR) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (kt + 1 < ksteps) { RN_ISSUE_B(cur_b ^ 1, tap_b, c0_b); RN_ADV(tap_b, c0_b); }
      if (kt + 2 < ksteps) {
        const int nxt = cur_a >= 1 ? cur_a - 1 : 2;   // (cur_a + 2) % 3
        RN_ISSUE_A(nxt, tap_a, c0_a); RN_ADV(tap_a, c0_a);
      }
      const char* base_a = smem + cur_a * A_BYTES;
      const char* base_b = smem + B0 + cur_b * B_BYTES - A_BYTES;   // rd_b carries + A_BYTES
#pragma unroll
      for (int kk = 0; kk < KSUB; ++kk) {
        bf16x8_t fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = *(const bf16x8_t*)(base_a + rd_a[i][kk]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = *(const bf16x8_t*)(base_b + rd_b[j][kk]);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = RN_MFMA_32x32x16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
      cur_a = cur_a == 2 ? 0 : cur_a + 1;
      cur_b ^= 1;
    }
    __syncthreads();   // the epilogue reuses the stages
#undef RN_ADV
#undef RN_ISSUE_B
#undef RN_ISSUE_A
  }
#undef RN_ADVANCE
#undef RN_ISSUE_TILE

  // ---- epilogue ------------------------------------------------------------------------------
  // fused BatchNorm backward reduction (rn_conv_segment.bn_bwd_y): the y values stage 2 needs — this thread's 4
  // channels of its BM / ROWS rows — are fetched NOW, so that their HBM latency runs under stage 1 and the barrier
  // (loaded where they are used, behind the stores of the previous row, each launch paid ~35 us for them)
  constexpr int E_TPR = BN / 4, E_ROWS = NTHREADS / E_TPR, E_NIT = BM / E_ROWS;
  uint2 ypre[E_NIT];
  if (!OUT_F32 && sg.bn_partial != nullptr && sg.bn_y != nullptr) {
    const int er_ = tid / E_TPR, n_ = n0 + (tid % E_TPR) * 4;
#pragma unroll
    for (int it = 0; it < E_NIT; ++it) {
      const int m_ = m0 + er_ + it * E_ROWS;
      ypre[it] = make_uint2(0u, 0u);
      if (m_ < M && n_ < sg.Cout) ypre[it] = *(const uint2*)(sg.bn_y + (long long)m_ * sg.Cout + n_);
    }
  }
  // stage 1: registers -> LDS fp32 [BM][BN]: conv (+bias) output and BatchNorm affine, each rounded to bf16 where
  // the reference holds a bf16 tensor between two layers (rnet_hip.h, rn_conv_segment)
  float* cl = (float*)smem;
  const int Cout = sg.Cout;
  const bool affine = sg.scale != nullptr || sg.shift != nullptr;
  const bool has_res = sg.residual != nullptr;
  const bool round1 = !OUT_F32 && (affine || has_res);
  const bool round2 = !OUT_F32 && affine && has_res;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wave_n * WTN + j * 32 + (lane & 31);
    const int n = n0 + nl;
    float sc = 1.0f, sf = 0.0f, bs = 0.0f;
    if (n < Cout) {
      if (sg.scale) sc = sg.scale[n];
      if (sg.shift) sf = sg.shift[n];
      if (sg.bias) bs = sg.bias[n];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float t[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) t[r] = SPLIT ? acc[i][j][r] : acc[i][j][r] + bs;   // SPLIT: raw partial sums
      if (!SPLIT && round1) {   // uniform branches per stage, not per element
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = rn_rb(t[r]);
      }
      if (!SPLIT && affine) {
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = t[r] * sc + sf;
      }
      if (!SPLIT && round2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = rn_rb(t[r]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = wave_m * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        cl[ml * BN + nl] = t[r];
      }
    }
  }
  __syncthreads();
  // stage 2: row-contiguous read back, residual, activation, store
  constexpr int TPR = BN / 4;                 // threads per row (4 channels each)
  constexpr int ROWS = NTHREADS / TPR;        // rows per pass
  const int er = tid / TPR, ec = (tid % TPR) * 4;
  const int n = n0 + ec;
  // ---- SPLIT: partial tile -> workspace, count in; only the last part to arrive carries on (see the kernel's header) ----
  typedef unsigned cf_u32x4_t __attribute__((ext_vector_type(4)));
  constexpr int SLOT_BYTES = BM * BN * 4;
  __amdgpu_buffer_rsrc_t rs_parts = __builtin_amdgcn_make_buffer_rsrc((void*)sg.y, 0, 0, 0x00020000);   // (set below; unused unless SPLIT)
  float ssc[4] = {1.f, 1.f, 1.f, 1.f}, ssf[4] = {0.f, 0.f, 0.f, 0.f}, sbs[4] = {0.f, 0.f, 0.f, 0.f};
  if (SPLIT) {
    const int S_ = args.split_s;
    char* const slot0 = (char*)args.ws + RN_SPLITK_HEADER_BYTES + (size_t)tile * S_ * SLOT_BYTES;
    const __amdgpu_buffer_rsrc_t rs_mine =
        __builtin_amdgcn_make_buffer_rsrc((void*)(slot0 + (size_t)part * SLOT_BYTES), 0, SLOT_BYTES, 0x00020000);
#pragma unroll
    for (int it = 0; it < E_NIT; ++it) {
      const int rr = er + it * ROWS;
      const float4 v = *(const float4*)(cl + rr * BN + ec);
      const cf_u32x4_t u = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
      __builtin_amdgcn_raw_buffer_store_b128(u, rs_mine, (rr * BN + ec) * 4, 0, 16);   // aux 16 = sc1: write-through
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();            // every thread's stores have drained; nobody reads cl any more
    if (tid == 0) {
      unsigned* const cnt = (unsigned*)args.ws + tile;
      const unsigned old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == (unsigned)(S_ - 1)) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next launch
      *(volatile unsigned*)smem = old;
    }
    __syncthreads();
    if (*(volatile unsigned*)smem != (unsigned)(S_ - 1)) return;
    __syncthreads();            // (the statistics reduction below reuses smem)
    rs_parts = __builtin_amdgcn_make_buffer_rsrc((void*)slot0, 0, S_ * SLOT_BYTES, 0x00020000);
    if (n < sg.Cout) {          // this thread's four channels: the arithmetic stage 1 skipped
      if (sg.scale) { const float4 a = *(const float4*)(sg.scale + n); ssc[0] = a.x; ssc[1] = a.y; ssc[2] = a.z; ssc[3] = a.w; }
      if (sg.shift) { const float4 a = *(const float4*)(sg.shift + n); ssf[0] = a.x; ssf[1] = a.y; ssf[2] = a.z; ssf[3] = a.w; }
      if (sg.bias) { const float4 a = *(const float4*)(sg.bias + n); sbs[0] = a.x; sbs[1] = a.y; sbs[2] = a.z; sbs[3] = a.w; }
    }
  }
  // fused BatchNorm forward statistics (rn_conv_segment.bn_partial): sums of the STORED bf16 values of this
  // thread's 4 channels over its rows; reduced over the workgroup's 128 rows below
  const bool stats = !OUT_F32 && sg.bn_partial != nullptr;
  // ... or stage 1 of the BatchNorm BACKWARD reduction of the layer whose dz this launch writes
  // (rn_conv_segment.bn_bwd_y): sums of g = dz * [y*scale + shift > 0] and of g*xhat
  const bool bnbwd = stats && sg.bn_y != nullptr;
  float bsc[4] = {0.f, 0.f, 0.f, 0.f}, bsh[4] = {0.f, 0.f, 0.f, 0.f}, bmu[4] = {0.f, 0.f, 0.f, 0.f}, bis[4] = {0.f, 0.f, 0.f, 0.f};
  if (bnbwd && n < Cout) {
    const float4 m4 = *(const float4*)(sg.bn_fwd + n), i4 = *(const float4*)(sg.bn_fwd + Cout + n);
    const float4 a4 = *(const float4*)(sg.bn_fwd + 2 * Cout + n), b4 = *(const float4*)(sg.bn_fwd + 3 * Cout + n);
    bmu[0] = m4.x; bmu[1] = m4.y; bmu[2] = m4.z; bmu[3] = m4.w;
    bis[0] = i4.x; bis[1] = i4.y; bis[2] = i4.z; bis[3] = i4.w;
    bsc[0] = a4.x; bsc[1] = a4.y; bsc[2] = a4.z; bsc[3] = a4.w;
    bsh[0] = b4.x; bsh[1] = b4.y; bsh[2] = b4.z; bsh[3] = b4.w;
  }
  float st0[4] = {0.f, 0.f, 0.f, 0.f}, st1[4] = {0.f, 0.f, 0.f, 0.f};
  if (n < Cout) {
#pragma unroll
    for (int it = 0; it < E_NIT; ++it) {
      const int rr = er + it * ROWS;
      const int m = m0 + rr;
      if (m >= M) break;
      float4 v;
      if (SPLIT) {
        // all parts' loads in flight before the first add; parts past split_s lie outside the descriptor and read as
        // zeros (at most 8 parts: the host's plan)
        cf_u32x4_t pv[8];
#pragma unroll
        for (int p_ = 0; p_ < 8; ++p_)
          pv[p_] = __builtin_amdgcn_raw_buffer_load_b128(rs_parts, (rr * BN + ec) * 4 + p_ * SLOT_BYTES, 0, 16);   // sc1
        float f4[4] = {__uint_as_float(pv[0].x), __uint_as_float(pv[0].y), __uint_as_float(pv[0].z), __uint_as_float(pv[0].w)};
#pragma unroll
        for (int p_ = 1; p_ < 8; ++p_) {
          f4[0] += __uint_as_float(pv[p_].x); f4[1] += __uint_as_float(pv[p_].y);
          f4[2] += __uint_as_float(pv[p_].z); f4[3] += __uint_as_float(pv[p_].w);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float t = f4[q] + sbs[q];
          if (round1) t = rn_rb(t);
          if (affine) t = t * ssc[q] + ssf[q];
          if (round2) t = rn_rb(t);
          f4[q] = t;
        }
        v = make_float4(f4[0], f4[1], f4[2], f4[3]);
      } else {
        v = *(const float4*)(cl + rr * BN + ec);
      }
      const long long o = (long long)m * Cout + n;
      if (sg.residual) {
        const uint2 rv = *(const uint2*)(sg.residual + o);
        v.x += rn_bf16_to_f32((uint16_t)(rv.x & 0xffffu));
        v.y += rn_bf16_to_f32((uint16_t)(rv.x >> 16));
        v.z += rn_bf16_to_f32((uint16_t)(rv.y & 0xffffu));
        v.w += rn_bf16_to_f32((uint16_t)(rv.y >> 16));
      }
      {
        float f4[4] = {v.x, v.y, v.z, v.w};
        if (!OUT_F32 && args.act == RN_ACT_SWISH) {   // tf.nn.swish reads the layer output as a bf16 tensor
#pragma unroll
          for (int q = 0; q < 4; ++q) f4[q] = rn_rb(f4[q]);
        }
        rn_apply_act_n<4>(f4, args.act);
        v = make_float4(f4[0], f4[1], f4[2], f4[3]);
      }
      if (OUT_F32) {
        *(float4*)((float*)sg.y + o) = v;
      } else {
        uint2 pk;
        pk.x = rn_pack_bf16x2(v.x, v.y);
        pk.y = rn_pack_bf16x2(v.z, v.w);
        *(uint2*)((uint16_t*)sg.y + o) = pk;
        if (stats) {
          const float w4[4] = {rn_lo16(pk.x), rn_hi16(pk.x), rn_lo16(pk.y), rn_hi16(pk.y)};
          if (bnbwd) {
            const uint2 yv = ypre[it];
            const float y4[4] = {rn_lo16(yv.x), rn_hi16(yv.x), rn_lo16(yv.y), rn_hi16(yv.y)};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float g = (y4[q] * bsc[q] + bsh[q]) > 0.0f ? w4[q] : 0.0f;
              st0[q] += g;
              st1[q] += g * ((y4[q] - bmu[q]) * bis[q]);
            }
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) { st0[q] += w4[q]; st1[q] += w4[q] * w4[q]; }
          }
        }
      }
    }
  }
  if (stats) {   // uniform per workgroup (one segment per tile)
    __syncthreads();                       // every thread is done reading cl
    float* red = cl;                       // [2][ROWS][BN]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      red[er * BN + ec + q] = st0[q];
      red[(ROWS + er) * BN + ec + q] = st1[q];
    }
    __syncthreads();
    if (tid < BN && n0 + tid < Cout) {     // fixed order over the ROWS row lanes: deterministic
      float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) { s0 += red[r * BN + tid]; s1 += red[(ROWS + r) * BN + tid]; }
      float* dst = sg.bn_partial + (long long)(m0 / BM) * 2 * Cout + n0 + tid;
      dst[0] = s0;
      dst[Cout] = s1;
    }
  }
}

// ---- host side: the launch (rn_conv_dev.h: rn_launch_conv128) ----------------------------------
template <int BM, int BN, int BK, bool F32, bool SPLIT>
static int launch_conv(const ConvArgs& a, hipStream_t st) {
  constexpr int stage = (BM + BN) * BK * 2;
  constexpr int epi = BM * BN * 4;
  // as many stages (up to four) as leave two workgroups per CU: 128 x 64 x 64: three (72 KB); 128 x 128 x 32: four (64 KB);
  // 128 x 64 x 32: four (48 KB); 128 x 128 x 64 (32 KB per K step: three whole stages would be 96 KB, one workgroup per CU:
  // measured 35 - 45 % slower wherever a launch has more tiles than compute units, equal below) gets 32 = three stages of
  // pixels + two of weights, 80 KB
  constexpr int STAGES = (4 * stage <= 72 * 1024) ? 4 : ((3 * stage <= 72 * 1024) ? 3 : 32);
  static_assert(STAGES != 32 || (BM == 128 && BN == 128 && BK == 64), "the 3 + 2 stage ring is laid out for 128 x 128 x 64");
  constexpr int ring = STAGES == 32 ? 3 * BM * BK * 2 + 2 * BN * BK * 2 : STAGES * stage;
  constexpr int lds = (ring > epi) ? ring : epi;
  auto kern = conv_fwd_kernel<BM, BN, BK, F32, STAGES, SPLIT>;
  if (lds > 48 * 1024)
    RN_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(kern, dim3(SPLIT ? a.vtotal : a.total_tiles), dim3(CONV_THREADS), lds, st, a);
  RN_CHECK_LAUNCH();
  return RN_OK;
}
// the 128-row kernel by tile shape / output type / split
template <bool SPLIT>
static int launch_conv128(const ConvArgs& a, int BN, int BK, bool f32, hipStream_t st) {
  if (BN == 128 && BK == 64) return f32 ? launch_conv<128, 128, 64, true, SPLIT>(a, st) : launch_conv<128, 128, 64, false, SPLIT>(a, st);
  if (BN == 64 && BK == 64) return f32 ? launch_conv<128, 64, 64, true, SPLIT>(a, st) : launch_conv<128, 64, 64, false, SPLIT>(a, st);
  if (BN == 128 && BK == 32) return f32 ? launch_conv<128, 128, 32, true, SPLIT>(a, st) : launch_conv<128, 128, 32, false, SPLIT>(a, st);
  return f32 ? launch_conv<128, 64, 32, true, SPLIT>(a, st) : launch_conv<128, 64, 32, false, SPLIT>(a, st);
}
int rn_launch_conv128(const ConvArgs& a, int BN, int BK, bool f32, bool split, hipStream_t st) {
  return split ? launch_conv128<true>(a, BN, BK, f32, st) : launch_conv128<false>(a, BN, BK, f32, st);
}

// ---- weight / input packing ----------------------------------------------------------------
__global__ void pack_weight_kernel(const float* __restrict__ w, int R, int S, int Cin, int Cout, int Cin_pad,
                                   int Cout_pad, uint16_t* __restrict__ out) {
  const long long total = (long long)Cout_pad * R * S * Cin_pad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cin_pad);
    long long t = i / Cin_pad;
    const int s = (int)(t % S);
    t /= S;
    const int r = (int)(t % R);
    const int o = (int)(t / R);
    float v = 0.0f;
    if (o < Cout && c < Cin) v = w[(((long long)r * S + s) * Cin + c) * Cout + o];
    out[i] = rn_f32_to_bf16(v);
  }
}

extern "C" int rn_pack_conv_weight(const float* w_hwio, int R, int S, int Cin, int Cout, int Cin_pad,
                                   void* w_packed, void* stream) {
  RN_CHECK_ARG(w_hwio && w_packed && R > 0 && S > 0 && Cin > 0 && Cout > 0 && Cin_pad >= Cin,
               "rn_pack_conv_weight: bad argument");
  const int Cout_pad = rn_conv_cout_pad(Cout);
  const long long total = (long long)Cout_pad * R * S * Cin_pad;
  int blocks = (int)(rn_cdiv(total, 256) < 4096 ? rn_cdiv(total, 256) : 4096);
  hipLaunchKernelGGL(pack_weight_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w_hwio, R, S, Cin,
                     Cout, Cin_pad, Cout_pad, (uint16_t*)w_packed);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

// the same packing from the training engine's master layout [Cout][R][S][Cin] (f32)
__global__ void pack_weight_ohwi_kernel(const float* __restrict__ w, int RS, int Cin, int Cout, int Cin_pad,
                                        int Cout_pad, uint16_t* __restrict__ out) {
  const long long total = (long long)Cout_pad * RS * Cin_pad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cin_pad);
    const long long t = i / Cin_pad;   // = o * RS + tap
    float v = 0.0f;
    if (t < (long long)Cout * RS && c < Cin) v = w[t * Cin + c];
    out[i] = rn_f32_to_bf16(v);
  }
}

extern "C" int rn_pack_conv_weight_ohwi(const float* w_ohwi, int R, int S, int Cin, int Cout, int Cin_pad,
                                        void* w_packed, void* stream) {
  RN_CHECK_ARG(w_ohwi && w_packed && R > 0 && S > 0 && Cin > 0 && Cout > 0 && Cin_pad >= Cin,
               "rn_pack_conv_weight_ohwi: bad argument");
  const int Cout_pad = rn_conv_cout_pad(Cout);
  const long long total = (long long)Cout_pad * R * S * Cin_pad;
  int blocks = (int)(rn_cdiv(total, 256) < 4096 ? rn_cdiv(total, 256) : 4096);
  hipLaunchKernelGGL(pack_weight_ohwi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w_ohwi, R * S, Cin,
                     Cout, Cin_pad, Cout_pad, (uint16_t*)w_packed);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

// split-bf16 planes of an f32 kernel (rn_conv_segment.w_terms): [Cout_pad][R*S][terms][Cin_pad], plane 0 = rb(w),
// plane t = rb(w - planes before it) — x (a bf16 tensor) times the f32 weight, to 16 / 24 weight mantissa bits
__global__ void pack_weight_split_kernel(const float* __restrict__ w, int ohwi, int RS, int Cin, int Cout, int Cin_pad,
                                         int Cout_pad, int terms, uint16_t* __restrict__ out) {
  const long long total = (long long)Cout_pad * RS * Cin_pad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cin_pad);
    const long long t = i / Cin_pad;   // = o * RS + tap
    const int tap = (int)(t % RS), o = (int)(t / RS);
    float v = 0.0f;
    if (o < Cout && c < Cin) v = ohwi ? w[t * Cin + c] : w[((long long)tap * Cin + c) * Cout + o];
    uint16_t* dst = out + (t * terms) * Cin_pad + c;
    for (int k = 0; k < terms; ++k) {
      const uint16_t b = rn_f32_to_bf16(v);
      dst[(long long)k * Cin_pad] = b;
      v -= rn_bf16_to_f32(b);   // exact: the residual of a round-to-nearest is representable in fp32
    }
  }
}

// rn_conv_segment.w_pair: the two planes along Cout — packed row 64b + 32h + c = plane h of channel 32b + c
__global__ void pack_weight_pair_kernel(const float* __restrict__ w, int ohwi, int RS, int Cin, int Cout, int Cin_pad,
                                        int rows, uint16_t* __restrict__ out) {
  const long long total = (long long)rows * RS * Cin_pad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cin_pad);
    const long long t = i / Cin_pad;   // = row * RS + tap
    const int tap = (int)(t % RS), row = (int)(t / RS);
    const int o = (row >> 6) * 32 + (row & 31), plane = (row >> 5) & 1;
    float v = 0.0f;
    if (o < Cout && c < Cin) v = ohwi ? w[((long long)o * RS + tap) * Cin + c] : w[((long long)tap * Cin + c) * Cout + o];
    const uint16_t b = rn_f32_to_bf16(v);
    out[i] = plane ? rn_f32_to_bf16(v - rn_bf16_to_f32(b)) : b;
  }
}

extern "C" int rn_pack_conv_weight_pair(const float* w, int layout_ohwi, int R, int S, int Cin, int Cout, int Cin_pad,
                                        void* w_packed, void* stream) {
  RN_CHECK_ARG(w && w_packed && R > 0 && S > 0 && Cin > 0 && Cout > 0 && Cin_pad >= Cin,
               "rn_pack_conv_weight_pair: bad argument");
  const int rows = rn_conv_pair_rows(Cout);
  const long long total = (long long)rows * R * S * Cin_pad;
  int blocks = (int)(rn_cdiv(total, 256) < 4096 ? rn_cdiv(total, 256) : 4096);
  hipLaunchKernelGGL(pack_weight_pair_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, layout_ohwi, R * S,
                     Cin, Cout, Cin_pad, rows, (uint16_t*)w_packed);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

extern "C" int rn_pack_conv_weight_split(const float* w, int layout_ohwi, int R, int S, int Cin, int Cout, int Cin_pad,
                                         int terms, void* w_packed, void* stream) {
  RN_CHECK_ARG(w && w_packed && R > 0 && S > 0 && Cin > 0 && Cout > 0 && Cin_pad >= Cin && terms >= 1 && terms <= 3,
               "rn_pack_conv_weight_split: bad argument");
  const int Cout_pad = rn_conv_cout_pad(Cout);
  const long long total = (long long)Cout_pad * R * S * Cin_pad;
  int blocks = (int)(rn_cdiv(total, 256) < 4096 ? rn_cdiv(total, 256) : 4096);
  hipLaunchKernelGGL(pack_weight_split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, layout_ohwi, R * S,
                     Cin, Cout, Cin_pad, Cout_pad, terms, (uint16_t*)w_packed);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

// stem: HWIO [R,S,3,Cout] (S <= 8) -> [Cout_pad][R][8 taps][4 ch]; taps >= S and channel 3 are zero
__global__ void pack_stem_weight_kernel(const float* __restrict__ w, int R, int S, int Cout, int Cout_pad,
                                        uint16_t* __restrict__ out) {
  const int total = Cout_pad * R * 32;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int c = i & 3, s = (i >> 2) & 7, r = (i >> 5) % R, o = i / (R * 32);
    float v = 0.0f;
    if (o < Cout && c < 3 && s < S) v = w[((r * S + s) * 3 + c) * Cout + o];
    out[i] = rn_f32_to_bf16(v);
  }
}

extern "C" int rn_pack_stem_weight_rs(const float* w_hwio, int R, int S, int Cout, void* w_packed, void* stream) {
  RN_CHECK_ARG(w_hwio && w_packed && Cout > 0 && R > 0 && S > 0 && S <= 8, "rn_pack_stem_weight_rs: bad argument");
  const int Cout_pad = rn_conv_cout_pad(Cout);
  hipLaunchKernelGGL(pack_stem_weight_kernel, dim3((Cout_pad * R * 32 + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, w_hwio, R, S, Cout, Cout_pad, (uint16_t*)w_packed);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

extern "C" int rn_pack_stem_weight(const float* w_hwio, int Cout, void* w_packed, void* stream) {
  return rn_pack_stem_weight_rs(w_hwio, 7, 7, Cout, w_packed, stream);
}

extern "C" int rn_stem_padded_width(int W) { return (int)rn_align_up((size_t)W + 6 + 2, 8); }

// images f32 [N,H,W,3] -> bf16 [N,H+6,Wp,4], zero border of 3 (fixed_padding for k=7) and zero
// 4th channel.  One thread per output pixel (8-byte store); reads are 12-byte pixels.
__global__ void __launch_bounds__(256)
pack_stem_input_kernel(const float* __restrict__ img, int N, int H, int W, int pad_top, int pad_left, int Hp,
                       int Wp, uint2* __restrict__ out) {
  const long long total = (long long)N * Hp * Wp;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int xp = (int)(i % Wp);
    const long long t = i / Wp;
    const int yp = (int)(t % Hp);
    const int n = (int)(t / Hp);
    const int x = xp - pad_left, y = yp - pad_top;
    uint2 o = make_uint2(0u, 0u);
    if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
      const float* p = img + (((long long)n * H + y) * W + x) * 3;
      o.x = rn_pack_bf16x2(p[0], p[1]);
      o.y = rn_pack_bf16x2(p[2], 0.0f);
    }
    out[i] = o;
  }
}

extern "C" int rn_pack_image_nhwc4(const float* images, int N, int H, int W, int pad_top, int pad_left, int Hp,
                                   int Wp, void* packed, void* stream) {
  RN_CHECK_ARG(images && packed && N > 0 && H > 0 && W > 0 && pad_top >= 0 && pad_left >= 0 &&
                   Hp >= H + pad_top && Wp >= W + pad_left && Wp % 8 == 0,
               "rn_pack_image_nhwc4: bad argument");
  const long long total = (long long)N * Hp * Wp;
  int blocks = (int)(rn_cdiv(total, 256) < 8192 ? rn_cdiv(total, 256) : 8192);
  hipLaunchKernelGGL(pack_stem_input_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, images, N, H, W,
                     pad_top, pad_left, Hp, Wp, (uint2*)packed);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

extern "C" int rn_pack_stem_input(const float* images, int N, int H, int W, void* packed, void* stream) {
  RN_CHECK_ARG(images && packed && N > 0 && H > 0 && W > 0, "rn_pack_stem_input: bad argument");
  return rn_pack_image_nhwc4(images, N, H, W, 3, 3, H + 6, rn_stem_padded_width(W), packed, stream);
}
