// rn_fusion.hip — K7, the weighted FeatureFusion modes of the FPN top-down path ('fast_attention': two learned scalars per
// fusion, 'fast_channel_attention': two learned per-channel vectors), forward and backward.  16-bit NHWC, 8 channels
// (16 bytes) per thread.  Mode 'sum' is rn_fpn_topdown / rn_fpn_topdown_bwd_level (rn_pool.hip, rn_train.hip), untouched.
// Reference: retinanet/model/layers/feature_fusion.py:41-56 (relu of the weights, + 1e-4, feature * weight / sum, Add),
//            retinanet/model/neck/fpn.py:71-98 (one FeatureFusion + activation per level below the top).
//
// The arithmetic is one rounding to the storage type per TF op (rnet_hip.h, K7).  Every op is evaluated in fp32 and
// rounded with rn_rb.  The products x * a are exact in fp32 (two operands of at most 11 significant bits).  The quotient
// is the correctly rounded fp32 division the build flags give `/`, NOT a product with a reciprocal.  Why: with half
// storage p and s carry 11 bits and a rounding midpoint m of the result carries 12, so a quotient p / s that is no
// midpoint can be as close to one as one unit of the 23-bit product m s, 2^-23 relative — the size of the error of
// p * fl(1 / s) in fp32, which could therefore land on the other side (with bfloat16's 8 bits the margin is 2^-17 and the
// reciprocal would do, but one code path serves both builds).  The correctly rounded quotient is safe in both: m is an
// fp32 value and |p / s - m| = |p - m s| / s is at least one unit of m s over s, more than 2^-11 of m's own unit, i.e.
// more than half an fp32 unit of m, so rounding to fp32 can neither reach nor cross m; an exact tie p = m s gives m
// exactly in fp32 and the second rounding breaks it to even as a single rounding would.
#include "rn_common.h"

#define FU_THREADS 256
#define RN_PYR_MAX 8
#define FU_MAX_PARTIALS 1024   // stage-1 rows of the weight-gradient reduction (workgroups along the pixels)
#define FU_FIN_ROWS 16         // stage 2: partial rows summed side by side per channel

struct bf8 { float v[8]; };
__device__ __forceinline__ bf8 unpack8(uint4 u) {
  bf8 r;
  r.v[0] = rn_bf16_to_f32((uint16_t)(u.x & 0xffffu)); r.v[1] = rn_bf16_to_f32((uint16_t)(u.x >> 16));
  r.v[2] = rn_bf16_to_f32((uint16_t)(u.y & 0xffffu)); r.v[3] = rn_bf16_to_f32((uint16_t)(u.y >> 16));
  r.v[4] = rn_bf16_to_f32((uint16_t)(u.z & 0xffffu)); r.v[5] = rn_bf16_to_f32((uint16_t)(u.z >> 16));
  r.v[6] = rn_bf16_to_f32((uint16_t)(u.w & 0xffffu)); r.v[7] = rn_bf16_to_f32((uint16_t)(u.w >> 16));
  return r;
}
__device__ __forceinline__ uint4 pack8(const bf8& r) {
  uint4 u;
  u.x = rn_pack_bf16x2(r.v[0], r.v[1]); u.y = rn_pack_bf16x2(r.v[2], r.v[3]);
  u.z = rn_pack_bf16x2(r.v[4], r.v[5]); u.w = rn_pack_bf16x2(r.v[6], r.v[7]);
  return u;
}
__device__ __forceinline__ bf8 load8f(const float* p) {
  const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
  return bf8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}

// ---- the coefficient block of one fusion ----------------------------------------------------------------------------
// [a_l | a_u | s] as storage values [3][C] (what the forward multiplies and divides by, 16 bytes per channel group),
// then [c_l | c_u] = a / s as f32 [2][C] (the backward's factors).  C % 8 == 0 keeps every part 16-byte aligned.
struct Coef {
  const uint4 *a_l, *a_u, *s;
  const float *c_l, *c_u;
};
__host__ __device__ __forceinline__ Coef coef_view(const void* base, int C) {
  const char* b = (const char*)base;
  return Coef{(const uint4*)b, (const uint4*)(b + 2 * (size_t)C), (const uint4*)(b + 4 * (size_t)C),
              (const float*)(b + 6 * (size_t)C), (const float*)(b + 10 * (size_t)C)};
}
extern "C" size_t rn_fpn_fusion_coef_bytes(int C) { return C > 0 ? 14 * (size_t)C : 0; }

struct FusionPrep {
  int F, C, mode;
  const float* wl[RN_PYR_MAX - 1];
  const float* wu[RN_PYR_MAX - 1];
  void* coef[RN_PYR_MAX - 1];
};
__global__ void __launch_bounds__(FU_THREADS) fusion_prepare_kernel(FusionPrep p) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.F * p.C) return;
  const int j = idx / p.C, c = idx - j * p.C;
  const int src = p.mode == RN_FUSION_FAST_ATTENTION ? 0 : c;
  const float a_l = rn_rb(fmaxf(p.wl[j][src], 0.0f)), a_u = rn_rb(fmaxf(p.wu[j][src], 0.0f));
  const float s = rn_rb(rn_rb(a_l + a_u) + rn_rb(1e-4f));
  uint16_t* h = (uint16_t*)p.coef[j];
  float* f = (float*)((char*)p.coef[j] + 6 * (size_t)p.C);
  h[c] = rn_f32_to_bf16(a_l);
  h[p.C + c] = rn_f32_to_bf16(a_u);
  h[2 * p.C + c] = rn_f32_to_bf16(s);
  f[c] = a_l / s;
  f[p.C + c] = a_u / s;
}

// ---- forward ------------------------------------------------------------------------------------------------------------
struct FusedPyramid {
  int L, N, H0, W0, C8, act;
  const uint4* in[RN_PYR_MAX];
  uint4* out[RN_PYR_MAX];
  const void* coef[RN_PYR_MAX - 1];
  long long begin[RN_PYR_MAX + 1];
};

static int fu_blocks(long long items) {
  long long b = rn_cdiv(items, FU_THREADS);
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

// One launch writes the levels [lo, hi), each thread walking its chain down from level hi, as fpn_topdown_kernel does.
// A stage is two products, two correctly rounded divisions (v_div_scale / v_rcp / v_fma chain / v_div_fmas / v_div_fixup,
// ~13 instructions each), an add and five roundings per element: the compiled kernel has 330 more VALU instructions per
// 16-byte group and stage than fpn_topdown_kernel (958 against 628 in all, index arithmetic included).  What rn_pool.hip
// says about re-evaluating the chain at training sizes therefore holds here with more force, and large pyramids are cut
// into launches of ONE stage per element by the same rule (fused_cuts); small ones (serving) stay one launch, where the
// launch latency is what the step costs.  The coefficients of a thread's own level — the only stage of a one-stage
// launch — stay in registers while its channel group does (always, when C / 8 divides the grid stride: every
// power-of-two channel count); the activation selector is wave-uniform and outside the element loop (rn_apply_act_n).
__global__ void __launch_bounds__(FU_THREADS) fpn_fused_kernel(FusedPyramid p, int lo, int hi) {
  const long long first = p.begin[lo], total = p.begin[hi];
  const uint4* __restrict__ src_hi = hi == p.L - 1 ? p.in[hi] : p.out[hi];
  const int C = p.C8 * 8;
  int own_key = -1;
  bf8 own_al, own_au, own_s;
  for (long long i = first + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int l = lo;
    while (i >= p.begin[l + 1]) ++l;
    const int Wl = p.W0 >> l, Hl = p.H0 >> l;
    const RnIdx4 d = rn_decode4(i - p.begin[l], p.C8, Wl, Hl, rn_decode_mode(total, p.C8));
    const int c = d.c, x = d.x, y = d.y, n = d.n;
    if (own_key != l * p.C8 + c) {
      const Coef cf = coef_view(p.coef[l], C);
      own_al = unpack8(cf.a_l[c]); own_au = unpack8(cf.a_u[c]); own_s = unpack8(cf.s[c]);
      own_key = l * p.C8 + c;
    }
    bf8 v = unpack8(src_hi[(((long long)n * (p.H0 >> hi)) + (y >> (hi - l))) * (p.W0 >> hi) * p.C8 +
                           (long long)(x >> (hi - l)) * p.C8 + c]);
    for (int k = hi - 1; k >= l; --k) {
      const int Hk = p.H0 >> k, Wk = p.W0 >> k;
      const bf8 u = unpack8(p.in[k][(((long long)n * Hk) + (y >> (k - l))) * Wk * p.C8 +
                                   (long long)(x >> (k - l)) * p.C8 + c]);
      bf8 al = own_al, au = own_au, s = own_s;
      if (k != l) {
        const Coef cf = coef_view(p.coef[k], C);
        al = unpack8(cf.a_l[c]); au = unpack8(cf.a_u[c]); s = unpack8(cf.s[c]);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float lower = rn_rb(rn_rb(u.v[q] * al.v[q]) / s.v[q]);
        const float upper = rn_rb(rn_rb(v.v[q] * au.v[q]) / s.v[q]);
        v.v[q] = rn_rb(lower + upper);
      }
      rn_apply_act_n<8>(v.v, p.act);
#pragma unroll
      for (int q = 0; q < 8; ++q) v.v[q] = rn_rb(v.v[q]);
    }
    p.out[l][(((long long)n * Hl) + y) * Wl * p.C8 + (long long)x * p.C8 + c] = pack8(v);
  }
}

static int fused_fill(FusedPyramid& p, void* const* in, void* const* out, int L, int N, int H0, int W0, int C) {
  if (L < 2 || L > RN_PYR_MAX || N <= 0 || H0 <= 0 || W0 <= 0 || C <= 0 || C % 8 != 0) return -1;
  if ((H0 >> (L - 1)) < 1 || (W0 >> (L - 1)) < 1) return -1;
  if ((H0 % (1 << (L - 1))) || (W0 % (1 << (L - 1)))) return -1;
  p.L = L; p.N = N; p.H0 = H0; p.W0 = W0; p.C8 = C / 8;
  p.begin[0] = 0;
  for (int l = 0; l < L; ++l) {
    p.in[l] = in ? (const uint4*)in[l] : nullptr;
    p.out[l] = out ? (uint4*)out[l] : nullptr;
    p.begin[l + 1] = p.begin[l] + (long long)N * (H0 >> l) * (W0 >> l) * (C / 8);
  }
  return 0;
}

// the launch cuts of rn_fpn_topdown: one launch for small pyramids (serving: launch latency is what they cost), from 2^21
// 16-byte items on the finest level the two finest levels as one-stage launches behind one launch for the coarse rest
static int fused_cuts(const FusedPyramid& p, int cuts[4]) {
  int ncuts = 0;
  if (p.L >= 3 && p.begin[1] >= (1ll << 21)) {
    if (p.L > 3) cuts[ncuts++] = p.L - 1;
    cuts[ncuts++] = 2;
    cuts[ncuts++] = 1;
  } else {
    cuts[ncuts++] = p.L - 1;
  }
  return ncuts;
}

extern "C" int rn_fpn_topdown_fused_launches(int num_levels, int N, int H0, int W0, int C) {
  FusedPyramid p;
  int cuts[4];
  if (fused_fill(p, nullptr, nullptr, num_levels, N, H0, W0, C) != 0) return 0;
  return fused_cuts(p, cuts);
}

extern "C" int rn_fpn_topdown_fused(void* const* p_in, void* const* p_out, const float* const* w_lower,
                                    const float* const* w_upper, void* const* coef, int num_levels, int N, int H0,
                                    int W0, int C, int act, int mode, void* stream) {
  FusedPyramid p;
  RN_CHECK_ARG(p_in && p_out && fused_fill(p, p_in, p_out, num_levels, N, H0, W0, C) == 0,
               "rn_fpn_topdown_fused: bad pyramid (levels must halve exactly, C %% 8 == 0)");
  RN_CHECK_ARG(w_lower && w_upper && coef, "rn_fpn_topdown_fused: null weight / coefficient array");
  RN_CHECK_ARG(mode == RN_FUSION_FAST_ATTENTION || mode == RN_FUSION_FAST_CHANNEL_ATTENTION,
               "rn_fpn_topdown_fused: mode %d is neither fast_attention nor fast_channel_attention", mode);
  RN_CHECK_ARG(act >= RN_ACT_NONE && act <= RN_ACT_SWISH, "rn_fpn_topdown_fused: bad activation %d", act);
  FusionPrep fp;
  fp.F = num_levels - 1; fp.C = C; fp.mode = mode;
  for (int l = 0; l < num_levels; ++l)
    RN_CHECK_ARG(p.in[l] && p.out[l], "rn_fpn_topdown_fused: null level %d", l);
  for (int j = 0; j < num_levels - 1; ++j) {
    RN_CHECK_ARG(w_lower[j] && w_upper[j] && coef[j] && ((uintptr_t)coef[j] & 15) == 0,
                 "rn_fpn_topdown_fused: fusion %d: null weights or coefficient block (16-byte aligned)", j);
    fp.wl[j] = w_lower[j]; fp.wu[j] = w_upper[j]; fp.coef[j] = coef[j];
    p.coef[j] = coef[j];
  }
  p.act = act;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fusion_prepare_kernel, dim3((unsigned)rn_cdiv((long long)fp.F * C, FU_THREADS)), dim3(FU_THREADS), 0,
                     st, fp);
  RN_CHECK_LAUNCH();
  int cuts[4];
  const int ncuts = fused_cuts(p, cuts);
  for (int q = 0; q < ncuts; ++q) {
    const int hi = cuts[q], lo = q + 1 < ncuts ? cuts[q + 1] : 0;
    hipLaunchKernelGGL(fpn_fused_kernel, dim3(fu_blocks(p.begin[hi] - p.begin[lo])), dim3(FU_THREADS), 0, st, p, lo, hi);
    RN_CHECK_LAUNCH();
  }
  return RN_OK;
}

// ---- backward, one level ------------------------------------------------------------------------------------------------
// A workgroup is PR pixels x CB channel groups (CB = min(C / 8, 256), PR = 256 / CB; consecutive threads read consecutive
// 16 bytes) and walks the pixels with a stride of gridDim.x * PR: a thread keeps ONE channel group, so it reads its
// coefficients once and carries its 16 sums (8 channels x {Sl, Su}) in registers, in pixel order.  The PR partial sums of a
// channel are then added by a fixed tree in LDS and the workgroup writes one [2][C] row: nothing depends on timing.
struct FusedBwd {
  const uint4* dout;
  const uint4* g_finer;
  const float* cu_finer;
  const uint4* out;
  const uint4* in_lower;
  const uint4* out_upper;
  const float* c_l;
  uint4* g;
  uint4* din;
  float* partial;
  int N, H, W, C8, act, CB, PR;
};

__device__ __forceinline__ float gate01(float z, int act) {
  if (act == RN_ACT_RELU) return z > 0.0f ? 1.0f : 0.0f;
  if (act == RN_ACT_RELU6) return (z > 0.0f && z < 6.0f) ? 1.0f : 0.0f;
  return 1.0f;
}

__global__ void __launch_bounds__(FU_THREADS) fpn_fused_bwd_kernel(FusedBwd a) {
  __shared__ float red[16 * FU_THREADS];
  const int tid = threadIdx.x, cl = tid % a.CB, pr = tid / a.CB;
  const int cg = blockIdx.y * a.CB + cl;
  const bool live = pr < a.PR && cg < a.C8;
  const bool top = a.g == nullptr;            // the coarsest level: no gate, no fusion weights below its output
  const long long P = (long long)a.N * a.H * a.W;
  float sl[8], su[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) sl[q] = su[q] = 0.0f;
  if (live) {
    bf8 cuf, clo;
#pragma unroll
    for (int q = 0; q < 8; ++q) cuf.v[q] = clo.v[q] = 0.0f;
    if (a.g_finer) cuf = load8f(a.cu_finer + 8 * cg);
    if (!top) clo = load8f(a.c_l + 8 * cg);
    const int mode = rn_decode_mode(P, 1);
    const int H2 = a.H >> 1, W2 = a.W >> 1;
    for (long long pix = (long long)blockIdx.x * a.PR + pr; pix < P; pix += (long long)gridDim.x * a.PR) {
      const RnIdx4 d = rn_decode4(pix, 1, a.W, a.H, mode);
      const int x = d.x, y = d.y, n = d.n;
      const long long i = pix * a.C8 + cg;
      bf8 t = unpack8(a.dout[i]);
      if (a.g_finer) {
        bf8 s4;
#pragma unroll
        for (int q = 0; q < 8; ++q) s4.v[q] = 0.0f;
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx) {
            const bf8 v =
                unpack8(a.g_finer[(((long long)n * 2 * a.H + 2 * y + dy) * 2 * a.W + 2 * x + dx) * a.C8 + cg]);
#pragma unroll
            for (int q = 0; q < 8; ++q) s4.v[q] += v.v[q];
          }
#pragma unroll
        for (int q = 0; q < 8; ++q) t.v[q] += cuf.v[q] * s4.v[q];
      }
      if (top) {
        a.din[i] = pack8(t);
        continue;
      }
      if (a.out && a.act != RN_ACT_NONE) {
        const bf8 z = unpack8(a.out[i]);
#pragma unroll
        for (int q = 0; q < 8; ++q) t.v[q] *= gate01(z.v[q], a.act);
      }
      const uint4 gp = pack8(t);
      a.g[i] = gp;
      const bf8 gs = unpack8(gp);   // the STORED g: what din and the sums are taken over
      bf8 dd;
#pragma unroll
      for (int q = 0; q < 8; ++q) dd.v[q] = clo.v[q] * gs.v[q];
      a.din[i] = pack8(dd);
      const bf8 xl = unpack8(a.in_lower[i]);
      const bf8 xu = unpack8(a.out_upper[(((long long)n * H2 + (y >> 1)) * W2 + (x >> 1)) * a.C8 + cg]);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        sl[q] += gs.v[q] * xl.v[q];
        su[q] += gs.v[q] * xu.v[q];
      }
    }
  }
  if (top) return;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    red[q * FU_THREADS + tid] = sl[q];
    red[(8 + q) * FU_THREADS + tid] = su[q];
  }
  __syncthreads();
  for (int n = a.PR; n > 1;) {
    const int h = (n + 1) >> 1;
    if (pr < (n >> 1)) {   // pr + h < n <= PR: the partner is inside the live part of the workgroup
#pragma unroll
      for (int q = 0; q < 16; ++q) red[q * FU_THREADS + tid] += red[q * FU_THREADS + tid + h * a.CB];
    }
    __syncthreads();
    n = h;
  }
  if (pr == 0 && cg < a.C8) {
    const int C = a.C8 * 8;
    float* row = a.partial + (long long)blockIdx.x * 2 * C;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      row[cg * 8 + q] = red[q * FU_THREADS + tid];
      row[C + cg * 8 + q] = red[(8 + q) * FU_THREADS + tid];
    }
  }
}

struct BwdGeom { int CB, PR, gx, gy; };
static BwdGeom bwd_geom(int N, int H, int W, int C) {
  BwdGeom g;
  const int C8 = C / 8;
  g.CB = C8 < FU_THREADS ? C8 : FU_THREADS;
  g.PR = FU_THREADS / g.CB;
  g.gy = (int)rn_cdiv(C8, g.CB);
  long long b = rn_cdiv((long long)N * H * W, g.PR);
  g.gx = (int)(b > FU_MAX_PARTIALS ? FU_MAX_PARTIALS : b);
  return g;
}
// stage-1 rows [gx][2][C], then the finalised per-channel sums [2][C]
extern "C" size_t rn_fpn_fused_bwd_workspace_bytes(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0) return 0;
  return ((size_t)bwd_geom(N, H, W, C).gx + 1) * 2 * (size_t)C * sizeof(float);
}

extern "C" int rn_fpn_fused_bwd_level(const void* dout, const void* g_finer, const void* coef_finer, const void* out,
                                      const void* in_lower, const void* out_upper, const void* coef, void* g, void* din,
                                      void* workspace, size_t workspace_bytes, int N, int H, int W, int C, int act,
                                      void* stream) {
  RN_CHECK_ARG(dout && din && C > 0 && C % 8 == 0 && N > 0 && H > 0 && W > 0, "rn_fpn_fused_bwd_level: bad argument");
  RN_CHECK_ARG(!(out && act == RN_ACT_SWISH),
               "rn_fpn_fused_bwd_level: swish' needs the pre-activation sum, which is not an argument (only out is)");
  RN_CHECK_ARG(!g_finer == !coef_finer, "rn_fpn_fused_bwd_level: g_finer and coef_finer go together");
  const bool top = !g;
  if (top) {
    RN_CHECK_ARG(!in_lower && !out_upper && !coef && g_finer,
                 "rn_fpn_fused_bwd_level: the top level takes g_finer / coef_finer and no fusion of its own");
  } else {
    RN_CHECK_ARG(in_lower && out_upper && coef && workspace, "rn_fpn_fused_bwd_level: null argument");
    RN_CHECK_ARG(H % 2 == 0 && W % 2 == 0, "rn_fpn_fused_bwd_level: %d x %d does not halve exactly", H, W);
    RN_CHECK_ARG(din != g && din != dout, "rn_fpn_fused_bwd_level: din aliases g / dout");
    if (workspace_bytes < rn_fpn_fused_bwd_workspace_bytes(N, H, W, C)) {
      rn_set_error("rn_fpn_fused_bwd_level: workspace of %zu bytes, %zu needed", workspace_bytes,
                   rn_fpn_fused_bwd_workspace_bytes(N, H, W, C));
      return RN_ENOMEM;
    }
  }
  const BwdGeom ge = bwd_geom(N, H, W, C);
  FusedBwd a;
  a.dout = (const uint4*)dout; a.g_finer = (const uint4*)g_finer;
  a.cu_finer = coef_finer ? coef_view(coef_finer, C).c_u : nullptr;
  a.out = (const uint4*)out; a.in_lower = (const uint4*)in_lower; a.out_upper = (const uint4*)out_upper;
  a.c_l = coef ? coef_view(coef, C).c_l : nullptr;
  a.g = (uint4*)g; a.din = (uint4*)din; a.partial = (float*)workspace;
  a.N = N; a.H = H; a.W = W; a.C8 = C / 8; a.act = act; a.CB = ge.CB; a.PR = ge.PR;
  hipLaunchKernelGGL(fpn_fused_bwd_kernel, dim3(ge.gx, ge.gy), dim3(FU_THREADS), 0, (hipStream_t)stream, a);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

// ---- backward, stage 2 ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fusion_dw(float Sl, float Su, float a_l, float a_u, float s, float w_l, float w_u,
                                          float* dw_l, float* dw_u) {
  const float s2 = s * s;
  const float da_l = (Sl * (s - a_l) - Su * a_u) / s2, da_u = (Su * (s - a_u) - Sl * a_l) / s2;
  *dw_l = w_l > 0.0f ? da_l : 0.0f;
  *dw_u = w_u > 0.0f ? da_u : 0.0f;
}
__device__ __forceinline__ float h16_at(const uint4* p, int c) { return rn_bf16_to_f32(((const uint16_t*)p)[c]); }

// 16 channels per workgroup; 16 threads per channel add every 16th stage-1 row in row order, then a fixed tree
__global__ void __launch_bounds__(FU_THREADS)
fusion_finalize_kernel(const float* __restrict__ partial, int rows, int C, Coef cf, const float* __restrict__ w_l,
                       const float* __restrict__ w_u, int mode, float* __restrict__ sums_ws, float* sums,
                       float* dw_l, float* dw_u) {
  __shared__ float red[2 * FU_THREADS];
  const int tid = threadIdx.x, cl = tid % 16, r = tid / 16;
  const int c = blockIdx.x * 16 + cl;      // C % 8 == 0: the last workgroup may have 8 idle channels
  float sl = 0.0f, su = 0.0f;
  if (c < C)
    for (int b = r; b < rows; b += FU_FIN_ROWS) {
      sl += partial[(long long)b * 2 * C + c];
      su += partial[(long long)b * 2 * C + C + c];
    }
  red[tid] = sl;
  red[FU_THREADS + tid] = su;
  __syncthreads();
  for (int h = FU_FIN_ROWS / 2; h > 0; h >>= 1) {
    if (r < h) {
      red[tid] += red[tid + h * 16];
      red[FU_THREADS + tid] += red[FU_THREADS + tid + h * 16];
    }
    __syncthreads();
  }
  if (r == 0 && c < C) {
    const float Sl = red[tid], Su = red[FU_THREADS + tid];
    sums_ws[c] = Sl;
    sums_ws[C + c] = Su;
    if (sums) {
      sums[c] = Sl;
      sums[C + c] = Su;
    }
    if (mode == RN_FUSION_FAST_CHANNEL_ATTENTION)
      fusion_dw(Sl, Su, h16_at(cf.a_l, c), h16_at(cf.a_u, c), h16_at(cf.s, c), w_l[c], w_u[c], dw_l + c, dw_u + c);
  }
}
// fast_attention: the per-channel sums added over the channels (thread t: channels t, t + 256, .. in order, then a tree)
__global__ void __launch_bounds__(FU_THREADS)
fusion_finalize_scalar_kernel(const float* __restrict__ sums_ws, int C, Coef cf, const float* __restrict__ w_l,
                              const float* __restrict__ w_u, float* dw_l, float* dw_u) {
  __shared__ float red[2 * FU_THREADS];
  const int tid = threadIdx.x;
  float sl = 0.0f, su = 0.0f;
  for (int c = tid; c < C; c += FU_THREADS) {
    sl += sums_ws[c];
    su += sums_ws[C + c];
  }
  red[tid] = sl;
  red[FU_THREADS + tid] = su;
  __syncthreads();
  for (int h = FU_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      red[tid] += red[tid + h];
      red[FU_THREADS + tid] += red[FU_THREADS + tid + h];
    }
    __syncthreads();
  }
  if (tid == 0)
    fusion_dw(red[0], red[FU_THREADS], h16_at(cf.a_l, 0), h16_at(cf.a_u, 0), h16_at(cf.s, 0), w_l[0], w_u[0], dw_l, dw_u);
}

extern "C" int rn_fpn_fused_bwd_finalize(void* workspace, size_t workspace_bytes, int N, int H, int W, int C,
                                         const float* w_lower, const float* w_upper, const void* coef, int mode,
                                         float* sums, float* dw_lower, float* dw_upper, void* stream) {
  RN_CHECK_ARG(workspace && w_lower && w_upper && coef && dw_lower && dw_upper && C > 0 && C % 8 == 0 && N > 0 &&
                   H > 0 && W > 0, "rn_fpn_fused_bwd_finalize: bad argument");
  RN_CHECK_ARG(mode == RN_FUSION_FAST_ATTENTION || mode == RN_FUSION_FAST_CHANNEL_ATTENTION,
               "rn_fpn_fused_bwd_finalize: mode %d is neither fast_attention nor fast_channel_attention", mode);
  if (workspace_bytes < rn_fpn_fused_bwd_workspace_bytes(N, H, W, C)) {
    rn_set_error("rn_fpn_fused_bwd_finalize: workspace of %zu bytes, %zu needed", workspace_bytes,
                 rn_fpn_fused_bwd_workspace_bytes(N, H, W, C));
    return RN_ENOMEM;
  }
  const int rows = bwd_geom(N, H, W, C).gx;
  float* partial = (float*)workspace;
  float* sums_ws = partial + (size_t)rows * 2 * C;
  const Coef cf = coef_view(coef, C);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fusion_finalize_kernel, dim3((unsigned)rn_cdiv(C, 16)), dim3(FU_THREADS), 0, st, partial, rows, C,
                     cf, w_lower, w_upper, mode, sums_ws, sums, dw_lower, dw_upper);
  RN_CHECK_LAUNCH();
  if (mode == RN_FUSION_FAST_ATTENTION) {
    hipLaunchKernelGGL(fusion_finalize_scalar_kernel, dim3(1), dim3(FU_THREADS), 0, st, sums_ws, C, cf, w_lower, w_upper,
                       dw_lower, dw_upper);
    RN_CHECK_LAUNCH();
  }
  return RN_OK;
}
