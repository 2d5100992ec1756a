// rn_conv_i8.hip — INT8 serving of the detection heads (include/rnet_hip.h, DESIGN.md "INT8 serving"):
// the 3x3 convolution on v_mfma_i32_32x32x32_i8, the weight packer, the activation quantiser and the two calibration
// statistics.  Symmetric quantisation throughout: int8 0 is the real 0, so zero padding is the value 0.
#include "rn_common.h"

typedef int rn_i32x4 __attribute__((ext_vector_type(4)));
typedef int rn_i32x16 __attribute__((ext_vector_type(16)));

// ---- convolution ---------------------------------------------------------------------------------------------------
// Implicit GEMM: a workgroup (4 waves) owns 128 output pixels (linear over [N,H,W]) x 64*NB output channels and walks
// K = 9 taps x Cin in steps of 64 bytes.  Per step the 128 x 64 pixel bytes (the tap's shifted pixels, zeros outside
// the map) and the 64*NB x 64 weight bytes go through LDS; the next step's global loads are issued before the MFMAs of
// the current one.  The weights are the MFMA's A operand (rows = output channels), the pixels its B operand (columns),
// so a lane ends up with ONE pixel and groups of four consecutive channels: rows (reg & 3) + 8 * (reg >> 2) + 4 * (lane
// >> 5) — packed stores.  Both operands take k = 16 * (lane >> 5) + byte of the lane's 16 bytes.
#define I8_BM 128
#define I8_LD 80   // LDS row pitch in bytes: 64 data + 16 pad (keeps 16-byte alignment, spreads rows over the banks)

struct I8Seg {
  const int8_t* x;
  const int8_t* w;
  void* y;
  const float* mul;
  const float* add;
  float out_inv_scale;
  int N, H, W, Cin, Cout;
  int M;          // N * H * W
  int m_tiles;    // ceil(M / 128)
  int tile_begin; // first workgroup of this segment
};
struct I8Params {
  I8Seg seg[RN_CONV_MAX_SEGMENTS];
  int num_segments, act, out_f32;
};

template <int NB>
__global__ __launch_bounds__(256) void conv3x3_i8_kernel(const I8Params P) {
  constexpr int BN = 64 * NB;
  __shared__ __attribute__((aligned(16))) int8_t Ws[BN * I8_LD];
  __shared__ __attribute__((aligned(16))) int8_t Xs[I8_BM * I8_LD];

  int si = 0;
#pragma unroll 1
  for (int i = 1; i < P.num_segments; ++i)
    if ((int)blockIdx.x >= P.seg[i].tile_begin) si = i;
  const I8Seg& S = P.seg[si];
  const int local = (int)blockIdx.x - S.tile_begin;
  const int n_tile = local / S.m_tiles;
  const int m0 = (local - n_tile * S.m_tiles) * I8_BM;
  const int n0 = n_tile * BN;
  const int H = S.H, W = S.W, Cin = S.Cin, M = S.M;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = tid >> 2, lchunk = (tid & 3) * 16;
  // the two pixels this thread stages, and its weight rows
  int py[2], px[2];
  long long pimg[2];   // pixel index of (n, 0, 0)
  bool pin[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = m0 + lrow + 64 * i;
    pin[i] = p < M;
    const int q = pin[i] ? p : 0;
    const int n = q / (H * W);
    const int rem = q - n * (H * W);
    py[i] = rem / W;
    px[i] = rem - py[i] * W;
    pimg[i] = (long long)n * H * W;
  }
  const int kc = Cin >> 6;
  const int steps = 9 * kc;

  rn_i32x4 rx[2], rw[NB];
  auto gload = [&](int step) {
    const int tap = step / kc, cc = step - tap * kc;
    const int r = tap / 3, s = tap - r * 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int yy = py[i] + r - 1, xx = px[i] + s - 1;
      const bool ok = pin[i] && yy >= 0 && yy < H && xx >= 0 && xx < W;
      rx[i] = rn_i32x4{0, 0, 0, 0};
      if (ok) rx[i] = *(const rn_i32x4*)(S.x + ((pimg[i] + (long long)yy * W + xx) * Cin + cc * 64 + lchunk));
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)   // packed rows reach the next multiple of 128 channels: always in bounds
      rw[i] = *(const rn_i32x4*)(S.w + (((long long)(n0 + lrow + 64 * i) * 9 + tap) * Cin + cc * 64 + lchunk));
  };

  rn_i32x16 acc[NB][2];
#pragma unroll
  for (int a = 0; a < NB; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0;

  const int wp = wave & 1, wc = wave >> 1;   // the wave's 64 pixels and 32*NB channels
  const int frow = lane & 31, fk = 16 * (lane >> 5);
  gload(0);
#pragma unroll 1
  for (int step = 0; step < steps; ++step) {
    __syncthreads();   // the MFMAs of the previous step have read the tiles
#pragma unroll
    for (int i = 0; i < 2; ++i) *(rn_i32x4*)(Xs + (lrow + 64 * i) * I8_LD + lchunk) = rx[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) *(rn_i32x4*)(Ws + (lrow + 64 * i) * I8_LD + lchunk) = rw[i];
    __syncthreads();
    if (step + 1 < steps) gload(step + 1);
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      rn_i32x4 fa[NB], fb[2];
#pragma unroll
      for (int a = 0; a < NB; ++a) fa[a] = *(const rn_i32x4*)(Ws + (wc * 32 * NB + 32 * a + frow) * I8_LD + kh * 32 + fk);
#pragma unroll
      for (int b = 0; b < 2; ++b) fb[b] = *(const rn_i32x4*)(Xs + (wp * 64 + 32 * b + frow) * I8_LD + kh * 32 + fk);
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
  }

  // epilogue: three separately rounded fp32 steps (the build has -ffp-contract=off), activation, output
  const int Cout = S.Cout, act = P.act;
  const float inv = S.out_inv_scale;
  const bool vec = (Cout & 3) == 0 && (((uintptr_t)S.y) & 15) == 0;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int p = m0 + wp * 64 + 32 * b + frow;
    if (p >= M) continue;
#pragma unroll
    for (int a = 0; a < NB; ++a) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = n0 + wc * 32 * NB + 32 * a + 8 * g + 4 * (lane >> 5);
        if (c0 >= Cout) continue;
        float t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = c0 + e < Cout ? c0 + e : Cout - 1;
          float v = (float)acc[a][b][4 * g + e] * S.mul[c];
          t[e] = v + S.add[c];
        }
        rn_apply_act_n<4>(t, act);
        const long long o = (long long)p * Cout + c0;
        if (P.out_f32) {
          float* y = (float*)S.y + o;
          if (vec) {
            *(float4*)y = float4{t[0], t[1], t[2], t[3]};
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c0 + e < Cout) y[e] = t[e];
          }
        } else {
          int q[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) q[e] = (int)fminf(fmaxf(rintf(t[e] * inv), -127.0f), 127.0f);
          int8_t* y = (int8_t*)S.y + o;
          if (vec) {
            *(uint32_t*)y = (uint32_t)(q[0] & 255) | ((uint32_t)(q[1] & 255) << 8) | ((uint32_t)(q[2] & 255) << 16) |
                            ((uint32_t)(q[3] & 255) << 24);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c0 + e < Cout) y[e] = (int8_t)q[e];
          }
        }
      }
    }
  }
}

extern "C" size_t rn_conv_i8_weight_bytes(int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0) return 0;
  return (size_t)rn_cdiv(Cout, 128) * 128 * 9 * (size_t)Cin;
}

extern "C" int rn_conv3x3_i8_fwd(const rn_conv_i8_problem* pr, void* stream) {
  RN_CHECK_ARG(pr != nullptr, "rn_conv3x3_i8_fwd: null problem");
  RN_CHECK_ARG(pr->num_segments >= 1 && pr->num_segments <= RN_CONV_MAX_SEGMENTS, "rn_conv3x3_i8_fwd: num_segments %d",
               pr->num_segments);
  RN_CHECK_ARG(pr->act == RN_ACT_NONE || pr->act == RN_ACT_RELU || pr->act == RN_ACT_RELU6,
               "rn_conv3x3_i8_fwd: activation %d (none, relu and relu6 only)", pr->act);
  RN_CHECK_ARG(pr->out_dtype == RN_DT_I8 || pr->out_dtype == RN_DT_F32, "rn_conv3x3_i8_fwd: out_dtype %d", pr->out_dtype);
  I8Params P;
  P.num_segments = pr->num_segments;
  P.act = pr->act;
  P.out_f32 = pr->out_dtype == RN_DT_F32;
  int max_cout = 0;
  for (int i = 0; i < pr->num_segments; ++i) max_cout = pr->seg[i].Cout > max_cout ? pr->seg[i].Cout : max_cout;
  const int BN = max_cout <= 64 ? 64 : 128;
  long long tiles = 0;
  for (int i = 0; i < pr->num_segments; ++i) {
    const rn_conv_i8_segment& s = pr->seg[i];
    RN_CHECK_ARG(s.x && s.w && s.y && s.mul && s.add, "rn_conv3x3_i8_fwd: segment %d has a null pointer", i);
    RN_CHECK_ARG((((uintptr_t)s.x) & 15) == 0 && (((uintptr_t)s.w) & 15) == 0,
                 "rn_conv3x3_i8_fwd: segment %d: x and w must be 16-byte aligned", i);
    RN_CHECK_ARG(s.N >= 1 && s.H >= 1 && s.W >= 1 && s.Cout >= 1, "rn_conv3x3_i8_fwd: segment %d: shape", i);
    RN_CHECK_ARG(s.Cin % 64 == 0 && s.Cin >= 64 && s.Cin <= 512,
                 "rn_conv3x3_i8_fwd: segment %d: Cin %d (a multiple of 64 in [64, 512])", i, s.Cin);
    const long long M = (long long)s.N * s.H * s.W;
    RN_CHECK_ARG(M < (1ll << 30), "rn_conv3x3_i8_fwd: segment %d: %lld pixels", i, M);
    if (pr->out_dtype == RN_DT_F32) RN_CHECK_ARG((((uintptr_t)s.y) & 3) == 0, "rn_conv3x3_i8_fwd: segment %d: y alignment", i);
    I8Seg& d = P.seg[i];
    d.x = (const int8_t*)s.x;
    d.w = (const int8_t*)s.w;
    d.y = s.y;
    d.mul = s.mul;
    d.add = s.add;
    d.out_inv_scale = s.out_inv_scale;
    d.N = s.N; d.H = s.H; d.W = s.W; d.Cin = s.Cin; d.Cout = s.Cout;
    d.M = (int)M;
    d.m_tiles = (int)rn_cdiv(M, I8_BM);
    d.tile_begin = (int)tiles;
    tiles += (long long)d.m_tiles * rn_cdiv(s.Cout, BN);
    RN_CHECK_ARG(tiles < (1ll << 30), "rn_conv3x3_i8_fwd: too many tiles");
  }
  hipStream_t st = (hipStream_t)stream;
  if (BN == 64)
    hipLaunchKernelGGL(conv3x3_i8_kernel<1>, dim3((unsigned)tiles), dim3(256), 0, st, P);
  else
    hipLaunchKernelGGL(conv3x3_i8_kernel<2>, dim3((unsigned)tiles), dim3(256), 0, st, P);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

// ---- weight packing ------------------------------------------------------------------------------------------------
// one workgroup per packed row (output channel; rows >= Cout are zero): max |w| of the row, then the quantised bytes
__global__ __launch_bounds__(256) void pack_w_i8_kernel(const float* __restrict__ w, int ohwi, int Cin, int Cout,
                                                        int8_t* __restrict__ out, float* __restrict__ w_scale) {
  const int c = blockIdx.x, K = 9 * Cin;
  int8_t* row = out + (long long)c * K;
  if (c >= Cout) {
    for (int k = threadIdx.x; k < K; k += 256) row[k] = 0;
    return;
  }
  // element k = tap * Cin + ci
  auto at = [&](int k) { return ohwi ? w[(long long)c * K + k] : w[(long long)k * Cout + c]; };
  float m = 0.0f;
  for (int k = threadIdx.x; k < K; k += 256) m = fmaxf(m, fabsf(at(k)));
  __shared__ float red[256];
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  m = red[0];
  const float sc = m > 0.0f ? m / 127.0f : 1.0f;
  if (threadIdx.x == 0) w_scale[c] = sc;
  for (int k = threadIdx.x; k < K; k += 256) row[k] = (int8_t)(int)fminf(fmaxf(rintf(at(k) / sc), -127.0f), 127.0f);
}

extern "C" int rn_pack_conv_weight_i8(const float* w, int layout_ohwi, int Cin, int Cout, void* w_packed, float* w_scale,
                                      void* stream) {
  RN_CHECK_ARG(w && w_packed && w_scale, "rn_pack_conv_weight_i8: null pointer");
  RN_CHECK_ARG(Cin >= 1 && Cout >= 1 && (long long)9 * Cin * Cout < (1ll << 31), "rn_pack_conv_weight_i8: Cin %d Cout %d", Cin,
               Cout);
  const int rows = (int)rn_cdiv(Cout, 128) * 128;
  hipLaunchKernelGGL(pack_w_i8_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, w, layout_ohwi ? 1 : 0, Cin, Cout,
                     (int8_t*)w_packed, w_scale);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

// ---- activation quantiser --------------------------------------------------------------------------------------------
struct QSeg {
  const uint16_t* x;
  int8_t* y;
  long long total;   // pixels * C
  long long begin;   // first element of this segment in the launch's flat index
  int C, pix_stride;
  float inv_scale;
};
struct QParams {
  QSeg seg[RN_CONV_MAX_SEGMENTS];
  int num_segments;
  long long total;
};

__global__ __launch_bounds__(256) void quantize_i8_kernel(const QParams P) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < P.total; t += stride) {
    int si = 0;
    for (int i = 1; i < P.num_segments; ++i)
      if (t >= P.seg[i].begin) si = i;
    const QSeg& S = P.seg[si];
    const long long e = t - S.begin;
    const long long pix = e / S.C;
    const int c = (int)(e - pix * S.C);
    const float v = rn_bf16_to_f32(S.x[pix * S.pix_stride + c]);
    S.y[e] = (int8_t)(int)fminf(fmaxf(rintf(v * S.inv_scale), -127.0f), 127.0f);
  }
}

extern "C" int rn_quantize_i8(const rn_quant_problem* pr, void* stream) {
  RN_CHECK_ARG(pr != nullptr, "rn_quantize_i8: null problem");
  RN_CHECK_ARG(pr->num_segments >= 1 && pr->num_segments <= RN_CONV_MAX_SEGMENTS, "rn_quantize_i8: num_segments %d",
               pr->num_segments);
  QParams P;
  P.num_segments = pr->num_segments;
  long long total = 0;
  for (int i = 0; i < pr->num_segments; ++i) {
    const rn_quant_segment& s = pr->seg[i];
    RN_CHECK_ARG(s.x && s.y, "rn_quantize_i8: segment %d has a null pointer", i);
    RN_CHECK_ARG(s.pixels >= 1 && s.C >= 1 && s.pix_stride >= s.C, "rn_quantize_i8: segment %d: shape", i);
    QSeg& d = P.seg[i];
    d.x = (const uint16_t*)s.x;
    d.y = (int8_t*)s.y;
    d.total = (long long)s.pixels * s.C;
    d.begin = total;
    d.C = s.C;
    d.pix_stride = s.pix_stride;
    d.inv_scale = s.inv_scale;
    total += d.total;
  }
  P.total = total;
  const long long blocks = rn_cdiv(total, 256 * 4);
  hipLaunchKernelGGL(quantize_i8_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks)), dim3(256), 0,
                     (hipStream_t)stream, P);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

// ---- calibration statistics ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void calib_absmax_kernel(const uint16_t* __restrict__ x, long long total, int C, int pix_stride,
                                                           unsigned* __restrict__ amax_bits) {
  const long long stride = (long long)gridDim.x * 256;
  float m = 0.0f;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const long long pix = t / C;
    const float v = fabsf(rn_bf16_to_f32(x[pix * pix_stride + (t - pix * C)]));
    m = v > m ? v : m;   // a NaN never enters
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  // non-negative floats order like their bit patterns
  if ((threadIdx.x & 63) == 0) atomicMax(amax_bits, __float_as_uint(m));
}

extern "C" int rn_calib_absmax(const void* x, int64_t pixels, int C, int pix_stride, float* amax, void* stream) {
  RN_CHECK_ARG(x && amax, "rn_calib_absmax: null pointer");
  RN_CHECK_ARG(pixels >= 1 && C >= 1 && pix_stride >= C, "rn_calib_absmax: shape");
  const long long total = (long long)pixels * C;
  const long long blocks = rn_cdiv(total, 256 * 8);
  hipLaunchKernelGGL(calib_absmax_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)x, total, C, pix_stride, (unsigned*)amax);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

__global__ __launch_bounds__(256) void calib_histogram_kernel(const uint16_t* __restrict__ x, long long total, int C, int pix_stride,
                                                              float bins_per_unit, unsigned long long* __restrict__ counts) {
  __shared__ unsigned h[RN_CALIB_BINS];
  for (int i = threadIdx.x; i < RN_CALIB_BINS; i += 256) h[i] = 0;
  __syncthreads();
  const long long stride = (long long)gridDim.x * 256;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const long long pix = t / C;
    const float v = fabsf(rn_bf16_to_f32(x[pix * pix_stride + (t - pix * C)]));
    const float f = fminf(v * bins_per_unit, (float)(RN_CALIB_BINS - 1));   // (a NaN lands in the last bin)
    int b = (int)f;
    b = b < 0 ? 0 : b > RN_CALIB_BINS - 1 ? RN_CALIB_BINS - 1 : b;
    atomicAdd(&h[b], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < RN_CALIB_BINS; i += 256)
    if (h[i]) atomicAdd(&counts[i], (unsigned long long)h[i]);
}

extern "C" int rn_calib_histogram(const void* x, int64_t pixels, int C, int pix_stride, float range, int64_t* counts,
                                  void* stream) {
  RN_CHECK_ARG(x && counts, "rn_calib_histogram: null pointer");
  RN_CHECK_ARG(pixels >= 1 && C >= 1 && pix_stride >= C, "rn_calib_histogram: shape");
  RN_CHECK_ARG(range > 0.0f && range < __builtin_huge_valf(), "rn_calib_histogram: range %g", (double)range);
  const long long total = (long long)pixels * C;
  // each block's LDS bins are 32-bit: at most 2^20 elements per block
  long long blocks = rn_cdiv(total, 256 * 16);
  blocks = blocks > 4096 ? 4096 : blocks;
  if (rn_cdiv(total, blocks) > (1ll << 30)) blocks = rn_cdiv(total, 1ll << 30);
  const float bins_per_unit = (float)RN_CALIB_BINS / range;
  hipLaunchKernelGGL(calib_histogram_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, total,
                     C, pix_stride, bins_per_unit, (unsigned long long*)counts);
  RN_CHECK_LAUNCH();
  return RN_OK;
}
