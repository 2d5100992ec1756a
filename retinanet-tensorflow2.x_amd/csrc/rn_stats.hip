// rn_stats.hip — the reference's --enable_weights_info telemetry (executor.py:329-344, called at :660-665) over the
// flat fp32 parameter arena of rn_optim.hip: per-variable tf.norm, and the TensorBoard histogram of every variable.
// The reference runs one reduction and one host read per tf.Variable (295 of them) and copies every tensor to the host
// for its histogram; here a variable is a segment of the arena and a block of OPT_CHUNK elements belongs to one
// segment, so the whole model is
//   rn_arena_stats      one streaming launch (per-block partials: sum of squares, finite min / max, non-finite count)
//                       and one small launch (one wave per segment combines its blocks),
//   rn_arena_histogram  one streaming launch (per-workgroup LDS histogram, one global integer add per bucket).
// Nothing here writes the arena; the reserved floats, the padding between segments and the bytes past the last
// segment are never read.  Deterministic: no floating-point atomics, fixed combine trees.  The contract is in
// include/rnet_hip.h.
#include "rn_common.h"

#define ST_THREADS 256
#define ST_WAVES (ST_THREADS / 64)
#define ST_MAX_BUCKETS 64
// copies of every bucket per wave, picked by lane & 7 and laid out [bucket][copy]: weight tensors put most of their mass
// into a few central buckets, and LDS adds of one wave-instruction to ONE address run one after another; the copies of
// a bucket sit in eight neighbouring banks
#define ST_COPIES 8

// Total order of the finite floats as unsigned integers (negative values: all bits flipped; others: the sign bit set).
// Integer compares flush no subnormal whatever the wave's denormal mode.  Neither ~0u (min sentinel) nor 0u (max
// sentinel) is the key of a finite value: they are the keys of two NaN patterns.
__device__ __forceinline__ uint32_t st_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float st_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ bool st_finite(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ uint32_t st_wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t st_wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ int st_wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The block's elements [b0, b1) of its segment, or b1 = b0 when the tables do not describe the block (a block the
// segment does not own, a segment index outside the table): such a block reads nothing.
struct StSpan { long long base; int n; };
__device__ __forceinline__ StSpan st_span(const OptSeg* __restrict__ segs, int nseg, int si, int blk) {
  StSpan r;
  r.base = 0;
  r.n = 0;
  if (si < 0 || si >= nseg) return r;
  const OptSeg s = segs[si];
  const long long k = (long long)blk - s.block_begin;
  if (k < 0 || k >= s.nblocks) return r;
  const long long b0 = k * OPT_CHUNK;
  if (b0 >= s.size) return r;
  const long long left = s.size - b0;
  r.base = s.offset + b0;
  r.n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
  return r;
}

// Every element of the span once: 16 bytes per lane where the block's offset is a multiple of 4 (the arena aligns
// every tensor to 4 elements and OPT_CHUNK is one), fewer than 4 tail elements one lane each; a scalar loop otherwise.
// A lane sees at most ST_ELEMS_PER_LANE = OPT_CHUNK / ST_THREADS elements of the vector body and one tail element.
#define ST_ELEMS_PER_LANE (OPT_CHUNK / ST_THREADS)
template <typename F>
__device__ __forceinline__ void st_for_each(const float* __restrict__ a, const StSpan sp, F&& one) {
  if ((sp.base & 3) == 0) {
    const int n4 = sp.n >> 2;
    const float4* a4 = (const float4*)(a + sp.base);
    for (int i = threadIdx.x; i < n4; i += ST_THREADS) {
      const float4 v = a4[i];
      one(v.x); one(v.y); one(v.z); one(v.w);
    }
    if ((int)threadIdx.x < (sp.n & 3)) one(a[sp.base + 4 * n4 + threadIdx.x]);
  } else {
    for (int i = threadIdx.x; i < sp.n; i += ST_THREADS) one(a[sp.base + i]);
  }
}

// Stage 1: per-block partials.  The squares and a lane's running sum are fp32, one rounding per product and per sum
// (-ffp-contract=off): the longest chain of fp32 additions is ST_ELEMS_PER_LANE + 1.  From there on the sums are fp64.
__global__ void __launch_bounds__(ST_THREADS)
arena_stats_partial_kernel(const float* __restrict__ a, const OptSeg* __restrict__ segs, int nseg,
                           const int* __restrict__ block_seg, double* __restrict__ p_sq, uint32_t* __restrict__ p_min,
                           uint32_t* __restrict__ p_max, int* __restrict__ p_bad) {
  const int blk = blockIdx.x;
  const StSpan sp = st_span(segs, nseg, block_seg[blk], blk);
  float acc = 0.0f;
  uint32_t kmin = 0xffffffffu, kmax = 0u;
  int bad = 0;
  st_for_each(a, sp, [&](const float x) {
    acc += x * x;
    const uint32_t u = __float_as_uint(x);
    if (st_finite(u)) {
      const uint32_t k = st_key(u);
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    } else {
      ++bad;
    }
  });
  __shared__ double r_sq[ST_WAVES];
  __shared__ uint32_t r_min[ST_WAVES], r_max[ST_WAVES];
  __shared__ int r_bad[ST_WAVES];
  const double d = rn_wave_sum_d((double)acc);
  kmin = st_wave_min_u32(kmin);
  kmax = st_wave_max_u32(kmax);
  bad = st_wave_sum_i32(bad);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    r_sq[w] = d;
    r_min[w] = kmin;
    r_max[w] = kmax;
    r_bad[w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    uint32_t mn = 0xffffffffu, mx = 0u;
    int nb = 0;
    for (int k = 0; k < ST_WAVES; ++k) {
      t += r_sq[k];
      mn = r_min[k] < mn ? r_min[k] : mn;
      mx = r_max[k] > mx ? r_max[k] : mx;
      nb += r_bad[k];
    }
    p_sq[blk] = t;
    p_min[blk] = mn;
    p_max[blk] = mx;
    p_bad[blk] = nb;
  }
}

// Stage 2: one wave per segment.  Lane l adds the segment's blocks l, l + 64, ... in that order, then the 64 lane sums
// meet in the xor butterfly: a fixed tree, the same bits on every run.
__global__ void __launch_bounds__(64)
arena_stats_combine_kernel(const OptSeg* __restrict__ segs, int num_blocks, const double* __restrict__ p_sq,
                           const uint32_t* __restrict__ p_min, const uint32_t* __restrict__ p_max,
                           const int* __restrict__ p_bad, float* __restrict__ stats, int* __restrict__ nonfinite) {
  const int si = blockIdx.x;
  const OptSeg s = segs[si];
  double sq = 0.0;
  uint32_t kmin = 0xffffffffu, kmax = 0u;
  int bad = 0;
  for (int b = threadIdx.x; b < s.nblocks; b += 64) {
    const long long g = (long long)s.block_begin + b;
    if (g < 0 || g >= num_blocks) break;
    sq += p_sq[g];
    kmin = p_min[g] < kmin ? p_min[g] : kmin;
    kmax = p_max[g] > kmax ? p_max[g] : kmax;
    bad += p_bad[g];
  }
  sq = rn_wave_sum_d(sq);
  kmin = st_wave_min_u32(kmin);
  kmax = st_wave_max_u32(kmax);
  bad = st_wave_sum_i32(bad);
  if (threadIdx.x == 0) {
    const bool none = kmin > kmax;   // no finite element: the sentinels are untouched
    stats[3 * si + 0] = (float)sqrt(sq);
    stats[3 * si + 1] = none ? 0.0f : st_unkey(kmin);
    stats[3 * si + 2] = none ? 0.0f : st_unkey(kmax);
    nonfinite[si] = bad;
  }
}

// TensorBoard's histogram buckets over the finite elements of the block, min / max from rn_arena_stats.  fp64, one
// rounding per operation, a true division (numpy float64 gives the same integers).  The index is clamped at both ends
// before it addresses LDS, whatever `stats` holds.
__global__ void __launch_bounds__(ST_THREADS)
arena_histogram_kernel(const float* __restrict__ a, const OptSeg* __restrict__ segs, int nseg,
                       const int* __restrict__ block_seg, const float* __restrict__ stats, int nbuckets,
                       int* __restrict__ counts) {
  __shared__ int hist[ST_WAVES][ST_MAX_BUCKETS][ST_COPIES];
  int* flat = &hist[0][0][0];
  for (int i = threadIdx.x; i < ST_WAVES * ST_MAX_BUCKETS * ST_COPIES; i += ST_THREADS) flat[i] = 0;
  __syncthreads();
  const int blk = blockIdx.x;
  const int si = block_seg[blk];
  const StSpan sp = st_span(segs, nseg, si, blk);
  if (sp.n > 0) {
    const float mn = stats[3 * si + 1], mx = stats[3 * si + 2];
    const bool single = mx == mn;
    const double dmin = (double)mn;
    const double width = ((double)mx - dmin) / (double)nbuckets;
    const int last = nbuckets - 1;
    int* mine = &hist[threadIdx.x >> 6][0][threadIdx.x & (ST_COPIES - 1)];
    st_for_each(a, sp, [&](const float x) {
      if (!st_finite(__float_as_uint(x))) return;
      int idx = last;
      if (!single) {
        const double q = floor(((double)x - dmin) / width);
        idx = q >= (double)last ? last : (q > 0.0 ? (int)q : 0);   // a NaN quotient (foreign stats) lands in bucket 0
      }
      atomicAdd(mine + idx * ST_COPIES, 1);
    });
  }
  __syncthreads();
  if ((int)threadIdx.x < nbuckets && sp.n > 0) {
    int t = 0;
    for (int w = 0; w < ST_WAVES; ++w)
#pragma unroll
      for (int c = 0; c < ST_COPIES; ++c) t += hist[w][threadIdx.x][c];
    if (t) atomicAdd(counts + (long long)si * nbuckets + threadIdx.x, t);
  }
}

struct StWs { double* sq; uint32_t* mn; uint32_t* mx; int* bad; };
static StWs st_ws(void* workspace, int num_blocks) {
  StWs w;
  const size_t b8 = rn_align_up((size_t)num_blocks * sizeof(double), 256);
  const size_t b4 = rn_align_up((size_t)num_blocks * sizeof(uint32_t), 256);
  char* p = (char*)workspace;
  w.sq = (double*)p;
  w.mn = (uint32_t*)(p + b8);
  w.mx = (uint32_t*)(p + b8 + b4);
  w.bad = (int*)(p + b8 + 2 * b4);
  return w;
}

extern "C" size_t rn_arena_stats_workspace_bytes(int num_blocks, int num_segments) {
  (void)num_segments;   // the per-segment results go straight to the caller's arrays
  if (num_blocks < 0) num_blocks = 0;
  return rn_align_up((size_t)num_blocks * sizeof(double), 256) + 3 * rn_align_up((size_t)num_blocks * sizeof(uint32_t), 256);
}

extern "C" int rn_arena_stats(const float* arena, const void* segs_dev, int num_segments, const int32_t* block_seg_dev,
                              int num_blocks, float* stats, int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                              void* stream) {
  RN_CHECK_ARG(arena && segs_dev && block_seg_dev && stats && nonfinite && workspace && num_segments > 0 &&
                   num_blocks > 0, "rn_arena_stats: bad argument");
  if (workspace_bytes < rn_arena_stats_workspace_bytes(num_blocks, num_segments)) {
    rn_set_error("rn_arena_stats: workspace too small");
    return RN_ENOMEM;
  }
  const StWs w = st_ws(workspace, num_blocks);
  const OptSeg* segs = (const OptSeg*)segs_dev;
  hipLaunchKernelGGL(arena_stats_partial_kernel, dim3(num_blocks), dim3(ST_THREADS), 0, (hipStream_t)stream, arena, segs,
                     num_segments, block_seg_dev, w.sq, w.mn, w.mx, w.bad);
  RN_CHECK_LAUNCH();
  hipLaunchKernelGGL(arena_stats_combine_kernel, dim3(num_segments), dim3(64), 0, (hipStream_t)stream, segs, num_blocks,
                     w.sq, w.mn, w.mx, w.bad, stats, nonfinite);
  RN_CHECK_LAUNCH();
  return RN_OK;
}

extern "C" int rn_arena_histogram(const float* arena, const void* segs_dev, int num_segments,
                                  const int32_t* block_seg_dev, int num_blocks, const float* stats, int num_buckets,
                                  int32_t* counts, void* stream) {
  RN_CHECK_ARG(arena && segs_dev && block_seg_dev && stats && counts && num_segments > 0 && num_blocks > 0,
               "rn_arena_histogram: bad argument");
  RN_CHECK_ARG(num_buckets >= 1 && num_buckets <= ST_MAX_BUCKETS, "rn_arena_histogram: num_buckets %d is outside 1..%d",
               num_buckets, ST_MAX_BUCKETS);
  RN_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)num_segments * num_buckets * sizeof(int32_t), (hipStream_t)stream));
  hipLaunchKernelGGL(arena_histogram_kernel, dim3(num_blocks), dim3(ST_THREADS), 0, (hipStream_t)stream, arena,
                     (const OptSeg*)segs_dev, num_segments, block_seg_dev, stats, num_buckets, counts);
  RN_CHECK_LAUNCH();
  return RN_OK;
}
