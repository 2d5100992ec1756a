"""The float64 / numpy statement of the contract of rn_arena_stats and rn_arena_histogram (include/rnet_hip.h), shared by the
CPU and GPU tests.  It imports nothing from the package.

For one variable x (float32, any shape):
  norm       sqrt(sum of x * x), every square rounded to float32 as the contract has it (a square below 2^-149 is 0, one
             above float32 is +inf), the sum and the root in float64, the result rounded to float32.  A NaN element gives
             NaN, an infinite one and no NaN gives +inf.
  min, max   over the finite elements, exact (subnormals included); 0, 0 when there is none.
  nonfinite  the number of NaN or +-inf elements.
  counts     TensorBoard's `histogram` summary buckets (summary_v2, bucket_count = 30 by default) over the FINITE elements:
             max == min -> everything in the last bucket; otherwise, in float64 with one rounding per operation,
                 width = (float64(max) - float64(min)) / buckets
                 index = min(buckets - 1, int(floor((float64(x) - float64(min)) / width)))
             The bucket edges are numpy.linspace(min, max, buckets + 1).  (TensorBoard itself lets non-finite values
             poison the edges; here they are counted apart, so that sum(counts) + nonfinite == size.)
"""
import numpy as np

BUCKETS = 30


def norm(x):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sq = (x * x).astype(np.float32)                       # one float32 rounding per square
        return np.float32(np.sqrt(np.sum(sq.astype(np.float64))))


def finite_min_max(x):
    """(min, max, nonfinite) — min = max = 0 when no element is finite"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    ok = np.isfinite(x)
    bad = int(x.size - ok.sum())
    if not ok.any():
        return np.float32(0.0), np.float32(0.0), bad
    return np.float32(x[ok].min()), np.float32(x[ok].max()), bad


def bucket_index(x, lo, hi, buckets=BUCKETS):
    """bucket of every element of x (all finite) for the range [lo, hi]"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if np.float32(hi) == np.float32(lo):
        return np.full(x.shape, buckets - 1, dtype=np.int64)
    lo64, hi64 = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    width = (hi64 - lo64) / np.float64(buckets)
    idx = np.floor((x.astype(np.float64) - lo64) / width).astype(np.int64)
    return np.minimum(idx, buckets - 1)


def histogram(x, buckets=BUCKETS):
    """int32[buckets] over the finite elements, range = their own minimum and maximum"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    lo, hi, _ = finite_min_max(x)
    fin = x[np.isfinite(x)]
    if fin.size == 0:
        return np.zeros((buckets,), dtype=np.int32)
    return np.bincount(bucket_index(fin, lo, hi, buckets), minlength=buckets).astype(np.int32)


def stats(x, buckets=BUCKETS):
    lo, hi, bad = finite_min_max(x)
    return {"norm": norm(x), "min": lo, "max": hi, "nonfinite": bad, "counts": histogram(x, buckets)}


def norm_bound(size, chunk, threads=256):
    """Relative bound on |kernel norm - norm(x)| / norm(x) from the kernel's summation shape.

    A workgroup of `threads` lanes takes `chunk` elements of one variable; a lane adds its squares in float32, four per
    16-byte load and one for a tail element when the block's length is no multiple of 4, so the longest chain of float32
    additions in a block of n elements is 4 * ceil((n // 4) / threads) + (1 if n % 4 else 0) — at most chunk / threads + 1 —
    and everything after the lane is float64.  Positive terms: a chain of k additions is off by at most k * 2^-24
    relatively; the root halves it; the roundings to float32 of the kernel's result and of the reference's add one 2^-24
    each.  (chain + 3) * 2^-24 covers that with room."""
    chain = 0
    for b0 in range(0, size, chunk):
        n = min(chunk, size - b0)
        n4 = n // 4
        chain = max(chain, 4 * -(-n4 // threads) + (1 if n % 4 else 0))
    return (chain + 3) * 2.0 ** -24, chain
