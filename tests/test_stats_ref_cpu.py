"""CPU: stats_ref.py, the reference the GPU tests of rn_arena_stats / rn_arena_histogram compare against, pinned by answers
derived by hand."""
import numpy as np

import stats_ref as S


def test_integers_0_to_30_have_unit_buckets_and_a_clamped_maximum():
    x = np.arange(31, dtype=np.float32)
    c = S.histogram(x)
    # width = (30 - 0) / 30 = 1 exactly: value v lands in bucket v, and 30 (index 30) is clamped into bucket 29
    assert S.bucket_index(np.float32([7.0]), 0.0, 30.0)[0] == 7
    assert c.tolist() == [1] * 29 + [2]
    assert c.dtype == np.int32 and c.sum() == 31
    lo, hi, bad = S.finite_min_max(x)
    assert (lo, hi, bad) == (0.0, 30.0, 0)
    assert S.norm(x) == np.float32(np.sqrt(9455.0))          # sum of squares 0..30 = 30 * 31 * 61 / 6


def test_two_distinct_values_fill_the_end_buckets():
    x = np.float32([-0.5] * 5 + [0.75] * 3)
    c = S.histogram(x)
    assert c[0] == 5 and c[29] == 3 and c.sum() == 8 and not c[1:29].any()


def test_constant_tensor_goes_to_the_last_bucket():
    c = S.histogram(np.full((17,), 0.25, dtype=np.float32))
    assert c.tolist() == [0] * 29 + [17]
    z = S.stats(np.zeros((9,), dtype=np.float32))              # zero-initialised gammas
    assert z["counts"].tolist() == [0] * 29 + [9] and z["norm"] == 0.0 and z["min"] == 0.0 and z["max"] == 0.0


def test_non_finite_elements_are_counted_apart():
    s = S.stats(np.float32([np.nan, np.inf, -np.inf, 1.0, 2.0]))
    assert s["nonfinite"] == 3 and s["min"] == 1.0 and s["max"] == 2.0
    assert s["counts"].sum() == 2 and s["counts"][0] == 1 and s["counts"][29] == 1
    assert np.isnan(s["norm"])
    t = S.stats(np.float32([np.inf, -np.inf, 3.0]))             # no NaN: +inf
    assert t["norm"] == np.inf and t["nonfinite"] == 2 and t["counts"].tolist() == [0] * 29 + [1]


def test_no_finite_element():
    s = S.stats(np.float32([np.nan, np.inf]))
    assert s["min"] == 0.0 and s["max"] == 0.0 and s["nonfinite"] == 2 and not s["counts"].any()


def test_subnormals_are_kept():
    tiny = np.float32(2.0 ** -149)
    x = np.float32([tiny, 3 * tiny, -2 * tiny])
    s = S.stats(x)
    assert s["min"] == -2 * tiny and s["max"] == 3 * tiny and s["min"] != 0 and s["counts"].sum() == 3
    assert s["counts"][0] == 1 and s["counts"][29] == 1
    assert s["norm"] == 0.0                                    # float32 squares of subnormals are 0


def test_counts_and_nonfinite_add_up_on_random_input():
    rng = np.random.default_rng(11)
    for n, buckets in ((1, 30), (5, 30), (1000, 30), (8193, 1), (4097, 64)):
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.random(n) < 0.01] = np.nan
        x[rng.random(n) < 0.01] = np.inf
        s = S.stats(x, buckets)
        assert s["counts"].shape == (buckets,) and int(s["counts"].sum()) + s["nonfinite"] == n
        fin = x[np.isfinite(x)]
        if fin.size and fin.min() != fin.max():
            edges = np.linspace(np.float64(s["min"]), np.float64(s["max"]), buckets + 1)
            want = np.histogram(fin.astype(np.float64), bins=edges)[0]
            assert np.abs(s["counts"] - want).sum() <= 4       # numpy's own binning agrees up to elements on an edge


def test_norm_bound_chain_lengths():
    # chunk 8192, 256 lanes: a full block is 8 loads of 4 per lane; a tail element adds one
    assert S.norm_bound(8192, 8192)[1] == 32
    assert S.norm_bound(8191, 8192)[1] == 33
    assert S.norm_bound(1, 8192)[1] == 1 and S.norm_bound(3, 8192)[1] == 1
    assert S.norm_bound(4, 8192)[1] == 4 and S.norm_bound(5, 8192)[1] == 5 and S.norm_bound(7, 8192)[1] == 5
    assert S.norm_bound(2 * 8192 + 5, 8192)[1] == 32
    assert S.norm_bound(8193, 8192)[0] == 35 * 2.0 ** -24
