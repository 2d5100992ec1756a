"""What keeps tests/test_gpu_postprocess_edges.py from being vacuous, pinned with the oracle alone: the staircase lists
really select in every sorted chunk of the hard-NMS kernel, the two logit regimes really are one that flushes the
compaction list inside a workgroup and one that does not, the top-k filter really cuts, the tie run really holds the cut."""
import numpy as np
import pytest

import oracle as o
import postprocess_cases as pc


def _selected_ranks(n, G, step, side, md, seed=0):
    bx, sc, rank = pc.staircase(np.random.default_rng(seed), n, G, step, side)
    idx, _, v = o.nms_v5(bx, sc, md, 0.5, 0.05, 0.0)
    return rank[idx[:v]], v


def test_staircase_geometry():
    """same cell: IoU > 0.5; different cells: disjoint — at both grid sizes in use"""
    for side, G in ((8, 64), (16, 200)):
        bx, _, rank = pc.staircase(np.random.default_rng(3), 3000, G, 10, side)
        cell = (np.floor((bx[:, 0] + bx[:, 2]) / 2 * side) * side + np.floor((bx[:, 1] + bx[:, 3]) / 2 * side)).astype(int)
        a, b = bx[:400, None].astype(np.float64), bx[None].astype(np.float64)
        ih = np.clip(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), 0, None)
        iw = np.clip(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), 0, None)
        area = lambda z: (z[..., 2] - z[..., 0]) * (z[..., 3] - z[..., 1])
        iou = ih * iw / (area(a) + area(b) - ih * iw)
        same = cell[:400, None] == cell[None]
        assert iou[same].min() > 0.5 and iou[~same].max() == 0.0
        assert bx.min() > 0.0 and bx.max() < 1.0 and sorted(rank) == list(range(3000))


@pytest.mark.parametrize("case,want_bands,want_valid,want_last", [
    (0, [3, 21, 20, 20], 64, 12600), (1, [8, 64, 64, 64], 200, 12736), (2, [6, 41, 0], 47, 4600)])
def test_staircase_band_counts(case, want_bands, want_valid, want_last):
    n, G, step, side, md = pc.STAIRCASES[case]
    ranks, v = _selected_ranks(n, G, step, side, md)
    bands = pc.band_counts(ranks, n)
    # the third list ends 92 ranks past the second seam: its first two bands count
    assert min(bands[:2] if case == 2 else bands) >= 2, bands
    # the first ranks of the cells, whatever the seed: rank g * step opens cell g
    assert bands == want_bands and v == want_valid and ranks.max() == want_last
    assert sorted(ranks) == [g * step for g in range(G)]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_staircase_shows_a_lost_carry(case):
    """the defect the staircase is for: an NMS that runs each sorted chunk on its own — the boxes selected before a seam are
    not tested behind it — selects the first rank of every open cell again in every chunk.  The staircase's expected output
    differs from that in every chunk past the first."""
    n, G, step, side, md = pc.STAIRCASES[case]
    bx, sc, rank = pc.staircase(np.random.default_rng(0), n, G, step, side)
    order = np.argsort(rank)
    bx, sc = bx[order], sc[order]                      # row = rank
    idx, _, v = o.nms_v5(bx, sc, md, 0.5, 0.05, 0.0)
    want = set(idx[:v].tolist())
    edges = [0] + [s for s in pc.SEAMS if s < n] + [n]
    for lo, hi in zip(edges[1:-1], edges[2:]):
        idx_c, _, v_c = o.nms_v5(bx[lo:hi], sc[lo:hi], md, 0.5, 0.05, 0.0)
        alone = set((idx_c[:v_c] + lo).tolist())
        assert len(alone - want) >= 2, (lo, hi)       # cells opened before the seam come back


def test_staircase_cut_at_seams():
    """the lists that end on a seam or one past it still select (in their last chunk, too)"""
    n, G, step, side, md = pc.STAIRCASES[0]
    bx, sc, rank = pc.staircase(np.random.default_rng(0), n, G, step, side)
    for cut in (512, 513, 4608, 4609):
        keep = rank < cut
        idx, _, v = o.nms_v5(bx[keep], sc[keep], md, 0.5, 0.05, 0.0)
        assert v == (cut + step - 1) // step and rank[keep][idx[:v]].max() == (v - 1) * step


@pytest.mark.parametrize("K", pc.FUSED_K)
def test_sparse_and_dense_regimes(K):
    A = sum(pc.LEVELS_128)
    x = pc.logits_two_regimes(np.random.default_rng(1000 + K), A, K)
    got, size = pc.subtile_survivors(x, pc.LEVELS_128)
    # the kernel flushes its list before the workgroup's end when more than a quarter of a sub-tile's logits were collected
    assert (got[1] * 4 > size).all(), "dense image: every sub-tile flushes"
    if K >= pc.SPARSE_FROM_K:
        assert (got[0] * 4 <= size).all(), "sparse image: no sub-tile flushes on its own"
    else:
        # class 0 alone, raised to 80 % survivors, is a quarter of the logits or more at these counts
        assert (got[0] * 4 > size).any()
    cand = (o.sigmoidf(x) > 0.05).sum(axis=1)          # [B,K]
    assert cand.max() > pc.FUSED_TOP_K and cand[0].min() >= 0
    assert cand[0, 0] > pc.FUSED_TOP_K                # the sparse image's raised class is cut by the filter as well
    if K > 1:
        assert cand[0, 1:].max() < 400                # ... and its other classes are sparse
    # exact ties among the dense image's candidates
    col = x[1, :, 0]
    assert (np.unique(col, return_counts=True)[1] >= 6).any()


def test_compaction_path_table():
    """the K -> (load path, list size) table of DESIGN.md, from the arithmetic of rn_detect_per_class"""
    want = {1: ("scalar", 1.25), 2: ("scalar", 1.25), 3: ("scalar", 1.25), 4: ("prefetch", 1.25), 20: ("prefetch", 1.25),
            80: ("prefetch", 1.25), 90: ("scalar", 1.25), 91: ("scalar", 1.25), 96: ("prefetch", 1.25),
            100: ("float4", 1.25), 101: ("scalar", 1.25), 102: ("scalar", 1.0), 104: ("float4", 1.0),
            124: ("float4", 1.0), 125: ("scalar", 1.0), 126: ("scalar", None)}
    for K, w in want.items():
        assert pc.compaction_path(K) == w, K
    assert set(pc.FUSED_K) <= set(want)


def test_tie_run_straddles_the_cut():
    k = 1000
    s = pc.tie_run_scores(np.random.default_rng(5), 2, 3000, 5, k)
    for b in range(2):
        for c in range(5):
            col = s[b, :, c]
            v, cnt = np.unique(col, return_counts=True)
            tie = v[cnt.argmax()]
            assert cnt.max() == 400 and (cnt > 1).sum() == 1
            above = int((col > tie).sum())
            assert above < k < above + 400 and above == k - 150       # members on both sides of rank k
    ws, wi = o.topk_per_class(s, k)
    run = ws[0, :, 0] == ws[0, k - 1, 0]
    assert run.sum() == 150 and (np.diff(wi[0, run, 0]) > 0).all()    # the cut keeps the run's lowest rows, in row order
