"""Inputs of the post-process edge tests (tests/test_gpu_postprocess_edges.py) and what pins them on the CPU
(tests/test_postprocess_cases_cpu.py).  No GPU, no library call: numpy only; expectations always come from the oracle."""
import numpy as np

F32 = np.float32
LEVELS_128 = [2304, 576, 144, 36, 9]        # A = 3069: full compaction tiles, a one-sub-tile tail, a 16-row tail, short levels
LEVELS_256 = [9216, 2304, 576, 144, 36]     # A = 12276
SUB_TILE = 64                               # anchors of a compaction sub-tile (RN_CT_ANCHORS)
SEAMS = (512, 4608, 8704)                   # hard NMS sorts 512 keys first, then 4096 at a time
LOGIT_005 = float(np.log(0.05 / 0.95))

# class counts of the fused path -> the load path and the survivor list compact_logits_kernel takes at that count
FUSED_K = (1, 2, 3, 4, 20, 90, 91, 96, 100, 101, 102, 104, 124, 125)
FUSED_K_SOFT = (1, 91, 100, 125)
FUSED_TOP_K = 2000
FUSED_MAX_DET = 100
# from this count on, the sparse image's raised class (about 51 of a sub-tile's 64 anchors) and the 5 % of the other classes
# stay below the quarter of a sub-tile's 64 * K logits that makes the kernel flush: 51 + 3.2 (K - 1) against 16 K
SPARSE_FROM_K = 20

# (n, G, step, side, max_det) of the hard-NMS staircases
STAIRCASES = ((13000, 64, 200, 8, 100), (13000, 200, 64, 16, 256), (4700, 47, 100, 8, 64))


def compaction_path(K):
    """(load path, survivor list in sub-tiles) of compact_logits_kernel, from the arithmetic of rn_detect_per_class"""
    def lds(cap_list):
        return (cap_list * 8 + 4 + K * 8 + 16 + 15) // 16 * 16
    load = "scalar" if K % 4 else ("prefetch" if SUB_TILE * K <= 6 * 256 * 4 else "float4")
    if lds(SUB_TILE * K + SUB_TILE * K // 4) <= 65536:
        return load, 1.25
    return (load, 1.0) if lds(SUB_TILE * K) <= 65536 else (load, None)


def logits_two_regimes(rng, A, K, B=2):
    """f32[B,A,K]: image 0 sparse — N(-4.6, 1), class 0 raised by 2.5 — every further image dense, N(-1, 2): about 80 % above
    logit(0.05), so every sub-tile collects more than a quarter of its logits and flushes before the workgroup's end.  The
    dense image holds a few runs of exactly equal logits."""
    x = np.empty((B, A, K), F32)
    x[0] = rng.normal(-4.6, 1.0, (A, K))
    x[0, :, 0] += F32(2.5)
    for b in range(1, B):
        x[b] = rng.normal(-1.0, 2.0, (A, K))
        for t in range(3):
            rows = rng.choice(A, 6, replace=False)
            x[b, rows, t % K] = F32(0.5 + 0.25 * t)
    return x


def subtile_survivors(logits, levels, x_skip=LOGIT_005 - 1e-3):
    """per image the number of logits that pass the kernel's pre-test in each sub-tile of 64 anchors of each level, and the
    number of logits of that sub-tile: two lists of int arrays [B][sub-tiles]"""
    B, A, K = logits.shape
    got, size = [[] for _ in range(B)], []
    off = 0
    for n in levels:
        for a0 in range(0, n, SUB_TILE):
            rows = min(SUB_TILE, n - a0)
            size.append(rows * K)
            for b in range(B):
                got[b].append(int((logits[b, off + a0:off + a0 + rows] >= F32(x_skip)).sum()))
        off += n
    return [np.array(g) for g in got], np.array(size)


def staircase(rng, n, G, step, side):
    """A hard-NMS list whose selections are spread over its whole sorted order: (boxes f32[n,4], scores f32[n], rank i64[n]).
    G disjoint cells of a side x side grid; the box of a rank is its cell's centred square of edge 0.8 / side with a jitter of
    +-0.002 per coordinate, so boxes of one cell overlap with IoU > 0.5 and boxes of two cells never do: the selected
    candidates are exactly the first ranks of the cells.  Scores fall linearly with the rank from 0.99 to 0.06; rank i opens
    cell i // step when i % step == 0 (and i // step < G), every other rank falls into a cell opened before it.  The rows are
    shuffled: rank[r] is the rank of row r."""
    assert G <= side * side
    i = np.arange(n)
    opened = np.minimum(i // step + 1, G)
    cell = np.minimum((rng.random(n) * opened).astype(np.int64), opened - 1)
    opens = (i % step == 0) & (i // step < G)
    cell[opens] = i[opens] // step
    ctr = np.stack([(cell // side + 0.5) / side, (cell % side + 0.5) / side], -1).astype(F32)
    half = F32(0.4 / side)
    boxes = np.concatenate([ctr - half, ctr + half], -1).astype(F32)
    boxes = (boxes + rng.uniform(-0.002, 0.002, (n, 4)).astype(F32)).astype(F32)
    scores = np.linspace(0.99, 0.06, n, dtype=F32)
    rank = rng.permutation(n)
    return boxes[rank], scores[rank], rank


def staircase_lists(seed, n, G, step, side, B, K):
    """[B,n,K] scores, [B,n,K,4] boxes, [B,n,K] ranks: one staircase per (image, class), each from a seed of its own"""
    scores, boxes = np.zeros((B, n, K), F32), np.zeros((B, n, K, 4), F32)
    ranks = np.zeros((B, n, K), np.int64)
    for b in range(B):
        for c in range(K):
            bx, sc, rk = staircase(np.random.default_rng([seed, b, c]), n, G, step, side)
            boxes[b, :, c], scores[b, :, c], ranks[b, :, c] = bx, sc, rk
    return scores, boxes, ranks


def band_counts(ranks, n):
    """selected ranks -> how many fall into [0,512), [512,4608), [4608,8704), [8704,n)"""
    edges = [0] + [s for s in SEAMS if s < n] + [n]
    return [int(((ranks >= lo) & (ranks < hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]


def encode_for(boxes, anchors, h, w):
    """float64 inverse of TransformBoxesAndScores' decode (no box variance), rounded to float32: the box-predictions whose
    decoded boxes are `boxes` up to rounding.  boxes [n,4] normalised corners, anchors [n,4] (centre, size)."""
    p = np.asarray(boxes, np.float64) * np.array([h, w, h, w], np.float64)
    an = np.asarray(anchors, np.float64)
    ctr, wh = (p[:, :2] + p[:, 2:]) / 2.0, p[:, 2:] - p[:, :2]
    return np.concatenate([(ctr - an[:, :2]) / an[:, 2:], np.log(wh / an[:, 2:])], -1).astype(F32)


def tie_run_scores(rng, B, A, K, k, run=400, lead=150):
    """f32[B,A,K] distinct scores per (image, class), except the ranks k - lead .. k - lead + run - 1 of every list, which all
    take the score of the first of them: a run of `run` equal scores that contains rank k"""
    s = np.empty((B, A, K), F32)
    for b in range(B):
        for c in range(K):
            col = rng.permutation(np.linspace(0.01, 0.99, A, dtype=F32))
            order = np.argsort(-col.astype(np.float64), kind="stable")
            col[order[k - lead:k - lead + run]] = col[order[k - lead]]
            s[b, :, c] = col
    return s
