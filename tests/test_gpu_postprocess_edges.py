"""GPU parity of the post-process kernels where tests/test_gpu_postprocess.py does not go: every load path and list size of
compact_logits_kernel (class counts 1 .. 125), the refusals past its bounds, hard NMS whose selections depend on boxes selected
in earlier sorted chunks (seams at ranks 512, 4608, 8704), merge_kernel at K = 1 and at K * max_det = 16 384, score
threshold 0, and the edges of rn_topk_per_class / rn_rowmax_argmax.  Bit for bit against the oracle; the inputs come from
tests/postprocess_cases.py and are pinned by tests/test_postprocess_cases_cpu.py."""
import numpy as np
import pytest
import torch

import oracle as o
import postprocess_cases as pc
from test_gpu_postprocess import _check, _fused, _params, _soft_lists

pytestmark = pytest.mark.gpu


def _anchors(p, size):
    return o.generate_anchors(size, size, 3, 7, p.anchor_params.areas, p.anchor_params.aspect_ratios, p.anchor_params.scales)


def _fused_twice(cuda, p, logits, enc, splits):
    """(first call's outputs, the outputs of a second call on the same device buffers)"""
    from retinanet.model.layers import DetectionPostProcess
    from test_gpu_postprocess import _split
    post = DetectionPostProcess(p)
    preds = {"class-predictions": _split(logits, splits, cuda), "box-predictions": _split(enc, splits, cuda)}
    outs = []
    for _ in range(2):
        out = post(preds)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
    return outs


def _run_fused_case(cuda, K, mode, sigma, thr=0.05):
    rng = np.random.default_rng(1000 + K)
    A = sum(pc.LEVELS_128)
    md = pc.FUSED_MAX_DET if K * pc.FUSED_MAX_DET <= 16384 else 50
    p = _params(128, K, mode=mode, pre_nms_top_k=pc.FUSED_TOP_K, max_detections=md, score_threshold=thr)
    logits = pc.logits_two_regimes(rng, A, K)
    enc = rng.normal(0, 0.3, (2, A, 4)).astype(np.float32)
    out, again = _fused_twice(cuda, p, logits, enc, pc.LEVELS_128)
    wb, ws, wc, wv = o.postprocess(logits, enc, _anchors(p, 128), 128, 128, pre_nms_top_k=pc.FUSED_TOP_K,
                                   score_threshold=thr, sigma=sigma, max_detections=md)
    _check(out, wb, ws, wc, wv)
    assert out["valid_detections"].min() > 0
    for k in out:   # a second call on the same buffers: the same bits
        assert out[k].tobytes() == again[k].tobytes(), k
    return out


# ---- (a) class counts on the fused path ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", pc.FUSED_K)
def test_fused_class_counts_hard(cuda, K):
    """compact_logits_kernel's three load paths (prefetching float4: K % 4 == 0 up to 96; plain float4: above; scalar: the rest)
    and two list sizes (5/4 sub-tile up to K = 101, one sub-tile up to 125), on a sparse and a dense image; merge_kernel without
    its radix select at K = 1"""
    _run_fused_case(cuda, K, "PerClassHardNMS", 0.0)


@pytest.mark.parametrize("K", pc.FUSED_K_SOFT)
def test_fused_class_counts_soft(cuda, K):
    _run_fused_case(cuda, K, "PerClassSoftNMS", 0.5)


def test_fused_score_threshold_zero(cuda):
    """the logit pre-test is off: every anchor of every class is a candidate, every sub-tile fills the list to the brim"""
    out = _run_fused_case(cuda, 4, "PerClassHardNMS", 0.0, thr=0.0)
    assert (out["valid_detections"] == pc.FUSED_MAX_DET).all()


# ---- (b) refusals ----------------------------------------------------------------------------------------------------
def test_refused_class_count(cuda):
    """K = 126: the compaction sub-tile passes 64 KB of LDS; refused on the host, with the bound in the message"""
    from retinanet import _C
    K, A = 126, sum(pc.LEVELS_128)
    p = _params(128, K, pre_nms_top_k=pc.FUSED_TOP_K, max_detections=100)
    logits = np.full((1, A, K), -1.0, np.float32)
    enc = np.zeros((1, A, 4), np.float32)
    with pytest.raises(_C.RnetError, match=r"status -1"):
        _fused(cuda, p, logits, enc, pc.LEVELS_128)
    msg = _C.lib().rn_last_error().decode()
    assert "rn_detect_per_class" in msg and "K=126 > 125" in msg, msg
    torch.cuda.synchronize()


def test_refused_merge_size(cuda):
    """K * max_det = 65 * 256 = 16 640 > 16 384: refused by both entry points' shared check"""
    from retinanet import _C
    from retinanet.model.layers import GenerateDetections
    K, n = 65, 8
    gen = GenerateDetections(iou_threshold=0.5, score_threshold=0.05, max_detections=256, num_classes=K, mode="PerClassHardNMS")
    x = {"scores": torch.full((1, n, K), 0.5, device=cuda), "boxes": torch.zeros((1, n, K, 4), device=cuda)}
    with pytest.raises(_C.RnetError, match=r"status -1"):
        gen(x)
    msg = _C.lib().rn_last_error().decode()
    assert "K*max_det=16640 > 16384" in msg, msg


def _nms_standalone(cuda, scores, boxes, md, K):
    from retinanet.model.layers import GenerateDetections
    gen = GenerateDetections(iou_threshold=0.5, score_threshold=0.05, max_detections=md, soft_nms_sigma=0.5, num_classes=K,
                             mode="PerClassHardNMS")
    out, idx = gen._run(torch.from_numpy(scores).to(cuda), torch.from_numpy(boxes).to(cuda), 0.5, 0.0, want_index=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, idx.cpu().numpy()


def test_merge_at_its_limit(cuda):
    """K = 64, max_det = 256: merge_kernel selects 256 of 16 384 padded scores, 12 800 of them real — every class selects its
    200 cells over all four sorted chunks — and, the scores being a function of the rank, in runs of 64 equal scores that the
    class-major slot orders"""
    n, G, step, side, md = pc.STAIRCASES[1]
    K = 64
    scores, boxes, _ = pc.staircase_lists(64, n, G, step, side, 1, K)
    out, idx = _nms_standalone(cuda, scores, boxes, md, K)
    wb, ws, wc, wv, wi = o.per_class_nms(scores, boxes, 0.5, 0.05, 0.0, md, return_index=True)
    _check(out, wb, ws, wc, wv)
    np.testing.assert_array_equal(idx, wi)
    assert wv[0] == 256 and (wc[0].reshape(4, 64) == np.arange(64)).all()


# ---- (c) hard NMS across chunk seams, stand-alone ------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1, 2])
def test_hard_nms_selections_in_every_chunk(cuda, case):
    """rn_nms_per_class on staircase lists: the selected boxes are the first ranks of the cells, spread over all sorted chunks
    (512 keys, then 4 096 at a time), so a selection in chunk 3 stands only if the boxes selected in chunks 1 and 2 were carried
    over and tested; class 2 is a pile (every box overlaps every other one: suppression eats through the chunks)"""
    n, G, step, side, md = pc.STAIRCASES[case]
    B, K = 2, 3
    scores, boxes, ranks = pc.staircase_lists(100 + case, n, G, step, side, B, K)
    m = min(n, 9000)
    ps, pb = _soft_lists(np.random.default_rng(200 + case), B, m, 1, "pile")
    scores[:, :, 2], boxes[:, :, 2] = 0.0, 0.0
    scores[:, :m, 2], boxes[:, :m, 2] = ps[:, :, 0], pb[:, :, 0]
    out, idx = _nms_standalone(cuda, scores, boxes, md, K)
    wb, ws, wc, wv, wi = o.per_class_nms(scores, boxes, 0.5, 0.05, 0.0, md, return_index=True)
    # not vacuous: what the merged output keeps of the staircase classes comes from at least two bands (the low bands lose the
    # merge to the pile's scores), and each staircase list on its own selects in every band (test_postprocess_cases_cpu.py)
    for b in range(B):
        for c in (0, 1):
            rows = wi[b, :wv[b]][wc[b, :wv[b]] == c]
            assert sum(x > 0 for x in pc.band_counts(ranks[b, rows, c], n)) >= 2
    _check(out, wb, ws, wc, wv)
    np.testing.assert_array_equal(idx, wi)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_hard_nms_single_class_every_band(cuda, case):
    """one staircase per image and nothing else (K = 1: merge_kernel passes the list through), so no other class outscores
    the low ranks in the merge and the detections themselves come from every band: a selection lost or gained past a seam
    shows in the output"""
    n, G, step, side, md = pc.STAIRCASES[case]
    B, K = 2, 1
    scores, boxes, ranks = pc.staircase_lists(400 + case, n, G, step, side, B, K)
    out, idx = _nms_standalone(cuda, scores, boxes, md, K)
    wb, ws, wc, wv, wi = o.per_class_nms(scores, boxes, 0.5, 0.05, 0.0, md, return_index=True)
    for b in range(B):
        bands = pc.band_counts(ranks[b, wi[b, :wv[b]], 0], n)
        assert min(bands[:2] if case == 2 else bands) >= 2, bands
    assert (wv == G).all()
    _check(out, wb, ws, wc, wv)
    np.testing.assert_array_equal(idx, wi)


@pytest.mark.parametrize("n", [512, 513, 4608, 4609])
def test_hard_nms_list_ends_at_a_seam(cuda, n):
    """the first staircase cut to the ranks below n: the seam (or one candidate past it) is the end of the list"""
    n0, G, step, side, md = pc.STAIRCASES[0]
    B, K = 1, 3
    s0, b0, r0 = pc.staircase_lists(300, n0, G, step, side, B, K)
    scores, boxes = np.zeros((B, n, K), np.float32), np.zeros((B, n, K, 4), np.float32)
    for c in range(K):
        keep = r0[0, :, c] < n
        scores[0, :, c], boxes[0, :, c] = s0[0, keep, c], b0[0, keep, c]
    out, idx = _nms_standalone(cuda, scores, boxes, md, K)
    wb, ws, wc, wv, wi = o.per_class_nms(scores, boxes, 0.5, 0.05, 0.0, md, return_index=True)
    _check(out, wb, ws, wc, wv)
    np.testing.assert_array_equal(idx, wi)
    assert wv[0] == min(md, K * ((n + step - 1) // step))


# ---- (d) hard NMS across chunk seams, fused ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_staircase():
    """256 x 256 pyramid, K = 4: class 0 carries the first staircase cut to A ranks (boxes through box-predictions, scores
    through logit(score)), the other classes sparse noise"""
    rng = np.random.default_rng(2024)
    size, K, A = 256, 4, sum(pc.LEVELS_256)
    p = _params(size, K)
    an = _anchors(p, size)
    n0, G, step, side, _ = pc.STAIRCASES[0]
    bx, sc, rank = pc.staircase(rng, n0, G, step, side)
    keep = rank < A
    bx, sc = bx[keep], sc[keep]
    logits = rng.normal(-4.6, 1.0, (1, A, K)).astype(np.float32)
    logits[0, :, 0] = np.log(sc.astype(np.float64) / (1.0 - sc.astype(np.float64))).astype(np.float32)
    enc = pc.encode_for(bx, an, size, size)[None]
    s0 = o.sigmoidf(logits[0, :, 0])
    assert np.unique(s0).size == A          # the ranks survive logit -> sigmoid
    return logits, enc, an, np.sort(s0)[::-1].copy()


def _class0_ranks(out_scores, out_classes, valid, sorted_desc):
    s = out_scores[0, :valid[0]][out_classes[0, :valid[0]] == 0]
    return np.searchsorted(-sorted_desc, -s)          # rank = number of class-0 candidates with a higher score


@pytest.mark.parametrize("topk", [-1, 5000])
def test_fused_hard_nms_across_seams(cuda, fused_staircase, topk):
    logits, enc, an, sorted_desc = fused_staircase
    A = logits.shape[1]
    p = _params(256, 4, mode="PerClassHardNMS", pre_nms_top_k=topk, max_detections=100)
    out = _fused(cuda, p, logits, enc, pc.LEVELS_256)
    wb, ws, wc, wv = o.postprocess(logits, enc, an, 256, 256, pre_nms_top_k=topk, max_detections=100)
    want_ranks = _class0_ranks(ws, wc, wv, sorted_desc)
    if topk < 0:    # radix select over cap = A, chunks of 512 / 4096 / 4096 / 3572 keys
        bands = pc.band_counts(want_ranks, A)
        assert sum(x > 0 for x in bands) >= 3, bands
    else:           # the band past 4608 is cut at 5000
        assert want_ranks.max() < 5000 and (want_ranks >= 4608).any(), want_ranks
    _check(out, wb, ws, wc, wv)
    got_ranks = _class0_ranks(out["scores"], out["classes"], out["valid_detections"], sorted_desc)
    np.testing.assert_array_equal(got_ranks, want_ranks)


# ---- (e) rn_topk_per_class / rn_rowmax_argmax ----------------------------------------------------------------------------
def _topk(cuda, scores, k):
    from retinanet.model.layers import FilterTopKDetections
    B, A, K = scores.shape
    st = {"scores": torch.from_numpy(scores).to(cuda), "boxes": torch.zeros((B, A, 4), device=cuda)}
    f = FilterTopKDetections(top_k=k)(st)
    torch.cuda.synchronize()
    ws, wi = o.topk_per_class(scores, k)
    assert tuple(f["scores"].shape) == ws.shape
    np.testing.assert_array_equal(f["indices"].cpu().numpy(), wi)
    np.testing.assert_array_equal(f["scores"].cpu().numpy().view(np.uint32), ws.view(np.uint32))


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("A,k", [(300, 500), (8192, 8192), (8193, 8192), (12276, 9000)])
def test_topk_shapes(cuda, A, k, K):
    """A < top_k; the whole list as one LDS sort; one candidate more than that (a radix select that drops one key); two chunks"""
    rng = np.random.default_rng(A + k + K)
    scores = rng.random((2, A, K), dtype=np.float32)
    scores[1, ::7, 0] = scores[1, 0, 0]          # and ties, ordered by the anchor
    _topk(cuda, scores, k)


@pytest.mark.parametrize("A,k", [(3000, 1000), (12276, 8300)])
def test_topk_tie_run_straddles_the_cut(cuda, A, k):
    """400 equal scores around rank k (for k = 8300 the run also straddles the first chunk's end at 8192): the cut keeps the
    run's lowest anchors"""
    _topk(cuda, pc.tie_run_scores(np.random.default_rng(k), 2, A, 5, k), k)


@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("K", [1, 7])
def test_rowmax_ties(cuda, rows, K):
    """tf.argmax: the first maximum — rows of equal values, the maximum at the first and the last class and at both"""
    from retinanet import _C
    rng = np.random.default_rng(rows + K)
    x = rng.normal(0, 1, (rows, K)).astype(np.float32)
    x[0::4] = x[0::4, :1]                         # all equal
    x[1::4, 0] = x[1::4, K - 1] = 5.0             # first and last
    x[2::4, K - 1] = 5.0                          # last only
    x[3::4, K // 2:] = x[3::4, K // 2:K // 2 + 1] # a run of equal values that may hold the maximum
    d = torch.from_numpy(x).to(cuda)
    mx = torch.empty((rows,), dtype=torch.float32, device=cuda)
    arg = torch.empty((rows,), dtype=torch.int32, device=cuda)
    with torch.cuda.device(cuda):
        _C.check(_C.lib().rn_rowmax_argmax(_C.ptr(d), rows, K, _C.ptr(mx), _C.ptr(arg), _C.current_stream()), "rowmax")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mx.cpu().numpy().view(np.uint32), x.max(axis=1).view(np.uint32))
    np.testing.assert_array_equal(arg.cpu().numpy(), x.argmax(axis=1).astype(np.int32))
