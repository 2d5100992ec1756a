"""GPU: the anchor matcher / target encoder (csrc/rn_match.hip) at its edges, bit for bit against the oracle:
more ground-truth boxes than one pass of the LDS fill (G = 300, G = Gmax = 1024), clamped counts, an ignore band, an IoU
exactly on a threshold, scaled box targets (and their decode), anchor tables that end inside a workgroup, best-anchor
ties inside and across workgroups, degenerate boxes, 33 images of 0 .. 32 boxes in one launch.  Everything — matches,
class targets, box targets as uint32, num-positives — equals oracle.encode_sample."""
import numpy as np
import pytest
import torch

import oracle as o
from make_golden import synth_gt

pytestmark = pytest.mark.gpu
SIZE = 128


def _encoder(cuda, shape=(SIZE, SIZE), match_iou=0.5, ignore_iou=0.5, variance=None, scale=False, aux=False):
    from retinanet.cfg import default_params
    from retinanet.dataloader import LabelEncoder
    p = default_params(input_size=shape[0])
    p.input.input_shape = list(shape)
    p.encoder_params.match_iou, p.encoder_params.ignore_iou = match_iou, ignore_iou
    p.encoder_params.scale_box_targets = scale
    if variance is not None:
        p.encoder_params.box_variance = list(variance)
    p.architecture.auxillary_head.use_auxillary_head = aux
    return LabelEncoder(p, device=cuda)


def _pad(gts, Gmax=None):
    B = len(gts)
    Gmax = max(1, max(g[0].shape[0] for g in gts)) if Gmax is None else Gmax
    gb, gc, cnt = np.zeros([B, Gmax, 4], np.float32), np.zeros([B, Gmax], np.float32), np.zeros([B], np.int32)
    for i, (b, c) in enumerate(gts):
        n = min(b.shape[0], Gmax)
        gb[i, :n], gc[i, :n], cnt[i] = b[:n], c[:n], b.shape[0]
    return torch.from_numpy(gb), torch.from_numpy(gc), torch.from_numpy(cnt)


def _encode(enc, gts, Gmax=None, counts=None):
    gb, gc, cnt = _pad(gts, Gmax)
    if counts is not None:
        cnt = torch.tensor(counts, dtype=torch.int32)
    t = enc.encode_batch(gb, gc, cnt)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t["_flat"].items()}
    out["num-positives"] = t["num-positives"].cpu().numpy()
    return out


def _raw_encode(cuda, anchors, gts, match_iou=0.5, ignore_iou=0.5):
    """rn_anchor_match_encode on any anchor table (LabelEncoder's per-level views need a whole pyramid)"""
    from retinanet import _C
    lib = _C.lib()
    gb, gc, cnt = (t.to(cuda) for t in _pad(gts))
    an = torch.from_numpy(np.ascontiguousarray(anchors)).to(cuda)
    B, Gmax, A = gb.shape[0], gb.shape[1], an.shape[0]
    m = torch.empty((B, A), dtype=torch.int32, device=cuda)
    ct, bt = torch.empty((B, A), device=cuda), torch.empty((B, A, 4), device=cuda)
    npos = torch.empty((B,), device=cuda)
    ws = torch.empty((max(256, lib.rn_match_workspace_bytes(B, Gmax)),), dtype=torch.uint8, device=cuda)
    _C.check(lib.rn_anchor_match_encode(_C.ptr(an), A, _C.ptr(gb), _C.ptr(gc), _C.ptr(cnt), B, Gmax, match_iou, ignore_iou,
                                        None, _C.ptr(m), _C.ptr(ct), _C.ptr(bt), _C.ptr(npos), _C.ptr(ws), ws.numel(),
                                        _C.current_stream()), "rn_anchor_match_encode")
    torch.cuda.synchronize()
    return {"matches": m.cpu().numpy(), "class-targets": ct.cpu().numpy(), "box-targets": bt.cpu().numpy(),
            "num-positives": npos.cpu().numpy()}


def _want(an, gb, gc, **kw):
    with np.errstate(all="ignore"):
        return o.encode_sample(an, gb, gc, **kw)


def _assert_sample(got, i, want):
    m, ct, bt, npos = want
    np.testing.assert_array_equal(got["matches"][i], m)
    np.testing.assert_array_equal(got["class-targets"][i], ct)
    np.testing.assert_array_equal(got["box-targets"][i].view(np.uint32), bt.view(np.uint32))
    assert got["num-positives"][i] == npos


@pytest.fixture(scope="module")
def table(cuda):
    """the 128 x 128 anchor table (A = 3069; bit-exact against the oracle in test_gpu_anchors_match.py) and its encoder"""
    enc = _encoder(cuda)
    an = enc.anchors.boxes.cpu().numpy()
    assert an.shape == (3069, 4)
    return enc, an


@pytest.fixture(scope="module")
def g300(cuda, table):
    gts = [synth_gt(np.random.default_rng(300), 300, SIZE), synth_gt(np.random.default_rng(301), 257, SIZE)]
    return gts, _encode(table[0], gts)


# ---- many boxes, clamped counts ---------------------------------------------------------------------------------------
def test_more_boxes_than_one_lds_fill_pass(table, g300):
    """G = 300 and 257 > 256 threads: the strided LDS fills of both passes"""
    gts, got = g300
    for i, (gb, gc) in enumerate(gts):
        _assert_sample(got, i, _want(table[1], gb, gc))
    assert (got["matches"] >= 256).any()


def test_gmax_1024_is_the_limit(cuda, table):
    enc, an = table
    gts = [synth_gt(np.random.default_rng(1024), 1024, SIZE), synth_gt(np.random.default_rng(5), 3, SIZE)]
    got = _encode(enc, gts)
    for i, (gb, gc) in enumerate(gts):
        _assert_sample(got, i, _want(an, gb, gc))
    assert got["matches"][0].max() > 768
    from retinanet._C import RnetError
    with pytest.raises(RnetError, match="Gmax=1025 outside 0..1024"):
        enc.encode_batch(torch.zeros((1, 1025, 4)), torch.zeros((1, 1025)), torch.zeros((1,), dtype=torch.int32))


def test_counts_are_clamped_to_the_padded_width(table):
    enc, an = table
    gb, gc = synth_gt(np.random.default_rng(40), 40, SIZE)
    got = _encode(enc, [(gb, gc)] * 4, Gmax=40, counts=[2000, -3, 40, 0])
    full, none = _want(an, gb, gc), _want(an, gb[:0], gc[:0])
    _assert_sample(got, 0, full)        # 2000 behaves as 40
    _assert_sample(got, 1, none)        # -3 behaves as 0
    _assert_sample(got, 2, full)
    _assert_sample(got, 3, none)
    assert (got["matches"][1] == -1).all() and got["num-positives"][1] == 0 and (got["box-targets"][1] == 0).all()


# ---- thresholds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("match_iou,ignore_iou", [(0.5, 0.4), (0.7, 0.3), (0.5, 0.5)])
def test_thresholds(cuda, table, match_iou, ignore_iou):
    an = table[1]
    gb, gc = synth_gt(np.random.default_rng(40), 40, SIZE)
    got = _encode(_encoder(cuda, match_iou=match_iou, ignore_iou=ignore_iou), [(gb, gc)])
    want = _want(an, gb, gc, match_iou=match_iou, ignore_iou=ignore_iou)
    if ignore_iou < match_iou:
        assert (want[0] == -2).any() and (want[0] == -1).any() and (want[0] >= 0).any()
        assert (want[1] == -2.0).sum() == (want[0] == -2).sum()
    _assert_sample(got, 0, want)


@pytest.mark.parametrize("match_iou,ignore_iou", [(0.5, 0.4), (0.5, 0.5)])
def test_iou_exactly_on_the_threshold(cuda, table, match_iou, ignore_iou):
    """a 32 x 16 box on the centre of the 32 x 32 anchor 903: in float32 four anchors have IoU exactly 0.5 with it.
    0.5 is not > match_iou, and not < match_iou either: apart from the forced match they are background, not ignored."""
    an = table[1]
    assert tuple(an[903]) == (36.0, 52.0, 32.0, 32.0)
    gb, gc = np.array([[36.0, 52.0, 32.0, 16.0]], np.float32), np.array([7.0], np.float32)
    iou = o.compute_iou_pairwise(gb, an)[0]
    assert iou.max() == 0.5 and np.flatnonzero(iou == np.float32(0.5)).tolist() == [759, 903, 906, 1047]
    got = _encode(_encoder(cuda, match_iou=match_iou, ignore_iou=ignore_iou), [(gb, gc)])
    want = _want(an, gb, gc, match_iou=match_iou, ignore_iou=ignore_iou)
    assert want[0][759] == 0 and (want[0][[903, 906, 1047]] == -1).all() and want[3] == 1
    assert ((want[0] == -2).sum() > 0) == (ignore_iou < match_iou)
    _assert_sample(got, 0, want)


# ---- scaled box targets and their decode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variance", [None, [0.1, 0.3, 0.2, 0.7]], ids=["default-variance", "uneven-variance"])
def test_scaled_box_targets_and_their_decode(cuda, table, variance):
    """scale_box_targets: the `use_var` divisions of match_pass2; then the same variance back through decode_kernel"""
    from retinanet.model.layers.postprocessing_ops import TransformBoxesAndScores
    an = table[1]
    enc = _encoder(cuda, scale=True, variance=variance)
    var = list(enc.encoder_params.box_variance)
    assert var == (variance or [0.1, 0.1, 0.2, 0.2])
    gts = [synth_gt(np.random.default_rng(41), 40, SIZE), synth_gt(np.random.default_rng(42), 5, SIZE)]
    got = _encode(enc, gts)
    plain = _encode(table[0], gts)
    for i, (gb, gc) in enumerate(gts):
        want = _want(an, gb, gc, box_variance=var)
        _assert_sample(got, i, want)
        assert (want[0] >= 0).sum() > 10
    assert np.array_equal(got["matches"], plain["matches"]) and not np.array_equal(got["box-targets"], plain["box-targets"])
    # decode: the targets of every anchor (zeros where not positive: they decode to the anchor itself)
    bnd = enc.anchors.anchor_boundaries
    bt = torch.from_numpy(got["box-targets"]).to(cuda)
    levels = [bt[:, bnd[i]:bnd[i + 1]].contiguous() for i in range(len(bnd) - 1)]
    boxes = TransformBoxesAndScores(enc._params, anchors=enc.anchors).decode(levels, [int(b) for b in bnd], len(gts))
    torch.cuda.synchronize()
    want = o.decode_boxes(got["box-targets"], an, SIZE, SIZE, box_variance=var)
    np.testing.assert_array_equal(boxes.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # and it is the inverse: a positive anchor's decoded box is its ground-truth box (corners / input size)
    m = got["matches"][0]
    gtc = o.convert_to_corners(gts[0][0])[m[m >= 0]] / np.float32(SIZE)
    np.testing.assert_allclose(boxes.cpu().numpy()[0][m >= 0], gtc, atol=2e-5)


# ---- anchor tables that end inside a workgroup --------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1000, 1025, 1024, 1])
def test_anchor_table_tails(cuda, table, A):
    """a workgroup covers 1024 anchors, 4 per thread: A = 1000 ends inside the only one, A = 1025 puts ONE anchor into a
    second; a box equal to the last anchor makes that anchor its best one"""
    an = table[1][:A].copy()
    rng = np.random.default_rng(A)
    gb, gc = synth_gt(rng, 6, SIZE)
    gb[2] = an[A - 1]
    gts = [(gb, gc), (gb[2:3], gc[2:3]), (gb[:0], gc[:0])]
    got = _raw_encode(cuda, an, gts, 0.5, 0.4)
    for i, (b, c) in enumerate(gts):
        want = _want(an, b, c, match_iou=0.5, ignore_iou=0.4)
        _assert_sample(got, i, want)
    assert got["matches"][1][A - 1] == 0 and (A == 1 or got["matches"][0][A - 1] == 2)


def test_non_square_input(cuda):
    enc = _encoder(cuda, shape=(96, 160), match_iou=0.5, ignore_iou=0.4)
    an = enc.anchors.boxes.cpu().numpy()
    assert an.shape[0] == 9 * (12 * 20 + 6 * 10 + 3 * 5 + 2 * 3 + 1 * 2)
    rng = np.random.default_rng(96)
    gb, gc = synth_gt(rng, 12, 96)
    gb[:, 0] = rng.uniform(0, 160, 12).astype(np.float32)
    gb[3] = an[-1]
    got = _encode(enc, [(gb, gc)])
    _assert_sample(got, 0, _want(an, gb, gc, match_iou=0.5, ignore_iou=0.4))
    assert got["matches"][0][-1] == 3


# ---- ties and collisions ------------------------------------------------------------------------------------------------------
def test_ties_and_collisions(cuda, table):
    an = table[1]
    rng = np.random.default_rng(9)
    gb, gc = synth_gt(rng, 8, SIZE)
    gc = np.arange(10, 18, dtype=np.float32)
    gb[5] = gb[1]                                        # two identical boxes: the lower index keeps the best anchor
    gb[2] = an[1500]                                     # two different boxes with one best anchor
    gb[6] = an[1500] * np.array([1, 1, 0.9, 0.9], np.float32)
    gb[3] = [5000.0, 5000.0, 10.0, 10.0]                 # no overlap with anything: its best anchor is anchor 0
    iou = o.compute_iou_pairwise(gb, an)
    best = iou.argmax(axis=1)
    assert best[5] == best[1] and best[2] == best[6] == 1500 and iou[3].max() == 0 and best[3] == 0
    got = _encode(_encoder(cuda, match_iou=0.5, ignore_iou=0.4), [(gb, gc)])
    want = _want(an, gb, gc, match_iou=0.5, ignore_iou=0.4)
    assert want[0][best[1]] == 1 and want[0][1500] == 2 and want[0][0] == 3
    _assert_sample(got, 0, want)


def test_best_anchor_tie_across_workgroups(cuda, table):
    """an 8 x 8 box inside 19 equally large anchors (IoU exactly 1/16 each) on both sides of anchor 1024, where one
    workgroup ends and the next begins: the forced match goes to the lowest of them, which the 64-bit atomic maximum
    over the workgroups decides.  Then with a copy of that anchor more than 1024 places further on, and with one in
    a workgroup in FRONT of all of them."""
    an = table[1].copy()
    gb, gc = np.array([[36.0, 52.0, 8.0, 8.0]], np.float32), np.array([3.0], np.float32)
    iou = o.compute_iou_pairwise(gb, an)[0]
    tied = np.flatnonzero(iou == iou.max())
    assert len(tied) > 1 and 0 < iou.max() < 0.4 and tied.min() < 1024 <= tied.max() < 2000
    far = 2000
    an[far] = an[tied[0]]
    iou = o.compute_iou_pairwise(gb, an)[0]
    tied2 = np.flatnonzero(iou == iou.max())
    assert tied2.tolist() == tied.tolist() + [far] and far - tied[0] > 1024
    got = _raw_encode(cuda, an, [(gb, gc)], 0.5, 0.4)
    want = _want(an, gb, gc, match_iou=0.5, ignore_iou=0.4)
    assert want[0][tied[0]] == 0 and want[0][far] == -1 and want[3] == 1
    _assert_sample(got, 0, want)
    _assert_sample(_encode(_encoder(cuda, match_iou=0.5, ignore_iou=0.4), [(gb, gc)]), 0,
                   _want(table[1], gb, gc, match_iou=0.5, ignore_iou=0.4))          # the table as it is
    # the other way round: the copy in FRONT of the tied anchors, in a workgroup of its own
    an2 = np.concatenate([an[tied[0]:tied[0] + 1], np.tile(an[3068:3069], (1023, 1)), an], axis=0)
    got = _raw_encode(cuda, an2, [(gb, gc)], 0.5, 0.4)
    want = _want(an2, gb, gc, match_iou=0.5, ignore_iou=0.4)
    assert want[0][0] == 0 and want[0][1024 + tied[0]] == -1
    _assert_sample(got, 0, want)


# ---- degenerate boxes -------------------------------------------------------------------------------------------------------
def test_degenerate_boxes(cuda, table):
    """w = 0, h = 0, a 1e-9-wide box, a zero box: the 1e-8 clamps of the union and of the box target"""
    enc, an = table
    gb = np.array([[40.0, 40.0, 0.0, 30.0], [80.0, 60.0, 25.0, 0.0], [64.0, 64.0, 1e-9, 20.0], [0.0, 0.0, 0.0, 0.0],
                   [64.0, 64.0, 40.0, 40.0]], np.float32)
    gc = np.array([1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    got = _encode(enc, [(gb, gc), (gb[:4], gc[:4])])
    for i, n in enumerate((5, 4)):
        want = _want(an, gb[:n], gc[:n])
        assert np.isfinite(want[2]).all() == np.isfinite(got["box-targets"][i]).all()
        _assert_sample(got, i, want)
    assert (got["matches"][0] == 4).sum() > 1 and got["num-positives"][1] >= 1


# ---- no leak between the images of one launch -------------------------------------------------------------------------------
def test_33_images_of_0_to_32_boxes(cuda, table):
    enc, an = table
    rng = np.random.default_rng(33)
    gts = [synth_gt(rng, n, SIZE) for n in range(33)]
    got = _encode(enc, gts)
    for i, (gb, gc) in enumerate(gts):
        _assert_sample(got, i, _want(an, gb, gc))
    assert got["num-positives"][0] == 0 and (got["num-positives"][1:] > 0).all()


# ---- the entry point that also writes iou-targets -----------------------------------------------------------------------------
def test_iou_entry_point_gives_the_same_four_outputs(cuda, table, g300):
    gts, old = g300
    new = _encode(_encoder(cuda, aux=True), gts)
    assert "iou-targets" in new and "iou-targets" not in old
    for k in ("matches", "class-targets", "num-positives"):
        assert np.array_equal(new[k], old[k]), k
    assert np.array_equal(new["box-targets"].view(np.uint32), old["box-targets"].view(np.uint32))
    pos = new["matches"] >= 0
    assert (new["iou-targets"][~pos] == -1.0).all() and (new["iou-targets"][pos] >= 0).all()
