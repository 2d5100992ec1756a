"""The float64 references of tests/pyramid_ref.py pinned on the CPU: hand-written windows for the tie rule of the
max-pool backward, torch float64 autograd for the BalanceFeatures backward on a tie-free input, the rounding helper
against torch's own casts, and the proof that the acceptance rule has teeth: deliberately wrong REFERENCES are
rejected at the small shapes of test_gpu_pyramid_kernels.py, the unmodified one (also when it is rounded through fp32
first) is accepted."""
import pytest
import torch
import torch.nn.functional as F

import pyramid_ref as R

DTYPES = [torch.bfloat16, torch.float16]
BF = torch.bfloat16


def _nhwc(rows):
    """[H][W] numbers -> float64 [1, H, W, 1]"""
    return torch.tensor(rows, dtype=R.F64)[None, :, :, None]


def _hw(t):
    return t[0, :, :, 0].tolist()


# ---- the rounding helper ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_round_storage_is_one_rounding_to_nearest_even(dtype):
    g = torch.Generator().manual_seed(1)
    fi = torch.finfo(dtype)
    x = torch.cat([torch.randn(4096, generator=g) * 8, torch.randn(4096, generator=g) * fi.smallest_normal * 4,
                   torch.tensor([0.0, -0.0, fi.max, -fi.max, fi.smallest_normal, fi.smallest_normal / 4])])
    # every midpoint between neighbours of the storage type around 1 and around 6, and a subnormal one
    grid = torch.arange(-64, 65, dtype=torch.float32) * fi.eps * 0.5
    x = torch.cat([x, 1.0 + grid, 6.0 + 4 * grid, grid * fi.smallest_normal])
    want = x.to(dtype).to(R.F64)          # exact in fp32: torch's cast is the single rounding
    assert torch.equal(R.round_storage(x.to(R.F64), dtype), want)
    # a float64 a hair above a midpoint rounds up; through float32 it would land ON the midpoint and go to even (down)
    mid = 1.0 + float(fi.eps) / 2
    v = torch.tensor([mid + 2.0 ** -40, mid, mid - 2.0 ** -40], dtype=R.F64)
    assert R.round_storage(v, dtype).tolist() == [1.0 + float(fi.eps), 1.0, 1.0]
    assert v.to(torch.float32).to(dtype).to(R.F64).tolist() == [1.0, 1.0, 1.0]
    assert R.round_storage(torch.tensor([float(fi.max) * 1.01], dtype=R.F64), dtype).item() == float("inf")


# ---- the tie rule of the max-pool backward, by hand -----------------------------------------------------------------
def test_maxpool_bwd_tie_between_an_earlier_and_a_later_tap():
    # 3x3 / stride 2 SAME on 4x4: pad 0 top/left, windows start at rows/cols 0 and 2, the last row/col of the second is padding
    assert R.same_geometry(4, 3, 2) == (2, 0)
    x = _nhwc([[5, 1, 0, 0],
               [1, 5, 0, 0],     # window (0,0): 5 at tap (0,0) and at tap (1,1) -> the earlier one, pixel (0,0)
               [0, 0, 0, 0],
               [0, 0, 0, 7]])
    dy = _nhwc([[1, 2], [4, 8]])
    r = R.maxpool_bwd(x, dy, 3, 2, 0, 0, BF)
    # window (0,1) = cols 2..3 (+ pad), rows 0..2: all zero -> its first tap, pixel (0,2); window (1,0) = rows 2..3,
    # cols 0..2: all zero -> pixel (2,0); window (1,1): 7 at pixel (3,3)
    assert _hw(r.value) == [[1, 0, 2, 0], [0, 0, 0, 0], [4, 0, 0, 0], [0, 0, 0, 8]]
    assert _hw(R.maxpool_fwd(x, 3, 2, 0, 0, 2, 2)) == [[5, 0], [0, 7]]
    last = R.maxpool_bwd(x, dy, 3, 2, 0, 0, BF, pick="last")
    # the last tap INSIDE the image: (1,1) of window (0,0), (2,3) of window (0,1), (3,2) of window (1,0)
    assert _hw(last.value) == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 2], [0, 0, 4, 8]]


def test_maxpool_bwd_tie_across_two_overlapping_windows():
    x = _nhwc([[0, 0, 9, 0],
               [0, 0, 9, 0],     # column 2 belongs to windows (0,0) and (0,1): both see 9 twice, both pick row 0
               [0, 0, 0, 0],
               [0, 0, 0, 0]])
    dy = _nhwc([[1, 2], [4, 8]])
    dx0 = _nhwc([[0.5] * 4] * 4)
    r = R.maxpool_bwd(x, dy, 3, 2, 0, 0, BF, dx0=dx0)
    # windows (1,0) and (1,1) are all zero: first taps, pixels (2,0) and (2,2)
    assert _hw(r.value) == [[0.5, 0.5, 3.5, 0.5], [0.5, 0.5, 0.5, 0.5], [4.5, 0.5, 8.5, 0.5], [0.5, 0.5, 0.5, 0.5]]
    assert _hw(r.terms) == _hw(r.value) and r.n == 5


def test_maxpool_bwd_tie_that_involves_the_padded_border():
    # odd size: 3x3 / stride 2 SAME on 3x3 pads 1 on every side; a constant image ties every tap, and the first tap
    # INSIDE the image wins: the padded row -1 / column -1 (at -inf) is skipped
    assert R.same_geometry(3, 3, 2) == (2, 1)
    x = _nhwc([[2, 2, 2], [2, 2, 2], [2, 2, 2]])
    dy = _nhwc([[1, 2], [4, 8]])
    r = R.maxpool_bwd(x, dy, 3, 2, 1, 1, BF)
    assert _hw(r.value) == [[1, 2, 0], [4, 8, 0], [0, 0, 0]]
    assert _hw(R.maxpool_fwd(x, 3, 2, 1, 1, 2, 2)) == [[2, 2], [2, 2]]
    # and on the even size the padded LAST row / column never wins against an equal earlier tap
    r4 = R.maxpool_bwd(_nhwc([[3] * 4] * 4), dy, 3, 2, 0, 0, BF)
    assert _hw(r4.value) == [[1, 0, 2, 0], [0, 0, 0, 0], [4, 0, 8, 0], [0, 0, 0, 0]]


def test_maxpool_2x2_on_an_odd_size_pads_after():
    assert R.same_geometry(7, 2, 2) == (4, 0) and R.same_geometry(10, 2, 2) == (5, 0) and R.same_geometry(7, 3, 2) == (4, 1)
    x = _nhwc([[1, 1, 4], [1, 1, 4], [6, 6, 5]])
    r = R.maxpool_bwd(x, _nhwc([[1, 2], [4, 8]]), 2, 2, 0, 0, BF)
    assert _hw(r.value) == [[1, 0, 2], [0, 0, 0], [4, 0, 8]]


def test_placement_references():
    x = torch.arange(2 * 3 * 16, dtype=R.F64).reshape(1, 2, 3, 16)
    y = R.depth_to_space2x(x)
    assert y.shape == (1, 4, 6, 4)
    for a in range(2):
        for b in range(2):
            assert torch.equal(y[:, a::2, b::2], x[..., (2 * a + b) * 4:(2 * a + b + 1) * 4])
    u = R.upsample_zero2x(x, 3, 6)
    assert torch.equal(u[:, ::2, ::2], x) and u.sum() == x.sum() and u.shape == (1, 3, 6, 16)
    v, a, n = R.reduce_rows(torch.tensor([[1.0, -2.0], [3.0, -4.0]], dtype=R.F64), 0.5)
    assert v.tolist() == [4.5, -5.5] and a.tolist() == [4.5, 6.5] and n == 3


# ---- BalanceFeatures backward against autograd ----------------------------------------------------------------------
@pytest.mark.parametrize("L,mid", [(5, 1), (5, 2), (3, 0)])
def test_balance_bwd_reference_against_float64_autograd(L, mid):
    g = torch.Generator().manual_seed(10 * L + mid)
    N, H0, W0, C = 2, 16, 32, 3
    shapes = [(N, H0 >> l, W0 >> l, C) for l in range(L)]
    # tie-free: a permutation per tensor, so autograd's argmax needs no tie rule
    ins = [torch.randperm(N * h * w * c, generator=g).to(R.F64).reshape(N, h, w, c) / 7.0 for (N, h, w, c) in shapes]
    avg = torch.randperm(N * (H0 >> mid) * (W0 >> mid) * C, generator=g).to(R.F64).reshape(shapes[mid]) / 5.0
    douts = [torch.randn(s, generator=g, dtype=R.F64) for s in shapes]
    davg, dins = R.balance_bwd(douts, ins, avg, mid, None)

    def nchw(t):
        return t.permute(0, 3, 1, 2)

    # (1) davg: the gradient of sum_l <resize_back_l(avg), dout_l> with respect to avg
    a = nchw(avg).clone().requires_grad_(True)
    loss = 0.0
    for l in range(L):
        f = 1 << abs(l - mid)
        back = a if l == mid else (F.interpolate(a, scale_factor=f, mode="nearest") if l < mid else F.max_pool2d(a, f))
        loss = loss + (back * nchw(douts[l])).sum()
    loss.backward()
    torch.testing.assert_close(nchw(davg.value), a.grad, rtol=1e-12, atol=1e-12)
    # (2) din_l: dout_l plus the gradient of <mean_l resize_l(in_l), davg> with respect to in_l
    leaves = [nchw(t).clone().requires_grad_(True) for t in ins]
    rs = []
    for l in range(L):
        f = 1 << abs(l - mid)
        rs.append(leaves[l] if l == mid else (F.max_pool2d(leaves[l], f) if l < mid else
                                              F.interpolate(leaves[l], scale_factor=f, mode="nearest")))
    ((sum(rs) / L) * a.grad).sum().backward()
    for l in range(L):
        torch.testing.assert_close(nchw(dins[l].value), nchw(douts[l]) + leaves[l].grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("act", ["relu", "relu6", "none"])
def test_topdown_bwd_reference_against_float64_autograd(act):
    g = torch.Generator().manual_seed(3)
    L, N, H0, W0, C = 3, 1, 4, 12, 2
    ins = [torch.randn((N, H0 >> l, W0 >> l, C), generator=g, dtype=R.F64) * 3 for l in range(L)]
    douts = [torch.randn(t.shape, generator=g, dtype=R.F64) for t in ins]
    leaves = [t.clone().requires_grad_(True) for t in ins]
    outs = [None] * L
    outs[L - 1] = leaves[L - 1]
    for l in range(L - 2, -1, -1):
        outs[l] = R.act_fwd(leaves[l] + R.up(outs[l + 1], 2), act)
    sum((o * d).sum() for o, d in zip(outs, douts)).backward()
    fwd = R.topdown_fwd(ins, act, None)
    for l in range(L):
        torch.testing.assert_close(fwd[l].value, outs[l].detach(), rtol=0, atol=0)
    dins = R.topdown_bwd(douts, [o.value for o in fwd[:-1]] + [None], [act] * (L - 1) + ["none"], None)
    for l in range(L):
        torch.testing.assert_close(dins[l].value, leaves[l].grad, rtol=1e-12, atol=1e-12)


# ---- teeth: wrong references are rejected, the right one is accepted -------------------------------------------------
def _balance_case(dtype, L=5, mid=1, N=2, H0=16, W0=48, C=24, seed=7):
    g = torch.Generator().manual_seed(seed)
    shapes = [(N, H0 >> l, W0 >> l, C) for l in range(L)]
    ins = [R.f64(R.grid(s, g, dtype)) for s in shapes]
    avg = R.f64(R.grid(shapes[mid], g, dtype))
    douts = [R.f64(R.grads(s, g, dtype)) for s in shapes]
    return douts, ins, avg


def _swap_hw(t):
    """the same buffer read as [N, W, H, C]"""
    return t.reshape(t.shape[0], t.shape[2], t.shape[1], t.shape[3])


@pytest.mark.parametrize("dtype", DTYPES)
def test_rule_rejects_wrong_balance_backward_references(dtype):
    L, mid = 5, 1
    douts, ins, avg = _balance_case(dtype)
    davg, dins = R.balance_bwd(douts, ins, avg, mid, dtype)
    w = R._windows(avg, 8)
    assert ((w == w.amax(-1, keepdim=True)).sum(-1) > 1).any(), "the coarsest level's windows must hold ties"

    def accepted(wrong):
        wd, wl = wrong
        return [R.accept(R.through_fp32(x, dtype), r, dtype) for x, r in zip([wd] + wl, [davg] + dins)]

    assert all(accepted((davg, dins))), "the unmodified reference, rounded through fp32, must pass"
    # the coarsest level's routing dropped: davg changes, and with it every level's din
    assert not any(accepted(R.balance_bwd(douts, ins, avg, mid, dtype, drop_level=L - 1)))
    # last maximum instead of first: davg (levels 2..4 route by avg) and din_0 (routes by in_0) change
    got = accepted(R.balance_bwd(douts, ins, avg, mid, dtype, pick="last"))
    assert not got[0] and not got[1], got
    # H and W exchanged: the same buffers decoded as [N, W, H, C]
    sw = R.balance_bwd([_swap_hw(t) for t in douts], [_swap_hw(t) for t in ins], _swap_hw(avg), mid, dtype)
    sw = (sw[0]._replace(value=_swap_hw(sw[0].value)), [r._replace(value=_swap_hw(r.value)) for r in sw[1]])
    assert not any(accepted(sw)[:4]), "every level with more than one row"
    # the argmax of the coarse levels taken from the wrong tensor (in instead of avg at the middle level)
    assert not accepted(R.balance_bwd(douts, ins, ins[mid], mid, dtype))[0]
    # davg left unrounded: NOT distinguishable, by the derivation (half a step, and every reader is granted a whole one)
    nr = R.balance_bwd(douts, ins, avg, mid, dtype, round_davg=False)
    assert all(R.accept(R.through_fp32(x, dtype), r, dtype) for x, r in zip(nr[1], dins))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 2])
def test_rule_rejects_wrong_maxpool_backward_references(dtype, k):
    g = torch.Generator().manual_seed(11)
    N, H, W, C = 2, 7, 10, 24
    (Ho, pt), (Wo, pl) = R.same_geometry(H, k, 2), R.same_geometry(W, k, 2)
    x, dy = R.f64(R.grid((N, H, W, C), g, dtype)), R.f64(R.grads((N, Ho, Wo, C), g, dtype))
    dx0 = R.f64(R.grads((N, H, W, C), g, dtype))
    assert not torch.equal(R.maxpool_argmax(x, k, 2, pt, pl, Ho, Wo), R.maxpool_argmax(x, k, 2, pt, pl, Ho, Wo, "last"))
    for base in (None, dx0):
        ref = R.maxpool_bwd(x, dy, k, 2, pt, pl, dtype, dx0=base)
        assert R.accept(R.through_fp32(ref, dtype), ref, dtype)
        last = R.maxpool_bwd(x, dy, k, 2, pt, pl, dtype, dx0=base, pick="last")
        assert not R.accept(R.through_fp32(last, dtype), ref, dtype)
        sw = R.maxpool_bwd(_swap_hw(x), _swap_hw(dy), k, 2, pl, pt, dtype, dx0=None if base is None else _swap_hw(base))
        assert not R.accept(_swap_hw(R.through_fp32(sw, dtype)), ref, dtype)
        if base is not None:   # accumulate ignored
            assert not R.accept(R.through_fp32(R.maxpool_bwd(x, dy, k, 2, pt, pl, dtype), dtype), ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["relu", "relu6"])
def test_rule_rejects_wrong_gates_of_the_topdown_backward(dtype, act):
    g = torch.Generator().manual_seed(5)
    L, N, H0, W0, C = 3, 2, 8, 20, 24
    ins = [R.f64(R.grid((N, H0 >> l, W0 >> l, C), g, dtype, lim=16)) for l in range(L)]
    fwd = R.topdown_fwd(ins, act, dtype)
    for l in range(L):
        assert R.accept(R.through_fp32(fwd[l], dtype), fwd[l], dtype)
    outs = [o.value for o in fwd[:-1]] + [None]
    acts = [act] * (L - 1) + ["none"]
    assert all((o == 0).any() for o in outs[:-1]) and (act == "relu" or all((o == 6).any() for o in outs[:-1]))
    douts = [R.f64(R.grads(t.shape, g, dtype)) for t in ins]
    ref = R.topdown_bwd(douts, outs, acts, dtype)
    assert all(R.accept(R.through_fp32(r, dtype), r, dtype) for r in ref)
    lo = R.topdown_bwd(douts, outs, acts, dtype, lo_inclusive=True)       # z >= 0 instead of z > 0
    assert not any(R.accept(R.through_fp32(w, dtype), r, dtype) for w, r in zip(lo[:-1], ref[:-1]))
    if act == "relu6":
        hi = R.topdown_bwd(douts, outs, acts, dtype, hi_inclusive=True)   # z <= 6 instead of z < 6
        assert not any(R.accept(R.through_fp32(w, dtype), r, dtype) for w, r in zip(hi[:-1], ref[:-1]))
    sw = R.topdown_bwd([_swap_hw(t) for t in douts], [None if o is None else _swap_hw(o) for o in outs], acts, dtype)
    assert not any(R.accept(_swap_hw(R.through_fp32(w, dtype)), r, dtype) for w, r in zip(sw[1:], ref[1:]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,mid,N,H0,W0,C", [(5, 1, 2, 16, 48, 24), (5, 2, 1, 16, 32, 16), (3, 0, 1, 16, 32, 16),
                                             (6, 1, 1, 32, 64, 8)])
def test_references_rounded_through_fp32_stay_inside_the_rule(dtype, L, mid, N, H0, W0, C):
    douts, ins, avg = _balance_case(dtype, L, mid, N, H0, W0, C, seed=L * 10 + mid)
    davg, dins = R.balance_bwd(douts, ins, avg, mid, dtype)
    for r in [davg] + dins:
        assert R.accept(R.through_fp32(r, dtype), r, dtype)
    favg, fouts = R.balance_fwd(ins, mid, dtype)
    for r in [favg] + fouts:
        assert R.accept(R.through_fp32(r, dtype), r, dtype)
    g = torch.Generator().manual_seed(1)
    y0, x = R.f64(R.grads((N, H0, W0, C), g, dtype)), R.f64(R.grads((N, H0 // 2, W0 // 2, C), g, dtype))
    s = R.scatter_add2x(x, y0, dtype)
    assert R.accept(R.through_fp32(s, dtype), s, dtype) and not R.accept(y0, s, dtype)
