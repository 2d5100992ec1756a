"""The small NHWC kernels around the convolutions against float64 references of their own operation (pyramid_ref.py):
max-pool forward / backward, the FPN top-down pass forward / backward, BalanceFeatures forward / backward, the stride-2
placement kernels, the activation gate, the casts and the row reduction — at odd and non-square sizes, channel-group
counts that are no power of two (24, 112 channels: 3 and 14 groups), inputs full of ties, and shapes that reach the
32-bit-division index decode (`rn_decode4` mode 1, from 2^22 pixels up) and more than one grid sweep.

Acceptance (derivation in pyramid_ref.py): every element, without exception,
    |got - ref| <= ulp_s(ref) + n 2^-23 sum|terms| (+ one storage step of every rounded intermediate the element reads,
                                                     scaled as the formula scales it)
with ulp_s(ref) = eps max(|ref|, smallest normal), eps = 2^-7 (bfloat16) or 2^-10 (half), n the fp32 operations of the
element and sum|terms| computed by the reference.  Data movement and routing (max-pool forward, upsample, depth-to-space
without accumulate, the casts, the activation gate) is compared bit for bit.

Inputs: activations and `avg` from a coarse grid (integers / 4) so that windows tie all the time and relu6 meets exact
0 and 6; gradients from randn rounded to storage.  Every test asserts its own precondition — ties exist, the decode mode
is the intended one (computed as the launch computes it), the window is 16 wide — so that a later change of shape cannot
turn it into a repeat of the easy case."""
import pytest
import torch

import pyramid_ref as R

pytestmark = pytest.mark.gpu

# The 16-bit storage type under test, set per test from its `build` parameter (as in test_gpu_train_kernels.py)
H16 = torch.bfloat16
_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
BUILDS = ["bf16", "f16"]
SWEEP = 8192 * 256          # threads of the largest grid these kernels launch: more items than this = a second pass


@pytest.fixture(autouse=True)
def _storage_type(request):
    global H16
    params = request.node.callspec.params if hasattr(request.node, "callspec") else {}
    H16 = _DT[params.get("build", "bf16")]
    yield
    H16 = torch.bfloat16


def _lib():
    from retinanet import _C
    return _C.lib(H16 == torch.float16)


def decode_mode(total, C8):
    """rn_decode_mode (csrc/rn_common.h) of a launch over `total` 16-byte items"""
    return 0 if total >= (1 << 31) else (2 if total < (C8 << 22) else 1)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _within(got, ref, what):
    """print the figure, then assert the rule on every element"""
    ok, ratio, outside = R.check(got.cpu(), ref, H16)
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f}, {outside} of {got.numel()} elements outside")
    assert ok, (what, ratio, outside)


def _tied_windows(x, k, stride, pt, pl, Ho, Wo):
    return not torch.equal(R.maxpool_argmax(x, k, stride, pt, pl, Ho, Wo, "first"),
                           R.maxpool_argmax(x, k, stride, pt, pl, Ho, Wo, "last"))


# ---- max-pool -----------------------------------------------------------------------------------------------------------
def _run_maxpool(cuda, x, k, stride, pt, pl, Ho, Wo):
    from retinanet import _C
    N, H, W, C = x.shape
    y = torch.empty((N, Ho, Wo, C), dtype=H16, device=cuda)
    xd = x.to(cuda)
    _C.check(_lib().rn_maxpool2d_nhwc(_C.ptr(xd), _C.ptr(y), N, H, W, C, k, stride, pt, pl, Ho, Wo, _C.current_stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _run_maxpool_bwd(cuda, x, dy, k, stride, pt, pl, base):
    from retinanet import _C
    N, H, W, C = x.shape
    xd, dyd = x.to(cuda), dy.to(cuda)
    dx = torch.empty_like(xd) if base is None else base.to(cuda).clone()
    _C.check(_lib().rn_maxpool2d_nhwc_bwd(_C.ptr(xd), _C.ptr(dyd), _C.ptr(dx), N, H, W, C, k, stride, pt, pl,
                                          dy.shape[1], dy.shape[2], 0 if base is None else 1, _C.current_stream()))
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("k", [3, 2])
@pytest.mark.parametrize("N,H,W,C", [(2, 7, 10, 24), (3, 12, 20, 8)])
def test_maxpool_forward_backward(cuda, build, N, H, W, C, k):
    """3x3 / stride 2 SAME (pad 0 top/left on the even size, 1 on the odd one) and 2x2 / stride 2, odd and non-square,
    3 channel groups; the backward routes to the FIRST maximum of windows full of ties, with and without accumulate."""
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + k)
    (Ho, pt), (Wo, pl) = R.same_geometry(H, k, 2), R.same_geometry(W, k, 2)
    assert (pt, pl) == ((H % 2, W % 2) if k == 3 else (0, 0))
    x, dy, base = R.grid((N, H, W, C), g, H16), R.grads((N, Ho, Wo, C), g, H16), R.grads((N, H, W, C), g, H16)
    assert H != W and _tied_windows(R.f64(x), k, 2, pt, pl, Ho, Wo), "non-square, and first / last maximum differ"
    assert decode_mode(N * H * W * (C // 8), C // 8) == 2
    assert torch.equal(_run_maxpool(cuda, x, k, 2, pt, pl, Ho, Wo).float(), R.maxpool_fwd(x.float(), k, 2, pt, pl, Ho, Wo))
    for b in (None, base):
        ref = R.maxpool_bwd(R.f64(x), R.f64(dy), k, 2, pt, pl, H16, dx0=None if b is None else R.f64(b))
        _within(_run_maxpool_bwd(cuda, x, dy, k, 2, pt, pl, b), ref, f"maxpool_bwd k={k} accumulate={b is not None}")


@pytest.mark.parametrize("build", BUILDS)
def test_maxpool_decode_with_32bit_divisions(cuda, build):
    """N=1, 2048 x 2056, C=8: 4 210 688 pixels >= 2^22 is decode mode 1, and more than one grid sweep.  The backward
    (one thread per INPUT pixel) at the stem's 3x3 / stride 2; the forward (one thread per OUTPUT pixel) needs an output
    that large, so it runs 2x2 / stride 1."""
    g = torch.Generator().manual_seed(77)
    N, H, W, C = 1, 2048, 2056, 8
    x = R.grid((N, H, W, C), g, H16)
    total = N * H * W * (C // 8)
    assert decode_mode(total, C // 8) == 1 and total > SWEEP
    Ho, Wo = H - 1, W - 1
    assert decode_mode(N * Ho * Wo * (C // 8), C // 8) == 1 and N * Ho * Wo * (C // 8) > SWEEP
    assert torch.equal(_run_maxpool(cuda, x, 2, 1, 0, 0, Ho, Wo).float(), R.maxpool_fwd(x.float(), 2, 1, 0, 0, Ho, Wo))
    (Ho, pt), (Wo, pl) = R.same_geometry(H, 3, 2), R.same_geometry(W, 3, 2)
    dy = R.grads((N, Ho, Wo, C), g, H16)
    ref = R.maxpool_bwd(R.f64(x), R.f64(dy), 3, 2, pt, pl, H16)
    _within(_run_maxpool_bwd(cuda, x, dy, 3, 2, pt, pl, None), ref, "maxpool_bwd mode 1")
    torch.cuda.empty_cache()


# ---- FPN top-down -----------------------------------------------------------------------------------------------------
def _run_topdown(cuda, ins, act):
    from retinanet import _C
    L, (N, H0, W0, C) = len(ins), ins[0].shape
    ind = [t.to(cuda) for t in ins]
    outs = [torch.empty_like(t) for t in ind[:-1]] + [ind[-1]]
    _C.check(_lib().rn_fpn_topdown(_C.ptr_array(ind), _C.ptr_array(outs), L, N, H0, W0, C, _C.ACT_IDS[act],
                                   _C.current_stream()))
    torch.cuda.synchronize()
    return outs


def _run_topdown_bwd(cuda, douts, outs, acts):
    """level by level, the finest first, every level reading the kernel's own finer din: as the engine chains it"""
    from retinanet import _C
    L, (N, H0, W0, C) = len(douts), douts[0].shape
    dd = [t.to(cuda) for t in douts]
    od = [None if o is None else o.to(cuda) for o in outs]
    din = [torch.empty_like(t) for t in dd]
    for l in range(L):
        _C.check(_lib().rn_fpn_topdown_bwd_level(_C.ptr(dd[l]), _C.ptr(din[l - 1]) if l else None, _C.ptr(od[l]),
                                                 _C.ptr(din[l]), N, H0 >> l, W0 >> l, C, _C.ACT_IDS[acts[l]],
                                                 _C.current_stream()))
    torch.cuda.synchronize()
    return din


def _topdown_case(cuda, L, N, H0, W0, C, act, seed):
    g = torch.Generator().manual_seed(seed)
    ins = [R.grid((N, H0 >> l, W0 >> l, C), g, H16, lim=16) for l in range(L)]
    fwd = R.topdown_fwd([R.f64(t) for t in ins], act, H16)
    got = _run_topdown(cuda, ins, act)
    for l in range(L):
        _within(got[l], fwd[l], f"fpn_topdown {act} level {l}")
    # the backward on the reference's own forward outputs (given tensors), gate none on the coarsest level
    outs = [o.value.to(H16) for o in fwd[:-1]] + [None]
    acts = [act] * (L - 1) + ["none"]
    if act != "none":
        assert all((o == 0).any() for o in outs[:-1]), "the gate's lower edge z == 0 must occur"
    if act == "relu6":
        assert all((o == 6).any() for o in outs[:-1]), "the gate's upper edge z == 6 must occur"
    douts = [R.grads(t.shape, g, H16) for t in ins]
    ref = R.topdown_bwd([R.f64(t) for t in douts], [None if o is None else R.f64(o) for o in outs], acts, H16)
    din = _run_topdown_bwd(cuda, douts, outs, acts)
    for l in range(L):
        _within(din[l], ref[l], f"fpn_topdown_bwd {act} level {l}")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("act", ["relu", "relu6", "none"])
def test_fpn_topdown_forward_backward(cuda, build, act):
    L, N, H0, W0, C = 3, 2, 8, 20, 24
    assert (C // 8) & (C // 8 - 1) and H0 != W0
    _topdown_case(cuda, L, N, H0, W0, C, act, 31)


@pytest.mark.parametrize("build", BUILDS)
def test_fpn_topdown_five_levels_14_channel_groups(cuda, build):
    assert (112 // 8) & (112 // 8 - 1)
    _topdown_case(cuda, 5, 1, 16, 48, 112, "relu6", 32)


def _large_pyramid():
    L, N, H0, C = 5, 1, 1792, 8
    begin = [0]
    for l in range(L):
        begin.append(begin[-1] + N * (H0 >> l) * (H0 >> l) * (C // 8))
    assert begin[L] == 4277504
    return L, N, H0, C, begin


@pytest.mark.parametrize("build", BUILDS)
def test_fpn_topdown_large_pyramid_forward(cuda, build):
    """L=5, N=1, 1792 x 1792, C=8: 4 277 504 items.  rn_fpn_topdown cuts it into one-stage launches (finest level >= 2^21
    items); its first launch (levels 2 and 3, item numbers up to begin[4]) decodes in mode 1, and the launch of the finest
    level makes more than one grid sweep."""
    L, N, H0, C, begin = _large_pyramid()
    assert begin[1] >= (1 << 21), "the staged-launch branch"
    assert decode_mode(begin[L - 1], C // 8) == 1, "the launch of levels [2, L - 1)"
    assert begin[1] > SWEEP
    g = torch.Generator().manual_seed(33)
    ins = [R.grid((N, H0 >> l, H0 >> l, C), g, H16, lim=16) for l in range(L)]
    fwd = R.topdown_fwd([R.f64(t) for t in ins], "relu6", H16)
    got = _run_topdown(cuda, ins, "relu6")
    for l in range(L):
        _within(got[l], fwd[l], f"fpn_topdown large level {l}")
    torch.cuda.empty_cache()


@pytest.mark.parametrize("build", BUILDS)
def test_fpn_topdown_large_pyramid_backward(cuda, build):
    """The same pyramid through rn_fpn_topdown_bwd_level: the finest level makes more than one grid sweep.  (Each level is
    a launch of its own over fewer than 2^22 pixels, so these stay in decode mode 2: mode 1 would need a level of 2^22
    pixels under a finer one of 2^24.)  `out` is a given tensor here: relu6 of a grid, with exact 0 and 6."""
    L, N, H0, C, begin = _large_pyramid()
    assert begin[1] > SWEEP and decode_mode(begin[1], C // 8) == 2
    g = torch.Generator().manual_seed(34)
    outs = [R.grid((N, H0 >> l, H0 >> l, C), g, H16, lim=32).clamp_(0.0, 6.0) for l in range(L - 1)] + [None]
    assert all((o == 0).any() and (o == 6).any() for o in outs[:-1])
    acts = ["relu6"] * (L - 1) + ["none"]
    douts = [R.grads((N, H0 >> l, H0 >> l, C), g, H16) for l in range(L)]
    ref = R.topdown_bwd([R.f64(t) for t in douts], [None if o is None else R.f64(o) for o in outs], acts, H16)
    din = _run_topdown_bwd(cuda, douts, outs, acts)
    for l in range(L):
        _within(din[l], ref[l], f"fpn_topdown_bwd large level {l}")
    torch.cuda.empty_cache()


# ---- BalanceFeatures --------------------------------------------------------------------------------------------------
def _balance_inputs(L, mid, N, H0, W0, C, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(N, H0 >> l, W0 >> l, C) for l in range(L)]
    ins = [R.grid(s, g, H16) for s in shapes]
    avg = R.grid(shapes[mid], g, H16)      # independent of `ins`: an argmax taken from the wrong tensor shows
    douts = [R.grads(s, g, H16) for s in shapes]
    return ins, avg, douts


def _balance_forward(cuda, ins, mid):
    from retinanet import _C
    L, (N, H0, W0, C) = len(ins), ins[0].shape
    ind = [t.to(cuda) for t in ins]
    outs = [torch.empty_like(t) for t in ind]
    scratch = torch.empty_like(ind[mid])
    _C.check(_lib().rn_balance_features(_C.ptr_array(ind), _C.ptr_array(outs), L, mid, N, H0, W0, C, _C.ptr(scratch),
                                        _C.current_stream()))
    torch.cuda.synchronize()
    avg, ref = R.balance_fwd([R.f64(t) for t in ins], mid, H16)
    _within(scratch, avg, "balance_features avg")
    for l in range(L):
        _within(outs[l], ref[l], f"balance_features level {l}")


def _balance_backward(cuda, ins, avg, douts, mid):
    from retinanet import _C
    lib = _lib()
    L, (N, H0, W0, C) = len(ins), ins[0].shape
    dd, ind, avd = [t.to(cuda) for t in douts], [t.to(cuda) for t in ins], avg.to(cuda)
    din = [torch.empty_like(t) for t in dd]
    nbytes = lib.rn_balance_features_bwd_scratch_bytes(L, mid, N, H0, W0, C)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=cuda)
    _C.check(lib.rn_balance_features_bwd(_C.ptr_array(dd), _C.ptr_array(ind), _C.ptr_array(din), _C.ptr(avd),
                                         _C.ptr(scratch), nbytes, L, mid, N, H0, W0, C, _C.current_stream()))
    torch.cuda.synchronize()
    davg, ref = R.balance_bwd([R.f64(t) for t in douts], [R.f64(t) for t in ins], R.f64(avg), mid, H16)
    # the scratch starts with davg in the storage type, [N, H0 >> mid, W0 >> mid, C]
    _within(scratch[:avg.numel() * 2].view(H16).reshape(avg.shape), davg, "balance_features_bwd davg")
    for l in range(L):
        _within(din[l], ref[l], f"balance_features_bwd level {l}")


def _has_tied_windows(t, f):
    w = R._windows(R.f64(t), f)
    return bool(((w == w.amax(-1, keepdim=True)).sum(-1) > 1).any())


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("L,mid,N,H0,W0,C", [
    (5, 1, 2, 16, 48, 24),    # the product's form, the <1, 5> kernels; 3 channel groups
    (5, 2, 1, 16, 32, 16),    # the generic kernels
    (3, 0, 1, 16, 32, 16),    # the generic kernels, nothing finer than the middle
    (6, 1, 1, 32, 64, 8)])    # 16 x 16 windows: the second group of eight columns of the argmax loader
def test_balance_features_forward_backward(cuda, build, L, mid, N, H0, W0, C):
    ins, avg, douts = _balance_inputs(L, mid, N, H0, W0, C, 100 * L + mid)
    assert H0 != W0 and _has_tied_windows(avg, 2) and (mid == 0 or _has_tied_windows(ins[0], 1 << mid))
    if L == 6:
        assert 1 << (L - 1 - mid) == 16, "the coarsest level's window must be 16 wide"
        # a maximum whose FIRST occurrence lies in columns 8..15 of a window row: the second group decides
        w = R._windows(R.f64(avg), 16)
        first = R._first(w == w.amax(-1, keepdim=True)).to(torch.int64).argmax(-1)
        assert ((first % 16) >= 8).any()
    _balance_forward(cuda, ins, mid)
    _balance_backward(cuda, ins, avg, douts, mid)


@pytest.mark.parametrize("build", BUILDS)
def test_balance_features_backward_decode_with_32bit_divisions(cuda, build):
    """L=5, mid=1, N=1, 1792 x 1792, C=8: the din launch runs over 4 277 504 items >= 2^22: decode mode 1, two sweeps."""
    L, mid, N, H0, C = 5, 1, 1, 1792, 8
    total = sum(N * (H0 >> l) * (H0 >> l) * (C // 8) for l in range(L))
    assert decode_mode(total, C // 8) == 1 and total > SWEEP
    ins, avg, douts = _balance_inputs(L, mid, N, H0, H0, C, 55)
    _balance_backward(cuda, ins, avg, douts, mid)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("build", BUILDS)
def test_balance_features_backward_refusals(cuda, build):
    """a short scratch is RN_ENOMEM and levels that do not halve exactly are RN_EINVAL, both before anything is launched:
    the outputs and the scratch keep their contents"""
    from retinanet import _C
    lib = _lib()
    L, mid, N, C = 5, 1, 1, 8
    for H0, W0, want in [(16, 48, _C.RN_ENOMEM), (24, 48, _C.RN_EINVAL), (16, 56, _C.RN_EINVAL)]:
        ins, avg, douts = _balance_inputs(L, mid, N, H0, W0, C, 9)     # every level is [H0 >> l, W0 >> l], as a launch would read it
        dd, ind, avd = [t.to(cuda) for t in douts], [t.to(cuda) for t in ins], avg.to(cuda)
        din = [torch.full_like(t, 3.0) for t in dd]
        nbytes = lib.rn_balance_features_bwd_scratch_bytes(L, mid, N, H0, W0, C)
        assert nbytes > avg.numel() * 2, "davg and the argmax bytes of the coarse levels"
        scratch = torch.zeros((nbytes,), dtype=torch.uint8, device=cuda)
        claim = nbytes - 1 if want == _C.RN_ENOMEM else nbytes
        assert lib.rn_balance_features_bwd(_C.ptr_array(dd), _C.ptr_array(ind), _C.ptr_array(din), _C.ptr(avd),
                                           _C.ptr(scratch), claim, L, mid, N, H0, W0, C, _C.current_stream()) == want
        assert (b"scratch too small" if want == _C.RN_ENOMEM else b"halve exactly") in lib.rn_last_error()
        torch.cuda.synchronize()
        assert all(bool((t == 3.0).all()) for t in din) and not scratch.any()
    assert lib.rn_balance_features_bwd_scratch_bytes(1, 0, N, 16, 48, C) == 0


# ---- stride-2 placement -------------------------------------------------------------------------------------------------
def _run_scatter(cuda, x, y0, accumulate, entry="rn_scatter_add2x"):
    from retinanet import _C
    N, H, W, C = x.shape
    xd, yd = x.to(cuda), y0.to(cuda).clone()
    a = (_C.ptr(xd), _C.ptr(yd), N, H, W, C, y0.shape[1], y0.shape[2])
    if entry == "rn_scatter_add2x":
        _C.check(_lib().rn_scatter_add2x(*a, accumulate, _C.current_stream()))
    else:
        _C.check(_lib().rn_upsample_zero2x(*a, _C.current_stream()))
    torch.cuda.synchronize()
    return yd.cpu()


@pytest.mark.parametrize("build", BUILDS)
def test_upsample_and_scatter_add_non_square(cuda, build):
    g = torch.Generator().manual_seed(41)
    N, H, W, C = 2, 5, 7, 24
    x = R.grads((N, H, W, C), g, H16)
    for Ho in (2 * H - 1, 2 * H):
        for Wo in (2 * W - 1, 2 * W):
            y0 = R.grads((N, Ho, Wo, C), g, H16)
            want = _bits(R.upsample_zero2x(x, Ho, Wo))
            assert torch.equal(_bits(_run_scatter(cuda, x, y0, 0, "rn_upsample_zero2x")), want), (Ho, Wo)
            assert torch.equal(_bits(_run_scatter(cuda, x, y0, 0)), want), (Ho, Wo)
            ref = R.scatter_add2x(R.f64(x), R.f64(y0), H16)
            got = _run_scatter(cuda, x, y0, 1)
            _within(got, ref, f"scatter_add2x {Ho}x{Wo}")
            keep = torch.ones((Ho, Wo), dtype=torch.bool)
            keep[::2, ::2] = False
            assert torch.equal(_bits(got)[:, keep], _bits(y0)[:, keep]), "the other positions are not touched"


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("C", [8, 24])
def test_upsample_decode_with_32bit_divisions(cuda, build, C):
    """2048 x 2056 output pixels (>= 2^22): mode 1 at one channel group and at three"""
    g = torch.Generator().manual_seed(42)
    N, H, W = 1, 1024, 1028
    Ho, Wo = 2 * H, 2 * W
    total = N * Ho * Wo * (C // 8)
    assert decode_mode(total, C // 8) == 1 and total > SWEEP
    x = R.grads((N, H, W, C), g, H16)
    got = _run_scatter(cuda, x, torch.ones((N, Ho, Wo, C), dtype=H16), 0, "rn_upsample_zero2x")
    assert torch.equal(_bits(got), _bits(R.upsample_zero2x(x, Ho, Wo)))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("build", BUILDS)
def test_scatter_add_decode_with_32bit_divisions(cuda, build):
    """one thread per INPUT pixel: 2048 x 2056 of them, into 4095 x 4111"""
    g = torch.Generator().manual_seed(43)
    N, H, W, C = 1, 2048, 2056, 8
    Ho, Wo = 2 * H - 1, 2 * W - 1
    assert decode_mode(N * H * W * (C // 8), C // 8) == 1 and N * H * W * (C // 8) > SWEEP
    x = R.grads((N, H, W, C), g, H16)
    # positive finite bit patterns: cheaper to draw than 135 M normal deviates
    y0 = torch.randint(0x3800, 0x4100, (N, Ho, Wo, C), generator=g, dtype=torch.int16).view(H16)
    got = _run_scatter(cuda, x, y0, 1)
    even = R.f64(y0[:, ::2, ::2])
    want = R.Ref(R.round_storage(even + R.f64(x), H16), even.abs() + R.f64(x).abs(), 2)
    _within(got[:, ::2, ::2], want, "scatter_add2x mode 1")
    got[:, ::2, ::2] = y0[:, ::2, ::2]
    assert torch.equal(_bits(got), _bits(y0)), "the other positions are not touched"
    torch.cuda.empty_cache()


def _run_d2s(cuda, x, y0, accumulate):
    from retinanet import _C
    N, H, W, C4 = x.shape
    xd, yd = x.to(cuda), y0.to(cuda).clone()
    _C.check(_lib().rn_depth_to_space2x(_C.ptr(xd), _C.ptr(yd), N, H, W, C4 // 4, accumulate, _C.current_stream()))
    torch.cuda.synchronize()
    return yd.cpu()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("N,H,W,C", [(2, 5, 7, 24), (1, 1024, 1028, 8)])
def test_depth_to_space(cuda, build, N, H, W, C):
    g = torch.Generator().manual_seed(44)
    total = N * H * W * 4 * (C // 8)
    assert decode_mode(total, C // 8) == (1 if H > 1000 else 2) and (H < 1000 or total > SWEEP) and H != W
    x, y0 = R.grads((N, H, W, 4 * C), g, H16), R.grads((N, 2 * H, 2 * W, C), g, H16)
    assert torch.equal(_bits(_run_d2s(cuda, x, y0, 0)), _bits(R.depth_to_space2x(x)))
    _within(_run_d2s(cuda, x, y0, 1), R.depth_to_space2x_add(R.f64(x), R.f64(y0), H16), "depth_to_space2x accumulate")
    torch.cuda.empty_cache()


# ---- the activation gate, the casts, the row sum ----------------------------------------------------------------------
def _neighbours_of_six():
    six = torch.tensor([6.0], dtype=H16).view(torch.int16)
    return torch.cat([six - 1, six, six + 1]).view(H16)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("act", ["relu", "relu6", "none"])
@pytest.mark.parametrize("n", [8, 8 * ((1 << 21) + 3)])
def test_act_bwd(cuda, build, act, n):
    """dy = dz * mask(z), bit for bit; z at +-0, the smallest positive storage value, 6 and its two storage neighbours —
    in the first eight elements and again in the last eight, which the large case reaches only in its second sweep"""
    from retinanet import _C
    assert n // 8 <= SWEEP if n == 8 else n // 8 > SWEEP
    g = torch.Generator().manual_seed(45)
    tiny = torch.tensor([1], dtype=torch.int16).view(H16)     # the smallest positive (subnormal) value
    edge = torch.cat([torch.tensor([0.0, -0.0], dtype=H16), tiny, _neighbours_of_six(), torch.tensor([-1.0, 1.0], dtype=H16)])
    assert edge.numel() == 8 and edge[2].item() > 0 and edge[3].item() < 6 < edge[5].item()
    z = R.grid((n,), g, H16, lim=32)
    z[:8], z[-8:] = edge, edge
    dz = R.grads((n,), g, H16)
    assert (dz[:8] != 0).all()
    zd, dzd = z.to(cuda), dz.to(cuda)
    dy = torch.empty_like(dzd)
    _C.check(_lib().rn_act_bwd(_C.ptr(dzd), _C.ptr(zd), _C.ptr(dy), n, _C.ACT_IDS[act], _C.current_stream()))
    torch.cuda.synchronize()
    want = dz * R.act_mask(z.float(), act).to(H16)            # a product with 0 or 1: exact, the sign of a zero included
    if act == "relu6":
        assert want[:8].ne(0).tolist() == [False, False, True, True, False, False, False, True]
    assert torch.equal(_bits(dy.cpu()), _bits(want))
    torch.cuda.empty_cache()


def _cast_inputs(g, P, C):
    fi = torch.finfo(H16)
    eps, tn, big = float(fi.eps), float(fi.smallest_normal), float(fi.max)
    j = torch.arange(0, 32, dtype=torch.float32)
    special = torch.cat([1.0 + (2 * j + 1) * eps / 2, -(6.0 + (2 * j + 1) * eps * 2),      # exact midpoints: ties to even
                         torch.tensor([0.0, -0.0, big, -big, float("inf"), float("-inf")]),
                         tn * (j + 1) / 32, -tn * (2 * j + 1) / 4096,                       # subnormals of the storage type
                         torch.tensor([big * (1 + eps / 4), -big * (1 + eps / 4)])])        # still rounds to the largest finite
    x = torch.randn((P * C,), generator=g) * 4
    x[:special.numel()] = special
    x[-special.numel():] = special.flip(0)
    return x.reshape(P, C)


@pytest.mark.parametrize("build", BUILDS)
def test_cast_f32_to_storage(cuda, build):
    from retinanet import _C
    x = _cast_inputs(torch.Generator().manual_seed(46), 33, 36)
    want = x.to(H16)
    assert want.isinf().sum() == 4 and (want.float().abs() == float(torch.finfo(H16).max)).sum() == 8
    assert ((want.float() != 0) & (want.float().abs() < float(torch.finfo(H16).smallest_normal))).any()
    xd = x.to(cuda)
    y = torch.empty(x.shape, dtype=H16, device=cuda)
    _C.check(_lib().rn_cast_f32_to_bf16(_C.ptr(xd), _C.ptr(y), x.numel(), _C.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(_bits(y.cpu()), _bits(want))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("C,Cpad", [(36, 64), (9, 12)])
def test_cast_pad_f32_to_storage(cuda, build, C, Cpad):
    from retinanet import _C
    P = 37
    x = _cast_inputs(torch.Generator().manual_seed(47), P, C)
    xd = x.to(cuda)
    y = torch.full((P, Cpad), 5.0, dtype=H16, device=cuda)
    _C.check(_lib().rn_cast_pad_f32_to_bf16(_C.ptr(xd), _C.ptr(y), P, C, Cpad, _C.current_stream()))
    torch.cuda.synchronize()
    y = y.cpu()
    assert torch.equal(_bits(y[:, :C]), _bits(x.to(H16)))
    assert not _bits(y[:, C:]).any(), "the padded columns are +0"


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("n", [1, 257])
def test_reduce_rows(cuda, rows, n):
    """dst[c] = add + sum_r src[r * stride + c], an fp32 sum of rows + 1 terms: |got - ref| <= (rows + 1) 2^-23 sum|terms|;
    the rows are added in index order, so two runs agree bit for bit.  (No 16-bit tensor: one build.)"""
    from retinanet import _C
    g = torch.Generator().manual_seed(rows * 1000 + n)
    stride, add = n + 3, 0.75
    src = torch.randn((rows, stride), generator=g) * 100
    sd = src.to(cuda)
    got = []
    for _ in range(2):
        dst = torch.full((n + 1,), -7.0, device=cuda)
        _C.check(_lib().rn_reduce_rows_f32(_C.ptr(sd), rows, stride, n, add, _C.ptr(dst), _C.current_stream()))
        torch.cuda.synchronize()
        got.append(dst.cpu())
    assert torch.equal(got[0], got[1]) and got[0][n].item() == -7.0, "deterministic; nothing written past n"
    ref, terms, nt = R.reduce_rows(R.f64(src[:, :n]), add)
    err = (R.f64(got[0][:n]) - ref).abs()
    print("reduce_rows: worst error / bound", float((err / (nt * 2.0 ** -23 * terms)).max()))
    assert nt == rows + 1 and bool((err <= nt * 2.0 ** -23 * terms).all())
