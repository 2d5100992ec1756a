"""GPU parity of the training kernels (backward of a5-a8, a10) against PyTorch-CPU autograd in
float32 on the same bf16-rounded inputs."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


# The 16-bit storage type under test: a test parametrized with build="f16" runs on librnet_hip_f16.so (-DRN_F16, IEEE half)
# with half tensors; everything else on the bfloat16 build.  Set per test from its own parameters by the autouse fixture.
H16 = torch.bfloat16
_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
BUILDS = ["bf16", "f16"]


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


def _bf(x):
    return x.to(H16)


def _ws(nbytes, dev):
    # zeros: the workspaces of the BatchNorm passes and the split-K convolutions hold ticket counters that start at zero
    return torch.zeros((max(int(nbytes), 256),), dtype=torch.uint8, device=dev)


# ---------------------------------------------------------------------------------------------
WGRAD_SHAPES = [
    # list of (N, H, Cin, Cout) segments, k, stride
    ([(2, 12, 128, 128)], 3, 1),
    ([(2, 16, 256, 128)], 1, 1),
    ([(1, 16, 128, 256)], 3, 2),
    ([(2, 8, 256, 36)], 3, 1),                                   # box prediction conv (Cout tail)
    ([(2, s, 256, 256) for s in (8, 4, 2, 1)], 3, 1),            # shared head conv over a pyramid
    ([(1, 10, 192, 720)], 3, 1),                                 # Cin tail tile, 6 co tiles (2 lockstep groups)
    ([(1, 6, 256, 640)], 3, 1),                                  # 5 co tiles in groups of 3 + 2 (padding tile)
    ([(2, s, 256, 256) for s in (80, 40, 20, 10, 5)], 3, 1),     # 256x256-tile kernel: shared head conv, 5 levels
    ([(2, 64, 256, 720)], 3, 1),                                 # 256x256-tile kernel: 3 co tiles, Cout tail
    ([(3, 48, 512, 256)], 1, 1),                                 # 256x256-tile kernel: 1x1, 2 ci tiles
    ([(2, 96, 256, 512)], 3, 2),                                 # 256x256-tile kernel: stride 2
    # wgrad_halo_kernel (3x3 / stride 1 / pad 1, all nine taps per workgroup, reduction over image rows)
    ([(3, 9, 64, 64)], 3, 1),                                    # one column strip with a tail (W = 9 < 16), odd H, N = 3
    ([(2, 13, 128, 136)], 3, 1),                                 # Cout tail inside the second 128-wide co tile (136 = 128 + 8)
    ([(1, 40, 128, 256), (2, 17, 128, 256), (5, 1, 128, 256)], 3, 1),   # segments: W = 40 (2.5 strips), 17 (tail of 1), H = W = 1
    ([(2, 33, 512, 64)], 3, 1),                                  # 8 ci tiles, W = 33 (third strip holds one column)
]
# square images in the list above; the halo cases add non-square ones below through _WGRAD_HW
_WGRAD_HW = {"halo_w9": (9, 9), "halo_co136": (11, 13), "halo_segs": None, "halo_ci512": (6, 33)}


_WGRAD_IDS = ["3x3", "1x1", "3x3s2", "pred36", "pyramid", "cin192_720", "co640", "big_pyramid", "big_720", "big_1x1",
              "big_s2", "halo_w9", "halo_co136", "halo_segs", "halo_ci512"]
# (build, shape, rn_launch_opts.wgrad_kernel, wgrad_target_blocks, kernel that must run: 0 = wgrad_kernel, 1 = wgrad_big_kernel,
# 2 = wgrad_halo_kernel).  The first seven shapes at these sizes: the dispatcher's own choice (the 128-tile kernel).
_WGRAD_CASES = ([("bf16", i, 0, 0, 0) for i in _WGRAD_IDS[:7]] + [("f16", _WGRAD_IDS[i], 0, 0, 0) for i in (0, 1, 2, 3, 4)]
                + [("bf16", "big_pyramid", 2, 0, 2), ("bf16", "big_720", 2, 0, 2), ("f16", "big_pyramid", 2, 0, 2),
                   ("f16", "big_720", 2, 0, 2),                       # 3x3 / stride 1: the halo kernel
                   ("bf16", "big_pyramid", 3, 0, 1), ("bf16", "big_720", 3, 0, 1), ("f16", "big_pyramid", 3, 0, 1),
                   ("bf16", "big_1x1", 2, 0, 1), ("bf16", "big_s2", 2, 0, 1), ("f16", "big_1x1", 2, 0, 1)]
                # halo kernel: tails, segments, and split-K plans from one chunk to many short ones (chunk boundaries in
                # the middle of a strip, chunks that span strips and segments)
                + [("bf16", i, 2, tb, 2) for i in _WGRAD_IDS[11:] for tb in (0, 1, 64)]
                + [("bf16", "pyramid", 2, 40, 2), ("bf16", "3x3", 2, 0, 2), ("f16", "halo_segs", 2, 64, 2)])


@pytest.mark.parametrize("build,shape_id,kernel_opt,target_blocks,want_kernel", _WGRAD_CASES)
def test_wgrad(cuda, build, shape_id, kernel_opt, target_blocks, want_kernel):
    from retinanet import _C
    lib = _lib()
    idx = _WGRAD_IDS.index(shape_id)
    segs, k, stride = WGRAD_SHAPES[idx]
    g = torch.Generator().manual_seed(len(segs) * 100 + k + stride)
    pad = (k - 1) // 2
    cin, cout = segs[0][2], segs[0][3]
    p = _C.WgradProblem()
    p.R = p.S = k
    p.stride_h = p.stride_w = stride
    p.pad_top = p.pad_left = pad
    p.num_segments = len(segs)
    p.opts = _C.LaunchOpts(wgrad_kernel=kernel_opt, wgrad_target_blocks=target_blocks)
    keep = []
    want = torch.zeros((cout, k, k, cin), dtype=torch.float64)
    for i, (N, H, ci, co) in enumerate(segs):
        Hh, Ww = _WGRAD_HW.get(shape_id) or (H, H)
        x = _bf(torch.randn((N, Hh, Ww, ci), generator=g))
        Ho, Wo = (Hh + 2 * pad - k) // stride + 1, (Ww + 2 * pad - k) // stride + 1
        dy = _bf(torch.randn((N, Ho, Wo, co), generator=g))
        xd, dyd = x.to(cuda), dy.to(cuda)
        s = p.seg[i]
        s.x, s.dy = xd.data_ptr(), dyd.data_ptr()
        s.N, s.H, s.W, s.Cin, s.Ho, s.Wo, s.Cout = N, Hh, Ww, ci, Ho, Wo, co
        keep += [xd, dyd]
        w = torch.zeros((co, ci, k, k), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x.double().permute(0, 3, 1, 2), w, stride=stride, padding=pad)
        y.backward(dy.double().permute(0, 3, 1, 2))
        want += w.grad.permute(0, 2, 3, 1)
    assert lib.rn_wgrad_kernel_id(ctypes.byref(p)) == want_kernel
    ws = _ws(lib.rn_wgrad_workspace_bytes(ctypes.byref(p)), cuda)
    ws.fill_(0x7f)      # stale workspace bytes must not leak into the sums
    dw = torch.full((cout, k, k, cin), 7.0, dtype=torch.float32, device=cuda)
    _C.check(lib.rn_conv2d_nhwc_wgrad(ctypes.byref(p), _C.ptr(dw), 0.0, _C.ptr(ws), ws.numel(), _C.current_stream()))
    torch.cuda.synchronize()
    scale = want.abs().max().item()
    torch.testing.assert_close(dw.cpu().double(), want, rtol=1e-3, atol=1e-3 * scale)
    # beta = 1 accumulates
    _C.check(lib.rn_conv2d_nhwc_wgrad(ctypes.byref(p), _C.ptr(dw), 1.0, _C.ptr(ws), ws.numel(), _C.current_stream()))
    torch.cuda.synchronize()
    torch.testing.assert_close(dw.cpu().double(), 2 * want, rtol=1e-3, atol=2e-3 * scale)


@pytest.mark.parametrize("build,k,stride,cin,cout,n,kernel,target_blocks", [
    ("bf16", 1, 1, 256, 64, 5, 0, 0),        # the dispatcher's own choice (128-tile kernel)
    ("bf16", 1, 1, 256, 512, 6, 2, 0),       # wide layers: wgrad_big_kernel
    ("bf16", 1, 1, 128, 256, 8, 1, 48),      # few workgroups: long pixel chunks
    ("bf16", 3, 2, 128, 128, 3, 0, 0),       # a strided 3x3 group (not the halo kernel's)
    ("f16", 1, 1, 256, 256, 4, 2, 0)])
def test_wgrad_group_layers_as_segments(cuda, build, k, stride, cin, cout, n, kernel, target_blocks):
    """Round 6: single-segment layers of identical geometry that the halo kernel does not serve (the 1x1 layers of a ResNet
    stage) run as ONE partial-tile launch — each layer a segment of a merged problem — plus one grouped reduction.  Every
    layer against float64, with beta, bit-identical repeats; a layer of different geometry breaks the group."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(7 * n + k + cin)
    pad = (k - 1) // 2
    N, H, W = 2, 18, 14
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    probs, keep, wants, dws, olds = [], [], [], [], []
    for layer in range(n):
        p = _C.WgradProblem()
        p.R = p.S = k
        p.stride_h = p.stride_w = stride
        p.pad_top = p.pad_left = pad
        p.num_segments = 1
        p.opts = _C.LaunchOpts(wgrad_kernel=kernel, wgrad_target_blocks=target_blocks)
        x = _bf(torch.randn((N, H, W, cin), generator=g))
        dy = _bf(torch.randn((N, Ho, Wo, cout), generator=g))
        xd, dyd = x.to(cuda), dy.to(cuda)
        sg = p.seg[0]
        sg.x, sg.dy = xd.data_ptr(), dyd.data_ptr()
        sg.N, sg.H, sg.W, sg.Cin, sg.Ho, sg.Wo, sg.Cout = N, H, W, cin, Ho, Wo, cout
        keep += [xd, dyd]
        w = torch.zeros((cout, cin, k, k), dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double().permute(0, 3, 1, 2), w, stride=stride, padding=pad).backward(dy.double().permute(0, 3, 1, 2))
        probs.append(p)
        wants.append(w.grad.permute(0, 2, 3, 1))
        old = torch.randn((cout, k, k, cin), generator=g)
        olds.append(old)
        dws.append(old.to(cuda).clone())
    arr = (ctypes.POINTER(_C.WgradProblem) * n)(*[ctypes.pointer(p) for p in probs])
    assert lib.rn_wgrad_group_fused(arr, n) == 1
    if kernel == 2:
        assert lib.rn_wgrad_kernel_id(ctypes.byref(probs[0])) == 1      # the 256-wide kernel really runs
    ws = _ws(lib.rn_wgrad_group_workspace_bytes(arr, n), cuda)
    ws.fill_(0x7f)
    beta = 0.5
    _C.check(lib.rn_conv2d_nhwc_wgrad_group(arr, n, _C.ptr_array(dws), beta, _C.ptr(ws), ws.numel(), _C.current_stream()))
    torch.cuda.synchronize()
    for layer in range(n):
        want = wants[layer] + beta * olds[layer].double()
        scale = wants[layer].abs().max().item()
        torch.testing.assert_close(dws[layer].cpu().double(), want, rtol=1e-3, atol=1e-3 * scale)
    first = [d.clone() for d in dws]
    for d, old in zip(dws, olds):
        d.copy_(old)
    _C.check(lib.rn_conv2d_nhwc_wgrad_group(arr, n, _C.ptr_array(dws), beta, _C.ptr(ws), ws.numel(), _C.current_stream()))
    torch.cuda.synchronize()
    for a, b in zip(first, dws):
        assert torch.equal(a, b)              # deterministic: ordered split-K reduction
    probs[1].seg[0].N = 1
    assert lib.rn_wgrad_group_fused(arr, n) == 0


@pytest.mark.parametrize("build,k,n,target_blocks,fused", [("bf16", 3, 4, 0, 1), ("bf16", 3, 8, 0, 1), ("bf16", 3, 3, 64, 1),
                                                          ("f16", 3, 4, 0, 1), ("bf16", 1, 3, 0, 0)])
def test_wgrad_group(cuda, build, k, n, target_blocks, fused):
    """rn_conv2d_nhwc_wgrad_group: n layers of identical geometry (here: shared head convs over a small pyramid) as ONE
    wgrad_halo_kernel launch over (layer, co tile, ci tile) tiles + one reduction launch — each layer against the float64
    reference; a group the halo kernel does not serve (1x1) is issued layer by layer and must equal the single calls
    bit for bit."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(31 + n + k)
    pad = (k - 1) // 2
    shapes = [(2, 24, 20), (2, 12, 10), (3, 5, 7)]      # N, H, W per segment
    cin, cout = 128, 192
    probs, keep, wants, dws = [], [], [], []
    for layer in range(n):
        p = _C.WgradProblem()
        p.R = p.S = k
        p.stride_h = p.stride_w = 1
        p.pad_top = p.pad_left = pad
        p.num_segments = len(shapes)
        p.opts = _C.LaunchOpts(wgrad_kernel=2, wgrad_target_blocks=target_blocks)
        want = torch.zeros((cout, k, k, cin), dtype=torch.float64)
        for i, (N, H, W) in enumerate(shapes):
            x = _bf(torch.randn((N, H, W, cin), generator=g))
            dy = _bf(torch.randn((N, H, W, cout), generator=g))
            xd, dyd = x.to(cuda), dy.to(cuda)
            sg = p.seg[i]
            sg.x, sg.dy = xd.data_ptr(), dyd.data_ptr()
            sg.N, sg.H, sg.W, sg.Cin, sg.Ho, sg.Wo, sg.Cout = N, H, W, cin, H, W, cout
            keep += [xd, dyd]
            w = torch.zeros((cout, cin, k, k), dtype=torch.float64, requires_grad=True)
            F.conv2d(x.double().permute(0, 3, 1, 2), w, padding=pad).backward(dy.double().permute(0, 3, 1, 2))
            want += w.grad.permute(0, 2, 3, 1)
        probs.append(p)
        wants.append(want)
        dws.append(torch.full((cout, k, k, cin), 7.0, dtype=torch.float32, device=cuda))
    arr = (ctypes.POINTER(_C.WgradProblem) * n)(*[ctypes.pointer(p) for p in probs])
    assert lib.rn_wgrad_group_fused(arr, n) == fused
    ws = _ws(lib.rn_wgrad_group_workspace_bytes(arr, n), cuda)
    ws.fill_(0x7f)
    _C.check(lib.rn_conv2d_nhwc_wgrad_group(arr, n, _C.ptr_array(dws), 0.0, _C.ptr(ws), ws.numel(), _C.current_stream()))
    torch.cuda.synchronize()
    for layer in range(n):
        scale = wants[layer].abs().max().item()
        torch.testing.assert_close(dws[layer].cpu().double(), wants[layer], rtol=1e-3, atol=1e-3 * scale)
    first = [d.clone() for d in dws]
    _C.check(lib.rn_conv2d_nhwc_wgrad_group(arr, n, _C.ptr_array(dws), 0.0, _C.ptr(ws), ws.numel(), _C.current_stream()))
    torch.cuda.synchronize()
    for a, b in zip(first, dws):
        assert torch.equal(a, b)              # deterministic: ordered split-K reduction
    if not fused:
        for layer in range(n):
            one = torch.zeros_like(dws[layer])
            w1 = _ws(lib.rn_wgrad_workspace_bytes(ctypes.byref(probs[layer])), cuda)
            _C.check(lib.rn_conv2d_nhwc_wgrad(ctypes.byref(probs[layer]), _C.ptr(one), 0.0, _C.ptr(w1), w1.numel(),
                                              _C.current_stream()))
            torch.cuda.synchronize()
            assert torch.equal(one, dws[layer])
    # a layer whose geometry differs breaks the group: per-layer calls, still the right sums
    if fused and n >= 3:
        probs[1].seg[0].N = 1
        assert lib.rn_wgrad_group_fused(arr, n) == 0


def test_kernels_with_compute_units_reserved_for_rccl(cuda):
    """rn_launch_opts.reserved_cus (data-parallel runs): the persistent kernels run on fewer workgroups than CUs, the
    256-wide weight-gradient kernels walk several work items per workgroup.  The 256-row convs must give bit-identical
    outputs (a tile's arithmetic does not depend on which workgroup computes it); the weight-gradient kernels re-plan
    their split-K chunks for the smaller machine, so their sums are compared with the float64 reference."""
    from retinanet import _C
    import test_gpu_conv as TC
    lib = _lib()
    g = torch.Generator().manual_seed(77)
    seg = {"x": torch.randn((4, 24, 24, 256), generator=g), "w": torch.randn((3, 3, 256, 256), generator=g) / 48.0,
           "bias": torch.randn((256,), generator=g), "scale": torch.rand((256,), generator=g) + 0.5,
           "shift": torch.randn((256,), generator=g) * 0.1}
    outs = {}
    for reserved, no_halo in ((0, 0), (128, 0), (0, 1), (100, 1)):
        outs[(reserved, no_halo)] = TC._conv_gpu(cuda, [seg], 3, 1, 1, "relu", False,
                                                 dict(conv_tile=2, reserved_cus=reserved, conv_no_halo=no_halo))[0]
    assert torch.equal(outs[(0, 0)], outs[(128, 0)]) and torch.equal(outs[(0, 1)], outs[(100, 1)])
    TC._close(outs[(0, 0)], TC._conv_ref(seg, 3, 1, 1, "relu", False), False)
    # out-of-range values are refused per call
    with pytest.raises(_C.RnetError):
        TC._conv_gpu(cuda, [seg], 3, 1, 1, "relu", False, dict(reserved_cus=129))
    # 256-wide weight-gradient kernels with 128 of the CUs reserved: several work items per workgroup
    N, H, ci, co, k = 4, 20, 256, 256, 3
    x = _bf(torch.randn((N, H, H, ci), generator=g))
    dy = _bf(torch.randn((N, H, H, co), generator=g))
    w = torch.zeros((co, ci, k, k), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    want = w.grad.permute(0, 2, 3, 1)
    xd, dyd = x.to(cuda), dy.to(cuda)
    got = {}
    for reserved in (0, 128):
        p = _C.WgradProblem()
        p.R = p.S = k
        p.stride_h = p.stride_w = p.pad_top = p.pad_left = 1
        p.num_segments = 1
        p.opts = _C.LaunchOpts(wgrad_kernel=2, reserved_cus=reserved)
        s = p.seg[0]
        s.x, s.dy = xd.data_ptr(), dyd.data_ptr()
        s.N, s.H, s.W, s.Cin, s.Ho, s.Wo, s.Cout = N, H, H, ci, H, H, co
        ws = _ws(lib.rn_wgrad_workspace_bytes(ctypes.byref(p)), cuda)
        dw = torch.zeros((co, k, k, ci), dtype=torch.float32, device=cuda)
        _C.check(lib.rn_conv2d_nhwc_wgrad(ctypes.byref(p), _C.ptr(dw), 0.0, _C.ptr(ws), ws.numel(), _C.current_stream()))
        torch.cuda.synchronize()
        got[reserved] = dw.cpu().double()
    scale = want.abs().max().item()
    for reserved in (0, 128):
        torch.testing.assert_close(got[reserved], want, rtol=1e-3, atol=1e-3 * scale)


def test_two_engines_in_one_process_do_not_share_launch_options(cuda):
    """the library keeps no mutable process-wide state.  Two rn_handle contexts hold different
    rn_launch_opts; a launch is a function of its own problem descriptor only."""
    from retinanet import _C
    lib = _lib()
    a = _C.Handle(lib, 0, _C.LaunchOpts(conv_tile=2, reserved_cus=8))
    b = _C.Handle(lib, 0, _C.LaunchOpts(conv_tile=1))
    assert a.device == b.device == 0 and a.num_cus == b.num_cus >= 64
    oa, ob = a.launch_opts(), b.launch_opts()
    assert (oa.conv_tile, oa.reserved_cus, ob.conv_tile, ob.reserved_cus) == (2, 8, 1, 0)
    with pytest.raises(_C.RnetError):
        a.set_launch_opts(_C.LaunchOpts(conv_tile=4))
    assert a.launch_opts().conv_tile == 2           # a refused update leaves the handle as it was
    with pytest.raises(_C.RnetError):
        a.set_launch_opts(_C.LaunchOpts(ablate=1))  # the timing variants exist in the probe build only
    oa = a.launch_opts()
    assert (oa.conv_tile, oa.reserved_cus, oa.ablate) == (2, 8, 0)
    p = _C.ConvProblem()
    p.R = p.S = 3
    p.stride_h = p.stride_w = p.pad_top = p.pad_left = 1
    p.out_dtype, p.num_segments = _C.RN_DT_BF16, 1
    sg = p.seg[0]
    sg.N, sg.H, sg.W, sg.Cin, sg.pix_stride, sg.Ho, sg.Wo, sg.Cout = 2, 24, 24, 256, 256, 24, 24, 256
    ids = []
    for h in (a, b, a):
        p.opts = h.launch_opts()
        ids.append(lib.rn_conv_kernel_id(ctypes.byref(p)))
    assert ids == [2, 0, 2]
    a.close()
    b.close()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("k,stride,cin,cout", [(3, 1, 128, 256), (1, 1, 256, 128), (3, 2, 128, 128), (1, 2, 256, 512)])
def test_dgrad_via_forward_kernel(cuda, build, k, stride, cin, cout):
    """dx = conv_fwd(dy [zero-upsampled for stride 2], flipped/transposed weights)."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(k * 10 + stride)
    N, H = 2, 12
    pad = (k - 1) // 2
    Ho = (H + 2 * pad - k) // stride + 1
    w = torch.randn((cout, k, k, cin), generator=g) / math.sqrt(k * k * cin)     # compute layout OHWI
    dy = _bf(torch.randn((N, Ho, Ho, cout), generator=g))
    xr = torch.zeros((N, cin, H, H), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xr, _bf(w).double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    y.backward(dy.double().permute(0, 3, 1, 2))
    want = xr.grad.permute(0, 2, 3, 1).float()
    wd = w.to(cuda).contiguous()
    wp = torch.empty((lib.rn_conv_cout_pad(cin), k, k, cout), dtype=H16, device=cuda)
    _C.check(lib.rn_pack_conv_weight_dgrad(_C.ptr(wd), k, k, cin, cout, cout, _C.ptr(wp), _C.current_stream()))
    dyd = dy.to(cuda).contiguous()
    if stride == 2:
        up = torch.empty((N, H, H, cout), dtype=H16, device=cuda)
        _C.check(lib.rn_upsample_zero2x(_C.ptr(dyd), _C.ptr(up), N, Ho, Ho, cout, H, H, _C.current_stream()))
        src = up
    else:
        src = dyd
    dx = torch.empty((N, H, H, cin), dtype=H16, device=cuda)
    acc = _bf(torch.randn((N, H, H, cin), generator=g)).to(cuda)   # accumulate into an existing gradient
    dx.copy_(acc)
    p = _C.ConvProblem()
    p.R = p.S = k
    p.stride_h = p.stride_w = 1
    p.pad_top = p.pad_left = k - 1 - pad
    p.act, p.out_dtype, p.num_segments = _C.RN_ACT_NONE, _C.RN_DT_BF16, 1
    s = p.seg[0]
    s.x, s.w, s.y, s.scale, s.shift, s.residual = src.data_ptr(), wp.data_ptr(), dx.data_ptr(), None, None, dx.data_ptr()
    s.N, s.H, s.W, s.Cin, s.pix_stride, s.Ho, s.Wo, s.Cout = N, H, H, cout, cout, H, H, cin
    _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(p), _C.current_stream()))
    torch.cuda.synchronize()
    ref = _bf(want + acc.float().cpu()).float()
    scale = ref.abs().max().item()
    torch.testing.assert_close(dx.float().cpu(), ref, rtol=1 / 128, atol=scale / 200)


@pytest.mark.parametrize("build,N,H,W,cin,cout,accumulate", [
    ("bf16", 2, 12, 12, 64, 64, False), ("bf16", 1, 20, 16, 128, 128, True), ("bf16", 2, 8, 10, 256, 256, False),
    ("bf16", 1, 6, 6, 32, 96, True), ("f16", 1, 20, 16, 128, 128, True)])
def test_dgrad_stride2_subpixel(cuda, build, N, H, W, cin, cout, accumulate):
    """Data gradient of a 3x3 / stride 2 / pad 1 conv in its sub-pixel form (rn_dgrad_pack.pad_ == 1): one 2x2
    stride-1 conv of dy with 4*Cin phase-major channels + rn_depth_to_space2x, against autograd."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(cin + cout + H)
    Ho, Wo = H // 2, W // 2
    w = torch.randn((cout, 3, 3, cin), generator=g) / math.sqrt(9 * cin)         # compute layout OHWI
    dy = _bf(torch.randn((N, Ho, Wo, cout), generator=g))
    xr = torch.zeros((N, cin, H, W), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xr, _bf(w).double().permute(0, 3, 1, 2), stride=2, padding=1)
    assert y.shape[2:] == (Ho, Wo)
    y.backward(dy.double().permute(0, 3, 1, 2))
    want = xr.grad.permute(0, 2, 3, 1).float()
    wd = w.to(cuda).contiguous()
    cwp = lib.rn_conv_cin_pad(cout)
    wp = torch.empty((lib.rn_conv_cout_pad(4 * cin), 2, 2, cwp), dtype=H16, device=cuda)
    item = (_C.DgradPack * 1)()
    item[0].w_ohwi, item[0].w_packed = wd.data_ptr(), wp.data_ptr()
    item[0].R, item[0].S, item[0].Cin, item[0].Cout, item[0].Cout_pad, item[0].pad_ = 3, 3, cin, cout, cwp, 1
    _C.check(lib.rn_pack_conv_weight_dgrad_batch(item, 1, _C.current_stream()))
    dyd = dy.to(cuda).contiguous()
    phases = torch.empty((N, Ho, Wo, 4 * cin), dtype=H16, device=cuda)
    p = _C.ConvProblem()
    p.R = p.S = 2
    p.stride_h = p.stride_w = 1
    p.pad_top = p.pad_left = 0
    p.act, p.out_dtype, p.num_segments = _C.RN_ACT_NONE, _C.RN_DT_BF16, 1
    s = p.seg[0]
    s.x, s.w, s.y = dyd.data_ptr(), wp.data_ptr(), phases.data_ptr()
    s.N, s.H, s.W, s.Cin, s.pix_stride, s.Ho, s.Wo, s.Cout = N, Ho, Wo, cout, cout, Ho, Wo, 4 * cin
    _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(p), _C.current_stream()))
    old = _bf(torch.randn((N, H, W, cin), generator=g))
    dx = old.to(cuda).clone()
    _C.check(lib.rn_depth_to_space2x(_C.ptr(phases), _C.ptr(dx), N, Ho, Wo, cin, 1 if accumulate else 0, _C.current_stream()))
    torch.cuda.synchronize()
    ref = _bf(_bf(want) + old.float()).float() if accumulate else _bf(want).float()
    scale = ref.abs().max().item()
    torch.testing.assert_close(dx.float().cpu(), ref, rtol=1 / 128, atol=scale / 200)


# ---------------------------------------------------------------------------------------------
def _bn_problem(cuda, segs, act, eps=1e-3, momentum=0.99, bessel=1, with_bwd=False):
    from retinanet import _C
    p = _C.BnProblem()
    p.num_segments, p.act, p.bessel, p.eps, p.momentum, p.count_scale = len(segs), _C.ACT_IDS[act], bessel, eps, momentum, 1.0
    dev = []
    for i, s in enumerate(segs):
        P, C = s["y"].shape[0] * s["y"].shape[1] * s["y"].shape[2], s["y"].shape[3]
        d = {k: (_bf(v).to(cuda).contiguous() if v is not None else None) for k, v in s.items()
             if k in ("y", "residual", "dz")}
        d["z"] = torch.empty_like(d["y"])
        d["dy"] = torch.empty_like(d["y"])
        d["dres"] = torch.zeros_like(d["y"])
        for k in ("sums", "bsums"):
            d[k] = torch.zeros((2, C), dtype=torch.float32, device=cuda)
        d["fwd"] = torch.zeros((4, C), dtype=torch.float32, device=cuda)
        for k in ("gamma", "beta", "moving_mean", "moving_var"):
            d[k] = s[k].to(cuda).float().contiguous()
        d["dgamma"] = torch.zeros((C,), dtype=torch.float32, device=cuda)
        d["dbeta"] = torch.zeros((C,), dtype=torch.float32, device=cuda)
        g = p.seg[i]
        for k in ("y", "z", "residual", "dz", "dy", "dres", "sums", "fwd", "bsums", "gamma", "beta", "moving_mean",
                  "moving_var", "dgamma", "dbeta"):
            t = d.get(k)
            setattr(g, k, t.data_ptr() if t is not None else None)
        g.P, g.C, g.dres_accumulate = P, C, 0
        dev.append(d)
    return p, dev


@pytest.mark.parametrize("build,act", [("bf16", "relu"), ("bf16", "relu6"), ("f16", "relu")])
def test_bn_backward_gate_from_the_bit_mask(cuda, build, act):
    """rn_bn_segment.act_mask: rn_bn_apply stores the relu gate of a residual layer as one bit per element and the two
    backward passes read it instead of z — every output must be bit-identical to the z-reading kernels."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(5)
    shapes = [(2, 9, 7, 64), (1, 5, 5, 256), (3, 4, 4, 8)]
    segs = [{"y": torch.randn((N, H, W, C), generator=g) * 2 + 0.5, "residual": torch.randn((N, H, W, C), generator=g) * 3,
             "dz": torch.randn((N, H, W, C), generator=g), "gamma": torch.rand((C,), generator=g) + 0.5,
             "beta": torch.randn((C,), generator=g) * 0.2, "moving_mean": torch.zeros((C,)), "moving_var": torch.ones((C,))}
            for (N, H, W, C) in shapes]
    out = {}
    for masked in (False, True):
        p, dev = _bn_problem(cuda, segs, act)
        masks = []
        for i, d in enumerate(dev):
            p.seg[i].dres = d["dres"].data_ptr()
            if masked:
                masks.append(torch.full((d["y"].numel() // 8,), 0xA5, dtype=torch.uint8, device=cuda))
                p.seg[i].act_mask = masks[-1].data_ptr()
        ws = _ws(lib.rn_bn_workspace_bytes(ctypes.byref(p)), cuda)
        st = _C.current_stream()
        _C.check(lib.rn_bn_stats_finalize(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
        _C.check(lib.rn_bn_apply(ctypes.byref(p), st))
        if masked:
            for d in dev:
                d["z"].fill_(float("nan"))     # the backward must not look at z any more
        _C.check(lib.rn_bn_bwd_reduce(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
        _C.check(lib.rn_bn_bwd_apply(ctypes.byref(p), st))
        torch.cuda.synchronize()
        out[masked] = [{k: d[k].clone() for k in ("dy", "dres", "bsums", "dgamma", "dbeta")} for d in dev]
        if masked:
            for d, mk in zip(out[False], masks):
                assert 0.05 < float((mk.int() != 0).float().mean()) <= 1.0
    for a, b in zip(out[False], out[True]):
        for k in a:
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k].view(torch.int16),
                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k].view(torch.int16)), k


@pytest.mark.parametrize("build,act,use_res", [
    ("bf16", "relu", True), ("bf16", "relu", False), ("bf16", None, False), ("bf16", "relu6", True), ("bf16", "swish", False),
    ("f16", "relu", True), ("f16", "relu", False), ("f16", "swish", False)])
def test_bn_train_forward_backward(cuda, build, act, use_res):
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(11)
    shapes = [(2, 9, 7, 64), (1, 5, 5, 256), (3, 4, 4, 8)]
    segs = []
    for (N, H, W, C) in shapes:
        segs.append({"y": torch.randn((N, H, W, C), generator=g) * 2 + 0.5,
                     "residual": torch.randn((N, H, W, C), generator=g) if use_res else None,
                     "dz": torch.randn((N, H, W, C), generator=g),
                     "gamma": torch.rand((C,), generator=g) + 0.5, "beta": torch.randn((C,), generator=g) * 0.2,
                     "moving_mean": torch.randn((C,), generator=g), "moving_var": torch.rand((C,), generator=g) + 0.5})
    p, dev = _bn_problem(cuda, segs, act)
    ws = _ws(lib.rn_bn_workspace_bytes(ctypes.byref(p)), cuda)
    st = _C.current_stream()
    if use_res:   # the two forms of the forward statistics must agree: separate calls / fused finalize
        _C.check(lib.rn_bn_stats(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
        _C.check(lib.rn_bn_finalize(ctypes.byref(p), st))
    else:
        _C.check(lib.rn_bn_stats_finalize(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
    _C.check(lib.rn_bn_apply(ctypes.byref(p), st))
    _C.check(lib.rn_bn_bwd_reduce(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
    _C.check(lib.rn_bn_bwd_apply(ctypes.byref(p), st))
    torch.cuda.synchronize()
    for s, d in zip(segs, dev):
        y = _bf(s["y"]).double().requires_grad_(True)
        gam = s["gamma"].double().requires_grad_(True)
        bet = s["beta"].double().requires_grad_(True)
        res = _bf(s["residual"]).double().requires_grad_(True) if use_res else None
        n = y.numel() // y.shape[-1]
        mean = y.mean(dim=(0, 1, 2))
        var = y.var(dim=(0, 1, 2), unbiased=False)
        v = (y - mean) / torch.sqrt(var + 1e-3) * gam + bet
        if use_res:
            v = v + res
        z = F.relu(v) if act == "relu" else (F.relu6(v) if act == "relu6" else (v * torch.sigmoid(v) if act == "swish" else v))
        torch.testing.assert_close(d["z"].float().cpu().double(), z.detach(), rtol=1 / 100, atol=2e-2)
        # backward through the bf16-rounded z mask the kernel sees (swish: through the recomputed pre-activation)
        zk = d["z"].float().cpu().double()
        if act == "swish":
            sg = torch.sigmoid(v.detach())
            mask = sg + v.detach() * sg * (1 - sg)
        else:
            mask = torch.ones_like(zk) if act is None else ((zk > 0) & ((zk < 6) if act == "relu6" else True)).double()
        gz = _bf(s["dz"]).double() * mask
        (v * gz.detach()).sum().backward()
        torch.testing.assert_close(d["dy"].float().cpu().double(), y.grad, rtol=2e-2, atol=2e-2 * y.grad.abs().max().item())
        torch.testing.assert_close(d["dgamma"].cpu().double(), gam.grad, rtol=2e-3, atol=2e-3 * gam.grad.abs().max().item() + 1e-4)
        torch.testing.assert_close(d["dbeta"].cpu().double(), bet.grad, rtol=2e-3, atol=2e-3 * bet.grad.abs().max().item() + 1e-4)
        if use_res:
            torch.testing.assert_close(d["dres"].float().cpu().double(), gz, rtol=1 / 128, atol=1e-2)
        # moving statistics: momentum 0.99, Bessel-corrected variance (fused BN)
        mm = s["moving_mean"].double() * 0.99 + mean.detach() * 0.01
        mv = s["moving_var"].double() * 0.99 + var.detach() * n / (n - 1) * 0.01
        torch.testing.assert_close(d["moving_mean"].cpu().double(), mm, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(d["moving_var"].cpu().double(), mv, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("build,use_res", [("bf16", False), ("bf16", True), ("f16", False)])
def test_bn_backward_apply_column_sums_of_dy(cuda, build, use_res):
    """rn_bn_segment.dy_colsum_partial: rn_bn_bwd_apply also sums the columns of the dy it stores (the bias gradient of a
    Conv2D in front of a training-mode BatchNorm: the engine finishes it with rn_bn_stats(ext_chunks) on the per-chunk
    partials instead of reading dy again).  dy and every other output bit-identical to the plain call; the finished sums
    equal the column sums of the stored tensor to fp32 accumulation error; repeats bit-identical; a problem whose channel
    groups do not divide 256 reports 0 chunks and refuses the field."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(23)
    shapes = [(2, 40, 40, 256), (1, 80, 80, 256), (3, 10, 10, 256), (1, 3, 3, 64)]      # 2048-unit chunks: 50 / 100 / 4.7 / 0.04
    segs = [{"y": torch.randn((N, H, W, C), generator=g) * 2 + 0.5,
             "residual": torch.randn((N, H, W, C), generator=g) if use_res else None,
             "dz": torch.randn((N, H, W, C), generator=g), "gamma": torch.rand((C,), generator=g) + 0.5,
             "beta": torch.randn((C,), generator=g) * 0.2, "moving_mean": torch.zeros((C,)), "moving_var": torch.ones((C,))}
            for (N, H, W, C) in shapes]
    out = {}
    for fused in (False, True, True):
        p, dev = _bn_problem(cuda, segs, "relu")
        st = _C.current_stream()
        ws = _ws(lib.rn_bn_workspace_bytes(ctypes.byref(p)), cuda)
        sums, keep = [], []
        if fused:
            p2 = _C.BnProblem()
            p2.num_segments, p2.act, p2.bessel, p2.eps, p2.momentum, p2.count_scale = len(segs), 0, 0, 0.0, 0.0, 1.0
            for i, d in enumerate(dev):
                ch = lib.rn_bn_bwd_colsum_chunks(ctypes.byref(p), i)
                C = d["y"].shape[3]
                assert ch == -(-(d["y"].numel() // 8) // 2048)
                sums.append(torch.zeros((2, C), dtype=torch.float32, device=cuda))
                q = p2.seg[i]
                q.y, q.sums, q.P, q.C, q.ext_chunks = d["dy"].data_ptr(), sums[-1].data_ptr(), d["y"].numel() // C, C, ch
            ws2 = torch.zeros((lib.rn_bn_workspace_bytes(ctypes.byref(p2)),), dtype=torch.uint8, device=cuda)
            for i in range(len(dev)):
                p.seg[i].dy_colsum_partial = ws2.data_ptr() + lib.rn_bn_partial_offset_bytes(ctypes.byref(p2), i)
            keep += [p2, ws2]
        _C.check(lib.rn_bn_stats_finalize(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
        _C.check(lib.rn_bn_apply(ctypes.byref(p), st))
        _C.check(lib.rn_bn_bwd_reduce(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
        _C.check(lib.rn_bn_bwd_apply(ctypes.byref(p), st))
        if fused:
            _C.check(lib.rn_bn_stats(ctypes.byref(p2), _C.ptr(ws2), ws2.numel(), st))
        torch.cuda.synchronize()
        res = [{k: d[k].clone() for k in ("dy", "dres", "bsums")} for d in dev]
        if fused:
            for r, sm in zip(res, sums):
                r["colsum"] = sm[0].clone()
        out.setdefault(fused, []).append(res)
    plain, (f1, f2) = out[False][0], out[True]
    for a, b, c in zip(plain, f1, f2):
        for k in ("dy", "dres", "bsums"):
            assert torch.equal(a[k].float(), b[k].float()), k
        assert torch.equal(b["colsum"], c["colsum"])
        want = b["dy"].double().reshape(-1, b["dy"].shape[3]).sum(0)
        scale = b["dy"].double().abs().sum(dim=(0, 1, 2)).max().item()
        torch.testing.assert_close(b["colsum"].double(), want, rtol=0, atol=2e-6 * scale)
    # channel groups that do not divide 256 (144 channels = 18 groups): the grid-stride form, no column sums
    odd = [{"y": torch.randn((1, 6, 6, 144), generator=g), "residual": None, "dz": torch.randn((1, 6, 6, 144), generator=g),
            "gamma": torch.ones((144,)), "beta": torch.zeros((144,)), "moving_mean": torch.zeros((144,)), "moving_var": torch.ones((144,))}]
    p, dev = _bn_problem(cuda, odd, "relu")
    assert lib.rn_bn_bwd_colsum_chunks(ctypes.byref(p), 0) == 0
    p.seg[0].dy_colsum_partial = dev[0]["fwd"].data_ptr()
    assert lib.rn_bn_bwd_apply(ctypes.byref(p), _C.current_stream()) == _C.RN_EINVAL


def test_bn_stage2_reduction_in_parts(cuda):
    """rn_bn_stats on external partial sums (rn_bn_segment.ext_chunks): a segment with more than 512 rows of partials has its
    stage-2 reduction cut into parts — write-through slots, a ticket per (segment, 16 channels), the last arriver adds the
    parts in part order.  Against float64 sums of the same partials; bit-equal over repeated launches (the counters return
    to zero) and against the unsplit form of the same rows; segments of one launch mix split and unsplit reductions."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(11)
    segs = [(256, 1600), (256, 400), (64, 6400), (136, 700), (2048, 26)]   # (C, rows of partial sums)
    p = _C.BnProblem()
    p.num_segments, p.act, p.bessel, p.eps, p.momentum, p.count_scale = len(segs), 0, 0, 1e-3, 0.9, 1.0
    sums = []
    for i, (C, ch) in enumerate(segs):
        sums.append(torch.zeros((2, C), dtype=torch.float32, device=cuda))
        q = p.seg[i]
        q.y, q.sums, q.P, q.C, q.ext_chunks = sums[-1].data_ptr(), sums[-1].data_ptr(), ch * 128, C, ch
    nbytes = lib.rn_bn_workspace_bytes(ctypes.byref(p))
    ws = torch.zeros((nbytes // 4,), dtype=torch.float32, device=cuda)
    parts = []
    for i, (C, ch) in enumerate(segs):
        off = lib.rn_bn_partial_offset_bytes(ctypes.byref(p), i) // 4
        t = torch.randn((ch, 2, C), generator=g) * torch.rand((1, 1, C), generator=g) * 50.0
        ws[off:off + t.numel()] = t.reshape(-1).to(cuda)
        parts.append(t)
    st = _C.current_stream()
    runs = []
    for _ in range(3):
        _C.check(lib.rn_bn_stats(ctypes.byref(p), _C.ptr(ws), nbytes, st))
        torch.cuda.synchronize()
        runs.append([s_.clone() for s_ in sums])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    for (C, ch), t, got in zip(segs, parts, runs[0]):
        want = t.double().sum(0)
        scale = t.double().abs().sum(0)
        assert ((got.cpu().double() - want).abs() <= 1e-7 * scale + 1e-30).all(), (C, ch)
    # the tail of the workspace (counters) is zero again
    tail0 = sum(2 * C * ch for C, ch in segs)
    n_cnt = sum(-(-C // 16) for C, _ in segs)
    tail = ws[(tail0 * 4 + 255) // 256 * 64:][:n_cnt].view(torch.int32)
    assert int(tail.abs().sum().item()) == 0
    # a workspace that was NOT zero-filled at allocation: rn_bn_workspace_init zeroes the counters (and only them)
    ws2 = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=cuda)
    ws2.view(torch.int32).fill_(0x7FC12345)
    ws2[:tail0] = ws[:tail0]
    _C.check(lib.rn_bn_workspace_init(ctypes.byref(p), _C.ptr(ws2), nbytes, st))
    assert torch.equal(ws2[:tail0], ws[:tail0])                      # the partial sums are untouched
    for s_ in sums:
        s_.zero_()
    _C.check(lib.rn_bn_stats(ctypes.byref(p), _C.ptr(ws2), nbytes, st))
    torch.cuda.synchronize()
    for a, b in zip(runs[0], sums):
        assert torch.equal(a, b)
    assert lib.rn_bn_workspace_init(ctypes.byref(p), _C.ptr(ws2), nbytes - 4, st) == _C.RN_ENOMEM


@pytest.mark.parametrize("build,k,tile", [("bf16", 1, 2), ("bf16", 3, 2), ("bf16", 1, 1), ("bf16", 3, 1), ("bf16", 3, 3),
                                          ("bf16", 3, 4), ("f16", 1, 2), ("f16", 3, 2), ("f16", 3, 1), ("f16", 3, 3), ("f16", 3, 4)])
def test_bn_forward_stats_fused_into_conv_epilogue(cuda, build, k, tile):
    """rn_conv_segment.bn_partial + rn_bn_segment.ext_chunks: the 256-row conv kernel writes the per-128-row partial
    sums, rn_bn_stats only runs the final reduction.  Must give the statistics of the unfused path on the same
    stored bf16 output (fp32 summation order differs), including pixel tails and a channel tail (Cout 320)."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(23)
    shapes = [(2, 19, 21, 128, 256), (1, 16, 16, 128, 320), (3, 7, 5, 128, 512)]   # N, H, W, Cin, Cout
    if tile == 3:   # 64 < Cout <= 128: the halo kernel's 512 x 128 tiles (4 row blocks of partial sums per tile)
        shapes = [(2, 19, 21, 128, 128), (1, 26, 26, 64, 96), (3, 7, 5, 128, 120)]
    pc = _C.ConvProblem()
    pc.R = pc.S = k            # k = 3: the halo-patch kernel (rn_conv_halo.hip), same epilogue
    pc.stride_h = pc.stride_w = 1
    pc.pad_top = pc.pad_left = (k - 1) // 2
    pc.act, pc.out_dtype, pc.num_segments = _C.RN_ACT_NONE, _C.RN_DT_BF16, len(shapes)
    keep, ys, segs = [], [], []
    for i, (N, H, W, cin, cout) in enumerate(shapes):
        x = _bf(torch.randn((N, H, W, cin), generator=g)).to(cuda)
        w = (torch.randn((k, k, cin, cout), generator=g) / (8 * k) + 0.02 / k).to(cuda).contiguous()
        wp = torch.empty((lib.rn_conv_cout_pad(cout), k, k, cin), dtype=H16, device=cuda)
        _C.check(lib.rn_pack_conv_weight(_C.ptr(w), k, k, cin, cout, cin, _C.ptr(wp), _C.current_stream()))
        y = torch.empty((N, H, W, cout), dtype=H16, device=cuda)
        s = pc.seg[i]
        s.x, s.w, s.y, s.scale, s.shift, s.residual = x.data_ptr(), wp.data_ptr(), y.data_ptr(), None, None, None
        s.N, s.H, s.W, s.Cin, s.pix_stride, s.Ho, s.Wo, s.Cout = N, H, W, cin, cin, H, W, cout
        keep += [x, w, wp]
        ys.append(y)
        segs.append({"y": torch.zeros((N, H, W, cout)), "gamma": torch.ones((cout,)), "beta": torch.zeros((cout,)),
                     "moving_mean": torch.zeros((cout,)), "moving_var": torch.ones((cout,))})
    st = _C.current_stream()
    # tile 1: the 128-row kernel (one partial row per tile) | 2: the 256-row kernels | 3: 512 x 128 halo tiles, narrow layers |
    # 4: 512 x 128 halo tiles on the wide shapes (what the dispatcher itself picks for them; several column tiles per row block)
    pc.opts = _C.LaunchOpts(conv_tile={1: 1, 2: 2, 3: 2, 4: 3}[tile])
    if True:
        rows = lib.rn_conv_tile_rows(ctypes.byref(pc))
        assert rows == {1: 128, 2: 256, 3: 512, 4: 512}[tile]
        if tile >= 2:
            assert lib.rn_conv_kernel_id(ctypes.byref(pc)) == (3 if tile >= 3 else (2 if k == 3 else 1))
        sums = {}
        for fused in (False, True):
            p, dev = _bn_problem(cuda, segs, None)
            for i, y in enumerate(ys):
                p.seg[i].y = y.data_ptr()
                if fused:
                    P = p.seg[i].P
                    p.seg[i].ext_chunks = (rows // 128) * ((P + rows - 1) // rows)
            ws = _ws(lib.rn_bn_workspace_bytes(ctypes.byref(p)), cuda)
            ws.fill_(0x7f)    # stale bytes must not leak into the sums
            for i in range(len(ys)):
                pc.seg[i].bn_partial = (ws.data_ptr() + lib.rn_bn_partial_offset_bytes(ctypes.byref(p), i)) if fused else None
                ys[i].zero_()
            _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(pc), st))
            _C.check(lib.rn_bn_stats(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
            torch.cuda.synchronize()
            sums[fused] = [d["sums"].cpu().double() for d in dev]
    for i, y in enumerate(ys):
        yd = y.float().cpu().double().reshape(-1, y.shape[-1])
        want = torch.stack([yd.sum(0), (yd * yd).sum(0)])
        tol = 1e-5 * want[1].abs().max().item()
        torch.testing.assert_close(sums[False][i], want, rtol=1e-5, atol=tol)
        torch.testing.assert_close(sums[True][i], want, rtol=1e-5, atol=tol)


@pytest.mark.parametrize("build,k,tile", [("bf16", 1, 2), ("bf16", 3, 2), ("bf16", 1, 1), ("bf16", 3, 1), ("bf16", 3, 3),
                                          ("bf16", 3, 4), ("f16", 1, 2), ("f16", 3, 2), ("f16", 3, 1), ("f16", 3, 3), ("f16", 3, 4)])
def test_bn_backward_reduction_fused_into_the_data_gradient(cuda, build, k, tile):
    """rn_conv_segment.bn_bwd_y + rn_bn_segment.ext_chunks_bwd: the launch that writes dz of a BatchNorm + ReLU layer
    also writes stage 1 of that layer's backward reduction (sum g, sum g*xhat); rn_bn_bwd_reduce only runs the ordered
    final pass.  dz must be bit-identical to the plain launch, the sums must match the
    unfused kernels on the same stored dz (fp32 association differs) and a float64 evaluation — 128-row kernel,
    conv_big_kernel and conv_halo_kernel, pixel tails and a channel tail (Cout 320)."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(29)
    shapes = [(2, 19, 21, 128, 256), (1, 16, 16, 128, 320), (3, 7, 5, 128, 512)]   # N, H, W, Cin, Cout
    if tile == 3:   # 64 < Cout <= 128: the halo kernel's 512 x 128 tiles (4 row blocks of partial sums per tile)
        shapes = [(2, 19, 21, 128, 128), (1, 26, 26, 64, 96), (3, 7, 5, 128, 120)]
    pc = _C.ConvProblem()
    pc.R = pc.S = k
    pc.stride_h = pc.stride_w = 1
    pc.pad_top = pc.pad_left = (k - 1) // 2
    pc.act, pc.out_dtype, pc.num_segments = _C.RN_ACT_NONE, _C.RN_DT_BF16, len(shapes)
    keep, dzs, segs = [], [], []
    for i, (N, H, W, cin, cout) in enumerate(shapes):
        x = _bf(torch.randn((N, H, W, cin), generator=g)).to(cuda)
        w = (torch.randn((k, k, cin, cout), generator=g) / (8 * k)).to(cuda).contiguous()
        wp = torch.empty((lib.rn_conv_cout_pad(cout), k, k, cin), dtype=H16, device=cuda)
        _C.check(lib.rn_pack_conv_weight(_C.ptr(w), k, k, cin, cout, cin, _C.ptr(wp), _C.current_stream()))
        dz = torch.empty((N, H, W, cout), dtype=H16, device=cuda)
        s = pc.seg[i]
        s.x, s.w, s.y, s.scale, s.shift, s.residual = x.data_ptr(), wp.data_ptr(), dz.data_ptr(), None, None, None
        s.N, s.H, s.W, s.Cin, s.pix_stride, s.Ho, s.Wo, s.Cout = N, H, W, cin, cin, H, W, cout
        keep += [x, w, wp]
        dzs.append(dz)
        # the BatchNorm layer whose output gradient the launch produces: raw conv output with a channel-dependent
        # mean and about half of the units switched off by the ReLU
        segs.append({"y": torch.randn((N, H, W, cout), generator=g) * 1.5 + torch.linspace(-3, 3, cout),
                     "dz": torch.zeros((N, H, W, cout)),
                     "gamma": torch.rand((cout,), generator=g) + 0.5, "beta": torch.randn((cout,), generator=g) * 0.3,
                     "moving_mean": torch.zeros((cout,)), "moving_var": torch.ones((cout,))})
    st = _C.current_stream()
    pc.opts = _C.LaunchOpts(conv_tile={1: 1, 2: 2, 3: 2, 4: 3}[tile])   # (as in the forward-statistics test above)
    if True:
        rows = lib.rn_conv_tile_rows(ctypes.byref(pc))
        assert rows == {1: 128, 2: 256, 3: 512, 4: 512}[tile]
        if tile >= 2:
            assert lib.rn_conv_kernel_id(ctypes.byref(pc)) == (3 if tile >= 3 else (2 if k == 3 else 1))
        out = {}
        for fused in (False, True):
            p, dev = _bn_problem(cuda, segs, "relu")
            ws = None
            for i, dz in enumerate(dzs):
                p.seg[i].dz = dz.data_ptr()
                if fused:
                    P = p.seg[i].P
                    p.seg[i].ext_chunks_bwd = (rows // 128) * ((P + rows - 1) // rows)
            ws = _ws(lib.rn_bn_workspace_bytes(ctypes.byref(p)), cuda)
            _C.check(lib.rn_bn_stats_finalize(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))   # mean | invstd | scale | shift
            _C.check(lib.rn_bn_apply(ctypes.byref(p), st))
            ws.fill_(0x7f)    # stale bytes must not leak into the sums
            for i in range(len(dzs)):
                sg = pc.seg[i]
                sg.bn_partial = (ws.data_ptr() + lib.rn_bn_bwd_partial_offset_bytes(ctypes.byref(p), i)) if fused else None
                sg.bn_bwd_y = dev[i]["y"].data_ptr() if fused else None
                sg.bn_bwd_fwd = dev[i]["fwd"].data_ptr() if fused else None
                dzs[i].zero_()
            _C.check(lib.rn_conv2d_nhwc_fwd(ctypes.byref(pc), st))
            _C.check(lib.rn_bn_bwd_reduce(ctypes.byref(p), _C.ptr(ws), ws.numel(), st))
            _C.check(lib.rn_bn_bwd_apply(ctypes.byref(p), st))
            torch.cuda.synchronize()
            out[fused] = dict(dz=[d.clone() for d in dzs], bsums=[d["bsums"].cpu().double() for d in dev],
                              dgamma=[d["dgamma"].cpu().double() for d in dev], dbeta=[d["dbeta"].cpu().double() for d in dev],
                              dy=[d["dy"].float().cpu() for d in dev], fwd=[d["fwd"].cpu().double() for d in dev],
                              y=[d["y"].float().cpu().double() for d in dev])
    for i in range(len(shapes)):
        assert torch.equal(out[True]["dz"][i], out[False]["dz"][i])
        C = shapes[i][4]
        y = out[True]["y"][i].reshape(-1, C)
        dz = out[True]["dz"][i].float().cpu().double().reshape(-1, C)
        mean, istd, sc, sh = out[True]["fwd"][i]
        gg = dz * ((y.float() * sc.float() + sh.float()) > 0).double()     # the kernels' fp32 mask
        want = torch.stack([gg.sum(0), (gg * (y - mean) * istd).sum(0)])
        tol = 2e-5 * want.abs().max().item()
        torch.testing.assert_close(out[False]["bsums"][i], want, rtol=1e-4, atol=tol)
        torch.testing.assert_close(out[True]["bsums"][i], want, rtol=1e-4, atol=tol)
        torch.testing.assert_close(out[True]["dbeta"][i], want[0], rtol=1e-4, atol=tol)
        torch.testing.assert_close(out[True]["dgamma"][i], want[1], rtol=1e-4, atol=tol)
        torch.testing.assert_close(out[True]["dy"][i], out[False]["dy"][i], rtol=1 / 128, atol=1e-3 * out[False]["dy"][i].abs().max().item())


@pytest.mark.parametrize("build", BUILDS)
def test_pool_topdown_balance_backward(cuda, build):
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(21)
    st = _C.current_stream()
    N, C = 2, 64
    # max-pool 2x2 backward
    x = _bf(torch.randn((N, 8, 8, C), generator=g))
    dy = _bf(torch.randn((N, 4, 4, C), generator=g))
    xd, dyd = x.to(cuda), dy.to(cuda)
    dx = torch.empty_like(xd)
    _C.check(lib.rn_maxpool2d_nhwc_bwd(_C.ptr(xd), _C.ptr(dyd), _C.ptr(dx), N, 8, 8, C, 2, 2, 0, 0, 4, 4, 0, st))
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    F.max_pool2d(xr, 2).backward(dy.float().permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    torch.testing.assert_close(dx.float().cpu(), xr.grad.permute(0, 2, 3, 1), rtol=0, atol=0)
    # the stem pool: 3x3 stride 2 SAME on an even size (pad 0 top/left, 1 bottom/right), overlapping
    # windows, accumulate into an existing gradient; distinct values so the argmax is unique
    x2 = _bf(torch.randperm(2 * 12 * 12 * 8, generator=g).float().reshape(2, 12, 12, 8) / 64.0)
    dy2 = _bf(torch.randn((2, 6, 6, 8), generator=g))
    base = _bf(torch.randn((2, 12, 12, 8), generator=g))
    x2d, dy2d, dx2 = x2.to(cuda), dy2.to(cuda), base.to(cuda).clone()
    _C.check(lib.rn_maxpool2d_nhwc_bwd(_C.ptr(x2d), _C.ptr(dy2d), _C.ptr(dx2), 2, 12, 12, 8, 3, 2, 0, 0, 6, 6, 1, st))
    xr2 = x2.float().permute(0, 3, 1, 2).requires_grad_(True)
    F.max_pool2d(F.pad(xr2, (0, 1, 0, 1), value=float("-inf")), 3, 2).backward(dy2.float().permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    want2 = _bf(base.float() + xr2.grad.permute(0, 2, 3, 1)).float()
    torch.testing.assert_close(dx2.float().cpu(), want2, rtol=1 / 128, atol=1e-2)
    # FPN top-down backward over 4 levels
    L, H0 = 4, 16
    ins = [_bf(torch.randn((N, H0 >> l, H0 >> l, C), generator=g)) for l in range(L)]
    douts = [_bf(torch.randn((N, H0 >> l, H0 >> l, C), generator=g)) for l in range(L)]
    leaves = [t.float().requires_grad_(True) for t in ins]
    outs = [None] * L
    outs[L - 1] = leaves[L - 1]
    for l in range(L - 2, -1, -1):
        up = F.interpolate(outs[l + 1].permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
        outs[l] = F.relu(leaves[l] + up)
    sum((o * d.float()).sum() for o, d in zip(outs, douts)).backward()
    outs_d = [o.detach().to(H16).to(cuda) for o in outs]
    d_d = [d.to(cuda) for d in douts]
    din = [torch.empty_like(t) for t in d_d]
    for l in range(L):
        _C.check(lib.rn_fpn_topdown_bwd_level(_C.ptr(d_d[l]), _C.ptr(din[l - 1]) if l > 0 else None,
                                              _C.ptr(outs_d[l]) if l < L - 1 else None, _C.ptr(din[l]), N,
                                              H0 >> l, H0 >> l, C, _C.RN_ACT_RELU if l < L - 1 else _C.RN_ACT_NONE, st))
    torch.cuda.synchronize()
    for l in range(L):
        ref = leaves[l].grad
        torch.testing.assert_close(din[l].float().cpu(), ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item())
    # BalanceFeatures backward, 5 levels, mid = 1
    L, H0, mid = 5, 32, 1
    ins = [_bf(torch.randn((N, H0 >> l, H0 >> l, C), generator=g)) for l in range(L)]
    douts = [_bf(torch.randn((N, H0 >> l, H0 >> l, C), generator=g)) for l in range(L)]
    leaves = [t.float().permute(0, 3, 1, 2) for t in ins]
    rs = [F.max_pool2d(leaves[0], 2), leaves[1]] + [F.interpolate(leaves[l], scale_factor=2 ** (l - 1), mode="nearest") for l in (2, 3, 4)]
    avg = sum(rs) / 5.0
    ins_d = [t.to(cuda) for t in ins]
    d_d = [t.to(cuda) for t in douts]
    din = [torch.empty_like(t) for t in d_d]
    avg_h = avg.permute(0, 2, 3, 1).contiguous().to(H16)   # the forward's stored average: an INPUT of the backward
    avg_d = avg_h.to(cuda)
    scratch = torch.empty((lib.rn_balance_features_bwd_scratch_bytes(L, mid, N, H0, H0, C),), dtype=torch.uint8, device=cuda)
    assert lib.rn_balance_features_bwd(_C.ptr_array(d_d), _C.ptr_array(ins_d), _C.ptr_array(din), _C.ptr(avg_d),
                                       _C.ptr(scratch), avg_d.numel() * 2, L, mid, N, H0, H0, C, st) == _C.RN_ENOMEM
    _C.check(lib.rn_balance_features_bwd(_C.ptr_array(d_d), _C.ptr_array(ins_d), _C.ptr_array(din), _C.ptr(avg_d),
                                         _C.ptr(scratch), scratch.numel(), L, mid, N, H0, H0, C, st))
    torch.cuda.synchronize()
    # the float64 reference takes the SAME rounded avg the kernel got, so no argmax is uncertain and every element is held
    # to |got - ref| <= ulp(ref) + n 2^-23 sum|terms| + the one-step uncertainty of the 16-bit davg scratch it reads
    # (derivation in pyramid_ref.py; the rule rejects a dropped level: test_pyramid_ref_cpu.py)
    import pyramid_ref as R
    _, ref = R.balance_bwd([R.f64(t) for t in douts], [R.f64(t) for t in ins], R.f64(avg_h), mid, H16)
    for l in range(L):
        ok, ratio, outside = R.check(din[l].cpu(), ref[l], H16)
        assert ok, (l, ratio, outside)


@pytest.mark.parametrize("build", BUILDS)
def test_optimizer_step(cuda, build):
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(5)
    sizes = [64, 36864, 256, 70001, 8, 13]   # 70001: a scalar tail behind the 16-byte body; then unaligned tensors
    wd = [0, 1, 0, 1, 0, 1]
    chunk = lib.rn_optim_chunk()
    offs, segs, block_seg, o, b = [], [], [], 0, 0
    for i, n in enumerate(sizes):
        nb = (n + chunk - 1) // chunk
        segs.append((o, n, wd[i], b, nb, 0, o if wd[i] else -1))
        block_seg += [i] * nb
        offs.append(o)
        o += n
        b += nb
    total = o
    w = torch.randn((total,), generator=g)
    gr = torch.randn((total,), generator=g) * torch.cat([torch.full((n,), s) for n, s in zip(sizes, [0.1, 0.2, 30.0, 0.05, 1.0, 0.5])])
    v = torch.randn((total,), generator=g) * 0.01
    ema = w.clone() + 0.01
    seg_np = np.zeros((len(sizes),), dtype=np.dtype([("offset", "<i8"), ("size", "<i8"), ("wd", "<i4"), ("bb", "<i4"),
                                                     ("nb", "<i4"), ("pad", "<i4"), ("bf", "<i8")]))
    for i, s in enumerate(segs):
        seg_np[i] = s
    segs_d = torch.from_numpy(seg_np.view(np.uint8)).to(cuda)
    bs_d = torch.tensor(block_seg, dtype=torch.int32, device=cuda)
    wdv, gd, vd, ed = w.to(cuda), gr.to(cuda), v.to(cuda), ema.to(cuda)
    bf = torch.zeros((total,), dtype=H16, device=cuda)
    metrics = torch.zeros((8,), dtype=torch.float32, device=cuda)
    ws = _ws(lib.rn_optim_workspace_bytes(len(block_seg), len(sizes)), cuda)
    alpha, R, clip, lr, mom, dec = 1e-4, 4, 10.0, 0.1, 0.9, 0.5
    st = _C.current_stream()
    loss_scale = 1024.0        # LossScaleOptimizer: the gradients arrive scaled, the kernel unscales them first
    gd.mul_(loss_scale)
    _C.check(lib.rn_optim_clip(_C.ptr(gd), _C.ptr(wdv), _C.ptr(segs_d), len(sizes), _C.ptr(bs_d), len(block_seg),
                               alpha / R, alpha, 1.0 / loss_scale, clip, _C.ptr(metrics), _C.ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    # reference (executor.py:401-407 on float64)
    gs, ws64 = gr.double(), w.double()
    parts = []
    for i, n in enumerate(sizes):
        t = gs[offs[i]:offs[i] + n] + (alpha / R * ws64[offs[i]:offs[i] + n] if wd[i] else 0)
        parts.append(t * (clip / max(t.norm().item(), clip)))
    gn = math.sqrt(sum(t.norm().item() ** 2 for t in parts))
    parts = [t * (clip / max(gn, clip)) for t in parts]
    want_g = torch.cat(parts)
    torch.testing.assert_close(gd.cpu().double(), want_g, rtol=1e-5, atol=1e-7)
    assert metrics[1].item() == pytest.approx(gn, rel=1e-5)
    assert metrics[0].item() == pytest.approx(min(gn, clip), rel=1e-5)
    l2 = sum(alpha * 0.5 * float((ws64[offs[i]:offs[i] + n] ** 2).sum()) for i, n in enumerate(sizes) if wd[i])
    assert metrics[3].item() == pytest.approx(l2, rel=1e-5)          # l2-regularization (executor.py:296-299)
    assert metrics[4].item() == 1.0 and metrics[5].item() == 0.0    # a clip factor fired; gradients finite
    # a dropped step (skip flag set): nothing moves
    flag = torch.ones((1,), dtype=torch.float32, device=cuda)
    _C.check(lib.rn_optim_sgd_step(_C.ptr(wdv), _C.ptr(gd), _C.ptr(vd), _C.ptr(ed), _C.ptr(bf), _C.ptr(segs_d),
                                   _C.ptr(bs_d), len(block_seg), lr, mom, dec, 0, _C.ptr(flag), st))
    torch.cuda.synchronize()
    assert torch.equal(wdv.cpu(), w) and torch.equal(vd.cpu(), v)
    # Keras SGD with nesterov=True on a copy: w += m*v_new - lr*g
    wn, vn = w.to(cuda).clone(), v.to(cuda).clone()
    _C.check(lib.rn_optim_sgd_step(_C.ptr(wn), _C.ptr(gd), _C.ptr(vn), None, _C.ptr(bf), _C.ptr(segs_d),
                                   _C.ptr(bs_d), len(block_seg), lr, mom, 0.0, 1, None, st))
    torch.cuda.synchronize()
    vnew = mom * v.double() - lr * want_g
    torch.testing.assert_close(wn.cpu().double(), w.double() + mom * vnew - lr * want_g, rtol=1e-5, atol=1e-6)
    flag.zero_()
    _C.check(lib.rn_optim_sgd_step(_C.ptr(wdv), _C.ptr(gd), _C.ptr(vd), _C.ptr(ed), _C.ptr(bf), _C.ptr(segs_d),
                                   _C.ptr(bs_d), len(block_seg), lr, mom, dec, 0, _C.ptr(flag), st))
    torch.cuda.synchronize()
    v2 = mom * v.double() - lr * want_g
    w2 = w.double() + v2
    e2 = ema.double() - (1 - dec) * (ema.double() - w2)
    torch.testing.assert_close(vd.cpu().double(), v2, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(wdv.cpu().double(), w2, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ed.cpu().double(), e2, rtol=1e-5, atol=1e-6)
    for i, n in enumerate(sizes):
        # one round-to-nearest-even of the kernel's own fp32 weight: bit for bit
        want = wdv[offs[i]:offs[i] + n].to(H16) if wd[i] else torch.zeros((n,), dtype=H16, device=cuda)
        assert torch.equal(bf[offs[i]:offs[i] + n], want)
    # non-finite gradients: flagged, so that the caller can drop the step and halve the loss scale
    gd[5] = float("inf")
    _C.check(lib.rn_optim_clip(_C.ptr(gd), _C.ptr(wdv), _C.ptr(segs_d), len(sizes), _C.ptr(bs_d), len(block_seg),
                               alpha / R, alpha, 1.0, clip, _C.ptr(metrics), _C.ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    assert metrics[5].item() == 1.0


@pytest.mark.parametrize("N,H,W,C,Ho,Wo", [(2, 5, 7, 16, 10, 14), (1, 4, 3, 64, 7, 5), (3, 8, 8, 8, 16, 16)])
def test_scatter_add2x(cuda, N, H, W, C, Ho, Wo):
    """rn_scatter_add2x: y[n,2h,2w,:] (+)= x[n,h,w,:] — the placement step of the low-resolution data gradient of a
    1x1 / stride-2 convolution; fp32 add with one rounding, the other positions untouched (accumulate) or zero."""
    from retinanet import _C
    lib = _lib()
    g = torch.Generator().manual_seed(N * 100 + C)
    x = _bf(torch.randn((N, H, W, C), generator=g))
    y0 = _bf(torch.randn((N, Ho, Wo, C), generator=g))
    for acc in (0, 1):
        xd, yd = x.to(cuda), y0.clone().to(cuda)
        _C.check(lib.rn_scatter_add2x(_C.ptr(xd), _C.ptr(yd), N, H, W, C, Ho, Wo, acc, _C.current_stream()))
        torch.cuda.synchronize()
        want = y0.float().clone() if acc else torch.zeros((N, Ho, Wo, C))
        hh, ww = (Ho + 1) // 2, (Wo + 1) // 2
        want[:, ::2, ::2, :] += x.float()[:, :hh, :ww, :]
        assert torch.equal(yd.float().cpu(), want.to(H16).float())


# ---------------------------------------------------------------------------------------------
# A tight test that spans several layers.  The whole-network gradient checks are bounded by the
# restatement's own fp32-vs-fp64 noise (cosines ~0.93 at 640^2): they prove wiring, not numerics; the per-launch tests
# are tight but span one kernel.  Here: one bottleneck tail of the REAL training engine at the bench geometry
#   conv3x3 128->128 -> BN(train) -> ReLU -> conv1x1 128->512 -> BN(train) -> + residual -> ReLU   (80 x 80, B = 32)
# = ResNet-50 `g2b1_b` -> `g2b1_out` at 640 x 640 (resnet.py:194-248), run through TrainEngine.forward / backward
# with its defaults (fused BatchNorm statistics in the conv epilogues, RNET_FUSE_BN_BWD stage 1 in the data-gradient
# epilogue, two streams, grouped weight gradients), and re-derived in float64 from the engine's OWN tensors at the
# slice's boundary — the slice input x, the residual, the upstream gradient dz — with the rounding points the engine has
# (every stored activation / gradient tensor is bf16).  Only what happens INSIDE the slice is compared, so no noise from
# the other 100 layers enters, and the bounds are bf16 rounding: every gradient's cosine > 0.9999 (measured: 0.999998),
# bf16 tensors within 2 ulp on all but <= 2 % and within 4 ulp on all but 0.5 % of the elements (a flipped rounding
# upstream moves a neighbour's sum), fp32 gradients within 2e-3 relative.
def _f64(t):
    return t.double()


def _conv3x3_f64(x, w):
    """x [N,H,W,C] f64 (device), w [3,3,C,K] f64 -> [N,H,W,K]: nine shifted GEMMs (rocBLAS dgemm), pad 1"""
    N, H, W, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    y = torch.zeros((N, H, W, w.shape[3]), dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            y += xp[:, r:r + H, s:s + W, :] @ w[r, s]
    return y


def _conv3x3_dgrad_f64(dy, w):
    N, H, W, K = dy.shape
    dp = torch.nn.functional.pad(dy, (0, 0, 1, 1, 1, 1))
    dx = torch.zeros((N, H, W, w.shape[2]), dtype=torch.float64, device=dy.device)
    for r in range(3):
        for s in range(3):
            dx += dp[:, 2 - r:2 - r + H, 2 - s:2 - s + W, :] @ w[r, s].t()
    return dx


def _conv3x3_wgrad_f64(x, dy):
    N, H, W, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    dw = torch.zeros((3, 3, C, dy.shape[3]), dtype=torch.float64, device=x.device)
    d2 = dy.reshape(-1, dy.shape[3])
    for r in range(3):
        for s in range(3):
            dw[r, s] = xp[:, r:r + H, s:s + W, :].reshape(-1, C).t() @ d2
    return dw


def _bn_train_f64(y, gamma, beta, eps):
    mean = y.mean(dim=(0, 1, 2))
    var = y.var(dim=(0, 1, 2), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (y - mean) * invstd
    return xhat * gamma + beta, xhat, invstd


def _bn_bwd_f64(g, xhat, invstd, gamma):
    """g = gradient wrt the BatchNorm output (after the activation gate) -> (dy, dgamma, dbeta)"""
    dbeta = g.sum(dim=(0, 1, 2))
    dgamma = (g * xhat).sum(dim=(0, 1, 2))
    n = g.shape[0] * g.shape[1] * g.shape[2]
    dy = gamma * invstd * (g - dbeta / n - xhat * dgamma / n)
    return dy, dgamma, dbeta


from ulp_ref import _ulp_outliers   # noqa: E402  (moved unchanged: the gradient-join tests share it)


def test_bottleneck_tail_forward_backward_tight(cuda):
    from retinanet.cfg import default_params
    from retinanet.dataloader import LabelEncoder
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    from make_golden import synth_gt
    size, B = 640, 32
    p = default_params(input_size=size, balanced=True)
    p.architecture.batch_norm.use_sync = False
    builder = ModelBuilder(p, "train", device=cuda, seed=5)
    model = builder()
    gen = torch.Generator().manual_seed(5)
    for k, v in model.variables.items():      # every branch carries signal (the reference zero-inits the last gamma of a block)
        if k.endswith("/gamma"):
            zero_init = model.graph.bns[k[:-len("/gamma")]]["gamma_zero"]
            lo, span = (0.2, 0.3) if zero_init else (0.75, 0.5)
            v.copy_((torch.rand(v.shape, generator=gen) * span + lo).to(cuda))
        elif k.endswith("/beta"):
            v.copy_((torch.randn(v.shape, generator=gen) * 0.1).to(cuda))
    rx = [builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables]
    eng = TrainEngine(model, B, frozen_regexes=rx, world_size=1)
    assert eng.fuse_bn_stats and eng.fuse_bn_bwd and eng.side_stream_on      # the defaults the bench runs
    enc = LabelEncoder(p, device=cuda)
    rng = np.random.default_rng(5)
    gts = [synth_gt(rng, int(rng.integers(2, 9)), size) for _ in range(B)]
    Gmax = max(x[0].shape[0] for x in gts)
    gb, gc, cnt = np.zeros([B, Gmax, 4], np.float32), np.zeros([B, Gmax], np.float32), np.zeros([B], np.int32)
    for i, (b_, c_) in enumerate(gts):
        gb[i, :len(b_)], gc[i, :len(c_)], cnt[i] = b_, c_, len(b_)
    targets = enc.encode_batch(torch.from_numpy(gb), torch.from_numpy(gc), torch.from_numpy(cnt))
    images = torch.randn((B, size, size, 3), generator=gen).to(cuda)
    with torch.cuda.device(cuda):
        eng._step_args = dict(wdc=0.0, alpha=0.0, unscale=1.0, clip=0.0)
        eng._prepack_dgrad_weights()
        preds = eng.forward(images)
        model.loss(targets, preds, compute_grads=True, grad_scale=1.0, grads_bf16=eng.loss_grad_buffers(), normalizer=None)
        eng._train_step_active = True
        try:
            eng.backward(None)
        finally:
            eng._train_step_active = False
        torch.cuda.synchronize()
    ops = {o["out"]: o for o in eng.ops if o["op"] == "conv"}
    ob, oo = ops["g2b1_b"], ops["g2b1_out"]
    assert eng.tensors["g2b1_b"][:3] == (80, 80, 128) and oo["residual"] == "g2b0_out"
    eps = eng.eps
    rb = lambda t: t.to(eng.h16).double()            # a stored bf16 tensor
    var = model.variables
    # ---- boundary tensors, taken from the engine -----------------------------------------------------------------
    x = _f64(eng.t["g2b1_a"])                         # slice input (post BN + ReLU of g2b1_a)
    res = _f64(eng.t["g2b0_out"])
    dz = _f64(eng.grad["g2b1_out"])                  # gradient wrt the block output, all contributions summed
    wb = rb(var[ob["conv"] + "/kernel"].to(cuda))     # kernels as the engine multiplies them: rounded to bf16
    wo = rb(var[oo["conv"] + "/kernel"].to(cuda))[0, 0]
    gam_b, bet_b = _f64(var[ob["bn"] + "/gamma"].to(cuda)), _f64(var[ob["bn"] + "/beta"].to(cuda))
    gam_o, bet_o = _f64(var[oo["bn"] + "/gamma"].to(cuda)), _f64(var[oo["bn"] + "/beta"].to(cuda))
    # ---- forward, float64 with the engine's rounding points ------------------------------------------------------
    yb = rb(_conv3x3_f64(x, wb))                      # Conv2D output: a bf16 tensor
    assert _ulp_outliers(eng.raw["g2b1_b"], _conv3x3_f64(x, wb), 1.0) < 1e-3
    ub, xhat_b, inv_b = _bn_train_f64(yb, gam_b, bet_b, eps)
    zb = rb(torch.relu(ub))
    assert _ulp_outliers(eng.t["g2b1_b"], torch.relu(ub), 2.0) < 2e-3
    yo64 = zb @ wo
    yo = rb(yo64)
    assert _ulp_outliers(eng.raw["g2b1_out"], yo64, 2.0) < 2e-3
    uo, xhat_o, inv_o = _bn_train_f64(yo, gam_o, bet_o, eps)
    so = rb(uo) + res                                 # BatchNorm output is a bf16 tensor, then the add, then ReLU
    zo = torch.relu(so)
    assert _ulp_outliers(eng.t["g2b1_out"], zo, 2.0) < 3e-3
    # ---- backward ---------------------------------------------------------------------------------------------------
    g_o = dz * (so > 0)
    dyo, dgam_o, dbet_o = _bn_bwd_f64(g_o, xhat_o, inv_o, gam_o)
    dyo_r = rb(dyo)
    dzb64 = dyo_r @ wo.t()                            # data gradient of the 1x1 conv = dz of the 3x3 conv's BatchNorm
    dwo = zb.reshape(-1, zb.shape[3]).t() @ dyo_r.reshape(-1, dyo_r.shape[3])
    g_b = rb(dzb64) * (ub > 0)
    dyb, dgam_b, dbet_b = _bn_bwd_f64(g_b, xhat_b, inv_b, gam_b)
    dyb_r = rb(dyb)
    dx64 = _conv3x3_dgrad_f64(dyb_r, wb)
    dwb = _conv3x3_wgrad_f64(x, dyb_r)
    # ---- the engine's gradients --------------------------------------------------------------------------------------
    def cos(a, b):
        a, b = a.double().reshape(-1), b.double().reshape(-1)
        return (a @ b / (a.norm() * b.norm() + 1e-300)).item()

    def rel(a, b):
        return ((a.double() - b).norm() / (b.norm() + 1e-300)).item()

    def kernel_grad(conv):
        c = eng.g.convs[conv]
        return eng._pview(conv + "/kernel", eng.G).reshape(c["cout"], c["k"], c["k"], c["cin"]).permute(1, 2, 3, 0)
    report = {}
    for name, got, want in (("dz(g2b1_b)", eng.grad["g2b1_b"], dzb64), ("dx(g2b1_a)", eng.grad["g2b1_a"], dx64)):
        # dx is a sum of 9 x 128 products of which a few had an input one ulp off (a flipped rounding of dy): 2 ulp on
        # all but ~1 % of the elements, 4 ulp on all but ~0.2 % (measured: 0.72 % / 0.22 %; dz: 0.03 % / 0.01 %)
        report[name] = (cos(got, want), _ulp_outliers(got, want, 2.0), _ulp_outliers(got, want, 4.0))
        assert report[name][0] > 0.9999 and report[name][1] < 2e-2 and report[name][2] < 5e-3, report
    for name, got, want in (("dW out", kernel_grad(oo["conv"])[0, 0], dwo), ("dW b", kernel_grad(ob["conv"]), dwb),
                            ("dgamma out", eng._pview(oo["bn"] + "/gamma", eng.G), dgam_o),
                            ("dbeta out", eng._pview(oo["bn"] + "/beta", eng.G), dbet_o),
                            ("dgamma b", eng._pview(ob["bn"] + "/gamma", eng.G), dgam_b),
                            ("dbeta b", eng._pview(ob["bn"] + "/beta", eng.G), dbet_b)):
        report[name] = (cos(got, want), rel(got, want))
        assert report[name][0] > 0.9999 and report[name][1] < 2e-3, report
    print("bottleneck tail, engine vs float64:", {k: (round(v[0], 7), float(f"{v[1]:.3g}")) for k, v in report.items()})
