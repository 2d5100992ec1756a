"""GPU: the INT8 kernels of rn_conv_i8.hip against tests/quant_ref.py, bit for bit, at the smallest shapes where they can
go wrong: maps smaller than the halo, a one-pixel map, odd widths, a tile and an image seam inside one segment, one and two
K steps per tap, channel counts below / at / above the channel tile, |acc| > 2^24 and the clamp, both output types, all
three activations, sentinels around every output."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import quant_ref as qr

pytestmark = pytest.mark.gpu

ACTS = ("none", "relu", "relu6")
GUARD = 64          # sentinel elements in front of and behind every output
MAPS5 = (10, 5, 3, 2, 1)


def _lib(f16=False):
    from retinanet import _C
    return _C, _C.lib(f16)


def _pack(cuda, w_ohwi, layout_ohwi=True):
    """f32 [Cout,3,3,Cin] -> (packed int8 device buffer, w_scale device f32) through rn_pack_conv_weight_i8"""
    _C, lib = _lib()
    cout, _, _, cin = w_ohwi.shape
    src = w_ohwi if layout_ohwi else np.ascontiguousarray(w_ohwi.transpose(1, 2, 3, 0))
    wd = torch.from_numpy(np.ascontiguousarray(src)).to(cuda)
    nbytes = lib.rn_conv_i8_weight_bytes(cin, cout)
    assert nbytes == -(-cout // 128) * 128 * 9 * cin
    packed = torch.full((nbytes,), 77, dtype=torch.int8, device=cuda)
    scale = torch.full((cout,), -1.0, dtype=torch.float32, device=cuda)
    _C.check(lib.rn_pack_conv_weight_i8(_C.ptr(wd), 1 if layout_ohwi else 0, cin, cout, _C.ptr(packed), _C.ptr(scale),
                                        _C.current_stream()), "rn_pack_conv_weight_i8")
    return packed, scale


def _launch(cuda, segs, act, out_f32):
    """segs: dicts x (int8 [N,H,W,Cin] numpy), packed (device), cout, mul, add (numpy f32), inv.  -> per segment the whole
    output buffer (guards included) as numpy"""
    _C, lib = _lib()
    p = _C.ConvI8Problem()
    p.act, p.out_dtype, p.num_segments = _C.ACT_IDS[act], (_C.RN_DT_F32 if out_f32 else _C.RN_DT_I8), len(segs)
    keep, outs = [], []
    for i, sg in enumerate(segs):
        x = torch.from_numpy(sg["x"]).to(cuda)
        mul, add = torch.from_numpy(sg["mul"]).to(cuda), torch.from_numpy(sg["add"]).to(cuda)
        n, h, w, cin = sg["x"].shape
        numel = n * h * w * sg["cout"]
        if out_f32:
            y = torch.full((numel + 2 * GUARD,), -12345.5, dtype=torch.float32, device=cuda)
        else:
            y = torch.full((numel + 2 * GUARD,), -77, dtype=torch.int8, device=cuda)
        keep += [x, mul, add]
        outs.append(y)
        s = p.seg[i]
        s.x, s.w, s.y = x.data_ptr(), sg["packed"].data_ptr(), y[GUARD:].data_ptr()
        s.mul, s.add, s.out_inv_scale = mul.data_ptr(), add.data_ptr(), float(sg.get("inv", 1.0))
        s.N, s.H, s.W, s.Cin, s.Cout = n, h, w, cin, sg["cout"]
    _C.check(lib.rn_conv3x3_i8_fwd(ctypes.byref(p), _C.current_stream()), "rn_conv3x3_i8_fwd")
    torch.cuda.synchronize()
    return [y.cpu().numpy() for y in outs]


def _check(got, want, out_f32):
    sentinel = np.float32(-12345.5) if out_f32 else np.int8(-77)
    assert (got[:GUARD] == sentinel).all() and (got[-GUARD:] == sentinel).all(), "bytes outside [N,H,W,Cout] changed"
    body = got[GUARD:-GUARD].reshape(want.shape)
    if out_f32:
        assert np.array_equal(body.view(np.uint32), want.view(np.uint32))
    else:
        assert np.array_equal(body, want)


@functools.lru_cache(maxsize=None)
def _case(cin, cout, maps, n, seed):
    """random int8 inputs / f32 weights and the int64 accumulators of every segment (computed once per shape)"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((cout, 3, 3, cin)) * 0.02).astype(np.float32)
    wq, ws = qr.quantize_weights(w)
    xs = [rng.integers(-127, 128, size=(n, m, m, cin), dtype=np.int64).astype(np.int8) for m in maps]
    accs = [qr.conv3x3_int(x, wq) for x in xs]
    return w, wq, ws, xs, accs


def _epilogue_vectors(rng, acc, ws, cout, i):
    """per-level mul / add as the engine folds them: s_in * w_scale * bn_scale, a shift of the size of the outputs"""
    bn = rng.uniform(0.75, 1.25, cout)
    s_in = (4.0 + 2.0 * i) / float(np.abs(acc.astype(np.float64) * (ws.astype(np.float64) * bn)).max())   # outputs reach 4 .. 12: relu6 clips
    mul = (s_in * ws.astype(np.float64) * bn).astype(np.float32)
    spread = float(np.abs(acc.astype(np.float64) * mul).max()) + 1e-6
    add = rng.uniform(-0.3 * spread, 0.3 * spread, cout).astype(np.float32)
    return mul, add, spread


@pytest.mark.parametrize("cin,cout", [(64, 36), (64, 256), (64, 720), (128, 36), (128, 256), (128, 720)])
def test_five_segment_launch(cuda, cin, cout):
    """maps 10^2, 5^2, 3^2, 2^2, 1^2 at N = 2 in ONE launch, every activation, both output types"""
    w, wq, ws, xs, accs = _case(cin, cout, MAPS5, 2, 11)
    packed, scale = _pack(cuda, w)
    assert np.array_equal(scale.cpu().numpy(), ws)
    rng = np.random.default_rng(5)
    vec = [_epilogue_vectors(rng, accs[i], ws, cout, i) for i in range(len(MAPS5))]
    for act in ACTS:
        for out_f32 in (False, True):
            segs = []
            for i, x in enumerate(xs):
                mul, add, spread = vec[i]
                top = min(spread, 6.0) if act == "relu6" else spread
                segs.append(dict(x=x, packed=packed, cout=cout, mul=mul, add=add, inv=np.float32(127.0 / (0.8 * top))))
            got = _launch(cuda, segs, act, out_f32)
            for i, sg in enumerate(segs):
                want = qr.epilogue(accs[i], sg["mul"], sg["add"], act, None if out_f32 else sg["inv"])
                _check(got[i], want, out_f32)
                if not out_f32 and i == 0:
                    assert np.abs(want).max() == 127 and len(np.unique(want)) > 50   # the case exercises the range


@pytest.mark.parametrize("out_f32", [False, True])
def test_tile_and_image_seam(cuda, out_f32):
    """20 x 20 at N = 2: 800 pixels cross a tile boundary and the image boundary inside one segment"""
    w, wq, ws, xs, accs = _case(64, 256, (20,), 2, 12)
    packed, _ = _pack(cuda, w, layout_ohwi=False)
    mul, add, spread = _epilogue_vectors(np.random.default_rng(6), accs[0], ws, 256, 0)
    inv = np.float32(127.0 / spread)
    got = _launch(cuda, [dict(x=xs[0], packed=packed, cout=256, mul=mul, add=add, inv=inv)], "relu", out_f32)
    _check(got[0], qr.epilogue(accs[0], mul, add, "relu", None if out_f32 else inv), out_f32)


@pytest.mark.parametrize("out_f32", [False, True])
def test_saturation(cuda, out_f32):
    """Cin 512, every input and weight +-127: |acc| reaches 9 * 512 * 127^2 > 2^24 (the int32 -> f32 conversion rounds)
    and the int8 output clamps; Cout 7 takes the unpacked stores"""
    cin, cout = 512, 7
    rng = np.random.default_rng(13)
    w = np.full((cout, 3, 3, cin), 127.0, dtype=np.float32)
    w[1] = -127.0
    w[2] = np.where(rng.random((3, 3, cin)) < 0.5, -127.0, 127.0)
    w[3, :, :, ::3] = -127.0
    x = np.full((2, 3, 3, cin), 127, dtype=np.int8)
    x[1] = np.where(rng.random((3, 3, cin)) < 0.25, -127, 127).astype(np.int8)
    wq, ws = qr.quantize_weights(w)
    assert np.abs(wq).min() == 127
    acc = qr.conv3x3_int(x, wq)
    assert np.abs(acc).max() == 9 * 512 * 127 * 127 and (np.abs(acc) > 2 ** 24).sum() > 10
    assert (acc.astype(np.int32).astype(np.float32).astype(np.int64) != acc).any()     # the conversion does round here
    packed, _ = _pack(cuda, w)
    mul = np.array([1e-6, 1e-5, 3e-5, 2e-6, 1e-5, 1.7e-6, 1.0], dtype=np.float32)
    add = np.array([0.25, -0.25, 0.0, 1.5, -3.0, 0.0, 0.5], dtype=np.float32)
    inv = np.float32(1.0)
    got = _launch(cuda, [dict(x=x, packed=packed, cout=cout, mul=mul, add=add, inv=inv)], "none", out_f32)
    want = qr.epilogue(acc, mul, add, "none", None if out_f32 else inv)
    if not out_f32:
        assert (want == 127).any() and (want == -127).any() and (np.abs(want) < 127).any()
    _check(got[0], want, out_f32)


def test_refusals(cuda):
    _C, lib = _lib()
    buf = torch.zeros(1 << 20, dtype=torch.int8, device=cuda)
    f = torch.zeros(1024, dtype=torch.float32, device=cuda)

    def status(cin=64, cout=8, act=_C.RN_ACT_RELU, dt=_C.RN_DT_I8, nseg=1):
        p = _C.ConvI8Problem()
        p.act, p.out_dtype, p.num_segments = act, dt, nseg
        s = p.seg[0]
        s.x = s.w = s.y = buf.data_ptr()
        s.mul = s.add = f.data_ptr()
        s.out_inv_scale = 1.0
        s.N, s.H, s.W, s.Cin, s.Cout = 1, 2, 2, cin, cout
        return lib.rn_conv3x3_i8_fwd(ctypes.byref(p), _C.current_stream())
    assert status() == _C.RN_OK
    assert status(act=_C.RN_ACT_SWISH) == _C.RN_EINVAL
    assert status(cin=32) == _C.RN_EINVAL and status(cin=96) == _C.RN_EINVAL and status(cin=576) == _C.RN_EINVAL
    assert status(cout=0) == _C.RN_EINVAL and status(dt=_C.RN_DT_BF16) == _C.RN_EINVAL
    assert status(nseg=0) == _C.RN_EINVAL and status(nseg=11) == _C.RN_EINVAL
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout_ohwi", [True, False])
def test_pack_weights(cuda, layout_ohwi):
    """scales and bytes of both source layouts; a zero channel gets scale 1; pad rows are zero"""
    cin, cout = 64, 37
    rng = np.random.default_rng(21)
    w = (rng.standard_normal((cout, 3, 3, cin)) * np.exp(rng.uniform(-6, 2, (cout, 1, 1, 1)))).astype(np.float32)
    w[5] = 0.0
    wq, ws = qr.quantize_weights(w)
    packed, scale = _pack(cuda, w, layout_ohwi)
    assert ws[5] == 1.0 and np.array_equal(scale.cpu().numpy(), ws)
    rows = packed.cpu().numpy().reshape(128, 3, 3, cin)
    assert np.array_equal(rows[:cout], wq) and not rows[cout:].any()


@pytest.mark.parametrize("f16", [False, True])
def test_quantize_and_calibration_kernels(cuda, f16):
    """rn_quantize_i8 (grouped, pix_stride > C, element counts that are no multiple of any vector width), rn_calib_absmax
    and rn_calib_histogram (both accumulated over two calls) against numpy, in both storage types"""
    _C, lib = _lib(f16)
    h16 = torch.float16 if f16 else torch.bfloat16
    gen = torch.Generator().manual_seed(31)
    shapes = [(37, 3, 5), (211, 64, 72), (1, 1, 1), (1000, 7, 8), (63, 256, 256)]     # (pixels, C, pix_stride)
    xs = [(torch.randn((p, ps), generator=gen) * (0.5 + i)).to(h16) for i, (p, c, ps) in enumerate(shapes)]
    xs[1][3, 2] = 1e4      # clamps
    xs[1][4, 2] = -1e4
    prob = _C.QuantProblem()
    prob.num_segments = len(shapes)
    dev_x, dev_y, inv = [], [], []
    for i, ((p, c, ps), x) in enumerate(zip(shapes, xs)):
        dx = x.to(cuda)
        dy = torch.full((p * c + 2 * GUARD,), -77, dtype=torch.int8, device=cuda)
        dev_x.append(dx)
        dev_y.append(dy)
        inv.append(np.float32(127.0 / (2.0 + i)))
        s = prob.seg[i]
        s.x, s.y, s.pixels, s.C, s.pix_stride, s.inv_scale = dx.data_ptr(), dy[GUARD:].data_ptr(), p, c, ps, float(inv[i])
    _C.check(lib.rn_quantize_i8(ctypes.byref(prob), _C.current_stream()), "rn_quantize_i8")
    torch.cuda.synchronize()
    for (p, c, ps), x, dy, iv in zip(shapes, xs, dev_y, inv):
        got = dy.cpu().numpy()
        want = qr.quantize(x[:, :c].float().numpy(), iv)
        assert (got[:GUARD] == -77).all() and (got[-GUARD:] == -77).all()
        assert np.array_equal(got[GUARD:-GUARD].reshape(p, c), want)
    # calibration: two calls accumulate; the pad channels (pix_stride > C) are never read
    (p, c, ps), a, b = shapes[1], dev_x[1], (dev_x[1] * 0.5).to(h16)
    a_np, b_np = a.cpu().float().numpy()[:, :c], b.cpu().float().numpy()[:, :c]
    amax = torch.zeros(1, dtype=torch.float32, device=cuda)
    for t in (b, a):
        _C.check(lib.rn_calib_absmax(_C.ptr(t), p, c, ps, _C.ptr(amax), _C.current_stream()), "rn_calib_absmax")
    assert amax.item() == max(np.abs(a_np).max(), np.abs(b_np).max())
    x3, (p3, c3, ps3) = dev_x[3], shapes[3]
    x3_np = x3.cpu().float().numpy()[:, :c3]
    rng_ = float(np.abs(x3_np).max()) * 0.75          # values above the range land in the last bin
    counts = torch.zeros(_C.RN_CALIB_BINS, dtype=torch.int64, device=cuda)
    for _ in range(2):
        _C.check(lib.rn_calib_histogram(_C.ptr(x3), p3, c3, ps3, rng_, _C.ptr(counts), _C.current_stream()),
                 "rn_calib_histogram")
    want = qr.histogram(x3_np, rng_)
    got = counts.cpu().numpy()
    assert want[-1] > 0 and got.sum() == 2 * p3 * c3 and np.array_equal(got, 2 * want)
    assert lib.rn_calib_histogram(_C.ptr(x3), p3, c3, ps3, 0.0, _C.ptr(counts), _C.current_stream()) == _C.RN_EINVAL
