"""CPU: the host side of INT8 serving (retinanet/model/quantization.py) against tests/quant_ref.py — the KL threshold
search, the scale rules, the mul / add folding, the table's file format and the configs the mode refuses."""
import numpy as np
import pytest

import quant_ref as qr


def _hist(seed):
    """a seeded 2048-bin histogram of |x| the way calibration sees it: a bulk, a long thin tail, some empty bins"""
    rng = np.random.default_rng(seed)
    bulk = np.abs(rng.standard_normal(200_000)) * (0.03 + 0.03 * seed)
    tail = rng.uniform(0.5, 1.0, 3 * seed)
    x = np.concatenate([bulk, tail, [1.0]]).astype(np.float32)
    h = qr.histogram(x, 1.0)
    h[rng.integers(0, 2048, 150)] = 0
    return h


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_vectorised_kl_search_equals_the_loop_form(seed):
    from retinanet.model import quantization as q
    h = _hist(seed)
    want = qr.kl_threshold_bin(h)
    assert 128 <= want < 2048                         # the tail is clipped: the search has something to decide
    assert q.kl_threshold_bin(h) == want
    assert q.entropy_scale(h, 3.5) == qr.entropy_scale(h, 3.5)


def test_flat_histogram_keeps_the_full_range():
    from retinanet.model import quantization as q
    h = np.full(2048, 37, dtype=np.int64)
    assert qr.kl_threshold_bin(h) == 2048 and q.kl_threshold_bin(h) == 2048
    assert q.entropy_scale(h, 2.0) == 2.0 / 127.0


def test_scaling_the_data_by_two_scales_every_scale_by_exactly_two():
    from retinanet.model import quantization as q
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(50_000) * 0.3).astype(np.float32)
    x[:20] *= 9.0
    a1, a2 = np.abs(x).max(), np.abs(2 * x).max()
    assert q.minmax_scale(a2) == 2.0 * q.minmax_scale(a1)
    h1, h2 = qr.histogram(x, a1), qr.histogram(2 * x, a2)
    assert np.array_equal(h1, h2)
    assert q.entropy_scale(h2, a2) == 2.0 * q.entropy_scale(h1, a1)
    assert q.minmax_scale(0.0) == 1.0 and q.entropy_scale(np.zeros(2048), 0.0) == 1.0


def test_mul_add_folding_is_conv_bias_batchnorm():
    """acc * mul + add against a float64 evaluation of BN(conv(x_real, w_real) + bias) on the dequantised operands"""
    from retinanet.model import quantization as q
    rng = np.random.default_rng(5)
    cin, cout, eps, s_in = 64, 24, 1e-3, 0.0173
    w = (rng.standard_normal((cout, 3, 3, cin)) * 0.03).astype(np.float32)
    wq, ws = qr.quantize_weights(w)
    xq = rng.integers(-127, 128, (1, 4, 5, cin)).astype(np.int8)
    bias = (rng.standard_normal(cout) * 0.05).astype(np.float32)
    gamma, beta = rng.uniform(0.75, 1.25, cout).astype(np.float32), (rng.standard_normal(cout) * 0.1).astype(np.float32)
    mean, var = (rng.standard_normal(cout) * 0.1).astype(np.float32), rng.uniform(0.75, 1.25, cout).astype(np.float32)
    acc = qr.conv3x3_int(xq, wq)
    for bn in (None, (gamma, beta, mean, var)):
        mul, add = q.fold_epilogue(s_in, ws, bias, bn, eps)
        assert mul.dtype == add.dtype == np.float32
        conv = acc.astype(np.float64) * (np.float64(s_in) * ws.astype(np.float64)) + bias.astype(np.float64)
        want = conv if bn is None else ((conv - mean.astype(np.float64)) / np.sqrt(var.astype(np.float64) + eps)
                                        * gamma.astype(np.float64) + beta.astype(np.float64))
        got = acc.astype(np.float64) * mul.astype(np.float64) + add.astype(np.float64)
        # mul and add are each rounded once to f32 (2^-24 relative), everything else here is float64
        bound = 2.0 ** -23 * (np.abs(acc.astype(np.float64) * mul) + np.abs(add)) + 1e-12
        assert (np.abs(got - want) <= bound).all()
        got32 = qr.epilogue(acc, mul, add, "none")
        assert np.abs(got32 - want).max() <= 4 * 2.0 ** -23 * np.abs(want).max()
    m0, a0 = q.fold_epilogue(s_in, ws, None, None, eps)
    assert not a0.any() and np.array_equal(m0, (np.float64(s_in) * ws.astype(np.float64)).astype(np.float32))


def test_quantization_json_round_trips(tmp_path):
    from retinanet.model import quantization as q
    rng = np.random.default_rng(6)
    scales = {f"box-head_t{i}_p{l}": float(rng.uniform(1e-4, 3.0)) for i in range(3) for l in range(3, 8)}
    scales["fpn_out3"] = float(np.float32(0.1)) / 127.0
    t = q.QuantizationTable(scales, "entropy", 24)
    path = tmp_path / "quantization.json"
    t.save(path)
    back = q.QuantizationTable.load(path)
    assert back.scales == t.scales and back.method == "entropy" and back.num_images == 24 and back.key == t.key
    import json
    d = json.load(open(path))
    assert d["version"] == q.FORMAT_VERSION and d["method"] == "entropy" and d["num_images"] == 24
    assert set(d["scales"]) == set(scales)
    d["version"] += 1
    with pytest.raises(ValueError):
        q.QuantizationTable.from_json(d)
    with pytest.raises(ValueError):
        q.QuantizationTable({"a": 0.0}, "minmax", 1)
    with pytest.raises(ValueError):
        q.QuantizationTable({"a": 1.0}, "percentile", 1)
    assert q.QuantizationTable(scales, "minmax", 24).key != t.key


def test_refusals():
    from retinanet.cfg import default_params, efficientnet_params
    from retinanet.model import quantization as q
    from retinanet.model.graph import build_retinanet_graph
    plan = q.head_plan(build_retinanet_graph(default_params(input_size=128)))
    assert len(plan) == 2 * 5 * 5 and len(q.calibrated_tensors(build_retinanet_graph(default_params(input_size=128)))) == 45
    with pytest.raises(NotImplementedError, match="separable"):
        q.head_plan(build_retinanet_graph(efficientnet_params("efficientnet-b0", input_size=256)))
    with pytest.raises(NotImplementedError, match="swish"):
        q.head_plan(build_retinanet_graph(default_params(input_size=128, activation="swish")))
    p = default_params(input_size=128)
    p.architecture.feature_fusion.filters = p.architecture.head.filters = 160
    with pytest.raises(NotImplementedError, match="multiple of 64"):
        q.head_plan(build_retinanet_graph(p))


def test_empty_calibration_directory_is_a_value_error(tmp_path):
    from retinanet.model import quantization as q
    (tmp_path / "notes.txt").write_text("no images here")
    with pytest.raises(ValueError):
        q.list_calibration_images(str(tmp_path), 8)
    for name in ("b.png", "a.jpg", "c.jpeg", "d.bmp"):
        (tmp_path / name).write_bytes(b"")
    got = [f.rsplit("/", 1)[1] for f in q.list_calibration_images(str(tmp_path), 2)]
    assert got == ["a.jpg", "b.png"]
