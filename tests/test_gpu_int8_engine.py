"""GPU: the INT8 detection heads of InferenceEngine(..., quantization=table) — every int8 launch replayed teacher-forced
through tests/quant_ref.py from the engine's own input buffers (bit for bit), graph capture, weight reloads, the f16 build and
the `python -m retinanet.export --precision int8` round trip."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import quant_ref as qr
from engine_cases import INFER_ENGINES, _infer_engine

pytestmark = pytest.mark.gpu

_BUILT = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _BUILT.clear()


def _int8_engine(eng16, variables, table, capture_graph=False):
    from retinanet.model.engine import InferenceEngine
    return InferenceEngine(eng16.g, variables, eng16.B, eng16.dev, bn_epsilon=eng16.eps, capture_graph=capture_graph,
                           f16=eng16.f16, quantization=table)


def _case(cuda, name):
    """(16-bit engine, variables, images, minmax table from two seeded batches, int8 engine after one pass)"""
    if name not in _BUILT:
        from retinanet.model.quantization import Calibrator
        model, size, B, kw = INFER_ENGINES[name]
        eng16, variables, images = _infer_engine(cuda, model, size, B, **kw)
        second = torch.randn(images.shape, generator=torch.Generator().manual_seed(99)) * 1.5
        table = Calibrator(eng16, "minmax").run([images, second])
        eng8 = _int8_engine(eng16, variables, table)
        eng8(images.to(cuda))
        torch.cuda.synchronize()
        _BUILT[name] = (eng16, variables, images, table, eng8)
    return _BUILT[name]


def _fold64(s_in, ws, variables, op, eps):
    """the test's own float64 folding: mul = s_in * w_scale * bn_scale, add = bias * bn_scale + bn_shift, rounded once"""
    f64 = lambda n: variables[n].detach().cpu().numpy().astype(np.float64)
    cout = ws.shape[0]
    scale, shift = np.ones(cout), np.zeros(cout)
    if op.get("bn"):
        scale = f64(op["bn"] + "/gamma") / np.sqrt(f64(op["bn"] + "/moving_variance") + np.float64(eps))
        shift = f64(op["bn"] + "/beta") - f64(op["bn"] + "/moving_mean") * scale
    bias = f64(op["conv"] + "/bias")
    return (np.float64(s_in) * ws.astype(np.float64) * scale).astype(np.float32), (bias * scale + shift).astype(np.float32)


def _replay(eng8, variables, table):
    """every int8 step from the buffers the engine left: returns the number of compared tensors"""
    g, compared = eng8.g, 0
    inv = lambda name: np.float32(1.0) / np.float32(table.scales[name])
    for n in eng8.int8.sources:                                   # the quantiser launch
        C = g.tensors[n][2]
        want = qr.quantize(eng8.t[n][..., :C].float().cpu().numpy(), inv(n))
        assert eng8.t[n + ":i8"].dtype == torch.int8 and np.array_equal(eng8.t[n + ":i8"].cpu().numpy(), want), n
        compared += 1
    weights = {}
    for name, ops in eng8.int8.launches:
        assert len(ops) <= 10
        for op in ops:
            if op["conv"] not in weights:
                w = variables[op["conv"] + "/kernel"].detach().cpu().numpy().transpose(3, 0, 1, 2)
                weights[op["conv"]] = qr.quantize_weights(np.ascontiguousarray(w))
            wq, ws = weights[op["conv"]]
            x = eng8.t[eng8.int8.x_name(op)].cpu().numpy()
            assert x.dtype == np.int8
            mul, add = _fold64(table.scales[op["inp"]], ws, variables, op, eng8.eps)
            got = eng8.t[op["out"]].cpu().numpy()
            if op["out_dtype"] == "f32":
                want = qr.conv3x3_i8(x, wq, mul, add, op["act"])
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, op["out"])
            else:
                want = qr.conv3x3_i8(x, wq, mul, add, op["act"], inv(op["out"]))
                assert got.dtype == np.int8 and np.array_equal(got, want), (name, op["out"])
                assert np.abs(want).max() > 16, (name, op["out"])       # the level carries signal
            compared += 1
    return compared


def _outputs(eng):
    return {k: {lv: t.clone() for lv, t in d.items()} for k, d in eng.outputs.items()}


def _same(a, b):
    return all(torch.equal(a[k][lv], b[k][lv]) for k in a for lv in a[k])


@pytest.mark.parametrize("name", ["resnet26-balanced-relu", "resnet26-plain-relu6", "resnet26-batch4", "resnet26-f16"])
def test_every_int8_step_teacher_forced(cuda, name):
    eng16, variables, images, table, eng8 = _case(cuda, name)
    assert table.method == "minmax" and table.num_images == 2 * eng16.B and len(table.scales) == 45
    # the launch list: one quantiser, four tower launches of ten segments, the two prediction launches
    names = [n for _, n in eng8.steps]
    i8 = [n for n in names if n.startswith(("quantize_i8:", "conv_i8:"))]
    assert i8 == ["quantize_i8:heads"] + [f"conv_i8:tower{i}" for i in range(4)] + ["conv_i8:pred_box", "conv_i8:pred_class"]
    assert not [n for n in names if n.startswith("conv:") and ("tower" in n or "pred_" in n)]
    assert [len(ops) for _, ops in eng8.int8.launches] == [10, 10, 10, 10, 5, 5]
    assert all(n in eng8.step_io for n in i8)
    assert _replay(eng8, variables, table) == 5 + 50
    # backbone and FPN are untouched: the head inputs are the 16-bit engine's, bit for bit
    eng16(images.to(cuda))
    torch.cuda.synchronize()
    for n in eng8.int8.sources:
        assert torch.equal(eng8.t[n], eng16.t[n]), n
    for k, d in eng8.outputs.items():
        for lv, t in d.items():
            assert t.dtype == torch.float32 and t.shape == eng16.outputs[k][lv].shape and bool(torch.isfinite(t).all())


@pytest.mark.parametrize("name", ["resnet26-balanced-relu", "resnet26-batch4"])
def test_captured_graph_equals_uncaptured(cuda, name):
    eng16, variables, images, table, eng8 = _case(cuda, name)
    want = _outputs(eng8)
    cap = _int8_engine(eng16, variables, table, capture_graph=True)
    for _ in range(2):                       # the capture pass, then a pure replay
        cap(images.to(cuda))
        torch.cuda.synchronize()
        assert _same(_outputs(cap), want)
    for n in eng8.int8.names:
        key = n if n in eng8.int8.outs else n + ":i8"
        assert torch.equal(cap.t[key], eng8.t[key]), n


def test_load_variables_repacks_in_place(cuda):
    eng16, variables, images, table, eng8 = _case(cuda, "resnet26-balanced-relu")
    x = images.to(cuda)
    eng8(x)
    torch.cuda.synchronize()
    before = _outputs(eng8)
    addr = {k: v.data_ptr() for k, v in eng8.int8.packed.items()}
    changed = {k: v.clone() for k, v in variables.items()}
    g = torch.Generator().manual_seed(7)
    for k, v in changed.items():
        if "head" in k and (k.endswith("/kernel") or k.endswith("/gamma")):
            v.mul_((torch.rand(v.shape, generator=g) * 0.5 + 0.75).to(v.device))
    with torch.cuda.device(cuda):
        eng8.load_variables(changed)
    eng8(x)
    torch.cuda.synchronize()
    assert not _same(_outputs(eng8), before)
    assert _replay(eng8, changed, table) == 55
    with torch.cuda.device(cuda):
        eng8.load_variables(variables)
    eng8(x)
    torch.cuda.synchronize()
    assert _same(_outputs(eng8), before)
    assert addr == {k: v.data_ptr() for k, v in eng8.int8.packed.items()}


def test_refused_tables_and_configs(cuda):
    from retinanet.model.quantization import QuantizationTable
    eng16, variables, images, table, eng8 = _case(cuda, "resnet26-balanced-relu")
    short = QuantizationTable({k: v for k, v in list(table.scales.items())[:-1]}, "minmax", 4)
    with pytest.raises(ValueError, match="no scale"):
        _int8_engine(eng16, variables, short)
    model, size, B, kw = INFER_ENGINES["efficientnet-b0"]
    from retinanet.cfg import efficientnet_params
    from retinanet.model import ModelBuilder
    net = ModelBuilder(efficientnet_params(model, input_size=size), "val", device=cuda)()
    with pytest.raises(NotImplementedError, match="separable"):
        net.inference_engine(B, quantization=table)


# ---- export round trip -------------------------------------------------------------------------------------------------
def _write_png(path, rgb):
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


@pytest.fixture(scope="module")
def exported(tmp_path_factory, cuda):
    """a tiny ResNet-14 config with a checkpoint of random weights, three generated PNGs, and two exports of it: with
    --precision int8 (entropy, three images in batches of two: the last batch is padded) and without --precision"""
    from retinanet import export
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    tmp = tmp_path_factory.mktemp("int8_export")
    p = default_params(input_size=128, inference_batch=2)
    p.architecture.backbone.depth = 14
    p.architecture.batch_norm.use_sync = False
    p.experiment.name = "tiny8"
    p.experiment.model_dir = str(tmp / "model_files")
    p.training.optimizer.use_moving_average = False
    net = ModelBuilder(p, "val", device=cuda)()
    g = torch.Generator().manual_seed(2)
    for k, v in net.variables.items():
        if "head" in k and k.endswith("/kernel"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.02).to(v.device))
    os.makedirs(os.path.join(p.experiment.model_dir, "tiny8"))
    net.save_weights(os.path.join(p.experiment.model_dir, "tiny8", "weights_step_0"))
    cfg = tmp / "config.json"
    cfg.write_text(json.dumps(p))
    rng = np.random.default_rng(3)
    os.makedirs(tmp / "calib")
    for i, (h, w) in enumerate([(60, 90), (128, 128), (150, 70)]):
        _write_png(tmp / "calib" / f"img{i}.png", rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    base = ["--config_path", str(cfg), "--mode", "tf", "--export_saved_model"]
    export.main(base + ["--export_dir", str(tmp / "e8"), "--precision", "int8", "--calibration_method", "entropy",
                        "--calibration_images_dir", str(tmp / "calib"), "--num_calibration_images", "3",
                        "--calibration_batch_size", "2"])
    export.main(base + ["--export_dir", str(tmp / "e16")])
    return tmp, p


def test_export_round_trips_through_precision_int8(exported, cuda):
    from retinanet import export
    from retinanet.model.quantization import FORMAT_VERSION, calibrated_tensors
    tmp, p = exported
    d = tmp / "e8" / "tiny8" / "tf"
    meta = json.load(open(d / "signatures.json"))
    q = json.load(open(d / "quantization.json"))
    assert meta["precision"] == "int8"
    assert q["method"] == "entropy" and q["num_images"] == 3 and q["version"] == FORMAT_VERSION
    sm = export.load(str(d), device=cuda)
    assert set(q["scales"]) == set(calibrated_tensors(sm.model.graph)) and all(v > 0 for v in q["scales"].values())
    image = torch.randn((2, 128, 128, 3), generator=torch.Generator().manual_seed(4))
    det = sm.signatures["serving_default"](image=image)
    spec = meta["signatures"]["serving_default"]["outputs"]
    assert set(det) == {"boxes", "scores", "classes", "valid_detections"}
    for k, v in det.items():
        assert list(v.shape) == spec[k]["shape"] and str(v.dtype) == "torch." + spec[k]["dtype"], k
    engines = list(sm.model._engines.values())
    assert len(engines) == 1 and engines[0].int8 is not None and engines[0].int8.table.scales == q["scales"]


def test_export_without_precision_loads_the_old_engine(exported, cuda):
    from retinanet import export
    tmp, p = exported
    d = tmp / "e16" / "tiny8" / "tf"
    assert "precision" not in json.load(open(d / "signatures.json")) and not (d / "quantization.json").exists()
    sm = export.load(str(d), device=cuda)
    det = sm.signatures["serving_default"](image=torch.zeros((2, 128, 128, 3)))
    assert det["boxes"].shape == (2, 100, 4)
    engines = list(sm.model._engines.values())
    assert sm.quantization is None and len(engines) == 1 and engines[0].int8 is None
    assert not [n for _, n in engines[0].steps if "i8" in n]
