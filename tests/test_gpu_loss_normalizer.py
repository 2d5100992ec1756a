"""GPU: the moving-average loss normaliser (loss.normalizer.use_moving_average) — the kernel rn_loss_normalizer_ema bit
for bit against normalizer_ref.py in both builds, RetinaNetLoss with the option on against the option off fed the reference
value, the training engine, checkpoint / resume, and two ranks (replica-local: no sum over ranks, no division)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

import normalizer_ref as N
from conftest import PKG

pytestmark = pytest.mark.gpu

BUILDS = ["bf16", "f16"]
SIZES = [1, 2, 63, 64, 65, 256, 1000]     # a partial wave, exactly one wave, the first strided element, many strides
MOMENTA = [0.99, 0.9, 0.5, 0.0, 1.0]
KEY = "loss/moving_average_normalizer"


def _lib(build):
    from retinanet import _C
    return _C.lib(build == "f16")


def _counts(n, seed):
    """integer-valued counts in [0, 16000] with zeros among them (n = 1: a zero count for odd seeds)"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 16001, n).astype(np.float32)
    c[rng.integers(0, n, max(1, n // 8))] = 0.0
    if n == 1:
        c[0] = 0.0 if seed % 2 else 16000.0
    return c


# ---- 1. kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_kernel_bit_exact(cuda, build):
    """state' and the normaliser, uint32 view, against the three-rounding float32 restatement: `state` and `normalizer`
    aliased and as two buffers, from the initial state 0 and from a state with a full mantissa"""
    from retinanet import _C
    lib, st = _lib(build), _C.current_stream()
    cases = [(n, m, s0) for n in SIZES for m in MOMENTA for s0 in (0.0, 1234.5677)]
    counts = {n: _counts(n, n) for n in SIZES}
    assert any((c == 0).any() for c in counts.values()) and max(c.sum() for c in counts.values()) + 1 < 1 << 24
    dev_counts = {n: torch.from_numpy(c).to(cuda) for n, c in counts.items()}
    init = torch.tensor([s0 for _, _, s0 in cases], dtype=torch.float32)
    alias = init.clone().to(cuda)                       # row i: state = normalizer = alias[i]
    state, norm = init.clone().to(cuda), torch.full((len(cases),), -7.0, device=cuda)
    for i, (n, m, _) in enumerate(cases):
        a, s, o = alias[i:i + 1], state[i:i + 1], norm[i:i + 1]
        _C.check(lib.rn_loss_normalizer_ema(_C.ptr(dev_counts[n]), n, m, _C.ptr(a), _C.ptr(a), st), "aliased")
        _C.check(lib.rn_loss_normalizer_ema(_C.ptr(dev_counts[n]), n, m, _C.ptr(s), _C.ptr(o), st), "two buffers")
    torch.cuda.synchronize()
    want = np.asarray([N.ema_step(np.float32(s0), N.value(counts[n]), m) for n, m, s0 in cases], dtype=np.float32)
    for name, got in (("aliased", alias), ("state", state), ("normalizer", norm)):
        bad = np.nonzero(N.bits(got.cpu().numpy()) != N.bits(want))[0]
        assert bad.size == 0, (name, [(cases[i], float(got[i]), float(want[i])) for i in bad[:4]])
    for n, c in counts.items():                          # the inputs are read only
        assert np.array_equal(dev_counts[n].cpu().numpy(), c)


@pytest.mark.parametrize("build", BUILDS)
def test_kernel_replays_the_seed0_sequence(cuda, build):
    """the 2000 steps of test_loss_normalizer_cpu.py through the kernel, the state fed back on the device: every step bit-equal
    to the three-rounding form — which differs from the fused form at 5 of them"""
    from retinanet import _C
    lib, st = _lib(build), _C.current_stream()
    values = N.seed0_values(2000)
    counts = torch.tensor([float(v) - 1.0 for v in values], dtype=torch.float32).to(cuda)    # the kernel adds the 1
    state = torch.zeros((1,), dtype=torch.float32, device=cuda)
    trace = torch.full((len(values),), -7.0, device=cuda)
    base, tbase = counts.data_ptr(), trace.data_ptr()
    for i in range(len(values)):
        rc = lib.rn_loss_normalizer_ema(base + 4 * i, 1, 0.99, _C.ptr(state), tbase + 4 * i, st)
        assert rc == _C.RN_OK, i
    torch.cuda.synchronize()
    want = N.sequence(values, 0.99)
    got = trace.cpu().numpy()
    bad = np.nonzero(N.bits(got) != N.bits(want))[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert N.bits(state.cpu().numpy())[0] == N.bits(want[-1])[0]


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_kernel_refusals(cuda, build):
    """RN_EINVAL before any launch: n = 0, n = -1, each pointer NULL in turn; the sentinel in `state` (and in `normalizer`)
    stays"""
    from retinanet import _C
    lib, st = _lib(build), _C.current_stream()
    counts = torch.tensor([3.0, 4.0], device=cuda)
    state = torch.tensor([-123.25], device=cuda)
    norm = torch.tensor([-77.5], device=cuda)
    c, s, o = _C.ptr(counts), _C.ptr(state), _C.ptr(norm)
    for what, args in (("n = 0", (c, 0, 0.99, s, o)), ("n = -1", (c, -1, 0.99, s, o)),
                       ("NULL num_positives", (None, 2, 0.99, s, o)), ("NULL state", (c, 2, 0.99, None, o)),
                       ("NULL normalizer", (c, 2, 0.99, s, None))):
        assert lib.rn_loss_normalizer_ema(*args, st) == _C.RN_EINVAL, what
        assert b"rn_loss_normalizer_ema" in lib.rn_last_error(), what
    torch.cuda.synchronize()
    assert state.item() == -123.25 and norm.item() == -77.5
    assert lib.rn_loss_normalizer_ema(c, 2, 0.99, s, o, st) == _C.RN_OK      # the call the refusals are variations of
    torch.cuda.synchronize()
    assert N.bits(state.cpu().numpy())[0] == N.bits(N.ema_step(-123.25, 8.0, 0.99))[0] and norm.item() == state.item()


# ---- 3. RetinaNetLoss alone ----------------------------------------------------------------------------------------------------
def _small_pyramid(cuda):
    """the shapes of test_gpu_loss.py::test_loss_bf16_gradient_outputs_match_the_cast: K = 8, 3 anchors, levels 8x8 / 4x4 / 2x2"""
    K, na, B = 8, 3, 2
    sizes = [(8, 8), (4, 4), (2, 2)]
    g = torch.Generator().manual_seed(5)
    preds = {"class-predictions": {}, "box-predictions": {}}
    for i, (h, w) in enumerate(sizes):
        preds["class-predictions"][str(3 + i)] = (torch.randn((B, h, w, na * K), generator=g) * 2 - 2).to(cuda)
        preds["box-predictions"][str(3 + i)] = torch.randn((B, h, w, na * 4), generator=g).to(cuda)
    A = sum(h * w * na for h, w in sizes)
    cls_t = torch.randint(-2, K, (B, A), generator=g).float()
    box_t = torch.randn((B, A, 4), generator=g) * (cls_t >= 0).float()[..., None]
    flat = {"class-targets": cls_t.to(cuda), "box-targets": box_t.to(cuda)}
    return K, preds, flat


def test_retinanet_loss_follows_the_reference_sequence(cuda):
    """three calls (one with all-zero counts, one with the counts on the host): num-anchors-matched is the reference sequence
    bit for bit; losses and fp32 gradients are those of a RetinaNetLoss with the option off that is handed the reference
    value; a caller's normalizer= is ignored"""
    from retinanet.cfg import default_params
    from retinanet.losses import RetinaNetLoss
    K, preds, flat = _small_pyramid(cuda)
    p = default_params()
    p.loss.normalizer.use_moving_average = True
    on, off = RetinaNetLoss(K, p.loss), RetinaNetLoss(K, default_params().loss)
    npos = [torch.tensor([5.0, 3.0], device=cuda), torch.tensor([0.0, 0.0], device=cuda), torch.tensor([17.0, 0.0])]
    want = N.sequence([N.value(c.cpu().numpy()) for c in npos], 0.99)
    bogus = torch.tensor([4321.0], device=cuda)
    for i, c in enumerate(npos):
        targets = {"num-positives": c, "_flat": flat}
        got = on(targets, preds, normalizer=bogus if i != 1 else None)
        grads = on.grads
        ref = off(dict(targets, **{"num-positives": torch.zeros(2, device=cuda)}), preds,
                  normalizer=torch.from_numpy(want[i:i + 1].copy()).to(cuda))
        torch.cuda.synchronize()
        assert N.bits(got["num-anchors-matched"].cpu().numpy())[0] == N.bits(want[i])[0], i
        assert N.bits(on.moving_average_normalizer.cpu().numpy())[0] == N.bits(want[i])[0], i
        for k in ("box-loss", "class-loss", "weighted-loss", "num-anchors-matched"):
            assert N.bits(got[k].cpu().numpy())[0] == N.bits(ref[k].cpu().numpy())[0], (i, k)
        assert got["iou-prediction-loss"] == ref["iou-prediction-loss"] == 0.0
        for key in ("class-predictions", "box-predictions"):
            for lv in preds[key]:
                assert torch.equal(grads[key][lv], off.grads[key][lv]), (i, key, lv)
                assert float(grads[key][lv].abs().max()) > 0
    assert on.moving_average_normalizer.device == flat["class-targets"].device
    assert bogus.item() == 4321.0 and off.moving_average_normalizer is None


# ---- 4. engine ------------------------------------------------------------------------------------------------------------------
def _engine(cuda, moving_average=True, seed=5, size=128, B=2):
    """test_gpu_frozen_bn.py::_resnet_engine with the default freeze list and the option"""
    from test_gpu_frozen_bn import _randomize
    from retinanet.cfg import default_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    p = default_params(input_size=size)
    p.architecture.batch_norm.use_sync = False
    p.loss.normalizer.use_moving_average = moving_average
    builder = ModelBuilder(p, "train", device=cuda, seed=seed)
    model = builder()
    _randomize(model, seed, cuda)
    rx = [builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables]
    eng = TrainEngine(model, B, frozen_regexes=rx, world_size=1)
    model.optimizer.lr = lambda step: 0.01
    return p, model, eng


def _batches(p, cuda, seeds, size=128, B=2):
    from test_gpu_frozen_bn import _batch
    return [_batch(p, cuda, size, B, s) for s in seeds]


def _f32_bits(t):
    return int(N.bits(t.detach().cpu().numpy())[0])


def test_engine_trains_with_the_moving_average_normalizer(cuda):
    """ResNet-50 at 128 x 128, B = 2 (before this feature: NotImplementedError from the model builder): three steps on
    batches with different positive counts; num-anchors-matched * B is the reference sequence bit for bit, nothing rode
    in a SyncBN message, the losses are finite"""
    B = 2
    p, model, eng = _engine(cuda)
    assert model.loss.use_moving_average_normalizer and model.loss.normalizer_momentum == 0.99
    batches = _batches(p, cuda, (5, 6, 7))
    values = [N.value(t["num-positives"].cpu().numpy()) for _, t in batches]
    assert len(set(float(v) for v in values)) == 3, values
    want = N.sequence(values, 0.99)
    for i, (images, targets) in enumerate(batches):
        out = eng.train_step(images, targets)
        torch.cuda.synchronize()
        assert _f32_bits(out["num-anchors-matched"] * B) == int(N.bits(want[i])[0]), (i, out["num-anchors-matched"], want[i])
        assert eng.small.c2_normalizer is None and eng.small._c2_local is None
        for k in ("weighted-loss", "class-loss", "box-loss", "total-loss", "gradient-norm"):
            assert np.isfinite(float(out[k].item())), (i, k)
    assert bool(torch.isfinite(eng.P).all()) and eng.syncbn_messages_per_step == 0
    assert _f32_bits(model.loss.moving_average_normalizer) == int(N.bits(want[-1])[0])


# ---- 5. resume ------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_keeps_the_moving_average(cuda, tmp_path):
    """save after step 1, restore into a fresh engine (loss state 0.0), step again: bit-equal to the uninterrupted run.  A
    checkpoint written with the option off has no `loss/moving_average_normalizer` and leaves the state at 0.0; an engine with
    the option off ignores the key."""
    p, model, eng = _engine(cuda, seed=7)
    (im1, t1), (im2, t2) = _batches(p, cuda, (7, 8))
    eng.train_step(im1, t1)
    prefix = str(tmp_path / "weights_step_1")
    eng.save_checkpoint(prefix)
    saved = _f32_bits(model.loss.moving_average_normalizer)
    assert saved == int(N.bits(N.ema_step(0.0, N.value(t1["num-positives"].cpu().numpy()), 0.99))[0])
    want = eng.train_step(im2, t2)
    torch.cuda.synchronize()
    # the option off: no such extra in a fresh save
    p3, model3, eng3 = _engine(cuda, moving_average=False, seed=7)
    eng3.train_step(im1, t1)
    prefix_off = str(tmp_path / "weights_off_step_1")
    eng3.save_checkpoint(prefix_off)
    eng3.restore_checkpoint(prefix_off)
    assert KEY not in model3.loaded_extras
    eng3.restore_checkpoint(prefix)                     # a file with the key, the option off: ignored
    assert KEY in model3.loaded_extras and model3.loss.moving_average_normalizer is None
    assert np.isfinite(float(eng3.train_step(im2, t2)["weighted-loss"].item()))
    del eng3, model3
    # a fresh engine with the option on
    p2, model2, eng2 = _engine(cuda, seed=7)
    eng2.restore_checkpoint(prefix_off)                 # a file without the key: the state stays at the initial 0.0
    state = model2.loss.moving_average_normalizer
    assert KEY not in model2.loaded_extras and (state is None or float(state.item()) == 0.0)
    eng2.restore_checkpoint(prefix)
    assert int(N.bits(np.asarray(model2.loaded_extras[KEY]))[0]) == saved      # a float32 scalar in the file
    assert _f32_bits(model2.loss.moving_average_normalizer) == saved and eng2.step_count == 1
    got = eng2.train_step(im2, t2)
    torch.cuda.synchronize()
    for k in ("weighted-loss", "num-anchors-matched"):
        assert _f32_bits(got[k]) == _f32_bits(want[k]), (k, got[k], want[k])
    assert torch.equal(eng2.P, eng.P) and torch.equal(eng2.V, eng.V) and torch.equal(eng2.E, eng.E)


# ---- the Executor: the configuration file is all a user changes -----------------------------------------------------------------
def test_executor_trains_and_resumes_with_the_option(cuda, tmp_path):
    """test_gpu_executor_optim.py's pattern: three steps through Executor.run, the final checkpoint holds the engine's average,
    and a second Executor resumes from it"""
    import copy
    from test_gpu_executor import _dataset, _params
    from test_gpu_executor_optim import _executor
    from retinanet import tf_checkpoint
    p = _params(tmp_path, _dataset(tmp_path))
    p.experiment.run_mode = "train"
    p.loss.normalizer.use_moving_average = True
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        ex = _executor(p, cuda)
        eng = ex._engine
        w0 = eng.P.clone()
        ex.run()
        assert eng.step_count == 3 and not torch.equal(w0, eng.P) and bool(torch.isfinite(eng.P).all())
        state = eng.model.loss.moving_average_normalizer
        # three updates from 0 with momentum 0.99 and v >= 1: at least 1 - 0.99^3 (less three roundings), far below v
        assert 0.0297 <= float(state.item()) < 1e4
        prefix = tf_checkpoint.latest_checkpoint(os.path.join(p.experiment.model_dir, p.experiment.name))
        arrays, _ = tf_checkpoint.load_weights(prefix)
        assert arrays[KEY].dtype == np.float32 and int(N.bits(arrays[KEY])[0]) == _f32_bits(state)
        p2 = copy.deepcopy(p)
        p2.training.train_steps = 4
        ex2 = _executor(p2, cuda)
        assert ex2._engine.step_count == 3
        assert _f32_bits(ex2._engine.model.loss.moving_average_normalizer) == _f32_bits(state)
        ex2.run()
        assert ex2._engine.step_count == 4 and bool(torch.isfinite(ex2._engine.P).all())
        assert float(ex2._engine.model.loss.moving_average_normalizer.item()) != float(state.item())
    finally:
        os.chdir(cwd)


# ---- 6. two ranks on one device (gloo), modelled on test_gpu_frozen_bn.py::test_two_ranks_with_frozen_batchnorm ----------------
SIZE, B2, SEED = 128, 4, 21


def _dp_build(world, rank, moving_average):
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import synth_gt
    from test_gpu_frozen_bn import _randomize
    from retinanet.cfg import default_params
    from retinanet.dataloader import LabelEncoder
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    dev = torch.device("cuda:0")
    p = default_params(input_size=SIZE, batch_train=B2)
    assert p.architecture.batch_norm.use_sync
    p.architecture.backbone.depth = 14
    p.training.optimizer.clipnorm = 1e9
    p.loss.normalizer.use_moving_average = moving_average
    builder = ModelBuilder(p, "train", device=dev, seed=SEED)
    model = builder()
    _randomize(model, SEED, dev)
    per = B2 // world
    rx = [builder.FREEZE_VARS_REGEX[n] for n in p.training.freeze_variables]
    eng = TrainEngine(model, per, frozen_regexes=rx, world_size=world)
    enc = LabelEncoder(p, device=dev)
    rng = np.random.default_rng(SEED)
    gts = [synth_gt(rng, int(rng.integers(2, 6)), SIZE) for _ in range(B2)]
    images = torch.randn((B2, SIZE, SIZE, 3), generator=torch.Generator().manual_seed(SEED))
    sl = slice(rank * per, (rank + 1) * per)
    gts = gts[sl]
    Gmax = max(x[0].shape[0] for x in gts)
    gb, gc, cnt = np.zeros([per, Gmax, 4], np.float32), np.zeros([per, Gmax], np.float32), np.zeros([per], np.int32)
    for i, (b, c) in enumerate(gts):
        gb[i, :len(b)], gc[i, :len(c)], cnt[i] = b, c, len(b)
    targets = enc.encode_batch(torch.from_numpy(gb), torch.from_numpy(gc), torch.from_numpy(cnt))
    return model, eng, images[sl].to(dev), targets, per


def _dp_step(world, rank, moving_average):
    model, eng, images, targets, per = _dp_build(world, rank, moving_average)
    model.optimizer.lr = lambda step: 0.01
    w0 = eng.P.cpu().numpy().copy()
    out = eng.train_step(images, targets)
    torch.cuda.synchronize()
    r = {"P": eng.P.cpu().numpy(), "moved": not np.array_equal(eng.P.cpu().numpy(), w0),
         "loss": float(out["weighted-loss"].item()), "messages": eng.syncbn_messages_per_step, "sync_bn": bool(eng.sync_bn),
         "rode": eng.small.c2_normalizer is not None, "pending": eng.small._c2_local is not None,
         "npos": float(targets["num-positives"].sum().item()),
         "matched_bits": int(N.bits((out["num-anchors-matched"] * per).cpu().numpy())[0])}
    del model, eng
    torch.cuda.empty_cache()
    return r


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out[rank] = {name: _dp_step(world, rank, on) for name, on in (("on", True), ("off", False))}
    dist.destroy_process_group()


def test_two_ranks_keep_replica_local_normalizers(cuda):
    """use_sync = True over two ranks: each rank's num-anchors-matched * B is ema_step(0, OWN count + 1, 0.99) — no sum over
    the ranks, no division by their number (retinanet_loss.py:40-44: the all-reduce is the other branch) —, nothing rides in
    the SyncBN messages and none is added or dropped, and the gradients are still summed: both ranks end on the same
    weights."""
    import torch.multiprocessing as mp
    from test_gpu_frozen_bn import _free_port
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=False)   # two children, no more
    deadline = time.monotonic() + 240.0
    try:
        while not ctx.join(timeout=5.0):          # raises on the first non-zero exit, after ending the other child
            assert time.monotonic() < deadline, "a rank did not finish"
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.kill()
    r0, r1 = out[0], out[1]
    a, b = r0["on"], r1["on"]
    assert a["sync_bn"] and b["sync_bn"]
    for r in (a, b):
        assert r["matched_bits"] == int(N.bits(N.ema_step(0.0, np.float32(r["npos"] + 1.0), 0.99))[0]), r["npos"]
        assert not r["rode"] and not r["pending"] and np.isfinite(r["loss"]) and r["moved"]
    assert a["npos"] != b["npos"]                 # or the check above could not tell a local count from the mean
    assert a["messages"] == b["messages"] == r0["off"]["messages"] == r1["off"]["messages"] > 0
    assert r0["off"]["rode"] and r1["off"]["rode"] and not r0["off"]["pending"]
    np.testing.assert_array_equal(a["P"], b["P"])
