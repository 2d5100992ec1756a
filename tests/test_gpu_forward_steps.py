"""Every forward step of both engines against float64, teacher-forced (tests/forward_ref.py).

The per-launch tests check the kernels; this file checks what the engines point them at — which tensor, weight pack, folded
scale / shift, residual and BatchNorm state every launch of the forward pass reads and writes.  Every stored tensor is
compared with the float64 value of the ONE op that writes it, computed from the inputs the engine itself stored, so the
bound is a few ulp of the storage type (join_ref.LIMITS), not a noise floor that grows with depth.

TrainEngine (every id of engine_cases.ENGINES): all of eng.t / eng.raw / eng.bal_out filled with NaN, one forward pass;
  * the buffers still entirely NaN are exactly those the plan never writes (the stem output under a fused stem + pool);
  * every other stored tensor, and the moving statistics of every live BatchNorm, are compared: the uncompared share is 0;
  * a second pass from the same BatchNorm state leaves every buffer and statistic bit-identical.
InferenceEngine (engine_cases.INFER_ENGINES):
  * a normal pass from NaN-filled buffers: every tensor with one writer is compared on the final buffers;
  * run_stepwise: every step alone, with every buffer it does not declare as read (step_io) filled with NaN — each written
    tensor against the restatement on the pre-step reads (the in-place squeeze-excite and BalanceFeatures steps too), the
    changed buffers exactly the declared writes; the chain it leaves is bit-identical to the normal pass, so the two-stream
    schedule (batch 4) and the one-stream one agree on every intermediate tensor.
test_the_engines_reach_every_launch_form asserts, from the engines' own plans, that the lists hold every launch form named
there.  One report line per engine (pytest -s).  Graph capture is left to its replay-equals-eager tests."""
import ctypes

import pytest
import torch

import forward_ref as FR
from engine_cases import ENGINES, INFER_ENGINES, _engine, _infer_engine

pytestmark = pytest.mark.gpu

_BUILT = {}     # (kind, id) -> what the builder returned: the coverage test and the cases share the engines


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    _BUILT.clear()


def _train(cuda, name):
    if ("train", name) not in _BUILT:
        model, size, B, kw = ENGINES[name]
        eng, images = _engine(cuda, model, size, B, **kw)
        # _engine leaves the conv biases at 0 and the moving statistics at 0 / 1, where a bias counted twice in a folded
        # shift, or a moving mean blended by the wrong momentum, moves little or nothing: randomise them as
        # test_gpu_model._randomize does and reload (the path restore_checkpoint takes)
        g, v = torch.Generator().manual_seed(17), eng.model.variables
        for k, t in v.items():
            if (k.endswith("/bias") and "prediction" not in k) or k.endswith("/moving_mean"):
                t.copy_((torch.randn(t.shape, generator=g) * (0.05 if k.endswith("/bias") else 0.1)).to(t.device))
            elif k.endswith("/moving_variance"):
                t.copy_((torch.rand(t.shape, generator=g) * 0.5 + 0.75).to(t.device))
        with torch.cuda.device(cuda):
            eng.load_from_model()
            for bn, st in eng.bn_state.items():
                st["mm"].copy_(v[bn + "/moving_mean"])
                st["mv"].copy_(v[bn + "/moving_variance"])
        _BUILT["train", name] = (eng, images)
    return _BUILT["train", name]


def _infer(cuda, name):
    if ("infer", name) not in _BUILT:
        model, size, B, kw = INFER_ENGINES[name]
        _BUILT["infer", name] = _infer_engine(cuda, model, size, B, **kw)
    return _BUILT["infer", name]


def _poison(tables, keep=("images",)):
    for table in tables:
        for k, v in table.items():
            if k not in keep:
                v.fill_(float("nan"))


def _snapshot(tables):
    return [{k: v.clone() for k, v in table.items()} for table in tables]


def _all_nan(table):
    return {k for k, v in table.items() if bool(torch.isnan(v).all())}


def _stored_keys(eng, skip):
    return ({k for k in eng.t if k not in skip} | {"raw:" + k for k in eng.raw} | {"bal:" + k for k in eng.bal_out})


def _assert_teeth(name, eng):
    """TEETH, on the engine's own numbers (forward_ref.wiring_teeth): its buffers must be rejected against restatements that
    carry one wiring error each — the errors of test_forward_ref_cpu.py, on real tensors"""
    teeth = FR.wiring_teeth(eng)
    assert len(teeth) >= 6, teeth
    loose = [(what, key) for what, key, rejected in teeth if not rejected]
    assert not loose, f"{name}: would pass with {loose}"


@pytest.mark.parametrize("name", list(ENGINES))
def test_train_forward_matches_float64(cuda, name):
    eng, images = _train(cuda, name)
    tables = (eng.t, eng.raw, eng.bal_out)
    stats = lambda: {bn: {k: v.clone() for k, v in st.items()} for bn, st in eng.bn_state.items()}
    with torch.cuda.device(cuda):
        before = stats()
        eng.t["images"].copy_(images)
        _poison(tables)
        eng.forward(eng.t["images"], draw=False)
        torch.cuda.synchronize()
        first, first_stats = _snapshot(tables), stats()
        for bn, st in before.items():       # the second pass starts from the same moving statistics, the buffers as they are
            for k, v in st.items():
                eng.bn_state[bn][k].copy_(v)
        eng.forward(eng.t["images"], draw=False)
        torch.cuda.synchronize()
    moved = [k for a, b in zip(first, tables) for k in a if not FR._same_bits(a[k], b[k])]
    moved += [bn + "/" + k for bn, st in first_stats.items() for k in st if not FR._same_bits(st[k], eng.bn_state[bn][k])]
    assert not moved, f"{name}: the second forward pass left other bits in {moved[:8]} ({len(moved)} buffers)"
    # never written: what the writers leave out, and what the plan says — the stem output under a fused stem + pool
    stem = next(o["out"] for o in eng.ops if o["op"] == "stem")
    unwritten = _all_nan(eng.t) | {"raw:" + k for k in _all_nan(eng.raw)} | {"bal:" + k for k in _all_nan(eng.bal_out)}
    assert unwritten == FR.never_written(eng) == ({stem} if eng.fused_pools else set()), (unwritten, FR.never_written(eng))
    rows = FR.check_state(eng, before)
    print(FR.report_line("TrainEngine " + name, rows))
    # coverage: every stored tensor and every live BatchNorm state is compared (inner tensors of a fused block have no buffer
    # and count through the block's output)
    compared = {r[0] for r in rows}
    live = {o["bn"] for o in FR.live_bn_ops(eng)}
    assert live == set(eng.bn_state)
    missing = (_stored_keys(eng, {"images"} | unwritten) | {t + bn for bn in live for t in ("mm:", "mv:")}) - compared
    assert len(missing) == 0, sorted(missing)
    if name == "resnet26-frozen-initial":
        assert eng.fused_pools and eng.bneck
    if name == "resnet26-f16":
        assert eng.h16 == torch.float16
    _assert_teeth(name, eng)
    bad = FR.failures(rows)
    assert not bad, f"{name}: {len(bad)} of {len(rows)} stored tensors / statistics miss their bound: {bad[:12]}"


@pytest.mark.parametrize("name", list(INFER_ENGINES))
def test_inference_steps_match_float64(cuda, name):
    from retinanet import _C
    eng, variables, images = _infer(cuda, name)
    view = FR.inference_view(eng, variables)
    table = FR.writers(view)
    with torch.cuda.device(cuda):
        _poison((eng.t,))
        eng(images.to(cuda))
        torch.cuda.synchronize()
        normal = _snapshot((eng.t,))[0]
        stem = next(o["out"] for o in view.ops if o["op"] == "stem")
        assert _all_nan(eng.t) == FR.never_written(view) == ({stem} if view.fused_pools else set())
        final_rows = FR.check_state(view)
        _poison((eng.t,))
        rows, covered = [], set()
        FR.run_stepwise(eng, FR.step_checker(view, rows, covered), _C.current_stream())
        torch.cuda.synchronize()
    apart = [k for k, v in normal.items() if not FR._same_bits(v, eng.t[k])]
    assert not apart, f"{name}: the stepwise chain and the normal pass ({len(eng.side_steps)} side launches) differ in {apart[:8]}"
    print(FR.report_line("InferenceEngine " + name + " (stepwise)", rows))
    print(FR.report_line("InferenceEngine " + name + " (final buffers)", final_rows))
    # coverage: every writer of every stored tensor was judged on its own step; the final buffers add nothing new
    every = {(k, i) for k, ws in table.items() for i in range(len(ws))}
    assert len(every - covered) == 0 and covered <= every, sorted(every ^ covered)
    assert set(table) == set(eng.t) - {"images"} - FR.never_written(view)
    assert {r[0] for r in final_rows} == {k for k, ws in table.items() if len(ws) == 1}
    if name == "resnet26-f16":
        assert eng.h16 == torch.float16
    if name == "resnet26-batch4":
        assert eng.two_streams and eng.side_steps
    _assert_teeth(name, view)
    bad = FR.failures(rows) + FR.failures(final_rows)
    assert not bad, f"{name}: {len(bad)} of {len(rows) + len(final_rows)} comparisons miss their bound: {bad[:12]}"


def _forms(cuda):
    """launch form -> the engines (of both lists) whose plan holds it"""
    seen = {}
    mark = lambda form, who: seen.setdefault(form, []).append(who) if who not in seen.get(form, []) else None
    for name in INFER_ENGINES:
        eng = _infer(cuda, name)[0]
        who = "infer:" + name
        steps = [n for _, n in eng.steps]
        for n, p in eng.conv_problems.items():
            if eng.lib.rn_conv_splitk_workspace_bytes(ctypes.byref(p)) > 0:
                mark("split-K conv launch", who)
            if p.num_segments > 1:
                mark("multi-segment conv launch", who)
            if any(p.seg[i].w_pair or p.seg[i].w_terms > 1 for i in range(p.num_segments)):
                mark("w_pair / w_terms > 1 prediction conv", who)
        if eng.side_steps:
            mark("side-stream launch", who)
        if any(n.endswith(":rest") for n in steps):
            mark("second launch of split_by_depth", who)
        if any(n.startswith("bneck:") for n in steps):
            mark("fused bneck block", who)
        if set(eng.step_io["conv:stem"][1]) != {next(o["out"] for o in eng.g.ops if o["op"] == "stem")}:
            mark("fused stem + pool", who)
        if any(p.num_segments > 1 for _, p in eng.dw_launches):
            mark("multi-segment depthwise launch", who)
        if any(n.startswith("se:") for n in steps):
            mark("in-place squeeze-excite step", who)
        if "balance_features" in steps:
            mark("in-place balance step", who)
    for name in ENGINES:
        eng = _train(cuda, name)[0]
        who = "train:" + name
        for n, p in eng.conv_launches:
            if not n.startswith("fwd:"):
                continue
            if eng.lib.rn_conv_splitk_workspace_bytes(ctypes.byref(p)) > 0:
                mark("split-K conv launch", who)
            if p.num_segments > 1:
                mark("multi-segment conv launch", who)
            if any(p.seg[i].w_pair or p.seg[i].w_terms > 1 for i in range(p.num_segments)):
                mark("w_pair / w_terms > 1 prediction conv", who)
            if any(p.seg[i].bn_partial for i in range(p.num_segments)):
                mark("training conv with the fused-statistics epilogue", who)
            if n.endswith(":rest"):
                mark("second launch of split_by_depth", who)
        if eng.bneck:
            mark("fused bneck block", who)
        if eng.fused_pools:
            mark("fused stem + pool", who)
        if any(kind == "fwd" and p.num_segments > 1 for _, kind, p, _ in eng.dw_launches):
            mark("multi-segment depthwise launch", who)
    return seen


FORMS = ["split-K conv launch", "side-stream launch", "second launch of split_by_depth", "fused bneck block",
         "fused stem + pool", "multi-segment conv launch", "multi-segment depthwise launch",
         "w_pair / w_terms > 1 prediction conv", "in-place squeeze-excite step", "in-place balance step",
         "training conv with the fused-statistics epilogue"]


def test_the_engines_reach_every_launch_form(cuda):
    """read from the engines' own plans: each launch form occurs in at least one engine of the two lists"""
    seen = _forms(cuda)
    for form in FORMS:
        print(f"{form}: {len(seen.get(form, []))} engines, e.g. {seen.get(form, ['-'])[0]}")
    missing = [f for f in FORMS if not seen.get(f)]
    assert not missing, missing
