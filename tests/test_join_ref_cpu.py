"""tests/join_ref.py is itself right, and the comparison of test_gpu_gradient_joins.py has teeth — no GPU needed.

A fake engine state (ops, tensors, t, raw, grad, bal_out, dy_of, joins.writers — the attributes join_ref.py reads) is filled
from ONE whole-graph float64 autograd run without rounding over a small graph that holds every kind of join:
two bottleneck blocks (the first with a projection shortcut, one BatchNorm frozen under its trainable conv), an MBConv block
(expand, depthwise, squeeze-excite, projection with drop_connect and a skip), a lateral conv and two max-pools feeding a
three-level top-down with an out-conv per level, BalanceFeatures, and two shared prediction convs per level.  The forward
run composes join_ref's local functions; what the test checks is everything else: that the per-writer contributions,
each computed from stored boundary tensors alone, sum to the whole-graph gradient of every key (1e-12), i.e. the label
mapping, the teacher forcing and what each buffer holds.  The writers come from train_engine.GradientJoins, driven in the
planners' order with the planners' labels.

Keys that cannot be rebuilt from stored tensors: none (cap: 2 per engine).  The restatement alone is checked against it."""
import types

import pytest
import torch

import join_ref as J
from fake_graph import _graph, _local_ops
from join_counts import check_joins

F64 = torch.float64
UNCHECKED_CAP = 2


def _plan_joins(eng):
    """The planners' calls of GradientJoins, in their order and with their labels (train_engine._build_backward)"""
    from retinanet.model.train_engine import GradientJoins
    joins = GradientJoins(eng.grad, eng.bal_src)
    plan, done = [], set()
    for op in eng.ops:
        if op["op"] in ("conv", "dwconv"):
            grp = op.get("group")
            if grp is None:
                plan.append([op])
            elif (op["op"], grp) not in done:
                done.add((op["op"], grp))
                plan.append([o for o in eng.ops if o["op"] == op["op"] and o.get("group") == grp])
        else:
            plan.append(op)
    for item in reversed(plan):
        if isinstance(item, list):
            for op in item:
                if op.get("residual"):
                    joins.add(op["residual"], "bn:" + item[0]["out"], balanced=False)
            launches = []
            for op in item:
                for sub in launches:
                    if all(o["inp"] != op["inp"] for o in sub):
                        sub.append(op)
                        break
                else:
                    launches.append([op])
            for sub in launches:
                name = ("dgrad:" + (sub[0].get("group") or sub[0]["out"]) if sub[0]["op"] == "conv"
                        else "dw_dgrad:" + "+".join(o["out"] for o in sub))
                for op in sub:
                    joins.add(op["inp"], name)
        elif item["op"] == "se":
            joins.sole(item["inp"], "se:" + item["out"])
        elif item["op"] == "maxpool":
            joins.add(item["inp"], "maxpool:" + item["out"], balanced=False)
        elif item["op"] == "topdown":
            for i, o in zip(item["ins"], item["outs"]):
                if i != o:
                    joins.sole(i, "topdown")
                else:
                    assert joins.add(i, "topdown", balanced=False)[1]
        elif item["op"] == "balance":
            for n in item["tensors"]:
                joins.sole(n, "balance")
    return joins


def _fake_engine(seed=0):
    """-> (engine stand-in, {key: whole-graph autograd gradient})"""
    g = _graph()
    gen = torch.Generator().manual_seed(seed)
    B = 2
    variables = {}
    for name, spec in g.var_specs.items():
        shape = spec["shape"]
        if name.endswith(("/gamma", "/moving_variance")):
            v = torch.rand(shape, generator=gen, dtype=F64) + 0.5
        elif name.endswith(("/beta", "/moving_mean", "/bias")):
            v = torch.randn(shape, generator=gen, dtype=F64) * 0.1
        else:
            v = torch.randn(shape, generator=gen, dtype=F64) / (shape[0] * shape[1] * shape[2]) ** 0.5
        variables[name] = v
    tensors, ops = _local_ops(g)
    eng = types.SimpleNamespace(
        g=g, ops=ops, tensors=tensors, t={}, raw={}, grad={}, bal_out={}, bal_src={}, dy_of={}, h16=None, eps=1e-3,
        model=types.SimpleNamespace(variables=variables), requires={n: True for n in tensors},
        dc_masks={"m_proj": (torch.tensor([1.0 / 0.9, 0.0], dtype=F64), 0.9)},
        _bn_trainable=lambda op: bool(op.get("bn")) and op["bn"] != "b_b_bn",
        _bn_frozen=lambda op: op.get("bn") == "b_b_bn")
    live = {"x0": torch.randn((B, 16, 16, 8), generator=gen, dtype=F64).requires_grad_(True)}
    live_bal = {}
    src = lambda n: live_bal.get(n, live[n])
    for op in ops:
        kind = op["op"]
        if kind in ("conv", "dwconv"):
            y, out = J.layer(eng, op, src(op["inp"]), live[op["residual"]] if op.get("residual") else None)
            if op.get("bn"):
                eng.raw[op["out"]] = y.detach()
            live[op["out"]] = out
        elif kind == "se":
            live[op["out"]] = J.squeeze_excite(eng, op, live[op["inp"]])
        elif kind == "maxpool":
            live[op["out"]] = J.maxpool(eng, op, live[op["inp"]])
        elif kind == "topdown":
            # the gradient buffer of outs[j] holds what the READERS of the tensor put there; what the level below sends
            # up stays inside the top-down kernels — so the readers get a copy whose gradient is exactly that
            L = len(op["ins"])
            inner = {op["outs"][L - 1]: live[op["outs"][L - 1]]}
            for j in range(L - 2, -1, -1):
                inner[op["outs"][j]] = J.topdown_level(eng, op, j, live[op["ins"][j]], inner[op["outs"][j + 1]])
                live[op["outs"][j]] = inner[op["outs"][j]] + 0.0
        elif kind == "balance":
            for n, o in zip(op["tensors"], J.balance(eng, op, [live[n] for n in op["tensors"]])):
                live_bal[n] = o
                eng.bal_src[n] = None
    for t in list(live.values()) + list(live_bal.values()):
        t.retain_grad()
    heads = [o["out"] for o in ops if o.get("out_dtype") == "f32"]
    up = {n: torch.randn(live[n].shape, generator=gen, dtype=F64) for n in heads}
    sum((live[n] * up[n]).sum() for n in heads).backward()
    eng.t = {n: t.detach() for n, t in live.items()}
    eng.bal_out = {n: t.detach() for n, t in live_bal.items()}
    eng.dy_of = up
    eng.grad = {n: t.grad for n, t in live.items() if n not in heads}
    eng.grad.update({"bal:" + n: t.grad for n, t in live_bal.items()})
    eng.joins = _plan_joins(eng)
    return eng, dict(eng.grad)


@pytest.fixture(scope="module")
def fake():
    eng, true = _fake_engine()
    cache = {}
    want = {key: J.expected(eng, key, cache=cache) for key in eng.joins.writers}
    parts = {key: J.writer_parts(eng, key, cache=cache) for key in eng.joins.writers}
    return eng, true, want, parts


def test_fake_graph_holds_every_kind_of_join(fake):
    eng, true, want, parts = fake
    check_joins(eng)
    writers = eng.joins.writers
    # every gradient buffer that a step writes is a key, and every key is restated: the unchecked share is 0
    assert set(writers) == set(eng.grad)
    assert len(set(writers) - set(want)) == 0 <= UNCHECKED_CAP
    kinds = {J.join_kind(eng, k) for k in writers}
    assert {"bn+dgrad+dgrad", "bn+dgrad", "dgrad", "bn", "dw_dgrad", "se", "maxpool", "maxpool+topdown", "dgrad+topdown", "topdown",
            "balance", "dgrad+dgrad"} <= kinds, kinds
    assert writers["bal:p_out0"] == ["dgrad:pred", "dgrad:pred"]
    assert writers["p_in2"] == ["dgrad:fpn_out", "topdown"] and writers["p_in1"] == ["topdown", "maxpool:p_in2"]


def test_restatement_equals_whole_graph_autograd(fake):
    eng, true, want, parts = fake
    for key in eng.joins.writers:
        err = ((want[key] - true[key]).norm() / true[key].norm()).item()
        assert true[key].norm() > 0 and err < 1e-12, (key, err)
        assert len(parts[key]) == len(eng.joins.writers[key])
        assert ((sum(parts[key]) - true[key]).norm() / true[key].norm()).item() < 1e-12, key


def test_unknown_label_raises(fake):
    eng = fake[0]
    with pytest.raises(KeyError):
        J.contribution(eng, "a_out", "scatter:a_out")
    with pytest.raises(KeyError):      # a label that stands once more than the ops it matches
        J.contribution(eng, "bal:p_out0", "dgrad:pred", count=3)


def _rejected(got, want):
    return not J.accept(J.figures(got, want), want.numel())


def test_comparison_accepts_the_truth_and_rejects_every_mutation(fake):
    """The thresholds of test_gpu_gradient_joins.py (join_ref.LIMITS) on the bugs the test exists for.  `got` is the
    mutated sum rounded to bfloat16, as an engine would store it."""
    eng, true, want, parts = fake
    bf = lambda t: t.to(torch.bfloat16)
    seen = {m: 0 for m in ("dropped", "doubled", "gate", "stale", "store")}
    for key, ps in parts.items():
        assert not _rejected(bf(true[key]), want[key]), key
        assert _rejected(bf(want[key] + 1024.0), want[key]), ("a first writer added onto a stale 1024.0", key)
        seen["stale"] += 1
        if len(ps) < 2:
            continue
        for i, p in enumerate(ps):
            assert _rejected(bf(want[key] - p), want[key]), ("contribution dropped", key, eng.joins.writers[key][i])
            assert _rejected(bf(want[key] + p), want[key]), ("contribution doubled", key, eng.joins.writers[key][i])
            seen["dropped"] += 1
            seen["doubled"] += 1
        assert _rejected(bf(ps[-1]), want[key]), ("the last writer stored where it should add", key)
        seen["store"] += 1
    # the skip gradient taken in front of the activation gate of the block's output: dz itself instead of dz * act'
    for op in eng.ops:
        if op.get("residual") and op.get("act") == "relu":
            key = op["residual"]
            gated = J.contribution(eng, key, "bn:" + op["out"])
            mutated = want[key] - gated + eng.grad[op["out"]]
            assert _rejected(bf(mutated), want[key]), ("skip gradient taken before the gate", key)
            seen["gate"] += 1
    joined = [w for w in eng.joins.writers.values() if len(w) > 1]
    assert seen["gate"] == 2 and seen["store"] == len(joined) == 8 and seen["dropped"] == sum(map(len, joined)) == 17, seen


def test_small_tensors_are_judged_by_counts():
    """fewer than 1000 elements: the 2 % / 0.5 % fractions become counts that are never below 2"""
    assert J.accept((1.0, 2 / 64, 2 / 64), 64) and not J.accept((1.0, 3 / 64, 0.0), 64)
    assert J.accept((1.0, 19 / 999, 4 / 999), 999) and not J.accept((1.0, 20 / 999, 0.0), 999)
    assert not J.accept((1.0, 0.0, 5 / 999), 999)
    assert J.accept((1.0, 0.019, 0.004), 1000) and not J.accept((1.0, 0.02, 0.0), 1000)
    assert not J.accept((0.9999, 0.0, 0.0), 10 ** 6) and not J.accept((float("nan"), 0.0, 0.0), 10 ** 6)
