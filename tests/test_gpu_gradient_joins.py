"""Every gradient join's ARITHMETIC against float64, from the engine's own buffers (tests/join_ref.py).

tests/join_counts.py checks the plan (who writes which buffer, how often); this file runs the kernels.  For every key of
engine.joins.writers, eng.grad[key] after forward + backward is compared with the sum of its labelled writers' contributions,
each restated in float64 (torch autograd on a local function of one op) from the engine's boundary tensors — teacher-forced,
so no rounding noise accumulates across layers and the tolerance is a few ulp (join_ref.LIMITS, the numbers of
test_bottleneck_tail_forward_backward_tight), not a cosine floor.

Per engine:
  * check_joins(eng) first;
  * POISON: every eng.grad[*] buffer is filled with 1024.0 (exact in bf16 and f16) before backward — a first writer that
    accumulates, or a kernel that reads its destination when told to store, fails on this first step;
  * REPEAT: backward runs a second time on the same inputs with the buffers left as they are; every buffer must be
    bit-identical to the first run;
  * TEETH: for every join with two or more writers, the buffer is also compared with the restatement minus / plus each
    single writer's contribution, and must be rejected (the mutations of test_join_ref_cpu.py, on real numbers);
  * every key of joins.writers is compared: the share of unchecked keys is 0 (cap for keys that cannot be rebuilt from stored
    tensors: 2 per engine; none is used);
  * one report line: keys, keys with >= 2 writers, the worst cosine and outlier fractions with their keys.

What the check cannot see: an error INSIDE one op that its restatement shares or that the per-launch tests own (the conv,
BatchNorm, depthwise, squeeze-excite kernels' own arithmetic is judged here only through the gradient they hand to a join)."""
import ctypes

import pytest
import torch

import join_ref as J
from engine_cases import ENGINES, _engine
from join_counts import check_joins

pytestmark = pytest.mark.gpu

UNCHECKED_CAP = 2


def _bits(t):
    return t.contiguous().view(torch.int16)


def run_engine(cuda, name, floor=False):
    """Build engine `name`, run forward, poisoned backward and the repeat; -> (engine, rows) with one row per key of
    joins.writers: (key, join kind, elements, figures of the engine, accepted[, figures of the float32 restatement against
    the float64 one — the floor of this comparison, for tools that measure it])."""
    model, size, B, kw = ENGINES[name]
    eng, images = _engine(cuda, model, size, B, **kw)
    check_joins(eng)
    with torch.cuda.device(cuda):
        preds = eng.forward(images.to(cuda), draw=False)
        g = torch.Generator().manual_seed(99)
        up = {k: {lv: torch.randn(preds[k][lv].shape, generator=g).to(cuda) for lv in preds[k]} for k in preds}
        for buf in eng.grad.values():
            buf.fill_(1024.0)
        eng.backward(up)
        torch.cuda.synchronize()
        first = {k: v.clone() for k, v in eng.grad.items()}
        eng.backward(up)
        torch.cuda.synchronize()
    moved = [k for k in eng.joins.writers if not torch.equal(_bits(first[k]), _bits(eng.grad[k]))]
    assert not moved, f"{name}: the second backward pass left other bits in {moved[:8]} ({len(moved)} buffers)"
    rows, cache, cache32 = [], {}, {}
    for key in eng.joins.writers:
        want = J.expected(eng, key, cache=cache)
        got = eng.grad[key]
        assert tuple(got.shape) == tuple(want.shape), (key, got.shape, want.shape)
        fig = J.figures(got, want)
        row = (key, J.join_kind(eng, key), want.numel(), fig, J.accept(fig, want.numel()))
        if floor:
            row += (J.figures(J.expected(eng, key, dtype=torch.float32, cache=cache32).to(eng.h16), want),)
        rows.append(row)
        # teeth, on the engine's own numbers: had any one writer of this join been lost or counted twice, the buffer would
        # differ from what it holds by that writer's contribution — the comparison must not accept that either
        parts = J.writer_parts(eng, key, cache=cache) if len(eng.joins.writers[key]) > 1 else []
        for label, p in zip(eng.joins.writers[key], parts):
            for what, mutated in (("dropped", want - p), ("doubled", want + p)):
                assert not J.accept(J.figures(got, mutated), want.numel()), \
                    f"{name}: {key} would pass with the contribution of {label} {what}"
    return eng, rows


def report_line(name, eng, rows):
    writers = eng.joins.writers
    worst = lambda i, pick: pick(rows, key=lambda r: r[3][i])
    c, o2, o4 = worst(0, min), worst(1, max), worst(2, max)
    return (f"gradient joins, {name}: {len(rows)} keys checked of {len(writers)}, {sum(len(w) > 1 for w in writers.values())} with "
            f">= 2 writers; worst cosine {c[3][0]:.7f} ({c[0]}), beyond 2 ulp {o2[3][1]:.3g} ({o2[0]}), "
            f"beyond 4 ulp {o4[3][2]:.3g} ({o4[0]})")


@pytest.mark.parametrize("name", list(ENGINES))
def test_every_gradient_join_matches_float64(cuda, name):
    eng, rows = run_engine(cuda, name)
    print(report_line(name, eng, rows))
    if name == "resnet26-persistent":     # the persistent kernels really run the data gradients of this engine
        ids = {n: eng.lib.rn_conv_kernel_id(ctypes.byref(p)) for n, p in eng.conv_launches}
        assert ids["fwd:tower0"] == 2 and ids["dgrad:tower3"] == 2 and ids["dgrad:g3b0_sc"] == 1, ids   # (eligible at 128^2)
    if name == "resnet26-f16":
        assert eng.f16 and eng.h16 == torch.float16
    if name == "resnet26-frozen-bn":
        assert all(grp.frozen for grp in eng.bn_groups.values())
    if name == "resnet26-frozen-initial":
        assert not eng.requires["g1b1_out"] and "g1b1_out" not in eng.joins.writers and "g2b0_a" in eng.joins.writers
    if name == "efficientnet-b0":
        kinds = {r[1] for r in rows}
        assert len(eng.dc_masks) == 9 and "se" in kinds and any("dw_dgrad" in k for k in kinds), kinds
    unchecked = set(eng.joins.writers) - {r[0] for r in rows}
    assert len(unchecked) == 0 <= UNCHECKED_CAP
    bad = [(r[0], r[1], r[2], tuple(float(f"{v:.4g}") for v in r[3])) for r in rows if not r[4]]
    assert not bad, f"{name}: {len(bad)} of {len(rows)} joins miss cos > 0.9999 / 2 ulp < 2e-2 / 4 ulp < 5e-3: {bad[:12]}"
