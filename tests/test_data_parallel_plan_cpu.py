"""Host logic of the data-parallel step without a GPU or the native library: the gradient-bucket planner
(retinanet/model/data_parallel.py plan_buckets) and the backward-step record (train_engine.BackwardStep)."""
import sys

import pytest

from conftest import PKG

sys.path.insert(0, PKG)

NAMES = ["v0", "v1", "v2", "v3", "v4", "v5"]
# six variables of 10, 3, 40, 8, 5 and 17 floats, optimizer chunk 16, laid out as TrainEngine._alloc_params does: the first
# offset is 4 (the flag slots), every size is rounded up to 4
P_OFF = {"v0": (4, 10), "v1": (16, 3), "v2": (20, 40), "v3": (60, 8), "v4": (68, 5), "v5": (76, 17)}
SEG_BLOCKS = {"v0": (0, 1), "v1": (1, 1), "v2": (2, 3), "v3": (5, 1), "v4": (6, 1), "v5": (7, 2)}
ARENA, BLOCKS = 96, 9
EXTENTS = [(0, 20, 0, 2), (20, 60, 2, 3), (60, 76, 5, 2), (76, 96, 7, 2)]     # begin, end, block_begin, block_count
IN_ORDER = {"v5": 0, "v4": 1, "v3": 2, "v2": 3, "v1": 4, "v0": 5}
V2_LAST = {"v5": 0, "v4": 1, "v3": 2, "v2": 6, "v1": 4, "v0": 3}              # bucket 0 would not be the last to complete


def _plan(ready_step, bucket_bytes=64):
    from retinanet.model.data_parallel import plan_buckets
    return plan_buckets(NAMES, P_OFF, SEG_BLOCKS, ready_step, bucket_bytes)


def _check_properties(buckets, bucket_at):
    assert buckets[0]["begin"] == 0 and buckets[-1]["end"] == ARENA
    for a, b in zip(buckets, buckets[1:]):            # the extents tile the arena: no gap, no overlap
        assert a["begin"] < a["end"] == b["begin"]
        assert a["block_begin"] + a["block_count"] == b["block_begin"]
    assert sum(b["block_count"] for b in buckets) == BLOCKS
    visited = [j for step in sorted(bucket_at) for j in bucket_at[step]]
    assert sorted(visited) == list(range(len(buckets)))     # every bucket once ...
    assert visited[-1] == 0                                  # ... the one with the flag slots last
    for step, js in bucket_at.items():
        assert all(buckets[j]["ready"] == step for j in js)


def test_buckets_in_backward_order():
    buckets, bucket_at = _plan(IN_ORDER)
    assert [(b["begin"], b["end"], b["block_begin"], b["block_count"]) for b in buckets] == EXTENTS
    assert [b["ready"] for b in buckets] == [5, 3, 2, 0]
    assert bucket_at == {5: [0], 3: [1], 2: [2], 0: [3]}
    _check_properties(buckets, bucket_at)


def test_bucket_0_goes_last_when_a_later_bucket_completes_after_it():
    buckets, bucket_at = _plan(V2_LAST)
    assert [(b["begin"], b["end"], b["block_begin"], b["block_count"]) for b in buckets] == EXTENTS
    assert [b["ready"] for b in buckets] == [6, 6, 2, 0]
    assert bucket_at == {6: [1, 0], 2: [2], 0: [3]}      # bucket 0 behind bucket 1 within the same step
    _check_properties(buckets, bucket_at)


@pytest.mark.parametrize("ready_step", [IN_ORDER, V2_LAST])
def test_one_bucket_when_the_arena_is_smaller_than_a_bucket(ready_step):
    buckets, bucket_at = _plan(ready_step, bucket_bytes=1 << 20)
    assert len(buckets) == 1
    assert (buckets[0]["begin"], buckets[0]["end"], buckets[0]["block_begin"], buckets[0]["block_count"]) == (0, ARENA, 0, BLOCKS)
    assert bucket_at == {max(ready_step.values()): [0]}
    _check_properties(buckets, bucket_at)


def test_backward_step_record():
    from retinanet.model.train_engine import BackwardStep
    calls = []
    step = BackwardStep(lambda st: calls.append(st) or "ran")
    assert step.side is False and step.writes == () and step.wgrad is None
    assert step("stream") == "ran" and calls == ["stream"]
    side = BackwardStep(calls.append, side=True, writes=["a/kernel"], wgrad=("p", "dw", "ws", 1))
    assert side.side is True and side.writes == ["a/kernel"] and side.wgrad[0] == "p"
    side("other")
    assert calls == ["stream", "other"]
    with pytest.raises(AttributeError):
        side.sdie = True              # a typo is an error, not a new attribute
