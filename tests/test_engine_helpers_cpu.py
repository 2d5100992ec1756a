"""Host-side helpers of the engines that need no GPU."""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "retinanet-tensorflow2.x_amd"))


def _graph(depths):
    g = types.SimpleNamespace()
    g.convs = {f"c{i}": {"k": k, "cin": cin} for i, (k, cin) in enumerate(depths)}
    ops = [{"op": "conv", "conv": f"c{i}", "group": "grp"} for i in range(len(depths))]
    return g, ops


def test_split_by_depth_groups_the_deep_segments(monkeypatch):
    """engine.split_by_depth: a grouped forward launch whose segments differ 2x or more in K depth becomes two launches, the
    deep segments first; homogeneous groups and single ops stay one launch; RNET_GROUP_SPLIT=0 switches it off."""
    from retinanet.model.engine import split_by_depth
    monkeypatch.delenv("RNET_GROUP_SPLIT", raising=False)
    g, ops = _graph([(1, 2048), (1, 512), (1, 1024), (1, 2048)])       # the FPN lateral convs (c6-pre, p3, p4, p5)
    parts = split_by_depth(g, ops)
    assert [[o["conv"] for o in p] for p in parts] == [["c0", "c2", "c3"], ["c1"]]
    g, ops = _graph([(3, 256)] * 5)                                      # a shared head conv over five levels
    assert split_by_depth(g, ops) == [ops]
    g, ops = _graph([(1, 512), (1, 768)])                                # less than 2x apart
    assert split_by_depth(g, ops) == [ops]
    g, ops = _graph([(3, 64)])
    assert split_by_depth(g, ops) == [ops]
    monkeypatch.setenv("RNET_GROUP_SPLIT", "0")
    g, ops = _graph([(1, 2048), (1, 512)])
    assert split_by_depth(g, ops) == [ops]


def _joins():
    from retinanet.model.train_engine import GradientJoins
    names = ["c2", "c3", "p3", "bal:p3", "p4", "bal:p4"]
    return GradientJoins({n: "buffer of " + n for n in names}, {"p3": None, "p4": None})


def test_gradient_joins_first_writer_stores_later_ones_accumulate():
    """train_engine.GradientJoins.add: accumulate is False for the first caller of a key and True afterwards; the writers
    record lists the labels per key in call order."""
    j = _joins()
    assert j.add("c2", "dgrad:a") == ("buffer of c2", False)
    assert j.add("c3", "dgrad:b") == ("buffer of c3", False)
    assert j.add("c2", "bn:b", balanced=False) == ("buffer of c2", True)
    assert j.add("c2", "maxpool:c") == ("buffer of c2", True)
    assert j.writers == {"c2": ["dgrad:a", "bn:b", "maxpool:c"], "c3": ["dgrad:b"]}
    assert list(j.writers) == ["c2", "c3"]


def test_gradient_joins_balanced_names_go_to_the_bal_key():
    """A reader of a balanced level writes the `bal:` buffer, balanced=False (residual inputs) the tensor's own; the two keys
    count their writers apart."""
    j = _joins()
    assert j.add("p3", "dgrad:head") == ("buffer of bal:p3", False)
    assert j.add("p3", "bn:x", balanced=False) == ("buffer of p3", False)
    assert j.add("p3", "dgrad:head2") == ("buffer of bal:p3", True)
    assert j.add("c3", "dgrad:lateral") == ("buffer of c3", False)       # not balanced: its own key either way
    assert j.writers == {"bal:p3": ["dgrad:head", "dgrad:head2"], "p3": ["bn:x"], "c3": ["dgrad:lateral"]}


def test_gradient_joins_sole_refuses_an_earlier_writer():
    """sole: for kernels that overwrite their destination.  After an add, and a second time, it raises RuntimeError naming
    the tensor and the earlier writer; an add after it accumulates."""
    import pytest
    j = _joins()
    assert j.sole("c3", "topdown") == "buffer of c3"
    assert j.add("c3", "dgrad:late") == ("buffer of c3", True)          # sole, then add
    with pytest.raises(RuntimeError, match=r"se:x .*\bc3\b.*topdown"):   # sole twice (add in between)
        j.sole("c3", "se:x")
    j = _joins()
    j.sole("p4", "balance")
    with pytest.raises(RuntimeError, match=r"topdown .*\bp4\b.*balance"):   # sole twice
        j.sole("p4", "topdown")
    assert j.add("p4", "dgrad:head") == ("buffer of bal:p4", False)     # sole wrote the tensor's own key
    j = _joins()
    j.add("c2", "dgrad:a", balanced=False)
    with pytest.raises(RuntimeError, match=r"balance .*\bc2\b.*dgrad:a"):   # add, then sole
        j.sole("c2", "balance")
    assert j.writers == {"c2": ["dgrad:a"]}                               # the refused write is not recorded


def test_gradient_joins_needs_a_buffer_for_every_key():
    import pytest
    j = _joins()
    with pytest.raises(KeyError):
        j.add("c9", "dgrad:a")
    with pytest.raises(KeyError):
        j.sole("c9", "topdown")
    assert j.writers == {}
