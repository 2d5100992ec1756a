"""How many backward steps must write every activation-gradient buffer of a built TrainEngine, counted from its graph
alone, and the check of the planner's own record (engine.joins.writers) against it."""
from collections import Counter


def expected_writers(eng):
    """key of eng.grad -> number of gradient contributions the graph sends there: one per reader that needs a gradient at
    what it read.  Readers of a balanced pyramid level read BalanceFeatures' copy (the `bal:` key); a residual input is
    read as it is."""
    n = Counter()
    for op in eng.ops:
        kind = op["op"]
        if kind in ("conv", "dwconv") and eng.requires.get(op["inp"]):
            n["bal:" + op["inp"] if op["inp"] in eng.bal_src else op["inp"]] += 1
        if op.get("residual") and eng.requires.get(op["residual"]):
            n[op["residual"]] += 1
        if kind == "topdown":
            n.update(op["ins"])
        elif kind == "maxpool" and eng.requires.get(op["inp"]):
            n[op["inp"]] += 1
        elif kind == "se":
            n[op["inp"]] += 1
        elif kind == "balance":
            n.update(op["tensors"])
    return n


def check_joins(eng):
    """No contribution lost or doubled: every key has exactly the writers the graph gives it, every written key has a
    buffer, and a step whose kernel overwrites its destination (top-down, squeeze-excite, BalanceFeatures) is the first
    writer of it.  One kind of key is no overwrite: a top-down level that passes through (the top one, outs[l] IS ins[l])
    has one gradient buffer for dout and din, which its step updates in place — there the readers of the output must
    have written first, and the top-down step comes exactly once.  Returns the expected counts."""
    want = expected_writers(eng)
    writers = eng.joins.writers
    got = {key: len(labels) for key, labels in writers.items()}
    assert got == dict(want), sorted((k, got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert set(writers) <= set(eng.grad), sorted(set(writers) - set(eng.grad))
    through = {i for op in eng.ops if op["op"] == "topdown" for i, o in zip(op["ins"], op["outs"]) if i == o}
    for key, labels in writers.items():
        if key in through:
            assert labels.count("topdown") == 1 and labels[0] != "topdown", (key, labels)
            continue
        late = [s for s in labels[1:] if s in ("topdown", "balance") or s.startswith("se:")]
        assert not late, (key, labels)
    return want
