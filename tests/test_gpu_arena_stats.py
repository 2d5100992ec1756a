"""rn_arena_stats / rn_arena_histogram against stats_ref.py on hand-built arenas laid out by the engine's rule (first
segment at offset 4, every segment padded to a multiple of 4, slack behind the last one).  The reserved floats, all
padding and the tail hold NaN and 1e30 alternately: one of them read or counted breaks a norm, a maximum or a count.
Segment sizes sit on every path of the kernels: one lane, the tail alone, one 16-byte group, group + tail, a block less /
exactly / more than one element, three blocks.  Integers (counts, nonfinite) must be equal, min / max equal by value, the
norm within the bound stats_ref.norm_bound derives from the kernel's summation shape."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as O
import stats_ref as S

pytestmark = pytest.mark.gpu

# ST_THREADS of csrc/rn_stats.hip; a block is rn_optim_chunk() elements.  The only float32 additions of the norm are a lane's
# own: in a block of n elements, chain(n) = 4 * ceil((n // 4) / THREADS) + (1 if n % 4 else 0) — four per 16-byte load, one
# for a tail element, at most chunk / THREADS + 1 = 33 — and a segment's chain is the longest of its blocks
# (stats_ref.norm_bound computes exactly this).  Bound: (chain + 3) * 2^-24, relative.
THREADS = 256
RN_EINVAL, RN_ENOMEM = -1, -2


def _sizes(ch):
    return [1, 3, 4, 5, 7, ch - 1, ch, ch + 1, 2 * ch + 5]


def _subnormals(rng, n):
    bits = rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)
    return bits.view(np.float32)


def _contents(which, ch):
    rng = np.random.default_rng(77 + which)
    n = _sizes(ch)
    normal = lambda k, sigma: (rng.standard_normal(k) * sigma).astype(np.float32)     # noqa: E731
    if which == 0:
        hot = (0.5 + 0.01 * rng.random(n[8])).astype(np.float32)      # all but two elements inside one bucket of [-10, 10]
        hot[5], hot[ch + 17] = -10.0, 10.0
        return [normal(n[0], 1e-3),                                   # a single value: the last bucket
                np.float32([-0.5, 0.75, -0.5]),                       # two values: buckets 0 and 29
                np.zeros((n[2],), np.float32),                        # zero-initialised gammas
                np.full((n[3],), 0.25, np.float32),
                np.float32([np.nan, 1.0, np.inf, 2.0, -np.inf, 1.5, -3.0]),
                _subnormals(rng, n[5]),
                (np.arange(n[6]) % 31).astype(np.float32),            # 0 .. 30: width exactly 1, 30 clamped into bucket 29
                normal(n[7], 10.0),
                hot]
    mixed = normal(n[6], 1e-2)
    mixed[rng.integers(0, n[6], 40)] = np.nan
    mixed[rng.integers(0, n[6], 40)] = np.inf
    mixed[rng.integers(0, n[6], 40)] = -np.inf
    both = normal(n[7], 1.0)
    both[::3] = _subnormals(rng, len(both[::3]))
    return [np.float32([0.25]),
            normal(n[1], 0.1),
            np.arange(n[2], dtype=np.float32),
            np.float32([np.nan, np.inf, -np.inf, np.nan, np.inf]),    # no finite element
            normal(n[4], 1.0),
            normal(n[5], 1e-3),
            mixed,
            both,
            normal(n[8], 10.0)]


class Case:
    def __init__(self, which, dev):
        ch = O.chunk()
        n = len(_sizes(ch))
        self.lay = lay = O.build_layout(_sizes(ch), [0] * n, [False] * n, ch)
        self.parts = _contents(which, ch)
        arena = np.empty((lay.total,), np.float32)
        arena[0::2], arena[1::2] = np.nan, 1e30
        for i, x in enumerate(self.parts):
            lo, hi = lay.rng(i)
            assert hi - lo == x.size
            arena[lo:hi] = x
        used = np.zeros((lay.total,), bool)
        used[lay.elem.numpy()] = True
        assert not used[:4].any() and not used[-4:].any() and (~used).sum() == lay.untouched.numel()
        self.host = arena
        self.arena = torch.from_numpy(arena.copy()).to(dev)
        self.segs = torch.from_numpy(lay.segs.view("uint8").copy()).to(dev)
        self.bs = torch.from_numpy(lay.block_seg.copy()).to(dev)
        self.dev, self.n, self.nblk, self.chunk = dev, n, lay.n_blocks, ch
        self.ref = {b: [S.stats(x, b) for x in self.parts] for b in (1, 30, 64)}      # computed once, never changed


@pytest.fixture(scope="module")
def cases(cuda):
    return [Case(0, cuda), Case(1, cuda)]


def _lib(build):
    from retinanet import _C
    return _C.lib(build == "f16")


class Out:
    """sentinel-filled outputs and a workspace of the size the library asks for"""

    def __init__(self, lib, c, buckets=30):
        self.stats = torch.full((c.n, 3), 777.0, dtype=torch.float32, device=c.dev)
        self.bad = torch.full((c.n,), -7, dtype=torch.int32, device=c.dev)
        self.counts = torch.full((c.n, buckets), -7, dtype=torch.int32, device=c.dev)
        self.ws = torch.full((int(lib.rn_arena_stats_workspace_bytes(c.nblk, c.n)),), 0x5a, dtype=torch.uint8, device=c.dev)
        self.buckets = buckets

    def untouched(self):
        return bool((self.stats == 777.0).all() and (self.bad == -7).all() and (self.counts == -7).all()
                    and (self.ws == 0x5a).all())

    def bytes(self):
        return [t.cpu().numpy().tobytes() for t in (self.stats, self.bad, self.counts)]


def _run(lib, c, o, stream=None, histogram=True):
    from retinanet import _C
    st = _C.current_stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)
    _C.check(lib.rn_arena_stats(_C.ptr(c.arena), _C.ptr(c.segs), c.n, _C.ptr(c.bs), c.nblk, _C.ptr(o.stats), _C.ptr(o.bad),
                                _C.ptr(o.ws), o.ws.numel(), st), "rn_arena_stats")
    if histogram:
        _C.check(lib.rn_arena_histogram(_C.ptr(c.arena), _C.ptr(c.segs), c.n, _C.ptr(c.bs), c.nblk, _C.ptr(o.stats),
                                        o.buckets, _C.ptr(o.counts), st), "rn_arena_histogram")


def _compare(c, o, buckets):
    stats, bad, counts = o.stats.cpu().numpy(), o.bad.cpu().numpy(), o.counts.cpu().numpy()
    for i, (x, r) in enumerate(zip(c.parts, c.ref[buckets])):
        bound, chain = S.norm_bound(x.size, c.chunk, THREADS)
        got = stats[i, 0]
        if np.isfinite(r["norm"]):
            err = abs(float(got) - float(r["norm"])) / float(r["norm"]) if r["norm"] else abs(float(got))
            print(f"segment {i} size {x.size}: norm {got:.9g} ref {r['norm']:.9g} rel err {err:.3g} bound {bound:.3g} "
                  f"(chain {chain}) min {stats[i, 1]:.9g} max {stats[i, 2]:.9g} nonfinite {bad[i]}")
            assert np.isfinite(got) and err <= bound, (i, got, r["norm"], err, bound)
        elif np.isnan(r["norm"]):
            assert np.isnan(got), (i, got)
        else:
            assert got == np.inf, (i, got)
        assert stats[i, 1] == r["min"] and stats[i, 2] == r["max"], (i, stats[i], r["min"], r["max"])
        assert bad[i] == r["nonfinite"], (i, bad[i], r["nonfinite"])
        assert (counts[i] == r["counts"]).all(), (i, counts[i].tolist(), r["counts"].tolist())
        assert int(counts[i].sum()) + int(bad[i]) == x.size, i


@pytest.mark.parametrize("build", ["bf16", "f16"])
@pytest.mark.parametrize("which", [0, 1])
def test_stats_and_histogram_match_the_reference(cuda, cases, which, build):
    c, lib = cases[which], _lib(build)
    o = Out(lib, c)
    _run(lib, c, o)
    torch.cuda.synchronize()
    _compare(c, o, 30)
    if which == 0:                                   # the hand-derived answers of test_stats_ref_cpu.py, on the device
        counts = o.counts.cpu().numpy()
        assert counts[0].tolist() == [0] * 29 + [1] and counts[1, 0] == 2 and counts[1, 29] == 1
        assert counts[2].tolist() == [0] * 29 + [4] and counts[3].tolist() == [0] * 29 + [5]
        assert counts[8].max() == c.parts[8].size - 2 and counts[8, 0] == 1 and counts[8, 29] == 1      # the hot bucket
        assert o.stats[5, 1].item() != 0.0 and abs(o.stats[5, 1].item()) < 2.0 ** -126                    # subnormal kept
    assert c.arena.cpu().numpy().tobytes() == c.host.tobytes()                                           # read only


@pytest.mark.parametrize("buckets", [1, 64])
def test_one_bucket_and_sixty_four(cuda, cases, buckets):
    lib = _lib("bf16")
    for c in cases:
        o = Out(lib, c, buckets)
        _run(lib, c, o)
        torch.cuda.synchronize()
        _compare(c, o, buckets)


def test_same_bytes_on_every_run_and_stream(cuda, cases):
    c, lib = cases[0], _lib("bf16")
    before = c.arena.clone()
    first, again, side = Out(lib, c), Out(lib, c), Out(lib, c)
    _run(lib, c, first)
    _run(lib, c, again)
    _run(lib, c, again)                               # a second call into the same outputs: counts are cleared by the call
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    _run(lib, c, side, stream=s)
    s.synchronize()
    torch.cuda.synchronize()
    assert first.bytes() == again.bytes() == side.bytes()
    assert torch.equal(before.view(torch.int32), c.arena.view(torch.int32))       # byte for byte, NaN padding included
    assert c.arena.cpu().numpy().tobytes() == c.host.tobytes()


def test_refusals_leave_the_outputs_alone(cuda, cases):
    from retinanet import _C
    c, lib = cases[0], _lib("bf16")
    o = Out(lib, c)
    good = dict(arena=_C.ptr(c.arena), segs=_C.ptr(c.segs), nseg=c.n, bs=_C.ptr(c.bs), nblk=c.nblk, stats=_C.ptr(o.stats),
                bad=_C.ptr(o.bad), ws=_C.ptr(o.ws), wsb=o.ws.numel(), buckets=30, counts=_C.ptr(o.counts))

    def stats(**kw):
        a = dict(good, **kw)
        return lib.rn_arena_stats(a["arena"], a["segs"], a["nseg"], a["bs"], a["nblk"], a["stats"], a["bad"], a["ws"], a["wsb"],
                                  _C.current_stream())

    def hist(**kw):
        a = dict(good, **kw)
        return lib.rn_arena_histogram(a["arena"], a["segs"], a["nseg"], a["bs"], a["nblk"], a["stats"], a["buckets"],
                                      a["counts"], _C.current_stream())

    for kw in (dict(arena=None), dict(segs=None), dict(bs=None), dict(stats=None), dict(bad=None), dict(ws=None),
               dict(nseg=0), dict(nseg=-1), dict(nblk=0), dict(nblk=-3)):
        assert stats(**kw) == RN_EINVAL, kw
    assert stats(wsb=o.ws.numel() - 1) == RN_ENOMEM and stats(wsb=0) == RN_ENOMEM
    for kw in (dict(arena=None), dict(segs=None), dict(bs=None), dict(stats=None), dict(counts=None), dict(nseg=0),
               dict(nblk=0), dict(buckets=0), dict(buckets=-1), dict(buckets=65)):
        assert hist(**kw) == RN_EINVAL, kw
    torch.cuda.synchronize()
    assert o.untouched()
    assert lib.rn_arena_stats_workspace_bytes(c.nblk, c.n) >= c.nblk * 20
    assert stats() == 0 and hist() == 0                # the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    assert not o.untouched()
