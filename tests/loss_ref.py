"""Float32 restatement of the focal-loss kernels' per-logit formula (csrc/rn_loss.hip: focal_pair, which focal_elem
follows with two reciprocals instead of one), and the tolerance the elementwise GPU checks derive from it.

Two references, neither derived from the other
----------------------------------------------
  * the truth is float64: oracle.focal_loss_elem / oracle.focal_loss_grad_elem, the reference's formula as written;
  * `focal_f32` is what an fp32 evaluation of the KERNEL's formula can reach: the same operations in the same order,
    every one rounded to float32 (numpy's exp2 / log2 / sqrt / division are correctly rounded or within an ulp; a fused
    multiply-add is the float64 product and sum rounded once more to float32).

`EMU_WORST` is the worst relative error of `focal_f32` against float64 over `sweep_x()` — logits in [-20, 20], both
labels, gamma 1.5 / 2.0 / 0.5 — for the loss (label smoothing 0 and 0.1) and for the gradient (label smoothing 0; with
label smoothing the gradient crosses zero and only a mixed bound can hold, `mixed_bound`).  The GPU tests allow
`ELEM_RTOL = 4 * EMU_WORST` against float64: the factor 4 is for the hardware's 1-ulp v_exp / v_log / v_rcp / v_sqrt
where numpy rounds correctly.  Nothing here looks at what the kernel returns.

form="old" is the gradient term the kernels had before: mod * (p - ys) for every logit.  For a positive with a confident
logit p rounds to 1 and p - 1 loses -(1 - p); tests/test_loss_ref_cpu.py asserts that this form misses ELEM_RTOL, i.e.
that the tolerance tells the two apart.  form="fixed" is what the kernels compute now: -(1 - p) - (ys - 1) for a positive
with x > SWITCH_X = 4, p - ys everywhere else (up to there p - 1 costs no more than the rest of the formula does:
EMU_WORST is 3.92e-6 with the switch at 0 or 3, 4.17e-6 at 4, 1.2e-5 at 5, 3.2e-5 at 6).
"""
import functools

import numpy as np

import oracle as o

F32 = np.float32
LOG2E = F32(1.44269504088896341)
GAMMAS = (1.5, 2.0, 0.5)
ALPHA = 0.25
SWITCH_X = F32(4.0)         # csrc/rn_loss.hip: RN_FOCAL_SWITCH_X
ELEM_RTOL_LIMIT = 5e-5       # if the restatement needed more than this, the formula would be the problem, not the bound
MIXED_ATOL = 1e-6            # label smoothing != 0: |err| <= rtol |want| + MIXED_ATOL max|want|


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(F32)


def focal_f32(x, pos, alpha=ALPHA, gamma=1.5, ls=0.0, form="fixed"):
    """(loss, grad) of one logit each, float32, in focal_pair's operation order.  x: f32 array, pos: bool array."""
    x = np.asarray(x, F32)
    pos = np.asarray(pos, bool)
    alpha, gamma, ls = F32(alpha), F32(gamma), F32(ls)
    one, two = F32(1.0), F32(2.0)
    y = np.where(pos, one, F32(0.0))
    ys = y * (one - ls) + F32(0.5) * ls
    t = np.exp2(-np.abs(x) * LOG2E)
    xp = np.maximum(x, F32(0.0))
    d1, d2 = one + t, two + t
    r = one / (d1 * d2)
    inv = r * d2                                   # 1 / (1 + t)
    s = t * (r * d1)                               # t / (2 + t)
    z = s * s
    pl = np.full_like(x, F32(1.0 / 15.0))
    for c in (13.0, 11.0, 9.0, 7.0, 5.0, 3.0, 1.0):
        pl = _fma(pl, z, F32(1.0 / c))
    l1p = two * s * pl
    ce = xp - x * ys + l1p
    ti = t * inv
    p = np.where(x >= 0, inv, ti)
    omp = np.where(x >= 0, ti, inv)
    q = np.where(pos, omp, p)
    a_t = np.where(pos, alpha, one - alpha)
    if gamma == F32(1.5):
        mod = q * np.sqrt(q)
    else:
        with np.errstate(divide="ignore"):
            mod = np.where(q > 0, np.exp2(gamma * np.log2(q)), F32(0.0)).astype(F32)
    loss = a_t * mod * ce
    dm = np.where(pos, -p, omp)
    dmod = gamma * dm * mod
    if form == "old":
        pmy = p - ys
    else:                                          # a positive with x > 4: -(1 - p) - (ys - 1), no p - 1
        pmy = np.where(pos & (x > SWITCH_X), -omp - (ys - one), p - ys)
    grad = a_t * (mod * pmy + ce * dmod)
    return loss.astype(F32), grad.astype(F32)


def sweep_x():
    """dense grid over [-20, 20] (every multiple of 1/256: 10 241 points, the integers among them) plus 20 000 random"""
    grid = np.arange(-20 * 256, 20 * 256 + 1, dtype=np.float64) / 256.0
    rnd = np.random.default_rng(20).uniform(-20.0, 20.0, 20000)
    return np.concatenate([grid, rnd]).astype(F32)


def truth(x, pos, gamma, ls, alpha=ALPHA):
    y = np.asarray(pos, np.float64)
    x = np.asarray(x, np.float64)
    return o.focal_loss_elem(x, y, alpha, gamma, ls), o.focal_loss_grad_elem(x, y, alpha, gamma, ls)


def rel_err(got, want):
    return np.abs(got.astype(np.float64) - want) / np.abs(want)


def mixed_bound(want, rtol):
    return rtol * np.abs(want) + MIXED_ATOL * np.abs(want).max()


@functools.lru_cache(maxsize=None)
def emu_table(form="fixed"):
    """{(gamma, ls, pos): (worst relative error of the loss, of the gradient)} over sweep_x()"""
    x = sweep_x()
    out = {}
    for gamma in GAMMAS:
        for ls in (0.0, 0.1):
            for pos in (False, True):
                m = np.full(x.shape, pos)
                lo, gr = focal_f32(x, m, gamma=gamma, ls=ls, form=form)
                wl, wg = truth(x, m, gamma, ls)
                out[(gamma, ls, pos)] = (float(rel_err(lo, wl).max()), float(rel_err(gr, wg).max()))
    return out


@functools.lru_cache(maxsize=None)
def emu_worst():
    t = emu_table()
    return max([v[0] for v in t.values()] + [v[1] for k, v in t.items() if k[1] == 0.0])


def elem_rtol():
    r = 4.0 * emu_worst()
    assert r <= ELEM_RTOL_LIMIT, f"the float32 restatement needs ELEM_RTOL = {r:.3g} > {ELEM_RTOL_LIMIT:.3g}"
    return r
