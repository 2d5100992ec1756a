"""The activation references of tests/act_ref.py and their acceptance rule, pinned on the CPU: the sweep holds every
finite value of the storage type, the float64 derivative equals autograd's, an fp32 transcription of the kernels'
formulas is ACCEPTED on every input of both storage types, and four deliberately wrong results are REJECTED — so a
kernel that passes test_gpu_activation_math.py cannot have any of these defects."""
import pytest
import torch

import act_ref as A
import pyramid_ref as R

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_holds_every_finite_value_once(dtype):
    x = A.sweep(dtype)
    assert x.shape == (1024, A.C) and x.dtype == dtype and bool(torch.isfinite(x.float()).all())
    assert A.n_finite(dtype) == (65280 if dtype == torch.bfloat16 else 63488)
    bits = x.view(torch.int16).reshape(-1).to(torch.int32) & 0xffff
    keep = bits != 0
    assert torch.equal(bits[keep], torch.arange(1 << 16, dtype=torch.int32)[keep]), "element i is bit pattern i"
    fi = torch.finfo(dtype)
    v = x.float()
    assert v.max().item() == fi.max and v.min().item() == -fi.max
    assert bool((v == 6).any()) and bool((x.view(torch.int16) == -32768).any()), "6 and -0 are there"
    assert bool(((v != 0) & (v.abs() < fi.smallest_normal)).any()), "subnormals are there"


def test_reference_derivative_is_autograd_of_the_reference_value():
    u = torch.linspace(-30, 30, 4001, dtype=A.F64).requires_grad_(True)
    A.act_fwd(u, "swish").sum().backward()
    assert (u.grad - A.act_deriv(u.detach(), "swish")).abs().max().item() < 1e-14
    z = torch.tensor([-1.0, -0.0, 0.0, 2.0 ** -133, 5.96875, 6.0, 6.03125, 7.0], dtype=A.F64)
    assert A.act_deriv(z, "relu").tolist() == [0, 0, 0, 1, 1, 1, 1, 1]
    assert A.act_deriv(z, "relu6").tolist() == [0, 0, 0, 1, 1, 0, 0, 0]
    assert A.act_deriv(z, "none").tolist() == [1] * 8
    assert A.act_fwd(z, "relu6").tolist() == [0, 0, 0, 2.0 ** -133, 5.96875, 6, 6, 6]
    # the ends of the domain: no NaN, swish(-big) = -0, swish(big) = big, the derivative 0 and 1
    big = torch.tensor([-3.0e38, 3.0e38], dtype=A.F64)
    assert A.act_fwd(big, "swish").tolist() == [-0.0, 3.0e38] and A.act_deriv(big, "swish").tolist() == [0.0, 1.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_rule_accepts_the_fp32_transcription_on_every_input(dtype):
    x = A.sweep(dtype)
    ref = A.act_fwd(R.f64(x), "swish")
    ok, ratio, outside, worst = A.check(A.fp32_swish(x, dtype), ref, dtype, A.value_slack(ref, "swish"))
    print(f"swish value {dtype}: worst ratio {ratio:.4f} at x = {x.reshape(-1)[worst].item()!r}")
    assert ok, (ratio, outside, x.reshape(-1)[worst].item())
    ref = A.act_deriv(R.f64(x), "swish")
    ok, ratio, outside, worst = A.check(A.fp32_swish_deriv(x, dtype), ref, dtype, A.deriv_slack(ref, "swish"))
    print(f"swish derivative {dtype}: worst ratio {ratio:.4f} at x = {x.reshape(-1)[worst].item()!r}")
    assert ok, (ratio, outside, x.reshape(-1)[worst].item())
    # inputs below -88.7: fp32 returns -0 where the value is a tiny negative number; the 1e-30 floor accepts it
    far = x.float() < -89.0
    assert bool((A.fp32_swish(x, dtype)[far].float() == 0).all())
    if dtype == torch.bfloat16:
        assert A.act_fwd(R.f64(x), "swish")[far].abs().max().item() > float(torch.finfo(dtype).smallest_normal)
    # the piecewise-linear activations: results are storage values, compared bit for bit (zeros by value)
    for act in ("none", "relu", "relu6"):
        want = A.act_fwd(R.f64(x), act).to(dtype)
        assert A.same_values(A.act_fwd(x.float(), act).to(dtype), want)
        assert A.accept(want, A.act_fwd(R.f64(x), act), dtype, A.value_slack(R.f64(x), act))
    assert A.same_values(torch.tensor([0.0, -0.0], dtype=dtype), torch.tensor([-0.0, 0.0], dtype=dtype))
    assert not A.same_values(torch.tensor([0.0, 1.0], dtype=dtype), torch.tensor([0.0, -1.0], dtype=dtype))
    assert not A.same_values(torch.tensor([float("nan")], dtype=dtype), torch.tensor([float("nan")], dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rule_accepts_a_flushed_subnormal_and_nothing_else_that_small(dtype):
    tiny = float(torch.finfo(dtype).smallest_normal)
    ref = torch.tensor([tiny / 2, tiny / 2, tiny / 2, tiny * 4], dtype=A.F64)
    got = torch.tensor([tiny / 2, 0.0, tiny * 2, 0.0], dtype=A.F64)
    ok, _, outside, worst = A.check(got, ref, dtype, torch.zeros_like(ref))
    assert not ok and outside == 2
    assert A.accept(got[:2], ref[:2], dtype, torch.zeros(2, dtype=A.F64))
    assert not A.accept(torch.tensor([float("nan")], dtype=A.F64), ref[:1], dtype, torch.zeros(1, dtype=A.F64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rule_rejects_an_identity_gate_for_swish(dtype):
    x = A.sweep(dtype)
    ref = A.act_deriv(R.f64(x), "swish")
    ok, ratio, outside, _ = A.check(torch.ones_like(x), ref, dtype, A.deriv_slack(ref, "swish"))
    print(f"identity gate {dtype}: {outside} inputs outside, worst ratio {ratio:.1f}")
    assert not ok and outside > 40000


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("res", [0.5, -3.0])
def test_rule_rejects_a_gate_taken_in_front_of_the_residual_add(dtype, res):
    y = A.sweep(dtype)
    v = R.round_storage(R.f64(y) + res, dtype)                   # what the forward pass fed to swish
    v = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
    ref = A.act_deriv(v, "swish")
    slack = A.deriv_slack(ref, "swish")
    assert A.accept(A.fp32_swish_deriv(v.to(dtype), dtype), ref, dtype, slack), "the gate at the stored sum"
    ok, ratio, outside, _ = A.check(A.fp32_swish_deriv(y, dtype), ref, dtype, slack)
    print(f"gate without the residual {res} {dtype}: {outside} inputs outside, worst ratio {ratio:.1f}")
    assert not ok and outside > 20000


@pytest.mark.parametrize("dtype", DTYPES)
def test_rule_rejects_a_sigmoid_that_is_off_by_2_to_the_minus_12(dtype):
    x = A.sweep(dtype)
    ref = A.act_fwd(R.f64(x), "swish")
    ok, ratio, outside, _ = A.check(A.fp32_swish(x, dtype, rel=2.0 ** -12), ref, dtype, A.value_slack(ref, "swish"))
    print(f"value with sigmoid (1 + 2^-12) {dtype}: {outside} inputs outside, worst ratio {ratio:.2f}")
    assert not ok and outside >= 1
    ref = A.act_deriv(R.f64(x), "swish")
    ok, ratio, outside, _ = A.check(A.fp32_swish_deriv(x, dtype, rel=2.0 ** -12), ref, dtype, A.deriv_slack(ref, "swish"))
    print(f"derivative with sigmoid (1 + 2^-12) {dtype}: {outside} inputs outside, worst ratio {ratio:.2f}")
    assert not ok and outside >= 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_rule_rejects_swish_of_the_unrounded_residual_sum(dtype):
    """pairs (y, residual) whose sum is not a storage value: residual = 7/16 of y's spacing, so rs(y + residual) = y"""
    eps = float(torch.finfo(dtype).eps)
    y = A.sweep(dtype)
    y = y[(y.float() >= 0.5) & (y.float() < 8.0)]
    y64 = R.f64(y)
    _, e = torch.frexp(y64)
    res = torch.exp2((e - 1).to(A.F64)) * eps * 7 / 16
    assert torch.equal(R.round_storage(res, dtype), res), "the residual is a storage value"
    stored = R.round_storage(y64 + res, dtype)
    assert torch.equal(stored, y64) and bool((y64 + res != stored).all()), "the two sums differ in every pair"
    ref = A.act_fwd(stored, "swish")
    slack = A.value_slack(ref, "swish")
    assert A.accept(A.fp32_swish(stored.to(dtype), dtype), ref, dtype, slack)
    wrong = torch.from_numpy((y64 + res).float().numpy() * A.fp32_sigmoid((y64 + res).float().numpy())).to(dtype)
    ok, ratio, outside, _ = A.check(wrong, ref, dtype, slack)
    print(f"swish of the unrounded sum {dtype}: {outside} of {y.numel()} pairs outside, worst ratio {ratio:.2f}")
    assert not ok and outside > y.numel() // 20
