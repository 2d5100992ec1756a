"""The ulp-outlier metric shared by the tight slice test (test_gpu_train_kernels.py) and the gradient-join tests."""
import torch


def _ulp_outliers(got, want64, ulps=2.0, mantissa_bits=7):
    """fraction of bf16 elements farther than `ulps` bf16 ulps from the float64 value (ulp of the element's own magnitude,
    floored at 2^-8 of the tensor's rms: a sum that cancels to ~0 has the rounding of its terms, not of its value).
    mantissa_bits: the stored fraction bits of the storage type — 7 = bfloat16, 10 = IEEE half (the float16 build)"""
    w = want64.abs()
    rms = want64.pow(2).mean().sqrt()
    mag = torch.maximum(w, rms * 2.0 ** -8)
    ulp = torch.pow(2.0, torch.floor(torch.log2(mag)) - mantissa_bits)
    return ((got.double() - want64).abs() > ulps * ulp).double().mean().item()
