"""Tolerances of the fp64 parity tests (test_rowwise_parity_gpu.py, test_head_parity_gpu.py; the attention kernels' file,
test_attention_parity_gpu.py, takes its absolute term A from tol_a and adds a per-element bound: tests/attention_ref.py).

Every comparison is  kernel output  against  r = the operation in float64 on the CPU, from the same bf16 / fp32 inputs.
The absolute term A of a tolerance comes from the REFERENCE alone: the same operation by torch's own float32 op on the CPU
gives e32 = max |r32 - r| over the test's inputs, and A = max(8 * e32, 2^-20 * max |r|). The factor 8 covers a kernel's
different summation order (wave trees against sequential sums) and the fast exp / rsqrt / rcp instructions, a few ulp each;
the floor is about 8 fp32 ulp of the output's largest value, for the cases where torch's float32 op happens to be exact.

  fp32 outputs:  |got - r| <= A
  bf16 outputs:  |got - r| <= 2^-8 |r| + A      (rounding to bf16 is 2^-9 relative, doubled for a value on a boundary)

No element is left out of a comparison. Each check prints its figures before it asserts (name, e32, A, largest error,
share of A used - for a bf16 output after taking off the 2^-8 |r| that correct rounding may use by itself): run with -s to
collect them (profiles/rowwise_head_parity.md is such a collection).
"""
import torch


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0, shift=0.0, dtype=torch.float32):
    """Seeded normal inputs, made on the CPU (the same on every machine)."""
    return (torch.randn(shape, generator=gen(seed)) * scale + shift).to(dtype)


def leaf(t, dtype):
    """A fresh autograd leaf in `dtype` (never the input tensor itself, which .to() returns for an equal dtype)."""
    return t.detach().to(dtype).clone().requires_grad_(True)


def _cpu64(t):
    return t.detach().to("cpu", torch.float64)


def tol_a(r32, r64):
    r64 = _cpu64(r64)
    e32 = float((_cpu64(r32) - r64).abs().max()) if r64.numel() else 0.0
    peak = float(r64.abs().max()) if r64.numel() else 0.0
    return e32, max(8.0 * e32, 2.0 ** -20 * peak)


def _report(name, kind, e32, a, err, used):
    print(f"PARITY {name} [{kind}] e32={e32:.3e} A={a:.3e} max_err={err:.3e} used={used:.3f}")


def check_f32(name, got, r64, r32):
    """fp32 output against the fp64 reference: |got - r| <= A everywhere."""
    assert got.dtype == torch.float32, got.dtype
    r = _cpu64(r64)
    g = _cpu64(got)
    assert g.shape == r.shape, (g.shape, r.shape)
    e32, a = tol_a(r32, r)
    err = float((g - r).abs().max()) if r.numel() else 0.0
    _report(name, "f32", e32, a, err, err / a if a > 0 else 0.0)
    assert torch.isfinite(g).all(), name
    assert err <= a, f"{name}: max |got - r| = {err:.3e} > A = {a:.3e} (e32 = {e32:.3e})"


def check_bf16(name, got, r64, r32):
    """bf16 output against the fp64 reference: |got - r| <= 2^-8 |r| + A everywhere."""
    assert got.dtype == torch.bfloat16, got.dtype
    r = _cpu64(r64)
    g = _cpu64(got)
    assert g.shape == r.shape, (g.shape, r.shape)
    e32, a = tol_a(r32, r)
    bound = 2.0 ** -8 * r.abs() + a
    diff = (g - r).abs()
    # share of A used by what the rounding to bf16 (up to 2^-8 |r| by itself, just above a power of two) does not explain
    used = float(((diff - 2.0 ** -8 * r.abs()) / a).clamp(min=0).max()) if r.numel() and a > 0 else float((diff > bound).any())
    err = float(diff.max()) if r.numel() else 0.0
    _report(name, "bf16", e32, a, err, used)
    assert torch.isfinite(g).all(), name
    bad = diff > bound
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside 2^-8 |r| + A, A = {a:.3e}; "
                           f"worst |got - r| = {float(diff[bad].max()):.3e}")
