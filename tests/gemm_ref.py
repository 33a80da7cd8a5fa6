"""Reference, data makers, checks and case tables of the GEMM parity tests (test_gemm_ref_cpu.py pins this file on the CPU,
test_gemm_parity_gpu.py judges the kernels of gemm_bf16.hip, gemm256.hip, gemm_w4.hip, gemm_a4.hip, gemm_tn*.hip by it).

Two kinds of data, two kinds of check.

EXACT data (`ints`): integers uniform in [-lim, lim] times a power of two, as bf16. With lim <= 16 and K <= 4224 every
product and every partial sum is an integer multiple of scale^2 below 2^24, so an fp32 accumulator is exact in ANY order
and the float64 reference is the one right answer: `check_exact` is torch.equal on the whole allocation, sentinels
included. Biases are odd quarters (no pre-activation is zero, nothing kept by a dropout can round back onto its
residual), residuals and the `aux` input small integers / bf16-exact sixteenths.

RANDOM data (and the transcendental epilogues on exact data): `check_bound`, for EVERY element

    |got - r| <= half_ulp(r, out dtype) + (K + adds) * 2^-23 * S + a_extra            A := the last two terms

  r        the operation in float64 from the same bf16 / fp32 inputs
  S        the same operation on absolute values (|alpha| |A| @ |B|^T + |bias| + |C0| ...), in float64
  K + adds the fp32 additions behind an element: K products, and `adds` further ones (split shares of an atomic form, bias,
           residual). (K + adds) * 2^-23 * S is the worst case of such a sum in any order with unit 2^-23, not 2^-24: one
           correctly rounded add per product is documented for the fp32 MFMA only, so the bound allows the bf16 MFMA a
           truncating internal add. Derived, not measured.
  half_ulp half a unit in the last place of the output type at |r| (0 for fp32); within A of a power of two the larger
           binade's - the fp32 value that is rounded may lie on the other side of it.
  a_extra  the transcendental epilogues only: parity_util.tol_a (factor 8, as documented there) of the same epilogue by
           torch's float32 gelu / gelu' (through autograd) on the CPU against float64, on the same pre-activations. Those
           cases run on exact data (their S is taken as 0: the product carries no error), so a_extra is their whole
           tolerance.

Order of the epilogue (gemm_common.h epilogue8_pre): alpha, bias, saved value (pre-activation or gelu'), GELU, * gelu'(aux) (or
* aux with AUX_GRAD), dropout scaled by float32(1 / (1 - float32(p))), residual. The atomic output adds alpha * product
into what C held and takes no epilogue.
"""
import functools

import numpy as np
import torch

from oracle import dropout_oracle as do
from stonkgs_amd import _hip as H
from tests.parity_util import gen, randn, tol_a

B, G, R, SV, GB, D, AG = (H.EPI_BIAS, H.EPI_GELU, H.EPI_RESID, H.EPI_SAVE_PREACT, H.EPI_GELU_BWD, H.EPI_DROPOUT,
                          H.EPI_AUX_GRAD)
BF16, F32, ATOMIC, F16 = H.EPI_OUT_BF16, H.EPI_OUT_F32, H.EPI_OUT_F32_ATOMIC, H.EPI_OUT_F16
OUT_DTYPE = {BF16: torch.bfloat16, F32: torch.float32, ATOMIC: torch.float32, F16: torch.float16}
TILE128, WAVE8, WAVE4, WAVE4_192, ASM4, ASM4_192 = (H.GEMM_TILE128, H.GEMM_WAVE8, H.GEMM_WAVE4, H.GEMM_WAVE4_192,
                                                    H.GEMM_ASM4, H.GEMM_ASM4_192)
KERNEL_NAMES = {H.GEMM_AUTO: "AUTO", TILE128: "TILE128", WAVE8: "WAVE8", WAVE4: "WAVE4", WAVE4_192: "WAVE4_192",
                H.GEMM_DISPATCHED: "DISPATCHED", H.GEMM_DISPATCHED2: "DISPATCHED2", ASM4: "ASM4", ASM4_192: "ASM4_192"}
SENTINEL = -768.0      # what every output allocation is filled with (exact in bf16, fp16 and fp32)
PAD = 1000.0           # what the padding of every operand holds: large, finite, must not leak in


def epi_name(out, epi):
    bits = "|".join(n for n, b in (("B", B), ("G", G), ("SV", SV), ("GB", GB), ("AG", AG), ("D", D), ("R", R)) if epi & b)
    return {BF16: "bf16", F32: "f32", ATOMIC: "atomic", F16: "f16"}[out] + ":" + (bits or "0")


# ---------------------------------------------------------------------------------------------------- the instance table
# Every `case` (and every early return) of the four launchers' switches: (kernel, output mode, epilogue, where it is
# listed). An epilogue that a switch sends to its `default` (the runtime-flag instance, EPI = -1) is marked so.
INSTANCES = [
    # launch_tile128, gemm_bf16.hip
    (TILE128, ATOMIC, 0, "gemm_bf16.hip:300 launch<2, true, -1>"),
    (TILE128, F16, 0, "gemm_bf16.hip:301 launch<3, true, 0>"),
    (TILE128, F32, 0, "gemm_bf16.hip:302 launch<1, true, 0>"),
    (TILE128, F32, B, "gemm_bf16.hip:302 launch<1, true, -1> (runtime flags)"),
    (TILE128, BF16, 0, "gemm_bf16.hip:304 case 0"),
    (TILE128, BF16, B, "gemm_bf16.hip:305 case B"),
    (TILE128, BF16, B | G | SV, "gemm_bf16.hip:306 case B | G | SV"),
    (TILE128, BF16, GB, "gemm_bf16.hip:307 case GB"),
    (TILE128, BF16, B | G | SV | AG, "gemm_bf16.hip:308 case B | G | SV | AG"),
    (TILE128, BF16, GB | AG, "gemm_bf16.hip:309 case GB | AG"),
    (TILE128, BF16, R, "gemm_bf16.hip:310 case R"),
    (TILE128, BF16, B | R, "gemm_bf16.hip:311 case B | R"),
    (TILE128, BF16, B | R | D, "gemm_bf16.hip:312 case B | R | D"),
    # ... and its runtime-flag instance (gemm_bf16.hip:313 default, :302 for fp32 output) on what no case lists
    (TILE128, BF16, B | G, "gemm_bf16.hip:313 default launch<0, true, -1>: bias + GELU, no saved pre-activation"),
    (TILE128, BF16, B | D, "gemm_bf16.hip:313 default: dropout without a residual"),
    (TILE128, F32, D, "gemm_bf16.hip:302 launch<1, true, -1>: dropout alone, fp32 output"),
    (TILE128, F32, B | R | D, "gemm_bf16.hip:302 launch<1, true, -1>: bias + dropout + residual, fp32 output"),
    (TILE128, BF16, GB | AG | R, "gemm_bf16.hip:313 default: both side operands (ldaux and ldr in one launch)"),
    # stonk_gemm256_launch, gemm256.hip
    (WAVE8, F32, 0, "gemm256.hip:566 launch256<1, 0>"),
    (WAVE8, F32, B, "gemm256.hip:566 launch256<1, -1> (runtime flags)"),
    (WAVE8, ATOMIC, 0, "gemm256.hip:567 launch256<2, 0>"),
    (WAVE8, F16, 0, "gemm256.hip:568 launch256<3, 0>"),
    (WAVE8, BF16, 0, "gemm256.hip:570 case 0"),
    (WAVE8, BF16, B, "gemm256.hip:571 case B"),
    (WAVE8, BF16, B | G, "gemm256.hip:572 case B | G"),
    (WAVE8, BF16, B | G | SV, "gemm256.hip:573 case B | G | SV"),
    (WAVE8, BF16, GB, "gemm256.hip:574 case GB"),
    (WAVE8, BF16, B | G | SV | AG, "gemm256.hip:575 case B | G | SV | AG"),
    (WAVE8, BF16, GB | AG, "gemm256.hip:576 case GB | AG"),
    (WAVE8, BF16, R, "gemm256.hip:577 case R"),
    (WAVE8, BF16, B | R, "gemm256.hip:578 case B | R"),
    (WAVE8, BF16, B | R | D, "gemm256.hip:579 default launch256<0, -1> (runtime flags)"),
    (WAVE8, BF16, GB | AG | R, "gemm256.hip:579 default: both side operands (ldaux and ldr in one launch)"),
    # stonk_gemm_w4_launch, gemm_w4.hip
    (WAVE4_192, BF16, 0, "gemm_w4.hip:528 case 0 (192)"),
    (WAVE4_192, BF16, B, "gemm_w4.hip:529 case B (192)"),
    (WAVE4_192, BF16, R, "gemm_w4.hip:530 case R (192)"),
    (WAVE4_192, BF16, B | R, "gemm_w4.hip:531 case B | R (192)"),
    (WAVE4_192, BF16, B | R | D, "gemm_w4.hip:532 default (192): epi_has_192 leaves B | R | D only"),
    (WAVE4, F32, 0, "gemm_w4.hip:535 launch_w4<1, 0>"),
    (WAVE4, F32, B, "gemm_w4.hip:535 launch_w4<1, -1> (runtime flags)"),
    (WAVE4, ATOMIC, 0, "gemm_w4.hip:536 launch_w4<2, 0>"),
    (WAVE4, BF16, 0, "gemm_w4.hip:538 case 0"),
    (WAVE4, BF16, B, "gemm_w4.hip:539 case B"),
    (WAVE4, BF16, B | G, "gemm_w4.hip:540 case B | G"),
    (WAVE4, BF16, B | G | SV, "gemm_w4.hip:541 case B | G | SV"),
    (WAVE4, BF16, GB, "gemm_w4.hip:542 case GB"),
    (WAVE4, BF16, B | G | SV | AG, "gemm_w4.hip:543 case B | G | SV | AG"),
    (WAVE4, BF16, GB | AG, "gemm_w4.hip:544 case GB | AG"),
    (WAVE4, BF16, R, "gemm_w4.hip:545 case R"),
    (WAVE4, BF16, B | R, "gemm_w4.hip:546 case B | R"),
    (WAVE4, BF16, B | R | D, "gemm_w4.hip:547 case B | R | D"),
    (WAVE4, BF16, B | D, "gemm_w4.hip:548 default launch_w4<0, -1> (runtime flags)"),
    # stonk_gemm_a4_launch / stonk_gemm_a4_has_instance, gemm_a4.hip
    (ASM4, F16, 0, "gemm_a4.hip:473 launch_a4<OUT_F16, 256> (has_instance :445)"),
    (ASM4_192, ATOMIC, 0, "gemm_a4.hip:474 launch_a4<OUT_F32_ATOMIC, 192> (has_instance :447)"),
    (ASM4_192, BF16, 0, "gemm_a4.hip:477 case 0 (192)"),
    (ASM4_192, BF16, B, "gemm_a4.hip:478 case B (192)"),
    (ASM4_192, BF16, R, "gemm_a4.hip:479 case R (192)"),
    (ASM4_192, BF16, B | R, "gemm_a4.hip:480 case B | R (192)"),
    (ASM4_192, BF16, B | R | D, "gemm_a4.hip:481 default (192): epi_has_192 (gemm_common.h:215) leaves B | R | D only"),
    (ASM4, BF16, 0, "gemm_a4.hip:485 case 0"),
    (ASM4, BF16, B, "gemm_a4.hip:486 case B"),
    (ASM4, BF16, B | G, "gemm_a4.hip:487 case B | G"),
    (ASM4, BF16, B | G | SV, "gemm_a4.hip:488 case B | G | SV"),
    (ASM4, BF16, GB, "gemm_a4.hip:489 case GB"),
    (ASM4, BF16, B | G | SV | AG, "gemm_a4.hip:490 case B | G | SV | AG"),
    (ASM4, BF16, GB | AG, "gemm_a4.hip:491 case GB | AG"),
    (ASM4, BF16, R, "gemm_a4.hip:492 case R"),
    (ASM4, BF16, B | R, "gemm_a4.hip:493 case B | R"),
    (ASM4, BF16, B | R | D, "gemm_a4.hip:494 case B | R | D"),
]

# One refusal per kernel and reason: (kernel, output mode, epilogue, kwargs, status, why)
REFUSALS = [
    (WAVE8, BF16, B, dict(alpha=0.5), H.ESHAPE, "the eight-wave kernel's bias rides in the accumulators: alpha == 1"),
    (WAVE4, F16, 0, {}, H.ESHAPE, "the four-wave kernel has no fp16 output"),
    (WAVE4, BF16, 0, dict(K=192), H.ESHAPE, "the four-wave kernel walks K tiles in pairs"),
    (WAVE4, BF16, GB | R, {}, H.ESHAPE, "one side operand at most"),
    (WAVE4_192, BF16, B | G, {}, H.ESHAPE, "no 192-wide GELU instance (epi_has_192)"),
    (WAVE4_192, F32, 0, {}, H.ESHAPE, "192-wide tiles: bf16 output only"),
    (WAVE4_192, BF16, 0, dict(N=256), H.ESHAPE, "192-wide tiles: N % 192 == 0"),
    (ASM4, F32, 0, {}, H.ESHAPE, "the written-out kernel has no plain fp32 output"),
    (ASM4, BF16, 0, dict(alpha=0.5), H.ESHAPE, "bf16 output: alpha == 1"),
    (ASM4, BF16, 0, dict(K=192), H.ESHAPE, "an even number of K tiles"),
    (ASM4, BF16, B | D, {}, H.ESHAPE, "gemm_a4.hip:495 default: no runtime-flag instance"),
    (ASM4, ATOMIC, 0, {}, H.ESHAPE, "the atomic form exists on 256 x 192 tiles only (has_instance :447)"),
    (ASM4_192, F16, 0, {}, H.ESHAPE, "fp16 output on 256-wide tiles only (has_instance :445)"),
    (ASM4_192, BF16, GB, {}, H.ESHAPE, "no 192-wide GELU' instance (epi_has_192)"),
    (TILE128, F16, B, {}, H.EINVAL, "fp16 output takes no epilogue"),
    (TILE128, BF16, AG, {}, H.EINVAL, "AUX_GRAD alone"),
    (TILE128, BF16, 0, dict(split_k=2), H.EINVAL, "a K split needs the atomic output"),
]

# AUTO: one case per arm of the routing lambda of stonk_gemm_nt_bf16 (gemm_bf16.hip:398-422): (arm, M, N, K, out, epi, alpha)
AUTO_ARMS = [
    ("written-out kernel: bf16, M >= 1024 (:401)", 1024, 768, 128, BF16, B | R, 1.0),
    ("written-out kernel: fp16 logits (:401)", 1024, 256, 128, F16, 0, 1.0),
    ("four-wave: side operand, alpha != 1 (:413)", 1024, 256, 128, BF16, R, 0.5),
    ("four-wave: wide bias alone, N % 192 == 0, alpha != 1 (:413)", 1024, 1536, 128, BF16, B, 0.5),
    ("eight-wave: wide fp32 output (:417)", 1024, 1536, 128, F32, 0, 1.0),
    ("four-wave on 192-wide tiles: plain N = 768, alpha != 1 (:419)", 1024, 768, 128, BF16, 0, 0.5),
    ("128x128: fewer than 1024 rows (:422)", 301, 768, 128, BF16, B | R, 1.0),
    ("128x128: fp32 output, N < 1536 (:422)", 1024, 256, 128, F32, 0, 0.5),
]

HOST_M = (1, 129, 255, 256, 257, 301, 1024)       # host row counts either side of the 128- and 256-row tile edges
DEV_M = (0, 1, 255, 256, 257)                     # *m_dev (and the capacity M itself)
DEV_K = (0, 1, 63, 64, 65, 129)                   # *k_dev (and K itself)
SEEDS = (0, 77, 2 ** 32 - 1)


def is_transcendental(epi):
    """Does the epilogue evaluate erf / exp (GELU, a stored gelu', gelu'(aux))? Those go through check_bound."""
    return bool(epi & G) or (epi & GB and not epi & AG)


# ---------------------------------------------------------------------------------------------------------- data makers
def ints(shape, lim, seed, scale=1.0):
    """Integers uniform in [-lim, lim] times `scale` (a power of two), as bf16; made on the CPU, the same everywhere."""
    assert lim <= 127 and float(np.log2(scale)).is_integer()
    v = torch.randint(-lim, lim + 1, tuple(shape), generator=gen(seed)).to(torch.float32) * scale
    out = v.to(torch.bfloat16)
    assert torch.equal(out.float(), v)
    return out


def quarters(n, seed):
    """fp32 bias of odd quarters, +-0.25 / 0.5 / 0.75: added to an integer it never gives zero."""
    q = torch.randint(1, 4, (n,), generator=gen(seed)).float() * 0.25
    s = torch.randint(0, 2, (n,), generator=gen(seed + 1)).float() * 2 - 1
    return q * s


def sixteenths(shape, seed, lim=48):
    """bf16-exact multiples of 1/16 in [-lim/16, lim/16]: the `aux` input of the GELU' epilogues."""
    return ints(shape, lim, seed, 1.0 / 16)


@functools.lru_cache(maxsize=None)
def oracle_keep(M, N, seed, p):
    """The epilogue's keep mask, stonk_keep_key(rowkey(m), colkey(n)), from the oracle: bool [M, N]."""
    return torch.from_numpy(do.keep(np.arange(M), np.arange(N), seed, p).copy())


def drop_scale(p, dt=torch.float64):
    """What the launcher computes in C float: 1.0f / (1.0f - p)."""
    return torch.tensor(float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))), dtype=dt)


# ------------------------------------------------------------------------------------------------------------ reference
def _gelu(x):
    return torch.nn.functional.gelu(x)


def _gelu_grad(x):
    leaf = x.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_gelu(leaf).sum(), leaf)
    return g.detach()


def _nt(A, Bm, flags, bias, resid, aux_in, alpha, C0, rows, keep, drop_p, dt, prod=None):
    """The operation in `dt` (float64: the reference; float32: the emulation r32), rows [0, rows): (value before the
    output rounding, aux to be stored or None). prod: A @ Bm^T in `dt` where the caller has it already."""
    rows = A.shape[0] if rows is None else rows
    out, epi = flags & 3, flags & ~3
    v = (A[:rows].to(dt) @ Bm.to(dt).t() if prod is None else prod[:rows].to(dt)) * torch.tensor(alpha, dtype=dt)
    if out == ATOMIC:
        return C0[:rows].to(dt) + v, None
    aux = None
    if epi & B:
        v = v + bias.to(dt)
    if epi & SV:
        aux = _gelu_grad(v) if epi & AG else v.clone()
    if epi & G:
        v = _gelu(v)
    if epi & GB:
        u = aux_in[:rows].to(dt)
        v = v * (u if epi & AG else _gelu_grad(u))
    if epi & D:
        v = torch.where(keep[:rows], v * drop_scale(drop_p, dt), torch.zeros((), dtype=dt))
    if epi & R:
        v = v + resid[:rows].to(dt)
    return v, aux


def gemm_nt_ref(A, Bm, flags=0, bias=None, resid=None, aux_in=None, alpha=1.0, C0=None, rows=None, keep_mask=None,
                drop_p=0.0, prod=None):
    """float64: (the value before the output rounding, the aux to be stored or None), rows [0, rows) x N."""
    return _nt(A, Bm, flags, bias, resid, aux_in, alpha, C0, rows, keep_mask, drop_p, torch.float64, prod)


def gemm_nt_r32(A, Bm, flags=0, bias=None, resid=None, aux_in=None, alpha=1.0, C0=None, rows=None, keep_mask=None,
                drop_p=0.0):
    """The emulation r32: the same operation in torch float32 on the CPU, then torch's own rounding to the output type
    (and to bf16 for the stored aux)."""
    v, aux = _nt(A, Bm, flags, bias, resid, aux_in, alpha, C0, rows, keep_mask, drop_p, torch.float32)
    dtype = OUT_DTYPE[flags & 3]
    v = v.clamp(-65504.0, 65504.0) if dtype == torch.float16 else v
    return v.to(dtype), None if aux is None else aux.to(torch.bfloat16)


def gemm_nt_S(A, Bm, flags=0, bias=None, resid=None, aux_in=None, alpha=1.0, C0=None, rows=None, drop_p=0.0, prod_abs=None):
    """S of check_bound: the operation on absolute values (a GELU passes |x| on: |gelu(x)| <= |x|, slope <= 1.13)."""
    rows = A.shape[0] if rows is None else rows
    out, epi = flags & 3, flags & ~3
    s = (A[:rows].double().abs() @ Bm.double().abs().t() if prod_abs is None else prod_abs[:rows]) * abs(alpha)
    if out == ATOMIC:
        return s + C0[:rows].double().abs()
    if epi & B:
        s = s + bias.double().abs()
    if epi & G:
        s = s * 1.13
    if epi & GB:
        u = aux_in[:rows].double()
        s = s * (u.abs() if epi & AG else _gelu_grad(u).abs())
    if epi & D:
        s = s * drop_scale(drop_p)
    if epi & R:
        s = s + resid[:rows].double().abs()
    return s


def _tn(dY, X, k, alpha, C0, b0, dt):
    k = dY.shape[0] if k is None else k
    a = torch.tensor(alpha, dtype=dt)
    dW = a * (dY[:k].to(dt).t() @ X[:k].to(dt))
    db = a * dY[:k].to(dt).sum(0)
    return (dW if C0 is None else C0.to(dt) + dW), (db if b0 is None else b0.to(dt) + db)


def gemm_tn_ref(dY, X, k=None, alpha=1.0, C0=None, b0=None):
    """float64: dW = C0 + alpha * dY[:k]^T X[:k], db = b0 + alpha * colsum(dY[:k])."""
    return _tn(dY, X, k, alpha, C0, b0, torch.float64)


def gemm_tn_r32(dY, X, k=None, alpha=1.0, C0=None, b0=None):
    return _tn(dY, X, k, alpha, C0, b0, torch.float32)


# ----------------------------------------------------------------------------------------------------- rounding helpers
def _f32_exact(x64):
    x32 = x64.to(torch.float32)
    assert torch.equal(x32.double(), x64.double()), "the value is not an fp32 number: the case's data is not exact"
    return x32


def rne_bf16(x64):
    """Round-to-nearest-even to bf16 of an fp32-exact float64 value, by torch's own conversion."""
    return _f32_exact(x64).to(torch.bfloat16)


def rne_f16_sat(x64):
    """... to IEEE fp16, saturated at +-65504 (to_f16_sat of common.h)."""
    return _f32_exact(x64).clamp(-65504.0, 65504.0).to(torch.float16)


def round_exact(x64, dtype):
    return {torch.bfloat16: rne_bf16, torch.float16: rne_f16_sat, torch.float32: _f32_exact}[dtype](x64)


_FORMAT = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}   # significant bits, smallest normal exponent


def half_ulp(r, dtype, a=0.0):
    """Half a unit in the last place of `dtype` at |r| (float64 tensor); within `a` of a power of two the larger binade's.
    0 for fp32."""
    r = r.double()
    if dtype == torch.float32:
        return torch.zeros_like(r)
    bits, emin = _FORMAT[dtype]
    mag = r.abs() + a
    _, e = torch.frexp(mag)                                   # mag = m * 2^e with m in [0.5, 1): floor(log2 mag) = e - 1
    e = torch.where(mag > 0, e - 1, torch.full_like(e, emin)).clamp(min=emin)
    return torch.ldexp(torch.ones_like(r), e - bits)          # ulp = 2^(e - bits + 1)


# --------------------------------------------------------------------------------------------------------------- checks
def check_exact(name, got, expect):
    """torch.equal on the whole buffer (sentinels included); on failure the count and the first few (m, n, got, expect)."""
    got, expect = got.detach().cpu(), expect.detach().cpu()
    assert got.dtype == expect.dtype and got.shape == expect.shape, (name, got.dtype, expect.dtype, got.shape, expect.shape)
    if torch.equal(got, expect):
        return
    g2 = got.reshape(got.shape[0], -1) if got.dim() > 1 else got.reshape(1, -1)
    e2 = expect.reshape(g2.shape)
    bad = (g2 != e2) | (torch.isnan(g2) != torch.isnan(e2))
    idx = bad.nonzero()[:8]
    first = [(int(m), int(n), float(g2[m, n]), float(e2[m, n])) for m, n in idx]
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first (m, n, got, expect): {first}")


def bound_a(S, K, adds, a_extra=0.0):
    return (K + adds) * 2.0 ** -23 * S.double() + a_extra


def check_bound(name, got, r64, S, K, adds, out_dtype, a_extra=0.0):
    """|got - r| <= half_ulp(r, out_dtype) + (K + adds) * 2^-23 * S + a_extra for every element. Prints PARITY with the
    share of A = the last two terms that is used after taking off the half ulp; returns that share."""
    got = got.detach().cpu()
    assert got.dtype == out_dtype and got.shape == r64.shape, (name, got.dtype, out_dtype, got.shape, r64.shape)
    r = r64.double()
    if out_dtype == torch.float16:
        r = r.clamp(-65504.0, 65504.0)
    g = got.double()
    assert torch.isfinite(g).all(), f"{name}: non-finite output"
    a = bound_a(S, K, adds, a_extra)
    hu = half_ulp(r, out_dtype, a)
    diff = (g - r).abs()
    over = (diff - hu).clamp(min=0)
    used = torch.where(a > 0, over / a.clamp(min=1e-300), torch.where(over > 0, torch.full_like(over, float("inf")),
                                                                      torch.zeros_like(over)))
    used_max = float(used.max()) if used.numel() else 0.0
    kind = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}[out_dtype]
    print(f"PARITY {name} [{kind}] a_extra={float(a_extra):.3e} A<={float(a.max()) if a.numel() else 0.0:.3e} "
          f"max_err={float(diff.max()) if diff.numel() else 0.0:.3e} used={used_max:.3f}")
    bad = diff > hu + a
    if bad.any():
        idx = bad.reshape(bad.shape[0], -1).nonzero()[:8]
        g2, r2, b2 = g.reshape(bad.shape[0], -1), r.reshape(bad.shape[0], -1), (hu + a).reshape(bad.shape[0], -1)
        first = [(int(m), int(n), float(g2[m, n]), float(r2[m, n]), float(b2[m, n])) for m, n in idx]
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound; "
                             f"first (m, n, got, r, bound): {first}")
    return used_max


def a_extra_of(r32_value, r64_value):
    """The transcendental term: parity_util.tol_a (8 x the error of torch's float32 epilogue, floored) on this case's values."""
    return tol_a(r32_value, r64_value)[1]


# --------------------------------------------------------------------------------------------- operands of an NT case
@functools.lru_cache(maxsize=64)
def nt_operands(M, N, K, kind):
    """CPU operands of one NT case, made once and never changed. kind: 'ints' (lim 8: the exact bf16 / fp32 cases),
    'ints16' (lim 16: the exact fp16 case, with one planted row that saturates both ways), 'gelu' (lim 8 scaled by 2^-3 /
    2^-4: pre-activations over about [-6, 6] in steps of 1/128 + quarters, still exact), 'randn' (A ~ N(0, 1),
    B ~ N(0, 0.05)), 'rows' (the same with the rows of A scaled by 2^-10 ... 2^10)."""
    seed = 1000003 * M + 1009 * N + K
    if kind in ("ints", "ints16", "gelu"):
        lim = 16 if kind == "ints16" else 8
        sa, sb = (2.0 ** -3, 2.0 ** -4) if kind == "gelu" else (1.0, 1.0)
        A, Bm = ints((M, K), lim, seed, sa), ints((N, K), lim, seed + 1, sb)
        if kind == "ints16":
            A[M // 2] = 16.0
            Bm[0] = 16.0
            Bm[1] = -16.0
    else:
        A, Bm = randn((M, K), seed, dtype=torch.bfloat16), randn((N, K), seed + 1, 0.05, dtype=torch.bfloat16)
        if kind == "rows":
            scale = torch.ldexp(torch.ones(M), (torch.arange(M) % 21) - 10).unsqueeze(1)
            A = (A.float() * scale).to(torch.bfloat16)
    bias = quarters(N, seed + 2)
    resid = ints((M, N), 4, seed + 4)
    u = sixteenths((M, N), seed + 5)
    C0 = ints((M, N), 8, seed + 6).float()
    return A, Bm, bias, resid, u, C0


@functools.lru_cache(maxsize=64)
def nt_products(M, N, K, kind):
    """float64 A @ B^T and |A| @ |B|^T of nt_operands(M, N, K, kind): computed once, shared by the cases on those operands."""
    A, Bm, *_ = nt_operands(M, N, K, kind)
    return A.double() @ Bm.double().t(), A.double().abs() @ Bm.double().abs().t()
