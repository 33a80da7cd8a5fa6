"""CPU: pins tests/gemm_ref.py before any kernel is judged by it (test_gemm_parity_gpu.py). The data conditions the exact
cases rest on are asserted from the reference alone; the emulation r32 (the same operation in torch float32, then torch's
own rounding) must pass every check; eleven wrong implementations must be refused by the check their case uses."""
import math

import numpy as np
import pytest
import torch

from oracle import dropout_oracle as do
from tests import gemm_ref as gr
from tests.gemm_ref import AG, ATOMIC, B, BF16, D, F16, F32, G, GB, R, SV

M, N = 512, 768
P_CASES = [(0.5, 0), (0.1, 77), (0.0, 2 ** 32 - 1), (0.1, 0), (0.5, 77)]


def _case(K, kind="ints", m=M, n=N):
    return gr.nt_operands(m, n, K, kind)


def _bf16_stats(r):
    """Share of values not representable in bf16, share of exact ties (the 16 dropped fp32 bits are 0x8000)."""
    bits = gr._f32_exact(r).view(torch.int32) & 0xFFFF
    return float((bits != 0).float().mean()), float((bits == 0x8000).float().mean())


# ------------------------------------------------------------------------------------------------------ data conditions
@pytest.mark.parametrize("K", [128, 192, 256])
def test_reference_on_integer_data_is_integer_arithmetic(K):
    A, Bm, bias, resid, u, C0 = _case(K)
    want = A.to(torch.int64) @ Bm.to(torch.int64).t()
    r, _ = gr.gemm_nt_ref(A, Bm)
    assert torch.equal(r, want.double()) and int(want.abs().max()) < 2 ** 24
    r, _ = gr.gemm_nt_ref(A, Bm, ATOMIC, alpha=0.5, C0=C0)
    assert torch.equal(r * 2, (want + 2 * C0.to(torch.int64)).double())
    r, _ = gr.gemm_nt_ref(A, Bm, B | R, bias=bias, resid=resid)
    assert torch.equal(r * 4, (4 * want + (4 * bias).to(torch.int64) + 4 * resid.to(torch.int64)).double())
    dW, db = gr.gemm_tn_ref(A, Bm[:M], k=300, alpha=0.5, C0=C0[:K, :K], b0=bias[:K])
    want_tn = A[:300].to(torch.int64).t() @ Bm[:300].to(torch.int64)
    assert torch.equal(dW * 2, (want_tn + 2 * C0[:K, :K].to(torch.int64)).double())
    assert torch.equal(db * 4, (2 * A[:300].to(torch.int64).sum(0) + (4 * bias[:K]).to(torch.int64)).double())


@pytest.mark.parametrize("K", [128, 256])
def test_exact_bf16_cases_round_and_tie(K):
    """Without values that bf16 cannot hold and without ties, a truncating or a round-half-up store would pass."""
    A, Bm, *_ = _case(K)
    r, _ = gr.gemm_nt_ref(A, Bm)
    inexact, ties = _bf16_stats(r)
    print(f"K={K}: inexact {inexact:.3f} ties {ties:.3f} std {float(r.std()):.0f} max {float(r.abs().max()):.0f}")
    assert inexact >= 0.15 and ties >= 0.05


def test_exact_fp16_case_rounds_and_saturates():
    A, Bm, *_ = _case(768, "ints16")
    r, _ = gr.gemm_nt_ref(A, Bm)
    out = gr.rne_f16_sat(r)
    inexact = float((out.double() != r).float().mean())
    print(f"fp16 K=768: inexact {inexact:.3f} std {float(r.std()):.0f} above 2048: {float((r.abs() > 2048).float().mean()):.3f}")
    assert inexact >= 0.15
    assert float(out[M // 2, 0]) == 65504.0 and float(out[M // 2, 1]) == -65504.0 and torch.isfinite(out).all()
    assert float(r[M // 2, 0]) == 16 * 16 * 768


@pytest.mark.parametrize("p,seed", P_CASES)
@pytest.mark.parametrize("K", [128, 256])
def test_dropout_cases_show_their_mask(K, p, seed):
    """No pre-activation is zero and no kept element rounds back onto its residual: dropped <=> out == resid."""
    A, Bm, bias, resid, u, C0 = _case(K)
    keep = gr.oracle_keep(M, N, seed, p)
    pre, _ = gr.gemm_nt_ref(A, Bm, B, bias=bias)
    assert float(pre.abs().min()) >= 0.25
    out, _ = gr.gemm_nt_r32(A, Bm, B | R | D, bias=bias, resid=resid, keep_mask=keep, drop_p=p)
    assert torch.equal(out != resid, keep)
    out0, _ = gr.gemm_nt_r32(A, Bm, D | F32, keep_mask=keep, drop_p=p)        # dropout alone: zero <=> dropped or product zero
    prod, _ = gr.gemm_nt_ref(A, Bm)
    assert torch.equal(out0 != 0, keep & (prod != 0))


@pytest.mark.parametrize("p,seed", P_CASES)
def test_masks_come_from_the_oracle_at_the_binomial_rate(p, seed):
    keep = gr.oracle_keep(M, N, seed, p)
    assert torch.equal(keep, torch.from_numpy(do.keep(np.arange(M), np.arange(N), seed, p)))
    n = M * N
    rate = 1.0 - float(keep.double().mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"p={p} seed={seed}: drop rate {rate:.5f}, 5 sigma {5 * sigma:.5f}")
    assert abs(rate - p) <= 5 * sigma
    if p == 0.0:
        assert keep.all()


def test_half_ulp_and_rounding_helpers():
    r = torch.tensor([1.0, 1.5, 255.0, 256.0, 2048.0, 2049.0, 0.0, 65504.0], dtype=torch.float64)
    assert gr.half_ulp(r, torch.bfloat16).tolist()[:4] == [2.0 ** -8, 2.0 ** -8, 0.5, 1.0]
    assert gr.half_ulp(r, torch.float16).tolist()[4:6] == [1.0, 1.0]
    assert gr.half_ulp(r, torch.float32).abs().max() == 0
    assert float(gr.half_ulp(r, torch.bfloat16)[6]) == 2.0 ** -134
    # within a of a power of two: the larger binade's
    assert float(gr.half_ulp(torch.tensor([255.9], dtype=torch.float64), torch.bfloat16, a=0.2)[0]) == 1.0
    assert float(gr.half_ulp(torch.tensor([255.9], dtype=torch.float64), torch.bfloat16, a=0.05)[0]) == 0.5
    x = torch.tensor([257.0, 259.0, 1.0 + 2.0 ** -8, 70000.0, -65519.0], dtype=torch.float64)     # ties to even, both ways
    assert gr.rne_bf16(x).double().tolist()[:3] == [256.0, 260.0, 1.0]
    assert gr.rne_f16_sat(x).double().tolist()[3:] == [65504.0, -65504.0]
    with pytest.raises(AssertionError):
        gr.rne_bf16(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))


# ---------------------------------------------------------------------------------------------- the emulation must pass
EXACT_EPIS = [(BF16, 0), (BF16, B), (BF16, R), (BF16, B | R), (BF16, GB | AG), (F32, 0), (F32, B), (ATOMIC, 0), (BF16, B | R | D),
              (BF16, B | D), (F32, D), (F32, B | R | D)]


def _kw(ops, epi, out, p=0.5, seed=77, alpha=1.0):
    A, Bm, bias, resid, u, C0 = ops
    kw = dict(alpha=alpha)
    if epi & B:
        kw["bias"] = bias
    if epi & R:
        kw["resid"] = resid
    if epi & GB:
        kw["aux_in"] = u
    if epi & D:
        kw.update(keep_mask=gr.oracle_keep(A.shape[0], Bm.shape[0], seed, p), drop_p=p)
    if out == ATOMIC:
        kw["C0"] = C0
    return kw


def _skw(kw):
    return {k: v for k, v in kw.items() if k != "keep_mask"}


@pytest.mark.parametrize("out,epi", EXACT_EPIS, ids=[gr.epi_name(o, e) for o, e in EXACT_EPIS])
def test_emulation_is_exact_on_exact_data(out, epi):
    ops = _case(256)
    kw = _kw(ops, epi, out, alpha=0.5 if out == ATOMIC else 1.0)
    r, _ = gr.gemm_nt_ref(ops[0], ops[1], out | epi, **kw)
    got, _ = gr.gemm_nt_r32(ops[0], ops[1], out | epi, **kw)
    gr.check_exact(gr.epi_name(out, epi), got, gr.round_exact(r, gr.OUT_DTYPE[out]))
    S = gr.gemm_nt_S(ops[0], ops[1], out | epi, **_skw(kw))
    assert gr.check_bound(gr.epi_name(out, epi), got, r, S, 256, 2, gr.OUT_DTYPE[out]) == 0.0


def test_emulation_is_exact_on_the_fp16_case_and_the_saved_preactivation():
    A, Bm, bias, *_ = _case(768, "ints16")
    r, _ = gr.gemm_nt_ref(A, Bm, F16)
    gr.check_exact("f16", gr.gemm_nt_r32(A, Bm, F16)[0], gr.rne_f16_sat(r))
    ops = _case(128)
    r, aux = gr.gemm_nt_ref(ops[0], ops[1], B | G | SV, bias=ops[2])
    got, got_aux = gr.gemm_nt_r32(ops[0], ops[1], B | G | SV, bias=ops[2])
    gr.check_exact("saved pre-activation", got_aux, gr.rne_bf16(aux))


GELU_EPIS = [B | G, B | G | SV, B | G | SV | AG, GB, GB | AG]


@pytest.mark.parametrize("epi", GELU_EPIS, ids=[gr.epi_name(BF16, e) for e in GELU_EPIS])
def test_emulation_passes_the_bound_on_the_gelu_family(epi):
    """On the power-of-two scaled data the product is exact: a_extra (from torch's float32 epilogue) is the whole bound."""
    ops = _case(256, "gelu")
    kw = _kw(ops, epi, BF16)
    r, aux = gr.gemm_nt_ref(ops[0], ops[1], epi, **kw)
    v32, aux32 = gr._nt(ops[0], ops[1], epi, kw.get("bias"), None, kw.get("aux_in"), 1.0, None, None, None, 0.0, torch.float32)
    pre, _ = gr.gemm_nt_ref(ops[0], ops[1], B, bias=ops[2])
    print(f"pre-activations: min {float(pre.min()):.2f} max {float(pre.max()):.2f} std {float(pre.std()):.2f}")
    assert 2 < float(pre.std()) < 4 and float((pre.abs() <= 6).double().mean()) > 0.9
    got, got_aux = gr.gemm_nt_r32(ops[0], ops[1], epi, **kw)
    S = gr.gemm_nt_S(ops[0], ops[1], epi, **_skw(kw))
    gr.check_bound(gr.epi_name(BF16, epi), got, r, S, 256, 1, torch.bfloat16, gr.a_extra_of(v32, r))
    if epi & SV and epi & AG:
        gr.check_bound("aux", got_aux, aux, torch.zeros_like(aux), 256, 1, torch.bfloat16, gr.a_extra_of(aux32, aux))
    elif epi & SV:
        gr.check_exact("aux", got_aux, gr.rne_bf16(aux))


@pytest.mark.parametrize("kind", ["randn", "rows"])
@pytest.mark.parametrize("out,epi", [(BF16, 0), (F32, 0), (F16, 0), (BF16, B | R), (ATOMIC, 0)])
def test_emulation_passes_the_bound_on_random_data(out, epi, kind):
    ops = gr.nt_operands(257, 768, 768, kind)
    kw = _kw(ops, epi, out, alpha=0.5 if out == ATOMIC else 1.0)
    r, _ = gr.gemm_nt_ref(ops[0], ops[1], out | epi, **kw)
    got, _ = gr.gemm_nt_r32(ops[0], ops[1], out | epi, **kw)
    S = gr.gemm_nt_S(ops[0], ops[1], out | epi, **_skw(kw))
    used = gr.check_bound(f"{kind} {gr.epi_name(out, epi)}", got, r, S, 768, 2, gr.OUT_DTYPE[out])
    assert used < 0.5


def test_emulation_passes_on_the_weight_gradient():
    dY, X = gr.ints((320, 256), 8, 1), gr.ints((320, 384), 8, 2)
    C0, b0 = gr.ints((256, 384), 8, 3).float(), gr.quarters(256, 4)
    for k in (0, 1, 65, 320):
        dW, db = gr.gemm_tn_ref(dY, X, k, 0.5, C0, b0)
        dW32, db32 = gr.gemm_tn_r32(dY, X, k, 0.5, C0, b0)
        gr.check_exact("dW", dW32, gr._f32_exact(dW))
        gr.check_exact("db", db32, gr._f32_exact(db))


# ------------------------------------------------------------------------------------- wrong implementations are refused
def _truncate_bf16(x32):
    return (x32.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


def _wrong(name, ops, K, p, seed):
    """(got, expected fp64 value, flags, kwargs of S) of one wrong implementation of a case on `ops`."""
    A, Bm, bias, resid, u, C0 = ops
    m, n = A.shape[0], Bm.shape[0]
    keep = gr.oracle_keep(m, n, seed, p)
    scale = gr.drop_scale(p, torch.float32)
    brd = dict(bias=bias, resid=resid, keep_mask=keep, drop_p=p)
    if name == "bf16 truncation":
        r, _ = gr.gemm_nt_ref(A, Bm)
        return _truncate_bf16(gr._nt(A, Bm, 0, None, None, None, 1.0, None, None, None, 0.0, torch.float32)[0]), r, 0, {}
    if name == "one K tile dropped":
        r, _ = gr.gemm_nt_ref(A, Bm, B, bias=bias)
        return gr.gemm_nt_r32(A[:, 64:], Bm[:, 64:], B, bias=bias)[0], r, B, dict(bias=bias)
    if name == "one K tile added twice":
        r, _ = gr.gemm_nt_ref(A, Bm, B, bias=bias)
        A2, B2 = torch.cat([A, A[:, 64:128]], 1), torch.cat([Bm, Bm[:, 64:128]], 1)
        return gr.gemm_nt_r32(A2, B2, B, bias=bias)[0], r, B, dict(bias=bias)
    if name == "bias shifted by 4 columns":
        r, _ = gr.gemm_nt_ref(A, Bm, B, bias=bias)
        return gr.gemm_nt_r32(A, Bm, B, bias=torch.roll(bias, 4))[0], r, B, dict(bias=bias)
    if name == "residual before the dropout":
        r, _ = gr.gemm_nt_ref(A, Bm, B | R | D, **brd)
        pre = gr._nt(A, Bm, B | R, bias, resid, None, 1.0, None, None, None, 0.0, torch.float32)[0]
        return torch.where(keep, pre * scale, torch.zeros(())).to(torch.bfloat16), r, B | R | D, _skw(brd)
    if name == "alpha after the bias":
        r, _ = gr.gemm_nt_ref(A, Bm, B, bias=bias, alpha=0.5)
        pre = gr._nt(A, Bm, B, bias, None, None, 1.0, None, None, None, 0.0, torch.float32)[0]
        return (pre * 0.5).to(torch.bfloat16), r, B, dict(bias=bias, alpha=0.5)
    if name == "mask keys swapped":
        r, _ = gr.gemm_nt_ref(A, Bm, B | R | D, **brd)
        swapped = torch.from_numpy(do.keep(np.arange(n), np.arange(m), seed, p).T.copy())
        return gr.gemm_nt_r32(A, Bm, B | R | D, **{**brd, "keep_mask": swapped})[0], r, B | R | D, _skw(brd)
    if name == "mask columns permuted in a group of 8":
        r, _ = gr.gemm_nt_ref(A, Bm, B | R | D, **brd)
        perm = keep[:, torch.arange(n) ^ 1]
        return gr.gemm_nt_r32(A, Bm, B | R | D, **{**brd, "keep_mask": perm})[0], r, B | R | D, _skw(brd)
    if name == "gelu'(u) where AUX_GRAD says u":
        r, _ = gr.gemm_nt_ref(A, Bm, GB | AG, aux_in=u)
        return gr.gemm_nt_r32(A, Bm, GB, aux_in=u)[0], r, GB | AG, dict(aux_in=u)
    raise KeyError(name)


WRONG = ["bf16 truncation", "one K tile dropped", "one K tile added twice", "bias shifted by 4 columns",
         "residual before the dropout", "alpha after the bias", "mask keys swapped", "mask columns permuted in a group of 8",
         "gelu'(u) where AUX_GRAD says u"]


@pytest.mark.parametrize("name", WRONG)
def test_wrong_implementation_is_refused_on_exact_data(name):
    """p = 0.5: the whole output is exact (check_exact). p = 0.1: values by check_bound, the mask by `out != resid`."""
    ops = _case(256)
    for p, seed in ((0.5, 77), (0.1, 0)):
        got, r, flags, skw = _wrong(name, ops, 256, p, seed)
        if p == 0.5:
            with pytest.raises(AssertionError, match="differ"):
                gr.check_exact(name, got, gr.rne_bf16(r))
        S = gr.gemm_nt_S(ops[0], ops[1], flags, **skw)
        with pytest.raises(AssertionError, match="outside the bound"):
            gr.check_bound(name, got, r, S, 256, 2, torch.bfloat16)
        if name.startswith("mask"):
            assert not torch.equal(got != ops[3], gr.oracle_keep(M, N, seed, p))


@pytest.mark.parametrize("name", WRONG[:6])
def test_wrong_implementation_is_refused_on_random_data(name):
    ops = gr.nt_operands(257, 768, 768, "randn")
    got, r, flags, skw = _wrong(name, ops, 768, 0.1, 77)
    S = gr.gemm_nt_S(ops[0], ops[1], flags, **skw)
    with pytest.raises(AssertionError, match="outside the bound"):
        gr.check_bound(name, got, r, S, 768, 2, torch.bfloat16)


def _buffer(value, rows, ld, pre=2, post=2, cap=None):
    """What the GPU file builds: the expected allocation around a [rows, N] value, sentinels everywhere else."""
    cap = value.shape[0] if cap is None else cap
    buf = torch.full((pre + cap + post, ld), gr.SENTINEL, dtype=value.dtype)
    buf[pre:pre + rows, :value.shape[1]] = value[:rows]
    return buf


def test_a_row_or_a_padding_column_too_many_is_refused():
    A, Bm, *_ = _case(128)
    full = gr.rne_bf16(gr.gemm_nt_ref(A, Bm)[0])
    for m_dev in (0, 1, 255, 256, 257):
        expect = _buffer(full, m_dev, N + 8, cap=M)
        gr.check_exact("as it should be", _buffer(full, m_dev, N + 8, cap=M), expect)
        with pytest.raises(AssertionError, match="differ"):                       # row *m_dev itself written
            gr.check_exact("row m_dev written", _buffer(full, m_dev + 1, N + 8, cap=M), expect)
        got = expect.clone()
        got[2 + max(m_dev - 1, 0), N] = 3.0                                       # one padding column [N, ldc) written
        with pytest.raises(AssertionError, match="differ"):
            gr.check_exact("padding column written", got, expect)
        got = expect.clone()
        got[1, 5] = 0.0                                                           # the row before the view
        with pytest.raises(AssertionError, match="differ"):
            gr.check_exact("row before the view written", got, expect)


def test_instance_table_names_kernels_and_lines():
    seen = {(k, o, e) for k, o, e, _ in gr.INSTANCES}
    assert len(seen) == len(gr.INSTANCES)
    for k, o, e, where in gr.INSTANCES:
        assert where.split(":")[0] in ("gemm_bf16.hip", "gemm256.hip", "gemm_w4.hip", "gemm_a4.hip"), where
    assert {k for k, *_ in gr.INSTANCES} == {gr.TILE128, gr.WAVE8, gr.WAVE4, gr.WAVE4_192, gr.ASM4, gr.ASM4_192}
