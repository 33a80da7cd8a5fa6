"""GPU parity of the fused attention kernels (stonk_attention_fwd / _bwd / _bwd_phases) against a float64 reference, element
by element: out, lse, dQ, dK and dV of every case of tests/attention_ref.py - padded with and without a mask, both branches of
the workgroup order, skipped key tiles up to and beyond 1024 keys, the packed layout with ragged lengths, masked rows and
query limits, sequences with no unmasked key - with the dropout mask taken from oracle/dropout_oracle.py, and the forward's
own mask recovered bit for bit. Reference, bounds and cases: tests/attention_ref.py (its CPU self-check:
test_attention_ref_cpu.py); figures of one run: profiles/attention_parity.md."""
import numpy as np
import pytest
import torch

from oracle import dropout_oracle as do
from tests import attention_ref as ar

pytestmark = pytest.mark.gpu


_RESULTS = {}   # one launch sequence per case, shared by the tests that look at it


def _args(hip, c, qkv, mask, cu, qo):
    H = c["NH"] * 64
    return (hip.ptr(qkv), hip.ptr(qkv) + 2 * H, hip.ptr(qkv) + 4 * H, 3 * H, hip.ptr(mask), hip.ptr(cu), hip.ptr(qo))


def _run(hip, name):
    """Forward, backward as one call, backward in phases (bitwise the single call's): the outputs on the CPU."""
    if name in _RESULTS:
        return _RESULTS[name]
    c = ar.CASES[name]
    B, NH, S, T = c["B"], c["NH"], c["S"], c["T"]
    H = NH * 64
    qkv, dout = (t.cuda() for t in ar.inputs(name))
    mask = None if c["mask"] is None else c["mask"].cuda()
    cu, qo = (None if t is None else t.cuda() for t in ar.offsets(c))
    out = torch.full((T, H), ar.OUT_SENTINEL, device="cuda", dtype=torch.bfloat16)
    lse = torch.full((B, NH, S), float("nan"), device="cuda")
    tail = (B, NH, S, 64, c["scale"], c["p"], c["seed"], hip.stream_ptr())
    hip.call("stonk_attention_fwd", *_args(hip, c, qkv, mask, cu, qo), hip.ptr(out), H, hip.ptr(lse), *tail)

    def bwd(entry, *phases):
        dqkv = torch.zeros_like(qkv)
        delta = torch.full((B, NH, S), float("nan"), device="cuda")
        for ph in phases or (None,):
            hip.call(entry, *(() if ph is None else (ph,)), *_args(hip, c, qkv, mask, cu, qo), hip.ptr(out), H, hip.ptr(dout), H,
                     hip.ptr(lse), hip.ptr(delta), hip.ptr(dqkv), hip.ptr(dqkv) + 2 * H, 3 * H, hip.ptr(dqkv) + 4 * H, *tail)
        return dqkv

    dqkv = bwd("stonk_attention_bwd")
    phased = bwd("stonk_attention_bwd_phases", hip.ATTN_BWD_DELTA, hip.ATTN_BWD_DKV, hip.ATTN_BWD_DQ)
    torch.cuda.synchronize()
    got = dict(out=out.cpu(), lse=lse.cpu(), dqkv=dqkv.cpu())
    # elements of dq, dk, dv at which the phases differ from the single call (as bit patterns: a NaN is unequal to itself)
    differ = (phased.cpu().view(torch.int16) != got["dqkv"].view(torch.int16)).view(T, 3, H)
    got["phases_differ"] = tuple(int(differ[:, i].sum()) for i in range(3))
    print(f"PHASES attn.{name} elements that differ from the single call: dq, dk, dv = {got['phases_differ']}")
    _RESULTS[name] = got
    return got


@pytest.mark.parametrize("name", list(ar.CASES))
def test_attention_against_float64(hip, name):
    got = _run(hip, name)
    ar.check_case(name, got)
    assert got["phases_differ"] == (0, 0, 0), f"{name}: dq, dk, dv of the phases differ from the single call's at {got['phases_differ']} elements"


@pytest.mark.parametrize("name", ["exact-pad-p0.25", "exact-packed-p0.25"])
def test_forward_mask_is_the_oracles_bit_for_bit(hip, name):
    """64 live keys per sequence with one-hot V rows: out[q][j] = P[q][key_j] keep[q][key_j] / (1-p), P > 0, so the zeros of
    `out` ARE the forward's dropped elements. They must be keep_block's - what ties the numpy oracle to csrc/common.h (the
    backward kernels are tied to it by test_attention_against_float64, whose reference uses the oracle's mask)."""
    c = ar.CASES[name]
    out = _run(hip, name)["out"].float()
    total = 0
    for b, lo, n, nq in ar.sequences(c):
        keys = np.array(c["onehot"][b])
        for h in range(c["NH"]):
            kept = out[lo:lo + nq, h * 64:h * 64 + 64] != 0
            want = do.keep_block((b * c["NH"] + h) * c["S"] + np.arange(nq), keys, c["seed"], c["p"])
            assert np.array_equal(kept.numpy(), want), (name, b, h, int((kept.numpy() != want).sum()))
            total += want.size
    assert total >= 64 * 64
