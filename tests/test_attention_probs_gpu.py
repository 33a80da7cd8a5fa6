"""GPU parity of stonk_attention_probs (csrc/attention_probs.hip) through the C ABI: the written-out attention
probabilities and the text / entity mass per query row, against a torch fp64 softmax computed from the same bf16 qkv (the
construction of tests/test_attention_gpu.py::_ref, finfo.min on masked keys), and against the attention kernel the model
actually runs (probs @ v vs stonk_attention_fwd's context).

Tolerance on the probabilities: rtol 5e-3, atol 1e-7 against fp64 - the forward's lse is held to atol 2e-3, which
p = exp(s - lse) turns into a 2e-3 relative error; the same allowance again on the score gives 5e-3. Measured maximum
relative error on the MI355X (entries above 1e-6): see profiles/attention_maps.md."""
import pytest
import torch

from tests.test_attention_gpu import _inputs, _relerr, _run_fwd

pytestmark = pytest.mark.gpu

RTOL, ATOL = 5e-3, 1e-7
CANARY = 4096   # floats behind each output


def _ref64(qkv, mask, B, S, NH):
    x = qkv.double().view(B, S, 3, NH, 64).permute(2, 0, 3, 1, 4)   # [3,B,NH,S,64]
    s = x[0] @ x[1].transpose(-1, -2) / 8.0
    if mask is not None:
        s = s + (1.0 - mask.double())[:, None, None, :] * torch.finfo(torch.float32).min
    return torch.softmax(s, -1)


def _run(hip, qkv, mask, B, S, NH, half=None, want_p=True, want_m=True):
    """(probs [B,NH,S,S] or None, modal [B,NH,S,2] or None); the canary floats behind each output are checked here."""
    H = NH * 64
    half = S // 2 if half is None else half
    pbuf = torch.full((B * NH * S * S + CANARY,), float("nan"), device="cuda") if want_p else None
    mbuf = torch.full((B * NH * S * 2 + CANARY,), float("nan"), device="cuda") if want_m else None
    hip.call("stonk_attention_probs", hip.ptr(qkv), hip.ptr(qkv) + 2 * H, 3 * H, hip.ptr(mask), hip.ptr(pbuf), hip.ptr(mbuf),
             B, NH, S, 64, half, 0.125, hip.stream_ptr())
    torch.cuda.synchronize()
    probs = modal = None
    if want_p:
        assert bool(torch.isnan(pbuf[-CANARY:]).all()), "probs: written past the end"
        probs = pbuf[:-CANARY].view(B, NH, S, S)
    if want_m:
        assert bool(torch.isnan(mbuf[-CANARY:]).all()), "modal_mass: written past the end"
        modal = mbuf[:-CANARY].view(B, NH, S, 2)
    return probs, modal


def _max_rel(p, ref):
    big = ref > 1e-6
    return float(((p.double() - ref).abs()[big] / ref[big]).max())


@pytest.mark.parametrize("B,S,NH,masked", [(1, 128, 1, False), (2, 256, 2, True), (3, 512, 12, True), (8, 128, 3, True),
                                          (2, 384, 2, True)])
def test_probs_parity_and_structure(hip, B, S, NH, masked):
    qkv, _, mask = _inputs(B, S, NH, 11 + S, masked)
    ref = _ref64(qkv, mask, B, S, NH)
    probs, modal = _run(hip, qkv, mask, B, S, NH)
    print(f"B{B} S{S} NH{NH}: max rel err (ref > 1e-6) {_max_rel(probs, ref):.3e}, "
          f"max abs err {float((probs.double() - ref).abs().max()):.3e}")
    assert bool(torch.isfinite(probs).all())
    torch.testing.assert_close(probs.double(), ref, rtol=RTOL, atol=ATOL)
    # structure, no tolerance involved
    if masked:
        dead = (mask == 0)[:, None, None, :].expand(B, NH, S, S)
        assert float(probs[dead].abs().max()) == 0.0                       # a masked key: exactly 0.0
    assert float((probs.double().sum(-1) - 1.0).abs().max()) < 1e-5       # every row, padded queries included
    probs2, modal2 = _run(hip, qkv, mask, B, S, NH)
    assert torch.equal(probs, probs2) and torch.equal(modal, modal2)      # bitwise from run to run
    # the mass of the two key halves, from the same launch
    half = S // 2
    assert float((modal[..., 0] - probs[..., :half].sum(-1)).abs().max()) < 1e-5
    assert float((modal[..., 1] - probs[..., half:].sum(-1)).abs().max()) < 1e-5
    assert float((modal.sum(-1) - 1.0).abs().max()) < 1e-5
    # the cheap mode (no S x S stores) gives bitwise the same mass
    none, modal3 = _run(hip, qkv, mask, B, S, NH, want_p=False)
    assert none is None and torch.equal(modal, modal3)
    probs3, none = _run(hip, qkv, mask, B, S, NH, want_m=False)
    assert none is None and torch.equal(probs, probs3)


def test_all_keys_masked_attends_uniformly(hip):
    B, S, NH = 2, 256, 2
    qkv, _, _ = _inputs(B, S, NH, 77, False)
    mask = torch.ones(B, S, dtype=torch.long, device="cuda")
    mask[0, :] = 0
    mask[1, 40:100] = 0
    probs, modal = _run(hip, qkv, mask, B, S, NH)
    u = torch.tensor(1.0 / 256, dtype=torch.float32)
    ulp = float(torch.nextafter(u, torch.tensor(1.0)) - u)
    assert float((probs[0] - u.item()).abs().max()) <= ulp                 # the reference's finfo.min absorbs every score
    assert float((modal[0] - 0.5).abs().max()) < 1e-6
    ref = _ref64(qkv, mask, B, S, NH)
    torch.testing.assert_close(probs[1].double(), ref[1], rtol=RTOL, atol=ATOL)   # the other sequence is unaffected
    assert float(probs[1][..., 40:100].abs().max()) == 0.0
    alone, _ = _run(hip, qkv[S:], mask[1:], 1, S, NH)
    assert torch.equal(alone[0], probs[1])


def test_spike_rows_stay_finite_and_exact(hip):
    """One query with scaled scores of about +40 and +80 against keys of later tiles (the running maximum moves twice) and
    about -80 against another: no inf / nan, and the row still matches fp64."""
    B, S, NH = 1, 256, 1
    qkv, _, _ = _inputs(B, S, NH, 5, False)
    x = qkv.float().clone()
    q3 = x[3, 0:64]
    n2 = float(q3 @ q3)
    x[70, 64:128] = q3 * (320.0 / n2)      # raw score ~ +320, scaled ~ +40
    x[130, 64:128] = q3 * (640.0 / n2)     # ~ +80 after scaling
    x[200, 64:128] = -q3 * (640.0 / n2)    # ~ -80
    qkv = x.to(torch.bfloat16)
    ref = _ref64(qkv, None, B, S, NH)
    assert float(ref[0, 0, 3, 130]) > 0.99 and float(ref[0, 0, 3, 200]) < 1e-60
    probs, modal = _run(hip, qkv, None, B, S, NH)
    assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(modal).all())
    print(f"spike: max rel err {_max_rel(probs, ref):.3e}")
    torch.testing.assert_close(probs.double(), ref, rtol=RTOL, atol=ATOL)
    assert float((probs.double().sum(-1) - 1.0).abs().max()) < 1e-5


def test_modal_mass_with_an_uneven_split(hip):
    B, S, NH, half = 2, 256, 2, 64
    qkv, _, mask = _inputs(B, S, NH, 33, True)
    probs, modal = _run(hip, qkv, mask, B, S, NH, half=half)
    assert float((modal[..., 0] - probs[..., :half].sum(-1)).abs().max()) < 1e-5
    assert float((modal[..., 1] - probs[..., half:].sum(-1)).abs().max()) < 1e-5
    assert float((modal.sum(-1) - 1.0).abs().max()) < 1e-5
    _, alone = _run(hip, qkv, mask, B, S, NH, half=half, want_p=False)
    assert torch.equal(alone, modal)


@pytest.mark.parametrize("B,S,NH", [(3, 512, 12), (2, 256, 2)])
def test_probs_times_v_is_the_forward_kernels_context(hip, B, S, NH):
    """What ties the map to the attention the model runs: probs @ v in fp32 torch against stonk_attention_fwd's output at
    p = 0, within the forward's own bound (relative L2 < 1e-2)."""
    qkv, _, mask = _inputs(B, S, NH, 11 + S, True)
    probs, _ = _run(hip, qkv, mask, B, S, NH, want_m=False)
    out, _ = _run_fwd(hip, qkv, mask, B, S, NH)
    v = qkv.float().view(B, S, 3, NH, 64)[:, :, 2].permute(0, 2, 1, 3)     # [B,NH,S,64]
    ctx = (probs @ v).permute(0, 2, 1, 3).reshape(B * S, NH * 64)
    e = _relerr(out, ctx)
    print(f"B{B} S{S} NH{NH}: probs @ v vs forward context, relative L2 {e:.3e}")
    assert e < 1e-2, e


def test_bad_arguments_on_the_device(hip):
    qkv = torch.zeros(256, 192, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros(256 * 256, device="cuda")
    lib = hip.lib()
    args = (hip.ptr(qkv), hip.ptr(qkv) + 128, 192, 0)
    assert lib.stonk_attention_probs(*args, hip.ptr(out), 0, 0, 1, 256, 64, 128, 0.125, hip.stream_ptr()) == hip.OK   # B == 0
    assert lib.stonk_attention_probs(*args, hip.ptr(out) + 4, 0, 1, 1, 256, 64, 128, 0.125, hip.stream_ptr()) == hip.EALIGN
    assert lib.stonk_attention_probs(*args, hip.ptr(out), 0, 1, 1, 256, 64, 96, 0.125, hip.stream_ptr()) == hip.EINVAL
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
