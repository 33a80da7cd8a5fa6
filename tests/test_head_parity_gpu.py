"""fp64 parity of the small head and loss launchers of csrc/small.hip and csrc/loss.hip (and stonk_scale_f32), at the
sizes where each takes another path: a second block, a grid-stride trip, the untiled weight gradient, a second sweep of a
logit row, a row count above the grid, nothing labelled, null outputs, error bits. Tolerances: tests/parity_util.py."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dropout_oracle as do
from tests.parity_util import check_bf16, check_f32, gen as _gen, leaf as _leaf, randn as _randn

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


# ---- stonk_elementwise_loss_fwd_bwd ----------------------------------------------------------------------------------

def _loss_ref(mode, x, y, dtype, gscale):
    x = _leaf(x, dtype)
    y = y.to(dtype)
    if mode == "bce":
        loss = torch.nn.BCEWithLogitsLoss()(x, y)
    elif mode == "mse":
        loss = torch.nn.MSELoss()(x, y)
    else:   # what the reference model computes for num_labels = 1 and 1-D labels: [B, 1] against [B] broadcasts to [B, B]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = torch.nn.MSELoss()(x, y.reshape(-1))
    (loss * gscale).backward()
    return loss.detach().reshape(1), x.grad


@pytest.mark.parametrize("B,C", [(1, 1), (5, 1), (255, 1), (257, 1), (300, 3), (64, 7)])
@pytest.mark.parametrize("mode,centre", [("mse", 0.0), ("mse", 50.0), ("broadcast", 0.0), ("broadcast", 50.0),
                                         ("bce", 0.0), ("bce", 25.0)])
def test_elementwise_loss_fp64(hip, mode, B, C, centre):
    """centre 50, spread 0.1: the broadcast form in its expanded shape x^2 - 2 x mean(y) + mean(y^2) was off by 2e-2 of the
    loss there in fp32, and a mean of y that is merely rounded to fp32 still costs 6e-6 of it and 2e-5 of the gradient.
    BCE logits stay within +-30: spread 10 about 0 (clamped, both ends present), and spread 0.1 about 25, where the loss is
    x (1 - y) + log1p(exp(-x)) with a second term of 1e-11."""
    code = {"mse": hip.LOSS_MSE, "broadcast": hip.LOSS_MSE_BROADCAST, "bce": hip.LOSS_BCE}[mode]
    if centre == 0.0:
        x = _randn((B, C), 60, 10.0 if mode == "bce" else 1.0)
        y = _randn((B, C), 61)
    else:
        x = _randn((B, C), 60, 0.1, centre)
        y = _randn((B, C), 61, 0.1, centre)
    if mode == "bce":
        if centre == 0.0:
            x = x.clamp(-30.0, 30.0)
            x.view(-1)[0] = 30.0
            x.view(-1)[-1] = -30.0
        assert float(x.abs().max()) <= 30.0
        y = torch.rand((B, C), generator=_gen(62))
    xd, yd = x.cuda(), y.cuda()

    def run(gscale, with_grad):
        loss = torch.full((1,), 7.0, device="cuda")
        dx = torch.full((B, C), 7.0, device="cuda") if with_grad else None
        hip.call("stonk_elementwise_loss_fwd_bwd", hip.ptr(xd), hip.ptr(yd), B, C, code, hip.ptr(loss), hip.ptr(dx), gscale,
                 hip.stream_ptr())
        torch.cuda.synchronize()
        return loss, dx

    if mode == "broadcast" and C > 1:
        with pytest.raises(hip.StonkHipError, match="-1"):
            run(1.0, True)
        return
    tag = f"loss[{mode},{B}x{C},c={centre:g}]"
    for gscale in (1.0, 0.25):
        l64, g64 = _loss_ref(mode, x, y, torch.float64, gscale)
        l32, g32 = _loss_ref(mode, x, y, torch.float32, gscale)
        loss, dx = run(gscale, True)
        check_f32(f"{tag}.loss", loss, l64, l32)
        check_f32(f"{tag}.dlogits.g{gscale:g}", dx, g64, g32)
    loss0, _ = run(1.0, False)
    assert torch.equal(loss0, loss)


# ---- stonk_dropout_f32, stonk_gelu_bwd_bf16, stonk_scale_f32, stonk_ratio_f32 ----------------------------------------

@pytest.mark.parametrize("n", [1, 255, 262147])
def test_dropout_f32_exact_mask(hip, n):
    """n = 262 147: three elements past one trip of the 1024-workgroup grid."""
    x = _randn((n,), 70)
    x[x == 0] = 1.0
    xd = x.cuda()

    def run(p, seed, src=None):
        src = xd if src is None else src
        y = torch.full((n + 1,), 7.0, device="cuda")
        hip.call("stonk_dropout_f32", hip.ptr(src), hip.ptr(y), n, p, seed, hip.stream_ptr())
        torch.cuda.synchronize()
        assert y[n].item() == 7.0
        return y[:n]

    assert torch.equal(run(0.0, 3), xd)                               # p = 0: the identity, bit for bit
    for p in (0.1, 0.5):
        keep = torch.from_numpy(do.keep_flat(n, 21, p))
        y = run(p, 21)
        assert torch.equal(run(p, 21), y)                             # same seed, same mask
        assert (y.cpu()[~keep] == 0).all() and (y.cpu()[keep] != 0).all()
        q = float(np.float32(p))
        check_f32(f"dropout_f32[n={n},p={p}]", y, torch.where(keep, x.double() / (1.0 - q), torch.zeros((), dtype=torch.float64)),
                  torch.where(keep, x / torch.tensor(1.0 - np.float32(p)), torch.zeros(())))
        inplace = xd.clone()                                          # x == y, as the engine calls it
        hip.call("stonk_dropout_f32", hip.ptr(inplace), hip.ptr(inplace), n, p, 21, hip.stream_ptr())
        assert torch.equal(inplace, y)


@pytest.mark.parametrize("n", [8, 8 * (4096 * 256) + 8])
def test_gelu_bwd_fp64(hip, n):
    """The larger size is one 16-byte piece past a full trip of the 4096-workgroup grid."""
    u = ((torch.rand(n, generator=_gen(71)) * 16.0) - 8.0).to(BF)
    u[0], u[1], u[2], u[-1] = 0.0, 8.0, -8.0, 0.0
    dg = _randn((n,), 72, 1.0, 0.0, BF)

    def ref(dtype):
        uu = _leaf(u, dtype)
        F.gelu(uu).backward(dg.to(dtype))      # the exact (erf) GELU
        return uu.grad

    ud, dgd = u.cuda(), dg.cuda()
    du = torch.full((n + 8,), 7.0, device="cuda", dtype=BF)
    hip.call("stonk_gelu_bwd_bf16", hip.ptr(dgd), hip.ptr(ud), hip.ptr(du), n, hip.stream_ptr())
    torch.cuda.synchronize()
    assert (du[n:] == 7.0).all()
    check_bf16(f"gelu_bwd[n={n}]", du[:n], ref(torch.float64), ref(torch.float32))


@pytest.mark.parametrize("n", [1, 1000003])
def test_scale_f32_bitwise(hip, n):
    x = _randn((n,), 73, 3.0)
    s = 0.3
    xd = torch.cat([x, torch.full((1,), 7.0)]).cuda()
    hip.call("stonk_scale_f32", hip.ptr(xd), n, s, hip.stream_ptr())
    assert torch.equal(xd[:n].cpu(), x * torch.tensor(np.float32(s))) and xd[n].item() == 7.0


def test_ratio_f32_within_one_ulp(hip):
    num = torch.tensor([1.0, 10.0, 354.75, -7.3, 1e-30, 3e20, 0.0, 5.0], dtype=torch.float32)
    den = torch.tensor([3.0, 4.0, 37.0, 2100.0, 7.0, 1e-10, 9.0, 1.0], dtype=torch.float32)
    nd, dd = num.cuda(), den.cuda()
    out = torch.full((num.numel(),), 7.0, device="cuda")
    for i in range(num.numel()):
        hip.call("stonk_ratio_f32", nd[i:].data_ptr(), dd[i:].data_ptr(), out[i:].data_ptr(), hip.stream_ptr())
    want = (num / den).numpy()
    got = out.cpu().numpy()
    ulp = np.spacing(np.abs(want))
    print("PARITY ratio_f32 [ulp] max_err_ulp=%.2f" % float(np.max(np.abs(got.astype(np.float64) - want) / ulp)))
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp), (got, want)


# ---- stonk_scatter_rows_f32_to_bf16 ----------------------------------------------------------------------------------

def test_scatter_rows_f32_to_bf16_bitwise(hip):
    n_src, cols, ld_src, n_dst, ld_dst, count = 40, 72, 84, 100, 80, 23
    src = _randn((n_src, ld_src), 74, 2.0)
    rows = torch.randperm(n_dst, generator=_gen(75))[:n_src].to(torch.int32)   # a longer list than the device count
    dst = torch.full((n_dst, ld_dst), 7.0, dtype=BF)
    want = dst.clone()
    want[rows[:count].long(), :cols] = src[:count, :cols].to(BF)
    dst_d, cnt = dst.cuda(), torch.tensor([count], dtype=torch.int32).cuda()
    src_d, rows_d = src.cuda(), rows.cuda()
    hip.call("stonk_scatter_rows_f32_to_bf16", hip.ptr(src_d), ld_src, hip.ptr(rows_d), hip.ptr(cnt), hip.ptr(dst_d), ld_dst,
             cols, hip.stream_ptr())
    assert torch.equal(dst_d.cpu().view(torch.int16), want.view(torch.int16))   # rows not named and columns >= cols untouched
    cnt.zero_()
    dst_d = dst.cuda()
    hip.call("stonk_scatter_rows_f32_to_bf16", hip.ptr(src_d), ld_src, hip.ptr(rows_d), hip.ptr(cnt), hip.ptr(dst_d), ld_dst,
             cols, hip.stream_ptr())
    assert torch.equal(dst_d.cpu(), dst)


# ---- stonk_small_linear_fwd / bwd ------------------------------------------------------------------------------------

@pytest.mark.parametrize("tanh", [False, True])
@pytest.mark.parametrize("xf32", [False, True])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (64, 9, 300), (6, 8, 256), (1536, 9, 100), (1537, 9, 100)])
def test_small_linear_fp64(hip, M, N, K, xf32, tanh):
    """M = 1536 is the most the tiled weight-gradient kernel takes (8 M floats in 48 KiB of LDS); at M = 1537 the untiled
    kernel runs. Both sum their rows 64 at a time: one running fp32 sum missed in db at these sizes."""
    ldx, ld_dxb = K + 8, K + 5
    x = _randn((M, ldx), 80, 1.0, 0.0, torch.float32 if xf32 else BF)
    W, b = _randn((N, K), 81, 1.0 / K ** 0.5), _randn((N,), 82, 0.3)
    dy = _randn((M, N), 83)
    dW0, db0 = _randn((N, K), 84, 2.0), _randn((N,), 85, 2.0)
    dxb0 = _randn((M, ld_dxb), 86, 1.0, 0.0, BF)
    act = (hip.SMALL_TANH if tanh else 0) | (hip.SMALL_X_F32 if xf32 else 0)
    tag = f"small_linear[{M}x{N}x{K},{'f32' if xf32 else 'bf16'},{'tanh' if tanh else 'id'}]"

    def ref(dtype, bias=True):
        xx, WW, bb = _leaf(x[:, :K], dtype), _leaf(W, dtype), _leaf(b, dtype)
        y = F.linear(xx, WW, bb if bias else None)
        if tanh:
            y = torch.tanh(y)
        y.backward(dy.to(dtype))
        return dict(y=y.detach(), dx=xx.grad, dW=dW0.to(dtype) + WW.grad, db=db0.to(dtype) + (bb.grad if bias else 0),
                    dxb=dxb0[:, :K].to(dtype) + xx.grad)

    xd, Wd, bd, dyd = x.cuda(), W.cuda(), b.cuda(), dy.cuda()

    def fwd(bias):
        y = torch.full((M * N + 1,), 7.0, device="cuda")
        hip.call("stonk_small_linear_fwd", hip.ptr(xd), ldx, hip.ptr(Wd), hip.ptr(bd if bias else None), hip.ptr(y), M, N, K, act,
                 hip.stream_ptr())
        torch.cuda.synchronize()
        assert y[M * N].item() == 7.0
        return y[: M * N].view(M, N)

    def bwd(y, with_db, f32_out, bf16_out):
        dW, db = dW0.cuda(), db0.cuda()
        dx = torch.full((M, K), 7.0, device="cuda") if f32_out else None
        dxb = dxb0.cuda() if bf16_out else None
        hip.call("stonk_small_linear_bwd", hip.ptr(dyd), hip.ptr(y), hip.ptr(xd), ldx, hip.ptr(Wd), hip.ptr(dW),
                 hip.ptr(db if with_db else None), hip.ptr(dx), hip.ptr(dxb), ld_dxb, M, N, K, act, hip.stream_ptr())
        torch.cuda.synchronize()
        return dW, db, dx, dxb

    r64, r32 = ref(torch.float64), ref(torch.float32)
    y = fwd(True)
    check_f32(f"{tag}.y", y, r64["y"], r32["y"])
    check_f32(f"{tag}.y.nobias", fwd(False), ref(torch.float64, False)["y"], ref(torch.float32, False)["y"])
    dW, db, dx, dxb = bwd(y, True, True, True)
    check_f32(f"{tag}.dW", dW, r64["dW"], r32["dW"])
    check_f32(f"{tag}.db", db, r64["db"], r32["db"])
    check_f32(f"{tag}.dx_f32", dx, r64["dx"], r32["dx"])
    check_bf16(f"{tag}.dx_bf16", dxb[:, :K], r64["dxb"], r32["dxb"])
    assert torch.equal(dxb[:, K:].cpu(), dxb0[:, K:])                       # the row stride's slack is not touched
    # null db, and neither input gradient: dW alone, the same numbers
    dW2, db2, _, _ = bwd(y, False, False, False)
    check_f32(f"{tag}.dW.nodb", dW2, r64["dW"], r32["dW"])
    assert torch.equal(db2.cpu(), db0)


# ---- stonk_nsp_xent_fwd_bwd ------------------------------------------------------------------------------------------

def _nsp_run(hip, logits, labels, gscale=1.0, with_grad=True):
    B, C = logits.shape
    ld, lb = logits.cuda(), labels.cuda()
    acc = torch.zeros(2, device="cuda")
    dl = torch.full((B * C + 1,), 7.0, device="cuda") if with_grad else None
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    hip.call("stonk_nsp_xent_fwd_bwd", hip.ptr(ld), hip.ptr(lb), B, C, hip.ptr(acc), hip.ptr(dl), gscale, hip.ptr(err),
             hip.stream_ptr())
    torch.cuda.synchronize()
    if with_grad:
        assert dl[B * C].item() == 7.0
        dl = dl[: B * C].view(B, C)
    return acc, dl, err.item()


@pytest.mark.parametrize("B,C", [(1, 2), (300, 2), (64, 5), (9, 64)])
def test_nsp_xent_fp64(hip, B, C):
    logits = _randn((B, C), 90, 3.0)
    labels = torch.randint(0, C, (B,), generator=_gen(91))
    tag = f"nsp[{B}x{C}]"
    gscale = 0.5
    for variant in ("all", "some_ignored"):
        lab = labels.clone()
        if variant == "some_ignored":
            if B == 1:
                continue
            lab[torch.rand(B, generator=_gen(92)) < 0.4] = -100
            lab[0], lab[B - 1] = -100, labels[B - 1]
        n = int((lab != -100).sum())

        def ref(dtype):
            x = _leaf(logits, dtype)
            s = F.cross_entropy(x, lab, reduction="sum", ignore_index=-100)
            (s * (gscale / n)).backward()
            return s.detach().reshape(1), x.grad

        (s64, g64), (s32, g32) = ref(torch.float64), ref(torch.float32)
        acc, dl, err = _nsp_run(hip, logits, lab, gscale)
        assert err == 0 and acc[1].item() == n
        check_f32(f"{tag}.{variant}.sum", acc[:1], s64, s32)
        check_f32(f"{tag}.{variant}.dlogits", dl, g64, g32)
        assert (dl[(lab == -100).cuda()] == 0).all()
        acc2, _, _ = _nsp_run(hip, logits, lab, gscale, with_grad=False)
        check_f32(f"{tag}.{variant}.sum.nograd", acc2[:1], s64, s32)
    # nothing labelled: sum 0, count 0, a zero gradient (not 0 / 0)
    acc, dl, err = _nsp_run(hip, logits, torch.full((B,), -100, dtype=torch.long))
    assert err == 0 and acc[0].item() == 0 and acc[1].item() == 0 and (dl == 0).all()
    for bad in (C, -1):
        lab = labels.clone()
        lab[B // 2] = bad
        assert _nsp_run(hip, logits, lab)[2] == 16


# ---- stonk_softmax_xent_fwd_bwd / stonk_softmax_xent_f16_fwd_bwd -----------------------------------------------------

XENT_CASES = [(n, c) for n in (1, 7, 8, 9, 2047, 8200) for c in (0, 1, 37)] + [(9, 2100)]


def _xent_run(hip, f16, logits, ncols, npad, tg, count, cap, gscale, with_grad=True):
    ld_d = npad + 8
    lg = (logits.half() if f16 else logits).cuda()
    tgd = tg.to(torch.int32).cuda()
    cnt = torch.tensor([count], dtype=torch.int32).cuda()
    loss = torch.zeros(1, device="cuda")
    dl = torch.full((cap + 1, ld_d), 7.0, device="cuda", dtype=BF) if with_grad else None
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    hip.call("stonk_softmax_xent_f16_fwd_bwd" if f16 else "stonk_softmax_xent_fwd_bwd", hip.ptr(lg), logits.shape[1], ncols,
             npad, hip.ptr(tgd), hip.ptr(cnt), hip.ptr(loss), hip.ptr(dl), ld_d, gscale, cap, hip.ptr(err), hip.stream_ptr())
    torch.cuda.synchronize()
    return loss, dl, err.item()


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("ncols,count", XENT_CASES)
def test_softmax_xent_fp64(hip, ncols, count, f16):
    """8200 columns: 1025 pieces, a second trip of the four-pieces-per-thread sweep; 2100 rows: more than the 2048
    workgroups; count 0: nothing is written at all.

    The loss sum is compared at every count: it is built in a fixed order (workgroup shares, then one sum in double), so
    2100 rows are as close to float64 as 37 - one fp32 atomicAdd per row was off by up to 1.4e-2 in a sum of 10 608 there."""
    npad = (ncols + 127) // 128 * 128
    cap = (count + 63) // 64 * 64 + 66
    ld = npad + 8
    logits = torch.full((cap, ld), 1e4)                    # what lies past ncols must not be read into the result
    logits[:, :ncols] = _randn((cap, ncols), 100, 3.0)
    tg = torch.randint(0, ncols, (cap,), generator=_gen(101))
    if ncols >= 2 and count >= 1:   # the row's maximum, +80, in the last piece, everything else -80
        logits[0, :ncols] = -80.0
        logits[0, ncols - 1] = 80.0
        tg[0] = 0
    src = logits.half().float() if f16 else logits
    tag = f"xent[{'f16' if f16 else 'f32'},{ncols}cols,{count}rows]"
    gscale = -0.5
    loss, dl, err = _xent_run(hip, f16, logits, ncols, npad, tg, count, cap, gscale)
    assert err == 0
    lim = (count + 63) // 64 * 64
    assert (dl[lim:] == 7.0).all(), "a row past roundup64(count) was written"
    assert (dl[:, npad:] == 7.0).all(), "a column past npad was written"
    assert (dl[count:lim, :npad] == 0).all(), "pad rows [count, roundup64) must be zero"
    if count == 0:
        assert loss.item() == 0
        return

    def ref(dtype):
        x = _leaf(src[:count, :ncols], dtype)
        s = F.cross_entropy(x, tg[:count], reduction="sum")
        (s * (gscale / count)).backward()
        return s.detach().reshape(1), x.grad

    (s64, g64), (s32, g32) = ref(torch.float64), ref(torch.float32)
    check_f32(f"{tag}.sum", loss, s64, s32)
    check_bf16(f"{tag}.dlogits", dl[:count, :ncols], g64, g32)
    assert (dl[:count, ncols:npad] == 0).all(), "columns [ncols, npad) must be zero"
    loss2, _, err = _xent_run(hip, f16, logits, ncols, npad, tg, count, cap, gscale, with_grad=False)
    assert err == 0
    check_f32(f"{tag}.sum.nograd", loss2, s64, s32)
    assert torch.equal(loss2, loss)                         # a fixed order of summation: the same bits on every launch
    for bad in (ncols, -1):
        t2 = tg.clone()
        t2[count - 1] = bad
        assert _xent_run(hip, f16, logits, ncols, npad, t2, count, cap, gscale)[2] == 8
        t2 = tg.clone()
        t2[count] = bad                                     # past the count: not a labelled row, not an error
        assert _xent_run(hip, f16, logits, ncols, npad, t2, count, cap, gscale)[2] == 0
