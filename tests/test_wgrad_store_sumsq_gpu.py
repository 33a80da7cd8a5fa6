"""GPU: stonk_gemm_tn_bf16_store_sumsq - the stored weight gradient that also leaves, per output tile, the sum of the
squares of what it stored. dW must be stonk_gemm_tn_bf16_store's bit for bit; the slots must be the same bits on every
launch and under every CU cap (a fixed order of summation), exactly zero for an empty token count, and as close to the
fp64 sum of squares of the stored output as stonk_sumsq_f32 over that output is - the project's 4x rule: at most four
times its relative error; where that error is zero, one fp32 ulp of the sum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 192
# (M', N', ldc, split_k, split_k of the second launch): the 256x256 kernel on 2 x 2 tiles with a padded destination, under
# two CU caps; the same kernel on 17 x 1 tiles, where the cap of 16 CUs makes a grid of 16 walk 17 tiles and all CUs make
# one of 17; the 128x128 kernel on 3 x 2 tiles (it has no cap: launched twice)
SHAPES = {"256x256": (512, 512, 640, 0, -16), "256x256, tiles > grid": (4352, 256, 256, 0, -16), "128x128": (384, 256, 320, 1, 1)}


def _operands(Mo, No, count, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dY = (torch.randn((T, Mo), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    X = (torch.randn((T, No), generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    dY[count:(count + 63) // 64 * 64] = 0   # (the contract: rows from the count up to the next multiple of 64 read as zero)
    X[count:(count + 63) // 64 * 64] = 0
    return dY, X, torch.tensor([count], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("alpha", [1.0, 0.37])
@pytest.mark.parametrize("count", [192, 130, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_slots_are_the_sum_of_squares_of_the_stored_values(hip, shape, count, alpha):
    Mo, No, ldc, split, split2 = SHAPES[shape]
    tile = 256 if split <= 0 else 128
    rt, ct = (Mo + tile - 1) // tile, (No + tile - 1) // tile
    assert hip.lib().stonk_gemm_tn_store_tiles(Mo, No, T, split) == rt * ct == hip.lib().stonk_gemm_tn_store_tiles(Mo, No, T, split2)
    dY, X, cnt = _operands(Mo, No, count, seed=Mo + count)
    a = (hip.ptr(dY), Mo, hip.ptr(X), No)
    b = (0, Mo, No, T, alpha)
    ref = torch.full((Mo, ldc), 77.0, device="cuda")
    hip.call("stonk_gemm_tn_bf16_store", *a, hip.ptr(ref), ldc, *b, split, hip.ptr(cnt), hip.stream_ptr())
    runs = []
    for sk in (split, split, split2):
        dW = torch.full((Mo, ldc), 77.0, device="cuda")
        slots = torch.full((rt * ct + 3,), float("nan"), device="cuda")   # (every slot is written: nothing is zeroed for it)
        hip.call("stonk_gemm_tn_bf16_store_sumsq", *a, hip.ptr(dW), ldc, *b, sk, hip.ptr(cnt), hip.ptr(slots), rt * ct,
                 hip.stream_ptr())
        runs.append((dW, slots))
    torch.cuda.synchronize()
    for dW, slots in runs:
        assert torch.equal(dW, ref)                                   # the stored gradient, bit for bit ...
        assert (dW[:, No:] == 77.0).all()                             # ... and nothing between N' and ldc
        assert torch.isnan(slots[rt * ct:]).all() and torch.isfinite(slots[:rt * ct]).all()
        assert torch.equal(slots[:rt * ct], runs[0][1][:rt * ct])     # the same bits: second launch, other CU cap
    slots = runs[0][1][:rt * ct]
    stored = ref[:, :No].contiguous()
    if count == 0:
        assert float(stored.abs().max()) == 0.0 and float(slots.abs().max()) == 0.0
        return
    # slot by slot: row_tile * col_tiles + col_tile
    per_tile = (stored.double() ** 2).view(rt, tile, ct, tile).sum(dim=(1, 3)).reshape(-1)
    assert float(((slots.double() - per_tile).abs() / per_tile).max()) < 1e-5
    # the 4x rule against stonk_sumsq_f32 over the same output
    exact = float((stored.double() ** 2).sum())
    out = torch.zeros(1, device="cuda")
    ws = torch.zeros(int(hip.lib().stonk_sumsq_workspace_floats()), device="cuda")
    hip.call("stonk_sumsq_f32", hip.ptr(stored), stored.numel(), hip.ptr(out), hip.ptr(ws), ws.numel(), hip.stream_ptr())
    err_ref = abs(float(out.double()) - exact) / exact
    err = abs(float(slots.double().sum()) - exact) / exact
    ulp = float(np.spacing(np.float32(exact))) / exact
    print(f"{shape} count {count} alpha {alpha}: relative error of the slots' sum {err:.3e}, of stonk_sumsq_f32 {err_ref:.3e}, "
          f"one fp32 ulp {ulp:.3e}")
    assert err <= (4 * err_ref if err_ref > 0 else ulp)


def test_refusals(hip):
    """Too few slots, no slots, and every shape the store entry refuses - with its status, nothing launched."""
    lib = hip.lib()
    dY, X, cnt = _operands(768, 768, 192, seed=1)
    dW = torch.full((768, 768), 5.0, device="cuda")
    slots = torch.full((64,), 9.0, device="cuda")
    a = (hip.ptr(dY), 768, hip.ptr(X), 768, hip.ptr(dW), 768, 0, 768, 768, T, 1.0)
    st = hip.stream_ptr()
    assert lib.stonk_gemm_tn_bf16_store_sumsq(*a, 1, 0, hip.ptr(slots), 35, st) == hip.EINVAL       # 36 tiles of 128x128
    assert lib.stonk_gemm_tn_bf16_store_sumsq(*a, 0, 0, hip.ptr(slots), 8, st) == hip.EINVAL        # 9 tiles of 256x256
    assert lib.stonk_gemm_tn_bf16_store_sumsq(*a, 1, 0, 0, 64, st) == hip.EINVAL
    assert lib.stonk_gemm_tn_bf16_store_sumsq(*a, 1, 0, hip.ptr(slots), -1, st) == hip.EINVAL
    assert lib.stonk_gemm_tn_bf16_store_sumsq(*a, 1, 0, hip.ptr(slots) + 2, 64, st) == hip.EALIGN
    for split in (2, 32, -1, -2000):                                                                # as the store entry
        assert lib.stonk_gemm_tn_bf16_store_sumsq(*a, split, 0, hip.ptr(slots), 64, st) == hip.ESHAPE
        assert lib.stonk_gemm_tn_bf16_store(*a, split, 0, st) == hip.ESHAPE
        assert lib.stonk_gemm_tn_store_tiles(768, 768, T, split) == hip.ESHAPE
    K = 4096                                                                                         # (32 K tiles: 9 tiles split)
    dY2, X2 = torch.zeros((K, 768), dtype=torch.bfloat16, device="cuda"), torch.zeros((K, 768), dtype=torch.bfloat16, device="cuda")
    a2 = (hip.ptr(dY2), 768, hip.ptr(X2), 768, hip.ptr(dW), 768, 0, 768, 768, K, 1.0)
    for split in (0, -160):
        assert lib.stonk_gemm_tn_bf16_store_sumsq(*a2, split, 0, hip.ptr(slots), 64, st) == hip.ESHAPE
        assert lib.stonk_gemm_tn_store_tiles(768, 768, K, split) == hip.ESHAPE
    bad = (hip.ptr(dY), 768, hip.ptr(X), 768, hip.ptr(dW), 512, 0, 768, 768, T, 1.0)                 # ldc < N'
    assert lib.stonk_gemm_tn_bf16_store_sumsq(*bad, 1, 0, hip.ptr(slots), 64, st) == hip.ESHAPE
    db = torch.zeros(768, device="cuda")
    withb = (hip.ptr(dY), 768, hip.ptr(X), 768, hip.ptr(dW), 768, hip.ptr(db), 768, 768, T, 1.0)     # bias over 3 column tiles
    assert lib.stonk_gemm_tn_bf16_store_sumsq(*withb, 0, 0, hip.ptr(slots), 64, st) == hip.ESHAPE
    torch.cuda.synchronize()
    assert (dW == 5.0).all() and (slots == 9.0).all()
