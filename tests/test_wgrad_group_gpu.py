"""GPU: stonk_gemm_tn_bf16_group - up to four accumulating weight gradients of the four-wave kernel in one launch.

Judged by tests/gemm_ref.py: the reference is float64 dY^T X on the same bf16 operands, the per-element bound is that
file's `check_bound` (K = the live tokens; adds = the K shares that meet in an element + the add into what the buffer
held - for db every share is further split over the problem's column tiles, the kernel's bias duty). Exact data (integers,
alpha 1) must come out bit-equal to single stonk_gemm_tn_bf16 launches, whatever the split.

Shapes: problems of 1, 2 tiles of 256 x 256 in either direction; leading dimensions that differ per problem (operands are
column slices of wider buffers); T = 128 (two K tiles), 192 (three: the even rounding pads one), 448 (seven). The common
split is limited to K tiles / 8 per problem, so at those T it is 1 whatever the cap; T = 1600 (25 K tiles, shares of
10 + 10 + 6 or 14 + 12) is the smallest row count at which a cap yields splits of 2 and 3 as well."""
import functools

import pytest
import torch

from tests import gemm_ref as gr
from tests.parity_util import randn

pytestmark = pytest.mark.gpu

SENTINEL, PAD = gr.SENTINEL, gr.PAD
PRE, POST = 2, 3
# (M', N', lda, column of dY in its buffer, ldb, column of X in its buffer)
GROUP2 = ((512, 256, 768, 128, 512, 256), (256, 256, 512, 256, 768, 64))
GROUP3 = ((256, 256, 512, 0, 768, 512), (256, 512, 768, 512, 512, 0), (512, 256, 768, 64, 512, 192))


@functools.lru_cache(maxsize=None)
def _operands(T, Mo, No, exact, seed):
    if exact:
        return gr.ints((T, Mo), 8, seed), gr.ints((T, No), 8, seed + 1)
    return randn((T, Mo), seed, dtype=torch.bfloat16), randn((T, No), seed + 1, 0.05, dtype=torch.bfloat16)


def _wide(view, ld, col):
    """GPU buffer [rows + POST, ld] of PAD with `view` at column `col`; returns (buffer, the slice)."""
    rows, cols = view.shape
    assert col + cols <= ld
    buf = torch.full((rows + POST, ld), PAD, dtype=view.dtype)
    buf[:rows, col:col + cols] = view
    g = buf.cuda()
    return g, g[:rows, col:col + cols]


def _common_split(group, T, cap):
    """The documented rule (include/stonk_hip.h)."""
    tiles = sum((Mo // 256) * (No // 256) for Mo, No, *_ in group)
    return max(1, min(cap // tiles, ((T + 63) // 64) // 8))


def run_group(hip, group, T, alpha, biases, k_devs, cap, exact):
    name = f"group of {len(group)} T={T} alpha={alpha} bias={biases} k_dev={k_devs} cap={cap} {'exact' if exact else 'random'}"
    sk = _common_split(group, T, cap)
    members, singles, keep = [], [], []
    for i, (Mo, No, lda, ca, ldb, cb) in enumerate(group):
        dY, X = _operands(T, Mo, No, exact, 7919 * T + 31 * Mo + No + i)
        gY, vY = _wide(dY, lda, ca)
        gX, vX = _wide(X, ldb, cb)
        ldc = No + 64
        outs = []
        for _ in range(2):   # [0]: the grouped launch, [1]: single launches
            w = torch.full((PRE + Mo + POST, ldc), SENTINEL)
            w[PRE:PRE + Mo, :No] = 0
            b = torch.full((8 + Mo + 8,), SENTINEL)
            b[8:8 + Mo] = 0
            outs.append((w.cuda(), b.cuda()))
        cnt = None if k_devs[i] is None else torch.tensor([k_devs[i]], dtype=torch.int32, device="cuda")
        keep.append((gY, gX, cnt, dY, X, outs))
        for j, lst in enumerate((members, singles)):
            w, b = outs[j]
            lst.append((hip.ptr(vY), lda, hip.ptr(vX), ldb, hip.ptr(w[PRE:]), ldc, hip.ptr(b[8:]) if biases[i] else 0, Mo, No, T,
                        alpha, hip.ptr(cnt)))
    probs = hip.tn_problems(members)
    hip.call("stonk_gemm_tn_bf16_group", probs, len(members), cap, hip.stream_ptr())
    for m in singles:
        hip.call("stonk_gemm_tn_bf16", *m[:11], 0, m[11], hip.stream_ptr())
    torch.cuda.synchronize()
    once = [(o[0][0].cpu(), o[0][1].cpu()) for *_, o in keep]
    hip.call("stonk_gemm_tn_bf16_group", probs, len(members), cap, hip.stream_ptr())
    torch.cuda.synchronize()
    used = 0.0
    for i, (gY, gX, cnt, dY, X, outs) in enumerate(keep):
        Mo, No = group[i][:2]
        k = T if k_devs[i] is None else k_devs[i]
        (w1, b1), (ws, bs), (w2, b2) = once[i], (outs[1][0].cpu(), outs[1][1].cpu()), (outs[0][0].cpu(), outs[0][1].cpu())
        dW, db = gr.gemm_tn_ref(dY, X, k, alpha)
        Sw = abs(alpha) * (dY[:k].double().abs().t() @ X[:k].double().abs())
        Sb = abs(alpha) * dY[:k].double().abs().sum(0)
        vw = lambda t: t[PRE:PRE + Mo, :No]
        nm = f"{name} [{i}]"
        # canaries: rows before / after the extent, columns past N', and a bias that was not asked for
        for t in (w1, ws, w2):
            assert (t[:PRE] == SENTINEL).all() and (t[PRE + Mo:] == SENTINEL).all() and (t[:, No:] == SENTINEL).all(), nm
        for t in (b1, bs, b2):
            assert (t[:8] == SENTINEL).all() and (t[8 + Mo:] == SENTINEL).all(), nm
        if k == 0:
            assert float(vw(w2).abs().max()) == 0.0 and float(b2[8:8 + Mo].abs().max()) == 0.0, nm
        used = max(used, gr.check_bound(nm + " dW", vw(w1), dW, Sw, k, sk + 1, torch.float32))
        used = max(used, gr.check_bound(nm + " dW against single launches", vw(w1), vw(ws).double(), Sw, k, sk + 1, torch.float32))
        used = max(used, gr.check_bound(nm + " dW twice", vw(w2), 2 * dW, 2 * Sw, k, 2 * (sk + 1), torch.float32))
        if biases[i]:
            shares = sk * (No // 256)
            vb = lambda t: t[8:8 + Mo]
            used = max(used, gr.check_bound(nm + " db", vb(b1), db, Sb, k, shares + 1, torch.float32))
            used = max(used, gr.check_bound(nm + " db against single launches", vb(b1), vb(bs).double(), Sb, k, shares + 1,
                                            torch.float32))
            used = max(used, gr.check_bound(nm + " db twice", vb(b2), 2 * db, 2 * Sb, k, 2 * (shares + 1), torch.float32))
        else:
            assert float(b1[8:8 + Mo].abs().max()) == 0.0 and float(b2[8:8 + Mo].abs().max()) == 0.0, nm   # (as allocated)
        if exact and alpha == 1.0:
            gr.check_exact(nm + " dW = single launches", w1, ws)
            gr.check_exact(nm + " db = single launches", b1, bs)
            exp_w, exp_b = w1.clone(), b1.clone()
            exp_w[PRE:PRE + Mo, :No] *= 2
            if biases[i]:
                exp_b[8:8 + Mo] *= 2
            gr.check_exact(nm + " dW twice", w2, exp_w)
            gr.check_exact(nm + " db twice", b2, exp_b)
        # the operands and their padding are read only
        assert float(gY[dY.shape[0]:].float().min()) == PAD and float(gX[X.shape[0]:].float().min()) == PAD, nm
    print(f"GROUP {name}: common split {sk}, bound used {used:.3f}")
    assert used <= 1.0


@pytest.mark.parametrize("exact", (True, False))
@pytest.mark.parametrize("T", (128, 192, 448))
def test_two_and_three_problems_bias_on_off_mixed(hip, T, exact):
    """Every dW and db within the fp64 bound and of single launches, exact data bit-equal to them; canaries survive; a
    second launch doubles the result. alpha 1 on exact data, 1 and 0.37 on random data."""
    for group, biases in ((GROUP2, (True, True)), (GROUP2, (False, False)), (GROUP3, (True, False, True)),
                          (GROUP3, (False, True, False))):
        for alpha in ((1.0,) if exact else (1.0, 0.37)):
            run_group(hip, group, T, alpha, biases, (None,) * len(group), 160, exact)


@pytest.mark.parametrize("cap,want", ((3, 1), (6, 2), (8, 2), (9, 3), (160, 3)))
def test_caps_that_yield_common_splits_of_1_2_3(hip, cap, want):
    """25 K tiles: at most 3 splits; the cap decides. Shares of unequal length (10 + 10 + 6, 14 + 12) and, with the three
    problems of GROUP3 (5 tiles), a cap that is no multiple of the tile count."""
    assert _common_split(GROUP2, 1600, cap) == want
    run_group(hip, GROUP2, 1600, 1.0, (True, False), (None, None), cap, True)
    run_group(hip, GROUP2, 1600, 0.37, (True, True), (None, None), cap, False)
    if cap >= 5:
        run_group(hip, GROUP3, 1600, 1.0, (False, True, True), (None, None, None), cap, True)


@pytest.mark.parametrize("T,k_devs", ((448, (0, 0)), (448, (100, 447)), (448, (0, None)), (1600, (700, 65)), (1600, (1599, 0))))
def test_device_side_token_counts(hip, T, k_devs):
    """*k_dev below T per problem, 0 included: rows past the count (they hold the operands' other rows) add nothing, a count
    of 0 leaves the zeros, nothing faults; a split whose share the count leaves empty adds nothing."""
    run_group(hip, GROUP2, T, 1.0, (True, True), k_devs, 160, True)
    run_group(hip, GROUP2, T, 0.37, (True, False), k_devs, 160, False)
