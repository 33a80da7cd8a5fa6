"""GPU: the GEMM kernels (gemm_bf16.hip, gemm256.hip, gemm_w4.hip, gemm_a4.hip, gemm_tn*.hip and the epilogues of
gemm_common.h) against tests/gemm_ref.py - bit for bit on exact data, per element against float64 elsewhere.

Every output is a view into a larger allocation filled with a sentinel: the rows before and after the view, the padding
columns [N, ld) and the rows at or past *m_dev must come back bit for bit (C, the stored aux, dW, db, the sum-of-squares
slots). Every operand is a view with ld > width as well, all the ld different, its padding holding 1000. No case
addresses outside its allocations by construction. Every non-atomic NT case is launched twice: the two must be equal.
Run with -s for the PARITY lines (profiles/gemm_parity.md is such a collection).
"""
import functools

import pytest
import torch

from tests import gemm_ref as gr
from tests.gemm_ref import (AG, ASM4, ASM4_192, ATOMIC, B, BF16, D, F16, F32, GB, R, SV, TILE128, WAVE4, WAVE4_192, WAVE8,
                            PAD, SENTINEL)

pytestmark = pytest.mark.gpu

PRE, POST = 2, 3                                   # sentinel rows before / after every view
KERNELS = (TILE128, WAVE8, WAVE4, WAVE4_192, ASM4, ASM4_192)
ODD_K_TILES = (TILE128, WAVE8)                     # the four-wave kernels walk K tiles in pairs
WIDE_192 = (WAVE4_192, ASM4_192)
RAGGED_N = (WAVE8, WAVE4, ASM4)                    # 256-wide tiles over any N % 128 == 0


def _alloc(view, ld, fill, pre=PRE, post=POST):
    """CPU allocation [pre + rows + post, ld] of `fill` with `view` in rows [pre, pre + rows), columns [0, cols)."""
    rows, cols = view.shape
    assert ld > cols and ld % 8 == 0
    buf = torch.full((pre + rows + post, ld), fill, dtype=view.dtype)
    buf[pre:pre + rows, :cols] = view
    return buf


def _alloc1(vec, fill, pad=8):
    buf = torch.full((pad + vec.numel() + pad,), fill, dtype=vec.dtype)
    buf[pad:pad + vec.numel()] = vec
    return buf


def _view(g, rows, cols, pre=PRE):
    return g[pre:pre + rows, :cols]


def _int(v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device="cuda")


def _launch_nt(hip, kernel, flags, M, N, K, gA, gB, gC, gbias, gres, gaux, alpha, split_k, m_dev, k_dev, p, seed):
    A, Bm, C = _view(gA, M, K), _view(gB, N, K), _view(gC, M, N)
    res = None if gres is None else _view(gres, M, N)
    aux = None if gaux is None else _view(gaux, M, N)
    bias = None if gbias is None else gbias[8:8 + N]
    return hip.lib().stonk_gemm_nt_bf16(
        hip.ptr(A), A.stride(0), hip.ptr(Bm), Bm.stride(0), hip.ptr(C), C.stride(0), M, N, K, flags, hip.ptr(bias),
        hip.ptr(res), 0 if res is None else res.stride(0), hip.ptr(aux), 0 if aux is None else aux.stride(0), alpha, split_k,
        hip.ptr(m_dev), hip.ptr(k_dev), p, seed, kernel, hip.stream_ptr())


def run_nt(hip, kernel, out, epi, M, N, K, kind="ints", *, alpha=1.0, split_k=1, m_dev=None, k_dev=None, p=0.5, seed=77,
           adds=2, expect_status=0):
    """One NT case: launch (twice unless atomic), compare the whole allocations. Exact data and no transcendental: bit for
    bit; otherwise check_bound on the view and bit for bit around it. Returns the share of the bound used (0 if exact)."""
    name = f"{gr.KERNEL_NAMES[kernel]} {gr.epi_name(out, epi)} {M}x{N}x{K} {kind}"
    A, Bm, bias, resid, u, C0 = gr.nt_operands(M, N, K, kind)
    prod, prod_abs = gr.nt_products(M, N, K, kind)
    dtype = gr.OUT_DTYPE[out]
    flags = out | epi
    kk = K
    if k_dev is not None:                          # the contract: columns [k, roundup64(k)) read as zero; past that, anything
        kk, up = min(k_dev, K), min(K, (min(k_dev, K) + 63) // 64 * 64)
        A, Bm = A.clone(), Bm.clone()
        A[:, kk:up], Bm[:, kk:up] = 0, 0
        A[:, up:], Bm[:, up:] = PAD, PAD
        prod, prod_abs = A[:, :kk].double() @ Bm[:, :kk].double().t(), A[:, :kk].double().abs() @ Bm[:, :kk].double().abs().t()
    lda, ldb, ldc, ldr, ldx = K + 64, K + 128, N + 8, N + 16, N + 24
    gA, gB = _alloc(A, lda, PAD).cuda(), _alloc(Bm, ldb, PAD).cuda()
    gbias = _alloc1(bias, PAD).cuda() if epi & B else None
    gres = _alloc(resid, ldr, PAD).cuda() if epi & R else None
    c_cpu = _alloc(C0 if out == ATOMIC else torch.full((M, N), SENTINEL, dtype=dtype), ldc, SENTINEL)
    aux_cpu = None
    if epi & GB:
        aux_cpu = _alloc(u, ldx, PAD)
    elif epi & SV:
        aux_cpu = _alloc(torch.full((M, N), SENTINEL, dtype=torch.bfloat16), ldx, SENTINEL)
    gm, gk = _int(m_dev), _int(k_dev)
    runs = []
    for _ in range(1 if out == ATOMIC or expect_status else 2):
        gC = c_cpu.cuda()
        gaux = None if aux_cpu is None else aux_cpu.cuda()
        status = _launch_nt(hip, kernel, flags, M, N, K, gA, gB, gC, gbias, gres, gaux, alpha, split_k, gm, gk, p, seed)
        assert status == expect_status, f"{name}: status {status}, expected {expect_status}"
        runs.append((gC, gaux))
    torch.cuda.synchronize()
    if expect_status:
        assert torch.equal(runs[0][0].cpu(), c_cpu), f"{name}: a refused launch wrote"
        return 0.0
    if len(runs) == 2:
        assert torch.equal(runs[0][0], runs[1][0]), f"{name}: two launches differ"
        if epi & SV:
            assert torch.equal(runs[0][1], runs[1][1]), f"{name}: two launches differ (aux)"
    got_c = runs[0][0].cpu()
    got_aux = runs[0][1].cpu() if epi & SV else None
    assert torch.equal(gA.cpu(), _alloc(A, lda, PAD)) and torch.equal(gB.cpu(), _alloc(Bm, ldb, PAD)), f"{name}: an operand was written"

    rows = M if m_dev is None else min(m_dev, M)
    keep = gr.oracle_keep(M, N, seed, p) if epi & D else None
    kw = dict(bias=bias, resid=resid, aux_in=u, alpha=alpha, C0=C0, rows=rows, drop_p=p)
    r, aux_r = gr.gemm_nt_ref(A, Bm, flags, keep_mask=keep, prod=prod, **kw)
    exact_values = kind in ("ints", "ints16") and not gr.is_transcendental(epi) and (not epi & D or p in (0.0, 0.5))
    expect_c = c_cpu.clone()
    used = 0.0
    if exact_values:
        expect_c[PRE:PRE + rows, :N] = gr.round_exact(r, dtype)
        gr.check_exact(name, got_c, expect_c)
    else:
        expect_c[PRE:PRE + rows, :N] = got_c[PRE:PRE + rows, :N]
        gr.check_exact(name + " (around the view)", got_c, expect_c)
        a_extra = 0.0
        if gr.is_transcendental(epi):
            v32, _ = gr._nt(A, Bm, flags, bias, resid, u, alpha, C0, rows, keep, p, torch.float32)
            a_extra = gr.a_extra_of(v32, r)
        S = gr.gemm_nt_S(A, Bm, flags, prod_abs=prod_abs, **kw)
        if kind == "gelu":                                   # the product is exact there: a_extra is the whole tolerance
            S = torch.zeros_like(S)
        used = gr.check_bound(name, got_c[PRE:PRE + rows, :N], r, S, kk, adds, dtype, a_extra)
    if epi & D and rows:                                     # the mask, element for element, whatever the values' check
        view = got_c[PRE:PRE + rows, :N]
        base = resid[:rows].to(dtype) if epi & R else torch.zeros((), dtype=dtype)
        # an element shows its fate where the kept value differs from the dropped one: everywhere with a bias of odd quarters
        # and alpha = 1 (test_gemm_ref_cpu.py asserts it); a zero product (no bias) or alpha * product = -bias shows nothing
        all_kept, _ = gr.gemm_nt_r32(A, Bm, flags, keep_mask=torch.ones(M, N, dtype=torch.bool), **kw)
        shows = all_kept != base
        assert shows.all() or not epi & B or alpha != 1.0, f"{name}: the data hides {int((~shows).sum())} mask elements"
        bad = ((view == base) != ~keep[:rows]) & shows
        assert not bad.any(), f"{name}: {int(bad.sum())} mask elements differ from the oracle, first {bad.nonzero()[:4].tolist()}"
    if epi & SV:
        expect_aux = aux_cpu.clone()
        if epi & AG:
            expect_aux[PRE:PRE + rows, :N] = got_aux[PRE:PRE + rows, :N]
            gr.check_exact(name + " aux (around the view)", got_aux, expect_aux)
            _, a32 = gr._nt(A, Bm, flags, bias, resid, u, alpha, C0, rows, keep, p, torch.float32)
            used = max(used, gr.check_bound(name + " aux", got_aux[PRE:PRE + rows, :N], aux_r, torch.zeros_like(aux_r), kk, adds,
                                            torch.bfloat16, gr.a_extra_of(a32, aux_r)))
        else:
            expect_aux[PRE:PRE + rows, :N] = gr.rne_bf16(aux_r)
            gr.check_exact(name + " aux", got_aux, expect_aux)
    return used


def _shapes(kernel, out, epi):
    """(M, N, K) of an instance: every host M on the plain product and on B | R | D, M in {257, 1024} otherwise; K in
    {128, 256} (+ 192 where an odd number of K tiles is taken), N in {256, 768} (192-wide tiles: 768, and 384 where the
    four-wave kernel has run it before), and N = 384 on the persistent kernels with 256-wide tiles: a ragged last column tile,
    whose stores, side-operand and bias reads past N each kernel has to mask itself."""
    ks = (128, 256, 192) if kernel in ODD_K_TILES else (128, 256)
    ns = (768, 384) if kernel == WAVE4_192 else (768, 768) if kernel == ASM4_192 else (256, 768)
    if out == F16:
        return [(257, 768, 768), (1024, 256, 768), (1, 256, 768)]
    if epi in (0, B | R | D) and out in (BF16, F32):
        shapes = [(M, ns[i % 2], ks[i % len(ks)]) for i, M in enumerate(gr.HOST_M)]
        return shapes + ([(301, 384, 128)] if kernel in RAGGED_N else [])
    return [(257, ns[1], 128), (1024, ns[0], 256), (257, ns[1], ks[-1])] + ([(257, 384, 256)] if kernel in RAGGED_N else [])


_IDS = [f"{gr.KERNEL_NAMES[k]}-{gr.epi_name(o, e)}" for k, o, e, _ in gr.INSTANCES]


@pytest.mark.parametrize("kernel,out,epi,where", gr.INSTANCES, ids=_IDS)
def test_every_compiled_instance(hip, kernel, out, epi, where):
    """a. Every (output mode, epilogue) pair of the launchers' switches, by explicit kernel id. Exact data: bf16 / fp16 / fp32
    outputs equal rne(exact float64 value), SAVE_PREACT stores rne_bf16(pre), GELU_BWD | AUX_GRAD is exact; dropout at p = 0.5
    (scale 2: exact). The GELU family runs on the power-of-two scaled data against the bound, a_extra its whole tolerance."""
    kind = "ints16" if out == F16 else "gelu" if gr.is_transcendental(epi) else "ints"
    used = 0.0
    for M, N, K in _shapes(kernel, out, epi):
        used = max(used, run_nt(hip, kernel, out, epi, M, N, K, kind, alpha=0.5 if out == ATOMIC else 1.0))
    print(f"INSTANCE {gr.KERNEL_NAMES[kernel]} {gr.epi_name(out, epi)} [{where}] bound used {used:.3f}")


ALPHA_FORMS = [(k, e) for k in (TILE128, WAVE4, WAVE4_192) for e in (0, B, B | R, B | R | D)] + \
              [(k, GB | AG) for k in (TILE128, WAVE4)] + [(WAVE8, e) for e in (0, R, GB | AG)] + [(TILE128, B | D)]


@pytest.mark.parametrize("kernel,epi", ALPHA_FORMS, ids=[f"{gr.KERNEL_NAMES[k]}-{gr.epi_name(BF16, e)}" for k, e in ALPHA_FORMS])
def test_alpha_is_applied_before_the_bias(hip, kernel, epi):
    """alpha != 1 on the kernels that accept it (the eight-wave kernel: without a bias), bf16 and fp32 output: exact."""
    for alpha in (0.5, -2.0):
        run_nt(hip, kernel, BF16, epi, 257, 768, 128, alpha=alpha)
        if kernel in (TILE128, WAVE4, WAVE8) and not epi & (GB | D) and kernel != WAVE4_192:
            run_nt(hip, kernel, F32, epi, 301, 256, 256, alpha=alpha)


@pytest.mark.parametrize("kernel,out,epi,kw,status,why", gr.REFUSALS,
                         ids=[f"{gr.KERNEL_NAMES[r[0]]}-{gr.epi_name(r[1], r[2])}-{i}" for i, r in enumerate(gr.REFUSALS)])
def test_refusals(hip, kernel, out, epi, kw, status, why):
    """A pair a kernel does not list, or arguments it cannot take: the documented status, and nothing written."""
    kw = dict(kw)
    N, K = kw.pop("N", 768), kw.pop("K", 128)
    run_nt(hip, kernel, out, epi, 257, N, K, expect_status=status, **kw)


@pytest.mark.parametrize("kernel", KERNELS, ids=[gr.KERNEL_NAMES[k] for k in KERNELS])
def test_device_row_count(hip, kernel):
    """*m_dev in {0, 1, 255, 256, 257, M} under a capacity of 512 rows, and a count above the capacity: rows at or past it
    keep the sentinel."""
    for m_dev in gr.DEV_M + (512, 600):
        run_nt(hip, kernel, BF16, 0, 512, 768, 128, m_dev=m_dev)
        run_nt(hip, kernel, BF16, B | R | D, 512, 768, 256, m_dev=m_dev)
    if kernel in (TILE128, WAVE8, ASM4):
        for m_dev in (0, 1, 257):
            run_nt(hip, kernel, F16, 0, 512, 256, 768, "ints16", m_dev=m_dev)


PERSISTENT = (WAVE8, WAVE4, WAVE4_192, ASM4, ASM4_192)


@pytest.mark.parametrize("kernel", PERSISTENT, ids=[gr.KERNEL_NAMES[k] for k in PERSISTENT])
def test_several_tiles_per_workgroup(hip, kernel):
    """260 tiles of 256 x 192 (195 of 256 x 256) on 256 CUs: tile boundaries of the persistent loops, ragged last row tile."""
    run_nt(hip, kernel, BF16, 0, 16640 - 37, 768, 128)
    run_nt(hip, kernel, BF16, B | R, 16640 - 37, 768, 128)


@pytest.mark.parametrize("M", [1024, 1280])
@pytest.mark.parametrize("kernel", [5, 6], ids=["DISPATCHED", "DISPATCHED2"])
def test_dispatched_forms(hip, kernel, M):
    """AUTO's choice with one / two work items per workgroup, an even and an odd tile count."""
    for epi in (0, B | R, B | R | D):
        run_nt(hip, kernel, BF16, epi, M, 768, 128)


DROPOUT_FORMS = [(k, BF16, B | R | D) for k in KERNELS] + [(TILE128, BF16, B | D), (TILE128, F32, D), (TILE128, F32, B | R | D),
                                                           (WAVE4, BF16, B | D)]


@pytest.mark.parametrize("p", [0.5, 0.1, 0.0])
@pytest.mark.parametrize("kernel,out,epi", DROPOUT_FORMS,
                         ids=[f"{gr.KERNEL_NAMES[k]}-{gr.epi_name(o, e)}" for k, o, e in DROPOUT_FORMS])
def test_dropout_masks_are_the_oracles(hip, kernel, out, epi, p):
    """Masks from dropout_oracle.keep(arange(M), arange(N), seed, p), element for element: the same on every kernel and tile
    width. p = 0.5: the whole output bit for bit; p = 0.1: the mask exact (dropped <=> out == resid), values within the
    bound; p = 0 with the flag set: everything kept."""
    for seed in gr.SEEDS:
        run_nt(hip, kernel, out, epi, 301, 768, 128, p=p, seed=seed)


SPLIT_KERNELS = (TILE128, WAVE8, WAVE4, ASM4_192)


@pytest.mark.parametrize("nk", [2, 6, 10, 66])
@pytest.mark.parametrize("kernel", SPLIT_KERNELS, ids=[gr.KERNEL_NAMES[k] for k in SPLIT_KERNELS])
def test_split_k_atomic_is_exact(hip, kernel, nk):
    """C (integers) += 0.5 * A . B^T over split_k shares, shares that do not divide the K tiles included: a K tile lost or
    taken twice at a share boundary shows. On ASM4_192 split_k is an upper bound."""
    N = 768 if kernel == ASM4_192 else 256
    for i, sk in enumerate((1, 2, 3, 4, 5, 8)):
        if sk > nk:
            continue
        if kernel == WAVE4 and nk % (2 * sk):        # the four-wave kernel: an even number of K tiles per share
            run_nt(hip, kernel, ATOMIC, 0, 301, N, 64 * nk, alpha=0.5, split_k=sk, expect_status=hip.ESHAPE)
            continue
        run_nt(hip, kernel, ATOMIC, 0, 301, N, 64 * nk, alpha=0.5, split_k=sk, m_dev=(None, 257, 1, 0, 256, 255)[i])


@pytest.mark.parametrize("kernel", [TILE128, WAVE8], ids=["TILE128", "WAVE8"])
def test_device_contraction_length(hip, kernel):
    """*k_dev in {0, 1, 63, 64, 65, 129, K}: K tiles past ceil(k / 64) are skipped (they hold 1000), the columns in
    [k, roundup64(k)) are zero by contract."""
    for k_dev in gr.DEV_K + (256,):
        for sk in (1, 2, 3):
            run_nt(hip, kernel, ATOMIC, 0, 257, 256, 256, alpha=0.5, split_k=sk, k_dev=k_dev)


@pytest.mark.parametrize("arm,M,N,K,out,epi,alpha", gr.AUTO_ARMS, ids=[a[0] for a in gr.AUTO_ARMS])
def test_auto_routing_arms(hip, arm, M, N, K, out, epi, alpha):
    run_nt(hip, hip.GEMM_AUTO, out, epi, M, N, K, alpha=alpha)


# ------------------------------------------------------------------------------------------------ b. random data, fp64
RANDOM_OUTS = {TILE128: (BF16, F32, F16, ATOMIC), WAVE8: (BF16, F32, F16, ATOMIC), WAVE4: (BF16, F32, ATOMIC), WAVE4_192: (BF16,),
               ASM4: (BF16, F16), ASM4_192: (BF16, ATOMIC)}


@pytest.mark.parametrize("kind", ["randn", "rows"])
@pytest.mark.parametrize("kernel", KERNELS, ids=[gr.KERNEL_NAMES[k] for k in KERNELS])
def test_random_data_within_the_bound(hip, kernel, kind):
    """A ~ N(0, 1), B ~ N(0, 0.05); 'rows': the rows of A scaled by 2^-10 ... 2^10, which a max-norm tolerance would hide."""
    used = 0.0
    for M, N, K in ((257, 768, 768), (301, 256, 3072)):
        if kernel in WIDE_192 and N % 192:
            continue
        for out in RANDOM_OUTS[kernel]:
            sk = 2 if out == ATOMIC else 1
            used = max(used, run_nt(hip, kernel, out, 0, M, N, K, kind, split_k=sk, adds=sk + 1))
            if out == BF16:
                used = max(used, run_nt(hip, kernel, out, B | R, M, N, K, kind))
    print(f"RANDOM {gr.KERNEL_NAMES[kernel]} {kind} bound used {used:.3f}")
    assert used <= 1.0


# ------------------------------------------------------------------------------------------------ the weight gradients
TN_ENTRIES = ("stonk_gemm_tn_bf16", "stonk_gemm_tn_bf16_store", "stonk_gemm_tn_bf16_store_sumsq")
TN_SPLITS = (1, 2, 3, 0, -1, -160)
TN_SHAPES = ((128, 128), (256, 256), (768, 256), (384, 640))
TN_T = (64, 192, 320, 2048)


def _tn_status(hip, entry, Mo, No, T, split, bias):
    """The documented routing (include/stonk_hip.h): what each entry admits."""
    nk = (T + 63) // 64
    store = entry != TN_ENTRIES[0]
    if split <= 0:
        if Mo < 256 or No < 256:
            return hip.ESHAPE
        if store:
            tiles = ((Mo + 255) // 256) * ((No + 255) // 256)
            cus = -split if split <= -16 else 256
            sk = 1 if tiles >= cus else cus // tiles
            if sk > nk // 8:
                sk = max(nk // 8, 1)
            if sk != 1 or split == -1 or (bias and No > 256):
                return hip.ESHAPE
    elif store and min(split, nk) != 1:
        return hip.ESHAPE
    return hip.OK


@functools.lru_cache(maxsize=None)
def _tn_operands(T, Mo, No, lim):
    seed = 7919 * T + 31 * Mo + No + lim
    return (gr.ints((T, Mo), lim, seed), gr.ints((T, No), lim, seed + 1), gr.ints((Mo, No), 8, seed + 2).float(),
            gr.quarters(Mo, seed + 3))


def run_tn(hip, entry, split, T, Mo, No, alpha, k_dev=None, lim=8):
    name = f"{entry} split {split} T={T} {Mo}x{No} alpha={alpha} k_dev={k_dev}"
    dY, X, dW0, db0 = _tn_operands(T, Mo, No, lim)
    store = entry != TN_ENTRIES[0]
    sumsq = entry == TN_ENTRIES[2]
    bias = not (store and split <= 0 and No > 256)          # (the store form of the 256x256 kernel: a bias with one column tile)
    k = T
    if k_dev is not None:
        k, up = k_dev, (k_dev + 63) // 64 * 64
        dY, X = dY.clone(), X.clone()
        # rows [k, roundup64(k)): zero where the kernel asks for it (128x128 and the eight-wave form), else 1000 like the rest
        fill = PAD if split in (0, -160) else 0
        dY[k:up], X[k:up] = fill, fill
        dY[up:], X[up:] = PAD, PAD
    lda, ldb, ldc = Mo + 64, No + 128, No + 8
    gY, gX = _alloc(dY, lda, PAD).cuda(), _alloc(X, ldb, PAD).cuda()
    w_cpu = _alloc(torch.full((Mo, No), SENTINEL) if store else dW0, ldc, SENTINEL)
    b_cpu = _alloc1(torch.full((Mo,), SENTINEL) if store else db0, SENTINEL)
    tile = 256 if split <= 0 else 128
    rt, ct = (Mo + tile - 1) // tile, (No + tile - 1) // tile
    s_cpu = torch.full((rt * ct + 3,), SENTINEL)
    gW, gb, gs, gk = w_cpu.cuda(), b_cpu.cuda(), s_cpu.cuda(), _int(k_dev)
    vY, vX, vW = _view(gY, T, Mo), _view(gX, T, No), _view(gW, Mo, No)
    args = [hip.ptr(vY), lda, hip.ptr(vX), ldb, hip.ptr(vW), ldc, hip.ptr(gb[8:8 + Mo]) if bias else 0, Mo, No, T, alpha, split,
            hip.ptr(gk)]
    if sumsq:
        args += [hip.ptr(gs), rt * ct]
    status = getattr(hip.lib(), entry)(*args, hip.stream_ptr())
    want = _tn_status(hip, entry, Mo, No, T, split, bias)
    assert status == want, f"{name}: status {status}, documented {want}"
    torch.cuda.synchronize()
    expect_w, expect_b, expect_s = w_cpu.clone(), b_cpu.clone(), s_cpu.clone()
    if status == hip.OK:
        dW, db = gr.gemm_tn_ref(dY, X, k, alpha, None if store else dW0, None if store else db0)
        expect_w[PRE:PRE + Mo, :No] = gr._f32_exact(dW)
        if bias:
            expect_b[8:8 + Mo] = gr._f32_exact(db)
        if sumsq:
            sq = (dW ** 2).view(rt, tile, ct, tile).sum(dim=(1, 3)).reshape(-1) if Mo % tile == 0 and No % tile == 0 else None
            assert sq is not None and float(sq.max()) * (4 if alpha == 0.5 else 1) < 2 ** 24, name
            expect_s[:rt * ct] = gr._f32_exact(sq)
    gr.check_exact(name + " dW", gW.cpu(), expect_w)
    gr.check_exact(name + " db", gb.cpu(), expect_b)
    gr.check_exact(name + " slots", gs.cpu(), expect_s)
    assert torch.equal(gY.cpu(), _alloc(dY, lda, PAD)) and torch.equal(gX.cpu(), _alloc(X, ldb, PAD)), f"{name}: an operand was written"
    return status


@pytest.mark.parametrize("split", TN_SPLITS)
@pytest.mark.parametrize("entry", TN_ENTRIES)
def test_weight_gradient_entries(hip, entry, split):
    """dW, db and the padding exact: accumulate into non-zero dW0 / db0, store over a sentinel; token counts T and shapes
    either side of the 128- and 256-wide tiles, ldc > No, alpha 1 and 0.5; what an entry does not admit is refused with
    the documented status and writes nothing."""
    sumsq = entry == TN_ENTRIES[2]
    launched = 0
    for i, (Mo, No) in enumerate(TN_SHAPES):
        if (Mo, No) == (384, 640) and split <= 0:
            continue                                         # (the 128x128 kernel only)
        if sumsq and (Mo % 256 or No % 256) and split <= 0:
            continue
        for j, T in enumerate(TN_T):
            if sumsq and T > 320:
                continue                                     # (the squares' sums must stay below 2^24)
            alpha = (1.0, 0.5)[(i + j) % 2]
            launched += run_tn(hip, entry, split, T, Mo, No, alpha, lim=1 if sumsq else 8) == hip.OK
    print(f"TN {entry} split {split}: {launched} launched")


@pytest.mark.parametrize("split", TN_SPLITS)
@pytest.mark.parametrize("entry", TN_ENTRIES)
def test_weight_gradient_device_token_count(hip, entry, split):
    """*k_dev in {0, 1, 63, 64, 65, 129, T}. The four-wave kernel range-checks the tokens (rows past the count hold 1000); the
    128x128 kernel and the eight-wave form need zeros up to the 64 round-up and skip the K tiles behind it (1000 there)."""
    sumsq = entry == TN_ENTRIES[2]
    for T, (Mo, No) in ((192, (256, 256)), (320, (768, 256))):
        for k in gr.DEV_K + (T,):
            run_tn(hip, entry, split, T, Mo, No, 0.5 if k % 2 else 1.0, k_dev=k, lim=1 if sumsq else 8)
