"""CPU (no GPU): stonk_adamw_step_tiled and stonk_gemm_tn_bf16_store refuse bad arguments with the documented status codes,
before anything is launched."""
from stonkgs_amd import _hip

OK, EINVAL, ESHAPE, EALIGN = _hip.OK, _hip.EINVAL, _hip.ESHAPE, _hip.EALIGN


def _adamw(**kw):
    a = dict(p=64, g=128, m=192, v=256, pb=320, n=1024, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, bc1=0.1, bc2=0.001,
             gnorm=0, max_norm=1.0, scale=1.0, decay=0, n_decay=0, keep=0, n_keep=0, desc=512, n_desc=1, tiles=4, flat=1024,
             n_flat=1, chunks=1, stream=0)
    a.update(kw)
    return _hip.lib().stonk_adamw_step_tiled(*a.values())


def test_tiled_adamw_argument_checks():
    assert (EINVAL, ESHAPE, EALIGN) == (-1, -2, -3)
    for null in ("p", "g", "m", "v", "pb", "desc"):
        assert _adamw(**{null: 0}) == EINVAL, null
    assert _adamw(n=1022) == EINVAL and _adamw(n=-4) == EINVAL             # n % 4
    assert _adamw(n_desc=0) == EINVAL and _adamw(tiles=0) == EINVAL
    assert _adamw(n_decay=2) == EINVAL and _adamw(n_keep=1) == EINVAL      # a count without its table
    assert _adamw(flat=0) == EINVAL and _adamw(n_flat=1, chunks=0) == EINVAL and _adamw(n_flat=0, chunks=3) == EINVAL
    assert _adamw(bc1=0.0) == EINVAL
    for name in ("p", "g", "m", "v"):
        assert _adamw(**{name: 68}) == EALIGN, name                         # 16-byte vectors
    assert _adamw(pb=322) == EALIGN
    assert _adamw(desc=516) == EALIGN and _adamw(flat=1028) == EALIGN      # table pointers: 8 bytes
    assert _adamw(decay=260, n_decay=1) == EALIGN and _adamw(keep=260, n_keep=1) == EALIGN
    assert _adamw(n=0) == OK                                                # nothing to do, nothing launched


def _store(dY=4096, lda=768, X=8192, ldb=768, dW=16384, ldc=768, db=0, M=768, N=768, K=1024, alpha=1.0, split=1, k_dev=0):
    return _hip.lib().stonk_gemm_tn_bf16_store(dY, lda, X, ldb, dW, ldc, db, M, N, K, alpha, split, k_dev, 0)


def test_store_mode_wgrad_argument_checks():
    assert _store(dY=0) == EINVAL and _store(X=0) == EINVAL and _store(dW=0) == EINVAL
    assert _store(M=700) == ESHAPE and _store(N=100) == ESHAPE and _store(K=0) == ESHAPE
    assert _store(lda=772) == EALIGN and _store(dY=4100) == EALIGN and _store(X=8200) == EALIGN
    assert _store(dW=16386) == EALIGN and _store(db=16386) == EALIGN
    assert _store(ldc=512) == ESHAPE                                        # ldc >= N
    assert _store(M=175104 * 4, split=-160) == ESHAPE                       # M * ldc * 4 >= 2^31
    assert _store(M=699136, ldc=768, split=1) == ESHAPE                     # (the same bound on the 128x128 kernel)
    assert _store(split=2) == ESHAPE and _store(split=32) == ESHAPE        # several producers per element
    assert _store(split=0) == ESHAPE and _store(split=-160) == ESHAPE      # 9 tiles: the automatic split is > 1
    assert _store(M=175104, split=-1) == ESHAPE                             # the eight-wave form has no store mode
    assert _store(M=175104, split=-160, db=64) == ESHAPE                    # bias over three column tiles of the 256x256 kernel
    assert _store(M=175104, split=-2000) == ESHAPE
