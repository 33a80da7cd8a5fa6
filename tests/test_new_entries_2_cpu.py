"""CPU (no GPU): stonk_gemm_tn_bf16_store_sumsq, stonk_gemm_tn_store_tiles and stonk_sumsq_f32_plus refuse bad arguments with
the documented status codes, before anything is launched."""
from stonkgs_amd import _hip

OK, EINVAL, ESHAPE, EALIGN = _hip.OK, _hip.EINVAL, _hip.ESHAPE, _hip.EALIGN


def _store(sumsq=True, dY=4096, lda=768, X=8192, ldb=768, dW=16384, ldc=768, db=0, M=768, N=768, K=1024, alpha=1.0, split=1,
           k_dev=0, slots=32768, n_slots=4096):
    a = (dY, lda, X, ldb, dW, ldc, db, M, N, K, alpha, split, k_dev)
    if sumsq:
        return _hip.lib().stonk_gemm_tn_bf16_store_sumsq(*a, slots, n_slots, 0)
    return _hip.lib().stonk_gemm_tn_bf16_store(*a, 0)


def test_store_sumsq_refuses_what_the_store_entry_refuses():
    cases = [dict(dY=0), dict(X=0), dict(dW=0), dict(M=700), dict(N=100), dict(K=0), dict(lda=772), dict(dY=4100), dict(X=8200),
             dict(dW=16386), dict(db=16386), dict(ldc=512), dict(M=175104 * 4, split=-160), dict(M=699136, split=1),
             dict(split=2), dict(split=32), dict(split=0), dict(split=-160), dict(M=175104, split=-1),
             dict(M=175104, split=-160, db=64), dict(M=175104, split=-2000)]
    for kw in cases:
        want = _store(sumsq=False, **kw)
        assert want in (EINVAL, ESHAPE, EALIGN), kw
        assert _store(**kw) == want, kw


def test_store_sumsq_slot_arguments():
    assert _store(slots=0) == EINVAL and _store(n_slots=-1) == EINVAL
    assert _store(slots=32770) == EALIGN
    assert _store(n_slots=35) == EINVAL                      # 768 x 768: 36 tiles of 128x128
    assert _store(M=175104, split=-160, n_slots=2051) == EINVAL   # 684 x 3 tiles of 256x256


def test_store_tiles_counts_or_refuses():
    tiles = _hip.lib().stonk_gemm_tn_store_tiles
    assert tiles(768, 768, 1024, 1) == 36
    assert tiles(175104, 768, 32768, -160) == 684 * 3 and tiles(175104, 768, 32768, 0) == 684 * 3
    assert tiles(29056, 768, 32768, 1) == 227 * 6
    assert tiles(384, 256, 192, 1) == 6 and tiles(512, 512, 192, 0) == 4 and tiles(512, 512, 192, -16) == 4
    assert tiles(768, 768, 1024, 2) == ESHAPE and tiles(768, 768, 1024, 0) == ESHAPE and tiles(768, 768, 1024, -160) == ESHAPE
    assert tiles(175104, 768, 32768, -1) == ESHAPE and tiles(175104, 768, 32768, -2000) == ESHAPE
    assert tiles(700, 768, 1024, 1) == ESHAPE and tiles(768, 100, 1024, 1) == ESHAPE and tiles(768, 768, 0, 1) == ESHAPE
    assert tiles(699136, 768, 1024, 1) == ESHAPE             # M * ldc * 4 >= 2^31


def _plus(x=4096, n=1024, out=64, ws=8192, ws_floats=257, extra=16384, n_extra=8):
    return _hip.lib().stonk_sumsq_f32_plus(x, n, out, ws, ws_floats, extra, n_extra, 0)


def test_sumsq_plus_argument_checks():
    for null in ("x", "out", "ws"):
        assert _plus(**{null: 0}) == EINVAL, null
    assert _plus(n=-1) == EINVAL and _plus(n_extra=-1) == EINVAL and _plus(extra=0) == EINVAL   # a count without its array
    assert _plus(ws_floats=256) == EINVAL
    assert _plus(x=4100) == EALIGN and _plus(ws=8194) == EALIGN and _plus(extra=16386) == EALIGN
    assert _plus(n=0, extra=0, n_extra=0) == OK                                                 # nothing to do, nothing launched
