"""GPU: stonk_row_topk_f32 / _f16 through ctypes against torch on the SAME input tensor. The stated total order (larger
value first, lower column first among equal values) is `torch.sort(..., descending=True, stable=True)` in fp64, the rank is
counted directly, the log-sum-exp is torch's in fp64. Ids, values, rank and the target's logit must match exactly, the
log-sum-exp within 1e-5 relative, two launches bit for bit. Inputs come from a CPU generator (the same on every machine)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -7
# (cap_rows, count, ncols, ld): a row shorter than one sweep with tile padding and rows past the count; the two decoders'
# real widths (29 056 = pad128(28 996): several sweeps of 8192, a ragged last one; 175 104: the long row); ncols = k = 16;
# and a row stride that is no multiple of 16 bytes in either dtype (the element-by-element sweep, no padding at all)
SHAPES = {"small": (40, 37, 300, 384), "text": (8, 8, 28996, 29056), "ent": (6, 5, 175094, 175104), "k16": (8, 7, 16, 24),
          "odd": (8, 8, 301, 301)}
_cache = {}


def _case(shape, dtype):
    """(input on the device, targets, expected dict) - built once per (shape, dtype) and left unchanged."""
    key = (shape, dtype)
    if key in _cache:
        return _cache[key]
    cap, count, ncols, ld = SHAPES[shape]
    g = torch.Generator().manual_seed(1234 + ncols)
    x = torch.full((cap, ld), 1.0e4)                       # padding columns: large and finite - must be ignored
    tgt = torch.zeros(cap, dtype=torch.int32)
    for r in range(cap):
        kind = r % 5
        if kind in (0, 4):
            row = torch.randn(ncols, generator=g) * 3.0
        elif kind == 1:
            row = torch.randint(-3, 4, (ncols,), generator=g).float()      # heavily tied
        elif kind == 2:
            row = torch.full((ncols,), 0.5)                                 # all equal
        else:
            row = torch.randn(ncols, generator=g) * 3.0
            row[ncols - 1] = 50.0                                           # the maximum in the last valid column
        x[r, :ncols] = row
        tgt[r] = (0, ncols - 1, int(torch.randint(0, ncols, (1,), generator=g)))[r % 3]
    x = x.to(dtype).cuda()
    tgt = tgt.cuda()
    xs = x[:count, :ncols].double()
    sv, si = torch.sort(xs, dim=1, descending=True, stable=True)
    t = tgt[:count].long()[:, None]
    T = xs.gather(1, t)
    col = torch.arange(ncols, device="cuda")[None]
    rank = (xs > T).sum(1) + ((xs == T) & (col < t)).sum(1)
    exp = dict(sv=sv[:, :16].float(), si=si[:, :16].int(), rank=rank.int(), tgt=T[:, 0].float(), lse=torch.logsumexp(xs, 1))
    _cache[key] = (x, tgt, exp)
    return _cache[key]


def _launch(hip, x, ncols, tgt, count, cap, k, with_targets=True):
    cnt = torch.tensor([count], device="cuda", dtype=torch.int32)
    out = dict(top_val=torch.full((cap, k), float(SENT), device="cuda"),
               top_idx=torch.full((cap, k), SENT, device="cuda", dtype=torch.int32),
               lse=torch.full((cap,), float(SENT), device="cuda"),
               rank=torch.full((cap,), SENT, device="cuda", dtype=torch.int32),
               tgt_logit=torch.full((cap,), float(SENT), device="cuda"))
    entry = "stonk_row_topk_f16" if x.dtype == torch.float16 else "stonk_row_topk_f32"
    hip.call(entry, hip.ptr(x), x.stride(0), ncols, hip.ptr(tgt) if with_targets else 0, hip.ptr(cnt), cap, k,
             hip.ptr(out["top_val"]), hip.ptr(out["top_idx"]), hip.ptr(out["lse"]),
             hip.ptr(out["rank"]) if with_targets else 0, hip.ptr(out["tgt_logit"]) if with_targets else 0, hip.stream_ptr())
    torch.cuda.synchronize()
    return out


def _check(out, exp, count, k):
    assert torch.equal(out["top_idx"][:count], exp["si"][:, :k])
    assert torch.equal(out["top_val"][:count], exp["sv"][:, :k])
    assert torch.equal(out["rank"][:count], exp["rank"])
    assert torch.equal(out["tgt_logit"][:count], exp["tgt"])
    lse, ref = out["lse"][:count].double(), exp["lse"]
    err = ((lse - ref).abs() / ref.abs()).max().item()
    print(f"lse: max relative error {err:.3e} (|lse| >= {ref.abs().min().item():.3f})")
    assert err <= 1e-5
    for name in out:                                       # rows at or past the count are not written
        assert (out[name][count:] == SENT).all(), name


CASES = [(s, k) for s in ("small", "text", "ent") for k in (1, 5, 10, 16)] + [("k16", 16), ("odd", 5), ("odd", 16)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape,k", CASES)
def test_row_topk_matches_torch_exactly(hip, shape, k, dtype):
    cap, count, ncols, ld = SHAPES[shape]
    x, tgt, exp = _case(shape, dtype)
    assert exp["lse"].abs().min().item() > 1.0             # (a relative bound needs a log-sum-exp away from zero)
    out = _launch(hip, x, ncols, tgt, count, cap, k)
    _check(out, exp, count, k)
    again = _launch(hip, x, ncols, tgt, count, cap, k)
    for name in out:                                       # the same input gives the same bits
        assert torch.equal(out[name].view(torch.int32), again[name].view(torch.int32)), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_row_topk_count_targets_and_capacity(hip, dtype):
    cap, count, ncols, ld = SHAPES["small"]
    x, tgt, exp = _case("small", dtype)
    # a count beyond the capacity is clamped to it; a count of zero writes nothing
    big = _launch(hip, x[:20], ncols, tgt, 10 ** 6, 20, 5)
    assert torch.equal(big["top_idx"], exp["si"][:20, :5]) and torch.equal(big["rank"], exp["rank"][:20])
    none = _launch(hip, x, ncols, tgt, 0, cap, 5)
    assert all((none[name] == SENT).all() for name in none)
    # without targets: top-k and log-sum-exp only, rank / tgt_logit untouched (null pointers)
    free = _launch(hip, x, ncols, tgt, count, cap, 5, with_targets=False)
    assert torch.equal(free["top_idx"][:count], exp["si"][:, :5]) and torch.equal(free["top_val"][:count], exp["sv"][:, :5])
    torch.testing.assert_close(free["lse"][:count].double(), exp["lse"], rtol=1e-5, atol=0)
    assert (free["rank"] == SENT).all() and (free["tgt_logit"] == SENT).all()
    # a target outside [0, ncols) - in the padding, or negative - reads nothing: rank -1, logit NaN, the row's other
    # outputs and every other row as before (the cross-entropy entry on the same targets raises the error bit)
    bad = tgt.clone()
    bad[3], bad[4] = ncols, -1
    out = _launch(hip, x, ncols, bad, count, cap, 5)
    assert out["rank"][3].item() == -1 and out["rank"][4].item() == -1
    assert math.isnan(out["tgt_logit"][3].item()) and math.isnan(out["tgt_logit"][4].item())
    keep = torch.ones(count, dtype=torch.bool, device="cuda")
    keep[3:5] = False
    assert torch.equal(out["rank"][:count][keep], exp["rank"][keep])
    assert torch.equal(out["top_idx"][:count], exp["si"][:, :5])
