"""GPU parity of the kernels behind evaluation and analysis - stonk_row_topk_f32 / _f16, stonk_input_attribution,
stonk_attention_probs, stonk_word_embed_grad, stonk_gather_rows_bf16 / stonk_scatter_rows_* / stonk_label_compact - through
the C ABI against float64, on the branches the feature tests do not reach: grid-stride trips beyond the launchers' caps,
every top-k instantiation and its boundaries, -0.0 / -inf / sorted rows, widths with idle lanes and lone second chunks,
S = 1024 and 4096, odd grids, sparse live keys, clamped gathers and three different strides.

Cases, references and the reasons for the shapes: tests/analysis_ref.py (pinned without a GPU by test_analysis_ref_cpu.py).
Outputs and operands are views inside sentinel-filled allocations whose margins are checked after the launches; every
launch is made twice and compared bit for bit (the word-table gradient, which adds with float atomics, is not).
Bounds: top-k ids, values, rank and target logit exact, log-sum-exp 1e-5 relative (test_topk_gpu.py's); attributions as in
test_input_attribution_kernel_gpu.py; probabilities and masses |got - r| <= A (tests/parity_util.py) and, above 1e-6,
relative error <= 8 x that of torch's float32 softmax on the same case; the word gradient count x 2^-23 x magnitude; the
movers bit for bit. Each check prints a PARITY line before it asserts (-s): profiles/analysis_parity.md is one run's.

The `misaligned` top-k case compares ids, values, rank and target logit bit for bit with the aligned launch; the
log-sum-exp of the element-by-element sweep sums in another order (a thread takes columns t, t + 256, ... instead of eight
consecutive ones), so it is held to the same 1e-5 against float64 and the number of differing rows is printed.
"""
import pytest
import torch

from tests import analysis_ref as ar
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

LEAD = 64                      # elements in front of a flat view (a multiple of 16 bytes for every type used)
FRAME = 7.0                    # what the margins of a bf16 / fp32 allocation hold where NaN would hide a compare
NAN = float("nan")


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(t, fill):
    return torch.equal(_bits(t), _bits(torch.full_like(t, fill)))


def _flat(n, fill, dtype=torch.float32, shift=0):
    """(allocation, view of n elements at LEAD + shift) - the margins hold `fill`."""
    full = torch.full((n + 2 * LEAD + 8,), fill, device="cuda", dtype=dtype)
    return full, full[LEAD + shift:LEAD + shift + n]


def _flat_ok(full, n, fill, shift=0):
    return _same(full[:LEAD + shift], fill) and _same(full[LEAD + shift + n:], fill)


def _framed(rows, cols, ld, fill, dtype, src=None, inner=None):
    """A [rows, cols] view of row stride ld, 8 columns in and one row down inside an allocation filled with `fill`."""
    assert cols + 8 <= ld
    full = torch.full((rows + 2, ld), fill, device="cuda", dtype=dtype)
    view = full[1:1 + rows, 8:8 + cols]
    if inner is not None:
        view.fill_(inner)
    if src is not None:
        view.copy_(src)
    return full, view


def _framed_ok(full, cols, fill):
    return all(_same(x, fill) for x in (full[0], full[-1], full[:, :8], full[:, 8 + cols:]))


def _report(name, bound, err):
    used = err / bound if bound > 0 else 0.0
    print(f"PARITY {name} bound={bound:.3e} err={err:.3e} used={used:.3f}")
    return used


# ---- top-k ----------------------------------------------------------------------------------------------------------
TOPK_OUT = (("top_val", torch.float32), ("top_idx", torch.int32), ("lse", torch.float32), ("rank", torch.int32),
            ("tgt_logit", torch.float32))


def _topk_launch(hip, xv, ncols, tgt, cnt, cap, k):
    """One launch into fresh sentinel-filled outputs: ({name: view}, margins intact)."""
    out, fulls = {}, {}
    for name, dtype in TOPK_OUT:
        n = cap * k if name in ("top_val", "top_idx") else cap
        fulls[name], out[name] = _flat(n, ar.TOPK_SENT, dtype)
    entry = "stonk_row_topk_f16" if xv.dtype == torch.float16 else "stonk_row_topk_f32"
    hip.call(entry, xv.data_ptr(), xv.stride(0), ncols, tgt.data_ptr(), cnt.data_ptr(), cap, k, out["top_val"].data_ptr(),
             out["top_idx"].data_ptr(), out["lse"].data_ptr(), out["rank"].data_ptr(), out["tgt_logit"].data_ptr(),
             hip.stream_ptr())
    torch.cuda.synchronize()
    ok = all(_flat_ok(fulls[name], out[name].numel(), ar.TOPK_SENT) for name in out)
    out["top_val"], out["top_idx"] = out["top_val"].view(cap, k), out["top_idx"].view(cap, k)
    return {n: v.cpu() for n, v in out.items()}, ok


def _topk_check(label, out, exp, count, k):
    assert torch.equal(out["top_idx"][:count], exp["si"][:, :k]), label
    assert torch.equal(out["top_val"][:count], exp["sv"][:, :k]), label
    assert torch.equal(out["rank"][:count], exp["rank"]), label
    assert torch.equal(out["tgt_logit"][:count], exp["tgt"]), label
    lse, ref = out["lse"][:count].double(), exp["lse"]
    err = float(((lse - ref).abs() / ref.abs()).max())
    _report(f"topk {label} lse (relative, |lse| >= {float(ref.abs().min()):.2f})", 1e-5, err)
    assert torch.isfinite(lse).all() and err <= 1e-5, label
    for name in out:                                       # rows at or past the count are not written
        assert (out[name][count:] == ar.TOPK_SENT).all(), (label, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", ["trips", "instances", "special", "sweep"])
def test_row_topk_against_float64(hip, name, dtype):
    cap, count, ncols, ld, ks = ar.TOPK_CASES[name]
    x, tgt = ar.topk_inputs(name, dtype)
    exp = ar.topk_expected(name, dtype)
    full, flat = _flat(cap * ld, NAN, dtype)
    xv = flat.view(cap, ld)
    xv.copy_(x)
    before = full.clone()
    tgt_d = tgt.cuda()
    cnt = torch.tensor([count], device="cuda", dtype=torch.int32)
    assert xv.data_ptr() % 16 == 0
    for k in ks:
        label = f"{name} {'f16' if dtype == torch.float16 else 'f32'} k={k} KC={ar.kc_of(k)}"
        out, ok = _topk_launch(hip, xv, ncols, tgt_d, cnt, cap, k)
        _topk_check(label, out, exp, count, k)
        assert ok, label
        again, ok = _topk_launch(hip, xv, ncols, tgt_d, cnt, cap, k)
        for n in out:                                      # the same input gives the same bits
            assert torch.equal(_bits(out[n]), _bits(again[n])), (label, n)
        assert ok, label
    assert torch.equal(_bits(full), _bits(before))        # the logits are read only


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_row_topk_from_a_misaligned_base(hip, dtype):
    cap, count, ncols, ld, ks = ar.TOPK_CASES["misaligned"]
    x, tgt = ar.topk_inputs("misaligned", dtype)
    exp = ar.topk_expected("misaligned", dtype)
    views = []
    for shift in (0, 1):
        full, flat = _flat(cap * ld, NAN, dtype, shift=shift)
        xv = flat.view(cap, ld)
        xv.copy_(x)
        views.append(xv)
    assert views[0].data_ptr() % 16 == 0 and views[1].data_ptr() % 16 == x.element_size() and ld * x.element_size() % 16 == 0
    tgt_d = tgt.cuda()
    cnt = torch.tensor([count], device="cuda", dtype=torch.int32)
    for k in ks:
        label = f"misaligned {'f16' if dtype == torch.float16 else 'f32'} k={k}"
        outs = []
        for xv in views:
            out, ok = _topk_launch(hip, xv, ncols, tgt_d, cnt, cap, k)
            _topk_check(label, out, exp, count, k)
            assert ok, label
            outs.append(out)
        for n in ("top_val", "top_idx", "rank", "tgt_logit"):
            assert torch.equal(_bits(outs[0][n]), _bits(outs[1][n])), (label, n)
        print(f"PARITY topk {label}: lse differs from the aligned launch in "
              f"{int((_bits(outs[0]['lse']) != _bits(outs[1]['lse'])).sum())} of {count} rows (another summation order)")
        again, _ = _topk_launch(hip, views[1], ncols, tgt_d, cnt, cap, k)
        for n in again:
            assert torch.equal(_bits(outs[1][n]), _bits(again[n])), (label, n)


# ---- input attribution ----------------------------------------------------------------------------------------------
def _attr_device(name):
    c = ar.attr_inputs(name)
    B, S, half, H = c["B"], c["S"], c["half"], c["H"]
    d = dict(c)
    d["ld"] = H + 24
    d["dsum_f"], d["dsum_v"] = _framed(B * S, H, d["ld"], NAN, torch.bfloat16, src=c["dsum"].cuda())
    d["text_f"], d["text_v"] = _flat(c["text"].numel(), NAN, torch.bfloat16)
    d["text_v"].copy_(c["text"].reshape(-1))
    d["kg_f"], d["kg_v"] = _flat(c["kg"].numel(), NAN)
    d["kg_v"].copy_(c["kg"].reshape(-1))
    d["ids_d"], d["rop_d"] = c["ids"].cuda().contiguous(), c["row_of_pos"].cuda()
    return d


def _attr_run(hip, d, layout, want_grad):
    B, S, half, H = d["B"], d["S"], d["half"], d["H"]
    n = B * S
    gxi_f, gxi = _flat(n, NAN)
    gn_f, gn = _flat(n, NAN)
    ld_out = H + 16
    grad_f, grad = _framed(n, H, ld_out, NAN, torch.float32) if want_grad else (None, None)
    hip.call("stonk_input_attribution", d["dsum_v"].data_ptr(), d["ld"], d["ids_d"].data_ptr(), d["text_v"].data_ptr(),
             d["kg_v"].data_ptr(), ar.ATTR_KG_ROWS, d["rop_d"].data_ptr() if layout == "packed" else 0, ar.ATTR_SCALE,
             gxi.data_ptr(), gn.data_ptr(), hip.ptr(grad), ld_out if want_grad else 0, B, S, half, H, hip.stream_ptr())
    torch.cuda.synchronize()
    ok = _flat_ok(gxi_f, n, NAN) and _flat_ok(gn_f, n, NAN) and (not want_grad or _framed_ok(grad_f, H, NAN))
    return gxi.cpu(), gn.cpu(), (grad.cpu() if want_grad else None), ok


@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("name", list(ar.ATTR_CASES))
def test_input_attribution_against_float64(hip, name, layout):
    d = _attr_device(name)
    r = ar.attr_reference(name, layout)
    live, dead = r["live"], ~r["live"]
    S, half = d["S"], d["half"]
    operands = [d[k].clone() for k in ("dsum_f", "text_f", "kg_f")]
    gxi, gn, grad, ok = _attr_run(hip, d, layout, True)
    label = f"attribution {name} {layout}"
    assert ok, label
    err = (gxi.double() - r["gxi"]).abs()
    used = float((err[live] / (1e-5 * r["gx"][live]).clamp(min=1e-300)).max())
    print(f"PARITY {label} grad_x_input used={used:.3f} of 1e-5 |g||x|")
    assert torch.isfinite(gxi).all() and bool((err <= 1e-5 * r["gx"]).all()), label
    rel = float(((gn.double() - r["gn"]).abs()[live] / r["gn"][live]).max())
    _report(f"{label} grad_norm (relative)", 1e-6, rel)
    assert torch.isfinite(gn).all() and rel <= 1e-6, label
    relg = float(((grad.double() - r["g"]).abs() / r["g"].abs().clamp(min=1e-300)).max())
    _report(f"{label} grad_out (relative)", 1e-6, relg)
    assert bool(((grad.double() - r["g"]).abs() <= 1e-6 * r["g"].abs()).all()), label
    if layout == "packed":                                 # dropped positions: exactly 0, everywhere
        assert int(dead.sum()) > 20
        assert float(gxi[dead].abs().max()) == 0.0 and float(gn[dead].abs().max()) == 0.0 and float(grad[dead].abs().max()) == 0.0
    if half < S:                                           # ids -1, -(1 << 40) and kg_rows: x counts as 0, the gradient is there
        bad = slice(S - 4, S - 1)
        assert bool((gxi[bad] == 0).all()) and bool((gn[bad] > 0).all()) and float(gxi[S - 1]) != 0.0
    plain = _attr_run(hip, d, layout, False)
    again = _attr_run(hip, d, layout, True)
    assert plain[3] and again[3]
    assert torch.equal(_bits(gxi), _bits(plain[0])) and torch.equal(_bits(gn), _bits(plain[1]))    # with or without grad_out
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((gxi, gn, grad), again[:3]))          # bitwise repeatable
    assert all(torch.equal(_bits(d[k]), _bits(o)) for k, o in zip(("dsum_f", "text_f", "kg_f"), operands))


# ---- attention probabilities ----------------------------------------------------------------------------------------
def _probs_run(hip, c, qv, kv, mask, want_p=True, want_m=True):
    B, NH, S = c["B"], c["NH"], c["S"]
    n_p, n_m = B * NH * S * S, B * NH * S * 2
    p_f, p = _flat(n_p, NAN) if want_p else (None, None)
    m_f, m = _flat(n_m, NAN) if want_m else (None, None)
    hip.call("stonk_attention_probs", qv.data_ptr(), kv.data_ptr(), qv.stride(0), mask.data_ptr(), hip.ptr(p), hip.ptr(m),
             B, NH, S, 64, c["half"], c["scale"], hip.stream_ptr())
    torch.cuda.synchronize()
    ok = (not want_p or _flat_ok(p_f, n_p, NAN)) and (not want_m or _flat_ok(m_f, n_m, NAN))
    return (p.view(B, NH, S, S) if want_p else None), (m.view(B, NH, S, 2) if want_m else None), ok


@pytest.mark.parametrize("name", list(ar.PROBS_CASES))
def test_attention_probs_against_float64(hip, name):
    c = ar.probs_inputs(name)
    B, NH, S = c["B"], c["NH"], c["S"]
    (p64, m64), (p32, m32) = ar.probs_expected(name)
    ld = NH * 64 + 16
    q_f, qv = _framed(B * S, NH * 64, ld, NAN, torch.bfloat16, src=c["q"].cuda())      # two allocations, NaN around the views
    k_f, kv = _framed(B * S, NH * 64, ld, NAN, torch.bfloat16, src=c["k"].cuda())
    operands = (q_f.clone(), k_f.clone())
    mask = c["key_mask"].cuda()
    p, m, ok = _probs_run(hip, c, qv, kv, mask)
    assert ok, name
    p2, m2, ok = _probs_run(hip, c, qv, kv, mask)
    assert ok and torch.equal(_bits(p), _bits(p2)) and torch.equal(_bits(m), _bits(m2))       # bitwise from run to run
    del p2
    none, m3, ok = _probs_run(hip, c, qv, kv, mask, want_p=False)
    assert ok and none is None and torch.equal(_bits(m), _bits(m3))                          # the two output modes: one mass
    p3, none, ok = _probs_run(hip, c, qv, kv, mask, want_m=False)
    assert ok and none is None and torch.equal(_bits(p), _bits(p3))
    del p3
    assert torch.equal(_bits(q_f), _bits(operands[0])) and torch.equal(_bits(k_f), _bits(operands[1]))
    p, m = p.cpu(), m.cpu()
    # structure first: a masked key is exactly 0.0, a single live key exactly 1.0
    dead = (c["key_mask"] == 0)[:, None, None, :].expand_as(p)
    assert float(p[dead].abs().max()) == 0.0, name
    if c["mask"] == "sparse":
        one = p[0, ..., ar.ONE_LIVE_KEY]
        print(f"PARITY probs {name}: single live key, {int((one != 1.0).sum())} of {one.numel()} rows are not exactly 1.0 "
              f"(largest |p - 1| = {float((one - 1.0).abs().max()):.3e})")
        assert bool((one == 1.0).all()), name
        assert bool((m[0, ..., 1] == 1.0).all()) and bool((m[0, ..., 0] == 0.0).all())
        assert bool((m[1, ..., 0] == 0.0).all()) and bool((m[2, ..., 1] == 0.0).all())           # a half without a live key
    pu.check_f32(f"probs {name} P", p, p64, p32)
    rel32, rel = ar.probs_rel(p32, p64), ar.probs_rel(p, p64)
    used = _report(f"probs {name} P relative above {ar.PROBS_FLOOR:g} (r32 relative {rel32:.3e}, kernel / r32 = "
                   f"{rel / rel32:.2f})", ar.PROBS_REL_FACTOR * rel32, rel)
    assert used <= 1.0, name
    pu.check_f32(f"probs {name} modal mass", m, m64, m32)


# ---- word-embedding gradient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("name", list(ar.WEG_CASES))
def test_word_embed_grad_against_float64(hip, name, packed):
    c = ar.weg_inputs(name, packed)
    B, S, H, vocab, table = c["B"], c["S"], c["H"], c["vocab"], c["table"]
    ids_d, dsum_d = c["ids"].cuda().contiguous(), c["dsum"].cuda()
    rop_d = None if c["row_of_pos"] is None else c["row_of_pos"].cuda()
    for padding_idx in (0, -1):
        tab_d = table.clone().cuda()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        hip.call("stonk_word_embed_grad", dsum_d.data_ptr(), c["ld"], ids_d.data_ptr(), hip.ptr(rop_d), tab_d[1].data_ptr(),
                 c["ld_w"], vocab, padding_idx, B, S, H, err.data_ptr(), hip.stream_ptr())
        torch.cuda.synchronize()
        got = tab_d.cpu()
        ref, mag, count = ar.weg_reference(c, padding_idx)
        assert int(err.item()) == 0
        body = got[1:vocab + 1, :H]
        # n additions onto the preset, each within 2^-24 of a partial sum that |preset| + sum |contribution| bounds, in any
        # arrival order; a factor of two on top (test_word_embed_grad_gpu.py's bound)
        bound = count[:, None].double() * 2.0 ** -23 * mag
        diff = (body.double() - ref).abs()
        touched = count > 0
        used = float((diff[touched] / bound[touched]).max())
        print(f"PARITY word_embed_grad {name} {'packed' if packed else 'padded'} pad={padding_idx} "
              f"max_err={float(diff.max()):.3e} hot row n={int(count[ar.WEG_HOT])} used={used:.3f} of n 2^-23 magnitude")
        assert torch.isfinite(body).all() and bool((diff <= bound).all())
        assert torch.equal(_bits(body[~touched]), _bits(table[1:vocab + 1, :H][~touched]))         # bit-identical
        assert torch.equal(_bits(got[:, H:]), _bits(table[:, H:]))                                 # the columns past H
        assert torch.equal(_bits(got[0]), _bits(table[0])) and torch.equal(_bits(got[vocab + 1]), _bits(table[vocab + 1]))


# ---- row movers -----------------------------------------------------------------------------------------------------
def _mover_src(n_src, cols, ld_src, seed, dtype=torch.bfloat16):
    src = (torch.randn(n_src, cols, generator=ar.gen(seed)) * 3.0).to(dtype)
    full, view = _framed(n_src, cols, ld_src, NAN, dtype, src=src.cuda())
    return src, full, view


def _gather(hip, src_v, rows_d, count, cap, n_dst, cols, ld_dst):
    dst_f, dst = _framed(n_dst, cols, ld_dst, FRAME, torch.bfloat16, inner=ar.MOVER_FILL)
    cnt = torch.tensor([count], device="cuda", dtype=torch.int32)
    hip.call("stonk_gather_rows_bf16", src_v.data_ptr(), src_v.stride(0), rows_d.data_ptr(), cnt.data_ptr(), dst.data_ptr(),
             ld_dst, cols, cap, hip.stream_ptr())
    torch.cuda.synchronize()
    return dst.cpu(), _framed_ok(dst_f, cols, FRAME)


def _scatter(hip, src_v, rows_d, count, n_dst, cols, ld_dst):
    dst_f, dst = _framed(n_dst, cols, ld_dst, FRAME, torch.bfloat16, inner=ar.MOVER_FILL)
    cnt = torch.tensor([count], device="cuda", dtype=torch.int32)
    entry = "stonk_scatter_rows_bf16" if src_v.dtype == torch.bfloat16 else "stonk_scatter_rows_f32_to_bf16"
    hip.call(entry, src_v.data_ptr(), src_v.stride(0), rows_d.data_ptr(), cnt.data_ptr(), dst.data_ptr(), ld_dst, cols,
             hip.stream_ptr())
    torch.cuda.synchronize()
    return dst.cpu(), _framed_ok(dst_f, cols, FRAME)


def test_gather_and_scatters_beyond_one_trip_of_the_grid(hip):
    t = ar.MOVER_TRIPS
    n_src, count, cap, cols, ld_src, ld_dst = (t[k] for k in ("n_src", "count", "cap", "cols", "ld_src", "ld_dst"))
    rows = ar.mover_rows(n_src, cap + 100, 5)                    # a list longer than the count (and than the capacity)
    rows_d = rows.cuda()
    src, src_f, src_v = _mover_src(n_src, cols, ld_src, 6)
    before = src_f.clone()
    want = ar.gather_reference(src, rows, count, cap, cap + 4, cols)
    for _ in range(2):
        got, ok = _gather(hip, src_v, rows_d, count, cap, cap + 4, cols, ld_dst)
        assert ok and torch.equal(_bits(got), _bits(want))       # moved, zero-filled and untouched rows, bit for bit
    assert float(want[count:cap].abs().max()) == 0.0 and bool((want[cap:] == ar.MOVER_FILL).all())
    for dtype in (torch.bfloat16, torch.float32):
        s_src, s_f, s_v = _mover_src(cap, cols, ld_src, 7, dtype)
        want = ar.scatter_reference(s_src, rows, count, n_src, cols)
        for _ in range(2):
            got, ok = _scatter(hip, s_v, rows_d, count, n_src, cols, ld_dst)
            assert ok and torch.equal(_bits(got), _bits(want)), dtype
    assert torch.equal(_bits(src_f), _bits(before))


@pytest.mark.parametrize("cap", ar.MOVER_CAPS)
@pytest.mark.parametrize("count", ar.MOVER_COUNTS)
def test_gather_clamp_and_strides(hip, count, cap):
    s = ar.MOVER_SMALL
    n_src, cols, ld_src, ld_dst = s["n_src"], s["cols"], s["ld_src"], s["ld_dst"]
    rows = ar.mover_rows(n_src, 256, 11)
    rows_d = rows.cuda()
    src, src_f, src_v = _mover_src(n_src, cols, ld_src, 12)
    n_dst = 260
    want = ar.gather_reference(src, rows, count, cap, n_dst, cols)
    lim = ar.gather_lim(count, cap)
    assert bool((want[lim:] == ar.MOVER_FILL).all()) and (lim == count or float(want[count:lim].abs().max()) == 0.0)
    for _ in range(2):
        got, ok = _gather(hip, src_v, rows_d, count, cap, n_dst, cols, ld_dst)
        assert ok and torch.equal(_bits(got), _bits(want))
    for dtype in (torch.bfloat16, torch.float32):
        s_src, s_f, s_v = _mover_src(256, cols, ld_src, 13, dtype)
        want = ar.scatter_reference(s_src, rows, count, n_src, cols)
        for _ in range(2):
            got, ok = _scatter(hip, s_v, rows_d, count, n_src, cols, ld_dst)
            assert ok and torch.equal(_bits(got), _bits(want)), dtype


@pytest.mark.parametrize("name", list(ar.COMPACT_CASES))
def test_label_compact_for_both_decoders(hip, name):
    B, half, S, frac = ar.COMPACT_CASES[name]
    labels, row_map = ar.compact_labels(name)
    labels_d, map_d = labels.cuda(), row_map.cuda()
    n = B * half
    for offset in (0, half):                                     # the text decoder / the entity decoder
        for rmap, rmap_d in ((None, None), (row_map, map_d)):
            want_rows, want_tg = ar.compact_reference(labels, half, S, offset, rmap)
            c = len(want_rows)
            results = []
            for _ in range(2):
                rows_f, rows = _flat(n, -1, torch.int32)
                tg_f, tg = _flat(n, -1, torch.int32)
                cnt = torch.full((1,), -5, device="cuda", dtype=torch.int32)
                hip.call("stonk_label_compact", labels_d.data_ptr(), n, half, S, offset, rows.data_ptr(), tg.data_ptr(),
                         cnt.data_ptr(), hip.ptr(rmap_d), hip.stream_ptr())
                torch.cuda.synchronize()
                assert _flat_ok(rows_f, n, -1) and _flat_ok(tg_f, n, -1)
                results.append((rows.cpu(), tg.cpu(), int(cnt.item())))
            rows, tg, got_c = results[0]
            assert got_c == c and torch.equal(rows[:c], want_rows) and torch.equal(tg[:c], want_tg), (offset, rmap is None)
            assert bool((rows[c:] == -1).all()) and bool((tg[c:] == -1).all())
            assert torch.equal(rows, results[1][0]) and torch.equal(tg, results[1][1]) and results[1][2] == c
