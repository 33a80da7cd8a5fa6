"""GPU: stonk_input_attribution against fp64 torch on the same bf16 / fp32 inputs - padded and packed layout, ld > H,
special and out-of-table entity ids, a negative scale, with and without the gradient output, each scalar output alone,
exact zeros on dropped positions, and bitwise repeatability.

Bounds (the inputs are identical on both sides, the sums are fp32 sums of at most 1024 products):
|d grad_x_input| <= 1e-5 |g| |x| per position; grad_norm and grad_out relative 1e-6."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S, HALF, SCALE = 3, 256, 128, -19.0
KG_ROWS = 333


def _row_plan():
    """A hand-made packed layout: about a third of the text positions dropped, in runs of which some start or end at a
    sequence boundary; position 0 of every sequence and every entity position kept."""
    keep = torch.ones(B, S, dtype=torch.bool)
    keep[0, 86:128] = False            # a run that ends at the boundary of the text half
    keep[1, 1:40] = False              # a run that starts right behind position 0
    keep[1, 90:97] = False
    keep[2, 50:91] = False
    keep[2, 127] = False               # a single position at the end of the half
    flat = keep.flatten()
    row_of_pos = torch.full((B * S,), -1, dtype=torch.int32)
    row_of_pos[flat] = torch.arange(int(flat.sum()), dtype=torch.int32)
    assert 0.30 < float((~keep[:, :HALF]).float().mean()) < 0.37 and bool(keep[:, 0].all())
    return keep, row_of_pos


@pytest.fixture(scope="module", params=[128, 768, 1024])
def case(request, hip):
    """Inputs on the device and the fp64 reference, computed once per width and left unchanged."""
    H = request.param
    g = torch.Generator().manual_seed(1000 + H)
    ld = H + 24
    dsum = (torch.randn(B * S, ld, generator=g) * 0.05).to(torch.bfloat16)
    text = torch.randn(B * HALF, H, generator=g).to(torch.bfloat16)
    kg = torch.randn(KG_ROWS, H, generator=g) * 0.3
    ids = torch.randint(0, KG_ROWS, (B, S), generator=g)
    ids[0, HALF:HALF + 4] = torch.tensor([100, 102, 103, KG_ROWS - 1])
    ids[2, S - 1] = KG_ROWS            # outside the table
    keep, row_of_pos = _row_plan()
    ref = {}
    for layout in ("padded", "packed"):
        rows = torch.arange(B * S) if layout == "padded" else row_of_pos.long()
        live = rows >= 0
        gd = torch.zeros(B * S, H, dtype=torch.float64)
        gd[live] = SCALE * dsum[rows[live], :H].double()
        x = torch.cat([text.double().view(B, HALF, H), kg.double()[ids[:, HALF:].clamp(max=KG_ROWS - 1)]], 1).view(B * S, H)
        x[2 * S + S - 1] = 0.0         # the out-of-table id counts as x = 0
        ref[layout] = dict(live=live, g=gd, gxi=(gd * x).sum(1), gn=gd.norm(dim=1), gx=gd.norm(dim=1) * x.norm(dim=1))
    dev = {k: v.cuda() for k, v in dict(dsum=dsum, text=text, kg=kg, ids=ids, row_of_pos=row_of_pos).items()}
    return dict(H=H, ld=ld, dev=dev, ref=ref, hip=hip)


def _run(c, layout, want_gxi=True, want_gn=True, want_grad=False):
    H, d = c["H"], c["dev"]
    gxi = torch.full((B * S,), float("nan"), device="cuda") if want_gxi else None
    gn = torch.full((B * S,), float("nan"), device="cuda") if want_gn else None
    ld_out = H + 8
    grad = torch.full((B * S, ld_out), float("nan"), device="cuda") if want_grad else None
    hip = c["hip"]
    hip.call("stonk_input_attribution", d["dsum"].data_ptr(), c["ld"], d["ids"].data_ptr(), d["text"].data_ptr(),
             d["kg"].data_ptr(), KG_ROWS, d["row_of_pos"].data_ptr() if layout == "packed" else 0, SCALE, hip.ptr(gxi),
             hip.ptr(gn), hip.ptr(grad), ld_out if want_grad else 0, B, S, HALF, H, hip.stream_ptr())
    torch.cuda.synchronize()
    return gxi, gn, grad


def _check(c, layout, gxi, gn, grad):
    r = c["ref"][layout]
    live, dead = r["live"], ~r["live"]
    if gxi is not None:
        err = (gxi.cpu().double() - r["gxi"]).abs()
        print(f"H {c['H']} {layout}: max |d grad_x_input| / (|g||x|) = {float((err[live] / r['gx'][live].clamp(min=1e-30)).max()):.2e}")
        assert bool((err <= 1e-5 * r["gx"]).all())
        assert float(gxi.cpu()[dead].abs().max()) == 0.0 if bool(dead.any()) else True
        assert float(gxi[2 * S + S - 1]) == 0.0                       # the out-of-table id
    if gn is not None:
        rel = (gn.cpu().double() - r["gn"]).abs()[live] / r["gn"][live]
        print(f"H {c['H']} {layout}: max relative grad_norm error {float(rel.max()):.2e}")
        assert float(rel.max()) <= 1e-6
        assert float(gn.cpu()[dead].abs().max()) == 0.0 if bool(dead.any()) else True
        assert float(gn[2 * S + S - 1]) > 0.0                         # ... still has a gradient, and the right norm (above)
    if grad is not None:
        got = grad[:, :c["H"]].cpu().double()
        assert bool(((got - r["g"]).abs() <= 1e-6 * r["g"].abs()).all())
        assert float(got[dead].abs().max()) == 0.0 if bool(dead.any()) else True
        assert bool(torch.isnan(grad[:, c["H"]:]).all())              # nothing is written past H


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_against_fp64(case, layout):
    assert layout == "padded" or int((~case["ref"]["packed"]["live"]).sum()) > 100
    full = _run(case, layout, want_grad=True)
    _check(case, layout, *full)
    plain = _run(case, layout)
    _check(case, layout, *plain)
    # the scalar outputs do not depend on whether the gradient is written, and two runs give the same bits
    assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1])
    again = _run(case, layout, want_grad=True)
    assert all(torch.equal(a, b) for a, b in zip((full[0], full[1], full[2][:, :case["H"]]),
                                                 (again[0], again[1], again[2][:, :case["H"]])))
    # each scalar output alone
    only_gxi = _run(case, layout, want_gn=False)
    only_gn = _run(case, layout, want_gxi=False, want_grad=True)
    assert only_gxi[1] is None and torch.equal(only_gxi[0], full[0])
    assert only_gn[0] is None and torch.equal(only_gn[1], full[1]) and torch.equal(only_gn[2][:, :case["H"]],
                                                                                  full[2][:, :case["H"]])
