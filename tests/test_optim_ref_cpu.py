"""The optimizer reference (tests/optim_ref.py) without a GPU: adamw_ref in float64 IS torch.optim.AdamW with HF's two
parameter groups behind clip_grad_norm_; r32 - the same in float32 - goes through the kernel's checks in place of a
kernel's output for every case of test_optim_parity_gpu.py, so the tolerances are known to be satisfiable by a correctly
rounding fp32 implementation before a GPU is used; and the same checks refuse the two look-alike AdamW forms and small
localised errors."""
import pytest
import torch

from tests import optim_ref as orf
from tests import parity_util as pu


def test_adamw_ref_in_float64_is_torch_adamw_with_two_groups_behind_clip_grad_norm():
    index, numel = orf.layout()
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 0.01
    flat = torch.zeros(numel, dtype=torch.float64)
    params = {}
    for i, (name, (off, _, _, n)) in enumerate(index.items()):
        flat[off:off + n] = pu.randn(n, 100 + i, 0.05, dtype=torch.float64)
        params[name] = torch.nn.Parameter(flat[off:off + n].clone())
    decayed = [n for n in params if n.endswith(".weight") and "LayerNorm" not in n]
    opt = torch.optim.AdamW([{"params": [params[n] for n in decayed], "weight_decay": wd},
                             {"params": [params[n] for n in params if n not in decayed], "weight_decay": 0.0}],
                            lr=lr, betas=(b1, b2), eps=eps)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    for step in (1, 2, 3):
        g = torch.zeros_like(flat)
        for i, (name, (off, _, _, n)) in enumerate(index.items()):
            g[off:off + n] = pu.randn(n, 1000 * step + i, 0.02, dtype=torch.float64)
            params[name].grad = g[off:off + n].clone()
        assert float(g.norm()) > 2.0   # the clip is active
        torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
        opt.step()
        flat, m, v, g2, _ = orf.adamw_ref(flat, g, m, v, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, bc1=1 - b1 ** step, bc2=1 - b2 ** step,
                                          gnorm_sq=float((g * g).sum()), max_norm=1.0, decay_spans=orf.decay_spans(index))
        assert not g2.any()
        for name, (off, _, _, n) in index.items():
            st = opt.state[params[name]]
            for what, got, want in (("p", flat, params[name].detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
                err, peak = float((got[off:off + n] - want).abs().max()), float(want.abs().max())
                assert err <= 1e-12 * peak, (step, name, what, err, peak)
    gaps = orf.span_mask(numel, [(off, off + n) for off, _, _, n in index.values()]).logical_not()
    assert gaps.any() and not flat[gaps].any()       # (zero parameters and gradients between the tensors stay zero)


def _r32_as_kernel_output(r32):
    return tuple(x.to(torch.float32) for x in r32[:4]) + (r32[4],)


@pytest.mark.parametrize("name", list(orf.CASES))
def test_r32_satisfies_every_assertion(name):
    index, numel = orf.layout()
    (p, g, m, v, kw), r, r32 = orf.references(name, numel, orf.decay_spans(index))
    orf.check_step(name, g, _r32_as_kernel_output(r32), r, r32)
    # what the file promises about the inputs: (1 - b2) g~^2 is a normal fp32 number or exactly zero
    coef = kw["grad_scale"] * (1.0 if kw["gnorm_sq"] is None else min(1.0, kw["max_norm"] / (kw["gnorm_sq"] ** 0.5 * kw["grad_scale"] + 1e-6)))
    sq = (1.0 - orf.B2) * (g.double() * coef) ** 2
    assert ((sq == 0) | (sq >= 2.0 ** -126)).all() and (g == 0).any() == (orf.CASES[name]["state"] == "mixed")


def test_cases_cover_what_they_are_meant_to():
    c = list(orf.CASES.values())
    assert {x["step"] for x in c} == {1, 3, 100000} and orf.f32(1.0 - 0.9 ** 100000) == 1.0
    assert {x["clip"] for x in c} == {"off", "active", "loose", "below", "above"}
    assert {x["gs"] for x in c if x["clip"] == "active"} == {1.0, 0.5, 0.125}
    assert {x["gs"] for x in c if x["clip"] in ("below", "above")} == {1.0, 0.5, 0.125}
    assert {(x["wd"], x["table"]) for x in c} == {(0.0, False), (0.01, False), (0.01, True), (10.0, True)}
    assert {x["step"] for x in c if x["p"] == "zero"} == {1, 3, 100000}
    assert any(x["g"] == "wide" and x["state"] == "mixed" for x in c)
    # the two edge cases sit on either side of the clip: the reference's clip factor is below 1 on one, exactly 1 on the other
    for name, x in orf.CASES.items():
        if x["clip"] in ("below", "above"):
            kw = orf.inputs(name, 8)[4]
            total = kw["gnorm_sq"] ** 0.5 * kw["grad_scale"]
            assert abs(total - 1.0) < 1e-6 and (total < 1.0) == (x["clip"] == "below")
    index, numel = orf.layout()
    a, d, b = index["a.weight"], index["d.weight"], index["b.weight"]
    assert a[1][0] < a[2][0] and a[1][0] % 64 and b[1][1] % 64 and d[1][0] % 64 and d[1][1] % 64 and numel < 1 << 20
    assert any(off + n < nxt for (off, _, _, n), nxt in zip(index.values(), [v[0] for v in list(index.values())[1:]]))


@pytest.mark.parametrize("name,variant", [("long-step100000-wd10-table", "decay_after"), ("p0-first-step-clip", "eps_first")])
def test_check_refuses_the_look_alike_adamw_forms(name, variant):
    """Decay applied to the updated parameter instead of before the update; eps added before the division by sqrt(bc2)
    (the kernel and torch both add it after). Both in float32, as a kernel would compute them."""
    index, numel = orf.layout()
    (p, g, m, v, kw), r, r32 = orf.references(name, numel, orf.decay_spans(index))
    wrong = orf.adamw_ref(p, g, m, v, dtype=torch.float32, variant=variant, **kw)
    with pytest.raises(AssertionError):
        orf.check_step(name, g, _r32_as_kernel_output(wrong), r, r32)


def test_check_refuses_localised_errors():
    name = "long-step100000-wd10-table"
    index, numel = orf.layout()
    spans = orf.decay_spans(index)
    (p, g, m, v, kw), r, r32 = orf.references(name, numel, spans)
    lo, hi = spans[1]

    def refused(edit):
        got = [x.clone() for x in _r32_as_kernel_output(r32)]
        edit(got)
        with pytest.raises(AssertionError):
            orf.check_step(name, g, got, r, r32)

    def undecayed_last(got):       # the last element of a decayed span keeps its weight
        got[0][hi - 1] += p[hi - 1] * kw["lr"] * kw["wd"]

    def decayed_gap(got):          # the element behind it loses some
        got[0][hi] -= p[hi] * kw["lr"] * kw["wd"]

    def stale_mirror(got):
        got[4][lo] = p[lo].to(orf.BF16) * 2

    def grad_left(got):
        got[3][numel - 1] = g[numel - 1]

    def moment(got):               # v' with b2 v only: the gradient's square never arrived
        got[2][7] = orf.B2 * v[7]

    for edit in (undecayed_last, decayed_gap, stale_mirror, grad_left, moment):
        refused(edit)


def test_sumsq_bound_follows_the_grid():
    assert [orf.sumsq_grid(n) for n in (0, 1, 1024, 1027, 262147, 1050003)] == [1, 1, 1, 1, 256, 256]
    assert orf.sumsq_bound(262147)[0] == 2 and orf.sumsq_bound(1050003)[0] == 5 and orf.sumsq_bound(1024)[0] == 1
    assert 29 * 2.0 ** -24 <= orf.sumsq_bound(1050003)[1] < 29.001 * 2.0 ** -24
