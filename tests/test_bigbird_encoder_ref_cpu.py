"""The BigBird encoder restatement (tests/bigbird_encoder_ref.py) without a GPU: against HuggingFace's own BigBirdModel in
float64, against the committed float32 fixtures, gelu_new and its derivative against torch autograd, and the two mutants
that the GPU tests must be able to tell from the feature.

Measured here (float64 restatement, relative norm of the difference to HuggingFace's float32 fixture, sequence output at
the fixture's rows / at the masked-query rows alone), next to the GPU bound 2 ||r16 - r|| / ||r||, about 1.2e-2:

    without the masked-query zeroing   3.3e-1 / 3.6e-1   twenty-seven to thirty times the bound
    erf GELU instead of gelu_new       3.1e-2 (s768), 2.9e-2 (s1024)      2.5 times the bound

The second margin exists because of the TAIL units of bigbird_encoder_ref.init_state_dict: with ordinary weights alone the
two activations differ by at most 4.7e-4 absolute where one bf16 rounding of their value is 2e-3 to 4e-3, and the erf
mutant is 1.7e-4 away - sixty times BELOW the bound, invisible to any test made of bf16 rounding points. Pre-activations
around -4.5, where the two forms differ by a factor of three, carried by large output weights, make the form of the
activation visible at the encoder's outputs."""
import numpy as np
import pytest
import torch

from tests import bigbird_encoder_ref as er


def _rows(c, t):
    return t.reshape(-1, c["hidden"])[er.sample_rows(c)]


@pytest.mark.parametrize("name,mode", [("s768", "eval"), ("s768", "train"), ("s1024", "eval"), ("s1024", "train")])
def test_float64_restatement_is_huggingfaces_model(name, mode):
    """hidden 128, 2 heads, 2 layers, B 2; masked positions inside a block, across a whole inner block, in block 0 and in
    block nb - 1. Every output within 1e-10 relative; the plans HuggingFace used are the fixture's."""
    pytest.importorskip("transformers")
    c = er.CASES[name]
    hf = er.huggingface_run(name, mode, torch.float64)
    plans = er.fixture_plans(er.load_fixture(name), mode)
    assert all(np.array_equal(a, b) for a, b in zip(hf["plans"], plans))
    r = er.reference(name, mode, "r64")
    m = c["mask"]
    nb = c["nb"]
    blocks = (m == 0).view(c["B"], nb, 64)
    assert bool(blocks[:, 0].any()) and bool(blocks[:, nb - 1].any()), "masked rows in block 0 and in block nb - 1"
    assert bool(blocks[:, 1:nb - 1].all(-1).any()), "a whole inner block masked"
    assert bool((blocks.any(-1) & ~blocks.all(-1))[:, 1:nb - 1].any()), "masked positions inside an inner block"
    figures = {"seq": er.rel(r["seq"], hf["seq"]), "pooled": er.rel(r["pooled"], hf["pooled"])}
    for k, g in hf["grads"].items():
        figures["grad." + k] = er.rel(r["grads"][k], g)
    print(f"HF-AGREEMENT {name} {mode}: " + " ".join(f"{k}={v:.1e}" for k, v in figures.items()))
    assert max(figures.values()) <= 1e-10, figures


@pytest.mark.parametrize("name", ["s768", "s1024"])
def test_masked_query_rows_are_what_a_zero_context_gives(name):
    """The claim of the feature, without a GPU: HuggingFace's context row of a masked query is exactly zero, so the first
    layer's output there is LayerNorm-FFN of (attention-output bias + the layer's input) - and NOT what the list
    formulation's row gives."""
    pytest.importorskip("transformers")
    c = er.CASES[name]
    sd, x, tt, _ = er.case_data(name)
    cfg = {**er.config_dict(c), "num_hidden_layers": 1}
    plans = er.fixture_plans(er.load_fixture(name), "eval")[:1]
    one = {k: v for k, v in sd.items() if not k.startswith("encoder.layer.1.")}
    got = er.encoder(one, cfg, x, c["mask"], tt, plans, "r64")["seq"].reshape(-1, c["hidden"])
    masked = c["mask"].view(-1) == 0
    # the same layer with every context row forced to zero: value weights and bias zero
    zero_ctx = dict(one)
    zero_ctx["encoder.layer.0.attention.self.value.weight"] = torch.zeros_like(sd["encoder.layer.0.attention.self.value.weight"])
    zero_ctx["encoder.layer.0.attention.self.value.bias"] = torch.zeros_like(sd["encoder.layer.0.attention.self.value.bias"])
    want = er.encoder(zero_ctx, cfg, x, c["mask"], tt, plans, "r64")["seq"].reshape(-1, c["hidden"])
    assert torch.equal(got[masked], want[masked])
    mutant = er.encoder(one, cfg, x, c["mask"], tt, plans, "r64", zero_masked_queries=False)["seq"].reshape(-1, c["hidden"])
    assert torch.equal(mutant[~masked], got[~masked])          # one layer: live rows cannot tell
    assert er.rel(mutant[masked], got[masked]) > 0.1


@pytest.mark.parametrize("name,mode", [(n, m) for n in er.CASES for m in er.case_modes(n)])
def test_restatement_meets_the_committed_fixture(name, mode):
    """Without `transformers`: the float64 restatement against HuggingFace's float32 numbers in tests/golden, within what
    that float32 run may be off by itself (bigbird_encoder_ref.HF_FLOAT32_ERROR, derived there; test_float64_restatement_is_
    huggingfaces_model holds the float64 run to 1e-10), and the data the fixture was made from is the data regenerated here."""
    c = er.CASES[name]
    fx = er.load_fixture(name)
    assert fx["meta"]["data_sha256"] == er.data_checksum(name), "the seeded weights / inputs are not the fixture's"
    assert np.array_equal(fx["arrays"]["mask"], c["mask"].numpy())
    A = fx["arrays"]
    r = er.reference(name, mode, "r64")
    H = c["hidden"]
    fig = {"seq": er.rel(_rows(c, r["seq"]), torch.from_numpy(A[f"{mode}.seq"])),
           "pooled": er.rel(r["pooled"], torch.from_numpy(A[f"{mode}.pooled"])),
           "grad.inputs_embeds": er.rel(r["grads"]["inputs_embeds"].reshape(-1, H)[er.grad_rows(c)],
                                        torch.from_numpy(A[f"{mode}.grad.inputs_embeds"]))}
    for k in er.grad_names(c):
        g = r["grads"][k]
        g = g[:c["S"]] if k == "embeddings.position_embeddings.weight" else g
        fig["grad." + k] = er.rel(er.grad_sample(g), torch.from_numpy(A[f"{mode}.grad.{k}"]))
    masked = c["mask"].view(-1)[er.sample_rows(c)] == 0
    assert int(masked.sum()) == int((c["mask"] == 0).sum())      # every masked-query row is in the fixture
    fig["seq.masked_query_rows"] = er.rel(_rows(c, r["seq"])[masked], torch.from_numpy(A[f"{mode}.seq"])[masked])
    print(f"FIXTURE {name} {mode}: " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    assert max(fig.values()) <= er.HF_FLOAT32_ERROR, fig


def _gpu_bound(name, mode, rows=None):
    """2 ||r16 - r|| / ||r|| of the sequence output (at `rows` of [B*S]): what tests/test_bigbird_encoder_gpu.py allows."""
    c = er.CASES[name]
    r, r16 = er.reference(name, mode, "r64"), er.reference(name, mode, "r16")
    a, b = r16["seq"].reshape(-1, c["hidden"]), r["seq"].reshape(-1, c["hidden"])
    if rows is not None:
        a, b = a[rows], b[rows]
    return 2.0 * er.rel(a, b)


def _mutant_distance(name, mode, rows=None, **kw):
    c = er.CASES[name]
    A = er.load_fixture(name)["arrays"]
    keep = er.sample_rows(c)
    m = _rows(c, er.reference(name, mode, "r64", **kw)["seq"])
    hf = torch.from_numpy(A[f"{mode}.seq"])
    if rows is not None:
        m, hf = m[rows[keep]], hf[rows[keep]]
    return er.rel(m, hf)


@pytest.mark.parametrize("name", ["s768", "s1024"])
def test_mutant_without_the_zeroing_misses_the_fixtures_by_more_than_the_gpu_bound(name):
    masked = er.CASES[name]["mask"].view(-1) == 0
    for rows, what in ((None, "the fixture's rows"), (masked, "the masked-query rows")):
        d, bound = _mutant_distance(name, "eval", rows, zero_masked_queries=False), _gpu_bound(name, "eval", rows)
        print(f"MUTANT no-zeroing {name} on {what}: distance {d:.3e}, GPU bound {bound:.3e}, margin x{d / bound:.1f}")
        assert d > 4.0 * bound


@pytest.mark.parametrize("name", ["s768", "s1024"])
def test_erf_gelu_mutant_misses_the_fixtures_by_more_than_the_gpu_bound(name):
    """(the margin comes from the tail units of the seeded weights: see the module docstring)"""
    d, bound = _mutant_distance(name, "eval", act="gelu"), _gpu_bound(name, "eval")
    print(f"MUTANT erf-gelu {name}: distance {d:.3e}, GPU bound {bound:.3e}, margin x{d / bound:.3f}")
    assert d > bound


# ------------------------------------------------------------------ gelu_new
def test_gelu_new_and_its_derivative_are_torchs_in_float64():
    u = torch.cat([torch.linspace(-12, 12, 4801, dtype=torch.float64),
                   torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1e-3, -1e-3, 1e4, -1e4, 1e20, -1e20, er.BF16_MAX, -er.BF16_MAX],
                                dtype=torch.float64)]).requires_grad_(True)
    ref = torch.nn.functional.gelu(u, approximate="tanh")
    ref.backward(torch.ones_like(ref))
    g, dg = er.gelu_new(u.detach()), er.gelu_new_grad(u.detach())
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(dg).all())
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(u.grad).all())      # (float64 holds bf16-max cubed)
    # per element, a few float64 roundings of max(1, |u|) (both forms cancel in 1 + tanh on the negative side)
    scale = u.detach().abs().clamp(min=1.0)
    assert float(((g - ref.detach()).abs() / scale).max()) <= 4e-16
    assert float(((dg - u.grad).abs() / scale).max()) <= 4e-15
    # the closed form stays finite in float32 as well, where the naive one is (1 - t^2) * inf = NaN
    big = torch.tensor([1e20, -1e20, er.BF16_MAX, -er.BF16_MAX], dtype=torch.float32)
    assert er.gelu_new_grad(big).tolist() == [1.0, 0.0, 1.0, 0.0]
    assert er.gelu_new(big).tolist() == [float(big[0]), 0.0, float(big[2]), 0.0]


def test_r16_differs_from_r_by_bf16_rounding_and_no_more():
    """The bound the GPU test uses is a bf16-sized one: 2 ||r16 - r|| / ||r|| between 2e-3 and 5e-2 for every output."""
    for name, mode in (("s768", "eval"), ("s768", "train")):
        r, r16 = er.reference(name, mode, "r64"), er.reference(name, mode, "r16")
        figs = {"seq": er.rel(r16["seq"], r["seq"]), "pooled": er.rel(r16["pooled"], r["pooled"])}
        figs.update({k: er.rel(r16["grads"][k], r["grads"][k]) for k in r["grads"]})
        print(f"R16 {name} {mode}: " + " ".join(f"{k}={v:.1e}" for k, v in figs.items()))
        assert all(1e-3 <= 2 * v <= 5e-2 for v in figs.values()), figs
