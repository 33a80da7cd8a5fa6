"""BigBirdEncoderModel on the GPU against the fixtures of tools/make_bigbird_encoder_golden.py (HuggingFace's BigBirdModel,
float32, CPU) and the float64 restatement of tests/bigbird_encoder_ref.py, with HuggingFace's captured plans installed.

Per output - the sequence output, its masked-query rows alone, the pooled vector, d(inputs_embeds) and the named parameter
gradients of the fixed scalar - the project's rule of tests/bigbird_ref.py:  ||got - r|| / ||r|| <= 2 ||r16 - r|| / ||r||,
r16 = the restatement with the kernels' bf16 rounding points, computed here on the CPU. The masked-query rows are the rows
that tell the feature from the kernels without the zeroing: there the mutant is 0.35 away in relative norm, thirty times
the bound; an erf-GELU encoder is 3e-2 away on every output, 2.5 times the bound (test_bigbird_encoder_ref_cpu.py). Every figure is printed as a PARITY line before it is asserted
(profiles/bigbird_encoder.md collects them)."""
import pytest
import torch

from stonkgs_amd.bigbird_encoder import BigBirdEncoderConfig, BigBirdEncoderModel
from stonkgs_amd.stonkgs_pretraining import FusedAdamW
from tests import bigbird_encoder_ref as er

pytestmark = pytest.mark.gpu


def _model(name, **over):
    c = er.CASES[name]
    model = BigBirdEncoderModel(BigBirdEncoderConfig(**{**er.config_dict(c), **over}))
    model.load_state_dict(er.case_data(name)[0])
    return model


def _install(model, name, mode):
    model.train(mode == "train")
    for i, ra in enumerate(er.fixture_plans(er.load_fixture(name), mode)):
        model.set_rand_attn(i, ra)


def _step(model, name):
    """forward + loss.backward() of the fixed scalar; returns (seq, pooled, loss, grads) on the CPU."""
    c = er.CASES[name]
    _, x, tt, (w, wp) = er.case_data(name)
    xd = x.cuda().requires_grad_(True)
    model.zero_grad()
    seq, pooled = model(xd, c["mask"].cuda(), tt.cuda())
    loss = (w.cuda() * seq).sum() + (wp.cuda() * pooled).sum()
    loss.backward()
    model.engine.check_errors()
    params = dict(model.named_parameters())
    grads = {"inputs_embeds": xd.grad.cpu()}
    for k in er.grad_names(c):
        g = params[k].grad.detach().cpu()
        grads[k] = g[:c["S"]] if k == "embeddings.position_embeddings.weight" else g
    return seq.detach().cpu(), pooled.detach().cpu(), float(loss), grads


def _cut(c, k, g):
    return g[:c["S"]] if k == "embeddings.position_embeddings.weight" else g


@pytest.mark.parametrize("name,mode", [(n, m) for n in er.CASES for m in er.case_modes(n)])
def test_outputs_and_gradients_against_the_restatement_and_huggingface(name, mode):
    c = er.CASES[name]
    H = c["hidden"]
    model = _model(name)
    _install(model, name, mode)
    seq, pooled, loss, grads = _step(model, name)
    r, r16 = er.reference(name, mode, "r64"), er.reference(name, mode, "r16")
    masked = (c["mask"].view(-1) == 0)
    outputs = [("seq", seq, r["seq"], r16["seq"]),
               ("seq.masked_query_rows", seq.reshape(-1, H)[masked], r["seq"].reshape(-1, H)[masked], r16["seq"].reshape(-1, H)[masked]),
               ("pooled", pooled, r["pooled"], r16["pooled"])]
    for k, g in grads.items():
        outputs.append(("grad." + k, g, _cut(c, k, r["grads"][k]), _cut(c, k, r16["grads"][k])))
    fails = []
    for key, got, want, want16 in outputs:
        assert bool(torch.isfinite(got).all()), key
        kr, rr = er.rel(got, want), er.rel(want16, want)
        print(f"PARITY bigbird_encoder.{name}.{mode}.{key} got_vs_r={kr:.3e} r16_vs_r={rr:.3e} ratio={kr / rr:.3f}")
        if kr > 2.0 * rr:
            fails.append(f"{key}: ||got - r|| / ||r|| = {kr:.3e} > 2 x r16's {rr:.3e}")
    # ... and HuggingFace's own float32 numbers, at the rows the fixture keeps (plus what that float32 run may be off by)
    A = er.load_fixture(name)["arrays"]
    rows = er.sample_rows(c)
    hf_seq, hf_pooled = torch.from_numpy(A[f"{mode}.seq"]), torch.from_numpy(A[f"{mode}.pooled"])
    for key, got, want, rr in (("hf.seq", seq.reshape(-1, H)[rows], hf_seq, er.rel(r16["seq"].reshape(-1, H)[rows], r["seq"].reshape(-1, H)[rows])),
                               ("hf.pooled", pooled, hf_pooled, er.rel(r16["pooled"], r["pooled"]))):
        kr = er.rel(got, want)
        print(f"PARITY bigbird_encoder.{name}.{mode}.{key} got_vs_hf={kr:.3e} r16_vs_r={rr:.3e} ratio={kr / rr:.3f}")
        if kr > 2.0 * rr + er.HF_FLOAT32_ERROR:
            fails.append(f"{key}: ||got - hf|| / ||hf|| = {kr:.3e} > 2 x r16's {rr:.3e}")
    assert not fails, f"{name} {mode}:\n  " + "\n  ".join(fails)


def test_bert_prefixed_checkpoint_and_repeated_calls_give_the_same_bits():
    name = "s768"
    c = er.CASES[name]
    sd, x, tt, _ = er.case_data(name)
    plain = _model(name)
    _install(plain, name, "eval")
    other = BigBirdEncoderModel(BigBirdEncoderConfig(**er.config_dict(c)), seed=3)
    extra = {"cls.predictions.bias": torch.zeros(4), "lm_backbone.embeddings.LayerNorm.weight": torch.ones(4)}
    with pytest.warns(UserWarning, match="ignored"):
        other.load_state_dict({**{"bert." + k: v for k, v in sd.items()}, **extra})
    assert sorted(other.ignored_keys) == sorted(extra)
    _install(other, name, "eval")
    with torch.no_grad():
        a = plain(x.cuda(), c["mask"].cuda(), tt.cuda())
        b = plain(x.cuda(), c["mask"].cuda(), tt.cuda())
        o = other(x.cuda(), c["mask"].cuda(), tt.cuda())
    for u, v, w in zip(a, b, o):
        assert torch.equal(u, v) and torch.equal(u, w)
    # a state dict round-trips, the dead word table included
    back = plain.state_dict()
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)


def test_dropout_call_is_finite_repeats_under_its_seed_and_differs_from_p0():
    name = "s768"
    c = er.CASES[name]
    _, x, tt, _ = er.case_data(name)
    model = _model(name, hidden_dropout_prob=0.1)
    _install(model, name, "train")
    outs = []
    for seed in (5, 5, 6):
        model.set_dropout_seed(seed)
        xd = x.cuda().requires_grad_(True)
        seq, pooled = model(xd, c["mask"].cuda(), tt.cuda())
        (seq.sum() + pooled.sum()).backward()
        # (the parameter gradients are summed with float atomics, as everywhere in the project: finite, not bitwise repeatable)
        outs.append((seq.detach().clone(), pooled.detach().clone(), xd.grad.clone(),
                     model.embeddings.LayerNorm.weight.grad.clone()))
        model.zero_grad()
    assert all(bool(torch.isfinite(t).all()) for o in outs for t in o)
    for what, a, b in zip(("sequence output", "pooled", "d(inputs_embeds)"), outs[0], outs[1]):
        assert torch.equal(a, b), f"the same seed gives other bits in the {what}"
    assert not torch.equal(outs[0][0], outs[2][0])
    p0 = _model(name)
    _install(p0, name, "train")
    with torch.no_grad():
        seq0, _ = p0(x.cuda(), c["mask"].cuda(), tt.cuda())
    assert not torch.equal(outs[0][0], seq0)


def test_three_fused_adamw_steps_lower_the_scalar():
    name = "s768"
    model = _model(name)
    _install(model, name, "train")
    opt = FusedAdamW(model._store)
    losses = []
    for _ in range(4):
        losses.append(_step(model, name)[2])
        opt.step(1e-3)
    print("PARITY bigbird_encoder.adamw losses " + " ".join(f"{v:.4f}" for v in losses))
    assert losses[3] < losses[2] < losses[1] < losses[0]


def test_lengths_huggingface_would_not_run_block_sparse_are_refused():
    model = _model("s768")
    for S, what in ((704, "full attention"), (800, "pads")):
        with pytest.raises(ValueError, match=what):
            model(torch.zeros(1, S, 128))
