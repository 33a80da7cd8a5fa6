"""GPU: where the trainer's gradient norm comes from. With one micro-batch per step on one rank and both decoders' weight
gradients stored, the sum-of-squares pass reads the complement of the decoders' spans and adds the sums the store epilogues
left ("epilogue"); in every other case it reads the whole buffer as it always did ("full pass") - and then the step is the
parent path's, bit for bit.

The model is the one tests/test_wgrad_store_gpu.py drives its trainer steps with, except for the entity vocabulary: with
300 entities the entity decoder's gradient splits K and the store entry refuses it (that file asserts the STONK_ESHAPE), so
the new route could never be taken; 62 000 entities make 485 tiles of 128x128, which the routing leaves unsplit like the
31 000-token text decoder. The 300-entity model is kept as the refused-store case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TEXT, ENT = "cls.predictions.text_decoder.weight", "cls.predictions.entity_decoder.weight"


def _trainer(kg=62000, gas=1):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    dims = dict(vocab_size=31000, kg_vocab_size=kg, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                intermediate_size=256, max_position_embeddings=256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    rows = torch.randn(kg, 128, generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 0.3
    torch.manual_seed(3)
    model = STonKGsForPreTraining(STonKGsConfig(**dims), kg_embeddings=rows)
    tr = Trainer(model, TrainingArguments(per_device_train_batch_size=4, gradient_accumulation_steps=gas, learning_rate=1e-3))
    return model, tr


def _batch(kg, seed):
    from stonkgs_amd.data import synthetic_batch

    return synthetic_batch(4, 31000, kg, 256, seed=seed, min_text=16)


def _spy(tr, model):
    """Record what the optimizer's update starts from (on the optimizer's stream, behind the norm pass)."""
    opt, st, seen = tr.optimizer, model._store, []
    inner = opt.apply_update

    def apply_update(lr, grad_scale=1.0, **kw):
        seen.append(dict(g=st.grad.clone(), p=st.data.clone(), m=opt.m.clone(), v=opt.v.clone(), norm=opt.gnorm_sq.clone(),
                         route=opt.norm_route, lr=lr, scale=grad_scale, step=opt.step_count))
        return inner(lr, grad_scale, **kw)

    opt.apply_update = apply_update
    return seen


def _full_pass(hip, g):
    out = torch.zeros(1, device="cuda")
    ws = torch.zeros(int(hip.lib().stonk_sumsq_workspace_floats()), device="cuda")
    hip.call("stonk_sumsq_f32", hip.ptr(g), g.numel(), hip.ptr(out), hip.ptr(ws), ws.numel(), hip.stream_ptr())
    return out


def _assert_parent_step(hip, model, tr, s):
    """The recorded step was the parent path's: its norm is stonk_sumsq_f32 over the whole buffer, bit for bit, and the
    parameters and Adam's moments are what the flat stonk_adamw_step makes of the recorded state with that norm."""
    opt = tr.optimizer
    norm = _full_pass(hip, s["g"])
    assert torch.equal(norm, s["norm"]), (float(norm), float(s["norm"]))
    p, g, m, v = s["p"].clone(), s["g"].clone(), s["m"].clone(), s["v"].clone()
    pb = torch.empty(p.numel(), dtype=torch.bfloat16, device="cuda")
    b1, b2 = opt.betas
    hip.call("stonk_adamw_step", hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(pb), p.numel(), s["lr"], b1, b2, opt.eps,
             0.0, 1.0 - b1 ** s["step"], 1.0 - b2 ** s["step"], hip.ptr(norm), opt.max_grad_norm, s["scale"], 0, 0, 0,
             hip.stream_ptr())
    model.engine.wait_params()
    torch.cuda.synchronize()
    assert torch.equal(p, model._store.data) and torch.equal(m, opt.m) and torch.equal(v, opt.v)
    assert torch.equal(pb, model._store.bf16)


def _rel_err(value, exact):
    return abs(float(value) - exact) / exact


def test_one_micro_batch_takes_the_norm_from_the_store_epilogues(hip):
    model, tr = _trainer()
    eng, seen = model.engine, _spy(tr, model)
    for i in range(3):
        eng.store_log.clear()
        tr.training_step(model, _batch(62000, 20 + i))
        eng.wait_params()
        torch.cuda.synchronize()
        assert list(eng.store_log) == [(ENT, hip.OK), (TEXT, hip.OK)]
        s = seen[-1]
        assert s["route"] == tr.optimizer.norm_route == "epilogue" and not eng.sumsq_valid
        # both routes against the fp64 sum over the flat gradient buffer; the yardstick of the full pass is torch's fp32 sum
        # of squares, the yardstick of the new route is the full pass (4x rule; one fp32 ulp where the yardstick is exact)
        exact = float((s["g"].double() ** 2).sum())
        ulp = float(np.spacing(np.float32(exact))) / exact
        err_new, err_full = _rel_err(s["norm"].double(), exact), _rel_err(_full_pass(hip, s["g"]).double(), exact)
        err_torch = _rel_err((s["g"] * s["g"]).sum().double(), exact)
        print(f"step {i}: sum g^2 = {exact:.6e}; relative error: epilogue route {err_new:.3e}, full pass {err_full:.3e}, "
              f"torch fp32 {err_torch:.3e}; one fp32 ulp {ulp:.3e}")
        assert err_full <= (4 * err_torch if err_torch > 0 else ulp)
        assert err_new <= (4 * err_full if err_full > 0 else ulp)
    model.engine.check_errors()


@pytest.mark.parametrize("case", ["two micro-batches", "refused store", "switched off"])
def test_every_other_case_is_the_full_pass_and_the_parent_step(hip, case):
    kg = 300 if case == "refused store" else 62000
    model, tr = _trainer(kg=kg, gas=2 if case == "two micro-batches" else 1)
    eng, seen = model.engine, _spy(tr, model)
    eng.norm_from_epilogue = case != "switched off"
    for i in range(4 if case == "two micro-batches" else 2):
        eng.store_log.clear()
        tr.training_step(model, _batch(kg, 30 + i))
        if case == "refused store":
            assert list(eng.store_log) == [(ENT, hip.ESHAPE), (TEXT, hip.OK)]
        assert not eng.sumsq_valid
    assert len(seen) == 2 and all(s["route"] == "full pass" for s in seen)
    _assert_parent_step(hip, model, tr, seen[-1])


def test_a_backward_outside_the_trainer_is_the_full_pass(hip):
    model, tr = _trainer()
    eng, opt, seen = model.engine, tr.optimizer, _spy(tr, model)
    tr.training_step(model, _batch(62000, 40))
    assert seen[-1]["route"] == "epilogue"
    eng.wait_params()
    model.forward_backward(_batch(62000, 41))          # (zeroes the stale decoder spans, accumulates: nothing is stored)
    assert not eng.sumsq_valid and eng.take_wgrad_sumsq() is None
    opt.step_count += 1
    opt.accumulate_grad_norm_sq(eng.take_wgrad_sumsq())
    opt.apply_update(5e-4, tables=eng.adamw_tables(), keep_grad=tr._keep_grad)
    assert seen[-1]["route"] == opt.norm_route == "full pass"
    _assert_parent_step(hip, model, tr, seen[-1])


@pytest.mark.parametrize("n,n_extra", [(70001, 0), (70001, 3), (70001, 1500), (70001, 3414), (0, 5)])
def test_sumsq_plus_adds_the_extras_in_index_order(hip, n, n_extra):
    g = torch.Generator(device="cuda").manual_seed(n_extra)
    x = torch.randn(max(n, 4), generator=g, device="cuda")
    extra = torch.rand(max(n_extra, 1), generator=g, device="cuda") * 50
    ws = torch.zeros(int(hip.lib().stonk_sumsq_workspace_floats()), device="cuda")
    base, out = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    hip.call("stonk_sumsq_f32", hip.ptr(x), n, hip.ptr(base), hip.ptr(ws), ws.numel(), hip.stream_ptr())
    hip.call("stonk_sumsq_f32_plus", hip.ptr(x), n, hip.ptr(out), hip.ptr(ws), ws.numel(), hip.ptr(extra) if n_extra else 0,
             n_extra, hip.stream_ptr())
    torch.cuda.synchronize()
    # in index order, in fp64, rounded once: 64 consecutive runs summed element by element, the run sums added one by one
    want, ex, per = np.float64(np.float32(base.item())), extra[:n_extra].cpu().numpy().astype(np.float64), (n_extra + 63) // 64
    for r in range(64):
        run = np.float64(0.0)
        for e in ex[r * per:(r + 1) * per]:
            run = run + e
        want = want + run
    want = np.float32(want)
    assert np.float32(out.item()).tobytes() == want.tobytes(), (float(out), float(want))
    if n:
        assert abs(float(base) - float((x[:n].double() ** 2).sum())) <= 1e-5 * float(base)
    assert float(ws[-1]) == 0.0     # the workspace is left ready: the ticket word is back at zero
