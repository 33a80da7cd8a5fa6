"""GPU parity of the whole hot path: the HIP STonKGsForPreTraining against
  (1) golden vectors produced by the REFERENCE itself (tests/golden/g2_hipsmall, see oracle/make_golden.py), and
  (2) the CPU oracle on fresh seeded inputs,
through the reference's own module contract (constructor, load_state_dict, forward, loss.backward, Trainer).
bf16 compute vs fp32 reference: tolerances are stated per check."""
import os

import numpy as np
import pytest
import torch

from oracle import stonkgs_oracle as orc
from tests.golden_util import load_case

pytestmark = pytest.mark.gpu


def _build(cfg, sd, tsv_rows, dropout=0.0):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    c = STonKGsConfig(**{k: getattr(cfg, k) for k in ("vocab_size", "kg_vocab_size", "hidden_size", "num_hidden_layers",
                                                      "num_attention_heads", "intermediate_size",
                                                      "max_position_embeddings", "type_vocab_size", "layer_norm_eps")},
                      hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    model = STonKGsForPreTraining(c, kg_embeddings=tsv_rows)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("decoder" in k for k in missing), missing  # only the tied/dead aliases may be absent
    return model


def _rel(a, b):
    """Relative L2 error; a reference that is analytically zero (the key-projection bias gradient: softmax is
    invariant to a per-query constant) is compared on an absolute scale instead."""
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    if b.norm() < 1e-5:
        return (a - b).norm().item() / 1e-2
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def g2(hip):
    cfg, sd, tsv_rows, batch, gold, meta = load_case("g2_hipsmall")
    return cfg, sd, tsv_rows, batch, gold, meta, _build(cfg, sd, tsv_rows)


def test_forward_matches_reference_golden(g2):
    cfg, sd, tsv_rows, batch, gold, meta, model = g2
    model.eval()
    with torch.no_grad():
        out = model(**batch, return_dict=True)
    model.engine.check_errors()
    # quirk Q2: LM special-token rows of the entity table
    for sid in (100, 102, 103):
        assert _rel(model.kg_backbone[sid], gold[f"special_{sid}"]) < 2e-2
    # loss: |delta| < 1e-2 absolute on ~12.7 (bf16 activations; measured 1-5e-3 - DESIGN section 2 relates this to
    # north_star's 1e-3); terms individually
    assert abs(float(out.loss) - float(gold["loss"])) < 1e-2
    terms = [float(t) for t in model.last_loss_terms]
    for got, key in zip(terms, ("masked_lm_loss", "ent_masked_lm_loss", "next_sentence_loss")):
        assert abs(got - float(gold[key])) < 1e-2, key
    assert _rel(out.pooler_output, gold["pooler_output"]) < 2e-2
    assert _rel(out.seq_relationship_logits, gold["nsp_logits"]) < 3e-2
    assert _rel(out.hidden_states[:, ::7, ::3], gold["hidden_states_s"]) < 2e-2
    tl, el = out.prediction_logits
    assert tl.shape == (3, 128, cfg.vocab_size) and el.shape == (3, 128, cfg.kg_vocab_size)
    assert _rel(tl[:, ::5, ::3], gold["text_logits_s"]) < 3e-2
    assert _rel(el[batch["ent_masked_lm_labels"].cuda() != -100], gold["ent_logits_lab"]) < 3e-2
    # tuple packing when return_dict is falsy (ref :247-249)
    with torch.no_grad():
        tup = model(**batch)
    assert len(tup) == 3 and torch.allclose(tup[0], out.loss) and tup[1][0].shape == tl.shape


def test_backward_matches_reference_golden(g2):
    cfg, sd, tsv_rows, batch, gold, meta, model = g2
    model.train()
    model.zero_grad()      # zeroes the flat gradient buffer the engine accumulates into
    loss = model(**batch)[0]
    assert abs(float(loss) - float(gold["loss"])) < 1e-2
    loss.backward()
    grads = dict(model.named_parameters())
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.requires_grad))
    assert abs(float(total) - float(gold["grad_norm"])) < 3e-2 * float(gold["grad_norm"])
    for k in meta["grad_keys"]:
        e = _rel(grads[k].grad, gold["grad::" + k])
        assert e < 6e-2, (k, e)
    # dead parameters (quirk Q4) exist, carry no gradient
    for k in ("bert.embeddings.word_embeddings.weight", "cls.predictions.bias", "cls.predictions.text_bias",
              "cls.predictions.entity_bias"):
        assert not grads[k].requires_grad
    assert "cls.predictions.decoder.weight" in model.state_dict()


def test_two_optimizer_steps_match_reference_golden(hip):
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    cfg, sd, tsv_rows, batch, gold, meta = load_case("g2_hipsmall")
    model = _build(cfg, sd, tsv_rows)
    tr = Trainer(model, TrainingArguments(max_steps=200, learning_rate=1e-4, per_device_train_batch_size=3))
    losses = [float(tr.training_step(model, batch)) for _ in range(2)]
    np.testing.assert_allclose(losses, gold["step_losses"], atol=1e-2)
    params = dict(model.named_parameters())
    for k in meta["grad_keys"]:
        before = sd[k]
        got_delta = params[k].detach().cpu() - before
        ref_delta = torch.from_numpy(gold["after2::" + k]) - before
        # Adam's first steps move every weight by ~lr regardless of gradient scale: compare the update direction
        if "key.bias" not in k:  # analytically zero gradient: Adam turns rounding noise into +-lr steps on both sides
            cos = torch.nn.functional.cosine_similarity(got_delta.flatten(), ref_delta.flatten(), dim=0).item()
            assert cos > 0.9, (k, cos)
            assert _rel(params[k], gold["after2::" + k]) < 1e-3, k
        else:  # two Adam steps of at most lr each, in either direction, on both sides
            assert (params[k].detach().cpu() - torch.from_numpy(gold["after2::" + k])).abs().max() <= 4.5e-4


def test_optimizer_stream_is_equivalent_to_serial_order(hip):
    """The optimizer on its own stream beside the next step's frozen-backbone forward (TrainingArguments.optimizer_overlap)
    against the serial order, three steps from the same state with the same dropout seeds: same losses and grad-norm,
    parameters equal except where split-K atomics reorder fp32 addends (last-bit gradient differences; Adam turns those
    into visible steps only for the analytically-zero gradients such as key.bias, hence the fraction-based bound)."""
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    cfg, sd, tsv_rows, batch, gold, meta = load_case("g2_hipsmall")
    res = []
    for overlap in (True, False):
        model = _build(cfg, sd, tsv_rows)
        model.engine.seed_base = 0x5710
        tr = Trainer(model, TrainingArguments(max_steps=200, learning_rate=1e-4, per_device_train_batch_size=3,
                                              optimizer_overlap=overlap))
        losses = [float(tr.training_step(model, batch)) for _ in range(3)]
        assert (model.engine._params_ready is not None) == overlap   # the overlapped step leaves its event for waiters
        params = {k: v.detach().clone() for k, v in model.named_parameters()}   # (accessor waits for the optimizer)
        res.append((losses, params, tr.optimizer.last_grad_norm()))
    (l0, p0, g0), (l1, p1, g1) = res
    assert l0 == pytest.approx(l1, rel=1e-4)
    assert g0 == pytest.approx(g1, rel=1e-4)
    diff = torch.cat([(p0[k] - p1[k]).abs().flatten() for k in p0])
    assert float(diff.max()) <= 6.1e-4            # three steps of lr = 1e-4 in opposite directions at the very worst
    assert float((diff > 2e-6).float().mean()) < 2e-3


def test_against_oracle_on_fresh_batch_and_masks(g2):
    """Oracle (pinned by test_oracle_golden.py) on a new batch with different padding, B = 5."""
    from stonkgs_amd.data import synthetic_batch

    cfg, sd, tsv_rows, batch, gold, meta, model = g2
    b = synthetic_batch(5, cfg.vocab_size, cfg.kg_vocab_size, cfg.max_position_embeddings, seed=77, min_text=16)
    with torch.no_grad():
        table = orc.build_kg_table(tsv_rows, orc.special_vectors(sd, cfg))
    sd2 = {k: v.clone() for k, v in sd.items()}
    res = orc.train_step(sd2, cfg, table, b, orc.AdamState(), max_grad_norm=0.0)
    model.load_state_dict(sd, strict=False)
    model.train()
    model.zero_grad()
    loss = model.forward_backward(b)
    assert abs(float(loss) - float(res["loss"])) < 1e-2
    gv = model.named_grad_views()
    for k in meta["grad_keys"]:
        e = _rel(gv[k], res["grads"][k])
        assert e < 6e-2, (k, e)


def test_out_of_table_entity_raises_keyerror(g2):
    cfg, sd, tsv_rows, batch, gold, meta, model = g2
    bad = {k: v.clone() for k, v in batch.items()}
    bad["input_ids"][0, -1] = cfg.kg_vocab_size + 3
    model.eval()
    with torch.no_grad():
        model(**bad)
    with pytest.raises(KeyError):
        model.engine.check_errors()


def test_dropout_training_mode_is_statistically_consistent(hip):
    """p = 0.1 (the reference's training mode, incl. dropout inside the frozen backbone, quirk Q6): loss stays near the
    p = 0 loss, differs between steps, and gradients stay finite. (Statistics only: the p = 0.1 step is held to the oracle
    element by element, under the step's exact masks, in tests/test_step_dropout_gpu.py.)"""
    cfg, sd, tsv_rows, batch, gold, meta = load_case("g2_hipsmall")
    model = _build(cfg, sd, tsv_rows, dropout=0.1)
    model.train()
    l1 = float(model.forward_backward(batch))
    l2 = float(model.forward_backward(batch))
    assert l1 != l2
    assert abs(l1 - float(gold["loss"])) < 0.5 and abs(l2 - float(gold["loss"])) < 0.5
    assert torch.isfinite(model._store.grad).all()
    model.eval()
    with torch.no_grad():
        le = float(model(**batch)[0])
    assert abs(le - float(gold["loss"])) < 1e-2  # eval mode switches every dropout off


def test_checkpoint_resume_continues_the_uninterrupted_run(hip, tmp_path):
    """Trainer.train with save_steps, then a fresh model resumed from the middle checkpoint (ref:stonkgs_pretraining.py:
    196-223: get_last_checkpoint -> train(resume_from_checkpoint)): parameters, Adam moments, step count, the position in
    the data stream and the dropout counter are restored, so the resumed run ends where the uninterrupted one did (up to
    the reordering of fp32 atomic sums). Dropout is ON: a resumed run that drew different masks would not agree."""
    from stonkgs_amd.data import synthetic_batch
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments, get_last_checkpoint

    cfg, sd, tsv_rows, batch, gold, meta = load_case("g2_hipsmall")
    S = cfg.max_position_embeddings
    ds = []
    for i in range(4):   # a dataset of already collated batches (the Trainer accepts any iterable of them)
        ds.append({k: v.cuda() for k, v in synthetic_batch(3, cfg.vocab_size, len(tsv_rows), S, seed=50 + i, min_text=8).items()})

    def run(out_dir, max_steps, resume=None):
        model = _build(cfg, sd, tsv_rows, dropout=0.1)
        tr = Trainer(model, TrainingArguments(output_dir=str(out_dir), max_steps=max_steps, learning_rate=1e-3, save_steps=2,
                                              per_device_train_batch_size=3, logging_steps=1, save_total_limit=2), ds)
        res = tr.train(resume_from_checkpoint=resume)
        return model, tr, res

    full, tr_full, res_full = run(tmp_path / "full", 6)
    assert sorted(os.listdir(tmp_path / "full")) == ["checkpoint-4", "checkpoint-6"]   # save_total_limit = 2
    assert get_last_checkpoint(str(tmp_path / "full")).endswith("checkpoint-6")
    # the interrupted run: same arguments (the learning-rate schedule spans all 6 steps), stopped after step 2
    part = _build(cfg, sd, tsv_rows, dropout=0.1)
    tr_part = Trainer(part, TrainingArguments(output_dir=str(tmp_path / "part"), max_steps=6, learning_rate=1e-3,
                                              save_steps=2, per_device_train_batch_size=3, save_total_limit=2), ds)
    for i in range(2):
        tr_part.training_step(part, ds[i])
    tr_part.save_checkpoint()
    ck = get_last_checkpoint(str(tmp_path / "part"))
    assert ck.endswith("checkpoint-2")
    resumed, tr_res, res = run(tmp_path / "part", 6, resume=ck)
    assert res["global_step"] == 6 and tr_res.optimizer.step_count == 6
    assert resumed.engine.seed_base == full.engine.seed_base
    assert res["training_loss"] == pytest.approx(res_full["training_loss"], rel=2e-3)
    a = {k: v.detach().float() for k, v in full.named_parameters()}
    b = {k: v.detach().float() for k, v in resumed.named_parameters()}
    diff = torch.cat([(a[k] - b[k]).abs().flatten() for k in a])
    assert float((diff > 1e-4).float().mean()) < 2e-3, float((diff > 1e-4).float().mean())
    # and the checkpoint is a plain HF-layout directory
    last = get_last_checkpoint(str(tmp_path / "part"))   # (checkpoint-2 itself was rotated out: save_total_limit = 2)
    assert last.endswith("checkpoint-6")
    assert {"config.json", "pytorch_model.bin", "optimizer.pt", "trainer_state.json"} <= set(os.listdir(last))


@pytest.mark.parametrize("safe", [False, True])
def test_save_pretrained_round_trip(g2, tmp_path, safe):
    """f3: save_pretrained -> from_pretrained(local_dir) in both HF weight formats: every state-dict entry (dead parameters
    included) comes back bit for bit, and the reloaded model computes the same loss."""
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    cfg, sd, tsv_rows, batch, gold, meta, model = g2
    model.save_pretrained(str(tmp_path), safe_serialization=safe)
    assert os.path.exists(tmp_path / ("model.safetensors" if safe else "pytorch_model.bin"))
    again = STonKGsForPreTraining.from_pretrained(str(tmp_path), kg_embeddings=tsv_rows)
    a, b = model.state_dict(), again.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    model.eval()
    again.eval()
    with torch.no_grad():
        la, lb = model(**batch, return_dict=True).loss, again(**batch, return_dict=True).loss
    assert float(la) == pytest.approx(float(lb), rel=1e-6)   # (the per-row loss terms are summed by float atomics)
