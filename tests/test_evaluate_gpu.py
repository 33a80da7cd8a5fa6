"""GPU: evaluation and masked top-k prediction without dense logits (Engine.evaluate, STonKGsForPreTraining.evaluate_batch /
predict_masked, Trainer.evaluate) on g2_hipsmall (B 3, S 256, V 512, K 300, 2 layers) against its golden loss terms and the
CPU oracle's logits, plus one full-vocabulary run. Ties and near-ties of the fp16 logits cannot decide a check: every
comparison with the oracle allows the error `eps` that the EXISTING eval-mode dense logits show against it (the dense path
is not code under test) plus the fp16 rounding of the label-sparse logits."""
import os

import pytest
import torch

from oracle import stonkgs_oracle as orc
from tests.golden_util import load_case

pytestmark = pytest.mark.gpu
HEADS = (("text", "masked_lm_labels", "masked_lm_loss", 0), ("ent", "ent_masked_lm_labels", "ent_masked_lm_loss", 1))


def _build(cfg, sd, tsv_rows, dropout=0.0):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    c = STonKGsConfig(**{k: getattr(cfg, k) for k in ("vocab_size", "kg_vocab_size", "hidden_size", "num_hidden_layers",
                                                      "num_attention_heads", "intermediate_size",
                                                      "max_position_embeddings", "type_vocab_size", "layer_norm_eps")},
                      hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    model = STonKGsForPreTraining(c, kg_embeddings=tsv_rows)
    model.load_state_dict(sd, strict=False)
    return model


@pytest.fixture(scope="module")
def g2(hip):
    """The case, a model, the oracle's dense logits and the existing eval-mode dense logits: computed once, left unchanged."""
    cfg, sd, tsv_rows, batch, gold, meta = load_case("g2_hipsmall")
    model = _build(cfg, sd, tsv_rows)
    with torch.no_grad():
        table = orc.build_kg_table(tsv_rows, orc.special_vectors(sd, cfg))
        ref = orc.forward(sd, cfg, table, batch["input_ids"], batch["attention_mask"], batch["token_type_ids"])
        model.eval()
        dense = model(**batch, return_dict=True).prediction_logits
    model.engine.check_errors()
    L = (ref["text_logits"].double(), ref["ent_logits"].double())
    return dict(cfg=cfg, sd=sd, tsv_rows=tsv_rows, batch=batch, gold=gold, model=model, L=L,
                dense=tuple(d.double().cpu() for d in dense), res=model.evaluate_batch(batch, k=10))


def test_bookkeeping_and_loss_terms(g2):
    batch, gold, res = g2["batch"], g2["gold"], g2["res"]
    for nm, lkey, term, _ in HEADS:
        lab = batch[lkey]
        where = (lab != -100).nonzero()                     # row-major order of labels != -100
        h = res[nm]
        assert torch.equal(h["batch_index"].cpu(), where[:, 0]) and torch.equal(h["position"].cpu(), where[:, 1])
        assert torch.equal(h["label"].cpu(), lab[lab != -100])
        n = where.shape[0]
        assert h["topk_ids"].shape == (n, 10) and h["topk_logprobs"].shape == (n, 10) and h["rank"].shape == (n,)
        assert abs(float(h["nll"].double().mean()) - float(gold[term])) < 1e-2, nm
        assert abs(float(res[term]) - float(gold[term])) < 1e-2, nm
        lp = h["topk_logprobs"]
        assert (lp[:, 1:] <= lp[:, :-1]).all() and (lp <= 0).all()
        assert all(len(set(row)) == 10 for row in h["topk_ids"].tolist())
        N = g2["cfg"].vocab_size if nm == "text" else g2["cfg"].kg_vocab_size
        assert (h["topk_ids"] >= 0).all() and (h["topk_ids"] < N).all() and (h["rank"] >= 0).all() and (h["rank"] < N).all()
        # rank < k exactly when the label is among the ids, at that place
        hit = (h["topk_ids"] == h["label"][:, None])
        assert torch.equal(hit.any(1), h["rank"] < 10)
        assert torch.equal(hit.float().argmax(1)[hit.any(1)], h["rank"][hit.any(1)])
    assert abs(float(res["next_sentence_loss"]) - float(gold["next_sentence_loss"])) < 1e-2
    assert abs(float(res["loss"]) - float(gold["loss"])) < 1e-2
    assert res["nsp_logits"].shape == (3, 2)


def test_consistent_with_the_oracle_logits_whatever_the_ties(g2):
    """eps = max |existing eval-mode dense logits - L| on the labelled rows + 2^-10 max |L| (the fp16 rounding of the
    label-sparse logits). Values against the oracle's at the returned ids and against its j-th largest within eps; the rank
    between the counts that 2 eps leave open; on rows whose oracle top-1 margin exceeds 2 eps the top-1 id IS the oracle's
    argmax, and such rows are at least a quarter of the labelled rows."""
    batch, model = g2["batch"], g2["model"]
    dev = {k: v.cuda() for k, v in batch.items()}
    out = model.engine.evaluate(dev["input_ids"], dev["attention_mask"], dev["token_type_ids"], dev["masked_lm_labels"],
                                dev["ent_masked_lm_labels"], dev["next_sentence_labels"], 10)
    decisive = labelled = 0
    for nm, lkey, _, hi in HEADS:
        lab = batch[lkey]
        sel = lab != -100
        L, dense = g2["L"][hi][sel], g2["dense"][hi][sel]   # [n, N], rows in the order of labels != -100
        n = L.shape[0]
        h = out[nm]
        assert int(h["count"].item()) == n
        eps = float((dense - L).abs().max() + 2.0 ** -10 * L.abs().max())
        top_val, top_idx = h["top_val"][:n].double().cpu(), h["top_idx"][:n].long().cpu()
        rank, t = h["rank"][:n].long().cpu(), lab[sel]
        assert torch.equal(h["targets"][:n].long().cpu(), t)
        srt = torch.sort(L, dim=1, descending=True).values
        e_at = (top_val - L.gather(1, top_idx)).abs().max().item()
        e_jth = (top_val - srt[:, :10]).abs().max().item()
        Lt = L.gather(1, t[:, None])
        lo = (L > Lt + 2 * eps).sum(1)
        hi_ = (L >= Lt - 2 * eps).sum(1) - 1                # (every class but the target itself)
        margin = srt[:, 0] - srt[:, 1]
        dec = margin > 2 * eps
        print(f"{nm}: eps {eps:.4e} (max |L| {L.abs().max().item():.3f}); |top_val - L[idx]| {e_at:.3e}, |top_val - jth| "
              f"{e_jth:.3e}; decisive rows {int(dec.sum())} of {n}")
        assert e_at <= eps and e_jth <= eps
        assert (lo <= rank).all() and (rank <= hi_).all()
        assert torch.equal(top_idx[dec, 0], L.argmax(1)[dec])
        decisive, labelled = decisive + int(dec.sum()), labelled + n
    print(f"decisive fraction {decisive / labelled:.3f}")
    assert decisive * 4 >= labelled


def test_predict_masked_is_the_evaluation_path(g2):
    batch, model, cfg = g2["batch"], g2["model"], g2["cfg"]
    half = cfg.max_position_embeddings // 2
    ids = batch["input_ids"]
    pred = model.predict_masked(ids, batch["attention_mask"], batch["token_type_ids"], k=7)
    mask = ids == 103
    assert mask[:, :half].any() and mask[:, half:].any()
    labelled = {k: v.clone() for k, v in batch.items()}
    for nm, lkey, _, hi in HEADS:
        m = mask[:, :half] if hi == 0 else mask[:, half:]
        where = m.nonzero()
        b, p, top_ids, lp = pred[nm]
        assert torch.equal(b.cpu(), where[:, 0]) and torch.equal(p.cpu(), where[:, 1])
        assert top_ids.shape == (where.shape[0], 7)
        labelled[lkey] = torch.where(m, 5, -100)            # labels on the same positions: any class
    res = model.evaluate_batch(labelled, k=7)
    for nm, _, _, _ in HEADS:
        assert torch.equal(pred[nm][2], res[nm]["topk_ids"])
        assert torch.equal(pred[nm][3].view(torch.int32), res[nm]["topk_logprobs"].view(torch.int32))   # bit for bit
    # explicit positions = the batch's labelled positions: the same rows, ids and log-probs as evaluate_batch's
    want = torch.cat([batch["masked_lm_labels"] != -100, batch["ent_masked_lm_labels"] != -100], dim=1)
    pred = model.predict_masked(ids, batch["attention_mask"], batch["token_type_ids"], positions=want, k=10)
    for nm, _, _, _ in HEADS:
        assert torch.equal(pred[nm][0], g2["res"][nm]["batch_index"]) and torch.equal(pred[nm][2], g2["res"][nm]["topk_ids"])
        assert torch.equal(pred[nm][3].view(torch.int32), g2["res"][nm]["topk_logprobs"].view(torch.int32))
    assert model.entity_names(pred["ent"][2][:2, :2]) and model.entity_names(103) == "[MASK]"
    # no attention mask (padded layout, every position a row): same positions, finite log-probs
    free = model.predict_masked(ids, k=3)
    assert torch.equal(free["text"][1].cpu(), mask[:, :half].nonzero()[:, 1]) and torch.isfinite(free["ent"][3]).all()


def _host_metrics(results, batches, k):
    """Trainer.evaluate's contract restated on the host from per-row outputs."""
    out, total = {}, 0.0
    for nm, _, term, _ in HEADS:
        nll = torch.cat([r[nm]["nll"].double().cpu() for r in results])
        rank = torch.cat([r[nm]["rank"].cpu() for r in results]).double()
        out[f"eval_{term}"] = float(nll.sum() / nll.numel())
        out[f"eval_{nm}_acc"] = float((rank == 0).double().mean())
        out[f"eval_{nm}_hits@k"] = float((rank < k).double().mean())
        out[f"eval_{nm}_mrr"] = float((1.0 / (rank + 1.0)).mean())
        out[f"eval_{nm}_labels"] = nll.numel()
        total += out[f"eval_{term}"]
    logits = torch.cat([r["nsp_logits"].double().cpu() for r in results])
    lab = torch.cat([b["next_sentence_labels"].reshape(-1) for b in batches])
    out["eval_next_sentence_loss"] = float(torch.nn.functional.cross_entropy(logits, lab))
    out["eval_nsp_acc"] = float((logits.argmax(1) == lab).double().mean())
    out["eval_rows"] = lab.numel()
    out["eval_loss"] = total + out["eval_next_sentence_loss"]
    return out


def test_trainer_evaluate_is_count_weighted_and_matches_the_rows(g2):
    import torch.distributed as dist

    from stonkgs_amd.data import synthetic_batch
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    cfg, batch = g2["cfg"], g2["batch"]
    model = _build(cfg, g2["sd"], g2["tsv_rows"])
    small = synthetic_batch(2, cfg.vocab_size, cfg.kg_vocab_size, cfg.max_position_embeddings, seed=31, min_text=16)
    batches = [batch, small]
    model.train()
    tr = Trainer(model, TrainingArguments(per_device_train_batch_size=3), eval_dataset=batches)
    got = tr.evaluate(k=5)
    assert model.training                                   # the mode is left as it was
    results = [model.evaluate_batch(b, k=5) for b in batches]
    want = _host_metrics(results, batches, 5)
    assert set(want) == set(got)
    for key, v in want.items():
        assert got[key] == pytest.approx(v, rel=1e-9, abs=1e-12), key
    assert got["eval_rows"] == 5 and results[0]["text"]["nll"].numel() != results[1]["text"]["nll"].numel()   # unequal counts
    # count-weighted: sum(nll) / sum(count) over the set - not the mean of the two batch losses, which differs
    for _, _, term, _ in HEADS:
        mean_of_means = sum(float(r[term]) for r in results) / 2
        assert abs(got[f"eval_{term}"] - mean_of_means) > 1e-5, term
    assert got["eval_loss"] == pytest.approx(
        got["eval_masked_lm_loss"] + got["eval_ent_masked_lm_loss"] + got["eval_next_sentence_loss"], rel=1e-12)
    assert tr.evaluate(k=5, max_batches=1)["eval_rows"] == 3
    # row dicts instead of collated batches: one pass in order, the ragged last batch included
    rows = [{k: v[i].tolist() for k, v in b.items()} for b in batches for i in range(b["input_ids"].shape[0])]
    tr.args.per_device_eval_batch_size = 3
    by_rows = tr.evaluate(rows, k=5)
    for key, v in want.items():
        assert by_rows[key] == pytest.approx(v, rel=1e-9, abs=1e-12), key
    # once more inside a one-rank process group: the sums go through one all-reduce and come back as they were
    from datetime import timedelta

    from stonkgs_amd.launch import free_port

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", torch.cuda.current_device()),
                            timeout=timedelta(seconds=120))
    try:
        grouped = Trainer(model, TrainingArguments(per_device_train_batch_size=3), eval_dataset=batches).evaluate(k=5)
    finally:
        dist.destroy_process_group()
    assert set(grouped) == set(got)
    for key, v in got.items():
        assert grouped[key] == pytest.approx(v, rel=1e-9, abs=1e-12), key


def test_evaluation_is_invisible_to_training(g2):
    """Five training steps with dropout 0.1 from a fixed dropout counter, the next batch's frozen-backbone forward
    prefetched, once with Trainer.evaluate between steps 2 and 3 and once without: losses, grad-norm and parameters after
    the five steps within the bounds test_optimizer_stream_is_equivalent_to_serial_order uses, as they stand there. The
    engine's state around the evaluation is compared directly and exactly: nothing may have moved."""
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    cfg, batch = g2["cfg"], g2["batch"]
    runs = []
    for with_eval in (True, False):
        model = _build(cfg, g2["sd"], g2["tsv_rows"], dropout=0.1)
        model.engine.seed_base = 0x5710
        tr = Trainer(model, TrainingArguments(max_steps=200, learning_rate=1e-4, per_device_train_batch_size=3),
                     eval_dataset=[batch])
        losses, snaps = [], {}
        for step in range(5):
            losses.append(float(tr.training_step(model, batch, next_inputs=batch)))
            if step == 1 and with_eval:
                eng = model.engine
                model.engine.wait_params()
                torch.cuda.synchronize()
                before = (eng.seed_base, eng._prefetch, eng.next_input_ids, eng.store_first, set(eng.grad_stale), eng.saved,
                          model._store.grad.clone(), model._store.data.clone(), list(eng.rows_executed))
                assert before[1] is not None                # a prefetched backbone forward is waiting for step 3
                metrics = tr.evaluate(k=10)
                torch.cuda.synchronize()
                assert metrics["eval_rows"] == 3 and model.training
                after = (eng.seed_base, eng._prefetch, eng.next_input_ids, eng.store_first, set(eng.grad_stale), eng.saved,
                         model._store.grad, model._store.data, list(eng.rows_executed))
                assert before[0] == after[0] and before[1] is after[1] and before[2] is after[2] and before[3:6] == after[3:6]
                assert torch.equal(before[6], after[6]) and torch.equal(before[7], after[7]) and before[8] == after[8]
            if step == 4:
                snaps[step] = {k: v.detach().clone() for k, v in model.named_parameters()}
        assert model.training
        runs.append((losses, snaps, tr.optimizer.last_grad_norm()))
    (l0, s0, g0), (l1, s1, g1) = runs
    print("losses with / without evaluation:", l0, l1, "grad norms:", g0, g1)
    assert l0 == pytest.approx(l1, rel=1e-4)
    assert g0 == pytest.approx(g1, rel=1e-4)
    diff = torch.cat([(s0[4][k] - s1[4][k]).abs().flatten() for k in s0[4]])
    print(f"after 5 steps: max |dparam| {float(diff.max()):.3e}, share > 2e-6: {float((diff > 2e-6).float().mean()):.2e}")
    assert float(diff.max()) <= 6.1e-4
    assert float((diff > 2e-6).float().mean()) < 2e-3


@pytest.mark.parametrize("call", ["evaluate", "attention_maps", "attributions_labels", "attributions_target"])
def test_a_failing_detached_call_puts_the_training_state_back(g2, call, monkeypatch):
    """The exception path of Engine._detached: with a prefetched backbone forward waiting and the hint for the next one
    set, the body fails in its first layer (Engine.layer_fwd is made to raise: host logic only, nothing runs that was not
    asked for). The call raises, and the dropout counter, the inputs-only flag, the prefetch, the hint, `saved` and - for
    the callers that restore it - `rows_executed` are what they were."""
    from stonkgs_amd.engine import Engine
    from tests.test_finetune_gpu import _build_cls

    batch = g2["batch"]
    inputs = {k: batch[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    model = g2["model"]
    if call == "attributions_target":
        sd = dict(g2["sd"])
        sd["classifier.weight"], sd["classifier.bias"] = torch.zeros(3, g2["cfg"].hidden_size), torch.zeros(3)
        model = _build_cls(g2["cfg"], sd, g2["tsv_rows"], 3)
    model.eval()
    eng = model.engine
    ids = batch["input_ids"].to(model.device)
    try:
        eng.prefetch_backbone(ids, False)
        eng.next_input_ids = ids
        before = (eng.seed_base, eng._inputs_only, eng._prefetch, eng.next_input_ids, list(eng.rows_executed))
        assert before[2] is not None and eng.saved is None

        def fail(*args, **kwargs):
            raise RuntimeError("layer_fwd was made to fail")

        monkeypatch.setattr(Engine, "layer_fwd", fail)
        with pytest.raises(RuntimeError, match="made to fail"):
            if call == "evaluate":
                model.evaluate_batch(batch, k=10)
            elif call == "attention_maps":
                model.attention_maps(**inputs, layers=[0])
            elif call == "attributions_labels":
                model.input_attributions(**inputs, labels={k: batch[k] for k in ("masked_lm_labels", "ent_masked_lm_labels",
                                                                                "next_sentence_labels")})
            else:
                model.input_attributions(**inputs)
        assert eng.seed_base == before[0] and eng._inputs_only == before[1]
        assert eng._prefetch is before[2] and eng.next_input_ids is before[3]
        if call != "attention_maps":   # (a successful attention_maps counts its rows: nothing to put back)
            assert list(eng.rows_executed) == before[4]
        assert eng.saved is None
    finally:   # the model is the module's: leave no prefetch behind
        monkeypatch.undo()
        torch.cuda.synchronize()
        eng._prefetch = eng.next_input_ids = None


def test_train_evaluates_every_eval_steps(g2):
    """TrainingArguments.eval_steps: during train() the evaluation result is appended to log_history with the step, every
    eval_steps optimizer steps, and the module is in training mode afterwards."""
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    cfg, batch = g2["cfg"], g2["batch"]
    model = _build(cfg, g2["sd"], g2["tsv_rows"])
    tr = Trainer(model, TrainingArguments(max_steps=2, per_device_train_batch_size=3, eval_steps=1, logging_steps=100,
                                          save_steps=0), train_dataset=[batch], eval_dataset=[batch])
    tr.train()
    evals = [e for e in tr.log_history if "eval_loss" in e]
    assert [e["step"] for e in evals] == [1, 2] and model.training
    assert all(e["eval_rows"] == 3 and e["eval_loss"] > 0 for e in evals)
    assert evals[1]["eval_loss"] < evals[0]["eval_loss"]      # one more optimizer step on the batch it is evaluated on
    off = Trainer(model, TrainingArguments(max_steps=1, per_device_train_batch_size=3, save_steps=0), train_dataset=[batch],
                  eval_dataset=[batch])
    off.train()
    assert not [e for e in off.log_history if "eval_loss" in e]   # eval_steps = 0: never


def test_full_vocabulary_evaluation(hip):
    """V 28 996, K 175 094, 2 layers, B 2: the real row widths through the whole path; the entity nll mean against the
    loss term of the existing labelled eval-mode forward (label-sparse, no dense logits)."""
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.data import synthetic_batch
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    cfg = STonKGsConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    assert (cfg.vocab_size, cfg.kg_vocab_size) == (28996, 175094)
    model = STonKGsForPreTraining(cfg, seed=3)
    batch = synthetic_batch(2, cfg.vocab_size, cfg.kg_vocab_size, 512, seed=41)
    res = model.evaluate_batch(batch, k=10)
    for nm in ("text", "ent"):
        h = res[nm]
        assert h["rank"].numel() == 76 and torch.isfinite(h["nll"]).all() and torch.isfinite(h["topk_logprobs"]).all()
        assert (h["topk_logprobs"][:, 1:] <= h["topk_logprobs"][:, :-1]).all()
    assert all(torch.isfinite(res[k]).all() for k in ("loss", "masked_lm_loss", "ent_masked_lm_loss", "next_sentence_loss"))
    model.eval()
    model.materialize_logits = False
    with torch.no_grad():
        model(**batch)
    model.engine.check_errors()
    terms = [float(t) for t in model.last_loss_terms]
    print("full vocabulary: nll means", float(res["text"]["nll"].mean()), float(res["ent"]["nll"].mean()), "terms", terms)
    assert abs(float(res["ent"]["nll"].double().mean()) - terms[1]) < 1e-2
    assert abs(float(res["text"]["nll"].double().mean()) - terms[0]) < 1e-2
