"""GPU: the text-only baseline (stonkgs_amd/nlp_baseline_model.py) against the fp32 restatement that
tests/test_text_embed_cpu.py pins to transformers' BertForSequenceClassification: eval forward, training forward + backward
(the word table's gradient included), one Trainer step, the embeddings kernel with half = 0 alone, checkpoint loading and the
cross-validation driver end to end. Bounds are those tests/test_finetune_gpu.py holds the STonKGs classifier to on the same
kernels."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden_util import GOLDEN
from tests.test_text_embed_cpu import (PAD, WORD, restatement_grads, text_batch, text_classifier, text_state_dict,
                                       tiny_config)

pytestmark = pytest.mark.gpu

LENGTHS = [1, 16, 100, 256, 60]
LM_DIR = os.path.join(GOLDEN, "g9_lm_backbone")
VOCAB_TXT = os.path.join(GOLDEN, "g10_tokenizer", "vocab.txt")


def _rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    if b.norm() < 1e-5:
        return (a - b).norm().item() / 1e-2
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def pinned():
    """Configuration, weights, the B = 5 batch and the restatement's loss / logits / gradients on it: computed once."""
    cfg = tiny_config()
    sd = text_state_dict(cfg)
    batch = text_batch(cfg, LENGTHS)
    loss, logits, grads = restatement_grads(sd, cfg, batch)
    return dict(cfg=cfg, sd=sd, batch=batch, loss=loss, logits=logits, grads=grads)


def _build(sd, cfg, num_labels=3):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.nlp_baseline_model import BertForSequenceClassification

    c = STonKGsConfig(**{k: getattr(cfg, k) for k in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads",
                                                      "intermediate_size", "max_position_embeddings", "type_vocab_size",
                                                      "layer_norm_eps")},
                      hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = BertForSequenceClassification(c, num_labels=num_labels)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return model


def test_eval_forward_matches_the_restatement(hip, pinned):
    cfg, sd, batch = pinned["cfg"], pinned["sd"], pinned["batch"]
    model = _build(sd, cfg)
    model.eval()
    with torch.no_grad():
        out = model(**batch, return_dict=True)
        loss, logits = model(**batch)
    assert out.logits.shape == (5, 3) and out.logits.dtype == torch.float32 and out.logits.device.type == "cuda"
    print("eval: loss", float(out.loss), "ref", float(pinned["loss"]), "logits rel", _rel(out.logits, pinned["logits"]))
    assert abs(float(out.loss) - float(pinned["loss"])) < 5e-3
    assert _rel(out.logits, pinned["logits"]) < 3e-2
    assert torch.equal(logits, out.logits) and float(loss) == float(out.loss)
    # L = 200 < S: right-padded on the device; without labels only the logits come back
    short = text_batch(cfg, [1, 16, 100, 200, 60], L=200, seed=6)
    with torch.no_grad():
        ref = text_classifier(sd, cfg, short["input_ids"], short["attention_mask"], short["token_type_ids"], short["labels"])
        out = model(**short, return_dict=True)
        (only_logits,) = model(short["input_ids"], short["attention_mask"], short["token_type_ids"])
    print("eval L=200: loss", float(out.loss), "ref", float(ref["loss"]), "logits rel", _rel(out.logits, ref["logits"]))
    assert abs(float(out.loss) - float(ref["loss"])) < 5e-3
    assert _rel(out.logits, ref["logits"]) < 3e-2 and torch.equal(only_logits, out.logits)
    with pytest.raises(ValueError):
        model(torch.zeros(2, 257, dtype=torch.long))
    model.engine.check_errors()


def test_training_forward_backward_matches_the_restatement(hip, pinned):
    cfg, sd, batch, grads = pinned["cfg"], pinned["sd"], pinned["batch"], pinned["grads"]
    model = _build(sd, cfg)
    model.train()
    model.zero_grad()
    loss, logits = model(**batch)           # p = 0: loss.backward() through the autograd bridge
    loss.backward()
    loss = loss.detach()
    params = dict(model.named_parameters())
    assert set(params) == set(grads)
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values()))
    ref_total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values()))
    print("train: loss", float(loss), "ref", float(pinned["loss"]), "grad norm", float(total), "ref", float(ref_total))
    assert abs(float(loss) - float(pinned["loss"])) < 5e-3
    assert abs(float(total) - float(ref_total)) < 4e-2 * float(ref_total)
    worst = max((_rel(params[k].grad, grads[k]), k) for k in grads)
    print("worst gradient tensor:", worst, "; word table:", _rel(params[WORD].grad, grads[WORD]))
    for k in grads:
        assert _rel(params[k].grad, grads[k]) < 8e-2, k
    dword = params[WORD].grad.cpu()
    ids = batch["input_ids"]
    assert (ids[batch["attention_mask"] == 1] == PAD).any()           # a [PAD] id at an attended position ...
    assert torch.count_nonzero(dword[PAD]) == 0                        # ... and its row is exactly zero
    absent = torch.ones(cfg.vocab_size, dtype=torch.bool)
    absent[ids.unique()] = False
    assert absent.sum() >= 20 and torch.count_nonzero(dword[absent]) == 0
    present = ~absent
    present[PAD] = False
    assert (dword[present].abs().amax(dim=1) > 0).all()
    # forward_backward = the autograd bridge
    bridge = {k: p.grad.clone() for k, p in params.items()}
    model.zero_grad()
    loss2 = model.forward_backward(batch)
    gv = model.named_grad_views()
    worst = max((_rel(gv[k], bridge[k]), k) for k in bridge)
    print("forward_backward vs bridge: loss", float(loss2), float(loss), "worst tensor", worst)
    assert abs(float(loss2) - float(loss)) < 1e-5
    for k in bridge:
        assert _rel(gv[k], bridge[k]) < 1e-5, k
    model.engine.check_errors()


def test_one_trainer_step_moves_exactly_the_rows_of_the_batch(hip, pinned):
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    cfg, sd, batch = pinned["cfg"], pinned["sd"], pinned["batch"]
    model = _build(sd, cfg)
    lr = 5e-5
    before = model.state_dict()[WORD].clone()
    trainer = Trainer(model, TrainingArguments(learning_rate=lr, max_steps=10, per_device_train_batch_size=5))
    loss = trainer.training_step(model, batch)
    torch.cuda.synchronize()
    model.engine.check_errors()
    before, after = before.cpu(), model.state_dict()[WORD].cpu()
    assert torch.equal(before, sd[WORD])
    moved = (after - before).abs()
    ids = batch["input_ids"]
    present = torch.zeros(cfg.vocab_size, dtype=torch.bool)
    present[ids[batch["attention_mask"] == 1].unique()] = True
    present[PAD] = False
    print("trainer step: loss", float(loss), "ref", float(pinned["loss"]), "largest move / lr", float(moved.max()) / lr,
          "smallest row move / lr", float(moved[present].amax(dim=1).min()) / lr)
    assert (moved[present].amax(dim=1) > 0).all() and moved.max() <= lr * 1.01
    # the first Adam step with a zero gradient is a zero update: absent ids and the pad row are bitwise unchanged
    assert torch.equal(after[~present], before[~present])
    assert abs(float(loss) - float(pinned["loss"])) < 5e-3


@pytest.mark.parametrize("packed", [False, True])
def test_embeddings_kernel_with_half_zero(hip, packed):
    """stonk_joint_embed_ln_fwd with half = 0, the fp32 word table as its table and kg_rows = vocab: word + position +
    token-type -> LayerNorm, on the padded and on the packed layout."""
    B, S, H, V = 3, 256, 128, 160
    g = torch.Generator(device="cuda").manual_seed(3)
    ids = torch.randint(0, V, (B, S), device="cuda", generator=g)
    tt = torch.randint(0, 2, (B, S), device="cuda", generator=g)
    word = torch.randn(V, H, device="cuda", generator=g) * 0.3
    pos = torch.randn(S, H, device="cuda", generator=g) * 0.02
    typ = torch.randn(2, H, device="cuda", generator=g) * 0.02
    gamma = torch.randn(H, device="cuda", generator=g) * 0.1 + 1
    beta = torch.randn(H, device="cuda", generator=g) * 0.1
    emb = word[ids] + pos[None] + typ[tt]
    ref_y = F.layer_norm(emb, (H,), gamma, beta, 1e-12)
    n = B * S
    pos_of_row, rows = None, n
    if packed:   # 301 rows: a shuffled subset of the positions, then a tail of -1 up to a multiple of 64
        keep = torch.randperm(n, device="cuda", generator=g)[:301].to(torch.int32)
        rows = 320
        pos_of_row = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        pos_of_row[:301] = keep
    ssum = torch.full((n, H), 7.0, device="cuda", dtype=torch.bfloat16)
    y = torch.full((n, H), 7.0, device="cuda", dtype=torch.bfloat16)
    mean = torch.empty(n, device="cuda")
    rstd = torch.empty(n, device="cuda")
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    hip.call("stonk_joint_embed_ln_fwd", hip.ptr(ids), hip.ptr(tt), hip.ptr(word), hip.ptr(word), hip.ptr(pos), hip.ptr(typ),
             hip.ptr(gamma), hip.ptr(beta), hip.ptr(ssum), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), B, S, 0, H, V, 2, 1e-12,
             0, 0.0, 0, hip.ptr(err), hip.ptr(pos_of_row), rows if packed else 0, hip.stream_ptr())
    torch.cuda.synchronize()
    assert err.item() == 0
    if packed:
        sel = keep.long()
        want_sum, want_y = emb.view(n, H)[sel], ref_y.view(n, H)[sel]
        got_sum, got_y, got_mean = ssum[:301].float(), y[:301].float(), mean[:301]
        assert torch.count_nonzero(y[301:rows]) == 0 and torch.count_nonzero(ssum[301:rows]) == 0   # the tail: zeros
        assert (y[rows:] == 7.0).all()                                                             # beyond n_rows: untouched
    else:
        want_sum, want_y = emb.view(n, H), ref_y.view(n, H)
        got_sum, got_y, got_mean = ssum.float(), y.float(), mean
    torch.testing.assert_close(got_sum, want_sum, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(got_y, want_y, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(got_mean, want_sum.mean(-1), rtol=1e-4, atol=1e-4)
    ids[1, 5] = V   # out of the table
    hip.call("stonk_joint_embed_ln_fwd", hip.ptr(ids), hip.ptr(tt), hip.ptr(word), hip.ptr(word), hip.ptr(pos), hip.ptr(typ),
             hip.ptr(gamma), hip.ptr(beta), hip.ptr(ssum), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), B, S, 0, H, V, 2, 1e-12,
             0, 0.0, 0, hip.ptr(err), 0, 0, hip.stream_ptr())
    assert err.item() & 1


def test_from_pretrained_round_trip_and_out_of_range_ids(hip, tmp_path):
    from stonkgs_amd.nlp_baseline_model import BertForSequenceClassification
    from stonkgs_amd.stonkgs_model import _load_weights_file

    with pytest.warns(UserWarning, match="newly initialized"):
        model = BertForSequenceClassification.from_pretrained(LM_DIR, num_labels=4)
    ckpt = _load_weights_file(LM_DIR)
    sd = model.state_dict()
    assert model.num_labels == 4 and sd["classifier.weight"].shape == (4, 128)
    for k, v in ckpt.items():   # a BertModel checkpoint: bare keys
        assert torch.equal(sd["bert." + k].cpu(), v), k
    assert set(sd) == {"bert." + k for k in ckpt} | {"classifier.weight", "classifier.bias"}
    for safe in (False, True):
        d = str(tmp_path / f"saved{int(safe)}")
        model.save_pretrained(d, safe_serialization=safe)
        again = BertForSequenceClassification.from_pretrained(d)
        sd2 = again.state_dict()
        assert again.num_labels == 4 and set(sd2) == set(sd) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    ids = torch.randint(1, 160, (2, 40))
    model.eval()
    with torch.no_grad():
        model(ids)
    model.engine.check_errors()
    ids[1, 7] = 160
    with torch.no_grad():
        model(ids)
    with pytest.raises(IndexError):
        model.engine.check_errors()
    model.engine.check_errors()   # (the flag is cleared by the raise)
    # ... and in training: the backward kernel raises the same flag and adds nothing for that position
    model.train()
    model.zero_grad()
    model.forward_backward({"input_ids": ids, "labels": torch.tensor([0, 3])})
    with pytest.raises(IndexError):
        model.engine.check_errors()


# ---------------------------------------------------------------------------------------------------- the driver
FILLER = ("the of and in protein kinase binds phosphorylates cell expression receptor complex growth factor signal pathway "
          "tumor akt mtor p53 by to a is with").split()
MARKERS = {"up": "activates", "down": "inhibits"}
CV = dict(epochs=20, lr=1e-3, batch_size=8, n_splits=3, seed=42)


def marker_rows(n=30, seed=1):
    """(evidence, class) rows from the golden tokenizer's words: the class is decided by which marker word occurs."""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        cls = "up" if i % 2 else "down"
        words = list(rng.choice(FILLER, size=rng.randint(4, 12)))
        words.insert(rng.randint(0, len(words) + 1), MARKERS[cls])
        rows.append((" ".join(words), cls))
    return rows


def write_marker_tsv(path, rows):
    import pandas as pd

    pd.DataFrame({"source": [f"n{i}" for i in range(len(rows))], "target": [f"m{i}" for i in range(len(rows))],
                  "evidence": [r[0] for r in rows], "class": [r[1] for r in rows]}).to_csv(path, sep="\t", index=False)


def test_cross_validation_driver_learns_the_marker_word(hip, tmp_path):
    """The TSV, the tokenizer, a fresh model per fold, Trainer steps with a ragged last batch, batched prediction, weighted
    F1. The fp32 restatement trained with torch.optim.AdamW on the same rows, splits, batches and schedule (seed 42, 20
    epochs, lr 1e-3) reaches a weighted F1 of 1.0 on every fold on the CPU (10 epochs: 0.74, one fold not yet separated) -
    the bar below tests the path and not the task."""
    from stonkgs_amd.nlp_baseline_model import run_nlp_baseline_classification_cv

    rows = marker_rows()
    path = str(tmp_path / "train.tsv")
    write_marker_tsv(path, rows)
    res = run_nlp_baseline_classification_cv(path, "\t", model_type=LM_DIR, vocab_file_path=VOCAB_TXT,
                                             output_dir=str(tmp_path / "out"), task_name="t", **CV)
    frame = res["result_df"]
    print("f1 per fold", res["f1_scores"])
    assert set(res) >= {"f1_score_mean", "f1_score_std"} and len(res["f1_scores"]) == 3
    assert list(frame.columns) == ["split", "index", "predicted_label", "true_label", "evidence"]
    assert len(frame) == len(rows) and sorted(frame["index"].tolist()) == list(range(len(rows)))
    assert all(frame["evidence"][i] == rows[frame["index"][i]][0] and frame["true_label"][i] == rows[frame["index"][i]][1]
               for i in range(len(frame)))
    assert set(frame["predicted_label"]) <= {"up", "down"}
    assert os.path.exists(str(tmp_path / "out" / "predicted_labels_nlp_tdf.tsv"))
    assert res["f1_score_mean"] == pytest.approx(float(np.mean(res["f1_scores"])))
    assert res["f1_score_mean"] > 0.75, res["f1_scores"]
