"""Text-only baseline: a BERT sequence classifier fine-tuned through the HIP path.

Mirror of ref:src/stonkgs/models/nlp_baseline_model.py - the second baseline the reference evaluates STonKGs against on
every fine-tuning task (the first, KG only, is ``kg_baseline_model.py``): BioBERT as
``AutoModelForSequenceClassification`` on the text evidence alone, 5-fold cross-validation, weighted F1.

* ``BertForSequenceClassification``: HF's module contract (state-dict keys, ``from_pretrained`` / ``save_pretrained``,
  ``forward`` signature and return packing) on ``engine.TextEngine`` - word + position + token-type embeddings with a
  TRAINABLE word table (its gradient: csrc/text_embed.hip), the packed-row encoder, pooler -> dropout -> classifier ->
  cross-entropy. No arithmetic runs in torch.
* ``INDRAEvidenceDataset`` (:47-64), ``get_train_test_splits`` (:67-100), ``run_nlp_baseline_classification_cv``
  (:103-277) and a command line in the style of the KG baseline's.

One stated deviation: the label map is ``sorted(set(labels))`` - the reference enumerates a ``set`` of strings, whose
order changes from run to run. Not mirrored, as in the other drivers: mlflow, DeepSpeed, pystow paths. Everything is read
from LOCAL files (``model_type`` is a directory, never a hub name)."""
from __future__ import annotations

import logging
import math
import os
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

from . import _hip as hip
from . import stonkgs_finetuning as _ft
from .config import STonKGsConfig
from .engine import TextEngine
from .params import FlatStore, _linear, build_bert_tree, trainable_specs
from .stonkgs_model import (STonKGsForPreTraining, SequenceClassifierOutput, _ClsStepFunction, _load_weights_file)

logger = logging.getLogger(__name__)

WORD = TextEngine.WORD


class BertForSequenceClassification(STonKGsForPreTraining):
    """hf:models/bert/modeling_bert.py BertForSequenceClassification as the reference uses it (:171-173), single-label
    cross-entropy. Inherits the flat-buffer plumbing of the STonKGs models (gradient views, ``zero_grad``, the autograd
    bridge, ``state_dict`` / ``save_pretrained``, ``Trainer`` compatibility) and none of their front: no frozen backbone,
    no entity table, no pre-training heads. ``input_ids`` may be ``[B, L]`` with any ``L <= max_position_embeddings``
    (the reference pads to the longest text of the split, :176-181): the batch is right-padded to the model's length on
    the device with mask 0, which the packed-row encoder drops again."""

    def __init__(self, config, num_labels: Optional[int] = None, *, device=None, seed: int = 0):
        nn.Module.__init__(self)
        if not torch.cuda.is_available():
            raise hip.StonkHipError("BertForSequenceClassification needs an MI355X: the hot path has no CPU fallback")
        self._device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        cfg = STonKGsConfig.from_any(config)
        if num_labels is not None:
            cfg.num_labels = int(num_labels)
        cfg.validate_for_hip()
        self.config = cfg
        self.num_labels = cfg.num_labels
        dev, H = self._device, cfg.hidden_size
        # backward-completion order, as for the STonKGs models: classifier first, the word table last (its gradient is the
        # last kernel of backward, behind the position / token-type gradients)
        specs = [("classifier.weight", (cfg.num_labels, H), None), ("classifier.bias", (cfg.num_labels,), None)]
        specs += trainable_specs(cfg, False) + [(WORD, (cfg.vocab_size, H), None)]
        self._store = FlatStore(specs, dev, trainable=True)
        self.bert = build_bert_tree(self._store, "bert", cfg, cfg.num_hidden_layers, True, None)
        self.dropout = nn.Dropout(cfg.hidden_dropout_prob)   # naming only; the engine applies it (classifier dropout =
        self.classifier = _linear(self._store, "classifier", True)   # hidden_dropout_prob: classifier_dropout is None)
        self.engine = TextEngine(cfg, self._store, dev)
        self._segment_hook = None
        self._anchor = torch.zeros((), device=dev, requires_grad=True)
        self._init_weights(seed)
        self._grad_views = {n: p.grad for n, p in self.named_parameters() if p.requires_grad}
        self.refresh()

    def _init_weights(self, seed: int) -> None:
        """BERT init (hf _init_weights: N(0, initializer_range) matrices / embeddings with a zero padding row, zero bias,
        unit LayerNorm)."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        std = self.config.initializer_range
        with torch.no_grad():
            for name, (off, shape, _) in self._store.index.items():
                v = self._store.view(name)
                if "LayerNorm.weight" in name:
                    v.fill_(1.0)
                elif name.endswith(".bias"):
                    v.zero_()
                else:
                    v.copy_((torch.randn(shape, generator=g) * std).to(v.device))
            self._store.view(WORD)[TextEngine.PADDING_IDX].zero_()

    # -------------------------------------------------------------- masters <-> derived copies (one store)
    def refresh(self) -> None:
        self.engine.refresh_derived(bf16_mirror=True)
        self._mark_synced()

    def _mark_synced(self, clear_pending: bool = True) -> None:
        self._synced_versions = (self._store.data._version,)
        if clear_pending:
            self._external_step_pending = False

    def _sync_derived(self) -> None:
        v = (self._store.data._version,)
        if v == self._synced_versions and not self._external_step_pending:
            return
        self._wait_params()
        self.engine.refresh_derived(bf16_mirror=True)
        self._mark_synced(clear_pending=v != self._synced_versions)

    # -------------------------------------------------------------- loaders
    @classmethod
    def from_pretrained(cls, path: str, num_labels: Optional[int] = None, **kwargs) -> "BertForSequenceClassification":
        """Local directory in HF layout holding a ``BertModel`` (bare keys), ``BertForPreTraining`` (``bert.`` keys, its
        ``cls.*`` heads ignored) or ``BertForSequenceClassification`` checkpoint. A checkpoint without a classifier gets a
        freshly initialised one, as ``AutoModelForSequenceClassification.from_pretrained(BioBERT)`` does."""
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path!r}: only local checkpoints can be loaded (no network)")
        cfg = STonKGsConfig.from_pretrained(path)
        model = cls(cfg, num_labels=num_labels, **kwargs)
        sd = _load_weights_file(path)
        if sd is None:
            raise FileNotFoundError(f"no pytorch_model.bin / model.safetensors under {path!r}")
        sd = {(k if k.startswith(("bert.", "classifier.")) else "bert." + k): v
              for k, v in sd.items() if not k.startswith("cls.") and not k.endswith("position_ids")}
        missing, _ = model.load_state_dict(sd, strict=False)
        bad = [k for k in missing if not k.startswith("classifier.")]
        if bad:
            raise KeyError(f"checkpoint misses {bad[:5]}...")
        if missing:
            import warnings

            warnings.warn(f"Some weights of {cls.__name__} were not initialized from the checkpoint at {path} and are "
                          f"newly initialized: {missing}. You should probably TRAIN this model on a down-stream task.")
        return model

    @classmethod
    def from_default_pretrained(cls, **kwargs):
        raise NotImplementedError("pass a local directory to from_pretrained")

    # -------------------------------------------------------------- forward
    def _prep(self, t):
        if t is None:
            return None
        t = torch.as_tensor(t)
        if t.device != self._device or t.dtype != torch.long or not t.is_contiguous():
            t = t.to(device=self._device, dtype=torch.long).contiguous()
        return t

    def _inputs(self, input_ids, attention_mask, token_type_ids):
        """[B, L] -> contiguous int64 [B, S] on the device: right-padded with [PAD] / mask 0 / type 0. No attention mask =
        every given position is attended, as in HF."""
        if input_ids is None:
            raise ValueError("input_ids is required")
        S = self.config.max_position_embeddings
        ids, am, tt = self._prep(input_ids), self._prep(attention_mask), self._prep(token_type_ids)
        if ids.dim() != 2 or ids.shape[1] > S or ids.shape[1] < 1:
            raise ValueError(f"input_ids must be [B, L] with 1 <= L <= {S}")
        if am is None:
            am = torch.ones_like(ids)
        pad = S - ids.shape[1]
        if pad:
            ids, am = nn.functional.pad(ids, (0, pad), value=TextEngine.PADDING_IDX), nn.functional.pad(am, (0, pad))
            tt = None if tt is None else nn.functional.pad(tt, (0, pad))
        return ids, am, tt

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, labels=None, return_dict=None):
        ids, am, tt = self._inputs(input_ids, attention_mask, token_type_ids)
        lab = None if labels is None else self._prep(torch.as_tensor(labels).reshape(-1))
        training = self.training
        self._sync_derived()
        need_bwd = lab is not None and torch.is_grad_enabled() and training
        out = self.engine.forward_cls(ids, am, tt, lab, self.num_labels, training, need_bwd)
        loss = None
        if lab is not None:
            loss = _ClsStepFunction.apply(self._anchor, self, out["loss"]) if need_bwd else out["loss"].clone()
        logits = out["logits"].clone()
        if not return_dict:
            return (loss, logits) if loss is not None else (logits,)
        return SequenceClassifierOutput(loss=loss, logits=logits, hidden_states=None, attentions=None)

    def forward_backward(self, inputs, gscale: float = 1.0, on_segment_done=None):
        ids, am, tt = self._inputs(inputs["input_ids"], inputs.get("attention_mask"), inputs.get("token_type_ids"))
        lab = self._prep(torch.as_tensor(inputs["labels"]).reshape(-1))
        self._sync_derived()
        out = self.engine.forward_cls(ids, am, tt, lab, self.num_labels, self.training, True)
        loss = out["loss"].clone()
        self.engine.backward_cls(gscale, on_segment_done)
        return loss

    def _stonkgs_only(self, *args, **kwargs):
        raise NotImplementedError("not available on the text-only model (attention maps, input attributions and the masked "
                                  "prediction helpers belong to the STonKGs models)")

    encode = attention_maps = input_attributions = evaluate_batch = predict_masked = entity_names = _stonkgs_only


# ---------------------------------------------------------------------------------------------------- the driver
class INDRAEvidenceDataset(torch.utils.data.Dataset):
    """ref:nlp_baseline_model.py:47-64: the tokenizer's encodings + numerically encoded labels -> per-item dicts."""

    def __init__(self, encodings, labels):
        self.encodings = encodings
        self.labels = labels

    def __getitem__(self, idx):
        item = {key: torch.tensor(val[idx]) for key, val in self.encodings.items()}
        item["labels"] = torch.tensor(self.labels[idx])
        return item

    def __len__(self):
        return len(self.labels)


def get_train_test_splits(data, max_dataset_size: int = 100000, label_column_name: str = "class", random_seed: int = 42,
                          n_splits: int = 5) -> List[Dict[str, np.ndarray]]:
    """ref:nlp_baseline_model.py:67-100: the same scikit-learn calls as ``stonkgs_finetuning.get_train_test_splits``."""
    return _ft.get_train_test_splits(data, label_column_name, random_seed, n_splits, max_dataset_size)


def run_nlp_baseline_classification_cv(train_data_path: str, sep: Optional[str] = "\t", model_type: Optional[str] = None,
                                       label_column_name: str = "class", text_data_column_name: str = "evidence",
                                       epochs: int = 10, lr: float = 5e-5, batch_size: int = 16,
                                       gradient_accumulation: int = 1, embedding_path: Optional[str] = None,
                                       max_dataset_size: int = 100000, vocab_file_path: Optional[str] = None,
                                       n_splits: int = 5, seed: int = 42, task_name: str = "",
                                       output_dir: Optional[str] = None) -> Dict:
    """ref:nlp_baseline_model.py:103-277. ``model_type``: LOCAL directory of the pre-trained BERT (config.json + weights,
    and vocab.txt unless ``vocab_file_path`` names one). ``embedding_path`` (optional): keep only the triples whose
    ``source`` and ``target`` have a row in that embedding table, as the reference does. Per fold: a fresh model from the
    pre-trained weights, the split tokenised with ``truncation=True, padding=True``, ``Trainer`` steps in RandomSampler
    order (ragged last batch), eval-mode prediction in batches, arg-max, weighted F1. Returns ``{"f1_score_mean",
    "f1_score_std"}`` as the reference, plus ``"f1_scores"`` (per fold) and ``"result_df"`` (``split``, ``index``,
    ``predicted_label``, ``true_label`` - both by name - and ``evidence``); with ``output_dir`` the frame is also written
    to ``predicted_labels_nlp_<task_name>df.tsv`` there."""
    import pandas as pd

    from .stonkgs_for_embeddings import _local_tokenizer
    from .stonkgs_pretraining import Trainer, TrainingArguments

    if model_type is None or not os.path.isdir(model_type):
        raise FileNotFoundError(f"model_type = {model_type!r}: pass the local directory of the pre-trained BERT (hub names "
                                "cannot be fetched)")
    indra_data = pd.read_csv(train_data_path, sep=sep)
    if embedding_path is not None:
        from .kg_baseline_model import filter_triples
        from .stonkgs_model import prepare_df

        original_length = len(indra_data)
        indra_data, left_out = filter_triples(indra_data, prepare_df(embedding_path).keys())
        logger.info(f"{left_out} out of {original_length} triples are left out because they contain nodes which are not "
                    f"present in the pre-training data")
    splits = get_train_test_splits(indra_data, max_dataset_size, label_column_name, seed, n_splits)
    evidences_text, labels_str = indra_data[text_data_column_name], indra_data[label_column_name]
    id2tag = sorted(set(labels_str))   # (the reference enumerates the set itself: an order that changes between runs)
    tag2id = {tag: i for i, tag in enumerate(id2tag)}
    labels = np.array([tag2id[tag] for tag in labels_str], dtype=np.int64)
    tokenizer = _local_tokenizer(vocab_file_path, None) if vocab_file_path is not None else _local_tokenizer(None, model_type)
    max_length = STonKGsConfig.from_pretrained(model_type).max_position_embeddings

    f1_scores, frames = [], []
    for idx, indices in enumerate(splits):
        tr_idx, te_idx = indices["train_idx"], indices["test_idx"]
        model = BertForSequenceClassification.from_pretrained(model_type, num_labels=len(id2tag), seed=seed + idx)
        train_ds, test_ds = (INDRAEvidenceDataset(
            tokenizer(evidences_text[ix].tolist(), truncation=True, padding=True, max_length=max_length), labels[ix].tolist())
            for ix in (tr_idx, te_idx))
        steps_per_epoch = max(1, math.ceil(len(train_ds) / (batch_size * gradient_accumulation)))
        args = TrainingArguments(learning_rate=lr, max_steps=epochs * steps_per_epoch,
                                 per_device_train_batch_size=batch_size, gradient_accumulation_steps=gradient_accumulation,
                                 seed=seed, logging_steps=max(1, steps_per_epoch))
        model.train()
        trainer = Trainer(model, args)
        g = torch.Generator().manual_seed(seed + idx)
        for _ in range(epochs):                       # RandomSampler order per epoch; the last batch may be ragged
            perm = torch.randperm(len(train_ds), generator=g).tolist()
            for lo in range(0, len(perm), batch_size):
                trainer.training_step(model, _ft._collate([train_ds[i] for i in perm[lo:lo + batch_size]]))
        model.engine.check_errors()
        predicted = np.argmax(_ft.predict_logits(model, test_ds, batch_size), axis=1)
        model.engine.check_errors()
        f1_scores.append(_ft.weighted_f1_score(labels[te_idx], predicted))
        frames.append(pd.DataFrame({"split": idx, "index": te_idx.tolist(),
                                    "predicted_label": [id2tag[i] for i in predicted],
                                    "true_label": [id2tag[i] for i in labels[te_idx]],
                                    "evidence": evidences_text[te_idx].tolist()}))
    result_df = pd.concat(frames, ignore_index=True)
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        result_df.to_csv(os.path.join(output_dir, "predicted_labels_nlp_" + task_name + "df.tsv"), index=False, sep="\t")
    logger.info(f"Mean f1-score: {np.mean(f1_scores)}")
    logger.info(f"Std f1-score: {np.std(f1_scores)}")
    return {"f1_score_mean": float(np.mean(f1_scores)), "f1_score_std": float(np.std(f1_scores)), "f1_scores": f1_scores,
            "result_df": result_df}


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="NLP baseline (a BERT sequence classifier on the text evidence), cross-validated")
    ap.add_argument("--train_data_path", required=True, help="TSV with the evidence and the label column")
    ap.add_argument("--model_type", required=True, help="local directory of the pre-trained BERT (config.json, weights, vocab.txt)")
    ap.add_argument("--vocab_file_path", default=None, help="vocab.txt, if the model directory holds none")
    ap.add_argument("--embedding_path", default=None, help="embedding table TSV: keep only triples whose nodes it knows")
    ap.add_argument("--label_column_name", default="class")
    ap.add_argument("--text_data_column_name", default="evidence")
    ap.add_argument("-e", "--epochs", type=int, default=5)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--gradient_accumulation_steps", type=int, default=1)
    ap.add_argument("--max_dataset_size", type=int, default=100000)
    ap.add_argument("--task_name", default="")
    ap.add_argument("--output_dir", default=None)
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    res = run_nlp_baseline_classification_cv(
        args.train_data_path, model_type=args.model_type, label_column_name=args.label_column_name,
        text_data_column_name=args.text_data_column_name, epochs=args.epochs, lr=args.lr, batch_size=args.batch_size,
        gradient_accumulation=args.gradient_accumulation_steps, embedding_path=args.embedding_path,
        max_dataset_size=args.max_dataset_size, vocab_file_path=args.vocab_file_path, task_name=args.task_name,
        output_dir=args.output_dir)
    print({k: res[k] for k in ("f1_score_mean", "f1_score_std")})


if __name__ == "__main__":
    main()
