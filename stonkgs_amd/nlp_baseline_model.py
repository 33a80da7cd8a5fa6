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
import os
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

from . import stonkgs_finetuning as _ft
from .config import STonKGsConfig
from .engine import TextEngine
from .flat_model import FlatBufferModel, SequenceClassifierFront, _load_weights_file
from .params import FlatStore, _linear, build_bert_tree, trainable_specs

logger = logging.getLogger(__name__)

WORD = TextEngine.WORD


class BertForSequenceClassification(SequenceClassifierFront, FlatBufferModel):
    """hf:models/bert/modeling_bert.py BertForSequenceClassification as the reference uses it (:171-173), single-label
    cross-entropy. Shares ``FlatBufferModel`` with the STonKGs models (gradient views, ``zero_grad``, the autograd
    bridge, ``state_dict`` / ``save_pretrained``, ``Trainer`` compatibility) and the classifier front with the STonKGs
    fine-tuning model, and has none of the STonKGs front: no frozen backbone, no entity table, no pre-training heads.
    ``input_ids`` may be ``[B, L]`` with any ``L <= max_position_embeddings`` (the reference pads to the longest text of
    the split, :176-181): the batch is right-padded to the model's length on the device with mask 0, which the packed-row
    encoder drops again."""

    def __init__(self, config, num_labels: Optional[int] = None, *, device=None, seed: int = 0):
        super().__init__(device)
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
        self._init_weights(seed)
        self._bind_grad_views()
        self.refresh()

    def _stores(self) -> tuple:
        return (self._store,)

    def _after_init_weights(self) -> None:
        self._store.view(WORD)[TextEngine.PADDING_IDX].zero_()   # hf _init_weights: the embedding's padding row is zero

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

    # -------------------------------------------------------------- forward
    def _inputs(self, input_ids, attention_mask, token_type_ids):
        """[B, L] -> contiguous int64 [B, S] on the device: right-padded with [PAD] / mask 0 / type 0. No attention mask =
        every given position is attended, as in HF."""
        if input_ids is None:
            raise ValueError("input_ids is required")
        S = self.config.max_position_embeddings
        ids, am, tt = self._long(input_ids), self._long(attention_mask), self._long(token_type_ids)
        if ids.dim() != 2 or ids.shape[1] > S or ids.shape[1] < 1:
            raise ValueError(f"input_ids must be [B, L] with 1 <= L <= {S}")
        if am is None:
            am = torch.ones_like(ids)
        pad = S - ids.shape[1]
        if pad:
            ids, am = nn.functional.pad(ids, (0, pad), value=TextEngine.PADDING_IDX), nn.functional.pad(am, (0, pad))
            tt = None if tt is None else nn.functional.pad(tt, (0, pad))
        return ids, am, tt

    def _cls_inputs(self, input_ids, attention_mask, token_type_ids, labels):
        ids, am, tt = self._inputs(input_ids, attention_mask, token_type_ids)
        lab = None if labels is None else self._long(torch.as_tensor(labels).reshape(-1))
        return ids, am, tt, lab, None   # (single-label cross-entropy)

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, labels=None, return_dict=None):
        return self._classify(*self._cls_inputs(input_ids, attention_mask, token_type_ids, labels), return_dict)


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
        predicted = np.argmax(_ft.train_and_predict_fold(
            model, train_ds, test_ds, epochs=epochs, lr=lr, batch_size=batch_size,
            gradient_accumulation=gradient_accumulation, seed=seed, fold=idx), axis=1)
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
