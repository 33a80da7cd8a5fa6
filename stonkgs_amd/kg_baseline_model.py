"""KG baseline on the fine-tuning classification tasks: max-pooled walk embeddings and one linear layer, 5-fold cross-validated.
Mirrors the surface of ref:src/stonkgs/models/kg_baseline_model.py, the knowledge-graph-only baseline every STonKGs
fine-tuning result is compared against. Run with::

    python -m stonkgs_amd.kg_baseline_model --triples_path task.tsv --embedding_path embeddings_best_model.tsv \
        --random_walks_path random_walks_best_model.tsv

What differs from the reference, and why:

* Its datasets materialise an [n, L, D] float64 array on the host (156 GB at n 100 000, L 254, D 768). Here a dataset holds
  the int32 id matrix [n, L] and the fp32 table; ``.pooled`` is one gather-and-max pass on the GPU (``stonk_walk_maxpool``).
  The pooled features are the same in every epoch, because the model's dropout comes AFTER the pooling.
* Its lightning loop makes 10^6 optimizer steps per fold at batch 8. Here ``stonk_kgb_train_steps`` walks up to
  ``max_steps()`` steps per launch with the model on chip, all folds side by side, one workgroup per fold.
* The step itself is the reference's, quirk included: ``forward`` returns probabilities and ``CrossEntropyLoss`` takes a
  second log-softmax over them.
* The label map is the SORTED list of label values (the reference enumerates a Python set, whose order is not fixed for
  strings); predictions stay aligned with ``index`` in the result frame (the reference pairs them with a shuffled sampler).
* mlflow logging and lightning checkpoints are not mirrored.
* Kept as in the reference: above ``max_dataset_size`` triples the fold indices are positions in the cut data and are
  applied to the uncut dataset (see ``run_kg_baseline_classification_cv``).

The kernels have no CPU fallback: ``.pooled``, ``fit``, ``predict`` and ``forward`` raise without an MI355X. Everything that
prepares their inputs (id matrices, the triple filter, class weights, epoch orders, launch spans) is plain numpy.
"""
from __future__ import annotations

import logging
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _hip as hip
from .graph_common import as_tensor, need_gpu, to_device
from .stonkgs_finetuning import get_train_test_splits, weighted_f1_score
from .stonkgs_model import prepare_df

logger = logging.getLogger(__name__)

DROPOUT = 0.1            # ref:kg_baseline_model.py:71
WEIGHT_DECAY = 0.01      # torch.optim.AdamW's default, which the reference gets (:102)
BETAS, EPS = (0.9, 0.999), 1e-8
_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- the dropout rule
def _hash32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def dropout_keep_mask(seed: int, run: int, global_step: int, batch: int, d_in: int, p: float) -> np.ndarray:
    """bool [batch, d_in]: the keep decisions of ``stonk_kgb_train_steps`` for one step, restated in numpy (csrc/common.h:
    ``stonk_keep``; csrc/graph_common.h: ``n2v_key``). A pure function of (seed, run, global step, row in batch, feature)."""
    seedkey = _hash32(((seed & _M32) * 0x9E3779B9 + 0x85EBCA6B) & _M32)
    stepkey = _hash32(_hash32((seedkey + run) & _M32) ^ (((global_step & _M32) * 0x9E3779B1) & _M32))
    thr = min(max(float(np.float32(p)) * 4294967296.0, 0.0), 4294967295.0)
    thr = np.uint64(int(thr + 0.5))
    rowkey = (np.arange(batch, dtype=np.uint64)[:, None] * 0x9E3779B1 + stepkey) & _M32
    colkey = (np.arange(d_in, dtype=np.uint64)[None, :] * 0x85EBCA77) & _M32
    x = rowkey ^ colkey
    y = ((x & 0xFFFFFF) * 0xB5297B + x) & _M32
    z = ((y >> 8) * 0x68E31D) & _M32
    return z >= thr


# ---------------------------------------------------------------------------------------------------- host preparation
def embedding_table(embedding_dict: Dict) -> Tuple[Dict, np.ndarray]:
    """``({name: row}, fp32 [N, D])`` in the dict's order; the reference's key -1 (its null vector) is no row."""
    names = [k for k in embedding_dict if not (isinstance(k, (int, np.integer)) and k == -1)]
    table = np.ascontiguousarray(np.stack([np.asarray(embedding_dict[k], dtype=np.float32) for k in names]))
    return {k: i for i, k in enumerate(names)}, table


def node2vec_id_matrix(row_of: Dict, random_walk_dict: Dict, sources, targets, max_len: int = 254) -> np.ndarray:
    """int32 [n, max_len]: the table rows of walk(source) + walk(target) per triple (ref :189-203). A walk node without a
    row - and the reference's key -1 - becomes -1, the null vector."""
    cache: Dict = {}

    def rows(name):
        got = cache.get(name)
        if got is None:
            got = np.array([row_of.get(node, -1) for node in np.asarray(random_walk_dict[name]).tolist()], dtype=np.int32)
            cache[name] = got
        return got

    sources, targets = list(sources), list(targets)
    ids = np.empty((len(sources), max_len), dtype=np.int32)
    for i, (s, t) in enumerate(zip(sources, targets)):
        walk = np.concatenate([rows(s), rows(t)])
        if len(walk) != max_len:
            raise ValueError(f"triple {i}: the two walks have {len(walk)} nodes, max_len is {max_len}")
        ids[i] = walk
    return ids


def transe_id_matrix(row_of: Dict, sources, relations, targets) -> np.ndarray:
    """int32 [n, 3]: rows of (source, relation, target) (ref :252-265); a name without a row becomes -1."""
    cols = [[row_of.get(x, -1) for x in col] for col in (sources, relations, targets)]
    return np.ascontiguousarray(np.array(cols, dtype=np.int32).T.reshape(-1, 3))


def filter_triples(triples_df, known) -> Tuple["object", int]:
    """Drop the triples whose source or target has no embedding (ref :356-359). Returns ``(frame, number left out)``."""
    keep = triples_df["source"].isin(known) & triples_df["target"].isin(known)
    return triples_df[keep].reset_index(drop=True), int((~keep).sum())


def inverse_count_class_weights(labels, train_idx, num_classes: int) -> np.ndarray:
    """fp32 [C]: 1 / (number of TRAINING examples of the class) - the test indices are not looked at (ref :419-430)."""
    counts = np.bincount(np.asarray(labels)[np.asarray(train_idx)], minlength=num_classes)
    if (counts == 0).any():
        raise ValueError(f"classes {np.flatnonzero(counts == 0).tolist()} have no training example in this fold")
    return (1.0 / counts).astype(np.float32)


def epoch_order(train_idx, seed: int, run: int, epoch: int) -> np.ndarray:
    """A seeded permutation of the fold's training indices: what ``SubsetRandomSampler`` draws in the reference (:415)."""
    return np.random.default_rng([seed & _M32, run, epoch]).permutation(np.asarray(train_idx)).astype(np.int32)


def steps_per_epoch(n_train: int, batch_size: int) -> int:
    return -(-int(n_train) // int(batch_size))


def cut_epoch(order: np.ndarray, batch_size: int, cap: int) -> List[np.ndarray]:
    """The epoch's order as spans of at most ``cap`` steps: int32 arrays of (steps * batch_size) entries, the ragged last
    batch padded with -1. Without the padding their concatenation is ``order``."""
    order = np.asarray(order, dtype=np.int32)
    steps = steps_per_epoch(len(order), batch_size)
    padded = np.full(steps * batch_size, -1, dtype=np.int32)
    padded[:len(order)] = order
    return [padded[lo * batch_size:min(lo + cap, steps) * batch_size] for lo in range(0, steps, cap)]


def max_steps() -> int:
    """Steps one launch of ``stonk_kgb_train_steps`` may walk (its compile-time cap)."""
    return int(hip.lib().stonk_kgb_max_steps())


# ---------------------------------------------------------------------------------------------------- kernels
NO_GPU = "the KG baseline kernels need an MI355X: there is no CPU fallback"


def walk_maxpool(ids, table):
    """``pooled[e] = max_t table[ids[e, t]]`` (fp32 [n, D], device) by ``stonk_walk_maxpool``; id -1 is a row of zeros.
    Raises if an id lies outside [-1, N)."""
    torch = need_gpu(NO_GPU)
    ids, table = as_tensor(ids, torch.int32).cuda(), as_tensor(table, torch.float32).cuda()
    if ids.dtype != torch.int32 or ids.dim() != 2 or ids.stride(1) != 1 or table.dtype != torch.float32 or \
            table.dim() != 2 or table.stride(1) != 1:
        raise ValueError("ids: int32 [n, L]; table: fp32 [N, D]; both with contiguous rows")
    pooled = torch.empty(ids.shape[0], table.shape[1], dtype=torch.float32, device=table.device)
    errors = torch.zeros(1, dtype=torch.int32, device=table.device)
    hip.call("stonk_walk_maxpool", hip.ptr(ids), ids.stride(0), ids.shape[0], ids.shape[1], hip.ptr(table), table.stride(0),
             table.shape[0], table.shape[1], hip.ptr(pooled), pooled.stride(0), hip.ptr(errors), hip.stream_ptr())
    bad = int(errors.item())
    if bad:
        raise hip.StonkHipError(f"walk_maxpool: {bad} examples name a table row outside [-1, {table.shape[0]})")
    return pooled


def kgb_predict(pooled, idx, weight, bias) -> Tuple[np.ndarray, np.ndarray]:
    """``(probabilities fp32 [k, C], arg-max int32 [k])`` of the examples ``idx`` by ``stonk_kgb_predict`` (eval mode)."""
    torch = need_gpu(NO_GPU)
    dev = pooled.device
    idx = to_device(idx, torch.int32, dev)
    weight, bias = to_device(weight, torch.float32, dev), to_device(bias, torch.float32, dev)
    C = weight.shape[0]
    probs = torch.empty(idx.shape[0], C, dtype=torch.float32, device=dev)
    pred = torch.empty(idx.shape[0], dtype=torch.int32, device=dev)
    errors = torch.zeros(1, dtype=torch.int32, device=dev)
    hip.call("stonk_kgb_predict", hip.ptr(pooled), pooled.stride(0), pooled.shape[0], pooled.shape[1], hip.ptr(idx),
             idx.shape[0], hip.ptr(weight), hip.ptr(bias), C, hip.ptr(probs), hip.ptr(pred), hip.ptr(errors), hip.stream_ptr())
    if int(errors.item()):
        raise hip.StonkHipError("kgb_predict: an example index lies outside the dataset")
    return probs.cpu().numpy(), pred.cpu().numpy()


class KGBTrainer:
    """R runs (folds) of the baseline's classifier trained side by side: the device state [R, C, D] of W, b and AdamW's
    moments, and ``run_spans``, one launch of ``stonk_kgb_train_steps``."""

    def __init__(self, pooled, labels, weights: Sequence, biases: Sequence, class_weights: Sequence, lr: float = 1e-3,
                 dropout: float = DROPOUT, weight_decay: float = WEIGHT_DECAY, seed: int = 42):
        torch = need_gpu(NO_GPU)
        self.pooled, dev = pooled, pooled.device
        self.labels = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
        self.W = torch.stack([torch.as_tensor(w, dtype=torch.float32) for w in weights]).to(dev).contiguous()
        self.b = torch.stack([torch.as_tensor(b, dtype=torch.float32) for b in biases]).to(dev).contiguous()
        self.cw = torch.as_tensor(np.ascontiguousarray(np.stack(class_weights), dtype=np.float32)).to(dev)
        self.R, self.C, self.D = self.W.shape
        if self.b.shape != (self.R, self.C) or self.cw.shape != (self.R, self.C) or self.D != pooled.shape[1]:
            raise ValueError("weights [C, D], biases [C] and class_weights [C] per run, D as the pooled features")
        self.mW, self.vW = torch.zeros_like(self.W), torch.zeros_like(self.W)
        self.mb, self.vb = torch.zeros_like(self.b), torch.zeros_like(self.b)
        self.errors = torch.zeros(self.R, dtype=torch.int32, device=dev)
        self.lr, self.dropout, self.weight_decay, self.seed = float(lr), float(dropout), float(weight_decay), int(seed)
        self.steps_done = [0] * self.R

    def run_spans(self, spans: Sequence[np.ndarray], batch_size: int) -> List[np.ndarray]:
        """One launch: run r walks ``spans[r]`` (int32, steps * batch_size entries, -1 padded; may be empty) from its
        global step ``steps_done[r]``. Returns the per-step losses of every run."""
        import torch

        n_steps = [len(s) // batch_size for s in spans]
        if len(spans) != self.R or any(len(s) != k * batch_size for s, k in zip(spans, n_steps)):
            raise ValueError("one span per run, a whole number of batches each")
        top = max(n_steps)
        if top == 0:
            return [np.zeros(0, dtype=np.float32) for _ in spans]
        order = np.full((self.R, top * batch_size), -1, dtype=np.int32)
        for r, s in enumerate(spans):
            order[r, :len(s)] = s
        dev = self.pooled.device
        order = torch.from_numpy(order).to(dev)
        counts = torch.tensor(n_steps, dtype=torch.int32, device=dev)
        first = torch.tensor(self.steps_done, dtype=torch.int32, device=dev)
        loss = torch.empty(self.R, top, dtype=torch.float32, device=dev)
        hip.call("stonk_kgb_train_steps", hip.ptr(self.pooled), self.pooled.stride(0), self.pooled.shape[0], self.D,
                 hip.ptr(self.labels), self.C, self.R, hip.ptr(order), order.stride(0), int(batch_size), hip.ptr(counts),
                 hip.ptr(first), top, hip.ptr(self.cw), hip.ptr(self.W), hip.ptr(self.b), hip.ptr(self.mW), hip.ptr(self.vW),
                 hip.ptr(self.mb), hip.ptr(self.vb), hip.ptr(loss), loss.stride(0), hip.ptr(self.errors), self.lr, BETAS[0],
                 BETAS[1], EPS, self.weight_decay, self.dropout, self.seed & _M32, hip.stream_ptr())
        self.steps_done = [d + k for d, k in zip(self.steps_done, n_steps)]
        host = loss.cpu().numpy()
        return [host[r, :k].copy() for r, k in enumerate(n_steps)]

    def train(self, train_indices: Sequence, epochs: int, batch_size: int, keep_losses: bool = False):
        """``epochs`` passes of every run over its own training indices, each epoch in the order ``epoch_order`` draws, cut
        into launches of at most ``max_steps()`` steps. Returns the per-step losses per run if asked to keep them."""
        cap = max_steps()
        losses = [[] for _ in range(self.R)]
        for epoch in range(epochs):
            cuts = [cut_epoch(epoch_order(idx, self.seed, r, epoch), batch_size, cap) for r, idx in enumerate(train_indices)]
            for j in range(max(len(c) for c in cuts)):
                out = self.run_spans([c[j] if j < len(c) else np.zeros(0, dtype=np.int32) for c in cuts], batch_size)
                if keep_losses:
                    for r in range(self.R):
                        losses[r].append(out[r])
        self.check_errors()
        return [np.concatenate(l) if l else np.zeros(0, np.float32) for l in losses] if keep_losses else None

    def check_errors(self):
        bad = np.flatnonzero(self.errors.cpu().numpy())
        if len(bad):
            raise hip.StonkHipError(f"stonk_kgb_train_steps: runs {bad.tolist()} met an example index outside the dataset "
                                    "or a label outside [0, C)")


# ---------------------------------------------------------------------------------------------------- datasets
class _WalkDataset:
    """What both datasets are: an int32 id matrix [n, L] (-1: the null vector), the fp32 table, integer labels."""

    def _finish(self, embedding_dict, labels):
        # (the reference adds the key -1 to the caller's dict (:155); this one leaves the caller's dict alone)
        self.embedding_dict = embedding_dict
        self.labels = labels
        self._pooled = self._table_dev = None

    @property
    def table_device(self):
        if self._table_dev is None:
            torch = need_gpu(NO_GPU)
            self._table_dev = torch.from_numpy(self.table).cuda()
        return self._table_dev

    @property
    def pooled(self):
        """fp32 [n, D] on the device: the dimension-wise maximum over each item's L table rows, one kernel pass."""
        if self._pooled is None:
            self._pooled = walk_maxpool(self.ids, self.table_device)
        return self._pooled

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, idx):
        """``(embedding sequence fp32 [L, D], label)`` as the reference returns it, gathered for this one item."""
        import torch

        rows = self.ids[idx]
        item = np.where((rows >= 0)[:, None], self.table[np.maximum(rows, 0)], np.float32(0))
        return torch.from_numpy(item), torch.tensor(int(np.asarray(self.labels)[idx]), dtype=torch.long)


class Node2VecINDRAEntityDataset(_WalkDataset):
    """ref:kg_baseline_model.py:143-205 without its [n, max_len, D] array."""

    def __init__(self, embedding_dict, random_walk_dict, sources, targets, labels, max_len: int = 254):
        self.max_length, self.sources, self.targets, self.random_walk_dict = max_len, sources, targets, random_walk_dict
        self.row_of, self.table = embedding_table(embedding_dict)
        self.ids = node2vec_id_matrix(self.row_of, random_walk_dict, sources, targets, max_len)
        self._finish(embedding_dict, labels)


class TransEINDRAEntityDataset(_WalkDataset):
    """ref:kg_baseline_model.py:208-267: the rows of (source, relation, target), L = 3."""

    def __init__(self, embedding_dict, sources, relations, targets, labels):
        self.sources, self.relations, self.targets = sources, relations, targets
        self.row_of, self.table = embedding_table(embedding_dict)
        self.ids = transe_id_matrix(self.row_of, sources, relations, targets)
        self._finish(embedding_dict, labels)


# ---------------------------------------------------------------------------------------------------- the model
class KGEClassificationModel:
    """ref:kg_baseline_model.py:43-140: max-pooling, dropout 0.1, ``linear`` (d_in x num_classes), softmax; trained by AdamW
    on a class-weighted cross-entropy OF THE PROBABILITIES. ``linear`` is a ``torch.nn.Linear`` made under the caller's
    seed; it holds the parameters between the kernel calls."""

    def __init__(self, num_classes: int, class_weights, d_in: int = 768, lr: float = 1e-3, dropout: float = DROPOUT):
        import torch

        self.linear = torch.nn.Linear(d_in, num_classes)
        self.class_weights = np.asarray(class_weights, dtype=np.float32)
        self.num_classes, self.d_in, self.lr, self.dropout = int(num_classes), int(d_in), float(lr), float(dropout)
        if self.class_weights.shape != (self.num_classes,):
            raise ValueError("one class weight per class")
        self.losses: Optional[np.ndarray] = None

    def state_dict(self):
        return {"linear.weight": self.linear.weight.detach().clone(), "linear.bias": self.linear.bias.detach().clone()}

    def load_state_dict(self, state):
        import torch

        with torch.no_grad():
            self.linear.weight.copy_(torch.as_tensor(state["linear.weight"]))
            self.linear.bias.copy_(torch.as_tensor(state["linear.bias"]))

    def forward(self, x):
        """``x`` fp32 [B, L, D] embedding sequences -> class probabilities [B, C] (eval mode: dropout acts in ``fit``
        only). The sequences are pooled by ``stonk_walk_maxpool`` as a table of B * L rows."""
        torch = need_gpu(NO_GPU)
        B, L, D = x.shape
        rows = x.to(device="cuda", dtype=torch.float32).reshape(B * L, D).contiguous()
        ids = torch.arange(B * L, dtype=torch.int32, device=rows.device).reshape(B, L)
        probs, _ = kgb_predict(walk_maxpool(ids, rows), np.arange(B), self.linear.weight.detach(), self.linear.bias.detach())
        return torch.from_numpy(probs)

    __call__ = forward

    def fit(self, dataset, train_idx, epochs: int = 100, batch_size: int = 8, seed: int = 42):
        trainer = KGBTrainer(dataset.pooled, dataset.labels, [self.linear.weight.detach()], [self.linear.bias.detach()],
                             [self.class_weights], self.lr, self.dropout, seed=seed)
        self.losses = trainer.train([train_idx], epochs, batch_size, keep_losses=True)[0]
        self.load_state_dict({"linear.weight": trainer.W[0].cpu(), "linear.bias": trainer.b[0].cpu()})
        return self

    def predict(self, dataset, idx) -> np.ndarray:
        """Predicted class per example of ``idx`` (the lowest index on a tie); ``predict_proba`` has the probabilities."""
        return kgb_predict(dataset.pooled, idx, self.linear.weight.detach(), self.linear.bias.detach())[1].astype(np.int64)

    def predict_proba(self, dataset, idx) -> np.ndarray:
        return kgb_predict(dataset.pooled, idx, self.linear.weight.detach(), self.linear.bias.detach())[0]


def init_fold_models(n_splits: int, num_classes: int, fold_class_weights, d_in: int, lr: float, dropout: float, seed: int):
    """The folds' models in fold order under ``torch.manual_seed(seed)`` (the caller's generator state is restored)."""
    import torch

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return [KGEClassificationModel(num_classes, fold_class_weights[r], d_in, lr, dropout) for r in range(n_splits)]


# ---------------------------------------------------------------------------------------------------- the driver
def run_kg_baseline_classification_cv(triples_path: str, embedding_path: str, random_walks_path: Optional[str] = None,
                                      n_splits: int = 5, epochs: int = 100, train_batch_size: int = 8,
                                      test_batch_size: int = 64, lr: float = 1e-3, label_column_name: str = "class",
                                      task_name: str = "", max_dataset_size: int = 100000, model_variant: str = "node2vec",
                                      output_dir: Optional[str] = None, seed: int = 42,
                                      dropout: float = DROPOUT) -> Dict[str, float]:
    """ref:kg_baseline_model.py:320-517. All folds train in one sequence of launches. ``test_batch_size`` is accepted for
    the reference's call shape; prediction is one launch. A QUIRK KEPT FROM THE REFERENCE: with more than
    ``max_dataset_size`` triples, ``get_train_test_splits`` returns positions in the stratified cut of the data, and the
    reference (:413-469) uses them, as this driver does, to index the UNCUT dataset and labels - the folds then cover the
    first ``max_dataset_size`` triples of the file, not the stratified sample. With ``output_dir`` the predicted-labels frame (``split``,
    ``index``, ``predicted_label``, ``true_label``, the labels by name) is written to
    ``predicted_labels_kg_<task_name>df.tsv`` there. Returns ``{"f1_score_mean", "f1_score_std"}``."""
    import pandas as pd

    if model_variant not in ("node2vec", "transe"):
        raise ValueError("model_variant: 'node2vec' or 'transe'")
    triples_df = pd.read_csv(triples_path, sep="\t", usecols=["source", "target", "relation", label_column_name])
    embeddings_dict = prepare_df(embedding_path)
    original_length = len(triples_df)
    triples_df, left_out = filter_triples(triples_df, embeddings_dict.keys())
    logger.info(f"{left_out} out of {original_length} triples are left out because they contain nodes which are not "
                f"present in the pre-training data")
    id2tag = sorted(triples_df[label_column_name].unique().tolist())
    tag2id = {tag: i for i, tag in enumerate(id2tag)}
    labels = np.array([tag2id[tag] for tag in triples_df[label_column_name]], dtype=np.int32)
    num_classes = len(id2tag)
    splits = get_train_test_splits(triples_df, type_column_name=label_column_name, random_seed=seed, n_splits=n_splits,
                                   max_dataset_size=max_dataset_size)
    if model_variant == "node2vec":
        if random_walks_path is None:
            raise ValueError("the node2vec variant needs random_walks_path")
        walks = prepare_df(random_walks_path)
        max_len = 2 * len(next(iter(walks.values())))
        dataset = Node2VecINDRAEntityDataset(embeddings_dict, walks, triples_df["source"], triples_df["target"], labels, max_len)
    else:
        dataset = TransEINDRAEntityDataset(embeddings_dict, triples_df["source"], triples_df["relation"],
                                           triples_df["target"], labels)
    fold_cw = [inverse_count_class_weights(labels, s["train_idx"], num_classes) for s in splits]
    models = init_fold_models(len(splits), num_classes, fold_cw, dataset.table.shape[1], lr, dropout, seed)
    trainer = KGBTrainer(dataset.pooled, labels, [m.linear.weight.detach() for m in models],
                         [m.linear.bias.detach() for m in models], fold_cw, lr, dropout, seed=seed)
    trainer.train([s["train_idx"] for s in splits], epochs, train_batch_size)

    f1_scores, frames = [], []
    for r, (model, split) in enumerate(zip(models, splits)):
        model.load_state_dict({"linear.weight": trainer.W[r].cpu(), "linear.bias": trainer.b[r].cpu()})
        predicted = model.predict(dataset, split["test_idx"])
        true = labels[split["test_idx"]]
        f1_scores.append(weighted_f1_score(true, predicted))
        frames.append(pd.DataFrame({"split": r, "index": split["test_idx"].tolist(),
                                    "predicted_label": [id2tag[i] for i in predicted],
                                    "true_label": [id2tag[i] for i in true]}))
    result_df = pd.concat(frames, ignore_index=True)
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        result_df.to_csv(os.path.join(output_dir, "predicted_labels_kg_" + task_name + "df.tsv"), index=False, sep="\t")
    logger.info(f"Mean f1-score: {np.mean(f1_scores)}")
    logger.info(f"Std f1-score: {np.std(f1_scores)}")
    return {"f1_score_mean": float(np.mean(f1_scores)), "f1_score_std": float(np.std(f1_scores))}


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="KG baseline (max-pooled walk embeddings + a linear classifier), cross-validated")
    ap.add_argument("--triples_path", required=True, help="TSV with source, target, relation and the label column")
    ap.add_argument("--embedding_path", required=True, help="embedding table TSV (node name, then the vector)")
    ap.add_argument("--random_walks_path", default=None, help="random walks TSV (node2vec variant)")
    ap.add_argument("--label_column_name", default="class")
    ap.add_argument("-e", "--epochs", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--max_dataset_size", type=int, default=100000)
    ap.add_argument("--model_variant", default="node2vec", choices=["node2vec", "transe"])
    ap.add_argument("--task_name", default="")
    ap.add_argument("--output_dir", default=None)
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    print(run_kg_baseline_classification_cv(
        args.triples_path, args.embedding_path, args.random_walks_path, epochs=args.epochs, train_batch_size=args.batch_size,
        lr=args.lr, label_column_name=args.label_column_name, task_name=args.task_name,
        max_dataset_size=args.max_dataset_size, model_variant=args.model_variant, output_dir=args.output_dir))


if __name__ == "__main__":
    main()
