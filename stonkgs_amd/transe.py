"""TransE on the GPU: triple list -> entity and relation embeddings -> the one TSV file the ``transe`` variant of the KG
baseline reads (``transe_embeddings_best_model.tsv``, ref:src/stonkgs/constants.py:70; read at
ref:src/stonkgs/models/kg_baseline_model.py:208-267 and ref:src/stonkgs/data/transe_indra_for_pretraining.py:43-44). The
reference does not produce that file - its authors trained it with PyKEEN outside the package; this module is the producer,
and the measure of its quality (raw and filtered rank metrics).

The model is Bordes et al. 2013: margin-ranking loss over corrupted triples, plain SGD, entity rows kept at unit L2 norm.
Host side only: names, launch plan, epoch orders and candidate lists on the CPU (numpy), device memory and streams through
torch, the three hot loops in csrc/transe.hip (``stonk_transe_step``, ``stonk_rows_l2_normalize``, ``stonk_transe_rank``).
There is no CPU fallback.

Command line: ``python -m stonkgs_amd.transe --pretraining_path triples.tsv --embeddings_output_path transe.tsv``
(``--test_fraction 0.1`` holds triples out and reports the filtered metrics on them).
"""
from __future__ import annotations

import logging
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _hip as hip
from .graph_common import cuts, decayed_lr, epoch_means, factorize_names, need_gpu, read_columns, to_device

logger = logging.getLogger(__name__)

LAUNCHES_PER_EPOCH = 64   # rows read inside a launch may be stale (TransE): an epoch is at least this many
METRICS = ("mrr", "mean_rank", "hits@1", "hits@3", "hits@10")


# ---------------------------------------------------------------------------------------------------- host preparation
def build_triples(sources, relations, targets) -> Tuple[list, list, np.ndarray]:
    """``(entity_names, relation_names, int32 [n, 3])`` of (head, relation, tail) ids; names numbered by first appearance
    (an entity: source before target of the same triple)."""
    src, rel, tgt = list(sources), list(relations), list(targets)
    if not len(src) == len(rel) == len(tgt):
        raise ValueError("sources, relations and targets differ in length")
    if not src:
        raise ValueError("empty triple list")
    e_codes, e_names = factorize_names(src, tgt)
    r_codes, r_names = factorize_names(rel)
    triples = np.stack([e_codes[:, 0], r_codes[:, 0], e_codes[:, 1]], axis=1).astype(np.int32)
    return e_names, r_names, np.ascontiguousarray(triples)


def _read_triples(triples_or_path, sep: str):
    """``(sources, relations, targets)`` of a TSV or DataFrame with ``source``, ``relation``, ``target`` columns, or of tuples."""
    return read_columns(triples_or_path, sep, ("source", "relation", "target"))


def known_index(triples) -> Dict[str, Dict[tuple, list]]:
    """``{"tails": {(h, r): [t, ...]}, "heads": {(r, t): [h, ...]}}`` of an int [n, 3] triple array, every list sorted and
    without duplicates: what the filtered setting must not count against a query."""
    tails: Dict[tuple, set] = {}
    heads: Dict[tuple, set] = {}
    for h, r, t in np.asarray(triples).reshape(-1, 3).tolist():
        tails.setdefault((h, r), set()).add(t)
        heads.setdefault((r, t), set()).add(h)
    return {"tails": {k: sorted(v) for k, v in tails.items()}, "heads": {k: sorted(v) for k, v in heads.items()}}


def candidate_lists(triples, side: int, known) -> Tuple[np.ndarray, np.ndarray]:
    """``(cand_ptr int64 [Q + 1], cand int32)``: per query the OTHER known-true entities of its side - the known tails of
    (h, r) without t for side 0, the known heads of (r, t) without h for side 1."""
    tri = np.asarray(triples).reshape(-1, 3)
    ptr = np.zeros(len(tri) + 1, dtype=np.int64)
    cand: List[int] = []
    for q, (h, r, t) in enumerate(tri.tolist()):
        others = known["tails"].get((h, r), ()) if side == 0 else known["heads"].get((r, t), ())
        true = t if side == 0 else h
        cand.extend(c for c in others if c != true)
        ptr[q + 1] = len(cand)
    return ptr, np.asarray(cand, dtype=np.int32)


def filtered_counts(less, equal, less_known, equal_known) -> Tuple[np.ndarray, np.ndarray]:
    """The filtered ``(less, equal)``: the raw counts minus the counts over the other known-true entities. A query the
    kernel refused (-1) stays -1."""
    less, equal = np.asarray(less), np.asarray(equal)
    bad = (less < 0) | (np.asarray(less_known) < 0)
    return np.where(bad, -1, less - less_known), np.where(bad, -1, equal - equal_known)


def realistic_rank(less, equal) -> np.ndarray:
    """``less + (equal + 1) / 2``: the mean rank of the true entity over all orders of its ties (``equal`` counts the true
    entity itself). NaN for a refused query."""
    less, equal = np.asarray(less, dtype=np.float64), np.asarray(equal, dtype=np.float64)
    return np.where(less < 0, np.nan, less + (equal + 1.0) / 2.0)


def rank_metrics(ranks) -> Dict[str, float]:
    """``{"mrr", "mean_rank", "hits@1", "hits@3", "hits@10"}`` of a vector of ranks (NaN entries are left out)."""
    r = np.asarray(ranks, dtype=np.float64)
    r = r[~np.isnan(r)]
    if not len(r):
        return {k: float("nan") for k in METRICS}
    return {"mrr": float((1.0 / r).mean()), "mean_rank": float(r.mean()), "hits@1": float((r <= 1).mean()),
            "hits@3": float((r <= 3).mean()), "hits@10": float((r <= 10).mean())}


def evaluation_report(ranks_tail, ranks_head) -> Dict[str, object]:
    """The metrics per side and over both (the ranks of the two sides pooled: the mean over the sides). The top-level
    figures are those of ``both``."""
    both = rank_metrics(np.concatenate([np.asarray(ranks_tail, dtype=np.float64), np.asarray(ranks_head, dtype=np.float64)]))
    return {**both, "tail": rank_metrics(ranks_tail), "head": rank_metrics(ranks_head), "both": both}


# ---------------------------------------------------------------------------------------------------- kernels
NO_GPU = "TransE needs an MI355X: the step, normalise and rank kernels have no CPU fallback"


def transe_rank(ent, rel, queries, side: int, norm: int, cand_ptr=None, cand=None) -> Tuple[np.ndarray, np.ndarray]:
    """``(less, equal)`` int32 [Q] by ``stonk_transe_rank``: the candidates closer than / as close as the true entity.
    ``ent`` / ``rel``: tables (numpy or device tensors); ``queries`` int [Q, 3]; candidates: every entity, or the lists
    ``cand[cand_ptr[q]:cand_ptr[q + 1]]``."""
    torch = need_gpu(NO_GPU)
    ent, rel = to_device(ent, torch.float32), to_device(rel, torch.float32)
    q = to_device(np.asarray(queries).reshape(-1, 3) if not torch.is_tensor(queries) else queries, torch.int32)
    n_q = q.shape[0]
    less = torch.empty(max(n_q, 1), dtype=torch.int32, device="cuda")
    equal = torch.empty(max(n_q, 1), dtype=torch.int32, device="cuda")
    ptr = to_device(cand_ptr, torch.int64) if cand_ptr is not None else None
    lst = to_device(cand, torch.int32) if cand_ptr is not None and len(cand) else None
    hip.call("stonk_transe_rank", hip.ptr(ent), hip.ptr(rel), ent.shape[0], rel.shape[0], ent.shape[1], norm, hip.ptr(q), n_q,
             side, hip.ptr(ptr), hip.ptr(lst), 0 if lst is None else lst.shape[0], hip.ptr(less), hip.ptr(equal),
             hip.stream_ptr())
    return less[:n_q].cpu().numpy(), equal[:n_q].cpu().numpy()


class TransE:
    """TransE (Bordes et al. 2013) trained by ``stonk_transe_step``: per triple ``negatives`` corrupted triples, the loss
    ``max(0, margin + ||h + r - t|| - ||h' + r - t'||)`` in the L1 or L2 norm, plain SGD with step ``lr`` (decaying
    linearly to ``min_lr`` over the run when that is given), the entity rows back on the unit sphere after every
    ``normalize_every``-th launch. An epoch is one pass over the triples in a seeded order, cut into at least
    ``launches_per_epoch`` launches."""

    def __init__(self, n_components: int = 768, epochs: int = 100, negatives: int = 1, margin: float = 1.0, norm: int = 1,
                 lr: float = 0.01, min_lr: Optional[float] = None, seed: int = 0,
                 launches_per_epoch: int = LAUNCHES_PER_EPOCH, normalize_every: int = 1):
        if n_components % 64 or not 64 <= n_components <= 1024:
            raise ValueError("n_components must be a multiple of 64, at most 1024")
        if epochs < 1 or negatives < 1 or launches_per_epoch < 1 or normalize_every < 1:
            raise ValueError("epochs, negatives, launches_per_epoch and normalize_every must be >= 1")
        if norm not in (1, 2):
            raise ValueError("norm must be 1 or 2")
        self.n_components, self.epochs, self.negatives = int(n_components), int(epochs), int(negatives)
        self.margin, self.norm, self.lr = float(margin), int(norm), float(lr)
        self.min_lr = None if min_lr is None else float(min_lr)
        self.seed, self.launches_per_epoch, self.normalize_every = int(seed), int(launches_per_epoch), int(normalize_every)
        self.entity_names: Optional[list] = None
        self.relation_names: Optional[list] = None
        self.triples: Optional[np.ndarray] = None
        self.entity_vectors: Optional[np.ndarray] = None
        self.relation_vectors: Optional[np.ndarray] = None
        self.loss_history: list = []
        self._entity_index: dict = {}
        self._relation_index: dict = {}
        self._ent = self._rel = None

    # ------------------------------------------------------------------ the schedule (CPU)
    def initial_vectors(self, n_entities: int, n_relations: int):
        """``(ent [N_e, D], rel [N_r, D])`` before training: uniform in +-6 / sqrt(D) from the seed, every row then at
        unit L2 norm (Bordes et al. 2013, algorithm 1). CPU tensors."""
        import torch

        g = torch.Generator().manual_seed(self.seed)
        bound = 6.0 / np.sqrt(self.n_components)
        out = []
        for n in (n_entities, n_relations):
            t = (torch.rand(n, self.n_components, generator=g) * 2.0 - 1.0) * bound
            out.append(t / t.norm(dim=1, keepdim=True).clamp_min(1e-12))
        return out[0], out[1]

    def launch_plan(self, n: int) -> List[Tuple[int, int, int]]:
        """``(epoch, g_lo, g_hi)`` per launch: every epoch's n groups cut into ``launches_per_epoch`` ranges (n ranges of
        one group where there are fewer groups than that)."""
        parts = min(n, self.launches_per_epoch)
        bounds = cuts(n, parts)
        return [(e, bounds[i], bounds[i + 1]) for e in range(self.epochs) for i in range(parts)]

    def launch_lr(self, i: int, n_launches: int) -> float:
        return decayed_lr(self.lr, self.min_lr, i, n_launches)

    def epoch_order(self, n: int, epoch: int) -> np.ndarray:
        """int32 [n]: the seeded permutation of the triples that epoch ``epoch`` walks (group g is triple order[g])."""
        return np.random.default_rng([self.seed & 0xFFFFFFFF, epoch]).permutation(n).astype(np.int32)

    def normalizes_after(self, i: int, n_launches: int) -> bool:
        return (i + 1) % self.normalize_every == 0 or i + 1 == n_launches

    # ------------------------------------------------------------------ device stages
    def train(self, triples, n_entities: int, n_relations: int):
        """All epochs over ``triples`` (int [n, 3]); returns ``(ent, rel)`` (fp32, device). ``loss_history``: the mean loss
        per term and epoch."""
        torch = need_gpu(NO_GPU)
        d = self.n_components
        tri = to_device(np.asarray(triples).reshape(-1, 3), torch.int32)
        n = tri.shape[0]
        ent0, rel0 = self.initial_vectors(n_entities, n_relations)
        ent, rel = ent0.cuda(), rel0.cuda()
        plan = self.launch_plan(n)
        loss = torch.zeros(len(plan), 2, device="cuda")
        stream = hip.stream_ptr()
        order, order_epoch = None, -1
        for i, (e, lo, hi) in enumerate(plan):
            if e != order_epoch:
                order, order_epoch = torch.from_numpy(self.epoch_order(n, e)).cuda(), e
            hip.call("stonk_transe_step", hip.ptr(ent), hip.ptr(rel), n_entities, n_relations, d, hip.ptr(tri), n,
                     hip.ptr(order), lo, hi, self.negatives, self.norm, self.margin, self.launch_lr(i, len(plan)),
                     self.seed & 0xFFFFFFFF, e, loss[i].data_ptr(), stream)
            if self.normalizes_after(i, len(plan)):
                hip.call("stonk_rows_l2_normalize", hip.ptr(ent), d, 0, n_entities, d, stream)
        self.loss_history = epoch_means(loss, [e for e, _, _ in plan], self.epochs)
        return ent, rel

    def fit(self, triples_or_path, sep: str = "\t"):
        """``triples_or_path``: a TSV with ``source``, ``relation`` and ``target`` columns, a DataFrame with them, or
        (source, relation, target) tuples."""
        need_gpu(NO_GPU)
        src, rel, tgt = _read_triples(triples_or_path, sep)
        names_e, names_r, triples = build_triples(src, rel, tgt)
        return self.fit_ids(names_e, names_r, triples)

    def fit_ids(self, entity_names, relation_names, triples):
        """``fit`` on triples that are ids already (``build_triples``' output, or a training share of it)."""
        need_gpu(NO_GPU)
        self.entity_names, self.relation_names = list(entity_names), list(relation_names)
        self.triples = np.ascontiguousarray(np.asarray(triples).reshape(-1, 3), dtype=np.int32)
        self._entity_index = {name: i for i, name in enumerate(self.entity_names)}
        self._relation_index = {name: i for i, name in enumerate(self.relation_names)}
        self._ent, self._rel = self.train(self.triples, len(self.entity_names), len(self.relation_names))
        self.entity_vectors, self.relation_vectors = self._ent.cpu().numpy(), self._rel.cpu().numpy()
        return self

    def predict(self, name) -> np.ndarray:
        """The vector of an entity - or, for a name that is no entity, of a relation."""
        if name in self._entity_index:
            return self.entity_vectors[self._entity_index[name]]
        return self.relation_vectors[self._relation_index[name]]

    # ------------------------------------------------------------------ evaluation
    def rank(self, triples, side: int, known=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(less, equal)`` per query: how many entities lie closer to ``h + r`` (side 0, ranking the tail) or ``t - r``
        (side 1, the head) than the true one, and how many as close (the true one included). With ``known`` - an int
        [m, 3] triple array or a ``known_index`` of one - the FILTERED counts: the other known-true entities of a query
        are not counted against it."""
        tri = np.asarray(triples).reshape(-1, 3)
        less, equal = transe_rank(self._ent, self._rel, tri, side, self.norm)
        if known is None:
            return less, equal
        index = known if isinstance(known, dict) else known_index(known)
        ptr, cand = candidate_lists(tri, side, index)
        less_k, equal_k = transe_rank(self._ent, self._rel, tri, side, self.norm, ptr, cand)
        return filtered_counts(less, equal, less_k, equal_k)

    def evaluate(self, test_triples, known_triples=None) -> Dict[str, object]:
        """``{"mrr", "mean_rank", "hits@1", "hits@3", "hits@10"}`` of the realistic rank ``less + (equal + 1) / 2`` over
        both sides, and the same per side under ``"tail"``, ``"head"`` (and ``"both"``). Filtered when ``known_triples``
        is given (pass training and test triples together)."""
        index = None if known_triples is None else \
            (known_triples if isinstance(known_triples, dict) else known_index(known_triples))
        ranks = [realistic_rank(*self.rank(test_triples, side, index)) for side in (0, 1)]
        return evaluation_report(ranks[0], ranks[1])

    # ------------------------------------------------------------------ the file
    def save_embeddings(self, path: str) -> None:
        """Entity lines, then relation lines: ``name\\t`` + D floats as ``repr`` writes them - what
        ``kg_baseline_model.prepare_df`` reads. An entity and a relation of one name could not be told apart in it."""
        clash = set(self.entity_names) & set(self.relation_names)
        if clash:
            raise ValueError(f"names that are both an entity and a relation: {sorted(map(str, clash))[:5]}")
        with open(path, "w") as f:
            for names, table in ((self.entity_names, self.entity_vectors), (self.relation_names, self.relation_vectors)):
                for name, row in zip(names, table):
                    f.write(f"{name}\t" + "\t".join(map(repr, row.tolist())) + "\n")


def split_triples(n: int, test_fraction: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(train positions, test positions)`` of n triples: a seeded share ``test_fraction`` is held out."""
    if not 0.0 <= test_fraction < 1.0:
        raise ValueError("test_fraction must lie in [0, 1)")
    perm = np.random.default_rng([seed & 0xFFFFFFFF, 0x7E57]).permutation(n)
    n_test = int(round(n * test_fraction))
    return np.sort(perm[n_test:]), np.sort(perm[:n_test])


def run_transe(pretraining_path, sep: str = "\t", *, embeddings_output_path: str, test_fraction: float = 0.0, **kwargs):
    """Train on the triples of ``pretraining_path`` and write the table. With ``test_fraction`` > 0 a seeded share of the
    triples is held out of training (every name keeps its row) and the filtered metrics on it are logged. Returns
    ``(model, metrics)``; ``metrics`` is None without a held-out share. Further keywords go to ``TransE``."""
    model = TransE(**kwargs)
    src, rel, tgt = _read_triples(pretraining_path, sep)
    names_e, names_r, triples = build_triples(src, rel, tgt)
    metrics = None
    if test_fraction > 0:
        train_pos, test_pos = split_triples(len(triples), test_fraction, model.seed)
        model.fit_ids(names_e, names_r, triples[train_pos])
        if len(test_pos):
            metrics = model.evaluate(triples[test_pos], known_triples=triples)
            logger.info("TransE held-out filtered metrics over %d triples: %s", len(test_pos),
                        {k: metrics[k] for k in METRICS})
    else:
        model.fit_ids(names_e, names_r, triples)
    model.save_embeddings(embeddings_output_path)
    return model, metrics


def main(argv=None) -> None:
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pretraining_path", required=True)
    ap.add_argument("--embeddings_output_path", required=True)
    ap.add_argument("--sep", default="\t")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--negatives", type=int, default=1)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--norm", type=int, default=1, choices=(1, 2))
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--test_fraction", type=float, default=0.0)
    a = ap.parse_args(argv)
    m, metrics = run_transe(a.pretraining_path, a.sep, embeddings_output_path=a.embeddings_output_path,
                            test_fraction=a.test_fraction, seed=a.seed, epochs=a.epochs, negatives=a.negatives,
                            margin=a.margin, norm=a.norm, lr=a.lr)
    print(f"{len(m.entity_names)} entities, {len(m.relation_names)} relations, mean loss first / last epoch "
          f"{m.loss_history[0]:.4f} / {m.loss_history[-1]:.4f}")
    if metrics is not None:
        print("held-out, filtered: " + ", ".join(f"{k} {metrics[k]:.4f}" for k in METRICS))


if __name__ == "__main__":
    main()
