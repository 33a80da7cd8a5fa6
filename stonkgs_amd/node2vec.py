"""node2vec on the GPU: edge list -> random walks + skip-gram embeddings -> the two TSV files the loaders read
(``embeddings_best_model.tsv`` for ``STonKGsForPreTraining(kg_embedding_dict_path=...)``, ``random_walks_best_model.tsv``
for ``preprocess_df_for_embeddings*``). Replaces ref:src/stonkgs/models/node2vec.py::run_node2vec, which drives
``nodevectors`` and ``gensim`` on CPU threads; the keyword surface is theirs.

Host side only: graph and noise-table construction on the CPU (numpy), device memory and streams through torch, the two
hot loops in csrc/node2vec.hip (``stonk_random_walks``, ``stonk_sgns_step``). There is no CPU fallback.
``run_node2vec_hpo`` (ref:node2vec.py:93-257) picks the best of several runs by the link-prediction score of
stonkgs_amd/link_prediction.py.

Command line: ``python -m stonkgs_amd.node2vec --pretraining_path edges.tsv --embeddings_output_path emb.tsv
--random_walks_output_path walks.tsv`` (one run); with ``--n_trials N`` the search.
"""
from __future__ import annotations

import itertools
from typing import List, Optional, Tuple

import numpy as np

from . import _hip as hip
from .graph_common import csr_to_device, cuts, decayed_lr, epoch_means, factorize_names, need_gpu, read_columns

LAUNCHES_PER_EPOCH = 64   # rows read inside a launch may be stale (node2vec): an epoch is at least this many


def build_csr(sources, targets) -> Tuple[list, np.ndarray, np.ndarray]:
    """Undirected CSR graph of an edge list. ``sources`` / ``targets``: equally long sequences of node names (any hashable)
    or ints. Returns ``(names, rowptr int64 [N+1], col int32 [nnz])``: node i is ``names[i]``, numbered by first appearance
    in the edge list (source before target); both directions of every edge are present, duplicates merged, every
    adjacency list sorted ascending."""
    src, tgt = list(sources), list(targets)
    if len(src) != len(tgt):
        raise ValueError("sources and targets differ in length")
    codes, uniques = factorize_names(src, tgt)
    n = len(uniques)
    if n == 0:
        raise ValueError("empty edge list")
    s, t = codes[:, 0].astype(np.int64), codes[:, 1].astype(np.int64)
    key = np.unique(np.concatenate([s * n + t, t * n + s]))     # sorted by (row, column), duplicates gone
    rows, col = key // n, (key % n).astype(np.int32)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return uniques, rowptr, col


def alias_table(counts, power: float = 0.75) -> Tuple[np.ndarray, np.ndarray]:
    """Walker / Vose alias table of the noise distribution ``counts ** power / sum`` with integer thresholds:
    ``(alias_thr uint32 [N], alias_idx int32 [N])``. A uniform slot s and a uniform 32-bit draw r give node
    ``s if r < alias_thr[s] else alias_idx[s]``. A slot that always keeps itself has ``alias_idx[s] == s`` (2^32 is not a
    uint32). A node with count 0 is never drawn: its slot has threshold 0 and no slot names it as alias."""
    c = np.asarray(counts, dtype=np.float64)
    if c.ndim != 1 or c.size == 0 or (c < 0).any() or not (c > 0).any():
        raise ValueError("counts: a non-empty vector of non-negative numbers, not all zero")
    n = c.size
    w = np.where(c > 0, c, 0.0) ** power
    w[c == 0] = 0.0
    p = w / w.sum() * n                            # mean 1
    thr = np.zeros(n, dtype=np.uint32)
    idx = np.arange(n, dtype=np.int32)
    order = np.argsort(p, kind="stable")
    small = [int(i) for i in order[::-1] if p[i] < 1.0]   # popped from the end: the smallest (the zeros) first
    large = [int(i) for i in order if p[i] >= 1.0]
    p = p.copy()
    while small and large:
        s, l = small.pop(), large[-1]
        thr[s] = min(int(p[s] * 4294967296.0), 4294967295)
        idx[s] = l
        p[l] -= 1.0 - p[s]
        if p[l] < 1.0:
            large.pop()
            small.append(l)
    for i in small + large:                        # what is left is 1 up to rounding: the slot keeps itself
        thr[i], idx[i] = 4294967295, i
    return thr, idx


def walk_thresholds(return_weight: float, neighbor_weight: float, other_weight: float = 1.0) -> Tuple[int, int, int]:
    """24-bit acceptance thresholds ``floor(weight / max_weight * 2^24)`` of the three candidate classes."""
    ws = (float(return_weight), float(neighbor_weight), float(other_weight))
    if min(ws) < 0 or max(ws) <= 0:
        raise ValueError("walk weights must be non-negative and not all zero")
    return tuple(int(np.floor(w / max(ws) * (1 << 24))) for w in ws)


class Node2Vec:
    """``nodevectors.Node2Vec`` as ref:node2vec.py:314-334 uses it: ``epochs`` walks of ``walklen`` nodes start at every
    node, one skip-gram pass (``window``, ``negative`` noise words, learning rate ``alpha`` -> ``min_alpha``) runs over them.
    ``return_weight`` / ``neighbor_weight`` weigh a step back to the previous node / to a common neighbour of the previous
    node; every other step has weight 1. ``p`` / ``q`` are the paper's spelling: weights ``(1/p, 1, 1/q)``."""

    def __init__(self, n_components: int = 768, walklen: int = 127, epochs: int = 4, return_weight: float = 1.0,
                 neighbor_weight: float = 1.0, window: int = 3, negative: int = 5, alpha: float = 0.025,
                 min_alpha: float = 1e-4, seed: int = 0, keep_walks: bool = True, p: Optional[float] = None,
                 q: Optional[float] = None, threads=None, verbose: bool = False, w2vparams: Optional[dict] = None):
        if n_components % 64 or not 64 <= n_components <= 1024:
            raise ValueError("n_components must be a multiple of 64, at most 1024")
        if walklen < 1 or epochs < 1:
            raise ValueError("walklen and epochs must be >= 1")
        w2v = dict(w2vparams or {})
        window, negative = int(w2v.pop("window", window)), int(w2v.pop("negative", negative))
        alpha, min_alpha = float(w2v.pop("alpha", alpha)), float(w2v.pop("min_alpha", min_alpha))
        self.n_components, self.walklen, self.epochs = int(n_components), int(walklen), int(epochs)
        self.window, self.negative, self.alpha, self.min_alpha = window, negative, alpha, min_alpha
        self.seed, self.keep_walks = int(seed), bool(keep_walks)
        if p is not None or q is not None:
            self.weights = (1.0 / (p if p is not None else 1.0), 1.0, 1.0 / (q if q is not None else 1.0))
        else:
            self.weights = (float(return_weight), float(neighbor_weight), 1.0)
        self.thresholds = walk_thresholds(*self.weights)
        self.names: Optional[list] = None
        self.rowptr: Optional[np.ndarray] = None   # the graph of the last fit (link_prediction.py scores the table on it)
        self.col: Optional[np.ndarray] = None
        self.walks = None
        self.counts: Optional[np.ndarray] = None
        self.loss_history: list = []
        self._index: dict = {}
        self._w_in = None

    # ------------------------------------------------------------------ device stages
    def random_walks(self, rowptr: np.ndarray, col: np.ndarray, device=None):
        """int32 [epochs * N, walklen] on the device: row e * N + n is the walk of epoch e that starts at node n."""
        import torch

        dev, rp, cl = csr_to_device(rowptr, col, device)
        n = len(rowptr) - 1
        total = self.epochs * n
        walks = torch.empty(total, self.walklen, dtype=torch.int32, device=dev)
        hip.call("stonk_random_walks", hip.ptr(rp), hip.ptr(cl), n, 0, 0, total, self.walklen, *self.thresholds,
                 self.seed & 0xFFFFFFFF, hip.ptr(walks), self.walklen, hip.stream_ptr())
        return walks

    def launch_plan(self, n: int):
        """The slices of one pass over the corpus, each one launch: every epoch (N walks) is cut into at least
        LAUNCHES_PER_EPOCH ranges of walks - and of positions where there are fewer walks than that."""
        n_w = min(n, LAUNCHES_PER_EPOCH)
        n_p = min(self.walklen, -(-LAUNCHES_PER_EPOCH // n_w))
        wcuts, pcuts = cuts(n, n_w), cuts(self.walklen, n_p)
        return [(e, e * n + wcuts[i], e * n + wcuts[i + 1], pcuts[j], pcuts[j + 1])
                for e in range(self.epochs) for i in range(n_w) for j in range(n_p)]

    def initial_vectors(self, n: int):
        """W_in before training: uniform in +-0.5 / D from the seed (word2vec's init; W_out starts at zero). CPU tensor."""
        import torch

        g = torch.Generator().manual_seed(self.seed)
        return (torch.rand(n, self.n_components, generator=g) - 0.5) / self.n_components

    def train(self, walks, n: int):
        """One skip-gram pass over ``walks``; returns W_in (fp32 [N, D], device). ``loss_history``: mean loss per epoch."""
        import torch

        dev, d = walks.device, self.n_components
        counts = torch.bincount(walks.flatten().clamp_min(0).long(), minlength=n).cpu().numpy()
        self.counts = counts
        thr, idx = alias_table(counts)
        a_thr = torch.from_numpy(thr.view(np.int32)).to(dev)
        a_idx = torch.from_numpy(idx).to(dev)
        w_in = self.initial_vectors(n).to(dev)
        w_out = torch.zeros(n, d, device=dev)
        plan = self.launch_plan(n)
        loss = torch.zeros(len(plan), 2, device=dev)
        stream = hip.stream_ptr()
        for i, (_, w_lo, w_hi, p_lo, p_hi) in enumerate(plan):
            lr = decayed_lr(self.alpha, self.min_alpha, i, len(plan))
            hip.call("stonk_sgns_step", hip.ptr(walks), walks.shape[1], walks.shape[1], w_lo, w_hi, p_lo, p_hi,
                     hip.ptr(w_in), hip.ptr(w_out), n, d, self.window, self.negative, hip.ptr(a_thr), hip.ptr(a_idx), lr,
                     self.seed & 0xFFFFFFFF, loss[i].data_ptr(), stream)
        self.loss_history = epoch_means(loss, [e for e, *_ in plan], self.epochs)
        self._w_out = w_out
        return w_in

    # ------------------------------------------------------------------ the nodevectors surface
    def fit(self, edges_or_path, sep: str = "\t"):
        """``edges_or_path``: a TSV with ``source`` and ``target`` columns, a DataFrame with them, or (source, target) pairs."""
        need_gpu("Node2Vec.fit needs an MI355X: the walk and skip-gram kernels have no CPU fallback")
        src, tgt = read_columns(edges_or_path, sep, ("source", "target"))
        self.names, rowptr, col = build_csr(src, tgt)
        self.rowptr, self.col = rowptr, col
        self._index = {name: i for i, name in enumerate(self.names)}
        n = len(self.names)
        walks = self.random_walks(rowptr, col)
        self._w_in = self.train(walks, n)
        self.vectors = self._w_in.cpu().numpy()
        self._own_walks = walks[:n].cpu().numpy()          # epoch 0: row n starts at node n
        self.walks = walks if self.keep_walks else None
        return self

    def predict(self, name) -> np.ndarray:
        return self.vectors[self._index[name]]

    def frequency_order(self) -> np.ndarray:
        """Nodes by corpus frequency, descending; ties by first appearance in the edge list (gensim's vocabulary sort)."""
        return np.argsort(-self.counts, kind="stable")

    def save_embeddings(self, path: str) -> None:
        """One line per node, ``name\\t`` + D floats as ``repr`` writes them, in frequency_order()."""
        with open(path, "w") as f:
            for i in self.frequency_order():
                f.write(f"{self.names[i]}\t" + "\t".join(map(repr, self.vectors[i].tolist())) + "\n")

    def save_walks(self, path: str) -> None:
        """One line per node in the same order: ``name\\t`` + the node's OWN epoch-0 walk, ``walklen`` names of which the
        first is the node itself (the reference's line format: prepare_df reads the name as key, the walk as value)."""
        with open(path, "w") as f:
            for i in self.frequency_order():
                f.write(f"{self.names[i]}\t" + "\t".join(str(self.names[j]) for j in self._own_walks[i].tolist()) + "\n")


def run_node2vec(pretraining_path: str, sep: str = "\t", n_threads: Optional[int] = None, *,
                 embeddings_output_path: str, random_walks_output_path: str, **node2vec_kwargs) -> Node2Vec:
    """ref:node2vec.py:270-370 with its hyper-parameters (walk length 127, 4 walks per node, 768 dimensions, window 3,
    5 negatives, one pass). ``n_threads`` is accepted and ignored; both output paths are required (the reference's defaults
    are directories of its own package). Further keywords go to Node2Vec."""
    model = Node2Vec(**node2vec_kwargs).fit(pretraining_path, sep=sep)
    model.save_embeddings(embeddings_output_path)
    model.save_walks(random_walks_output_path)
    return model


HPO_SEARCH_SPACE = {"epochs": [2, 4, 8], "window": [3, 4, 5]}   # ref:node2vec.py:156-158 (window_size: suggest_int(3, 5))


def hpo_trials(search_space: dict, n_trials: int, seed: int) -> List[dict]:
    """The trials of a search: ``min(n_trials, grid size)`` points of the grid ``search_space`` spans (keys in their given
    order, the last one varying fastest), drawn without replacement by ``np.random.RandomState(seed)``."""
    keys = list(search_space)
    grid = list(itertools.product(*(list(search_space[k]) for k in keys)))
    if not grid or n_trials < 1:
        raise ValueError("an empty search")
    picks = np.random.RandomState(seed & 0xFFFFFFFF).choice(len(grid), min(int(n_trials), len(grid)), replace=False)
    return [dict(zip(keys, grid[i])) for i in picks]


def search_trials(trials: List[dict], run_trial, score_key: str = "auc_hard_labels"):
    """The search loop: ``run_trial(params)`` returns ``(model, report)``; the model whose ``report[score_key]`` is largest
    is kept (the others are dropped as the loop goes on), ties go to the EARLIER trial. Returns ``(best model,
    [(params, report), ...])``. Warns when no trial stands out - all scores equal, or a classifier that never left its
    starting point (``n_iter`` 0: the table's features are too small for the fit's tolerance, typical of a barely
    trained table) - because the first trial is then returned without having been selected by anything."""
    import warnings

    best, best_score, results = None, -np.inf, []
    for params in trials:
        model, report = run_trial(params)
        results.append((params, report))
        if report[score_key] > best_score:
            best, best_score = model, report[score_key]
    scores = [r[score_key] for _, r in results]
    if len(results) > 1 and max(scores) == min(scores):
        warnings.warn(f"all {len(results)} trials score {scores[0]:.4f}: the first trial is returned, nothing was selected")
    elif any(r.get("n_iter") == 0 for _, r in results):
        warnings.warn("a trial's classifier stopped at its starting point (features too small for its tolerance): its score "
                      "of 0.5 says nothing about the table")
    return best, results


def run_node2vec_hpo(pretraining_path: str, sep: str = "\t", delete_database: bool = True, logging_uri: Optional[str] = None,
                     n_trials: int = 1, n_threads: Optional[int] = None, seed: Optional[int] = None, *,
                     embeddings_output_path: str, random_walks_output_path: str, search_space: Optional[dict] = None,
                     **fixed):
    """ref:node2vec.py:93-257: several node2vec runs over ``epochs`` in {2, 4, 8} and ``window`` in {3, 4, 5}, everything
    else as in ``run_node2vec`` (or ``fixed``), each scored by ``link_prediction_report``; the best one's two TSV files
    are written. There is no optuna here: the trials are ``hpo_trials(search_space, n_trials, seed)``, grid points without
    replacement. The positive and negative pairs are drawn ONCE and shared by all trials, so the scores are comparable
    (the reference redraws them per trial). The score is the reference's figure, ``auc_hard_labels``; ties go to the
    earlier trial. ``delete_database``, ``logging_uri`` and ``n_threads`` are accepted and ignored (no study database, no
    mlflow, no CPU threads). Returns ``(best model, [(params, report), ...])``."""
    from .link_prediction import link_prediction_examples, link_prediction_report

    if seed is None:
        seed = int(np.random.randint(1, 2 ** 31 - 1))
    trials = hpo_trials(search_space or HPO_SEARCH_SPACE, n_trials, seed)
    src, tgt = read_columns(pretraining_path, sep, ("source", "target"))
    edges = list(zip(src, tgt))
    _, rowptr, col = build_csr(src, tgt)
    examples = link_prediction_examples(rowptr, col, seed=seed)

    def run_trial(params):
        model = Node2Vec(**{"seed": seed & 0xFFFFFFFF, **fixed, **params}).fit(edges)
        return model, link_prediction_report(model, seed=seed, examples=examples)

    best, results = search_trials(trials, run_trial)
    best.save_embeddings(embeddings_output_path)
    best.save_walks(random_walks_output_path)
    return best, results


def main(argv=None) -> None:
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pretraining_path", required=True)
    ap.add_argument("--sep", default="\t")
    ap.add_argument("--n_threads", type=int, default=None)
    ap.add_argument("--embeddings_output_path", required=True)
    ap.add_argument("--random_walks_output_path", required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n_trials", type=int, default=None, help="run the hyper-parameter search with this many trials")
    a = ap.parse_args(argv)
    if a.n_trials is not None:
        m, results = run_node2vec_hpo(a.pretraining_path, a.sep, n_trials=a.n_trials, n_threads=a.n_threads, seed=a.seed,
                                      embeddings_output_path=a.embeddings_output_path,
                                      random_walks_output_path=a.random_walks_output_path)
        for params, report in results:
            print(f"{params}: score {report['auc_hard_labels']:.4f}  auc {report['auc']:.4f}")
        print(f"best: epochs {m.epochs}, window {m.window}; {len(m.names)} nodes")
        return
    m = run_node2vec(a.pretraining_path, a.sep, a.n_threads, embeddings_output_path=a.embeddings_output_path,
                     random_walks_output_path=a.random_walks_output_path, seed=a.seed)
    print(f"{len(m.names)} nodes, mean loss per epoch {m.loss_history}")


if __name__ == "__main__":
    main()
