"""Link-prediction score of a node2vec table: how good an entity table is, and the figure ``run_node2vec_hpo`` maximises.
Replaces ref:src/stonkgs/models/node2vec.py::run_link_prediction (:34-71), which takes half of the graph's edges and as many
random non-edges from stellargraph's ``EdgeSplitter``, builds the [n, D] matrix of Hadamard products of the two node vectors,
fits a default ``sklearn.linear_model.LogisticRegression`` on 75 % of it and scores the other 25 %.

Here the negatives are drawn on the GPU (``stonk_sample_non_edges``) and the feature matrix never exists: one evaluation of
the logistic loss and its gradient is one launch of ``stonk_linkpred_lossgrad`` (csrc/link_prediction.hip), which gathers the
two table rows of every example. The optimiser (L-BFGS, numpy fp64) runs on the host over D + 1 numbers; the table, the pairs
and the labels stay on the device. There is no CPU fallback for the two kernels.

THE SCORE IS THE REFERENCE'S HEURISTIC, NOT A HELD-OUT LINK PREDICTOR: like the reference, the embeddings that are scored
were trained on the FULL graph (EdgeSplitter's reduced graph is thrown away there, ``_`` in :50), so the positive examples
are edges the walks have seen. It ranks tables of one graph against each other; it does not estimate how well unseen edges
would be predicted.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np

from . import _hip as hip
from .graph_common import as_tensor, csr_to_device, need_gpu, to_device


# ---------------------------------------------------------------------------------------------------- examples
def sample_positive_edges(rowptr, col, p: float = 0.5, seed: int = 0) -> np.ndarray:
    """int32 [P, 2], P = floor(p * number of undirected edges): distinct edges (u, v), u < v, drawn uniformly without
    replacement (numpy, host) from the CSR graph ``build_csr`` makes. stellargraph's ``EdgeSplitter(g).train_test_split()``
    at its defaults: p = 0.5, method "global", keep_connected=False. Self-loops are no candidates."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    upper = rows < col                                # every undirected edge once
    u, v = rows[upper], col[upper]
    if not 0.0 < p <= 1.0:
        raise ValueError("p must be in (0, 1]")
    take = np.random.RandomState(seed & 0xFFFFFFFF).choice(len(u), int(np.floor(p * len(u))), replace=False)
    return np.stack([u[take], v[take]], axis=1).astype(np.int32)


def sample_non_edges(rowptr, col, count: int, seed: int, device=None):
    """int32 [count, 2] on the device: ordered pairs (u, v), u != v, not adjacent, uniform over such pairs, drawn by
    ``stonk_sample_non_edges`` (a pure function of (seed, row)). Negatives are drawn WITH replacement: two rows may be equal.
    Raises if a sample found no non-edge in its 64 attempts (a graph that is almost complete), naming how many did."""
    import torch

    dev, rp, cl = csr_to_device(rowptr, col, device)
    out = torch.empty(int(count), 2, dtype=torch.int32, device=dev)
    failures = torch.zeros(1, dtype=torch.int32, device=dev)
    hip.call("stonk_sample_non_edges", hip.ptr(rp), hip.ptr(cl), len(rowptr) - 1, 0, int(count), seed & 0xFFFFFFFF,
             hip.ptr(out), hip.ptr(failures), hip.stream_ptr())
    failed = int(failures.item())
    if failed:
        raise hip.StonkHipError(f"sample_non_edges: {failed} of {count} samples found no non-edge in 64 attempts "
                                "(the graph is too dense for rejection sampling)")
    return out


def link_prediction_examples(rowptr, col, p: float = 0.5, seed: int = 0, device=None) -> Tuple[np.ndarray, np.ndarray]:
    """``(pairs int32 [2 P, 2], labels float32 [2 P])`` on the host: P positive edges, then as many sampled non-edges."""
    pos = sample_positive_edges(rowptr, col, p, seed)
    if not len(pos):
        raise ValueError("the graph has too few edges for a link-prediction score")
    neg = sample_non_edges(rowptr, col, len(pos), seed, device).cpu().numpy()
    return np.concatenate([pos, neg]), np.r_[np.ones(len(pos), np.float32), np.zeros(len(neg), np.float32)]


def stratified_split(y, test_size: float = 0.25, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """``(train_idx, test_idx)``: every class's examples are permuted and round(test_size * class size) of them go to the
    test block (``train_test_split(..., stratify=y)``). The caller lays the examples out as ``[train_idx, test_idx]`` - two
    contiguous blocks, so that the kernel takes pointer offsets and no index indirection."""
    y = np.asarray(y)
    rng = np.random.RandomState(seed & 0xFFFFFFFF)
    train, test = [], []
    for c in np.unique(y):
        idx = rng.permutation(np.flatnonzero(y == c))
        k = int(round(test_size * len(idx)))
        test.append(idx[:k])
        train.append(idx[k:])
    train, test = np.concatenate(train), np.concatenate(test)
    return rng.permutation(train), rng.permutation(test)


# ---------------------------------------------------------------------------------------------------- optimiser
def lbfgs_minimize(fun: Callable, x0, m: int = 10, max_iter: int = 100, gtol: float = 1e-4):
    """Limited-memory BFGS in numpy fp64: two-loop recursion over the last ``m`` curvature pairs, backtracking Armijo line
    search (sufficient decrease 1e-4, halving), a pair (s, y) is kept only if <s, y> > 1e-10 |s| |y|. ``fun(x)`` returns
    ``(value, gradient)``. Stops at max |gradient| <= gtol. Returns ``(x, value, n_iter, converged, n_eval)``; a line search
    that finds no decrease in 30 halvings (the noise floor of ``fun``) ends the run unconverged."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    g = np.asarray(g, dtype=np.float64)
    n_eval, n_iter = 1, 0
    s_hist, y_hist = [], []
    while n_iter < max_iter:
        if np.abs(g).max() <= gtol:
            return x, float(f), n_iter, True, n_eval
        q = g.copy()
        alphas = []
        for s, yv in zip(reversed(s_hist), reversed(y_hist)):
            a = s.dot(q) / yv.dot(s)
            alphas.append(a)
            q -= a * yv
        if s_hist:
            q *= s_hist[-1].dot(y_hist[-1]) / y_hist[-1].dot(y_hist[-1])
        for (s, yv), a in zip(zip(s_hist, y_hist), reversed(alphas)):
            q += (a - yv.dot(q) / yv.dot(s)) * s
        d = -q
        slope = g.dot(d)
        if not slope < 0:                               # not a descent direction: forget the history
            s_hist, y_hist, d = [], [], -g
            slope = g.dot(d)
        t = 1.0 if s_hist else 1.0 / max(1.0, np.linalg.norm(g))
        for _ in range(30):
            f_new, g_new = fun(x + t * d)
            n_eval += 1
            if np.isfinite(f_new) and f_new <= f + 1e-4 * t * slope:
                break
            t *= 0.5
        else:
            return x, float(f), n_iter, False, n_eval
        g_new = np.asarray(g_new, dtype=np.float64)
        s, yv = t * d, g_new - g
        if s.dot(yv) > 1e-10 * np.linalg.norm(s) * np.linalg.norm(yv):
            s_hist.append(s)
            y_hist.append(yv)
            if len(s_hist) > m:
                s_hist.pop(0)
                y_hist.pop(0)
        x, f, g = x + s, f_new, g_new
        n_iter += 1
    return x, float(f), n_iter, bool(np.abs(g).max() <= gtol), n_eval


def logistic_objective(evaluate: Callable, n: int, C: float = 1.0) -> Callable:
    """The objective of scikit-learn's LogisticRegression in its current scaling, over theta = [w (D), b]:
    mean log-loss + |w|^2 / (2 C n), the intercept unpenalised. ``evaluate(w, b)`` returns the SUMS over the n examples
    ``(sum g x [D], sum g, sum loss)`` - from the kernel, or from a restatement of it."""
    def fun(theta):
        w, b = theta[:-1], float(theta[-1])
        gx, gsum, loss = evaluate(w, b)
        value = (float(loss) + 0.5 * w.dot(w) / C) / n
        grad = np.empty_like(theta)
        grad[:-1] = (np.asarray(gx, dtype=np.float64) + w / C) / n
        grad[-1] = float(gsum) / n
        return value, grad
    return fun


def roc_auc(scores, labels) -> float:
    """Area under the ROC curve by rank, tied scores at their average rank (``sklearn.metrics.roc_auc_score``). On 0 / 1
    scores - what the reference passes - this is the balanced accuracy."""
    scores, pos = np.asarray(scores, dtype=np.float64), np.asarray(labels) > 0
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if not n_pos or not n_neg:
        raise ValueError("roc_auc needs both classes")
    _, inverse, counts = np.unique(scores, return_inverse=True, return_counts=True)
    last = np.cumsum(counts)                            # rank of the last member of every group of equal scores
    rank = (last - (counts - 1) / 2.0)[inverse]
    return float((rank[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * float(n_neg)))


# ---------------------------------------------------------------------------------------------------- the classifier
def _device_examples(emb, pairs, y=None):
    torch = need_gpu("the link-prediction kernels need an MI355X: there is no CPU fallback")
    emb = as_tensor(emb, torch.float32)
    if not emb.is_cuda:
        emb = emb.cuda()
    if emb.dtype != torch.float32 or emb.dim() != 2 or emb.stride(1) != 1:
        raise ValueError("emb: an fp32 [N, D] table with contiguous rows")
    pairs = to_device(pairs, torch.int32, emb.device)
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs: int32 [n, 2]")
    if y is not None:
        y = to_device(y, torch.float32, emb.device)
        if y.shape != (pairs.shape[0],):
            raise ValueError("y: one label per pair")
    return emb, pairs, y


def linkpred_lossgrad(emb, pairs, y, w, b: float, scores=None, partials=None) -> None:
    """One launch of ``stonk_linkpred_lossgrad`` on device tensors (``scores`` / ``partials``: None skips the output)."""
    hip.call("stonk_linkpred_lossgrad", hip.ptr(emb), emb.stride(0), emb.shape[0], emb.shape[1], hip.ptr(pairs), hip.ptr(y),
             pairs.shape[0], hip.ptr(w), float(b), hip.ptr(scores), hip.ptr(partials), hip.stream_ptr())


class HadamardLogisticRegression:
    """``sklearn.linear_model.LogisticRegression`` (L2, lbfgs, fit_intercept) on the features ``emb[u] * emb[v]`` of a pair
    (u, v), without the feature matrix: minimises mean log-loss + |w|^2 / (2 C n) from zeros by ``lbfgs_minimize`` and
    stops at max |gradient| <= tol. ``tol`` is a tolerance on fp32 evaluations: the kernel's gradient carries the rounding
    of its format, and a much smaller tol is below that noise and is never reached. Every evaluation is one kernel launch
    and brings D + 2 numbers to the host. Labels are 0 / 1."""

    def __init__(self, C: float = 1.0, tol: float = 1e-4, max_iter: int = 100):
        self.C, self.tol, self.max_iter = float(C), float(tol), int(max_iter)
        self.coef_ = self.intercept_ = None
        self.n_iter_, self.converged_, self.n_eval_ = 0, False, 0

    def fit(self, emb, pairs, y):
        import torch

        emb, pairs, y = _device_examples(emb, pairs, y)
        n, d = pairs.shape[0], emb.shape[1]
        if n == 0:
            raise ValueError("no examples")
        partials = torch.empty(int(hip.lib().stonk_linkpred_partial_rows()), d + 2, dtype=torch.float32, device=emb.device)

        def evaluate(w, b):
            # (the kernel sees w rounded to fp32, the penalty below is taken from the fp64 w: a relative 6e-8 between the
            # two, four orders under tol)
            w_dev = torch.from_numpy(w.astype(np.float32)).to(emb.device)
            linkpred_lossgrad(emb, pairs, y, w_dev, b, None, partials)
            total = partials.sum(0, dtype=torch.float64).cpu().numpy()      # the G rows, in fp64; D + 2 numbers come back
            return total[:d], total[d], total[d + 1]

        theta, _, self.n_iter_, self.converged_, self.n_eval_ = lbfgs_minimize(
            logistic_objective(evaluate, n, self.C), np.zeros(d + 1), max_iter=self.max_iter, gtol=self.tol)
        self.coef_, self.intercept_ = theta[:-1].reshape(1, d), theta[-1:].copy()
        self.classes_ = np.array([0, 1])
        return self

    def decision_function(self, emb, pairs) -> np.ndarray:
        """z = <emb[u] * emb[v], coef_> + intercept_ per pair (float64 numpy): the kernel's forward-only call."""
        import torch

        if self.coef_ is None:
            raise ValueError("fit first")
        emb, pairs, _ = _device_examples(emb, pairs)
        scores = torch.empty(pairs.shape[0], dtype=torch.float32, device=emb.device)
        if pairs.shape[0]:
            w_dev = torch.from_numpy(self.coef_[0].astype(np.float32)).to(emb.device)
            linkpred_lossgrad(emb, pairs, None, w_dev, float(self.intercept_[0]), scores, None)
        return scores.cpu().numpy().astype(np.float64)

    def predict_proba(self, emb, pairs) -> np.ndarray:
        z = self.decision_function(emb, pairs)
        p1 = 0.5 * (1.0 + np.tanh(0.5 * z))             # sigmoid without overflow
        return np.stack([1.0 - p1, p1], axis=1)

    def predict(self, emb, pairs) -> np.ndarray:
        return (self.decision_function(emb, pairs) > 0).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- the score
def link_prediction_report(model, p: float = 0.5, test_size: float = 0.25, seed: int = 0, examples=None, vectors=None,
                           **logreg_kwargs) -> dict:
    """Score a fitted ``Node2Vec``: positives and negatives (``examples``: a ``link_prediction_examples`` result to share
    between models; default: drawn here from the model's own graph), a stratified 75 / 25 split, the classifier on the
    train block, the test block scored. ``vectors``: another [N, D] table of the same graph to score instead of the
    model's. Returns ``auc`` (ROC AUC of the predicted probabilities), ``auc_hard_labels`` (the reference's figure: it
    passes ``predict()`` output, 0 / 1, to ``roc_auc_score``, which makes it a balanced accuracy), ``n_train``, ``n_test``,
    ``n_iter``, ``converged``."""
    import torch

    if getattr(model, "rowptr", None) is None:
        raise ValueError("link_prediction_report needs a fitted Node2Vec (its graph and its table)")
    emb = model._w_in if vectors is None else vectors
    emb = to_device(emb, torch.float32)
    pairs, labels = examples if examples is not None else link_prediction_examples(model.rowptr, model.col, p, seed)
    train, test = stratified_split(labels, test_size, seed)
    order = np.concatenate([train, test])
    pairs_dev = to_device(pairs[order], torch.int32, emb.device)
    y_dev = to_device(labels[order], torch.float32, emb.device)
    k = len(train)
    clf = HadamardLogisticRegression(**logreg_kwargs).fit(emb, pairs_dev[:k], y_dev[:k])   # views: pointer offsets
    z = clf.decision_function(emb, pairs_dev[k:])
    y_test = labels[test]
    return {"auc": roc_auc(z, y_test),                  # (the probability is monotone in z: the same ranks)
            "auc_hard_labels": roc_auc(z > 0, y_test),
            "n_train": k, "n_test": len(test), "n_iter": clf.n_iter_, "converged": clf.converged_}


def run_link_prediction(kg_or_model, model=None, hard_labels: bool = True, **report_kwargs) -> float:
    """ref:node2vec.py:34-71 in its call shape, ``run_link_prediction(kg, model)``: the graph argument is accepted and
    ignored - a fitted ``Node2Vec`` carries its own graph (``run_link_prediction(model)`` works too). Returns the
    reference's figure (``auc_hard_labels``) by default, the AUC of the probabilities with ``hard_labels=False``."""
    report = link_prediction_report(model if model is not None else kg_or_model, **report_kwargs)
    return report["auc_hard_labels" if hard_labels else "auc"]
