"""CPU (no GPU): the host side of the link-prediction score (stonkgs_amd/link_prediction.py, run_node2vec_hpo's trial
drawing) and the numpy restatement of the two kernels of csrc/link_prediction.hip, exactly as that file's header states
them. The restatement is the SPEC: it is checked here against its own definition (uniform non-edges) and, through
lbfgs_minimize, against scikit-learn's LogisticRegression; the GPU tests (test_link_prediction_gpu.py) pin the kernels to
it - the sampler bit for bit, the loss / gradient kernel to the error of the fp32 number format.

lossgrad_ref(..., dtype): float64 is the reference. float32 is the format-error yardstick: the same formulas evaluated
plainly in fp32 - the dot product over D element by element, the sums over the examples one example after the other, every
intermediate rounded to fp32. (A kernel sums in another order - per lane, then a butterfly over 64 lanes, per wavefront,
then per workgroup - which is no less accurate than one running sum; what it may not be is worse than 4x the plain one.)"""
import functools
import os
import re

import numpy as np
import pytest

from stonkgs_amd import _hip
from stonkgs_amd.link_prediction import (lbfgs_minimize, logistic_objective, roc_auc, sample_positive_edges,
                                         stratified_split)
from stonkgs_amd.node2vec import HPO_SEARCH_SPACE, build_csr, hpo_trials, search_trials
from tests.test_node2vec_cpu import draw, hash32, key_of, mulhi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESHAPE, EALIGN = _hip.OK, _hip.EINVAL, _hip.ESHAPE, _hip.EALIGN
NONEDGE_SALT, NONEDGE_ATTEMPTS = 0x6E326E65, 64


# ---------------------------------------------------------------- the restatements
def non_edges_ref(rowptr, col, lo, hi, seed):
    """Rows [lo, hi) of stonk_sample_non_edges and the number of failed samples among them."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    edge_keys = rows * n + np.asarray(col, dtype=np.int64)      # sorted: membership == the binary search in u's list
    i = np.arange(lo, hi, dtype=np.int64)
    key = key_of(int(hash32(seed ^ NONEDGE_SALT)), i, 0)
    out = np.full((hi - lo, 2), -1, dtype=np.int32)
    pending = np.ones(hi - lo, dtype=bool)
    for a in range(NONEDGE_ATTEMPTS):
        j = np.flatnonzero(pending)
        if not len(j):
            break
        u = mulhi(draw(key[j], a, 0), n).astype(np.int64)
        v = mulhi(draw(key[j], a, 1), n).astype(np.int64)
        k = u * n + v
        if len(edge_keys):
            pos = np.minimum(np.searchsorted(edge_keys, k), len(edge_keys) - 1)
            is_edge = edge_keys[pos] == k
        else:
            is_edge = np.zeros(len(j), dtype=bool)
        accept = (u != v) & ~is_edge
        out[j[accept], 0], out[j[accept], 1] = u[accept], v[accept]
        pending[j[accept]] = False
    return out, int(pending.sum())


def lossgrad_ref(emb, pairs, y, w, b, dtype=np.float64):
    """stonk_linkpred_lossgrad in ``dtype``: (scores [n] - NaN where a node id is outside [0, N) -, sum g x [D], sum g,
    sum loss). Every sum is a running sum in ``dtype`` (np.cumsum adds one element after the other)."""
    dt = np.dtype(dtype).type
    emb, w, y, b = np.asarray(emb).astype(dtype), np.asarray(w).astype(dtype), np.asarray(y).astype(dtype), dt(b)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_nodes, d = emb.shape
    ok = ((pairs >= 0) & (pairs < n_nodes)).all(axis=1)
    scores = np.full(len(pairs), np.nan, dtype=dtype)
    if not ok.any():
        return scores, np.zeros(d, dtype=dtype), dt(0), dt(0)
    x = emb[pairs[ok, 0]] * emb[pairs[ok, 1]]
    z = np.cumsum(x * w, axis=1, dtype=dtype)[:, -1] + b
    scores[ok] = z
    yy = y[ok]
    with np.errstate(over="ignore"):
        g = dt(1) / (dt(1) + np.exp(-z)) - yy
    loss = np.maximum(z, dt(0)) + np.log1p(np.exp(-np.abs(z))) - yy * z
    return (scores, np.cumsum(g[:, None] * x, axis=0, dtype=dtype)[-1], np.cumsum(g, dtype=dtype)[-1],
            np.cumsum(loss, dtype=dtype)[-1])


def planted_problem(d, seed=0, n_nodes=200, n_examples=600):
    """200 nodes in four communities, vectors = community centre + noise scaled so that <x, 1> has O(1) spread; 600 pairs,
    half of them inside a community; label = same community, 10 % of the labels flipped. Returns (emb fp32 [200, d],
    pairs int32 [600, 2], y fp32 [600])."""
    rng = np.random.RandomState(seed)
    comm = np.arange(n_nodes) % 4
    s = d ** -0.25
    emb = ((rng.standard_normal((4, d))[comm] + rng.standard_normal((n_nodes, d))) * s).astype(np.float32)
    u = rng.randint(0, n_nodes, n_examples)
    same = np.arange(n_examples) % 2 == 0
    v = np.where(same, (u + 4 * rng.randint(1, n_nodes // 4, n_examples)) % n_nodes,
                 (u + 4 * rng.randint(0, n_nodes // 4, n_examples) + rng.randint(1, 4, n_examples)) % n_nodes)
    assert ((comm[u] == comm[v]) == same).all() and (u != v).all()
    y = same ^ (rng.random_sample(n_examples) < 0.1)
    order = rng.permutation(n_examples)
    return emb, np.stack([u, v], axis=1).astype(np.int32)[order], y.astype(np.float32)[order]


def fit_ref(emb, pairs, y, C=1.0, gtol=1e-4, max_iter=100):
    """lbfgs_minimize on the objective of HadamardLogisticRegression, evaluated by lossgrad_ref in fp64."""
    fun = logistic_objective(lambda w, b: lossgrad_ref(emb, pairs, y, w, b)[1:], len(pairs), C)
    return lbfgs_minimize(fun, np.zeros(emb.shape[1] + 1), max_iter=max_iter, gtol=gtol)


@functools.lru_cache(maxsize=None)
def planted_fit(d):
    """The fp64 fit of the planted problem's first 450 examples at the classifier's defaults (shared by the GPU tests):
    (problem, (theta, value, n_iter, converged, n_eval))."""
    emb, pairs, y = planted_problem(d)
    return (emb, pairs, y), fit_ref(emb, pairs[:450], y[:450])


# ---------------------------------------------------------------- tests
def _sample(**kw):
    a = dict(rowptr=4096, col=8192, N=10, lo=0, hi=8, seed=0, out=16384, fail=32768, stream=0)
    a.update(kw)
    return _hip.lib().stonk_sample_non_edges(*a.values())


def _lossgrad(**kw):
    a = dict(emb=4096, ld=64, N=10, D=64, pairs=8192, y=16384, n=8, w=32768, b=0.0, scores=65536, partials=131072, stream=0)
    a.update(kw)
    return _hip.lib().stonk_linkpred_lossgrad(*a.values())


def test_new_entries_are_declared_exported_bound_and_check_their_arguments():
    header = open(os.path.join(ROOT, "include", "stonk_hip.h")).read()
    for name in ("stonk_sample_non_edges", "stonk_linkpred_lossgrad"):
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert name in _hip.exported_symbols() and name in _hip._SIGNATURES and hasattr(_hip.lib(), name)
    assert re.search(r"^int64_t stonk_linkpred_partial_rows\(void\);", header, flags=re.M)
    assert "stonk_linkpred_partial_rows" in _hip.exported_symbols()
    rows = _hip.lib().stonk_linkpred_partial_rows()               # a size query: no GPU touched
    assert isinstance(rows, int) and 1 <= rows <= 4096
    assert _hip.lib().stonk_abi_version() == 5                    # additions: the ABI number stays
    # ---- negatives
    for null in ("rowptr", "col", "out", "fail"):
        assert _sample(**{null: 0}) == EINVAL, null
    assert _sample(N=0) == ESHAPE and _sample(N=1 << 31) == ESHAPE and _sample(lo=-1) == ESHAPE
    assert _sample(lo=9, hi=8) == ESHAPE and _sample(hi=1 << 30) == ESHAPE
    assert _sample(rowptr=4100) == EALIGN and _sample(col=8194) == EALIGN and _sample(out=16386) == EALIGN
    assert _sample(fail=32770) == EALIGN
    assert _sample(lo=8, hi=8) == OK and _sample(lo=0, hi=0) == OK          # empty range: nothing launched
    # ---- loss and gradient
    for null in ("emb", "pairs", "w"):
        assert _lossgrad(**{null: 0}) == EINVAL, null
    assert _lossgrad(scores=0, partials=0) == EINVAL                        # nothing to compute
    assert _lossgrad(y=0) == EINVAL                                         # a gradient needs the labels
    assert _lossgrad(y=0, partials=0, n=0) == OK                            # the forward pass does not
    assert _lossgrad(D=96, ld=96) == ESHAPE and _lossgrad(D=1088, ld=1088) == ESHAPE and _lossgrad(D=0) == ESHAPE
    assert _lossgrad(ld=63) == ESHAPE and _lossgrad(ld=1 << 31) == ESHAPE and _lossgrad(N=0) == ESHAPE
    assert _lossgrad(N=1 << 31) == ESHAPE and _lossgrad(n=-1) == ESHAPE
    assert _lossgrad(emb=4098) == EALIGN and _lossgrad(pairs=8196) == EALIGN and _lossgrad(y=16386) == EALIGN
    assert _lossgrad(w=32770) == EALIGN and _lossgrad(scores=65538) == EALIGN and _lossgrad(partials=131074) == EALIGN
    assert _lossgrad(n=0) == OK and _lossgrad(n=0, D=1024, ld=1024) == OK   # empty range: nothing launched


@pytest.mark.parametrize("d", [64, 768])
def test_lbfgs_on_the_restatement_finds_scikit_learns_coefficients(d):
    """The optimiser and the fp64 restatement against sklearn.linear_model.LogisticRegression(C=1, tol=1e-10,
    max_iter=20000) on the materialised Hadamard features. Gradient tolerance 1e-6 on the unscaled objective (1e-6 / n on
    the mean). Measured: 44 iterations at both sizes, max |coef - sklearn| 4.2e-7 (D 64) and 4.9e-7 (D 768); the bound
    leaves room for another BLAS or library build."""
    linear_model = pytest.importorskip("sklearn.linear_model")
    emb, pairs, y = planted_problem(d)
    theta, _, n_iter, converged, _ = fit_ref(emb, pairs, y, C=1.0, gtol=1e-6 / len(pairs), max_iter=500)
    x = emb[pairs[:, 0]].astype(np.float64) * emb[pairs[:, 1]]
    ref = linear_model.LogisticRegression(C=1.0, tol=1e-10, max_iter=20000).fit(x, y.astype(np.int64))
    diff = max(np.abs(theta[:-1] - ref.coef_[0]).max(), abs(theta[-1] - ref.intercept_[0]))
    print(f"D={d}: {n_iter} iterations, max |coef - sklearn| {diff:.3e}")
    assert converged and n_iter < 100
    assert diff <= 1e-5
    auc = roc_auc(lossgrad_ref(emb, pairs, y, theta[:-1], theta[-1])[0], y)
    assert auc > 0.8                                  # 10 % of the labels are flipped: about 0.9 is the ceiling


def test_lbfgs_minimize_on_a_quadratic_and_at_its_limits():
    rng = np.random.RandomState(0)
    a = rng.standard_normal((30, 12))
    h, c = a.T @ a + 0.1 * np.eye(12), rng.standard_normal(12)
    x, f, n_iter, converged, n_eval = lbfgs_minimize(lambda v: (0.5 * v @ h @ v - c @ v, h @ v - c), np.zeros(12),
                                                     max_iter=200, gtol=1e-10)
    assert converged and np.abs(x - np.linalg.solve(h, c)).max() < 1e-8 and n_eval >= n_iter + 1
    assert np.isclose(f, 0.5 * x @ h @ x - c @ x)
    _, _, n_iter, converged, _ = lbfgs_minimize(lambda v: (0.5 * v @ h @ v - c @ v, h @ v - c), np.zeros(12), max_iter=2,
                                                gtol=1e-12)
    assert n_iter == 2 and not converged              # the iteration cap
    x0 = np.linalg.solve(h, c)
    x, _, n_iter, converged, n_eval = lbfgs_minimize(lambda v: (0.5 * v @ h @ v - c @ v, h @ v - c), x0, gtol=1e-6)
    assert converged and n_iter == 0 and n_eval == 1 and np.array_equal(x, x0)      # already there


def test_roc_auc_equals_scikit_learns_with_and_without_ties():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.RandomState(2)
    labels = rng.randint(0, 2, 500)
    cont = rng.standard_normal(500) + 0.7 * labels
    hard = (cont > 0.3).astype(np.int64)              # 0 / 1 scores: two large groups of ties
    coarse = np.round(cont, 1)                        # and many small ones
    for s in (cont, hard, coarse):
        assert abs(roc_auc(s, labels) - metrics.roc_auc_score(labels, s)) < 1e-12
    assert roc_auc([0.1, 0.2, 0.8, 0.9], [0, 0, 1, 1]) == 1.0 and roc_auc([1, 1, 1, 1], [0, 1, 0, 1]) == 0.5
    tpr, tnr = (hard[labels == 1] == 1).mean(), (hard[labels == 0] == 0).mean()
    assert abs(roc_auc(hard, labels) - 0.5 * (tpr + tnr)) < 1e-12      # on hard labels: the balanced accuracy
    with pytest.raises(ValueError):
        roc_auc([0.1, 0.2], [1, 1])


def _small_graph():
    # 7 nodes: a triangle 0-1-2, a path 2-3-4-5, node 6 attached to 0
    return build_csr([0, 1, 0, 2, 3, 4, 6], [1, 2, 2, 3, 4, 5, 0])


def test_non_edge_restatement_is_uniform_over_non_adjacent_ordered_pairs():
    names, rowptr, col = _small_graph()
    n = len(names)
    adj = [set(col[rowptr[i]:rowptr[i + 1]].tolist()) for i in range(n)]
    allowed = [(u, v) for u in range(n) for v in range(n) if u != v and v not in adj[u]]
    assert len(allowed) == n * n - n - len(col)
    s = 40000
    out, failed = non_edges_ref(rowptr, col, 0, s, seed=9)
    assert failed == 0 and out.min() >= 0             # acceptance 28/49 per attempt: 64 rejections do not happen
    got = {}
    for u, v in out.tolist():
        got[(u, v)] = got.get((u, v), 0) + 1
    assert set(got) == set(allowed)                   # never an edge, never a self-pair, every non-edge reached
    prob = 1.0 / len(allowed)
    se = np.sqrt(s * prob * (1 - prob))
    for pair in allowed:
        assert abs(got[pair] - s * prob) <= 4 * se, (pair, got[pair], s * prob, se)
    # a pure function of (seed, i): a cut range gives the same rows; another seed gives others
    part, _ = non_edges_ref(rowptr, col, 137, 802, seed=9)
    assert np.array_equal(part, out[137:802])
    assert not np.array_equal(non_edges_ref(rowptr, col, 0, 100, seed=10)[0], out[:100])


def test_non_edge_restatement_fails_every_sample_on_a_complete_graph():
    a, b = np.triu_indices(12, 1)
    _, rowptr, col = build_csr(a.tolist(), b.tolist())
    out, failed = non_edges_ref(rowptr, col, 0, 300, seed=1)
    assert failed == 300 and (out == -1).all()
    keep = np.ones(len(a), dtype=bool)
    keep[[20, 40, 60]] = False                        # three edges fewer: 6 of 144 ordered pairs are acceptable
    names, rowptr, col = build_csr(a[keep].tolist(), b[keep].tolist())
    assert names == list(range(12))
    out, failed = non_edges_ref(rowptr, col, 0, 2000, seed=1)
    gone = {(int(x), int(y)) for x, y in zip(a[~keep], b[~keep])}
    assert 0 < failed < 2000 and failed == int((out[:, 0] < 0).sum())
    assert {tuple(sorted(r)) for r in out[out[:, 0] >= 0].tolist()} == gone
    expect = 2000 * (1 - 2 * len(gone) / 144.0) ** 64
    assert abs(failed - expect) <= 4 * np.sqrt(expect)


def test_lossgrad_restatement_skips_bad_ids_and_its_two_precisions_agree():
    rng = np.random.RandomState(4)
    emb = rng.uniform(-1, 1, (9, 64)).astype(np.float32)
    pairs = np.array([[0, 1], [2, 2], [-1, 3], [4, 9], [5, 0]], dtype=np.int32)
    y = np.array([1, 0, 1, 0, 1], dtype=np.float32)
    w = rng.uniform(-.3, .3, 64).astype(np.float32)
    scores, gx, gsum, loss = lossgrad_ref(emb, pairs, y, w, 0.25)
    assert np.isnan(scores[[2, 3]]).all() and np.isfinite(scores[[0, 1, 4]]).all()
    x = emb[[0, 2, 5]].astype(np.float64) * emb[[1, 2, 0]]
    z = x @ w.astype(np.float64) + 0.25
    g = 1 / (1 + np.exp(-z)) - y[[0, 1, 4]]
    assert np.allclose(scores[[0, 1, 4]], z, atol=1e-14) and np.allclose(gx, g @ x, atol=1e-14)
    assert np.isclose(gsum, g.sum()) and np.isclose(loss, (np.log1p(np.exp(z)) - y[[0, 1, 4]] * z).sum())
    s32, gx32, gsum32, loss32 = lossgrad_ref(emb, pairs, y, w, 0.25, np.float32)
    assert s32.dtype == gx32.dtype == np.float32
    assert np.nanmax(np.abs(s32 - scores)) < 1e-5 and np.abs(gx32 - gx).max() < 1e-5 and abs(loss32 - loss) < 1e-5
    big = lossgrad_ref(emb, pairs[:2], y[:2], 200 * w, 0.0, np.float32)     # |z| far beyond where exp(z) fits fp32's sum
    assert np.isfinite(big[3]) and np.abs(big[0]).max() > 30


def test_sample_positive_edges():
    rng = np.random.RandomState(5)
    a, b = np.triu_indices(40, 1)
    keep = rng.random_sample(len(a)) < 0.2
    _, rowptr, col = build_csr(a[keep].tolist() + [3], b[keep].tolist() + [3])     # (and a self-loop: no candidate)
    edges = int((np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)) < col).sum())
    for p in (0.5, 0.3, 1.0):
        pos = sample_positive_edges(rowptr, col, p, seed=3)
        assert pos.dtype == np.int32 and pos.shape == (int(np.floor(p * edges)), 2)
        assert (pos[:, 0] < pos[:, 1]).all() and len({tuple(r) for r in pos.tolist()}) == len(pos)
        assert all(v in col[rowptr[u]:rowptr[u + 1]] for u, v in pos.tolist())
    assert np.array_equal(sample_positive_edges(rowptr, col, 0.5, seed=3), sample_positive_edges(rowptr, col, 0.5, seed=3))
    assert not np.array_equal(sample_positive_edges(rowptr, col, 0.5, seed=3), sample_positive_edges(rowptr, col, 0.5, seed=4))


def test_stratified_split_keeps_the_class_shares_and_covers_everything():
    rng = np.random.RandomState(6)
    for n, share in ((1000, 0.5), (37, 0.3), (8, 0.5)):
        y = (rng.random_sample(n) < share).astype(np.float32)
        y[:2] = (0, 1)
        train, test = stratified_split(y, 0.25, seed=1)
        assert len(set(train.tolist()) & set(test.tolist())) == 0
        assert sorted(train.tolist() + test.tolist()) == list(range(n))
        for c in (0, 1):
            total = int((y == c).sum())
            assert abs(int((y[test] == c).sum()) - 0.25 * total) <= 1       # to within one example
        again = stratified_split(y, 0.25, seed=1)
        assert np.array_equal(train, again[0]) and np.array_equal(test, again[1])
    y = (rng.random_sample(1000) < 0.5).astype(np.float32)
    assert not np.array_equal(stratified_split(y, 0.25, seed=2)[1], stratified_split(y, 0.25, seed=1)[1])


def test_hpo_trials_are_drawn_without_replacement_capped_and_seeded():
    assert HPO_SEARCH_SPACE == {"epochs": [2, 4, 8], "window": [3, 4, 5]}
    grid = {(e, w) for e in (2, 4, 8) for w in (3, 4, 5)}
    for k in (1, 4, 9):
        trials = hpo_trials(HPO_SEARCH_SPACE, k, seed=11)
        assert len(trials) == k and len({(t["epochs"], t["window"]) for t in trials}) == k
        assert {(t["epochs"], t["window"]) for t in trials} <= grid
    assert {(t["epochs"], t["window"]) for t in hpo_trials(HPO_SEARCH_SPACE, 50, seed=0)} == grid      # capped at the grid
    assert hpo_trials(HPO_SEARCH_SPACE, 4, seed=11) == hpo_trials(HPO_SEARCH_SPACE, 4, seed=11)
    assert len({tuple(sorted(t.items())) for s in range(20) for t in hpo_trials(HPO_SEARCH_SPACE, 1, seed=s)}) > 3
    assert hpo_trials({"epochs": [1, 2], "window": [2, 3]}, 2, seed=5)[0].keys() == {"epochs", "window"}
    with pytest.raises(ValueError):
        hpo_trials(HPO_SEARCH_SPACE, 0, seed=0)


def test_search_keeps_the_highest_score_and_the_earlier_of_equal_ones():
    """search_trials with stubbed trials (no GPU): maximisation, the tie-break, the order of the results, the warnings."""
    import warnings

    def stub(scores, n_iter=5):
        ran = []

        def run_trial(params):
            ran.append(params["id"])
            return f"model{params['id']}", {"auc_hard_labels": scores[params["id"]], "auc": 1 - scores[params["id"]],
                                           "n_iter": n_iter}
        return [{"id": i} for i in range(len(scores))], run_trial, ran

    with warnings.catch_warnings():
        warnings.simplefilter("error")               # distinct scores, classifiers that iterated: no warning
        for scores, want in (([0.6, 0.9, 0.7], 1), ([0.9, 0.6, 0.7], 0), ([0.6, 0.7, 0.9], 2),    # the maximum, wherever it is
                             ([0.6, 0.9, 0.9], 1), ([0.8, 0.8, 0.7], 0)):                          # ties: the earlier trial
            trials, run_trial, ran = stub(scores)
            best, results = search_trials(trials, run_trial)
            assert best == f"model{want}", (scores, best)
            assert ran == [0, 1, 2] and [p for p, _ in results] == trials                     # every trial ran once, in order
            assert [r["auc_hard_labels"] for _, r in results] == scores
        trials, run_trial, _ = stub([0.6, 0.9, 0.7])
        assert search_trials(trials, run_trial, score_key="auc")[0] == "model0"                # (1 - score: another key)
        trials, run_trial, _ = stub([0.5])
        assert search_trials(trials, run_trial)[0] == "model0"                                 # one trial: nothing to warn of
    trials, run_trial, _ = stub([0.5, 0.5, 0.5])
    with pytest.warns(UserWarning, match="all 3 trials score 0.5000"):
        assert search_trials(trials, run_trial)[0] == "model0"
    trials, run_trial, _ = stub([0.5, 0.8], n_iter=0)
    with pytest.warns(UserWarning, match="starting point"):
        assert search_trials(trials, run_trial)[0] == "model1"
