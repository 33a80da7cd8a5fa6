"""TransE without a GPU: the three entry points exist in header, ctypes table and library and refuse bad arguments before any
launch; the host logic of stonkgs_amd/transe.py; and the numpy restatements of csrc/transe.hip - ``transe_step_ref`` (the
margin-ranking group exactly as the source file's header states it, random-number formula included) and ``rank_ref``.

The restatements are THE YARDSTICK of the GPU tests (test_transe_step_gpu.py, test_transe_rank_gpu.py, test_transe_gpu.py).
``transe_step_ref`` is anchored to the mathematics here, not to the kernel: its update is checked against central finite
differences of its own loss in fp64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from stonkgs_amd import _hip
from stonkgs_amd import kg_baseline_model as kgb
from stonkgs_amd import transe as tr
from stonkgs_amd.stonkgs_model import prepare_df

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("stonk_transe_step", "stonk_rows_l2_normalize", "stonk_transe_rank")
OK, EINVAL, ESHAPE, EALIGN = _hip.OK, _hip.EINVAL, _hip.ESHAPE, _hip.EALIGN
M32 = 0xFFFFFFFF
TRANSE_SALT = 0x74724573


# ---------------------------------------------------------------- the documented hash, on Python ints
def _h(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def _draw(key, attempt, which):
    return _h(key + (2 * attempt + which + 1) * 0x85EBCA77)


def group_negatives(g, epoch, h, t, n_entities, negatives, seed):
    """[(j, tail-replaced?, replacement entity, skipped?)] of group g: csrc/transe.hip's header, RANDOMNESS and (a)."""
    key = _h(_h(_h(seed ^ TRANSE_SALT) + g) ^ ((epoch * 0x9E3779B1) & M32))
    out = []
    for j in range(negatives):
        tail = bool(_draw(key, j, 1) >> 31)
        e = (_draw(key, j, 0) * n_entities) >> 32
        out.append((j, tail, e, e == (t if tail else h)))
    return out


def _dist(x, norm):
    return np.abs(x).sum(dtype=x.dtype) if norm == 1 else np.sqrt((x * x).sum(dtype=x.dtype))


def _grad(x, d, norm):
    if norm == 1:
        return np.sign(x)
    return np.zeros_like(x) if d < 1e-12 else x / d


def transe_step_ref(ent, rel, triples, order, groups, negatives, norm, margin, lr, seed, epoch, loss, log=None):
    """stonk_transe_step's groups one after the other in the dtype of ``ent`` (float64: the reference; float32: the error of
    the number format), in place. Mini-batch inside a group: everything from the rows as first read, then the adds.
    ``loss``: [sum, count]. ``log`` (a list) receives every decision taken: per group ``(g, triple, sign bytes of x_p for norm
    1, ((j, tail, e, skipped, active, sign bytes of x_j), ...))`` - a skipped group ``(g, triple, None, ())``."""
    dt = ent.dtype.type
    n_e, n_r, n = ent.shape[0], rel.shape[0], len(triples)
    margin, lr = dt(margin), dt(lr)
    for g in groups:
        tri = int(order[g]) if order is not None else g
        if not 0 <= tri < n:
            if log is not None:
                log.append((g, tri, None, ()))
            continue
        h, r, t = (int(v) for v in triples[tri])
        if not (0 <= h < n_e and 0 <= t < n_e and 0 <= r < n_r):
            if log is not None:
                log.append((g, tri, None, ()))
            continue
        hv, rv, tv = ent[h].copy(), rel[r].copy(), ent[t].copy()
        xp = (hv + rv) - tv
        dp = _dist(xp, norm)
        gp = _grad(xp, dp, norm)
        st, sh = np.zeros_like(xp), np.zeros_like(xp)
        adds, terms, active = [], [], 0
        for j, tail, e, skipped in group_negatives(g, epoch, h, t, n_e, negatives, seed):
            if skipped:
                terms.append((j, tail, e, True, False, b""))
                continue
            loss[1] += 1
            ev = ent[e]
            xj = (hv + rv) - ev if tail else (ev + rv) - tv
            dj = _dist(xj, norm)
            a = margin + dp - dj
            signs = np.sign(xj).astype(np.int8).tobytes() if norm == 1 else b""
            terms.append((j, tail, e, False, bool(a > 0), signs))
            if not a > 0:
                continue
            loss[0] += a
            active += 1
            gj = _grad(xj, dj, norm)
            if tail:
                st += gj
            else:
                sh += gj
            adds.append((e, -lr * gj if tail else lr * gj))
        if log is not None:
            log.append((g, tri, np.sign(xp).astype(np.int8).tobytes() if norm == 1 else b"", tuple(terms)))
        if not active:
            continue
        fa = dt(active)
        ent[h] += -lr * (fa * gp - st)
        rel[r] += -lr * ((fa * gp - st) - sh)
        ent[t] += -lr * (sh - fa * gp)
        for e, add in adds:
            ent[e] += add


def normalize_ref(table, row_lo, row_hi):
    """stonk_rows_l2_normalize in the dtype of ``table``, in place."""
    for i in range(row_lo, row_hi):
        nrm = np.sqrt((table[i] * table[i]).sum(dtype=table.dtype))
        if not nrm < 1e-12:
            table[i] = table[i] / nrm


def rank_distances(ent, rel, queries, side, norm):
    """``(dist [Q, N_e], true entity [Q], valid [Q])`` in the dtype of ``ent`` (any: float64, float32, or int64 on a table of
    integers): dist[q, c] = ||v_q - ent[c]||_1 or the squared L2 distance; v = h + r (side 0) or t - r (side 1)."""
    q = np.asarray(queries).reshape(-1, 3)
    n_e, n_r = ent.shape[0], rel.shape[0]
    valid = (q[:, 0] >= 0) & (q[:, 0] < n_e) & (q[:, 2] >= 0) & (q[:, 2] < n_e) & (q[:, 1] >= 0) & (q[:, 1] < n_r)
    qs = np.where(valid[:, None], q, 0)
    v = ent[qs[:, 0]] + rel[qs[:, 1]] if side == 0 else ent[qs[:, 2]] - rel[qs[:, 1]]
    dist = np.empty((len(q), n_e), dtype=ent.dtype)
    for i in range(len(q)):
        y = v[i][None, :] - ent
        dist[i] = np.abs(y).sum(axis=1, dtype=ent.dtype) if norm == 1 else (y * y).sum(axis=1, dtype=ent.dtype)
    return dist, np.where(valid, qs[:, 2] if side == 0 else qs[:, 0], -1), valid


def rank_ref(ent, rel, queries, side, norm, cand_ptr=None, cand=None):
    """stonk_transe_rank restated: ``(less, equal)`` int32 [Q]; -1 for a query with an id out of range."""
    dist, true, valid = rank_distances(ent, rel, queries, side, norm)
    less, equal = np.full(len(true), -1, dtype=np.int32), np.full(len(true), -1, dtype=np.int32)
    for i in np.flatnonzero(valid):
        if cand_ptr is None:
            d = dist[i]
        else:
            ids = np.asarray(cand[cand_ptr[i]:cand_ptr[i + 1]], dtype=np.int64)
            d = dist[i][ids[(ids >= 0) & (ids < ent.shape[0])]]
        less[i], equal[i] = (d < dist[i, true[i]]).sum(), (d == dist[i, true[i]]).sum()
    return less, equal


# ---------------------------------------------------------------- the symbols
def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "stonk_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert name in _hip._SIGNATURES
        assert hasattr(lib, name), name
    assert _hip.lib().stonk_abi_version() == 5
    assert "transe.o" in open(os.path.join(ROOT, "Makefile")).read()


def test_refusals_need_no_gpu():
    lib = _hip.lib()
    ok = dict(ent=16, rel=16, N_e=40, N_r=3, D=64, triples=16, n=10, order=0, g_lo=0, g_hi=5, K=1, norm=1, margin=1.0,
              lr=0.01, seed=0, epoch=0, loss=0, stream=0)

    def step(**kw):
        return lib.stonk_transe_step(*{**ok, **kw}.values())

    assert step(ent=0) == EINVAL and step(rel=0) == EINVAL and step(triples=0) == EINVAL
    assert step(norm=0) == EINVAL and step(norm=3) == EINVAL
    assert step(D=96) == ESHAPE and step(D=0) == ESHAPE and step(D=1088) == ESHAPE
    assert step(K=0) == ESHAPE and step(K=17, D=1024) == ESHAPE        # (17 rows of 1024 floats: beyond 64 KiB of LDS)
    assert step(g_lo=6) == ESHAPE and step(g_lo=-1) == ESHAPE and step(g_hi=11) == ESHAPE
    assert step(N_e=0) == ESHAPE and step(N_r=0) == ESHAPE and step(N_e=1 << 31) == ESHAPE and step(N_r=1 << 31) == ESHAPE
    assert step(n=1 << 31) == ESHAPE
    assert step(ent=24) == EALIGN and step(rel=8) == EALIGN and step(triples=18) == EALIGN and step(order=6) == EALIGN
    assert step(loss=2) == EALIGN
    assert step(g_lo=5) == OK and step(g_lo=0, g_hi=0) == OK           # (empty ranges: no launch)

    norm_ok = dict(table=16, ld=64, row_lo=0, row_hi=4, D=64, stream=0)

    def normalize(**kw):
        return lib.stonk_rows_l2_normalize(*{**norm_ok, **kw}.values())

    assert normalize(table=0) == EINVAL
    assert normalize(D=100) == ESHAPE and normalize(ld=63) == ESHAPE and normalize(row_lo=-1) == ESHAPE
    assert normalize(row_lo=5) == ESHAPE and normalize(row_hi=1 << 31) == ESHAPE and normalize(ld=1 << 31) == ESHAPE
    assert normalize(table=20) == EALIGN
    assert normalize(row_lo=4) == OK

    rank_ok = dict(ent=16, rel=16, N_e=40, N_r=3, D=64, norm=1, queries=16, Q=5, side=0, cand_ptr=0, cand=0, n_cand=0, less=16,
                   equal=16, stream=0)

    def rank(**kw):
        return lib.stonk_transe_rank(*{**rank_ok, **kw}.values())

    for null in ("ent", "rel", "queries", "less", "equal"):
        assert rank(**{null: 0}) == EINVAL, null
    assert rank(cand_ptr=16, cand=0, n_cand=3) == EINVAL
    assert rank(norm=0) == EINVAL and rank(side=2) == EINVAL and rank(side=-1) == EINVAL
    assert rank(D=32) == ESHAPE and rank(D=2048) == ESHAPE and rank(N_e=0) == ESHAPE and rank(N_r=1 << 31) == ESHAPE
    assert rank(Q=-1) == ESHAPE and rank(Q=1 << 31) == ESHAPE and rank(n_cand=-1) == ESHAPE
    assert rank(ent=8) == EALIGN and rank(cand_ptr=20, cand=16, n_cand=1) == EALIGN and rank(less=18) == EALIGN
    assert rank(Q=0) == OK


# ---------------------------------------------------------------- the step restated
def _tables(n_e, n_r, d, seed, dtype=np.float64):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1, 1, (n_e, d)).astype(dtype), rng.uniform(-1, 1, (n_r, d)).astype(dtype)


def test_negative_draws_follow_the_documented_formula():
    negs = group_negatives(7, 3, 2, 5, 40, 64, 11)
    assert [j for j, *_ in negs] == list(range(64))
    assert all(0 <= e < 40 for _, _, e, _ in negs)
    tails = sum(tail for _, tail, _, _ in negs)
    assert 16 <= tails <= 48                                              # a fair coin: 32 +- 4 sigma
    assert all(skipped == (e == (5 if tail else 2)) for _, tail, e, skipped in negs)
    assert negs != group_negatives(8, 3, 2, 5, 40, 64, 11) and negs != group_negatives(7, 4, 2, 5, 40, 64, 11)
    assert negs != group_negatives(7, 3, 2, 5, 40, 64, 12)
    assert negs[:5] == group_negatives(7, 3, 2, 5, 40, 5, 11)             # draw j does not depend on K
    many = [e for g in range(2000) for _, _, e, _ in group_negatives(g, 0, 0, 0, 7, 1, 0)]
    assert np.abs(np.bincount(many, minlength=7) / 2000 - 1 / 7).max() < 0.04    # uniform over the entities


@pytest.mark.parametrize("norm", [1, 2])
def test_step_restatement_is_the_gradient_of_its_own_loss(norm):
    """One group with active AND inactive terms: with lr = 1 the restatement moves the tables by minus the gradient of the
    loss it reports; central differences (step 1e-6, fp64) of that loss - the restatement itself at lr = 0 - agree."""
    n_e, n_r, d, K, seed, g = 6, 2, 64, 8, 5, 3
    ent0, rel0 = _tables(n_e, n_r, d, 1)
    triples = np.array([[0, 0, 1], [2, 1, 3], [4, 0, 4], [1, 1, 5]], dtype=np.int32)

    def loss_of(ent, rel, margin):
        acc = [0.0, 0]
        transe_step_ref(ent.copy(), rel.copy(), triples, None, [g], K, norm, margin, 0.0, seed, 0, acc)
        return acc[0]

    # a margin between the smallest and the largest d(x_j) - d(x_p): some terms active, some not
    probe = []
    transe_step_ref(ent0.copy(), rel0.copy(), triples, None, [g], K, norm, 0.0, 0.0, seed, 0, [0.0, 0], probe)
    h, r, t = triples[g]
    dp = _dist((ent0[h] + rel0[r]) - ent0[t], norm)
    gaps = sorted(_dist((ent0[h] + rel0[r]) - ent0[e] if tail else (ent0[e] + rel0[r]) - ent0[t], norm) - dp
                  for _, tail, e, skipped, _, _ in probe[0][3] if not skipped)
    margin = float((gaps[len(gaps) // 2 - 1] + gaps[len(gaps) // 2]) / 2)
    log = []
    ent, rel, acc = ent0.copy(), rel0.copy(), [0.0, 0]
    transe_step_ref(ent, rel, triples, None, [g], K, norm, margin, 1.0, seed, 0, acc, log)
    acts = [active for _, _, _, skipped, active, _ in log[0][3] if not skipped]
    assert any(acts) and not all(acts) and acc[1] == len(acts)
    assert abs(acc[0] - loss_of(ent0, rel0, margin)) < 1e-12
    grad_e, grad_r = ent0 - ent, rel0 - rel                               # lr = 1: the tables moved by -gradient
    eps = 1e-6
    for table, grad, which in ((ent0, grad_e, 0), (rel0, grad_r, 1)):
        for i in range(table.shape[0]):
            for k in range(0, d, 7):
                up, down = table.copy(), table.copy()
                up[i, k] += eps
                down[i, k] -= eps
                fd = (loss_of(up, rel0, margin) - loss_of(down, rel0, margin)) if which == 0 else \
                     (loss_of(ent0, up, margin) - loss_of(ent0, down, margin))
                assert abs(fd / (2 * eps) - grad[i, k]) < 1e-6, (which, i, k, fd / (2 * eps), grad[i, k])
    assert np.abs(grad_e).max() > 0.1 and np.abs(grad_r).max() > 0.1
    touched = {h, t} | {e for _, _, e, skipped, active, _ in log[0][3] if active}
    assert all((grad_e[i] == 0).all() for i in range(n_e) if i not in touched)


def test_step_restatement_skips_and_counts():
    ent0, rel0 = _tables(3, 1, 64, 2)
    triples = np.array([[0, 0, 0], [1, 0, 2], [0, 5, 1], [7, 0, 1]], dtype=np.int32)      # h == t; a bad relation; a bad head
    log, acc = [], [0.0, 0]
    ent, rel = ent0.copy(), rel0.copy()
    transe_step_ref(ent, rel, triples, None, range(4), 16, 1, 100.0, 0.01, 3, 0, acc, log)
    assert log[2][2] is None and log[3][2] is None                        # groups with an id outside its table
    terms = log[0][3] + log[1][3]
    skipped = sum(s for _, _, _, s, _, _ in terms)
    assert 0 < skipped < 32 and acc[1] == 32 - skipped                    # 3 entities: some replacements hit the replaced one
    pairs = [(tail, e) for _, tail, e, s, _, _ in log[1][3] if not s]
    assert len(set(pairs)) < len(pairs)                                   # equal negatives: each contributes
    ordered = [0.0, 0]
    e2, r2 = ent0.copy(), rel0.copy()
    transe_step_ref(e2, r2, triples[[1, 0, 3, 2]], np.array([1, 0, 3, 2], dtype=np.int32), range(4), 16, 1, 100.0, 0.01, 3, 0,
                    ordered)
    assert np.array_equal(e2, ent) and np.array_equal(r2, rel) and ordered == acc        # order undoes the permutation
    transe_step_ref(e2, r2, triples, np.array([9, -1], dtype=np.int32), range(2), 16, 1, 100.0, 0.01, 3, 0, ordered)
    assert np.array_equal(e2, ent) and ordered == acc                     # order entries outside [0, n): skipped


# ---------------------------------------------------------------- ranks
def test_rank_restatement_on_a_hand_made_table():
    ent = np.zeros((5, 64))
    ent[:, 0] = [0.0, 1.0, 2.0, 3.0, 1.0]                                  # entity 4 duplicates entity 1
    rel = np.zeros((1, 64))
    rel[0, 0] = 1.0
    q = np.array([[0, 0, 1], [1, 0, 3], [9, 0, 1]], dtype=np.int32)
    for norm in (1, 2):
        less, equal = rank_ref(ent, rel, q, 0, norm)                      # v = h + r: 1, 2, -
        assert less.tolist() == [0, 1, -1] and equal.tolist() == [2, 3, -1]          # query 1: closer entity 2; ties 1, 3, 4
        less, equal = rank_ref(ent, rel, q, 1, norm)                      # v = t - r: 0, 2, -; true heads 0, 1
        assert less.tolist() == [0, 1, -1] and equal.tolist() == [1, 3, -1]          # |2 - 1| = |2 - 3| = |2 - 1 (dup)|
        ptr, cand = np.array([0, 2, 2, 3]), np.array([4, 77, 0], dtype=np.int32)
        less, equal = rank_ref(ent, rel, q, 0, norm, ptr, cand)
        assert less.tolist() == [0, 0, -1] and equal.tolist() == [1, 0, -1]          # the list: 4 (a tie), 77 ignored; empty
    ints = (ent * 8).astype(np.int64), (rel * 8).astype(np.int64)
    assert [a.tolist() for a in rank_ref(*ints, q, 0, 2)] == [[0, 1, -1], [2, 3, -1]]


def test_rank_arithmetic_and_the_filtered_subtraction():
    less, equal = np.array([0, 2, 9, -1, 0]), np.array([1, 3, 1, -1, 2])
    ranks = tr.realistic_rank(less, equal)
    assert ranks[:3].tolist() == [1.0, 4.0, 10.0] and np.isnan(ranks[3]) and ranks[4] == 1.5
    m = tr.rank_metrics(ranks)
    assert m["mean_rank"] == pytest.approx((1 + 4 + 10 + 1.5) / 4) and m["mrr"] == pytest.approx((1 + 1 / 4 + 1 / 10 + 1 / 1.5) / 4)
    assert (m["hits@1"], m["hits@3"], m["hits@10"]) == (0.25, 0.5, 1.0)
    rep = tr.evaluation_report([1.0, 3.0], [2.0, 20.0])
    assert rep["tail"]["mean_rank"] == 2.0 and rep["head"]["mean_rank"] == 11.0 and rep["both"]["mean_rank"] == 6.5
    assert rep["mrr"] == rep["both"]["mrr"] == pytest.approx((1 + 1 / 3 + 1 / 2 + 1 / 20) / 4) and rep["hits@10"] == 0.75
    assert set(tr.METRICS) <= set(rep)
    # filtered: five closer entities of which three are other known tails, two ties of which one is one
    fl, fe = tr.filtered_counts([5, 0, -1], [3, 1, -1], [3, 0, -1], [1, 0, -1])
    assert fl.tolist() == [2, 0, -1] and fe.tolist() == [2, 1, -1]
    assert tr.realistic_rank(fl, fe)[0] == 2 + 1.5


def test_candidate_lists_leave_the_true_entity_out():
    known = np.array([[0, 0, 1], [0, 0, 2], [0, 0, 3], [4, 0, 1], [0, 1, 1], [0, 0, 2]])
    index = tr.known_index(known)
    assert index["tails"][(0, 0)] == [1, 2, 3] and index["heads"][(0, 1)] == [0, 4] and index["tails"][(0, 1)] == [1]
    queries = np.array([[0, 0, 2], [4, 0, 1], [5, 0, 6]])
    ptr, cand = tr.candidate_lists(queries, 0, index)
    assert ptr.dtype == np.int64 and cand.dtype == np.int32
    assert ptr.tolist() == [0, 2, 2, 2] and cand.tolist() == [1, 3]        # tails of (0, 0) without 2; (4, 0): only the true one
    ptr, cand = tr.candidate_lists(queries, 1, index)
    assert ptr.tolist() == [0, 0, 1, 1] and cand.tolist() == [0]           # heads of (0, 1) without 4; an unknown pair: empty


# ---------------------------------------------------------------- other host logic
def test_build_triples_numbers_by_first_appearance():
    names_e, names_r, triples = tr.build_triples(["b", "a", "b"], ["up", "down", "up"], ["a", "c", "b"])
    assert names_e == ["b", "a", "c"] and names_r == ["up", "down"]
    assert triples.dtype == np.int32 and triples.tolist() == [[0, 0, 1], [1, 1, 2], [0, 0, 0]]
    assert tr.build_triples([3, 7], [0, 0], [7, 9])[0] == [3, 7, 9]
    with pytest.raises(ValueError):
        tr.build_triples(["a"], ["r"], [])
    with pytest.raises(ValueError):
        tr.build_triples([], [], [])


def test_read_triples_from_a_file_a_frame_and_tuples(tmp_path):
    import pandas as pd

    df = pd.DataFrame({"source": ["a", "b"], "relation": ["r", "s"], "target": ["b", "c"], "evidence": ["x", "y"]})
    path = tmp_path / "pre.tsv"
    df.to_csv(path, sep="\t", index=False)
    want = (["a", "b"], ["r", "s"], ["b", "c"])
    assert tr._read_triples(str(path), "\t") == want and tr._read_triples(df, "\t") == want
    assert tr._read_triples([("a", "r", "b"), ("b", "s", "c")], "\t") == want


def test_launch_plan_covers_every_group_once_per_epoch():
    for n, per_epoch in ((1000, 64), (10, 64), (64, 64), (129, 7)):
        m = tr.TransE(epochs=3, launches_per_epoch=per_epoch)
        plan = m.launch_plan(n)
        assert len(plan) == 3 * min(n, per_epoch)
        for e in range(3):
            ranges = [(lo, hi) for ep, lo, hi in plan if ep == e]
            assert ranges[0][0] == 0 and ranges[-1][1] == n and all(lo < hi for lo, hi in ranges)
            assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))          # consecutive: every group exactly once
    m = tr.TransE(epochs=2, seed=4)
    o0, o1 = m.epoch_order(50, 0), m.epoch_order(50, 1)
    assert o0.dtype == np.int32 and sorted(o0.tolist()) == list(range(50)) and (o0 != o1).any()
    assert (m.epoch_order(50, 0) == o0).all() and (tr.TransE(seed=5).epoch_order(50, 0) != o0).any()
    assert m.launch_lr(3, 10) == 0.01
    decays = tr.TransE(lr=0.1, min_lr=0.01)
    assert decays.launch_lr(0, 10) == 0.1 and decays.launch_lr(5, 10) == pytest.approx(0.055)
    every = tr.TransE(normalize_every=4)
    assert [every.normalizes_after(i, 10) for i in range(10)] == [False] * 3 + [True] + [False] * 3 + [True, False, True]
    with pytest.raises(ValueError):
        tr.TransE(n_components=100)
    with pytest.raises(ValueError):
        tr.TransE(norm=3)
    with pytest.raises(ValueError):
        tr.TransE(negatives=0)


def test_initial_vectors_are_seeded_and_on_the_unit_sphere():
    m = tr.TransE(n_components=64, seed=3)
    ent, rel = m.initial_vectors(30, 4)
    assert ent.shape == (30, 64) and rel.shape == (4, 64) and ent.dtype == torch.float32
    assert torch.allclose(ent.norm(dim=1), torch.ones(30), atol=1e-6) and torch.allclose(rel.norm(dim=1), torch.ones(4), atol=1e-6)
    again = m.initial_vectors(30, 4)
    assert torch.equal(again[0], ent) and torch.equal(again[1], rel)
    assert not torch.equal(tr.TransE(n_components=64, seed=4).initial_vectors(30, 4)[0], ent)


def test_split_triples_is_seeded_and_disjoint():
    train, test = tr.split_triples(100, 0.1, 7)
    assert len(test) == 10 and len(train) == 90 and sorted(np.concatenate([train, test]).tolist()) == list(range(100))
    assert (tr.split_triples(100, 0.1, 7)[1] == test).all() and (tr.split_triples(100, 0.1, 8)[1] != test).any()
    with pytest.raises(ValueError):
        tr.split_triples(10, 1.0, 0)


def _fitted(names_e, names_r, d=64, seed=0):
    m = tr.TransE(n_components=d)
    rng = np.random.RandomState(seed)
    m.entity_names, m.relation_names = list(names_e), list(names_r)
    m.entity_vectors = rng.randn(len(names_e), d).astype(np.float32)
    m.relation_vectors = rng.randn(len(names_r), d).astype(np.float32)
    m._entity_index = {n: i for i, n in enumerate(m.entity_names)}
    m._relation_index = {n: i for i, n in enumerate(m.relation_names)}
    return m


def test_tsv_round_trip_through_the_baseline_loaders(tmp_path):
    m = _fitted(["p(HGNC:1)", "p(HGNC:2)", "a(CHEBI:3)"], ["increases", "decreases"])
    path = str(tmp_path / "transe.tsv")
    m.save_embeddings(path)
    emb = prepare_df(path)
    assert list(emb) == m.entity_names + m.relation_names                  # entity lines, then relation lines
    row_of, table = kgb.embedding_table(emb)
    assert table.dtype == np.float32 and np.array_equal(table[:3], m.entity_vectors) and np.array_equal(table[3:], m.relation_vectors)
    ids = kgb.transe_id_matrix(row_of, ["p(HGNC:1)", "a(CHEBI:3)"], ["decreases", "increases"], ["p(HGNC:2)", "p(HGNC:1)"])
    assert ids.tolist() == [[0, 4, 1], [2, 3, 0]] and (ids >= 0).all()
    assert np.array_equal(m.predict("a(CHEBI:3)"), m.entity_vectors[2]) and np.array_equal(m.predict("decreases"), m.relation_vectors[1])
    ds = kgb.TransEINDRAEntityDataset(emb, ["p(HGNC:1)"], ["increases"], ["a(CHEBI:3)"], [1])
    assert ds.ids.tolist() == [[0, 3, 2]]


def test_an_entity_and_a_relation_of_one_name_are_refused(tmp_path):
    m = _fitted(["a", "b", "binds"], ["binds"])
    with pytest.raises(ValueError):
        m.save_embeddings(str(tmp_path / "clash.tsv"))
    assert not os.path.exists(str(tmp_path / "clash.tsv"))


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_kernels_refuse_to_run_without_a_gpu():
    with pytest.raises(_hip.StonkHipError):
        tr.TransE(n_components=64, epochs=1).fit([("a", "r", "b")])
    with pytest.raises(_hip.StonkHipError):
        tr.transe_rank(np.zeros((2, 64), np.float32), np.zeros((1, 64), np.float32), [[0, 0, 1]], 0, 1)
