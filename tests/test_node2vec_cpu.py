"""CPU (no GPU): the host side of node2vec (stonkgs_amd/node2vec.py) and the numpy restatement of the two kernels of
csrc/node2vec.hip - the random-number formula, the walk step and the skip-gram group exactly as the source file's header
states them. The restatement is the SPEC: it is checked here against the analytic node2vec transition probabilities, and the
GPU tests (test_random_walk_gpu.py, test_sgns_gpu.py) pin the kernels to it - the walks bit for bit."""
import os
import re

import numpy as np
import pytest

from stonkgs_amd import _hip
from stonkgs_amd.node2vec import Node2Vec, alias_table, build_csr, walk_thresholds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESHAPE, EALIGN = _hip.OK, _hip.EINVAL, _hip.ESHAPE, _hip.EALIGN
M32 = 0xFFFFFFFF
WALK_SALT, SGNS_SALT, ATTEMPTS = 0x6E327677, 0x6E327367, 32


# ---------------------------------------------------------------- the documented hash, on uint64 arrays of 32-bit values
def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def key_of(seedkey, w, t):
    w = np.asarray(w, dtype=np.uint64) & np.uint64(M32)
    return hash32(hash32((np.uint64(seedkey) + w) & np.uint64(M32)) ^ np.uint64((t * 0x9E3779B1) & M32))


def draw(key, attempt, which):
    return hash32((np.asarray(key, dtype=np.uint64) + np.uint64(((2 * attempt + which + 1) * 0x85EBCA77) & M32)) & np.uint64(M32))


def mulhi(r, n):
    return (np.asarray(r, dtype=np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)


def walks_ref(rowptr, col, starts, n_walks, L, thr, seed, w_lo=0):
    """Rows [w_lo, w_lo + n_walks) of stonk_random_walks, all walks of the range stepped together."""
    n = len(rowptr) - 1
    seedkey = int(hash32(seed ^ WALK_SALT))
    w = np.arange(w_lo, w_lo + n_walks, dtype=np.int64)
    cur = (np.asarray(starts, dtype=np.int64)[w] if starts is not None else w % n).copy()
    prev = np.full(n_walks, -1, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    edge_keys = rows * n + col                      # sorted: membership here == the binary search in prev's list
    out = np.empty((n_walks, L), dtype=np.int32)
    out[:, 0] = cur
    first_order = thr[0] == thr[1] == thr[2]
    thr = np.asarray(thr, dtype=np.uint64)
    for t in range(1, L):
        lo = rowptr[cur]
        deg = (rowptr[cur + 1] - lo).astype(np.uint64)
        key = key_of(seedkey, w, t)
        nxt = cur.copy()
        pending = deg > 0
        if first_order or t == 1:
            pick = lo + mulhi(draw(key, 0, 0), deg).astype(np.int64)
            nxt[pending] = col[pick[pending]]
        else:
            for a in range(ATTEMPTS):
                i = np.flatnonzero(pending)
                if not len(i):
                    break
                cand = col[lo[i] + mulhi(draw(key[i], a, 0), deg[i]).astype(np.int64)].astype(np.int64)
                k = prev[i] * n + cand
                pos = np.minimum(np.searchsorted(edge_keys, k), len(edge_keys) - 1)
                cls = np.where(cand == prev[i], 0, np.where(edge_keys[pos] == k, 1, 2))
                accept = (draw(key[i], a, 1) >> np.uint64(8)) < thr[cls]
                nxt[i] = cand                      # (after the last attempt: the last candidate stays)
                pending[i[accept]] = False
        prev, cur = cur, nxt
        out[:, t] = cur
    return out


# ---------------------------------------------------------------- the skip-gram group, on Python ints and numpy rows
def _h(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def _draw(key, attempt, which):
    return _h(key + (2 * attempt + which + 1) * 0x85EBCA77)


def group_nodes(walks, w, t, n, window, negatives, alias_thr, alias_idx, seedkey):
    """(contexts, targets) of group (w, t): targets[0] is the centre, the rest its noise nodes (centre hits skipped).
    The skip rules of csrc/node2vec.hip's header: a centre outside [0, n) skips the group - ([], []) -, a context outside
    [0, n) the pair, an alias target outside [0, n) that noise node."""
    row = walks[w]
    L = len(row)
    c = int(row[t])
    if not 0 <= c < n:
        return [], []
    key = _h(_h(seedkey + w) ^ ((t * 0x9E3779B1) & M32))
    b = 1 + _draw(key, 0, 0) % window
    ctx = [int(row[u]) for u in range(max(t - b, 0), min(t + b, L - 1) + 1) if u != t and 0 <= int(row[u]) < n]
    tgt = [c]
    for j in range(negatives):
        slot = (_draw(key, j + 1, 0) * n) >> 32
        node = slot if _draw(key, j + 1, 1) < int(alias_thr[slot]) else int(alias_idx[slot])
        if node != c and 0 <= node < n:
            tgt.append(node)
    return ctx, tgt


def reduced_window(w, t, window, seed):
    """b of group (w, t): the kernel takes contexts from [t - b, t + b]."""
    key = _h(_h(_h(seed ^ SGNS_SALT) + w) ^ ((t * 0x9E3779B1) & M32))
    return 1 + _draw(key, 0, 0) % window


def sgns_ref(walks, w_in, w_out, groups, window, negatives, alias_thr, alias_idx, lr, seed, loss, nodes=group_nodes):
    """stonk_sgns_step's groups one after the other, in the dtype of w_in (float64: the reference; float32: the error of the
    number format). Mini-batch inside a group: every g from the rows as read first, then the adds. loss: [sum, count].
    A group whose centre is outside [0, N), or that has no valid context, adds nothing. ``nodes``: the group's node lists
    (tests/graph_ref.py swaps in deliberately wrong ones to show that its cases tell them apart)."""
    dt = w_in.dtype.type
    n = w_in.shape[0]
    seedkey = _h(seed ^ SGNS_SALT)
    lr = dt(lr)
    for w, t in groups:
        ctx, tgt = nodes(walks, w, t, n, window, negatives, alias_thr, alias_idx, seedkey)
        if not ctx:
            continue
        C, T = w_in[ctx], w_out[tgt]
        dots = C @ T.T
        label = np.zeros(len(tgt), dtype=w_in.dtype)
        label[0] = 1
        g = (label - dt(1) / (dt(1) + np.exp(-dots))) * lr
        z = np.where(label > 0, -dots, dots)      # -log sigmoid(dot) for the centre, -log sigmoid(-dot) for noise
        loss[0] += (np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))).sum(dtype=w_in.dtype)
        loss[1] += dots.size
        np.add.at(w_in, ctx, g @ T)
        np.add.at(w_out, tgt, g.T @ C)


# ---------------------------------------------------------------- tests
def test_build_csr_merges_sorts_and_keeps_names():
    src = ["b", "a", "b", "c", "a", "d"]
    tgt = ["a", "b", "c", "b", "c", "a"]           # a-b three times over both directions, b-c twice, a-c, a-d
    names, rowptr, col = build_csr(src, tgt)
    assert names == ["b", "a", "c", "d"]            # first appearance, source before target
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and rowptr.tolist() == [0, 2, 5, 7, 8]
    adj = {names[i]: [names[j] for j in col[rowptr[i]:rowptr[i + 1]]] for i in range(4)}
    assert adj == {"b": ["a", "c"], "a": ["b", "c", "d"], "c": ["b", "a"], "d": ["a"]}
    for i in range(4):
        seg = col[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(seg) > 0).all()             # sorted, no duplicates
    names2, rowptr2, col2 = build_csr([3, 7, 7], [7, 3, 9])
    assert names2 == [3, 7, 9] and rowptr2.tolist() == [0, 1, 3, 4] and col2.tolist() == [1, 0, 2, 1]
    with pytest.raises(ValueError):
        build_csr(["a"], [])


def test_alias_table_implies_the_noise_distribution():
    rng = np.random.RandomState(0)
    for n in (1, 2, 7, 1000):
        counts = rng.randint(0, 50, n).astype(np.int64)
        counts[rng.randint(n)] = 400                # one heavy node
        if n > 2:
            counts[:2] = 0                          # and nodes that never occur
        thr, idx = alias_table(counts)
        assert thr.dtype == np.uint32 and idx.dtype == np.int32 and len(thr) == len(idx) == n
        keep = np.where(idx == np.arange(n), 1.0, thr.astype(np.float64) / 2.0 ** 32)   # alias == self: always kept
        implied = keep.copy()
        np.add.at(implied, idx, 1.0 - keep)
        implied /= n
        want = counts.astype(np.float64) ** 0.75
        want[counts == 0] = 0
        want /= want.sum()
        assert np.abs(implied - want).max() <= n * 2.0 ** -32
        zero = np.flatnonzero(counts == 0)
        assert (thr[zero] == 0).all() and (idx[zero] != zero).all() and not np.isin(idx, zero).any()
    with pytest.raises(ValueError):
        alias_table([0, 0])


def test_thresholds_and_keyword_surface():
    assert walk_thresholds(1, 1, 1) == (1 << 24,) * 3
    assert walk_thresholds(4, 1, 0.25) == (1 << 24, 1 << 22, 1 << 20)
    assert walk_thresholds(0.25, 1, 4) == (1 << 20, 1 << 22, 1 << 24)
    m = Node2Vec()
    assert (m.n_components, m.walklen, m.epochs, m.window, m.negative, m.alpha, m.min_alpha, m.seed, m.keep_walks) == \
        (768, 127, 4, 3, 5, 0.025, 1e-4, 0, True)
    assert m.weights == (1.0, 1.0, 1.0)
    assert Node2Vec(return_weight=4, neighbor_weight=0.5).weights == (4.0, 0.5, 1.0)
    assert Node2Vec(p=0.25, q=4).weights == (4.0, 1.0, 0.25)
    assert Node2Vec(threads=96, verbose=True, w2vparams={"window": 5, "negative": 7, "iter": 1}).window == 5
    with pytest.raises(ValueError):
        Node2Vec(n_components=100)
    plan = Node2Vec(walklen=63, epochs=2).launch_plan(40)        # fewer walks than launches: positions are cut too
    assert len(plan) >= 2 * 64 and plan[0][1:] == (0, 1, 0, 31) and plan[-1][1:] == (79, 80, 31, 63)
    big = Node2Vec().launch_plan(1000)
    assert len(big) == 4 * 64 and all(p[3:] == (0, 127) for p in big) and big[-1][2] == 4000
    assert sum(hi - lo for _, lo, hi, _, _ in big) == 4000


def test_walk_restatement_matches_the_analytic_second_order_probabilities():
    """Triangle 0-1-2, path 2-3-4 (4 is a pendant: every step out of it is a return). Classes weighted (return, common
    neighbour, other) = (4, 1, 0.25): P(next = x | prev, cur) = weight(class of x) / sum over adj(cur). Over 2e5 second-order
    steps every observed frequency is within 4 binomial standard errors of it."""
    names, rowptr, col = build_csr([0, 1, 0, 2, 3], [1, 2, 2, 3, 4])
    assert names == [0, 1, 2, 3, 4]
    weights = (4.0, 1.0, 0.25)
    n_walks, L = 2000, 102                          # 2000 * 100 steps with a previous node
    walks = walks_ref(rowptr, col, None, n_walks, L, walk_thresholds(*weights), seed=11)
    adj = [set(col[rowptr[i]:rowptr[i + 1]].tolist()) for i in range(5)]
    prev, cur, nxt = walks[:, :-2].ravel(), walks[:, 1:-1].ravel(), walks[:, 2:].ravel()
    assert len(prev) == 200000
    checked = 0
    for p in range(5):
        for c in adj[p]:
            sel = (prev == p) & (cur == c)
            total = int(sel.sum())
            assert total > 1000
            wt = {x: weights[0] if x == p else weights[1] if x in adj[p] else weights[2] for x in adj[c]}
            for x, wx in wt.items():
                prob = wx / sum(wt.values())
                got = int((nxt[sel] == x).sum())
                se = np.sqrt(total * prob * (1 - prob))
                assert abs(got - total * prob) <= 4 * se + 1e-9, (p, c, x, got, total * prob, se)
                checked += 1
            assert not set(nxt[sel].tolist()) - adj[c]
    assert checked == sum(len(adj[c]) for p in range(5) for c in adj[p])
    # first-order walks (equal thresholds) are uniform over the neighbours
    uni = walks_ref(rowptr, col, None, 2000, 52, walk_thresholds(1, 1, 1), seed=3)
    at2 = uni[:, 1:][uni[:, :-1] == 2]
    for x in (0, 1, 3):
        prob, total = 1 / 3, len(at2)
        assert abs((at2 == x).sum() - total * prob) <= 4 * np.sqrt(total * prob * (1 - prob))


def _walks(**kw):
    a = dict(rowptr=4096, col=8192, N=10, starts=0, lo=0, hi=8, L=5, t0=1 << 24, t1=1 << 24, t2=1 << 24, seed=0, out=16384,
             ld=5, stream=0)
    a.update(kw)
    return _hip.lib().stonk_random_walks(*a.values())


def _sgns(**kw):
    a = dict(walks=4096, ld=5, L=5, wlo=0, whi=8, plo=0, phi=5, w_in=8192, w_out=16384, N=10, D=64, window=3, K=5,
             thr=32768, idx=65536, lr=0.025, seed=0, loss=0, stream=0)
    a.update(kw)
    return _hip.lib().stonk_sgns_step(*a.values())


def test_new_entries_are_declared_exported_bound_and_check_their_arguments():
    header = open(os.path.join(ROOT, "include", "stonk_hip.h")).read()
    for name in ("stonk_random_walks", "stonk_sgns_step"):
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert name in _hip.exported_symbols() and hasattr(_hip.lib(), name)
    assert _hip.lib().stonk_abi_version() == 5      # additions: the ABI number stays
    # ---- walks
    for null in ("rowptr", "col", "out"):
        assert _walks(**{null: 0}) == EINVAL, null
    assert _walks(L=0) == ESHAPE and _walks(lo=9, hi=8) == ESHAPE and _walks(ld=4) == ESHAPE and _walks(N=0) == ESHAPE
    assert _walks(lo=-1) == ESHAPE and _walks(t1=(1 << 24) + 1) == ESHAPE
    assert _walks(rowptr=4100) == EALIGN and _walks(col=8194) == EALIGN and _walks(starts=4098) == EALIGN
    assert _walks(out=16386) == EALIGN
    assert _walks(lo=8, hi=8) == OK and _walks(lo=0, hi=0) == OK          # empty range: nothing launched
    # ---- skip-gram
    for null in ("walks", "w_in", "w_out", "thr", "idx"):
        assert _sgns(**{null: 0}) == EINVAL, null
    assert _sgns(thr=0, idx=0, K=0, whi=0) == OK                          # no noise words: no alias table needed
    assert _sgns(D=96) == ESHAPE and _sgns(D=1088) == ESHAPE and _sgns(D=0) == ESHAPE
    assert _sgns(window=0) == ESHAPE and _sgns(K=-1) == ESHAPE
    assert _sgns(wlo=9, whi=8) == ESHAPE and _sgns(plo=3, phi=2) == ESHAPE and _sgns(phi=6) == ESHAPE
    assert _sgns(plo=-1) == ESHAPE and _sgns(ld=4) == ESHAPE and _sgns(N=0) == ESHAPE and _sgns(L=0, phi=0) == ESHAPE
    assert _sgns(D=1024, window=9) == ESHAPE                              # 18 context rows of 4 KiB: beyond the LDS
    assert _sgns(w_in=8200) == EALIGN and _sgns(w_out=16392) == EALIGN and _sgns(walks=4098) == EALIGN
    assert _sgns(thr=32770) == EALIGN and _sgns(idx=65538) == EALIGN and _sgns(loss=1026) == EALIGN
    assert _sgns(wlo=8, whi=8) == OK and _sgns(plo=2, phi=2) == OK        # empty ranges: nothing launched


def test_sgns_restatement_group_semantics():
    """The restatement itself: mini-batch inside a group (a revisited node gets one add per occurrence, all from the rows as
    read first), noise nodes equal to the centre skipped, fp32 and fp64 runs agree to fp32 rounding."""
    rng = np.random.RandomState(1)
    n, d = 6, 64
    walks = np.array([[0, 1, 0, 1, 2]], dtype=np.int32)
    thr, idx = alias_table([0, 1, 0, 0, 0, 0])      # all noise mass on node 1
    w_in, w_out = rng.uniform(-.5, .5, (n, d)), rng.uniform(-.5, .5, (n, d))
    seedkey = _h(5 ^ SGNS_SALT)
    ctx, tgt = group_nodes(walks, 0, 1, n, 3, 4, thr, idx, seedkey)
    assert tgt == [1] and set(ctx) <= {0, 1, 2} and ctx.count(0) >= 2   # centre 1: every noise draw hits it and is skipped
    a_in, a_out, loss = w_in.copy(), w_out.copy(), [0.0, 0]
    sgns_ref(walks, a_in, a_out, [(0, 1)], 3, 4, thr, idx, 0.5, 5, loss)
    g = (1 - 1 / (1 + np.exp(-(w_in[ctx] @ w_out[1])))) * 0.5
    want_in = w_in.copy()
    for gi, x in zip(g, ctx):
        want_in[x] += gi * w_out[1]
    assert np.allclose(a_in, want_in, atol=1e-15) and np.allclose(a_out[1], w_out[1] + g @ w_in[ctx], atol=1e-15)
    assert loss[1] == len(ctx) and np.isclose(loss[0], np.log1p(np.exp(-(w_in[ctx] @ w_out[1]))).sum())
    f_in, f_out, floss = w_in.astype(np.float32), w_out.astype(np.float32), [np.float32(0), 0]
    sgns_ref(walks, f_in, f_out, [(0, 1)], 3, 4, thr, idx, 0.5, 5, floss)
    assert f_in.dtype == np.float32 and np.abs(f_in - a_in).max() < 1e-6 and np.abs(f_out - a_out).max() < 1e-6
