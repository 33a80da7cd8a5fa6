"""GPU: stonk_sgns_step against the numpy restatement of tests/test_node2vec_cpu.py (sgns_ref).

(a) and (b) are exact by construction - one group per launch, or groups on disjoint rows - and compare W_in, W_out and the
loss sum with the restatement in fp64. Tolerance: the same restatement run in fp32 numpy deviates from fp64 by the rounding
of the number format on these very inputs; the kernel (another reduction order over 64 lanes, fused multiply-adds, a
few-ulp expf) is allowed 4x that figure, per quantity. The test prints its figures before it asserts. Measured on an
MI355X, max |x - fp64| after the whole sequence, fp32 numpy / kernel: D 768, K 5: W_in 1.48e-07 / 1.31e-07, W_out
4.53e-07 / 4.53e-07, loss sum 3.85e-05 / 3.85e-05; over all nine (D, K) cases W_in 1.3e-07 .. 1.9e-07 / 1.2e-07 .. 1.9e-07,
W_out 6.2e-08 .. 6.6e-07 / the same to two digits, loss sum 2.3e-06 .. 3.8e-05 / 2.3e-06 .. 3.8e-05 (kernel at most 1.6x
numpy); (b): W_in 3.2e-08 / 3.3e-08, W_out 3.2e-08 / 3.2e-08, loss sum 2.2e-04 / 9.8e-05.
(c) trains under real contention and compares the embedding quality with the restatement's; (d) is a star graph, where
every group touches the hub's rows. (c) measured: AUC 0.9995 for the restatement and 0.9995 for the kernel, 0.49 untrained."""
import numpy as np
import pytest
import torch

from stonkgs_amd.node2vec import Node2Vec, alias_table, build_csr
from tests.test_node2vec_cpu import sgns_ref

pytestmark = pytest.mark.gpu


def _tables(n, d, seed):
    rng = np.random.RandomState(seed)
    s = np.sqrt(3.0) * d ** -0.25                   # dot products of two rows have unit variance
    return (rng.uniform(-s, s, (n, d)).astype(np.float32), rng.uniform(-s, s, (n, d)).astype(np.float32))


def _step(hip, walks, lo, hi, plo, phi, w_in, w_out, window, k, thr, idx, lr, seed, loss):
    hip.call("stonk_sgns_step", hip.ptr(walks), walks.shape[1], walks.shape[1], lo, hi, plo, phi, hip.ptr(w_in),
             hip.ptr(w_out), w_in.shape[0], w_in.shape[1], window, k, hip.ptr(thr), hip.ptr(idx), lr, seed, hip.ptr(loss),
             hip.stream_ptr())


def _dev(thr, idx):
    return torch.from_numpy(thr.view(np.int32)).cuda(), torch.from_numpy(idx).cuda()


def _compare(tag, got, ref64, ref32):
    """got / ref64 / ref32: (W_in, W_out, loss sum, count). The kernel may deviate from fp64 by 4x what fp32 numpy does."""
    assert got[3] == ref64[3] == ref32[3], (tag, got[3], ref64[3])
    for name, g, r64, r32 in zip(("W_in", "W_out", "loss"), got, ref64, ref32):
        fmt = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max())
        ker = float(np.abs(np.asarray(g, dtype=np.float64) - r64).max())
        print(f"{tag} {name}: fp32-numpy {fmt:.3e}  kernel {ker:.3e}  allowed {4 * fmt:.3e}")
    for name, g, r64, r32 in zip(("W_in", "W_out", "loss"), got, ref64, ref32):
        fmt = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max())
        ker = float(np.abs(np.asarray(g, dtype=np.float64) - r64).max())
        assert np.isfinite(ker) and ker <= 4 * fmt, (tag, name, ker, fmt)


@pytest.mark.parametrize("K", [0, 1, 5])
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_single_groups_match_the_restatement(hip, D, K):
    """One group per launch: a walk with revisits (a b a b c), its first and last positions (truncated windows), a noise
    table concentrated on the centre (every noise draw is skipped), one concentrated on another node (equal negatives)."""
    n, window, lr, seed = 50, 3, 0.05, 77    # (a step size at which 45 groups on unit-variance dot products stay O(1))
    walks = np.array([[3, 4, 3, 4, 5], [9, 17, 9, 30, 17], [44, 2, 49, 0, 21]], dtype=np.int32)
    rng = np.random.RandomState(3)
    tables = [alias_table(rng.randint(1, 20, n)),                 # a spread-out noise distribution
              alias_table(np.eye(n)[4]),                          # all mass on node 4: the centre of (0, 1) and (0, 3)
              alias_table(np.eye(n)[7])]                          # all mass on node 7: K equal negatives
    groups = [(w, t) for w in range(3) for t in range(5)]
    w_in0, w_out0 = _tables(n, D, 5)
    r64 = [w_in0.astype(np.float64), w_out0.astype(np.float64), [0.0, 0]]
    r32 = [w_in0.copy(), w_out0.copy(), [np.float32(0), 0]]
    g_in, g_out = torch.from_numpy(w_in0).cuda(), torch.from_numpy(w_out0).cuda()
    g_walks, g_loss = torch.from_numpy(walks).cuda(), torch.zeros(2, device="cuda")
    for thr, idx in tables:
        d_thr, d_idx = _dev(thr, idx)
        for w, t in groups:
            _step(hip, g_walks, w, w + 1, t, t + 1, g_in, g_out, window, K, d_thr, d_idx, lr, seed, g_loss)
            for ref in (r64, r32):
                sgns_ref(walks, ref[0], ref[1], [(w, t)], window, K, thr, idx, lr, seed, ref[2])
    loss = g_loss.cpu().numpy()
    got = (g_in.cpu().numpy(), g_out.cpu().numpy(), float(loss[0]), int(loss[1]))
    assert np.abs(got[0] - w_in0).max() > 1e-3 and np.abs(got[1] - w_out0).max() > 1e-3     # the sequence did train
    _compare(f"D={D} K={K}", got, (r64[0], r64[1], float(r64[2][0]), r64[2][1]), (r32[0], r32[1], float(r32[2][0]), r32[2][1]))


def test_one_launch_over_disjoint_groups_matches_the_restatement(hip):
    """W = 1000 walks (no multiple of anything the grid is made of), L = 2, K = 0, positions [0, 1): walk w lives on its
    private nodes {2w, 2w + 1}, so the groups touch disjoint rows and one launch over all of them is exact whatever the
    scheduling - grid, tail and range indexing are what is left to go wrong. A second launch covers an inner range only."""
    W, D, window, lr, seed = 1000, 64, 3, 0.05, 5
    walks = np.arange(2 * W, dtype=np.int32).reshape(W, 2)
    w_in0, w_out0 = _tables(2 * W, D, 8)
    g_walks = torch.from_numpy(walks).cuda()
    for lo, hi in ((0, W), (137, 802)):
        r64 = [w_in0.astype(np.float64), w_out0.astype(np.float64), [0.0, 0]]
        r32 = [w_in0.copy(), w_out0.copy(), [np.float32(0), 0]]
        for ref in (r64, r32):
            sgns_ref(walks, ref[0], ref[1], [(w, 0) for w in range(lo, hi)], window, 0, None, None, lr, seed, ref[2])
        g_in, g_out, g_loss = torch.from_numpy(w_in0).cuda(), torch.from_numpy(w_out0).cuda(), torch.zeros(2, device="cuda")
        _step(hip, g_walks, lo, hi, 0, 1, g_in, g_out, window, 0, None, None, lr, seed, g_loss)
        loss = g_loss.cpu().numpy()
        got = (g_in.cpu().numpy(), g_out.cpu().numpy(), float(loss[0]), int(loss[1]))
        assert got[3] == hi - lo
        untouched = np.r_[0:2 * lo, 2 * hi:2 * W]
        assert np.array_equal(got[0][untouched], w_in0[untouched]) and np.array_equal(got[1][untouched], w_out0[untouched])
        _compare(f"disjoint [{lo},{hi})", got, (r64[0], r64[1], float(r64[2][0]), r64[2][1]),
                 (r32[0], r32[1], float(r32[2][0]), r32[2][1]))


def _auc(vectors, community):
    """AUC of the cosine similarity of two rows as a score for 'same community', by rank."""
    v = vectors / np.maximum(np.linalg.norm(vectors, axis=1, keepdims=True), 1e-30)
    i, j = np.triu_indices(len(v), 1)
    score, same = (v @ v.T)[i, j], community[i] == community[j]
    rank = np.empty(len(score))
    rank[np.argsort(score, kind="stable")] = np.arange(1, len(score) + 1)
    n_pos, n_neg = same.sum(), (~same).sum()
    return float((rank[same].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))


def _planted_partition():
    rng = np.random.RandomState(0)
    n = 128
    comm = np.arange(n) % 4
    a, b = np.triu_indices(n, 1)
    keep = rng.random_sample(len(a)) < np.where(comm[a] == comm[b], 0.3, 0.01)
    src, tgt = a[keep].tolist(), b[keep].tolist()
    seen = set(src) | set(tgt)
    for v in range(n):                               # an isolated node gets one edge into its community
        if v not in seen:
            src.append(v)
            tgt.append((v + 4) % n)
    names, rowptr, col = build_csr(src, tgt)
    return np.asarray(names), rowptr, col, comm


def test_training_under_contention_learns_the_communities(hip):
    """Planted partition, 128 nodes in 4 communities (node % 4), edge probability 0.3 inside / 0.01 across; D 64, L 40, 10
    walks per node, window 3, K 5, alpha 0.025 -> 1e-4, every epoch in 64 launches. AUC of cosine similarity, same-community
    pairs against the others: the restatement - the same walks, launches and learning rates, one group after the other -
    is the reference (0.9997 .. 0.9999 over three seeds on the CPU; a shortened schedule gives 0.71 .. 0.75, an untrained
    table 0.5); the kernel, whose groups of a launch run concurrently on stale rows, must reach it to within 0.01."""
    names, rowptr, col, comm = _planted_partition()
    n = len(names)
    assert n == 128
    community = comm[names]                          # node i of the graph is vertex names[i]
    m = Node2Vec(n_components=64, walklen=40, epochs=10, window=3, negative=5, alpha=0.025, min_alpha=1e-4, seed=1)
    walks = m.random_walks(rowptr, col)
    w_in = m.train(walks, n)
    vec, w_out = w_in.cpu().numpy(), m._w_out.cpu().numpy()
    assert np.isfinite(vec).all() and np.isfinite(w_out).all()
    assert m.loss_history[-1] < m.loss_history[0], m.loss_history
    plan = m.launch_plan(n)
    assert len(plan) >= 64 * m.epochs
    # the reference: the restatement over the same launches
    wk = walks.cpu().numpy()
    thr, idx = alias_table(m.counts)
    r_in, r_out, loss = m.initial_vectors(n).numpy().astype(np.float64), np.zeros((n, 64)), [0.0, 0]
    for i, (_, lo, hi, plo, phi) in enumerate(plan):
        lr = m.alpha - (m.alpha - m.min_alpha) * i / len(plan)
        sgns_ref(wk, r_in, r_out, [(w, t) for w in range(lo, hi) for t in range(plo, phi)], 3, 5, thr, idx, lr, m.seed, loss)
    ref_auc, gpu_auc, blank = _auc(r_in, community), _auc(vec, community), _auc(m.initial_vectors(n).numpy(), community)
    print(f"AUC: restatement {ref_auc:.4f}  kernel {gpu_auc:.4f}  untrained {blank:.4f}  loss per epoch {m.loss_history}")
    assert ref_auc > 0.99                            # the reference itself learned
    assert gpu_auc >= ref_auc - 0.01


def test_hub_contention_stays_finite(hip):
    """A 65-node star, D 768, one epoch: every group has the hub as centre or as context, so all of a launch's wavefronts
    add into the same two rows. (The per-row update count the kernel performs is not observable without an entry point of
    its own; the restatement's group semantics are pinned by the exact tests above.)"""
    names, rowptr, col = build_csr([0] * 64, list(range(1, 65)))
    m = Node2Vec(n_components=768, walklen=40, epochs=1, seed=2)
    walks = m.random_walks(rowptr, col)
    w_in = m.train(walks, 65)
    assert torch.isfinite(w_in).all() and torch.isfinite(m._w_out).all()
    assert not torch.equal(w_in.cpu(), m.initial_vectors(65)) and float(m._w_out.abs().max()) > 0
    assert np.isfinite(m.loss_history).all() and m.loss_history[0] > 0
