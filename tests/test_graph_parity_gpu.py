"""GPU: the graph-side kernels on the paths their first tests do not reach - csrc/node2vec.hip (skip-gram step),
csrc/transe.hip (step, row normalisation, ranks), csrc/link_prediction.hip (loss / gradient) and csrc/kg_baseline.hip.

Cases, references and the launch constants they are sized by live in tests/graph_ref.py; tests/test_graph_ref_cpu.py shows
without a GPU that every case reaches its branch and tells a restatement with one mistake apart. The rule is the
project's (graph_ref.compare): per quantity, over an array, the kernel may deviate from the float64 restatement by 4x what
the float32 restatement deviates from it on the same inputs; bit equality where the construction makes the arithmetic
exact. Every test prints its figures (lines starting with GRAPH) before it asserts; profiles/graph_parity.md records them
as measured on an MI355X, with the mutation table."""
import numpy as np
import pytest
import torch

from stonkgs_amd import kg_baseline_model as kgb
from stonkgs_amd import transe as tr
from tests import graph_ref as gr
from tests.test_kg_baseline_cpu import Restatement
from tests.test_kg_baseline_gpu import _pool_call, _state, _trainer, _walk
from tests.test_link_prediction_gpu import _case as linkpred_case
from tests.test_link_prediction_gpu import _rows, _totals
from tests.test_sgns_gpu import _dev, _step as sgns_step
from tests.test_transe_rank_gpu import integer_counts
from tests.test_transe_step_gpu import _step as transe_step

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ skip-gram: grid stride
def test_sgns_launch_beyond_the_grid_cap(hip):
    """cap + 904 groups on disjoint rows in one launch, four ranges: wavefront b takes groups b and b + cap; of the first
    904 some skip in their first trip (centre -1 or N; no valid context) and must still do their second group."""
    cap = gr.geometry()["sgns_cap"]
    walks, (w_in0, w_out0), _, _ = gr.sgns_stride_case()
    g_walks = torch.from_numpy(walks).cuda()
    m_in, m_out = torch.from_numpy(w_in0).cuda(), torch.from_numpy(w_out0).cuda()
    for lo, hi in gr.sgns_stride_ranges():
        assert hi - lo > cap, "sgns stride: the launcher's cap changed and this range no longer exceeds it"
        e64, e32 = gr.sgns_stride_expected(lo, hi, 0), gr.sgns_stride_expected(lo, hi, 1)
        g_in, g_out, g_loss = m_in.clone(), m_out.clone(), torch.zeros(2, device="cuda")
        sgns_step(hip, g_walks, lo, hi, 0, 1, g_in, g_out, 3, 0, None, None, gr.SGNS_STRIDE_LR, gr.SGNS_STRIDE_SEED, g_loss)
        k_in, k_out, k_loss = g_in.cpu().numpy(), g_out.cpu().numpy(), g_loss.cpu().numpy()
        bound = gr.sgns_stride_loss_bound(e64[3], e64[2])
        print(f"GRAPH sgns stride [{lo},{hi}): count kernel {int(k_loss[1])} restatement {e64[3]}; loss sum: fp32-restatement "
              f"{abs(e32[2] - e64[2]):.3e}  kernel {abs(float(k_loss[0]) - e64[2]):.3e}  allowed {bound:.3e}")
        assert int(k_loss[1]) == e64[3] == e32[3]
        assert abs(float(k_loss[0]) - e64[2]) <= bound
        still_in, still_out = gr.sgns_stride_untouched(lo, hi)
        assert still_in.sum() >= 2 * (len(walks) - (hi - lo)) and not still_in.all()
        assert _same_bits(k_in[still_in], w_in0[still_in]) and _same_bits(k_out[still_out], w_out0[still_out])
        gr.compare(f"sgns stride [{lo},{hi})", ("W_in", "W_out"), (k_in, k_out), e64[:2], e32[:2])


# ------------------------------------------------------------------------------------------------ skip-gram: window, ids
@pytest.mark.parametrize("D", [64, 1024])
def test_sgns_full_window_and_ids_outside_the_table(hip, D):
    """L 15, window 7, K 5 (at D 1024 the largest LDS shape the launcher accepts), one group per launch: groups with all 14
    context slots, walks with -1 and N as centre and as context, a row of -1, an alias table that points outside [0, N)."""
    walks, tables, launches, (w_in0, w_out0), r64, r32 = gr.sgns_window_case(D)
    g_in, g_out = torch.from_numpy(w_in0).cuda(), torch.from_numpy(w_out0).cuda()
    g_walks, g_loss = torch.from_numpy(walks).cuda(), torch.zeros(len(launches), 2, device="cuda")
    dev = [_dev(thr, idx) for thr, idx in tables]
    for i, (k, w, t) in enumerate(launches):
        sgns_step(hip, g_walks, w, w + 1, t, t + 1, g_in, g_out, gr.SGNS_WINDOW, gr.SGNS_WINDOW_K, dev[k][0], dev[k][1],
                  gr.SGNS_WINDOW_LR, gr.SGNS_WINDOW_SEED, g_loss[i])
    loss = g_loss.cpu().numpy()
    k_in, k_out = g_in.cpu().numpy(), g_out.cpu().numpy()
    counts = loss[:, 1].astype(np.int64).tolist()
    print(f"GRAPH sgns window D={D}: counts kernel {counts}")
    assert counts == r64[3] == r32[3]
    assert (loss[np.array(r64[3]) == 0, 0] == 0).all()                     # a skipped group adds nothing to its loss slot
    for got, ref, init in ((k_in, r64[0], w_in0), (k_out, r64[1], w_out0)):
        still = (ref == init).all(axis=1)
        assert _same_bits(got[still], init[still])
    gr.compare(f"sgns window D={D}", gr.SGNS_NAMES, (k_in, k_out, loss[:, 0]), r64[:3], r32[:3])


# ------------------------------------------------------------------------------------------------ TransE: grid stride
def test_transe_launch_beyond_the_grid_cap_is_bit_exact(hip):
    """cap + 400 groups on 50 entities in ONE launch, norm 1, tables on a grid of eighths, lr 2^-13, a margin at which every
    term is active, an order with entries outside [0, n) among its first cap: no x can change sign (asserted for any
    interleaving), so the tables must be BIT-EQUAL to the sequential restatement; with lr = 0 the loss sum is exact."""
    cap = gr.geometry()["transe_cap"]
    ent0, rel0, triples, order = gr.transe_stride_problem()
    g_tri, g_order = torch.from_numpy(triples).cuda(), torch.from_numpy(order).cuda()

    def launch(lo, hi, lr):
        g_ent, g_rel, g_loss = torch.from_numpy(ent0).cuda(), torch.from_numpy(rel0).cuda(), torch.zeros(2, device="cuda")
        transe_step(hip, g_ent, g_rel, g_tri, g_order, lo, hi, 1, 1, gr.TRANSE_STRIDE_MARGIN, lr, gr.TRANSE_STRIDE_SEED,
                    gr.TRANSE_STRIDE_EPOCH, g_loss)
        return g_ent.cpu().numpy(), g_rel.cpu().numpy(), g_loss.cpu().numpy()

    for lo, hi in gr.transe_stride_ranges():
        assert hi - lo > cap, "transe stride: the launcher's cap changed and this range no longer exceeds it"
        r_ent, r_rel, (still_loss, still_count), count, f = gr.transe_sign_safety(lo, hi)
        assert f["slack"] > 0 and f["margin"] > f["d_max"] and f["on_grid"] and f["largest"] < 8 and f["moved"]
        assert f["loss_units"] == int(f["loss_units"]) and f["loss_units"] < 2 ** 24 and f["skipped_groups"] >= 4
        k_ent, k_rel, k_loss = launch(lo, hi, 0.0)
        print(f"GRAPH transe stride [{lo},{hi}) lr 0: loss sum kernel {float(k_loss[0])!r} restatement {still_loss!r}, count "
              f"{int(k_loss[1])} / {still_count}")
        assert float(k_loss[0]) == still_loss and int(k_loss[1]) == still_count
        assert _same_bits(k_ent, ent0) and _same_bits(k_rel, rel0)
        k_ent, k_rel, k_loss = launch(lo, hi, gr.TRANSE_STRIDE_LR)
        print(f"GRAPH transe stride [{lo},{hi}) lr 2^-13: max |ent - restatement| {np.abs(k_ent - r_ent).max():.3e}, rel "
              f"{np.abs(k_rel - r_rel).max():.3e}, count {int(k_loss[1])} / {count}")
        assert _same_bits(k_ent, r_ent) and _same_bits(k_rel, r_rel)
        assert int(k_loss[1]) == count


def test_normalize_beyond_the_grid_cap(hip):
    """cap + 300 rows, D 64, ld 80: every wavefront below 300 has two rows; some of those skip their first (norm < 1e-12)."""
    cap = gr.geometry()["normalize_cap"]
    full, lo, hi, r64, r32 = gr.normalize_case()
    D = gr.NORMALIZE_D
    assert hi - lo > cap, "normalize: the launcher's cap changed and the range no longer exceeds it"
    t = torch.from_numpy(full).cuda()
    hip.call("stonk_rows_l2_normalize", hip.ptr(t), full.shape[1], lo, hi, D, hip.stream_ptr())
    got = t.cpu().numpy()
    gr.compare("normalize stride", ("rows",), (got[:, :D],), (r64,), (r32,))
    assert _same_bits(got[:, D:], full[:, D:])
    assert _same_bits(got[:lo], full[:lo]) and _same_bits(got[hi:], full[hi:])
    tiny = lo + 7 * np.arange(40)
    assert _same_bits(got[tiny], full[tiny])
    assert np.abs(np.linalg.norm(got[lo + cap:hi, :D].astype(np.float64), axis=1) - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------------ TransE: skips, zeros
@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D", [64, 1024])
def test_transe_skipped_groups_and_zero_x(hip, D, norm):
    """One group per launch, each from the initial tables: x_p = 0 (h + r == t; h == t with a zero relation row), a
    negative with x_j = 0 on either side - sign(0) = 0, and G = 0 below the 1e-12 threshold -, ids and order entries
    outside their range (nothing changes, the count is 0)."""
    ent0, rel0, triples, order, margin, launches, r64, r32, logs = gr.transe_zero_case(D, norm)
    assert logs[0] == logs[1], "the fp32 and fp64 restatements took different decisions"
    m_ent, m_rel = torch.from_numpy(ent0).cuda(), torch.from_numpy(rel0).cuda()
    g_tri, g_order = torch.from_numpy(triples).cuda(), torch.from_numpy(order).cuda()
    g_loss = torch.zeros(len(launches), 2, device="cuda")
    ents, rels = [], []
    for i, (g, epoch) in enumerate(launches):
        g_ent, g_rel = m_ent.clone(), m_rel.clone()
        transe_step(hip, g_ent, g_rel, g_tri, g_order, g, g + 1, gr.TRANSE_ZERO_K, norm, margin, gr.TRANSE_ZERO_LR,
                    gr.TRANSE_ZERO_SEED, epoch, g_loss[i])
        ents.append(g_ent)
        rels.append(g_rel)
    k_ent, k_rel, loss = torch.stack(ents).cpu().numpy(), torch.stack(rels).cpu().numpy(), g_loss.cpu().numpy()
    counts = loss[:, 1].astype(np.int64).tolist()
    print(f"GRAPH transe zeros D={D} norm={norm}: counts kernel {counts}")
    assert counts == r64[3] == r32[3]
    assert np.isfinite(k_ent).all() and np.isfinite(k_rel).all()
    skipped = np.array([signs is None for _, _, signs, _ in logs[0]])
    assert skipped.sum() == 7 * gr.TRANSE_ZERO_EPOCHS and (np.array(counts)[skipped] == 0).all()
    assert (loss[skipped, 0] == 0).all()
    for got, ref, init in ((k_ent, r64[0], ent0), (k_rel, r64[1], rel0)):
        still = (ref == init[None]).all(axis=2)                            # rows the restatement leaves alone: the same bits
        assert still[skipped].all()
        assert _same_bits(got[still], np.broadcast_to(init[None], got.shape)[still])
    gr.compare(f"transe zeros D={D} norm={norm}", gr.TRANSE_NAMES, (k_ent, k_rel, loss[:, 0]), r64[:3], r32[:3])


# ------------------------------------------------------------------------------------------------ ranks
@pytest.mark.parametrize("n_q", [1, 17])
def test_rank_counts_with_the_candidate_split_at_its_cap(hip, n_q):
    """N_e 70001, D 64: one or two query tiles, so the launcher asks for 2048 / 1024 slices and the cap of 1024 holds; the
    counts of all slices meet by integer atomics and must equal integer arithmetic on the grid's numerators."""
    assert gr.rank_split(n_q, gr.RANK_BIG_NE) == gr.geometry()["rank_split_cap"]
    ek, rk, queries = gr.rank_big_case()
    queries = queries[:n_q]
    d_ent = torch.from_numpy((ek / 8.0).astype(np.float32)).cuda()
    d_rel = torch.from_numpy((rk / 8.0).astype(np.float32)).cuda()
    for side in (0, 1):
        for norm in (1, 2):
            want = integer_counts(ek, rk, queries, side, norm)
            got = tr.transe_rank(d_ent, d_rel, queries, side, norm)
            print(f"GRAPH rank split Q={n_q} side {side} norm {norm}: less {got[0][:4].tolist()} equal {got[1][:4].tolist()}")
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (side, norm, got, want)
            assert (want[1][:min(n_q, 4)] >= 2).all()                      # the planted duplicates, from other slices


@pytest.mark.parametrize("D", [64, 1024])
def test_rank_candidate_lists_with_clamped_pointers(hip, D):
    """cand_ptr[0] = -4 and cand_ptr[Q] = n_cand + 16 (the allocation is that long): the lists counted are the clamped ones.
    D 1024: candidate lists on the path that raises the dynamic-LDS attribute."""
    ek, rk, queries, ptr, cand, n_cand, clamped = gr.rank_clamp_case(D)
    assert (gr.rank_lds_bytes(D) > gr.geometry()["rank_lds_static_limit"]) == (D == 1024)
    assert ptr[0] < 0 and ptr[-1] > n_cand and len(cand) == ptr[-1] and ptr[-3] < n_cand < ptr[-2] < ptr[-1]
    d_ent = torch.from_numpy((ek / 8.0).astype(np.float32)).cuda()
    d_rel = torch.from_numpy((rk / 8.0).astype(np.float32)).cuda()
    d_q, d_ptr, d_cand = torch.from_numpy(queries).cuda(), torch.from_numpy(ptr).cuda(), torch.from_numpy(cand).cuda()
    for side in (0, 1):
        for norm in (1, 2):
            less = torch.full((len(queries),), -7, dtype=torch.int32, device="cuda")
            equal = torch.full((len(queries),), -7, dtype=torch.int32, device="cuda")
            hip.call("stonk_transe_rank", hip.ptr(d_ent), hip.ptr(d_rel), len(ek), len(rk), D, norm, hip.ptr(d_q), len(queries),
                     side, hip.ptr(d_ptr), hip.ptr(d_cand), n_cand, hip.ptr(less), hip.ptr(equal), hip.stream_ptr())
            want = integer_counts(ek, rk, queries, side, norm, clamped, cand)
            got = less.cpu().numpy(), equal.cpu().numpy()
            print(f"GRAPH rank clamps D={D} side {side} norm {norm}: less {got[0].tolist()}")
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (side, norm, got, want)
            assert want[0][9] == -1 and want[0][16] == want[1][16] == 0    # the last list lies wholly beyond n_cand
            unclamped = integer_counts(ek, rk, queries, side, norm, np.maximum(ptr, 0), cand)
            assert not (np.array_equal(unclamped[0], want[0]) and np.array_equal(unclamped[1], want[1]))


# ------------------------------------------------------------------------------------------------ link prediction
def _linkpred_launch(hip, D):
    """The case of one D: (scores, partials) of two launches, and both restatements."""
    emb, pairs, y, w, b, r64, r32 = linkpred_case(D, gr.LINKPRED_N, "bad")
    wide = torch.full((emb.shape[0], D + gr.LINKPRED_PAD), float("nan"), device="cuda")
    wide[:, :D] = torch.from_numpy(emb).cuda()
    g_emb = wide[:, :D]
    g_pairs, g_y, g_w = (torch.from_numpy(v).cuda() for v in (pairs, y, w))
    out = []
    for _ in range(2):
        sc = torch.full((gr.LINKPRED_N,), -7.0, device="cuda")
        pt = torch.full((_rows(hip), D + 2), float("nan"), device="cuda")
        hip.call("stonk_linkpred_lossgrad", hip.ptr(g_emb), g_emb.stride(0), emb.shape[0], D, hip.ptr(g_pairs), hip.ptr(g_y),
                 gr.LINKPRED_N, hip.ptr(g_w), b, hip.ptr(sc), hip.ptr(pt), hip.stream_ptr())
        out.append((sc, pt))
    return out, r64, r32


@pytest.mark.parametrize("D", gr.LINKPRED_DS)
def test_linkpred_every_instantiation(hip, D):
    """linkpred_kernel<NF> for NF = D / 64 = 1 .. 16: n 1000, two pairs outside [0, N) (NaN scores, nothing added), a table
    with ld = D + 64 in a NaN-filled allocation; the scores and the D sums of g x by the rule, two launches bit for bit."""
    assert D // 64 in gr.geometry()["linkpred_nf"]
    ((sc, pt), (sc2, pt2)), r64, r32 = _linkpred_launch(hip, D)
    assert np.isnan(r64[0]).sum() == 2 and torch.isfinite(pt).all()
    gr.compare(f"linkpred NF={D // 64}", ("scores", "sum g x"), (sc.cpu().numpy(), _totals(pt, D)[0]), r64[:2], r32[:2])
    assert torch.equal(pt, pt2) and torch.equal(sc.view(torch.int32), sc2.view(torch.int32))


def test_linkpred_scalar_sums_of_all_instantiations(hip):
    """sum g and sum loss are one number per launch; the sixteen launches' numbers are judged as two arrays of sixteen."""
    got, r64, r32 = [[], []], [[], []], [[], []]
    for D in gr.LINKPRED_DS:
        ((_, pt), _), a, b = _linkpred_launch(hip, D)
        t = _totals(pt, D)
        for k in range(2):
            got[k].append(float(t[1 + k]))
            r64[k].append(float(a[2 + k]))
            r32[k].append(float(b[2 + k]))
    gr.compare("linkpred NF=1..16", ("sum g", "sum loss"), got, r64, r32)


# ------------------------------------------------------------------------------------------------ KG baseline: pooling
@pytest.mark.parametrize("D,L", gr.POOL_CASES)
def test_pooling_instantiations_two_and_four(hip, D, L):
    """walk_maxpool_kernel<2> (D 320: 16 lanes in the second register set; 512) and <4> (832: 16 lanes in the fourth; 1024),
    L 2 and 4: bit-exact against torch.max inside sentinel-filled strides."""
    assert gr.pool_nv(D) in (2, 4) and gr.pool_nv(D) in gr.geometry()["pool_nv"]
    n, N = 37, 50
    rng = np.random.RandomState(L * 1000 + D)
    table = (-np.abs(rng.randn(N, D)) - 0.05).astype(np.float32)
    table[::7] = np.abs(table[::7])
    ids = rng.randint(0, N, (n, L)).astype(np.int32)
    ids[rng.rand(n, L) < 0.1] = -1
    ids[5] = -1
    ids[6] = rng.choice(np.flatnonzero(np.arange(N) % 7), L)
    x = torch.cat([torch.from_numpy(table), torch.zeros(1, D)])[torch.from_numpy(np.where(ids < 0, N, ids)).long()]
    want = torch.max(x, dim=1).values.numpy()
    assert (want[5] == 0).all() and (want[6] < 0).all()
    got, errors = _pool_call(hip, ids, table, L + 3, D + 4, D + 8)
    assert errors == 0
    assert got[:, :D].tobytes() == want.tobytes()
    assert (got[:, D:] == -77.0).all()


# ------------------------------------------------------------------------------------------------ KG baseline: training
def _kgb_compare(tag, tr_, losses, pooled, labels, orders, weights, biases, cws, p):
    got = [np.concatenate(losses)] + _state(tr_)
    r64 = gr.kgb_restated(pooled, labels, orders, weights, biases, cws, p, torch.float64)
    r32 = gr.kgb_restated(pooled, labels, orders, weights, biases, cws, p, torch.float32)
    gr.compare(tag, gr.KGB_NAMES, got, r64, r32)


@pytest.mark.parametrize("name", sorted(gr.KGB_TRAIN_CASES))
def test_kgb_training_shapes(hip, name):
    """The shapes of graph_ref.KGB_TRAIN_CASES, several runs per launch."""
    pooled, labels, weights, biases, cws, orders, batch, p = gr.kgb_case(name)
    t = _trainer(pooled, labels, weights, biases, cws, p)
    losses = t.run_spans([o.reshape(-1) for o in orders], batch)
    t.check_errors()
    _kgb_compare(f"kgb {name}", t, losses, pooled, labels, orders, weights, biases, cws, p)


def test_kgb_pooled_rows_with_a_stride(hip):
    """`pooled` as a view of a wider NaN-filled allocation (ld_pooled = D + 72): the same bits as from a dense copy."""
    pooled, labels, weights, biases, cws, orders, batch, p = gr.kgb_case("stride")
    D = pooled.shape[1]
    wide = torch.full((len(pooled), D + gr.KGB_STRIDE_PAD), float("nan"), device="cuda")
    wide[:, :D] = torch.from_numpy(pooled).cuda()
    view = wide[:, :D]
    assert view.stride(0) == D + gr.KGB_STRIDE_PAD
    t = kgb.KGBTrainer(view, labels, weights, biases, cws, 1e-3, p, seed=11)
    losses = t.run_spans([o.reshape(-1) for o in orders], batch)
    t.check_errors()
    _kgb_compare("kgb stride", t, losses, pooled, labels, orders, weights, biases, cws, p)
    dense = _trainer(pooled, labels, weights, biases, cws, p)
    l2 = dense.run_spans([o.reshape(-1) for o in orders], batch)
    for a, b in zip(losses + _state(t), l2 + _state(dense)):
        assert a.tobytes() == b.tobytes()


def test_kgb_span_of_max_steps_and_one_more(hip):
    """max_steps() + 1 steps in two launches: against the restatement, and bit-equal cut as max_steps(), 1 and 1, max_steps()."""
    D, C, batch, runs, p = gr.KGB_SPAN_CASE
    cap = kgb.max_steps()
    assert cap == gr.geometry()["kgb_max_steps"]
    pooled, labels, weights, biases, cws = gr.kgb_runs(D, C, runs, seed=3)
    orders = gr.kgb_orders(2, len(pooled), cap + 1, batch, runs, ragged_to=5)
    a = _trainer(pooled, labels, weights, biases, cws, p)
    la, sa = _walk(a, orders, [cap, 1], batch)
    assert a.steps_done == [cap + 1] * runs
    got = [np.concatenate(la)] + sa
    r64 = gr.kgb_restated(pooled, labels, orders, weights, biases, cws, p, torch.float64)
    r32 = gr.kgb_restated(pooled, labels, orders, weights, biases, cws, p, torch.float32)
    gr.compare(f"kgb span {cap} + 1", gr.KGB_NAMES, got, r64, r32)
    lb, sb = _walk(_trainer(pooled, labels, weights, biases, cws, p), orders, [1, cap], batch)
    for x, y in zip(la + sa, lb + sb):
        assert x.tobytes() == y.tobytes()


def test_kgb_all_padding_step_in_the_middle_of_a_span(hip):
    """Step 2 of 5 is all padding: its loss is NaN, nothing is updated, and steps 3 and 4 use the global step number that
    counts it - bit for bit a trainer that walked steps 0 .. 1, had its step counter advanced by one, and walked 3 .. 4."""
    pooled, labels, weights, biases, cws, orders, batch, p = gr.kgb_padding_case()
    s = gr.KGB_PADDING_STEP
    a = _trainer(pooled, labels, weights, biases, cws, p)
    la = a.run_spans([o.reshape(-1) for o in orders], batch)
    a.check_errors()
    assert all(np.isnan(l[s]) and np.isfinite(np.delete(l, s)).all() for l in la)
    b = _trainer(pooled, labels, weights, biases, cws, p)
    lb0 = b.run_spans([o[:s].reshape(-1) for o in orders], batch)
    b.steps_done = [d + 1 for d in b.steps_done]
    lb1 = b.run_spans([o[s + 1:].reshape(-1) for o in orders], batch)
    for x, y in zip(_state(a), _state(b)):
        assert x.tobytes() == y.tobytes()
    for l, l0, l1 in zip(la, lb0, lb1):
        assert np.delete(l, s).tobytes() == np.concatenate([l0, l1]).tobytes()
    _kgb_compare("kgb all-padding step", a, la, pooled, labels, orders, weights, biases, cws, p)


# ------------------------------------------------------------------------------------------------ KG baseline: prediction
@pytest.mark.parametrize("D,C", gr.KGB_PREDICT_CASES)
def test_kgb_predict_with_indices_outside_the_dataset(hip, D, C):
    """Indices -1, n, n + 5, INT32_MIN and INT32_MAX among valid ones, ld_pooled = D + 40: NaN probabilities and pred -1 for
    those, the error counter at their number, every other example as the restatement."""
    pooled, labels, weights, biases, _ = gr.kgb_runs(D, C, 1, n=50, seed=8)
    weights[0] *= 4
    n = len(pooled)
    idx = np.random.RandomState(9).permutation(n)[:37].astype(np.int32)
    bad_at = np.array([0, 7, 18, 30, 36])
    idx[bad_at] = [-1, n, n + 5, -2 ** 31, 2 ** 31 - 1]
    ok = np.ones(len(idx), dtype=bool)
    ok[bad_at] = False
    wide = torch.full((n, D + gr.KGB_PREDICT_PAD), float("nan"), device="cuda")
    wide[:, :D] = torch.from_numpy(pooled).cuda()
    d_idx, d_w, d_b = torch.from_numpy(idx).cuda(), torch.from_numpy(weights[0]).cuda(), torch.from_numpy(biases[0]).cuda()
    probs = torch.full((len(idx), C), -7.0, device="cuda")
    pred = torch.full((len(idx),), -7, dtype=torch.int32, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.call("stonk_kgb_predict", hip.ptr(wide), wide.stride(0), n, D, hip.ptr(d_idx), len(idx), hip.ptr(d_w), hip.ptr(d_b), C,
             hip.ptr(probs), hip.ptr(pred), hip.ptr(errors), hip.stream_ptr())
    probs, pred = probs.cpu().numpy(), pred.cpu().numpy()
    assert int(errors.item()) == len(bad_at)
    assert np.isnan(probs[~ok]).all() and (pred[~ok] == -1).all()
    refs = []
    for dtype in (torch.float64, torch.float32):
        with torch.no_grad():
            refs.append(Restatement(weights[0], biases[0], np.ones(C), dtype=dtype).forward(pooled[idx[ok]]).double().numpy())
    gr.compare(f"kgb predict D{D} C{C}", ("probabilities",), [probs[ok]], [refs[0]], [refs[1]])
    top = np.sort(refs[0], axis=1)
    sure = top[:, -1] - top[:, -2] > 1e-5
    print(f"GRAPH kgb predict D{D} C{C}: {int((~sure).sum())} of {len(sure)} arg-maxes undecided (gap <= 1e-5)")
    assert (~sure).sum() <= 0.02 * len(sure)
    assert (pred[ok][sure] == refs[0].argmax(1)[sure]).all()
    with pytest.raises(hip.StonkHipError, match="outside"):
        kgb.kgb_predict(wide[:, :D], idx, weights[0], biases[0])
