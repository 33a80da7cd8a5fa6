"""CPU (no GPU): tests/graph_ref.py proves its cases. Every case of tests/test_graph_parity_gpu.py reaches the branch it is
there for - decided by constants read out of the launchers' source lines, so an edited launcher fails here by name - and
a restatement with ONE mistake (a group of the second trip lost, the window's last slot dropped, the skip rule off by one,
sign(0) taken for 1, ...) misses the float64 reference by at least 3x the tolerance the GPU test applies (12x the float32
restatement's own deviation), or by a count, or by a bit where the GPU test asks for bit equality."""
import numpy as np
import pytest
import torch

from tests import graph_ref as gr
from tests.test_link_prediction_cpu import lossgrad_ref
from tests.test_node2vec_cpu import SGNS_SALT, _h, group_nodes, sgns_ref


# ------------------------------------------------------------------------------------------------ geometry
def test_launch_constants_are_the_ones_the_cases_were_sized_for():
    g = gr.geometry()
    assert (g["sgns_cap"], g["transe_cap"], g["normalize_cap"]) == (4096, 4096, 8192)
    assert (g["rank_qt"], g["rank_target"], g["rank_rows_per_slice"], g["rank_split_cap"]) == (16, 2048, 64, 1024)
    assert g["linkpred_nf"] == list(range(1, 17)) and g["pool_nv"] == [1, 2, 3, 4]
    assert g["kgb_chain"] == [(2, 2), (4, 4), (8, 8), (16, 16)]
    assert (g["kgb_threads"], g["kgb_cols"], g["kgb_chunk"], g["kgb_max_batch"], g["kgb_max_steps"]) == (256, 4, 8, 64, 256)


# ------------------------------------------------------------------------------------------------ skip-gram restatement
def test_sgns_restatement_skips_ids_outside_the_table():
    """node2vec.hip's header: a centre outside [0, N) skips the group, a context outside it the pair, an alias target
    outside it that noise node."""
    n, window, K, seed = 10, 3, 6, 5
    seedkey = _h(seed ^ SGNS_SALT)
    walks = np.array([[1, -1, 2, n, 3], [4, 5, -1, 6, 7], [4, 5, n, 6, 7], [-1, -1, 8, -1, n]], dtype=np.int32)
    thr = np.zeros(n, dtype=np.uint32)                                     # threshold 0: the alias is always taken
    inside = np.full(n, 9, dtype=np.int32)
    ctx, tgt = group_nodes(walks, 0, 2, n, window, K, thr, inside, seedkey)
    assert ctx and set(ctx) <= {1, 3} and tgt == [2] + [9] * K
    for idx in (np.full(n, n, dtype=np.int32), np.full(n, -1, dtype=np.int32)):
        assert group_nodes(walks, 0, 2, n, window, K, thr, idx, seedkey) == (ctx, [2])
    assert group_nodes(walks, 1, 2, n, window, K, thr, inside, seedkey) == ([], [])
    assert group_nodes(walks, 2, 2, n, window, K, thr, inside, seedkey) == ([], [])
    assert group_nodes(walks, 3, 2, n, window, K, thr, inside, seedkey) == ([], [8] + [9] * K)     # no context left
    rng = np.random.RandomState(0)
    w_in, w_out = rng.uniform(-.5, .5, (n, 64)), rng.uniform(-.5, .5, (n, 64))
    a, b, loss = w_in.copy(), w_out.copy(), [0.0, 0]
    sgns_ref(walks, a, b, [(1, 2), (2, 2), (3, 2)], window, K, thr, inside, 0.1, seed, loss)
    assert np.array_equal(a, w_in) and np.array_equal(b, w_out) and loss == [0.0, 0]
    sgns_ref(walks, a, b, [(0, 2)], window, K, thr, inside, 0.1, seed, loss)
    assert loss[1] == len(ctx) * (K + 1) and not np.array_equal(a[1], w_in[1]) and np.array_equal(a[0], w_in[0])


# ------------------------------------------------------------------------------------------------ skip-gram: grid stride
def test_sgns_stride_case_takes_two_trips_and_skips_in_the_first():
    cap = gr.geometry()["sgns_cap"]
    walks, (w_in0, _), r64, r32 = gr.sgns_stride_case()
    W, N = len(walks), 2 * len(walks)
    assert W == cap + gr.SGNS_STRIDE_EXTRA
    bad_centre = np.flatnonzero((walks[:, 0] < 0) | (walks[:, 0] >= N))
    bad_context = np.flatnonzero((walks[:, 1] < 0) | (walks[:, 1] >= N))
    assert len(bad_centre) > 100 and len(bad_context) > 50 and {-1, N} <= set(walks[bad_centre, 0].tolist())
    assert (r64[3][bad_centre] == 0).all() and (r64[3][bad_context] == 0).all() and np.array_equal(r64[3], r32[3])
    assert gr.sgns_lds_bytes(64, 3, 0) <= gr.geometry()["sgns_lds_limit"]
    for lo, hi in gr.sgns_stride_ranges():
        n = hi - lo
        assert n > cap and gr.trips(n, cap) == 2, "sgns stride: the cap changed and the case no longer exceeds it"
        # wavefront b = w - lo skips group b (trip 1) and has group b + cap (trip 2), a valid one
        for bad in (bad_centre, bad_context):
            second = bad[(bad >= lo) & (bad - lo + cap < n)] + cap
            assert (len(second) >= 20 or n - cap < 300) and (r64[3][second] == 1).all(), (lo, hi)
        e64, e32 = gr.sgns_stride_expected(lo, hi, 0), gr.sgns_stride_expected(lo, hi, 1)
        assert e64[3] == e32[3] == n - len(set(bad_centre[(bad_centre >= lo) & (bad_centre < hi)]) |
                                           set(bad_context[(bad_context >= lo) & (bad_context < hi)]))
        for wrong in ("trip2", "stride"):
            w32 = gr.sgns_stride_expected(lo, hi, 1, wrong)
            assert gr.told_apart(("W_in", "W_out"), w32[:2], e64[:2], e32[:2]), (lo, hi, wrong)
        lost = gr.sgns_stride_expected(lo, hi, 1, "trip2")
        bound = gr.sgns_stride_loss_bound(e64[3], e64[2])
        assert lost[3] < e64[3] and abs(e32[2] - e64[2]) < bound / 50
        assert abs(lost[2] - e64[2]) > 3 * bound or n - cap < 300         # (one lost group: the count says so)
        still_in, still_out = gr.sgns_stride_untouched(lo, hi)
        assert still_in[:2 * lo].all() and still_in[2 * hi:].all() and still_out[2 * bad_centre[bad_centre >= lo][0]]


# ------------------------------------------------------------------------------------------------ skip-gram: window, ids
def test_sgns_window_case_fills_every_context_slot_and_meets_every_kind_of_id():
    facts = gr.sgns_window_facts()
    walks, tables = gr.sgns_window_inputs()
    n, window = gr.SGNS_WINDOW_N, gr.SGNS_WINDOW
    full = [(k, w, t) for k, w, t, b, ctx, _, _ in facts if b == window and len(ctx) == 2 * window]
    assert {(0, 0, 7), (0, 1, 7)} <= set(full)                             # b == window and nctx == 2 * window
    assert any(b == window and w == 2 and 0 < len(ctx) < 2 * window for _, w, _, b, ctx, _, _ in facts)   # invalid pairs inside
    assert gr.sgns_lds_bytes(1024, window, gr.SGNS_WINDOW_K) <= gr.geometry()["sgns_lds_limit"] < \
        gr.sgns_lds_bytes(1024, window + 1, gr.SGNS_WINDOW_K)              # the largest shape the launcher accepts
    assert set(walks[3, 6:9].tolist()) == {-1, n, n - 1} and (walks[4] == -1).all()
    by = {(k, w, t): (ctx, tgt, lost) for k, w, t, _, ctx, tgt, lost in facts}
    assert by[(0, 3, 6)][:2] == ([], []) and by[(0, 3, 7)][:2] == ([], []) and by[(0, 3, 8)][1][0] == n - 1
    assert all(by[(k, 4, t)][:2] == ([], []) for k in (0, 1) for t in gr.SGNS_WINDOW_POSITIONS)
    assert {-1, n} <= set(walks[2].tolist()) and all(0 <= x < n for v in by.values() for x in v[0] + v[1])
    assert any(n - 1 in by[(0, 5, t)][0] for t in gr.SGNS_WINDOW_POSITIONS)
    assert sum(lost for k, *_, lost in facts if k == 1) >= 10 and not any(lost for k, *_, lost in facts if k == 0)
    assert {-1, n} <= set(tables[1][1].tolist())
    for D in (64, 1024):
        _, _, launches, (w_in0, w_out0), r64, r32 = gr.sgns_window_case(D)
        assert r64[3] == r32[3] and r64[3].count(0) == 2 * (2 + 3) and max(r64[3]) == 2 * window * (gr.SGNS_WINDOW_K + 1)
        assert np.abs(r64[0] - w_in0).max() > 1e-3 and np.abs(r64[1] - w_out0).max() > 1e-3
        for wrong in gr.SGNS_WRONG:
            m = gr.sgns_window_case(D, wrong)[5]
            assert gr.told_apart(gr.SGNS_NAMES, m[:3], r64[:3], r32[:3]), (D, wrong)


# ------------------------------------------------------------------------------------------------ TransE: grid stride
def test_transe_stride_case_is_sign_safe_and_exact():
    cap = gr.geometry()["transe_cap"]
    ent0, rel0, triples, order = gr.transe_stride_problem()
    n = len(triples)
    assert n == cap + gr.TRANSE_STRIDE_EXTRA and len(order) == n
    bad = np.flatnonzero((order < 0) | (order >= n))
    assert len(bad) == 4                                                  # (their wavefronts have a second group: below)
    for lo, hi in gr.transe_stride_ranges():
        assert hi - lo > cap and gr.trips(hi - lo, cap) == 2
        assert all(lo <= g and g - lo + cap < hi for g in bad)
        ent, rel, (loss, count), count_lr, f = gr.transe_sign_safety(lo, hi)
        print(f"transe stride [{lo},{hi}): {f}")
        assert f["slack"] > 0 and f["margin"] > f["d_max"]                 # no sign flip in any interleaving; every term active
        assert f["on_grid"] and f["largest"] < 8 and f["moved"]            # multiples of lr below 8: every add exact in fp32
        assert f["loss_units"] == int(f["loss_units"]) and f["loss_units"] < 2 ** 24 and count == count_lr
        assert f["skipped_groups"] == 6                                    # four order entries, two triples with an id outside
        assert float(np.float32(loss)) == loss
        lost = gr.transe_sign_safety(lo, hi, "trip2")
        assert not np.array_equal(lost[0], ent) and not np.array_equal(lost[1], rel) and lost[2] != (loss, count)


def test_normalize_stride_case():
    cap = gr.geometry()["normalize_cap"]
    full, lo, hi, r64, r32 = gr.normalize_case()
    assert hi - lo == cap + gr.NORMALIZE_EXTRA and gr.trips(hi - lo, cap) == 2 and full.shape == (hi + 5, gr.NORMALIZE_LD)
    tiny = lo + 7 * np.arange(40)
    assert np.array_equal(r64[tiny], full[tiny, :64]) and (tiny + cap < hi).all()
    assert np.abs(np.linalg.norm(r64[tiny + cap], axis=1) - 1).max() < 1e-12
    _, _, _, w64, w32 = gr.normalize_case("trip2")
    assert gr.told_apart(("rows",), (w32,), (r64,), (r32,))


# ------------------------------------------------------------------------------------------------ TransE: skips, zeros
@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D", [64, 1024])
def test_transe_zero_case_meets_every_kind(D, norm):
    ent0, rel0, triples, order, margin, launches, r64, r32, logs = gr.transe_zero_case(D, norm)
    assert logs[0] == logs[1] and r64[3] == r32[3]
    ek = np.round(ent0 * 8).astype(np.int64)
    assert (ek == ent0 * 8).all() and np.array_equal(ent0[0] + rel0[0], ent0[1]) and not rel0[1].any()
    f = gr.transe_zero_facts(D, norm)
    print(f"transe zeros D={D} norm={norm}: margin {margin} {f}")
    assert f["skip_order"] == 3 * gr.TRANSE_ZERO_EPOCHS and f["skip_id"] == 4 * gr.TRANSE_ZERO_EPOCHS
    assert f["xp_zero_active"] >= 4 and f["xj_zero_tail"] >= 2 and f["xj_zero_head"] >= 2
    assert f["active"] >= 10 and f["inactive"] >= 10 and f["same"] >= 4
    assert np.isfinite(r64[0]).all() and np.isfinite(r32[0]).all()
    wrongs = ("sign0", "order") if norm == 1 else ("eps", "order")
    for wrong in wrongs:
        m = gr.transe_zero_case(D, norm, wrong)[7]
        assert m[3] != r64[3] or gr.told_apart(gr.TRANSE_NAMES, m[:3], r64[:3], r32[:3]), wrong
    assert gr.transe_zero_case(D, norm, "order")[7][3] != r64[3]


# ------------------------------------------------------------------------------------------------ ranks
def test_rank_cases_reach_the_split_cap_and_the_clamps():
    from tests.test_transe_rank_gpu import integer_counts

    g = gr.geometry()
    assert gr.rank_split(1, gr.RANK_BIG_NE) == gr.rank_split(17, gr.RANK_BIG_NE) == g["rank_split_cap"] == 1024
    assert gr.rank_split(1, 1000) == 16 and gr.rank_split(1, 65536) == 1024 and gr.rank_split(1, 65536 - 64) == 1023
    assert gr.rank_split(300, gr.RANK_BIG_NE) < 1024
    ek, rk, queries = gr.rank_big_case()
    assert np.abs(ek).max() <= 16 and queries[0].tolist() == [gr.RANK_BIG_NE - 1, 1, 0]
    per_slice = gr.RANK_BIG_NE / 1024
    for h, _, t in queries[:4].tolist():                                   # duplicates in other slices than the originals
        assert abs((t + 35000) % gr.RANK_BIG_NE - t) > 2 * per_slice and np.array_equal(ek[(t + 35000) % gr.RANK_BIG_NE], ek[t])
    assert gr.rank_lds_bytes(1024) > g["rank_lds_static_limit"] >= gr.rank_lds_bytes(960)
    for D in (64, 1024):
        ek, rk, queries, ptr, cand, n_cand, clamped = gr.rank_clamp_case(D)
        assert ptr[0] == -4 and clamped[0] == 0 and ptr[-1] == len(cand) == n_cand + 16 and clamped[-1] == n_cand
        assert ptr[-3] < n_cand < ptr[-2] < ptr[-1]                        # one list cut short, the last cut away
        assert clamped[-3] < clamped[-2] == clamped[-1]
        assert (cand < 0).any() and (cand >= 63).any()
        differs = 0
        for side in (0, 1):
            for norm in (1, 2):
                want = integer_counts(ek, rk, queries, side, norm, clamped, cand)
                loose = integer_counts(ek, rk, queries, side, norm, np.maximum(ptr, 0), cand)
                differs += not (np.array_equal(want[0], loose[0]) and np.array_equal(want[1], loose[1]))
                assert want[0][9] == -1
        assert differs == 4                                                # a kernel without the upper clamp counts otherwise


# ------------------------------------------------------------------------------------------------ link prediction
def test_linkpred_cases_select_every_instantiation():
    from tests.test_link_prediction_gpu import _case

    assert [d // 64 for d in gr.LINKPRED_DS] == gr.geometry()["linkpred_nf"]
    for d in gr.LINKPRED_DS:
        emb, pairs, y, w, b, r64, r32 = _case(d, gr.LINKPRED_N, "bad")
        assert emb.shape == (50, d) and np.isnan(r64[0]).sum() == 2 and np.isnan(r64[0][[5, gr.LINKPRED_N - 1]]).all()
        # a restatement that forgets the last 64 features (an instantiation one too small) is told apart
        cut = np.concatenate([emb[:, :d - 64], np.zeros((50, 64), np.float32)], axis=1)
        short = lossgrad_ref(cut, pairs, y, w, b, np.float32)
        assert gr.told_apart(("scores", "sum g"), (short[0], short[2]), (r64[0], r64[2]), (r32[0], r32[2])), d


# ------------------------------------------------------------------------------------------------ KG baseline
def test_kgb_cases_select_their_instantiations_columns_and_butterflies():
    g = gr.geometry()
    assert [gr.pool_nv(D) for D, _ in gr.POOL_CASES] == [2, 2, 2, 2, 4, 4, 4, 4]
    assert 320 // 4 - 64 == 16 and 832 // 4 - 3 * 64 == 16                 # lanes that carry a chunk in the last register set
    cases = gr.KGB_TRAIN_CASES
    assert [gr.kgb_cm(cases[k][1]) for k in ("d1024", "d320", "d832", "c9", "c12")] == [16, 4, 8, 16, 16]
    assert cases["d320"][1] == 4 and cases["d832"][1] == 8 and cases["d1024"][1] == g["kgb_max_classes"]   # the template filled
    assert gr.kgb_columns(1024) == [256] * 4 and gr.kgb_columns(320) == [256, 64, 0, 0]
    assert gr.kgb_columns(832) == [256, 256, 256, 64] and gr.kgb_columns(192) == [192, 0, 0, 0]
    assert gr.kgb_butterflies(9) == (3, 4, 1) and gr.kgb_butterflies(12) == (3, 4, 4) and gr.kgb_butterflies(16) == (4, 4, 4)
    assert cases["d1024"][2] == g["kgb_max_batch"] and cases["batch1"][2] == 1
    assert cases["batch9"][2] == g["kgb_chunk"] + 1 and cases["batch9"][5] < g["kgb_chunk"]   # (the ragged step: one chunk live)
    assert gr.KGB_STRIDE_CASE[0] + gr.KGB_STRIDE_PAD > gr.KGB_STRIDE_CASE[0]


def _restated_pair(case, wrong=None):
    pooled, labels, weights, biases, cws, orders, batch, p = case
    r64 = gr.kgb_restated(pooled, labels, orders, weights, biases, cws, p, torch.float64)
    r32 = gr.kgb_restated(pooled, labels, orders, weights, biases, cws, p, torch.float32)
    w32 = gr.kgb_restated(pooled, labels, orders, weights, biases, cws, p, torch.float32, wrong=wrong) if wrong else None
    return r64, r32, w32


@pytest.mark.parametrize("name,wrong", [("d1024", "columns"), ("d832", "columns"), ("c9", "classes"), ("c12", "classes")])
def test_kgb_training_cases_tell_a_lost_column_and_a_lost_butterfly_apart(name, wrong):
    r64, r32, w32 = _restated_pair(gr.kgb_case(name), wrong)
    assert np.isfinite(r64[0]).all()
    assert gr.told_apart(gr.KGB_NAMES, w32, r64, r32), (name, wrong)


def test_kgb_all_padding_step_is_restated_and_counted():
    case = gr.kgb_padding_case()
    orders = case[5]
    s = gr.KGB_PADDING_STEP
    assert all((o[s] == -1).all() and (np.delete(o, s, axis=0) >= 0).all() for o in orders) and 0 < s < len(orders[0]) - 1
    r64, r32, w32 = _restated_pair(case, "counter")
    steps = len(orders[0])
    nan = np.isnan(r64[0])
    assert nan.sum() == len(orders) and nan.reshape(len(orders), steps)[:, s].all()
    assert gr.told_apart(gr.KGB_NAMES, w32, r64, r32)                     # a step counter that does not count the step


def test_kgb_predict_case_leaves_few_arg_maxes_undecided():
    from tests.test_kg_baseline_cpu import Restatement

    for D, C in gr.KGB_PREDICT_CASES:
        pooled, _, weights, biases, _ = gr.kgb_runs(D, C, 1, n=50, seed=8)
        idx = np.random.RandomState(9).permutation(50)[:37]
        idx = np.delete(idx, [0, 7, 18, 30, 36])
        with torch.no_grad():
            q = Restatement(weights[0] * 4, biases[0], np.ones(C)).forward(pooled[idx]).numpy()
        top = np.sort(q, axis=1)
        undecided = (top[:, -1] - top[:, -2] <= 1e-5).sum()
        assert undecided <= 0.02 * len(idx), (D, C, undecided)            # the cap of test_kg_baseline_gpu.py: 2 %
