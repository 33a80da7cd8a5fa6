"""KG baseline on the GPU: stonk_walk_maxpool, stonk_kgb_train_steps and stonk_kgb_predict against the torch restatement of
tests/test_kg_baseline_cpu.py, and the cross-validation driver end to end through TSV files.

Tolerances follow tests/test_sgns_gpu.py::_compare: per quantity, the kernel may deviate from the fp64 restatement by 4x
what the fp32 restatement deviates from it on the same inputs. So that a quantity is never a single number (one fp32 result
can land on its fp64 value by luck), every step test walks several runs in one launch and compares the runs' values as one
array. Figures measured with this file are in profiles/kg_baseline.md."""
import logging
import os

import numpy as np
import pytest
import torch

from stonkgs_amd import kg_baseline_model as kgb
from stonkgs_amd.stonkgs_finetuning import get_train_test_splits, weighted_f1_score
from stonkgs_amd.stonkgs_model import prepare_df
from tests.test_kg_baseline_cpu import Restatement, pool_restated, train_restated

pytestmark = pytest.mark.gpu
NAMES = ("loss", "W", "b", "mW", "vW", "mb", "vb")


def _compare(tag, got, ref64, ref32, names=NAMES):
    rows = []
    for name, g, r64, r32 in zip(names, got, ref64, ref32):
        fmt = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max())
        ker = float(np.abs(np.asarray(g, dtype=np.float64) - r64).max())
        print(f"{tag} {name}: fp32-torch {fmt:.3e}  kernel {ker:.3e}  allowed {4 * fmt:.3e}")
        rows.append((name, ker, fmt))
    for name, ker, fmt in rows:
        assert np.isfinite(ker) and ker <= 4 * fmt, (tag, name, ker, fmt)


def _runs(D, C, R, n=40, seed=0):
    """n pooled rows and labels, and R runs with their own initial weights and unequal class weights."""
    rng = np.random.RandomState(seed)
    pooled = rng.randn(n, D).astype(np.float32)
    labels = rng.randint(0, C, n).astype(np.int32)
    bound = 1 / np.sqrt(D)
    weights = [((rng.rand(C, D) * 2 - 1) * bound).astype(np.float32) for _ in range(R)]
    biases = [((rng.rand(C) * 2 - 1) * bound).astype(np.float32) for _ in range(R)]
    cws = [(1.0 / rng.randint(1, 9, C)).astype(np.float32) for _ in range(R)]
    return pooled, labels, weights, biases, cws


def _orders(rng, n, steps, batch, ragged_to=None):
    order = rng.randint(0, n, (steps, batch)).astype(np.int32)
    if ragged_to is not None:
        order[-1, ragged_to:] = -1
    return order


def _trainer(pooled, labels, weights, biases, cws, p, seed=11, lr=1e-3):
    return kgb.KGBTrainer(torch.from_numpy(pooled).cuda(), labels, weights, biases, cws, lr, p, seed=seed)


def _state(tr):
    return [t.cpu().numpy().copy() for t in (tr.W, tr.b, tr.mW, tr.vW, tr.mb, tr.vb)]


def _restated_runs(pooled, labels, orders, weights, biases, cws, p, dtype, seed=11, lr=1e-3):
    losses, states = [], []
    for r, order in enumerate(orders):
        rs, ls = train_restated(pooled, labels, order, weights[r], biases[r], cws[r], lr, seed, r, p, dtype=dtype)
        losses.append(ls)
        states.append(rs.state())
    return [np.concatenate(losses)] + [np.stack([s[k] for s in states]) for k in range(6)]


# ------------------------------------------------------------------------------------------------------------ pooling
def _pool_call(hip, ids, table, ld_ids, ld_table, ld_pooled):
    n, L = ids.shape
    N, D = table.shape
    ids_dev = torch.full((n, ld_ids), 12345, dtype=torch.int32, device="cuda")
    ids_dev[:, :L] = torch.from_numpy(ids).cuda()
    table_dev = torch.full((N, ld_table), 7.0, device="cuda")          # (the padding would win every maximum if it were read)
    table_dev[:, :D] = torch.from_numpy(table).cuda()
    out = torch.full((n, ld_pooled), -77.0, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.call("stonk_walk_maxpool", hip.ptr(ids_dev), ld_ids, n, L, hip.ptr(table_dev), ld_table, N, D, hip.ptr(out), ld_pooled,
             hip.ptr(errors), hip.stream_ptr())
    return out.cpu().numpy(), int(errors.item())


@pytest.mark.parametrize("D", [64, 192, 768])
@pytest.mark.parametrize("L", [1, 3, 5, 254])
def test_pooling_is_bit_exact(hip, L, D):
    n, N = 37, 50
    rng = np.random.RandomState(L * 1000 + D)
    table = (-np.abs(rng.randn(N, D)) - 0.05).astype(np.float32)         # all negative: a -1 id changes the result
    table[::7] = np.abs(table[::7])                                      # (and some rows that beat the null vector)
    ids = rng.randint(0, N, (n, L)).astype(np.int32)
    ids[rng.rand(n, L) < 0.1] = -1
    ids[5] = -1                                                          # an example of only -1
    ids[6] = rng.choice(np.flatnonzero(np.arange(N) % 7), L)             # only negative rows, no -1
    want = np.where((ids >= 0)[:, :, None], table[np.maximum(ids, 0)], np.float32(0)).max(1)
    assert (want[5] == 0).all() and (want[6] < 0).all()
    got, errors = _pool_call(hip, ids, table, L + 3, D + 4, D + 8)
    assert errors == 0
    assert got[:, :D].tobytes() == want.tobytes()
    assert (got[:, D:] == -77.0).all()                                   # nothing outside the rows' D columns is written
    assert got[:, :D].tobytes() == pool_restated(table, ids, torch.float32).numpy().tobytes()
    # one id equal to N: that row NaN, the counter at 1, every other row right
    bad = ids.copy()
    bad[9, L // 2] = N
    got, errors = _pool_call(hip, bad, table, L + 3, D + 4, D + 8)
    assert errors == 1 and np.isnan(got[9, :D]).all()
    keep = np.arange(n) != 9
    assert got[keep, :D].tobytes() == want[keep].tobytes()
    if L == 3 and D == 64:
        with pytest.raises(hip.StonkHipError, match="outside"):
            kgb.walk_maxpool(bad, table)
        assert kgb.walk_maxpool(ids, table).cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("C", [2, 3, 16])
@pytest.mark.parametrize("D", [64, 768])
def test_one_step(hip, D, C, p):
    """Four runs, one step each: two full batches of 8, two ragged batches of 5 (padded with -1)."""
    pooled, labels, weights, biases, cws = _runs(D, C, 4, seed=D + C)
    rng = np.random.RandomState(1)
    orders = [_orders(rng, len(pooled), 1, 8, ragged_to=None if r < 2 else 5) for r in range(4)]
    tr = _trainer(pooled, labels, weights, biases, cws, p)
    losses = tr.run_spans([o.reshape(-1) for o in orders], 8)
    tr.check_errors()
    got = [np.concatenate(losses)] + _state(tr)
    ref64 = _restated_runs(pooled, labels, orders, weights, biases, cws, p, torch.float64)
    ref32 = _restated_runs(pooled, labels, orders, weights, biases, cws, p, torch.float32)
    _compare(f"one step D{D} C{C} p{p}", got, ref64, ref32)


@pytest.mark.parametrize("batch,ragged_to", [(12, 9), (64, 51), (16, None)])
def test_batches_above_one_chunk(hip, batch, ragged_to):
    """Rows are taken eight at a time; above eight they are re-read for the backward pass: a partial second chunk (12, and
    9 live rows of 12), a whole number of chunks (16) and the largest batch (64, 51 live), three steps each, two runs."""
    D, C, p = 192, 5, 0.1
    pooled, labels, weights, biases, cws = _runs(D, C, 2, n=90, seed=batch)
    rng = np.random.RandomState(batch)
    orders = [_orders(rng, len(pooled), 3, batch, ragged_to=ragged_to) for _ in range(2)]
    tr = _trainer(pooled, labels, weights, biases, cws, p)
    losses = tr.run_spans([o.reshape(-1) for o in orders], batch)
    tr.check_errors()
    got = [np.concatenate(losses)] + _state(tr)
    ref64 = _restated_runs(pooled, labels, orders, weights, biases, cws, p, torch.float64)
    ref32 = _restated_runs(pooled, labels, orders, weights, biases, cws, p, torch.float32)
    _compare(f"batch {batch}", got, ref64, ref32)


# ------------------------------------------------------------------------------------------------------------ 25 steps
def _walk(tr, orders, cuts, batch=8):
    """Walk every run's [steps, batch] order in launches of the given step counts; returns (losses per run, state)."""
    losses = [[] for _ in orders]
    lo = 0
    for k in cuts:
        out = tr.run_spans([o[lo:lo + k].reshape(-1) for o in orders], batch)
        for r, l in enumerate(out):
            losses[r].append(l)
        lo += k
    tr.check_errors()
    return [np.concatenate(l) for l in losses], _state(tr)


@pytest.mark.parametrize("D,C,p", [(64, 3, 0.0), (64, 3, 0.1), (768, 16, 0.1)])
def test_25_steps(hip, D, C, p):
    pooled, labels, weights, biases, cws = _runs(D, C, 2, seed=3)
    rng = np.random.RandomState(2)
    orders = [_orders(rng, len(pooled), 25, 8, ragged_to=5) for _ in range(2)]
    losses, state = _walk(_trainer(pooled, labels, weights, biases, cws, p), orders, [25])
    got = [np.concatenate(losses)] + state
    ref64 = _restated_runs(pooled, labels, orders, weights, biases, cws, p, torch.float64)
    ref32 = _restated_runs(pooled, labels, orders, weights, biases, cws, p, torch.float32)
    moved = float(np.abs(ref64[1] - np.stack(weights)).max())
    print(f"25 steps D{D} C{C} p{p}: the weights moved by {moved:.3e}")
    _compare(f"25 steps D{D} C{C} p{p}", got, ref64, ref32)
    # where the span is cut changes no bit, and neither does running it again
    for cuts in ([7, 18], [1] * 25, [25]):
        l2, s2 = _walk(_trainer(pooled, labels, weights, biases, cws, p), orders, cuts)
        for a, b in zip(losses + state, l2 + s2):
            assert a.tobytes() == b.tobytes(), cuts


# ------------------------------------------------------------------------------------------------------------ runs
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_runs_do_not_see_each_other(hip, p):
    """Three runs with (25, 24, 25) steps in one launch: each equals that run walking alone. A run's dropout stream is keyed
    by its run number, so 'alone' keeps the number: the other runs of the launch get no steps. Without dropout the run is
    also compared with a launch of one workgroup."""
    D, C = 192, 5
    pooled, labels, weights, biases, cws = _runs(D, C, 3, seed=4)
    rng = np.random.RandomState(5)
    orders = [_orders(rng, len(pooled), k, 8) for k in (25, 24, 25)]
    tr = _trainer(pooled, labels, weights, biases, cws, p)
    losses = tr.run_spans([o.reshape(-1) for o in orders], 8)
    tr.check_errors()
    state = _state(tr)
    assert [len(l) for l in losses] == [25, 24, 25] and tr.steps_done == [25, 24, 25]
    empty = np.zeros(0, dtype=np.int32)
    for r in range(3):
        alone = _trainer(pooled, labels, weights, biases, cws, p)
        l1 = alone.run_spans([orders[q].reshape(-1) if q == r else empty for q in range(3)], 8)
        assert l1[r].tobytes() == losses[r].tobytes()
        for a, b, init in zip(_state(alone), state, [np.stack(weights), np.stack(biases)] + [None] * 4):
            assert a[r].tobytes() == b[r].tobytes()
            for q in range(3):
                if q != r:                                                # a run without steps is left as it was
                    assert (a[q] == (init[q] if init is not None else 0)).all()
        if p == 0.0:
            single = _trainer(pooled, labels, weights[r:r + 1], biases[r:r + 1], cws[r:r + 1], p)
            l0 = single.run_spans([orders[r].reshape(-1)], 8)
            assert l0[0].tobytes() == losses[r].tobytes()
            for a, b in zip(_state(single), state):
                assert a[0].tobytes() == b[r].tobytes()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_error_flags(hip):
    D, C, n = 64, 3, 40
    pooled, labels, weights, biases, cws = _runs(D, C, 3, seed=6)
    tr = _trainer(pooled, labels, weights, biases, cws, 0.0)
    lib = hip.lib()
    buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")          # stands for every pointer of a refused call
    ptr = hip.ptr(buf)

    def status(D=64, C=3, batch=8, n_steps_max=4, pooled_ptr=ptr, loss_ptr=ptr):
        return lib.stonk_kgb_train_steps(pooled_ptr, D, n, D, ptr, C, 1, ptr, 1 << 30, batch, ptr, ptr, n_steps_max, ptr, ptr,
                                         ptr, ptr, ptr, ptr, ptr, loss_ptr, 1 << 30, ptr, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.0, 1, 0)

    assert status(C=17) == hip.ESHAPE and status(batch=65) == hip.ESHAPE and status(D=96) == hip.ESHAPE
    assert status(n_steps_max=kgb.max_steps() + 1) == hip.ESHAPE
    assert status(pooled_ptr=0) == hip.EINVAL and status(loss_ptr=0) == hip.EINVAL
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0                                      # no refused call wrote anything

    # an order entry of n (run 0) and a label of C (run 1): flagged, and the other rows give what the restatement gives
    # without that row; run 2 is clean
    rng = np.random.RandomState(7)
    orders = [_orders(rng, n, 3, 8) for _ in range(3)]
    for o in orders:
        o[o == 13] = 12                                                   # (example 13 gets the bad label: used once, below)
    orders[0][1, 3] = n
    orders[1][2, 6] = 13
    bad_labels = labels.copy()
    bad_labels[13] = C
    tr = _trainer(pooled, bad_labels, weights, biases, cws, 0.0)
    losses = tr.run_spans([o.reshape(-1) for o in orders], 8)
    assert tr.errors.cpu().tolist() == [1, 1, 0]
    with pytest.raises(hip.StonkHipError, match=r"\[0, 1\]"):
        tr.check_errors()
    clean = [o.copy() for o in orders]
    clean[0][1, 3] = -1
    clean[1][2, 6] = -1
    got = [np.concatenate(losses)] + _state(tr)
    ref64 = _restated_runs(pooled, labels, clean, weights, biases, cws, 0.0, torch.float64)
    ref32 = _restated_runs(pooled, labels, clean, weights, biases, cws, 0.0, torch.float32)
    _compare("refused rows", got, ref64, ref32)


# ------------------------------------------------------------------------------------------------------------ prediction
@pytest.mark.parametrize("D,C", [(64, 3), (768, 16), (1024, 2)])
def test_prediction(hip, D, C):
    pooled, labels, weights, biases, _ = _runs(D, C, 1, n=50, seed=8)
    weights[0] *= 4                                                       # (probabilities away from uniform)
    idx = np.random.RandomState(9).permutation(50)[:37]
    probs, pred = kgb.kgb_predict(torch.from_numpy(pooled).cuda(), idx, weights[0], biases[0])
    refs = []
    for dtype in (torch.float64, torch.float32):
        with torch.no_grad():
            refs.append(Restatement(weights[0], biases[0], np.ones(C), dtype=dtype).forward(pooled[idx]).double().numpy())
    _compare(f"predict D{D} C{C}", [probs], [refs[0]], [refs[1]], names=("probabilities",))
    top = np.sort(refs[0], axis=1)
    sure = top[:, -1] - top[:, -2] > 1e-5
    assert sure.sum() >= 30 and (pred[sure] == refs[0].argmax(1)[sure]).all()
    assert pred.dtype == np.int32 and ((pred >= 0) & (pred < C)).all()
    # a tie goes to the lowest index: two classes with equal rows and biases
    weights[0][C - 1] = weights[0][0]
    biases[0][C - 1] = biases[0][0]
    probs, pred = kgb.kgb_predict(torch.from_numpy(pooled).cuda(), idx, weights[0], biases[0])
    assert (probs[:, 0] == probs[:, C - 1]).all() and (pred != C - 1).all() and (pred == 0).any()


def test_model_forward_and_fit(hip):
    """The class surface: forward on [B, L, D] sequences equals pooling + prediction, fit moves the parameters and
    state_dict has the reference's keys."""
    torch.manual_seed(3)
    emb = {i: np.random.RandomState(i).randn(64) for i in range(20)}
    ds = kgb.TransEINDRAEntityDataset(emb, list(range(0, 12)), ["r"] * 12, list(range(8, 20)), [i % 2 for i in range(12)])
    model = kgb.KGEClassificationModel(2, [0.5, 1.0], d_in=64)
    assert sorted(model.state_dict()) == ["linear.bias", "linear.weight"]
    x = torch.stack([ds[i][0] for i in range(12)])
    probs = model(x)
    assert probs.shape == (12, 2) and (probs.numpy() == model.predict_proba(ds, np.arange(12))).all()
    with torch.no_grad():
        want = torch.softmax(model.linear(torch.max(x, dim=1).values), dim=1)
    assert torch.allclose(probs, want, atol=1e-6)
    before = model.state_dict()
    model.fit(ds, np.arange(10), epochs=2, batch_size=4, seed=1)
    assert len(model.losses) == 6 and np.isfinite(model.losses).all()
    assert (model.state_dict()["linear.weight"] != before["linear.weight"]).any()
    assert model.predict(ds, [10, 11]).shape == (2,)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """60 nodes in 3 clusters of 20, D 64, table = 0.6 * cluster mean + N(0, 0.3^2). Every node's walk is 3 nodes of its own
    cluster. 400 triples: source and target come from the label's cluster for 80 % of them, from anywhere otherwise; the
    first 40 labels are class 0. One walk holds a node without an embedding; two triples have a source without one."""
    root = tmp_path_factory.mktemp("kgb")
    rng = np.random.RandomState(0)
    means = rng.randn(3, 64)
    cluster = np.repeat(np.arange(3), 20)
    table = 0.6 * means[cluster] + 0.3 * rng.randn(60, 64)
    with open(root / "emb.tsv", "w") as f:
        for i in range(60):
            f.write("\t".join([str(i)] + [repr(float(x)) for x in table[i]]) + "\n")
    walks = np.array([rng.choice(np.flatnonzero(cluster == cluster[i]), 3) for i in range(60)])
    walks[17, 1] = 777                                                    # a walk node the table does not have
    with open(root / "walks.tsv", "w") as f:
        for i in range(60):
            f.write("\t".join([str(i)] + [str(x) for x in walks[i]]) + "\n")
    label = rng.randint(0, 3, 400)
    label[:40] = 0
    rows = ["source\ttarget\trelation\tclass"]
    for k in range(400):
        pool = np.flatnonzero(cluster == label[k]) if rng.rand() < 0.8 else np.arange(60)
        s, t = rng.choice(pool, 2)
        if k in (50, 300):
            s = 9000 + k                                                  # a source without an embedding
        rows.append(f"{s}\t{t}\trel{k % 4}\tc{label[k]}")
    (root / "triples.tsv").write_text("\n".join(rows) + "\n")
    return root


def _restated_cv(root, variant, p, epochs=5, batch=8, lr=1e-3, seed=42):
    """The driver's run restated: the same filter, folds, initial weights, epoch orders and masks, trained in fp64."""
    import pandas as pd

    df = pd.read_csv(root / "triples.tsv", sep="\t")
    emb = prepare_df(str(root / "emb.tsv"))
    df, left_out = kgb.filter_triples(df, emb.keys())
    names = sorted(df["class"].unique().tolist())
    labels = np.array([names.index(c) for c in df["class"]], dtype=np.int32)
    splits = get_train_test_splits(df, type_column_name="class", random_seed=seed, n_splits=5)
    row_of, table = kgb.embedding_table(emb)
    if variant == "node2vec":
        ids = kgb.node2vec_id_matrix(row_of, prepare_df(str(root / "walks.tsv")), df["source"], df["target"], 6)
    else:
        ids = kgb.transe_id_matrix(row_of, df["source"], df["relation"], df["target"])
    pooled = pool_restated(table, ids).numpy()
    cws = [kgb.inverse_count_class_weights(labels, s["train_idx"], 3) for s in splits]
    models = kgb.init_fold_models(5, 3, cws, 64, lr, p, seed)
    pred, gap, majority_f1 = {}, {}, []
    for r, s in enumerate(splits):
        steps = np.concatenate([np.concatenate(kgb.cut_epoch(kgb.epoch_order(s["train_idx"], seed, r, e), batch, 1 << 30))
                                for e in range(epochs)]).reshape(-1, batch)
        rs, _ = train_restated(pooled, labels, steps, models[r].linear.weight.detach().numpy(),
                               models[r].linear.bias.detach().numpy(), cws[r], lr, seed, r, p)
        with torch.no_grad():
            q = rs.forward(pooled[s["test_idx"]]).numpy()
        top = np.sort(q, axis=1)
        for i, a, g in zip(s["test_idx"], q.argmax(1), top[:, -1] - top[:, -2]):
            pred[int(i)], gap[int(i)] = names[a], g
        true = labels[s["test_idx"]]
        majority_f1.append(weighted_f1_score(true, np.full_like(true, np.bincount(labels).argmax())))
    return df, left_out, pred, gap, float(np.mean(majority_f1))


@pytest.mark.parametrize("variant,p", [("node2vec", 0.0), ("node2vec", 0.1), ("transe", 0.1)])
def test_cross_validation_end_to_end(hip, planted, tmp_path, caplog, variant, p):
    import pandas as pd

    with caplog.at_level(logging.INFO, logger="stonkgs_amd.kg_baseline_model"):
        result = kgb.run_kg_baseline_classification_cv(
            str(planted / "triples.tsv"), str(planted / "emb.tsv"), str(planted / "walks.tsv"), epochs=5, train_batch_size=8,
            lr=1e-3, task_name="planted_", model_variant=variant, output_dir=str(tmp_path), dropout=p)
    assert sorted(result) == ["f1_score_mean", "f1_score_std"]
    assert "2 out of 400 triples are left out" in caplog.text            # the two filtered triples are reported
    frame = pd.read_csv(os.path.join(tmp_path, "predicted_labels_kg_planted_df.tsv"), sep="\t")
    assert list(frame.columns) == ["split", "index", "predicted_label", "true_label"]
    df, left_out, pred, gap, majority_f1 = _restated_cv(planted, variant, p)
    assert left_out == 2 and len(frame) == len(df) == 398 and sorted(frame["index"]) == list(range(398))
    assert (frame["true_label"].to_numpy() == df["class"].to_numpy()[frame["index"]]).all()
    sure = np.array([gap[i] > 1e-5 for i in frame["index"]])
    want = np.array([pred[i] for i in frame["index"]])
    print(f"{variant} p{p}: {int((~sure).sum())} of 398 excluded, smallest gap {min(gap.values()):.3e}, "
          f"F1 {result['f1_score_mean']:.4f} (majority class {majority_f1:.4f})")
    assert (~sure).sum() <= 0.02 * len(frame)
    assert (frame["predicted_label"].to_numpy()[sure] == want[sure]).all()
    if variant == "node2vec":
        assert result["f1_score_mean"] > majority_f1
