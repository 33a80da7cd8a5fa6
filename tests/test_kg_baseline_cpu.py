"""KG baseline without a GPU: the three entry points exist in header, ctypes table and library; the dropout keep rule and one
optimizer step restated; the host logic of stonkgs_amd/kg_baseline_model.py.

THE YARDSTICK of the GPU tests lives here: ``Restatement`` is the reference's model and training step in the very torch
calls of ref:src/stonkgs/models/kg_baseline_model.py:70-73,93-110 - torch.max, dropout (as an injected mask), nn.Linear,
softmax, nn.CrossEntropyLoss(weight=...), torch.optim.AdamW(lr=...) - in fp64 or fp32. (The reference's module itself
needs pytorch_lightning and mlflow at import.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from stonkgs_amd import _hip
from stonkgs_amd import kg_baseline_model as kgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("stonk_walk_maxpool", "stonk_kgb_train_steps", "stonk_kgb_predict")


# ------------------------------------------------------------------------------------------------------ the yardstick
def pool_restated(table, ids, dtype=torch.float64):
    """torch.max(x, dim=1).values over the gathered [n, L, D] sequences; id -1 is the reference's null vector."""
    t = torch.cat([torch.as_tensor(table, dtype=dtype), torch.zeros(1, table.shape[1], dtype=dtype)])
    x = t[torch.as_tensor(np.where(ids < 0, len(table), ids), dtype=torch.long)]
    return torch.max(x, dim=1).values


class Restatement:
    """One fold's classifier trained a step at a time on already pooled rows, dropout mask injected."""

    def __init__(self, weight, bias, class_weights, lr=1e-3, dtype=torch.float64, double_softmax=True):
        self.dtype, self.double_softmax = dtype, double_softmax
        self.linear = torch.nn.Linear(weight.shape[1], weight.shape[0]).to(dtype)
        with torch.no_grad():
            self.linear.weight.copy_(torch.as_tensor(weight, dtype=dtype))
            self.linear.bias.copy_(torch.as_tensor(bias, dtype=dtype))
        self.loss_fct = torch.nn.CrossEntropyLoss(reduction="mean", weight=torch.as_tensor(class_weights, dtype=dtype))
        self.optimizer = torch.optim.AdamW(self.linear.parameters(), lr=lr)

    def forward(self, pooled, mask=None, p=0.0):
        h = torch.as_tensor(pooled, dtype=self.dtype)
        if mask is not None:
            h = h * torch.as_tensor(mask, dtype=self.dtype) * (1.0 / (1.0 - float(np.float32(p))))
        z = self.linear(h)
        return torch.softmax(z, dim=1) if self.double_softmax else z

    def step(self, pooled, y, mask=None, p=0.0):
        loss = self.loss_fct(self.forward(pooled, mask, p), torch.as_tensor(y, dtype=torch.long))
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return float(loss.detach())

    def state(self):
        """(W, b, mW, vW, mb, vb) as fp64 numpy."""
        st = self.optimizer.state
        w, b = self.linear.weight, self.linear.bias
        out = [w, b, st[w]["exp_avg"], st[w]["exp_avg_sq"], st[b]["exp_avg"], st[b]["exp_avg_sq"]]
        return [t.detach().double().numpy().copy() for t in out]


def train_restated(pooled, labels, order_steps, weight, bias, cw, lr, seed, run, p, first_step=0, dtype=torch.float64):
    """Walk ``order_steps`` ([steps, batch] int, -1 padded) with the kernel's keep masks. Returns (Restatement, losses).
    A step whose rows are all padding has the loss 0 / 0 = NaN and updates nothing (csrc/kg_baseline.hip, step (D)); it
    still counts as a global step: the masks of the steps after it are keyed by ``first_step + s``, and AdamW's bias
    corrections of the steps after it use the step number that counts it (the optimizer's own counter is advanced).
    ``first_step`` > 0 only offsets the masks: a run restated from the middle starts with fresh moments."""
    rs = Restatement(weight, bias, cw, lr, dtype)
    losses = []
    for s, row in enumerate(np.asarray(order_steps)):
        live = row >= 0
        if not live.any():
            assert rs.optimizer.state, "an all-padding step before the first real one: torch's AdamW has no counter yet"
            for st in rs.optimizer.state.values():
                st["step"] += 1
            losses.append(float("nan"))
            continue
        mask = kgb.dropout_keep_mask(seed, run, first_step + s, len(row), pooled.shape[1], p)[live] if p > 0 else None
        losses.append(rs.step(pooled[row[live]], labels[row[live]], mask, p))
    return rs, np.array(losses)


def _problem(D, C, n=40, seed=0):
    rng = np.random.RandomState(seed)
    pooled = rng.randn(n, D).astype(np.float32)
    labels = rng.randint(0, C, n).astype(np.int32)
    labels[:C] = np.arange(C)
    weight = (rng.rand(C, D).astype(np.float32) - 0.5) * (2 / np.sqrt(D))
    bias = (rng.rand(C).astype(np.float32) - 0.5) * (2 / np.sqrt(D))
    cw = (1.0 / rng.randint(1, 9, C)).astype(np.float32)
    return pooled, labels, weight, bias, cw


# ------------------------------------------------------------------------------------------------------ the symbols
def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "stonk_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert name in _hip._SIGNATURES
        assert hasattr(lib, name), name
    assert _hip.lib().stonk_abi_version() == 5
    assert 1 <= kgb.max_steps() <= 4096
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert "kg_baseline.o" in makefile


def test_refusals_need_no_gpu():
    lib = _hip.lib()
    ok = [16, 64, 40, 64, 16, 3, 1, 16, 64, 8, 16, 16, 8, 16, 16, 16, 16, 16, 16, 16, 16, 8, 16,
          1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 1, 0]

    def train(**kw):
        pos = {"pooled": 0, "D": 3, "C": 5, "batch": 9, "n_steps_max": 12, "ld_order": 8, "ld_loss": 21}
        args = list(ok)
        for k, val in kw.items():
            args[pos[k]] = val
        return lib.stonk_kgb_train_steps(*args)

    cap = kgb.max_steps()
    assert train(C=17, ld_order=1 << 20) == _hip.ESHAPE and train(C=1) == _hip.ESHAPE
    assert train(batch=65, ld_order=1 << 20) == _hip.ESHAPE
    assert train(D=96) == _hip.ESHAPE and train(D=1088) == _hip.ESHAPE
    assert train(n_steps_max=cap + 1, ld_order=1 << 30, ld_loss=1 << 30) == _hip.ESHAPE
    assert train(pooled=0) == _hip.EINVAL
    assert train(n_steps_max=0) == _hip.OK      # (nothing to do: no launch)
    assert lib.stonk_walk_maxpool(0, 4, 1, 4, 16, 64, 10, 64, 16, 64, 16, 0) == _hip.EINVAL
    assert lib.stonk_walk_maxpool(16, 4, 1, 4, 16, 96, 10, 96, 16, 96, 16, 0) == _hip.ESHAPE
    assert lib.stonk_walk_maxpool(16, 4, 1, 4, 16, 66, 10, 64, 16, 64, 16, 0) == _hip.EALIGN
    assert lib.stonk_kgb_predict(16, 64, 10, 64, 16, 4, 16, 16, 17, 16, 16, 16, 0) == _hip.ESHAPE
    assert lib.stonk_kgb_predict(16, 64, 10, 64, 0, 4, 16, 16, 3, 16, 16, 16, 0) == _hip.EINVAL


# ------------------------------------------------------------------------------------------------------ dropout
def _h(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _keep_scalar(seed, run, step, i, d, p):
    """csrc/common.h and graph_common.h, one element at a time in Python integers."""
    seedkey = _h(seed * 0x9E3779B9 + 0x85EBCA6B)
    stepkey = _h(_h(seedkey + run) ^ ((step * 0x9E3779B1) & 0xFFFFFFFF))
    x = ((i * 0x9E3779B1 + stepkey) & 0xFFFFFFFF) ^ ((d * 0x85EBCA77) & 0xFFFFFFFF)
    y = ((x & 0xFFFFFF) * 0xB5297B + x) & 0xFFFFFFFF
    z = ((y >> 8) * 0x68E31D) & 0xFFFFFFFF
    return z >= int(float(np.float32(p)) * 4294967296.0 + 0.5)


def test_dropout_keep_rule():
    mask = kgb.dropout_keep_mask(42, 3, 1234, 8, 768, 0.1)
    assert mask.shape == (8, 768) and mask.dtype == bool
    for i, d in [(0, 0), (7, 767), (3, 255), (5, 256), (1, 64)]:
        assert mask[i, d] == _keep_scalar(42, 3, 1234, i, d, 0.1)
    big = np.stack([kgb.dropout_keep_mask(7, 0, s, 64, 1024, 0.1) for s in range(8)])
    assert abs(big.mean() - 0.9) < 2e-3                                      # (524 288 draws: sigma 4e-4)
    assert np.abs(big.mean(axis=(0, 1)) - 0.9).max() < 0.07                   # per feature, 512 draws: sigma 0.013
    assert kgb.dropout_keep_mask(42, 3, 1234, 8, 768, 0.0).all()
    for other in [(43, 3, 1234), (42, 4, 1234), (42, 3, 1235)]:               # seed, run and step all matter
        assert (kgb.dropout_keep_mask(*other, 8, 768, 0.1) != mask).any()
    assert (kgb.dropout_keep_mask(42, 3, 1234, 5, 768, 0.1) == mask[:5]).all()    # a row does not depend on the batch size


# ------------------------------------------------------------------------------------------------------ the step
def _numpy_step(W, b, mom, x, y, mask, p, cw, lr, t, wd=0.01, b1=0.9, b2=0.999, eps=1e-8):
    """What csrc/kg_baseline.hip computes in one step, in fp64 numpy: both softmaxes written out, the gradient by hand."""
    h = x.astype(np.float64) * mask / (1.0 - float(np.float32(p)))
    z = h @ W.T + b
    q = np.exp(z - z.max(1, keepdims=True))
    q /= q.sum(1, keepdims=True)
    r = np.exp(q - q.max(1, keepdims=True))
    r /= r.sum(1, keepdims=True)
    wy = cw.astype(np.float64)[y]
    rows = np.arange(len(y))
    loss = (wy * -np.log(r[rows, y])).sum() / wy.sum()
    dq = r.copy()
    dq[rows, y] -= 1.0
    dq *= (wy / wy.sum())[:, None]
    dz = q * (dq - (dq * q).sum(1, keepdims=True))
    out = []
    for prm, g, (m, v) in ((W, dz.T @ h, mom[0]), (b, dz.sum(0), mom[1])):
        prm = prm * (1.0 - lr * wd)
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * g * g
        prm = prm - lr / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
        out.append((prm, m, v))
    return loss, out


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_the_step_restated_three_ways(p):
    D, C = 64, 3
    pooled, labels, weight, bias, cw = _problem(D, C)
    rows = np.array([5, 0, 17, 2, 9, 1, 30, 22])
    r64 = Restatement(weight, bias, cw, 1e-3, torch.float64)
    r32 = Restatement(weight, bias, cw, 1e-3, torch.float32)
    single = Restatement(weight, bias, cw, 1e-3, torch.float64, double_softmax=False)
    W, b = weight.astype(np.float64), bias.astype(np.float64)
    mom = [(np.zeros_like(W), np.zeros_like(W)), (np.zeros_like(b), np.zeros_like(b))]
    for t in (1, 2, 3):
        mask = kgb.dropout_keep_mask(9, 0, t - 1, len(rows), D, p)
        l64, l32 = r64.step(pooled[rows], labels[rows], mask, p), r32.step(pooled[rows], labels[rows], mask, p)
        l1 = single.step(pooled[rows], labels[rows], mask, p)
        ln, ((W, mW, vW), (b, mb, vb)) = _numpy_step(W, b, mom, pooled[rows], labels[rows], mask, p, cw, 1e-3, t)
        mom = [(mW, vW), (mb, vb)]
        assert abs(ln - l64) < 1e-13
        for mine, ref in zip((W, b, mW, vW, mb, vb), r64.state()):
            assert np.abs(mine - ref).max() < 1e-13
        assert abs(l32 - l64) < 1e-6
        # (an AdamW update is lr * m / (sqrt(v) + eps) per element, at most lr = 1e-3: where a gradient element is a sum
        # that nearly cancels, fp32 keeps 3 or 4 of its digits and the update moves by that fraction of lr)
        for k, (a32, a64) in enumerate(zip(r32.state(), r64.state())):
            assert np.abs(a32 - a64).max() < (1e-5 if k < 2 else 1e-6)
        # the double softmax is really there: probabilities lie in [0, 1], so the second softmax is nearly flat and the
        # loss stays near log C, while a single softmax on the same inputs gives another value
        assert abs(l1 - l64) > 1e-3
        if t == 1:
            with torch.no_grad():
                q = r64.forward(pooled[rows], mask, p)
            assert torch.allclose(q.sum(1), torch.ones(len(rows), dtype=torch.float64))


def test_pool_restated_null_vector_takes_part():
    table = -np.abs(np.random.RandomState(1).randn(5, 4)).astype(np.float32) - 0.1
    ids = np.array([[0, 1, 2], [3, -1, 4], [-1, -1, -1]], dtype=np.int32)
    got = pool_restated(table, ids).numpy()
    assert (got[0] == table[:3].max(0)).all() and (got[1] == 0).all() and (got[2] == 0).all()


# ------------------------------------------------------------------------------------------------------ host logic
def _emb(names, D=4):
    return {n: np.full(D, float(i)) for i, n in enumerate(names)}


def test_id_matrices_for_both_variants():
    emb = _emb(["a", "b", "c", "rel"])
    walks = {"a": np.array(["a", "b", "zz"], dtype=object), "b": np.array(["b", "c", "a"], dtype=object),
             "c": np.array(["c", -1, "b"], dtype=object)}
    ds = kgb.Node2VecINDRAEntityDataset(emb, walks, ["a", "c"], ["b", "a"], [0, 1], max_len=6)
    assert ds.ids.dtype == np.int32 and ds.ids.tolist() == [[0, 1, -1, 1, 2, 0], [2, -1, 1, 0, 1, -1]]
    assert ds.table.dtype == np.float32 and ds.table.shape == (4, 4) and -1 not in emb     # the caller's dict is left alone
    assert len(ds) == 2
    item, label = ds[1]
    assert item.shape == (6, 4) and item.dtype == torch.float32 and int(label) == 1 and label.dtype == torch.long
    assert item[:, 0].tolist() == [2.0, 0.0, 1.0, 0.0, 1.0, 0.0]               # -1: the null vector
    with pytest.raises(ValueError):
        kgb.node2vec_id_matrix(ds.row_of, walks, ["a"], ["b"], max_len=254)
    emb[-1] = np.zeros(4)                                                      # a dict the reference has already touched
    te = kgb.TransEINDRAEntityDataset(emb, ["a", "b"], ["rel", "unknown_relation"], ["c", "a"], [1, 0])
    assert te.ids.tolist() == [[0, 3, 2], [1, -1, 0]] and te.table.shape == (4, 4)
    assert te[1][0][:, 0].tolist() == [1.0, 0.0, 0.0]


def test_triple_filter_and_class_weights():
    import pandas as pd

    df = pd.DataFrame({"source": ["a", "x", "b", "c"], "target": ["b", "a", "y", "a"], "relation": ["r"] * 4,
                       "class": ["u", "v", "u", "v"]})
    kept, left_out = kgb.filter_triples(df, _emb(["a", "b", "c"]).keys())
    assert left_out == 2 and kept["source"].tolist() == ["a", "c"] and kept.index.tolist() == [0, 1]
    labels = np.array([0, 0, 0, 1, 1, 2, 2, 2, 2, 0])
    w = kgb.inverse_count_class_weights(labels, [0, 1, 3, 5, 6, 7], 3)          # train: two 0s, one 1, three 2s
    assert w.dtype == np.float32 and np.allclose(w, [1 / 2, 1, 1 / 3])
    with pytest.raises(ValueError):
        kgb.inverse_count_class_weights(labels, [0, 1, 5], 3)                  # class 1 only among the test indices


def test_epoch_cutter_and_fold_step_counts():
    idx = np.arange(100, 137)                                                  # 37 examples: 5 steps of 8, the last of 5
    order = kgb.epoch_order(idx, 42, 1, 0)
    assert sorted(order.tolist()) == idx.tolist() and order.dtype == np.int32
    assert (kgb.epoch_order(idx, 42, 1, 0) == order).all()
    assert (kgb.epoch_order(idx, 42, 1, 1) != order).any() and (kgb.epoch_order(idx, 42, 2, 0) != order).any()
    for cap in (1, 2, 3, 5, 4096):
        spans = kgb.cut_epoch(order, 8, cap)
        assert all(len(s) % 8 == 0 and 0 < len(s) // 8 <= cap for s in spans)
        flat = np.concatenate(spans)
        assert len(flat) == 40 and (flat[:37] == order).all() and (flat[37:] == -1).all()
        assert len(spans) == -(-5 // cap)
    # folds whose sizes differ by one across a batch boundary make step counts that differ by one
    assert kgb.steps_per_epoch(320, 8) == 40 and kgb.steps_per_epoch(321, 8) == 41
    cuts = [kgb.cut_epoch(kgb.epoch_order(np.arange(k), 0, r, 0), 8, 16) for r, k in enumerate((321, 320, 321))]
    assert [[len(s) // 8 for s in c] for c in cuts] == [[16, 16, 9], [16, 16, 8], [16, 16, 9]]


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_kernels_refuse_to_run_without_a_gpu():
    ds = kgb.TransEINDRAEntityDataset(_emb(["a", "b", "r"], 64), ["a"], ["r"], ["b"], [0])
    with pytest.raises(_hip.StonkHipError):
        ds.pooled
