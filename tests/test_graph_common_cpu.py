"""stonkgs_amd/graph_common.py: the host helpers node2vec.py, transe.py, link_prediction.py and kg_baseline_model.py share.
CPU only."""
import numpy as np
import pytest

from stonkgs_amd import graph_common as gc
from stonkgs_amd.node2vec import build_csr
from stonkgs_amd.transe import build_triples


def test_factorize_names_numbers_by_first_appearance_source_before_target():
    # repeated names, one name on both sides of a row, ints and strings mixed (1 and "1" are two names)
    src, tgt = ["b", "a", 1, "b", "c"], ["a", "a", "1", 1, "b"]
    codes, names = gc.factorize_names(src, tgt)
    assert names == ["b", "a", 1, "1", "c"]
    assert codes.shape == (5, 2) and codes.tolist() == [[0, 1], [1, 1], [2, 3], [0, 2], [4, 0]]
    # the numbering build_csr and build_triples document is this one
    assert build_csr(src, tgt)[0] == names
    rel = ["up", "down", "up", 7, "down"]
    names_e, names_r, triples = build_triples(src, rel, tgt)
    assert names_e == names and names_r == ["up", "down", 7]
    assert triples.tolist() == [[0, 0, 1], [1, 1, 1], [2, 0, 3], [0, 2, 2], [4, 1, 0]]
    one, only = gc.factorize_names(rel)
    assert one.shape == (5, 1) and one[:, 0].tolist() == [0, 1, 0, 2, 1] and only == names_r
    none, no_names = gc.factorize_names([], [])
    assert none.shape == (0, 2) and no_names == []


def test_read_columns_from_a_file_a_frame_and_tuples(tmp_path):
    import pandas as pd

    df = pd.DataFrame({"source": ["a", "b", "a"], "relation": ["r", "s", "r"], "target": ["b", "c", "c"], "evidence": list("xyz")})
    path = tmp_path / "rows.tsv"
    df.to_csv(path, sep="\t", index=False)
    names = ("source", "relation", "target")
    want = (["a", "b", "a"], ["r", "s", "r"], ["b", "c", "c"])
    rows = [("a", "r", "b"), ("b", "s", "c"), ("a", "r", "c")]
    assert gc.read_columns(str(path), "\t", names) == want and gc.read_columns(path, "\t", names) == want
    assert gc.read_columns(df, "\t", names) == want
    assert gc.read_columns(rows, "\t", names) == want and gc.read_columns(iter(rows), "\t", names) == want
    assert gc.read_columns(df, "\t", ("source", "target")) == (want[0], want[2])
    assert gc.read_columns([], "\t", ("source", "target")) == ([], [])
    with pytest.raises(ValueError):
        gc.read_columns(rows, "\t", ("source", "target"))         # triples where pairs are expected


@pytest.mark.parametrize("n, parts", [(3, 7), (7, 7), (10, 4), (129, 7), (1, 1), (0, 3)])
def test_cuts_tile_the_range_in_order(n, parts):
    bounds = gc.cuts(n, parts)
    assert len(bounds) == parts + 1 and bounds[0] == 0 and bounds[-1] == n
    sizes = np.diff(bounds)
    assert (sizes >= 0).all() and sizes.sum() == n and sizes.max() - sizes.min() <= 1
    assert [i for lo, hi in zip(bounds, bounds[1:]) for i in range(lo, hi)] == list(range(n))
    if n == parts:
        assert sizes.tolist() == [1] * n


def test_decayed_lr_with_and_without_a_floor():
    assert gc.decayed_lr(0.01, None, 3, 10) == 0.01 and gc.decayed_lr(0.01, None, 0, 1) == 0.01
    assert gc.decayed_lr(0.1, 0.01, 0, 10) == 0.1
    assert gc.decayed_lr(0.1, 0.01, 5, 10) == 0.1 - (0.1 - 0.01) * 5 / 10 == pytest.approx(0.055)
    assert gc.decayed_lr(0.1, 0.01, 9, 10) > 0.01                 # the last launch is still above the floor
    assert gc.decayed_lr(0.025, 0.025, 7, 10) == 0.025


def test_epoch_means_divide_by_the_count_clamped_to_one():
    import torch

    # launches 0, 2 -> epoch 0; 1, 4 -> epoch 1; 3 -> epoch 2, which counted no term (its sum column is not even zero)
    loss = torch.tensor([[3.0, 2.0], [1.0, 4.0], [5.0, 2.0], [0.5, 0.0], [2.0, 0.0]])
    assert gc.epoch_means(loss, [0, 1, 0, 2, 1], 3) == [2.0, 0.75, 0.5]
    assert gc.epoch_means(loss, [0, 1, 0, 2, 1], 4) == [2.0, 0.75, 0.5, 0.0]      # an epoch without a launch
    assert gc.epoch_means(torch.zeros(0, 2), [], 1) == [0.0]
