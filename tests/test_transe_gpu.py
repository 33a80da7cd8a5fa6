"""GPU, end to end: run_transe on the grid graph writes the TSV the ``transe`` variant of the KG baseline reads; the loaders
find every name in it; raw and filtered ``evaluate`` agree with the fp64 restatement run over the SAVED vectors.

'Agree': the kernel ranks in fp32, so a candidate whose fp64 distance lies within tau of the true entity's may fall on
either side; tau = 4x the largest deviation of the fp32 numpy restatement's distances from fp64 on these vectors (the rule
of test_transe_rank_gpu.py). Per query, less and less + equal must lie between the fp64 counts with the true distance moved
by -tau and +tau, raw and filtered; the metrics ``evaluate`` reports must be the host arithmetic on those counts."""
import numpy as np
import pytest

from stonkgs_amd import kg_baseline_model as kgb
from stonkgs_amd import transe as tr
from stonkgs_amd.stonkgs_model import prepare_df
from tests.test_transe_cpu import rank_distances
from tests.test_transe_rank_gpu import band_counts
from tests.test_transe_step_gpu import grid_graph

pytestmark = pytest.mark.gpu


def test_run_transe_writes_a_table_the_baseline_reads_and_evaluate_matches_the_restatement(hip, tmp_path):
    import pandas as pd

    rows = grid_graph()
    pre, out = str(tmp_path / "pretraining.tsv"), str(tmp_path / "transe.tsv")
    frame = pd.DataFrame(rows, columns=["source", "relation", "target"])
    frame["evidence"] = "text"
    frame.to_csv(pre, sep="\t", index=False)
    model, metrics = tr.run_transe(pre, embeddings_output_path=out, test_fraction=0.1, n_components=64, epochs=20, negatives=2,
                                   margin=4.0, norm=1, lr=0.02, seed=2, launches_per_epoch=8)
    assert len(model.entity_names) == 144 and len(model.relation_names) == 5 and len(model.triples) == 625 - 62
    assert set(tr.METRICS) <= set(metrics) and 0 < metrics["mrr"] <= 1 and metrics["mean_rank"] >= 1
    assert model.loss_history[-1] < model.loss_history[0]
    # the file, through the baseline's loaders
    emb = prepare_df(out)
    assert list(emb) == model.entity_names + model.relation_names
    ds = kgb.TransEINDRAEntityDataset(emb, frame["source"], frame["relation"], frame["target"], [0] * len(frame))
    assert ds.ids.shape == (625, 3) and (ds.ids >= 0).all()                # no missing name
    assert np.array_equal(ds.table[:144], model.entity_vectors) and np.array_equal(ds.table[144:], model.relation_vectors)
    assert np.array_equal(model.predict("n3_4"), ds.table[ds.row_of["n3_4"]]) and np.array_equal(model.predict("up"), ds.table[ds.row_of["up"]])
    pooled = ds.pooled.cpu().numpy()                                       # and through the baseline's first kernel
    assert np.array_equal(pooled[0], ds.table[ds.ids[0]].max(axis=0))
    # evaluate against the restatement over the saved vectors
    ent, rel = ds.table[:144], ds.table[144:]
    names_e, names_r, triples = tr.build_triples(frame["source"], frame["relation"], frame["target"])
    assert names_e == model.entity_names and names_r == model.relation_names
    _, test_pos = tr.split_triples(len(triples), 0.1, 2)
    test = triples[test_pos]
    index = tr.known_index(triples)
    for known in (None, index):
        ranks = []
        for side in (0, 1):
            d64, true, valid = rank_distances(ent.astype(np.float64), rel.astype(np.float64), test, side, 1)
            tau = 4 * float(np.abs(rank_distances(ent, rel, test, side, 1)[0].astype(np.float64) - d64).max())
            mask = None
            if known is not None:                                          # the other known-true entities do not count
                ptr, cand = tr.candidate_lists(test, side, index)
                mask = np.ones((len(test), 144), dtype=bool)
                for q in range(len(test)):
                    mask[q, cand[ptr[q]:ptr[q + 1]]] = False
            lo, hi, le_lo, le_hi = band_counts(d64, true, valid, tau, mask)
            less, equal = model.rank(test, side, known)
            print(f"{'filtered' if known else 'raw'} side {side}: tau {tau:.3e}, queries with a candidate inside the band "
                  f"{int((lo != hi).sum())} of {len(test)}")
            assert (lo <= less).all() and (less <= hi).all() and (le_lo <= less + equal).all() and (less + equal <= le_hi).all()
            assert (equal >= 1).all()
            ranks.append(tr.realistic_rank(less, equal))
        report = model.evaluate(test, known_triples=None if known is None else triples)
        assert report == tr.evaluation_report(*ranks)
        if known is not None:
            assert report == metrics                                       # what run_transe returned and logged
