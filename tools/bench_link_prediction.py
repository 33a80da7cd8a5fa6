#!/usr/bin/env python3
"""Times the link-prediction score (csrc/link_prediction.hip, stonkgs_amd/link_prediction.py) at the reference's size: the
synthetic graph of tools/bench_node2vec.py (175 094 nodes), a D 768 table trained on it by node2vec at its defaults (4 walks
of 127 per node; a table that is barely trained gives features so small that the fit stops at its starting point), 10^6
examples (half of them sampled non-edges).

Reports negatives per second; the time of one stonk_linkpred_lossgrad evaluation and of the forward-only call with the
bytes they gather per second (two table rows per example) against the achievable HBM rate (~6.3 TB/s); a whole
HadamardLogisticRegression fit on the 75 % train block with its evaluation count, at the default tolerance and at 1e-6; and scikit-learn's LogisticRegression on
the materialised features of a 10^5 subset (CPU; skipped when scikit-learn is not importable). Prints one JSON line and
writes it, with a short table, to --out.

    python tools/bench_link_prediction.py [--nodes 175094] [--examples 1000000] [--out profiles/link_prediction_bench.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_RATE = 6.3e12   # bytes per second a streaming kernel reaches on an MI355X (8 TB/s peak)


def timed(fn, repeats):
    import torch

    fn()                                              # warm-up: code object, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=175094)
    ap.add_argument("--degree", type=int, default=16)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--examples", type=int, default=1000000)
    ap.add_argument("--sklearn_examples", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_prediction_bench.md"))
    a = ap.parse_args()

    import torch
    from bench_node2vec import synthetic_graph

    from stonkgs_amd import _hip as hip
    from stonkgs_amd.link_prediction import (HadamardLogisticRegression, linkpred_lossgrad, roc_auc, sample_non_edges,
                                             sample_positive_edges, stratified_split)
    from stonkgs_amd.node2vec import Node2Vec

    if not torch.cuda.is_available():
        raise SystemExit("bench_link_prediction needs an MI355X: nothing here is measured on a CPU")
    src, tgt = synthetic_graph(a.nodes, a.degree)
    t0 = time.perf_counter()
    model = Node2Vec(n_components=a.dim, seed=0, keep_walks=False).fit(list(zip(src.tolist(), tgt.tolist())))
    torch.cuda.synchronize()
    node2vec_s = time.perf_counter() - t0
    n, rowptr, col = len(model.names), model.rowptr, model.col
    edges = len(col) // 2
    half = a.examples // 2
    pos = sample_positive_edges(rowptr, col, min(1.0, (half + 0.5) / edges), seed=0)[:half]

    sample_non_edges(rowptr, col, 1024, seed=1)       # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    neg = sample_non_edges(rowptr, col, len(pos), seed=0)     # (includes the upload of the graph and reading the counter)
    torch.cuda.synchronize()
    neg_s = time.perf_counter() - t0
    rp = torch.from_numpy(rowptr).cuda()
    cl = torch.from_numpy(col).cuda()
    out, fail = torch.empty(len(pos), 2, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    neg_kernel_s = timed(lambda: hip.call("stonk_sample_non_edges", hip.ptr(rp), hip.ptr(cl), n, 0, len(pos), 0, hip.ptr(out),
                                          hip.ptr(fail), hip.stream_ptr()), a.repeats)

    pairs = np.concatenate([pos, neg.cpu().numpy()])
    labels = np.r_[np.ones(len(pos), np.float32), np.zeros(len(pos), np.float32)]
    train, test = stratified_split(labels, 0.25, seed=0)
    order = np.concatenate([train, test])
    emb = model._w_in
    pairs_dev, y_dev = torch.from_numpy(pairs[order]).cuda(), torch.from_numpy(labels[order]).cuda()
    total = len(order)
    w = torch.from_numpy(np.random.RandomState(0).standard_normal(a.dim).astype(np.float32)).cuda()
    partials = torch.empty(int(hip.lib().stonk_linkpred_partial_rows()), a.dim + 2, device="cuda")
    scores = torch.empty(total, device="cuda")
    grad_s = timed(lambda: linkpred_lossgrad(emb, pairs_dev, y_dev, w, 0.1, None, partials), a.repeats)
    fwd_s = timed(lambda: linkpred_lossgrad(emb, pairs_dev, None, w, 0.1, scores, None), a.repeats)
    gathered = total * (2 * a.dim * 4 + 8 + 4)        # two rows, the pair and the label per example

    k = len(train)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    clf = HadamardLogisticRegression().fit(emb, pairs_dev[:k], y_dev[:k])
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    z = clf.decision_function(emb, pairs_dev[k:])
    auc, auc_hard = roc_auc(z, labels[test]), roc_auc(z > 0, labels[test])
    # the same fit at a tolerance 100 times smaller: a fit that iterates whatever the size of the table's entries
    t0 = time.perf_counter()
    tight = HadamardLogisticRegression(tol=1e-6, max_iter=200).fit(emb, pairs_dev[:k], y_dev[:k])
    torch.cuda.synchronize()
    tight_s = time.perf_counter() - t0
    zt = tight.decision_function(emb, pairs_dev[k:])
    tight_auc, tight_hard = roc_auc(zt, labels[test]), roc_auc(zt > 0, labels[test])

    line = {"bench": "link_prediction", "nodes": n, "edges": edges, "dim": a.dim, "examples": total, "train": k,
            "test": total - k, "node2vec_fit_seconds": round(node2vec_s, 3),
            "negatives": len(pos), "negatives_seconds_with_upload": round(neg_s, 5),
            "negatives_kernel_seconds": round(neg_kernel_s, 6), "negatives_per_s_kernel": round(len(pos) / neg_kernel_s, 1),
            "lossgrad_seconds": round(grad_s, 6), "lossgrad_gathered_bytes": int(gathered),
            "lossgrad_bytes_per_s": round(gathered / grad_s, 1), "lossgrad_hbm_fraction": round(gathered / grad_s / HBM_RATE, 4),
            "forward_seconds": round(fwd_s, 6), "forward_bytes_per_s": round((gathered - 4 * total) / fwd_s, 1),
            "forward_hbm_fraction": round((gathered - 4 * total) / fwd_s / HBM_RATE, 4),
            "table_bytes": int(n * a.dim * 4), "fit_seconds": round(fit_s, 4), "fit_iterations": clf.n_iter_,
            "fit_evaluations": clf.n_eval_, "fit_converged": bool(clf.converged_), "auc": round(auc, 4),
            "auc_hard_labels": round(auc_hard, 4), "tol1e-6_fit_seconds": round(tight_s, 4),
            "tol1e-6_fit_iterations": tight.n_iter_, "tol1e-6_fit_evaluations": tight.n_eval_,
            "tol1e-6_fit_converged": bool(tight.converged_), "tol1e-6_auc": round(tight_auc, 4),
            "tol1e-6_auc_hard_labels": round(tight_hard, 4),
            "table_mean_abs_entry": float(emb.abs().mean())}

    try:
        from sklearn.linear_model import LogisticRegression
    except ImportError:
        line["sklearn"] = "not importable: skipped"
    else:
        m = min(a.sklearn_examples, k)
        sub = pairs[train[:m]]
        table = model.vectors.astype(np.float64)
        t0 = time.perf_counter()
        x = table[sub[:, 0]] * table[sub[:, 1]]
        feat_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = LogisticRegression().fit(x, labels[train[:m]].astype(np.int64))
        sk_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        ours = HadamardLogisticRegression().fit(emb, pairs_dev[:m], y_dev[:m])
        torch.cuda.synchronize()
        line.update({"sklearn_examples": m, "sklearn_feature_seconds": round(feat_s, 3), "sklearn_fit_seconds": round(sk_s, 3),
                     "sklearn_iterations": int(ref.n_iter_[0]), "same_subset_fit_seconds": round(time.perf_counter() - t0, 4),
                     "same_subset_evaluations": ours.n_eval_,
                     "same_subset_max_coef_difference": float(np.abs(ours.coef_[0] - ref.coef_[0]).max())})

    text = json.dumps(line)
    print(text)
    with open(a.out, "w") as f:
        f.write("# Link-prediction score: output of the bench tool\n\n")
        f.write("`python tools/bench_link_prediction.py`, one MI355X, wall time around each stage with a device synchronisation,\n"
                f"kernel times the mean of {a.repeats} calls after a warm-up call (one run; no clock pinning). Graph: synthetic, see\n"
                "`synthetic_graph` in tools/bench_node2vec.py; table: node2vec at its defaults on it.\n\n")
        f.write("| stage | seconds | rate |\n|---|---|---|\n")
        f.write(f"| {len(pos)} negatives, kernel | {neg_kernel_s:.6f} | {len(pos) / neg_kernel_s:.3e} negatives/s |\n")
        f.write(f"| the same through `sample_non_edges` (graph upload, counter read) | {neg_s:.4f} | |\n")
        f.write(f"| loss + gradient, {total} examples, D {a.dim} | {grad_s:.6f} | {gathered / grad_s:.3e} gathered bytes/s = "
                f"{gathered / grad_s / HBM_RATE:.2f} of ~6.3 TB/s |\n")
        f.write(f"| forward only (scores) | {fwd_s:.6f} | {(gathered - 4 * total) / fwd_s:.3e} gathered bytes/s = "
                f"{(gathered - 4 * total) / fwd_s / HBM_RATE:.2f} of ~6.3 TB/s |\n")
        f.write(f"| whole fit, {k} examples | {fit_s:.3f} | {clf.n_iter_} iterations, {clf.n_eval_} evaluations, "
                f"converged {clf.converged_}; held-out auc {auc:.4f}, hard labels {auc_hard:.4f} |\n")
        f.write(f"| the same fit at tol 1e-6, max_iter 200 | {tight_s:.3f} | {tight.n_iter_} iterations, {tight.n_eval_} evaluations, "
                f"converged {tight.converged_}; held-out auc {tight_auc:.4f}, hard labels {tight_hard:.4f} |\n")
        if "sklearn_fit_seconds" in line:
            f.write(f"| scikit-learn fit, {line['sklearn_examples']} examples (CPU) | {line['sklearn_fit_seconds']:.3f} "
                    f"(+ {line['sklearn_feature_seconds']:.3f} building the features) | {line['sklearn_iterations']} iterations |\n")
            f.write(f"| this fit on the same {line['sklearn_examples']} examples | {line['same_subset_fit_seconds']:.3f} | "
                    f"{line['same_subset_evaluations']} evaluations; max coefficient difference "
                    f"{line['same_subset_max_coef_difference']:.2e} |\n")
        f.write("\nBench line:\n\n```\n" + text + "\n```\n")


if __name__ == "__main__":
    main()
