#!/usr/bin/env python3
"""Times the two node2vec kernels (csrc/node2vec.hip) at the reference's size: a synthetic graph of 175 094 nodes, D 768,
walk length 127, 4 walks per node, window 3, 5 negatives, one skip-gram pass in 64 launches per epoch.

Reports walk steps/s and, for the skip-gram pass, the bytes added by float atomics per second against the chip-wide atomic
rate (~1.3 TB/s of added bytes). Prints one JSON line and writes it, with a short table, to --out (profiles/node2vec.md).

    python tools/bench_node2vec.py [--nodes 175094] [--degree 16] [--out profiles/node2vec.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMIC_RATE = 1.3e12   # bytes of float atomic adds per second, chip-wide (MI355X)
M32 = 0xFFFFFFFF


def _hash32(x):
    x = x & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def context_rows(n_walks, L, window, seed):
    """Sum over all groups (w, t) of the number of context positions - the reduced window of the kernel's own formula."""
    seedkey = _hash32(np.uint64(seed ^ 0x6E327367))
    hw = _hash32((seedkey + np.arange(n_walks, dtype=np.uint64)) & np.uint64(M32))
    total = 0
    for t in range(L):
        key = _hash32(hw ^ np.uint64((t * 0x9E3779B1) & M32))
        b = 1 + (_hash32((key + np.uint64(0x85EBCA77)) & np.uint64(M32)) % np.uint64(window)).astype(np.int64)
        total += int((np.minimum(t + b, L - 1) - np.maximum(t - b, 0)).sum())
    return total


def synthetic_graph(n, degree, seed=0):
    """Every node draws `degree` partners, half of them uniform and half skewed towards low ids (n * u^3): a few hubs of
    degree in the thousands over a median of about 1.5 * degree."""
    rng = np.random.RandomState(seed)
    src = np.repeat(np.arange(n), degree)
    u = rng.random_sample(n * degree)
    tgt = np.where(np.arange(n * degree) % 2 == 0, (u * n).astype(np.int64), (u ** 3 * n).astype(np.int64))
    keep = src != tgt
    return src[keep], tgt[keep]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, default=175094)
    ap.add_argument("--degree", type=int, default=16)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--walklen", type=int, default=127)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node2vec.md"))
    a = ap.parse_args()

    import torch

    from stonkgs_amd import _hip as hip
    from stonkgs_amd.node2vec import Node2Vec, alias_table, build_csr

    src, tgt = synthetic_graph(a.nodes, a.degree)
    names, rowptr, col = build_csr(src, tgt)
    n = len(names)
    deg = np.diff(rowptr)
    m = Node2Vec(n_components=a.dim, walklen=a.walklen, epochs=a.epochs, seed=0)
    m.random_walks(np.zeros(2, dtype=np.int64), col[:1])   # a one-node graph: the first call loads the code object
    torch.cuda.synchronize()
    walk_s = {}
    second = Node2Vec(n_components=a.dim, walklen=a.walklen, epochs=a.epochs, p=0.25, q=4.0)
    for label, model in (("first_order", m), ("second_order", second)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w = model.random_walks(rowptr, col)
        torch.cuda.synchronize()
        walk_s[label] = time.perf_counter() - t0
        if label == "first_order":
            walks = w
    del w
    steps = a.epochs * n * (a.walklen - 1)

    counts = torch.bincount(walks.flatten().long(), minlength=n).cpu().numpy()
    thr, idx = alias_table(counts)
    a_thr, a_idx = torch.from_numpy(thr.view(np.int32)).cuda(), torch.from_numpy(idx).cuda()
    w_in, w_out = m.initial_vectors(n).cuda(), torch.zeros(n, a.dim, device="cuda")
    plan = m.launch_plan(n)
    loss = torch.zeros(len(plan), 2, device="cuda")
    stream = hip.stream_ptr()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, (_, w_lo, w_hi, p_lo, p_hi) in enumerate(plan):
        lr = m.alpha - (m.alpha - m.min_alpha) * i / len(plan)
        hip.call("stonk_sgns_step", hip.ptr(walks), a.walklen, a.walklen, w_lo, w_hi, p_lo, p_hi, hip.ptr(w_in), hip.ptr(w_out),
                 n, a.dim, m.window, m.negative, hip.ptr(a_thr), hip.ptr(a_idx), lr, 0, loss[i].data_ptr(), stream)
    torch.cuda.synchronize()
    sgns_s = time.perf_counter() - t0
    per = loss.double().cpu().numpy()
    groups = a.epochs * n * a.walklen
    # rows added: one per context occurrence (W_in) and one per target (W_out: the centre and the noise words; a noise draw
    # that hits the centre is skipped - under 0.1 % of the draws here, not subtracted)
    rows = context_rows(a.epochs * n, a.walklen, m.window, 0) + groups * (m.negative + 1)
    added = rows * a.dim * 4
    line = {"bench": "node2vec", "nodes": n, "edges": int(len(col) // 2), "max_degree": int(deg.max()),
            "median_degree": float(np.median(deg)), "dim": a.dim, "walklen": a.walklen, "walks_per_node": a.epochs,
            "window": m.window, "negatives": m.negative, "launches": len(plan),
            "walk_seconds_first_order": round(walk_s["first_order"], 4),
            "walk_steps_per_s_first_order": round(steps / walk_s["first_order"], 1),
            "walk_seconds_second_order_p0.25_q4": round(walk_s["second_order"], 4),
            "walk_steps_per_s_second_order": round(steps / walk_s["second_order"], 1),
            "sgns_seconds": round(sgns_s, 4), "sgns_seconds_per_epoch": round(sgns_s / a.epochs, 4),
            "sgns_groups_per_s": round(groups / sgns_s, 1), "sgns_added_bytes": int(added),
            "sgns_added_bytes_per_s": round(added / sgns_s, 1), "atomic_rate_fraction": round(added / sgns_s / ATOMIC_RATE, 4),
            "mean_loss_first_last_epoch": [round(float(per[:64, 0].sum() / per[:64, 1].sum()), 4),
                                           round(float(per[-64:, 0].sum() / per[-64:, 1].sum()), 4)],
            "finite": bool(torch.isfinite(w_in).all() and torch.isfinite(w_out).all())}
    text = json.dumps(line)
    print(text)
    with open(a.out, "w") as f:
        f.write("# node2vec kernels: measured rates\n\n`python tools/bench_node2vec.py`, one MI355X, wall time around each stage "
                "with a device synchronisation\n(one run; no clock pinning). Graph: synthetic, see `synthetic_graph` in the tool.\n\n")
        f.write("| stage | seconds | rate |\n|---|---|---|\n")
        f.write(f"| walks, first order ({a.epochs} x {n} walks of {a.walklen}) | {walk_s['first_order']:.3f} | "
                f"{steps / walk_s['first_order']:.3e} steps/s |\n")
        f.write(f"| walks, second order (p 0.25, q 4) | {walk_s['second_order']:.3f} | {steps / walk_s['second_order']:.3e} steps/s |\n")
        f.write(f"| skip-gram pass ({len(plan)} launches, {groups} groups) | {sgns_s:.3f} ({sgns_s / a.epochs:.3f} per epoch) | "
                f"{added / sgns_s:.3e} added bytes/s = {added / sgns_s / ATOMIC_RATE:.2f} of the ~1.3 TB/s atomic rate |\n")
        f.write("\nBench line:\n\n```\n" + text + "\n```\n")


if __name__ == "__main__":
    main()
