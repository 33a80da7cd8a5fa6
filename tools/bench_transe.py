#!/usr/bin/env python3
"""Times the three TransE kernels (csrc/transe.hip) at the reference's size: 175 094 entities, D 768, a synthetic triple list.

Reports, each against its ceiling:
  * step: groups/s of one epoch (64 launches), WITHOUT and WITH the per-launch normalise, and the bytes added by float
    atomics per second against the chip-wide atomic rate (~1.3 TB/s of added bytes); a group adds at most (3 + K) rows of 4 D
    bytes, so the ceiling is ATOMIC_RATE / ((3 + K) * 4 D) groups/s;
  * normalise: one pass over the entity table (read + write) against the HBM rate, and its share of an epoch at
    normalize_every = 1;
  * rank: queries/s and Q * N_e * D elements per second against the fp32 vector peak (a subtract and an accumulate per
    element, two instructions; the peak counts a fused multiply-add as two operations, so it is peak / 2 instructions and
    peak / 4 elements per second) and against what HBM could feed if every entity row came from HBM once per 16 queries.
Prints one JSON line and writes it, with a short table, to --out (profiles/transe.md).

    python tools/bench_transe.py [--entities 175094] [--triples 2000000] [--queries 512] [--out profiles/transe.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMIC_RATE = 1.3e12    # bytes of float atomic adds per second, chip-wide (MI355X)
HBM_RATE = 6.0e12       # bytes per second, a table swept in order
FP32_VECTOR_PEAK = 157.3e12   # FLOP/s, an FMA counted as two: half as many lane-instructions; a distance element takes two
RANK_TILE = 16          # queries a workgroup keeps in LDS (csrc/transe.hip)


def synthetic_triples(n_entities, n_relations, n_triples, seed=0):
    """Heads uniform, tails skewed towards low ids (n * u^3: a few hubs), relations uniform; self-loops dropped."""
    rng = np.random.RandomState(seed)
    h = rng.randint(0, n_entities, n_triples)
    t = (rng.random_sample(n_triples) ** 3 * n_entities).astype(np.int64)
    r = rng.randint(0, n_relations, n_triples)
    keep = h != t
    return np.stack([h[keep], r[keep], t[keep]], axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--entities", type=int, default=175094)
    ap.add_argument("--relations", type=int, default=32)
    ap.add_argument("--triples", type=int, default=2000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--negatives", type=int, default=1)
    ap.add_argument("--norm", type=int, default=1)
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transe.md"))
    a = ap.parse_args()

    import torch

    from stonkgs_amd import _hip as hip
    from stonkgs_amd.transe import TransE, transe_rank

    triples = synthetic_triples(a.entities, a.relations, a.triples)
    n, d, k = len(triples), a.dim, a.negatives
    m = TransE(n_components=d, epochs=1, negatives=k, norm=a.norm, seed=0)
    ent0, rel0 = m.initial_vectors(a.entities, a.relations)
    tri = torch.from_numpy(triples).cuda()
    order = torch.from_numpy(m.epoch_order(n, 0)).cuda()
    plan = m.launch_plan(n)
    stream = hip.stream_ptr()

    def epoch(normalise):
        ent, rel = ent0.cuda(), rel0.cuda()
        loss = torch.zeros(len(plan), 2, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, (e, lo, hi) in enumerate(plan):
            hip.call("stonk_transe_step", hip.ptr(ent), hip.ptr(rel), a.entities, a.relations, d, hip.ptr(tri), n, hip.ptr(order),
                     lo, hi, k, a.norm, m.margin, m.lr, 0, e, loss[i].data_ptr(), stream)
            if normalise:
                hip.call("stonk_rows_l2_normalize", hip.ptr(ent), d, 0, a.entities, d, stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ent, rel, loss.double().sum(0).cpu().numpy()

    epoch(True)                                            # the first calls load the code objects
    step_s, _, _, _ = epoch(False)
    both_s, ent, rel, loss = epoch(True)
    # one normalise pass alone (ten in a row, timed together)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        hip.call("stonk_rows_l2_normalize", hip.ptr(ent), d, 0, a.entities, d, stream)
    torch.cuda.synchronize()
    norm_s = (time.perf_counter() - t0) / 10
    norm_bytes = 2 * a.entities * d * 4
    # a group adds at most (3 + K) rows; what it did add: 3 rows per group with an active term, one per active term - not
    # observable from outside, so the at-most figure is reported as such
    added_max = n * (3 + k) * d * 4
    ceiling_groups = ATOMIC_RATE / ((3 + k) * 4 * d)

    queries = triples[np.random.RandomState(1).choice(n, a.queries, replace=False)]
    transe_rank(ent, rel, queries[:16], 0, a.norm)
    rank_s = {}
    for norm in (1, 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        less, equal = transe_rank(ent, rel, queries, 0, norm)
        torch.cuda.synchronize()
        rank_s[norm] = time.perf_counter() - t0
    elems = a.queries * a.entities * d
    line = {"bench": "transe", "entities": a.entities, "relations": a.relations, "triples": n, "dim": d, "negatives": k,
            "norm": a.norm, "launches_per_epoch": len(plan),
            "step_seconds_per_epoch": round(step_s, 4), "step_groups_per_s": round(n / step_s, 1),
            "step_ceiling_groups_per_s": round(ceiling_groups, 1), "step_fraction_of_ceiling": round(n / step_s / ceiling_groups, 4),
            "step_added_bytes_at_most_per_s": round(added_max / step_s, 1),
            "epoch_seconds_with_normalise_every_launch": round(both_s, 4),
            "normalise_share_of_epoch": round(1.0 - step_s / both_s, 4),
            "normalise_seconds": round(norm_s, 6), "normalise_bytes_per_s": round(norm_bytes / norm_s, 1),
            "normalise_fraction_of_hbm": round(norm_bytes / norm_s / HBM_RATE, 4),
            "rank_queries": a.queries, "rank_seconds_l1": round(rank_s[1], 4), "rank_seconds_l2": round(rank_s[2], 4),
            "rank_queries_per_s_l1": round(a.queries / rank_s[1], 1), "rank_queries_per_s_l2": round(a.queries / rank_s[2], 1),
            "rank_elements_per_s_l1": round(elems / rank_s[1], 1), "rank_elements_per_s_l2": round(elems / rank_s[2], 1),
            "rank_fraction_of_fp32_vector_peak_l1": round(4 * elems / rank_s[1] / FP32_VECTOR_PEAK, 4),
            "rank_fraction_of_fp32_vector_peak_l2": round(4 * elems / rank_s[2] / FP32_VECTOR_PEAK, 4),
            "rank_hbm_ceiling_elements_per_s": round(HBM_RATE / 4 * RANK_TILE, 1),
            "mean_loss": round(float(loss[0] / max(loss[1], 1.0)), 4),
            "finite": bool(torch.isfinite(ent).all() and torch.isfinite(rel).all()), "mean_less": round(float(less.mean()), 1)}
    text = json.dumps(line)
    print(text)
    with open(a.out, "w") as f:
        f.write("# TransE kernels: measured rates\n\n`python tools/bench_transe.py`, one MI355X, wall time around each stage with a "
                "device synchronisation\n(one run; no clock pinning; the rank times include the copy of the counts to the host). "
                "Triples: synthetic, see `synthetic_triples` in the tool.\n\n")
        f.write("| stage | seconds | rate | against |\n|---|---|---|---|\n")
        f.write(f"| step, one epoch ({len(plan)} launches, {n} groups, K {k}, norm {a.norm}) | {step_s:.3f} | {n / step_s:.3e} groups/s | "
                f"{n / step_s / ceiling_groups:.2f} of the {ceiling_groups:.3e} groups/s the ~1.3 TB/s atomic rate allows at "
                f"(3 + K) * 4 D added bytes a group |\n")
        f.write(f"| the same with a normalise after every launch | {both_s:.3f} | normalise share {1 - step_s / both_s:.1%} | - |\n")
        f.write(f"| normalise, one pass over [{a.entities}, {d}] | {norm_s:.6f} | {norm_bytes / norm_s:.3e} B/s | "
                f"{norm_bytes / norm_s / HBM_RATE:.2f} of {HBM_RATE:.1e} B/s |\n")
        for norm in (1, 2):
            f.write(f"| rank, {a.queries} queries, all {a.entities} candidates, norm {norm} | {rank_s[norm]:.4f} | "
                    f"{a.queries / rank_s[norm]:.3e} queries/s, {elems / rank_s[norm]:.3e} elements/s | "
                    f"{4 * elems / rank_s[norm] / FP32_VECTOR_PEAK:.2f} of the fp32 vector peak (two instructions an element); HBM could "
                    f"feed {HBM_RATE / 4 * RANK_TILE:.2e} elements/s at one row read per {RANK_TILE} queries |\n")
        f.write("\nThe step's ceiling counts (3 + K) added rows for EVERY group; a group whose terms are all inactive adds nothing, and how "
                "many there were is not observable from outside, so a fraction above 1 says that the kernel runs at the atomic rate, not "
                "above it.\n")
        f.write("\nBench line:\n\n```\n" + text + "\n```\n")


if __name__ == "__main__":
    main()
