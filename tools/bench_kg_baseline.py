"""Measures the KG baseline's kernels on the GPU and prints one JSON line per figure (profiles/kg_baseline.md quotes them):

* ``pool``: stonk_walk_maxpool at 100 000 examples, L 254, D 768 over a 175 094-row table, as gathered bytes per second
  (n * L * D * 4 bytes are read whatever the caches do) against the HBM rates;
* ``steps``: stonk_kgb_train_steps at the reference's shape (D 768, batch 8, 10 classes), one run and five runs per launch;
* ``longest``: time per step at the largest shape a launch accepts (D 1024, C 16, batch 64), which the step cap
  STONK_KGB_MAX_STEPS is chosen from;
* ``eager``: the same model trained with plain torch calls on the same GPU, one step per iteration - what a user has
  without the kernel.

    python tools/bench_kg_baseline.py [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stonkgs_amd import _hip as hip  # noqa: E402
from stonkgs_amd import kg_baseline_model as kgb  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12    # spec; a float4 copy as measured on this part


def _timed(fn, warmup, iters):
    """Median and spread of ``iters`` device-event timings (milliseconds)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def bench_pool(n, L, D, N):
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(N, D, device="cuda", generator=g)
    ids = torch.randint(0, N, (n, L), device="cuda", generator=g, dtype=torch.int32)
    pooled = torch.empty(n, D, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run():
        hip.call("stonk_walk_maxpool", hip.ptr(ids), L, n, L, hip.ptr(table), D, N, D, hip.ptr(pooled), D, hip.ptr(errors),
                 hip.stream_ptr())

    med, lo, hi = _timed(run, 2, 7)
    gathered = n * L * D * 4
    check = torch.stack([table[ids[e].long()].max(0).values for e in (0, n // 2, n - 1)])
    assert torch.equal(check, pooled[[0, n // 2, n - 1]]) and int(errors.item()) == 0
    print(json.dumps({"bench": "pool", "n": n, "L": L, "D": D, "table_rows": N, "ms_median": med, "ms_min": lo, "ms_max": hi,
                      "gathered_bytes": gathered, "table_bytes": N * D * 4, "gathered_bytes_per_s": gathered / (med * 1e-3),
                      "share_of_hbm_spec": gathered / (med * 1e-3) / HBM_PEAK,
                      "share_of_hbm_copy_rate": gathered / (med * 1e-3) / HBM_COPY}))


def _trainer(n, D, C, R, dropout=0.1):
    g = torch.Generator(device="cuda").manual_seed(1)
    pooled = torch.randn(n, D, device="cuda", generator=g)
    labels = np.random.RandomState(0).randint(0, C, n).astype(np.int32)
    lins = [torch.nn.Linear(D, C) for _ in range(R)]
    return kgb.KGBTrainer(pooled, labels, [l.weight.detach() for l in lins], [l.bias.detach() for l in lins],
                          [np.full(C, 1.0 / C, dtype=np.float32)] * R, 1e-3, dropout, seed=3)


def bench_steps(tag, n, D, C, batch, R, steps, iters=5):
    tr = _trainer(n, D, C, R)
    rng = np.random.RandomState(1)
    spans = [rng.randint(0, n, steps * batch).astype(np.int32) for _ in range(R)]
    med, lo, hi = _timed(lambda: tr.run_spans(spans, batch), 1, iters)   # (host time of a launch included: order upload, losses back)
    tr.check_errors()
    print(json.dumps({"bench": tag, "D": D, "C": C, "batch": batch, "runs": R, "steps_per_launch": steps, "ms_median": med,
                      "ms_min": lo, "ms_max": hi, "us_per_step": med * 1e3 / steps,
                      "steps_per_s_per_run": steps / (med * 1e-3), "steps_per_s_all_runs": R * steps / (med * 1e-3)}))


def bench_eager(n, D, C, batch, steps):
    g = torch.Generator(device="cuda").manual_seed(1)
    pooled = torch.randn(n, D, device="cuda", generator=g)
    labels = torch.randint(0, C, (n,), device="cuda", generator=g)
    linear, dropout = torch.nn.Linear(D, C).cuda(), torch.nn.Dropout(0.1)
    loss_fct = torch.nn.CrossEntropyLoss(weight=torch.full((C,), 1.0 / C, device="cuda"))
    opt = torch.optim.AdamW(linear.parameters(), lr=1e-3)
    order = torch.randint(0, n, (steps + 50, batch), device="cuda", generator=g)

    def run(lo, hi):
        for s in range(lo, hi):
            idx = order[s]
            loss = loss_fct(torch.softmax(linear(dropout(pooled[idx])), dim=1), labels[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()

    run(0, 50)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(50, 50 + steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"bench": "eager", "D": D, "C": C, "batch": batch, "runs": 1, "steps": steps, "us_per_step": dt * 1e6 / steps,
                      "steps_per_s_per_run": steps / dt}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a tenth of the sizes: a rehearsal, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kg_baseline needs the GPU: nothing is measured without one")
    q = 10 if args.quick else 1
    cap = kgb.max_steps()
    print(json.dumps({"bench": "setup", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                      "hip": torch.version.hip, "step_cap": cap}))
    bench_pool(100000 // q, 254, 768, 175094 // q)
    bench_steps("steps", 80000 // q, 768, 10, 8, 1, cap // q)
    bench_steps("steps", 80000 // q, 768, 10, 8, 5, cap // q)
    bench_steps("longest", 80000 // q, 1024, 16, 64, 1, cap // q, iters=3)
    bench_steps("longest", 80000 // q, 1024, 16, 64, 5, cap // q, iters=3)
    bench_eager(80000 // q, 768, 10, 8, 2000 // q)


if __name__ == "__main__":
    main()
