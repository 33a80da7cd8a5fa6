"""Input attributions at the benchmark's shape (batch 64, 12 layers / hidden 768, S 512, K = 175 094 entities, random
weights, dropout 0), one process, variants alternated, after warm-up. Prints one JSON line per measurement.

(a) stonk_input_attribution alone, padded and packed layout: us per launch (HIP events, N launches per window, median of
    REPS windows) and the bytes it must move - per live row 2 H of gradient plus 2 H (text, bf16) or 4 H (entity, fp32) of
    x, per live entity position its 8-byte id, per position 8 bytes of results and, in the packed layout, 4 of row map -
    over that time, as a fraction of the achievable HBM bandwidth of
    the MI355X (6.3 TB/s: MI355X_MICROARCH.md, 8 TB/s peak, 6.29 TB/s measured with a float4 copy).
(b) the three host-level calls of the classification model on the same batches: `input_attributions`, `encode` (forward
    only, pooled_only: the packed layout the other two run in) and `forward_backward`; ms per call (host clock around N
    calls, synchronised), median and spread over REPS windows.
B / N / REPS / K from the environment override the defaults. Needs the GPU; nothing is measured without one."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stonkgs_amd import _hip as hip  # noqa: E402
from stonkgs_amd.config import STonKGsConfig  # noqa: E402
from stonkgs_amd.data import synthetic_batch  # noqa: E402
from stonkgs_amd.stonkgs_model import STonKGsForSequenceClassification  # noqa: E402

ACHIEVABLE_TBS = 6.3
B, K = int(os.environ.get("B", 64)), int(os.environ.get("K", 175094))
N, REPS = int(os.environ.get("N", 10)), int(os.environ.get("REPS", 5))
N_KERNEL = int(os.environ.get("N_KERNEL", 200))


def kernel_part(model, batch):
    cfg = model.config
    S, half, H = cfg.max_position_embeddings, cfg.half_length, cfg.hidden_size
    ids, mask = batch["input_ids"], batch["attention_mask"]
    g = torch.Generator(device="cuda").manual_seed(0)
    dsum = (torch.randn(B * S, H, device="cuda", generator=g) * 0.01).to(torch.bfloat16)
    text = torch.randn(B * half, H, device="cuda", generator=g).to(torch.bfloat16)
    table = model.kg_backbone.table
    keep = (mask != 0).flatten()
    keep[::S] = True
    row_of_pos = torch.full((B * S,), -1, dtype=torch.int32, device="cuda")
    row_of_pos[keep] = torch.arange(int(keep.sum()), dtype=torch.int32, device="cuda")
    gxi, gn = torch.empty(B * S, device="cuda"), torch.empty(B * S, device="cuda")
    live = {"padded": torch.ones_like(keep), "packed": keep}
    fns = {}
    for layout in live:
        rp = row_of_pos.data_ptr() if layout == "packed" else 0
        fns[layout] = lambda rp=rp: hip.call(
            "stonk_input_attribution", dsum.data_ptr(), H, ids.data_ptr(), text.data_ptr(), table.data_ptr(), table.shape[0],
            rp, 1.0, gxi.data_ptr(), gn.data_ptr(), 0, 0, B, S, half, H, hip.stream_ptr())
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(REPS):
        for layout, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(N_KERNEL):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[layout].append(e0.elapsed_time(e1) / N_KERNEL * 1e3)
    for layout, t in times.items():
        lv = live[layout].view(B, S)
        n_text, n_ent = int(lv[:, :half].sum()), int(lv[:, half:].sum())
        nbytes = n_text * 4 * H + n_ent * (6 * H + 8) + B * S * (8 + (4 if layout == "packed" else 0))
        us = statistics.median(t)
        tbs = nbytes / us / 1e6
        print(json.dumps(dict(kernel="stonk_input_attribution", layout=layout, B=B, S=S, H=H, live_rows=n_text + n_ent,
                              launches=N_KERNEL, windows=REPS, us_median=round(us, 1), us_min=round(min(t), 1),
                              us_max=round(max(t), 1), bytes=nbytes, achieved_TBps=round(tbs, 3),
                              fraction_of_achievable=round(tbs / ACHIEVABLE_TBS, 3), achievable_TBps=ACHIEVABLE_TBS)),
              flush=True)


def host_part(model, batches):
    def attributions(b):
        model.input_attributions(b["input_ids"], b["attention_mask"], b["token_type_ids"], target=b["labels"])

    def encode(b):
        model.encode(b["input_ids"], b["attention_mask"], b["token_type_ids"], pooled_only=True)

    def forward_backward(b):
        model.forward_backward(b)

    variants = dict(input_attributions=attributions, encode=encode, forward_backward=forward_backward)
    model.train()   # (dropout is 0 in the config: forward_backward runs the training path without masks)
    for fn in variants.values():
        for b in batches[:3]:
            fn(b)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(REPS):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(N):
                fn(batches[i % len(batches)])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / N * 1e3)
    model._store.grad.zero_()
    for name, t in times.items():
        print(json.dumps(dict(call=name, B=B, calls_per_window=N, windows=REPS, ms_median=round(statistics.median(t), 3),
                              ms_min=round(min(t), 3), ms_max=round(max(t), 3))), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_attributions.py needs the GPU: nothing is measured without one")
    cfg = STonKGsConfig(kg_vocab_size=K, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_labels=3)
    model = STonKGsForSequenceClassification(cfg, seed=0)
    S = cfg.max_position_embeddings
    batches = []
    for i in range(4):
        b = synthetic_batch(B, cfg.vocab_size, cfg.kg_vocab_size, S, seed=70 + i)
        b = {k: b[k].cuda() for k in ("input_ids", "attention_mask", "token_type_ids")}
        b["labels"] = torch.randint(0, 3, (B,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(i))
        batches.append(b)
    kernel_part(model, batches[0])
    host_part(model, batches)
    model.engine.check_errors()


if __name__ == "__main__":
    main()
