"""Text-only baseline on the MI355X: what the word-embedding gradient kernel costs, and the fine-tuning step / eval forward
against eager PyTorch.

  python tools/bench_text_baseline.py [--steps 20] [--rounds 3] [--layers 12]

Prints one JSON line per measurement:
  kernel   stonk_word_embed_grad alone at B = 16, S = 512, H = 768, vocab = 28 996 - token ids from a Zipf-like distribution
           plus [CLS] / [SEP] per row, every position live (the upper bound of a step) - as added bytes / s, beside the
           chip-wide float-atomic rate the kernel was budgeted with (~1.3 TB/s) and beside torch.index_add_ on the same input
           (from the bf16 rows as the kernel reads them, and from rows already cast to fp32);
  kernel_in_step   the same kernel on the step's own batches (text lengths 32-512, padded positions dropped);
  step / eval      the whole fine-tuning step (forward, backward, clip, AdamW) and the eval forward at batch 16 through the
           HIP path, against the eager torch forward / backward / clip / AdamW of the fp32 restatement that
           tests/test_text_embed_cpu.py pins to transformers' BertForSequenceClassification, moved to the GPU under bf16
           autocast, on the same batches, in alternating rounds; and the kernel's share of the HIP step.
Times are host clocks around work that ends in a device synchronise (steps) or device events (the kernel)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMIC_RATE = 1.3e12   # bytes / s of fp32 adds, chip-wide (the budget figure of the kernel's design)
CLS, SEP = 101, 102


def zipf_ids(B, S, vocab, seed=0):
    """[B, S] token ids: rank r drawn with p ~ 1 / r, ranks spread over the word pieces (ids 1000 ...), [CLS] first and
    [SEP] last in every row."""
    g = torch.Generator().manual_seed(seed)
    n_rank = vocab - 1000
    w = 1.0 / torch.arange(1, n_rank + 1, dtype=torch.float64)
    ids = 1000 + torch.multinomial(w, B * S, replacement=True, generator=g).view(B, S)
    ids[:, 0], ids[:, -1] = CLS, SEP
    return ids


def event_time(fn, warmup=5, iters=50):
    """Seconds per call: `iters` calls between two device events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def bench_kernel(hip, ids, row_of_pos, H, vocab, rounds, tag):
    dev = "cuda"
    B, S = ids.shape
    ids_d = ids.to(dev).contiguous()
    rop = None if row_of_pos is None else row_of_pos.to(dev)
    live = torch.ones(B * S, dtype=torch.bool) if row_of_pos is None else row_of_pos >= 0
    live &= ids.view(-1) != 0
    n_rows = int((row_of_pos.max() + 1) if row_of_pos is not None else B * S)
    dsum = torch.randn(n_rows, H, device=dev).to(torch.bfloat16)
    dword = torch.zeros(vocab, H, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    src_rows = (torch.arange(B * S) if row_of_pos is None else row_of_pos.long())[live].to(dev)
    dst = ids.view(-1)[live].to(dev)
    dsum32 = dsum.float()

    def kernel():
        hip.call("stonk_word_embed_grad", dsum.data_ptr(), H, ids_d.data_ptr(), hip.ptr(rop), dword.data_ptr(), H, vocab, 0,
                 B, S, H, err.data_ptr(), hip.stream_ptr())

    def index_add_bf16():
        dword.index_add_(0, dst, dsum[src_rows].float())

    def index_add_f32():
        dword.index_add_(0, dst, dsum32[src_rows])

    t = {"kernel": [], "index_add_from_bf16": [], "index_add_from_f32": []}
    for _ in range(rounds):   # alternating
        t["kernel"].append(event_time(kernel))
        t["index_add_from_bf16"].append(event_time(index_add_bf16))
        t["index_add_from_f32"].append(event_time(index_add_f32))
    assert int(err.item()) == 0
    added = int(live.sum()) * H * 4
    counts = torch.bincount(ids.view(-1)[live])
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(what=tag, B=B, S=S, H=H, vocab=vocab, contributing_rows=int(live.sum()), added_bytes=added,
               max_rows_per_destination=int(counts.max()), destinations=int((counts > 0).sum()),
               kernel_us=med["kernel"] * 1e6, kernel_us_rounds=[x * 1e6 for x in t["kernel"]],
               kernel_added_GBps=added / med["kernel"] / 1e9, atomic_rate_budget_GBps=ATOMIC_RATE / 1e9,
               share_of_atomic_rate=added / med["kernel"] / ATOMIC_RATE,
               index_add_from_bf16_us=med["index_add_from_bf16"] * 1e6, index_add_from_f32_us=med["index_add_from_f32"] * 1e6)
    print(json.dumps(out), flush=True)
    return med["kernel"]


def make_batches(n, B, S, vocab, num_labels, seed=1):
    """`n` batches [B, Lmax] (Lmax = the longest text of the batch, as the reference pads): text lengths uniform in
    [32, S], Zipf-like ids, [CLS] ... [SEP], then [PAD] with mask 0."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        lens = torch.randint(32, S + 1, (B,), generator=g)
        L = int(lens.max())
        ids = zipf_ids(B, L, vocab, seed=seed + 100 + i)
        am = (torch.arange(L)[None] < lens[:, None]).long()
        ids[torch.arange(B), lens - 1] = SEP
        ids = ids * am
        out.append({"input_ids": ids, "attention_mask": am, "token_type_ids": torch.zeros_like(ids),
                    "labels": torch.randint(0, num_labels, (B,), generator=g)})
    return out


def packed_row_of_pos(am, S):
    """Position -> packed row for a [B, L] mask right-padded to S: attended positions and position 0 keep a row."""
    B, L = am.shape
    keep = torch.zeros(B, S, dtype=torch.bool)
    keep[:, :L] = am != 0
    keep[:, 0] = True
    flat = keep.view(-1)
    return torch.where(flat, torch.cumsum(flat.long(), 0) - 1, -1).to(torch.int32)


def timed_rounds(fns, steps, rounds):
    """{name: median seconds per call}: `rounds` alternating rounds of `steps` calls each, after one warm-up round."""
    for fn in fns.values():
        for _ in range(3):
            fn(0)
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                fn(i)
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / steps)
    return {k: statistics.median(v) for k, v in t.items()}, t


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_baseline needs an MI355X: there is nothing to measure without one")

    from oracle import stonkgs_oracle as orc
    from stonkgs_amd import _hip as hip
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.nlp_baseline_model import BertForSequenceClassification
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments
    from tests.test_text_embed_cpu import text_classifier

    B, S, H, V, C = args.batch, 512, 768, 28996, 3
    hip.lib()
    # ---- the kernel alone
    t_kernel_full = bench_kernel(hip, zipf_ids(B, S, V), None, H, V, args.rounds, "kernel")
    batches = make_batches(4, B, S, V, C)
    t_in_step = []
    for i, b in enumerate(batches[:2]):
        ids = torch.nn.functional.pad(b["input_ids"], (0, S - b["input_ids"].shape[1]))
        t_in_step.append(bench_kernel(hip, ids, packed_row_of_pos(b["attention_mask"], S), H, V, args.rounds,
                                      f"kernel_in_step[{i}]"))
    t_in_step = statistics.mean(t_in_step)

    # ---- the whole step and the eval forward, HIP against eager
    dims = dict(vocab_size=V, hidden_size=H, num_hidden_layers=args.layers, num_attention_heads=12, intermediate_size=3072,
                max_position_embeddings=S)
    ocfg = orc.OracleConfig(**dims, kg_vocab_size=8, backbone_layers=0)
    sd = {k: v for k, v in orc.init_state_dict(ocfg, seed=3).items() if k.startswith("bert.")}
    sd["classifier.weight"] = torch.randn(C, H) * 0.02
    sd["classifier.bias"] = torch.zeros(C)
    models, trainers = {}, {}
    for p in (0.1, 0.0):
        m = BertForSequenceClassification(STonKGsConfig(**dims, hidden_dropout_prob=p, attention_probs_dropout_prob=p),
                                          num_labels=C)
        m.load_state_dict(sd)
        models[p] = m
        trainers[p] = Trainer(m, TrainingArguments(learning_rate=5e-5, max_steps=100000, per_device_train_batch_size=B))
    dev_batches = [{k: v.cuda() for k, v in b.items()} for b in batches]
    params = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=5e-5, weight_decay=0.0)

    def eager_step(i):
        b = dev_batches[i % len(dev_batches)]
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = text_classifier(params, ocfg, b["input_ids"], b["attention_mask"], b["token_type_ids"], b["labels"])
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
        opt.step()
        return out["loss"]

    def eager_eval(i):
        b = dev_batches[i % len(dev_batches)]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return text_classifier(params, ocfg, b["input_ids"], b["attention_mask"], b["token_type_ids"])["logits"]

    def hip_step(p):
        return lambda i: trainers[p].training_step(models[p], dev_batches[i % len(dev_batches)])

    def hip_eval(i):
        b = dev_batches[i % len(dev_batches)]
        with torch.no_grad():
            return models[0.0](b["input_ids"], b["attention_mask"], b["token_type_ids"])[0]

    # same weights, dropout off: the two paths must agree before their times are compared
    models[0.0].eval()
    b0 = dev_batches[0]
    with torch.no_grad():
        l_hip = float(models[0.0](**b0)[0])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            l_eager = float(text_classifier(params, ocfg, b0["input_ids"], b0["attention_mask"], b0["token_type_ids"],
                                            b0["labels"])["loss"])
    med, raw = timed_rounds({"hip_eval": hip_eval, "eager_eval": eager_eval}, args.steps, args.rounds)
    print(json.dumps(dict(what="eval", layers=args.layers, batch=B, loss_hip=l_hip, loss_eager_bf16=l_eager,
                          hip_ms=med["hip_eval"] * 1e3, eager_bf16_autocast_ms=med["eager_eval"] * 1e3,
                          speedup=med["eager_eval"] / med["hip_eval"],
                          rounds_ms={k: [x * 1e3 for x in v] for k, v in raw.items()})), flush=True)
    med, raw = timed_rounds({"hip_p0.1": hip_step(0.1), "hip_p0": hip_step(0.0), "eager_p0": eager_step}, args.steps,
                            args.rounds)
    for m in models.values():
        m.engine.check_errors()
    print(json.dumps(dict(what="step", layers=args.layers, batch=B, hip_dropout_0p1_ms=med["hip_p0.1"] * 1e3,
                          hip_dropout_0_ms=med["hip_p0"] * 1e3, eager_bf16_autocast_dropout_0_ms=med["eager_p0"] * 1e3,
                          speedup_like_for_like=med["eager_p0"] / med["hip_p0"],
                          word_embed_grad_us_in_step=t_in_step * 1e6, word_embed_grad_us_every_position_live=t_kernel_full * 1e6,
                          kernel_share_of_step=t_in_step / med["hip_p0.1"],
                          kernel_share_of_step_upper_bound=t_kernel_full / med["hip_p0.1"],
                          rounds_ms={k: [x * 1e3 for x in v] for k, v in raw.items()})), flush=True)


if __name__ == "__main__":
    main()
