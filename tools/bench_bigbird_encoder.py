"""The BigBird encoder stack at ProtSTonKGs' shape - 12 layers, hidden 768, 12 heads, S 4096, B in {1, 2, 4}, dropout 0 -
forward and forward + backward, against the SAME stack with the dense attention kernels in the place of the block-sparse
ones (everything else equal: gelu_new passes, embeddings, GEMM chain), and the cost of the passes this encoder adds to a
layer: the two gelu_new kernels over [T, I] and the two embeddings kernels.

Timed as tools/bench_bigbird_attention.py times: all arms in ONE process, interleaved window by window, N calls per window
between two HIP events, a warm-up of every arm first, the median of REPS windows (min and max reported). A key mask with a
masked tail on every second sequence; the train-mode (drawn) plans. Prints one JSON line per (B, arm) and per (B, kernel);
`share_of_fwd` / `share_of_both` = a kernel's time x launches per stack / the block-sparse stack's time.
LAYERS / S / B / N / REPS from the environment override the defaults."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stonkgs_amd import _hip as hip  # noqa: E402
from stonkgs_amd.bigbird_encoder import BigBirdEncoderConfig, BigBirdEncoderModel, BigBirdEngine  # noqa: E402
from stonkgs_amd.layer_engine import LayerEngine  # noqa: E402

LAYERS, S = int(os.environ.get("LAYERS", 12)), int(os.environ.get("S", 4096))
N, REPS = int(os.environ.get("N", 3)), int(os.environ.get("REPS", 5))
BATCHES = [int(b) for b in os.environ.get("B", "1,2,4").split(",")]


class DenseAttentionEngine(BigBirdEngine):
    """The comparison arm: the dense attention core (no probability dropout), everything else the encoder's."""
    _attention_fwd = LayerEngine._attention_fwd
    _attention_bwd = LayerEngine._attention_bwd


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n   # ms per call


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_bigbird_encoder.py needs the GPU: nothing is measured without one")
    cfg = BigBirdEncoderConfig(num_hidden_layers=LAYERS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=64)
    model = BigBirdEncoderModel(cfg)
    model.train()
    H, I = cfg.hidden_size, cfg.intermediate_size
    engines = {"block_sparse": model.engine, "dense": DenseAttentionEngine(cfg, model._store, model.device)}
    plans = [model.plan_for(i, S // 64) for i in range(LAYERS)]
    st = hip.stream_ptr()
    for B in BATCHES:
        T = B * S
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, S, H, device="cuda", generator=g)
        dseq = torch.randn(B, S, H, device="cuda", generator=g)
        dpooled = torch.randn(B, H, device="cuda", generator=g)
        d_in = torch.empty_like(x)
        mask = torch.ones(B, S, dtype=torch.long, device="cuda")
        mask[1::2, S - 256:] = 0
        fns = {}
        for name, eng in engines.items():
            def fwd(eng=eng):
                eng.encode_embeds(x, mask, None, plans, False, None)

            def both(eng=eng):
                sv = {}
                eng.encode_embeds(x, mask, None, plans, True, sv)
                eng.backward_embeds(dseq, dpooled, sv, d_in)

            fns[name, "fwd"], fns[name, "both"] = fwd, both
        # the added passes alone, on buffers of the stack's shapes
        u = torch.randn(T, I, device="cuda", generator=g).to(torch.bfloat16)
        gg, dg = torch.empty_like(u), torch.randn(T, I, device="cuda", generator=g).to(torch.bfloat16)
        bf = lambda: torch.empty(T, H, device="cuda", dtype=torch.bfloat16)      # noqa: E731
        so, y, dxm, dsum = bf(), bf(), bf(), torch.randn(T, H, device="cuda", generator=g).to(torch.bfloat16)
        stats = torch.empty(2, T, device="cuda")
        P = model._store.view
        kernels = {
            "gelu_new_fwd": (lambda: hip.call("stonk_gelu_new_fwd_bf16", u.data_ptr(), gg.data_ptr(), T * I, st), LAYERS, "fwd"),
            "gelu_new_bwd": (lambda: hip.call("stonk_gelu_new_bwd_bf16", dg.data_ptr(), u.data_ptr(), gg.data_ptr(), T * I, st),
                             LAYERS, "bwd"),
            "embeds_ln_fwd": (lambda: hip.call(
                "stonk_embeds_ln_fwd", x.data_ptr(), H, 0, P("bert.embeddings.position_embeddings.weight").data_ptr(),
                P("bert.embeddings.token_type_embeddings.weight").data_ptr(), P("bert.embeddings.LayerNorm.weight").data_ptr(),
                P("bert.embeddings.LayerNorm.bias").data_ptr(), so.data_ptr(), y.data_ptr(), stats[0].data_ptr(),
                stats[1].data_ptr(), B, S, H, 2, 1e-12, 0.0, 1, st), 1, "fwd"),
            "embeds_ln_bwd_finish": (lambda: hip.call("stonk_embeds_ln_bwd_finish", dsum.data_ptr(), H, d_in.data_ptr(), H,
                                                      dxm.data_ptr(), T, H, 0.0, 1, st), 1, "bwd"),
        }
        for fn in list(fns.values()) + [k[0] for k in kernels.values()]:      # warm-up: every arm, every kernel
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        ktimes = {k: [] for k in kernels}
        for _ in range(REPS):            # interleaved: one window of every arm per round
            for k, fn in fns.items():
                times[k].append(window(fn, N))
            for k, (fn, _, _) in kernels.items():
                ktimes[k].append(window(fn, 20))
        med = {k: statistics.median(v) for k, v in times.items()}
        for name in engines:
            row = dict(arm=name, B=B, S=S, layers=LAYERS, hidden=H, calls_per_window=N, windows=REPS)
            for what in ("fwd", "both"):
                ms = med[name, what]
                row[what + "_ms"] = round(ms, 3)
                row[what + "_ms_per_layer"] = round(ms / LAYERS, 3)
                row[what + "_ms_min_max"] = [round(min(times[name, what]), 3), round(max(times[name, what]), 3)]
                row[what + "_ratio_to_dense"] = round(ms / med["dense", what], 3)
            print(json.dumps(row), flush=True)
        for k, (_, launches, where) in kernels.items():
            ms = statistics.median(ktimes[k])
            row = dict(kernel=k, B=B, S=S, us=round(ms * 1e3, 1), us_min_max=[round(min(ktimes[k]) * 1e3, 1), round(max(ktimes[k]) * 1e3, 1)],
                       launches_per_stack=launches, share_of_both=round(ms * launches / med["block_sparse", "both"], 4))
            if where == "fwd":
                row["share_of_fwd"] = round(ms * launches / med["block_sparse", "fwd"], 4)
            print(json.dumps(row), flush=True)
        for eng in engines.values():
            eng.check_errors()
        del x, dseq, d_in, u, gg, dg, so, y, dxm, dsum
        for eng in engines.values():
            eng.ws.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
