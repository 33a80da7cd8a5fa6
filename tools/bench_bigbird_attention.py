"""Block-sparse (BigBird) attention against the dense kernels on the same tensors, at ProtSTonKGs' encoder shape: S 4096,
12 heads of 64, B in {1, 2, 4}, a key mask with a masked tail on every second sequence.

Arms: stonk_attention_fwd / _bwd (dense, p = 0: all 64 x 64 key tiles per head), and stonk_block_sparse_attention_fwd / _bwd
with the eval plan (zeros: block 0 four times) and with a drawn plan (3 random blocks). For each: forward, backward, and
both. All arms run in ONE process, interleaved window by window (dense, eval, drawn, dense, ...): N launches per window
between two HIP events, a warm-up first, the median of REPS windows.

Prints one JSON line per (B, arm): tiles visited per launch (64 x 64 query x key tiles, all heads and sequences), us per
forward / backward / both, the ratio to the dense arm, and the fraction of the bf16 MFMA peak (2.5 PFLOP/s dense, spec) that
the VISITED tiles' matrix products amount to - 2 products per tile forward (Q K^T, P V), 7 backward (Q K^T and dO V^T in
both backward kernels, dS K, dS^T Q, P^T dO), 2 * 64^3 FLOP each. B / N / REPS from the environment override the defaults."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stonkgs_amd import _hip as hip  # noqa: E402
from stonkgs_amd.bigbird_attention import BlockSparsePlan, bigbird_rand_attn  # noqa: E402

PEAK_FLOPS = 2.5e15
S, NH = int(os.environ.get("S", 4096)), int(os.environ.get("NH", 12))
N, REPS = int(os.environ.get("N", 20)), int(os.environ.get("REPS", 7))
BATCHES = [int(b) for b in os.environ.get("B", "1,2,4").split(",")]
H, NB = NH * 64, S // 64
TILE_FLOP = 2 * 64 ** 3
PRODUCTS = dict(fwd=2, bwd=7, both=9)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3   # us per launch


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_bigbird_attention.py needs the GPU: nothing is measured without one")
    plans = dict(eval=BlockSparsePlan(NB, bigbird_rand_attn(NB, 3, NH, "eval")),
                 drawn=BlockSparsePlan(NB, bigbird_rand_attn(NB, 3, NH, "train", seed=0)))
    for B in BATCHES:
        g = torch.Generator(device="cuda").manual_seed(B)
        qkv = torch.randn(B * S, 3 * H, device="cuda", generator=g).to(torch.bfloat16)
        dout = torch.randn(B * S, H, device="cuda", generator=g).to(torch.bfloat16)
        mask = torch.ones(B, S, dtype=torch.long, device="cuda")
        mask[1::2, S - 256:] = 0
        out = torch.empty(B * S, H, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(B, NH, S, device="cuda")
        ws = torch.empty(2, B, NH, S, device="cuda")
        dqkv = torch.empty_like(qkv)
        q, d = hip.ptr(qkv), hip.ptr(dqkv)
        head = (q, q + 2 * H, q + 4 * H, 3 * H, hip.ptr(mask))
        grads = (hip.ptr(out), H, hip.ptr(dout), H, hip.ptr(lse), hip.ptr(ws), d, d + 2 * H, 3 * H, d + 4 * H)
        st = hip.stream_ptr()

        def dense_fwd():
            hip.call("stonk_attention_fwd", *head, 0, 0, hip.ptr(out), H, hip.ptr(lse), B, NH, S, 64, 0.125, 0.0, 0, st)

        def dense_bwd():
            hip.call("stonk_attention_bwd", *head, 0, 0, *grads, B, NH, S, 64, 0.125, 0.0, 0, st)

        arms = {"dense": (dense_fwd, dense_bwd, B * NH * NB * NB)}
        for name, plan in plans.items():
            lists, err = plan.on("cuda")
            lp = tuple(hip.ptr(t) for t in lists)

            def sparse_fwd(lp=lp, err=err):
                hip.call("stonk_block_sparse_attention_fwd", *head, *lp[:3], hip.ptr(out), H, hip.ptr(lse), B, NH, S, 64, 0.125,
                         hip.ptr(err), st)

            def sparse_bwd(lp=lp, err=err):
                hip.call("stonk_block_sparse_attention_bwd", *head, *lp, *grads, B, NH, S, 64, 0.125, hip.ptr(err), st)

            arms[name] = (sparse_fwd, sparse_bwd, B * int(plan.tiles().sum()))
        fns = {}
        for name, (fwd, bwd, tiles) in arms.items():
            fns[name, "fwd"], fns[name, "bwd"] = fwd, bwd
            fns[name, "both"] = lambda fwd=fwd, bwd=bwd: (fwd(), bwd())
        for fn in fns.values():          # warm-up: every arm, every shape of the timed windows (bwd after a fwd: a valid lse)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(REPS):            # interleaved: one window of every arm per round
            for k, fn in fns.items():
                times[k].append(window(fn))
        for name, (_, _, tiles) in arms.items():
            row = dict(arm=name, B=B, NH=NH, S=S, tiles=tiles, tile_fraction_of_dense=round(tiles / arms["dense"][2], 4),
                       launches=N, windows=REPS)
            for what in ("fwd", "bwd", "both"):
                us = statistics.median(times[name, what])
                row[what + "_us"] = round(us, 1)
                row[what + "_us_min_max"] = [round(min(times[name, what]), 1), round(max(times[name, what]), 1)]
                row[what + "_ratio_to_dense"] = round(us / statistics.median(times["dense", what]), 3)
                row[what + "_mfma_peak_fraction"] = round(tiles * PRODUCTS[what] * TILE_FLOP / (us * 1e-6) / PEAK_FLOPS, 4)
            print(json.dumps(row), flush=True)
        for plan in plans.values():
            assert int(plan.on("cuda")[1].item()) == 0
        del qkv, dout, out, lse, ws, dqkv


if __name__ == "__main__":
    main()
