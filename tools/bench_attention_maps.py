"""stonk_attention_probs alone at the benchmark's encoder shape (B 64, 12 heads, S 512, key-padding mask) and at B 8, in
both output modes: us per launch (HIP events, warm-up + N timed launches, median of REPS such windows) and achieved
bandwidth -
  probs mode       against the bytes the launch must STORE (B * NH * S * S * 4, plus the mass when both are asked for),
  modal_mass mode  against the q and k bytes it must READ (B * S * NH * 64 * 2 * 2)
- as a fraction of the achievable HBM bandwidth of the MI355X, 6.3 TB/s (MI355X_MICROARCH.md: 8 TB/s peak, 6.29 TB/s
measured with a float4 copy; no separate write-only figure is published, so stores are divided by the same number).
Prints one JSON line per case. B / S / NH / N / REPS from the environment override the defaults."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stonkgs_amd import _hip as hip  # noqa: E402

ACHIEVABLE_TBS = 6.3
S, NH = int(os.environ.get("S", 512)), int(os.environ.get("NH", 12))
N, REPS = int(os.environ.get("N", 200)), int(os.environ.get("REPS", 5))
BATCHES = [int(b) for b in os.environ.get("B", "64,8").split(",")]
H = NH * 64


def bytes_needed(B, mode):
    """(bytes the launch must move for its result, what they are)"""
    if mode == "modal_mass":
        return B * S * NH * 64 * 2 * 2, "q + k read"
    return B * NH * S * S * 4 + (B * NH * S * 2 * 4 if mode == "both" else 0), "probabilities stored"


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
        raise SystemExit("bench_attention_maps.py needs the GPU: nothing is measured without one")
    for B in BATCHES:
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B * S, 3 * H, device="cuda", generator=g).to(torch.bfloat16)
        mask = torch.ones(B, S, dtype=torch.long, device="cuda")
        for b in range(B):
            mask[b, 32 + 3 * (b % 64): S // 2] = 0
        probs = torch.empty(B, NH, S, S, device="cuda")
        modal = torch.empty(B, NH, S, 2, device="cuda")
        for mode in ("probs", "both", "modal_mass"):
            def fn():
                hip.call("stonk_attention_probs", hip.ptr(qkv), hip.ptr(qkv) + 2 * H, 3 * H, hip.ptr(mask),
                         hip.ptr(probs) if mode != "modal_mass" else 0, hip.ptr(modal) if mode != "probs" else 0,
                         B, NH, S, 64, S // 2, 0.125, hip.stream_ptr())
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            times = [window(fn) for _ in range(REPS)]
            us = statistics.median(times)
            nbytes, what = bytes_needed(B, mode)
            tbs = nbytes / us / 1e6
            print(json.dumps(dict(kernel="stonk_attention_probs", mode=mode, B=B, NH=NH, S=S, launches=N, windows=REPS,
                                  us_median=round(us, 1), us_min=round(min(times), 1), us_max=round(max(times), 1),
                                  bytes=nbytes, bytes_are=what, achieved_TBps=round(tbs, 3),
                                  fraction_of_achievable=round(tbs / ACHIEVABLE_TBS, 3), achievable_TBps=ACHIEVABLE_TBS)),
                  flush=True)
        del probs, modal, qkv


if __name__ == "__main__":
    main()
