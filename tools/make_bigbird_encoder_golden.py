"""Writes tests/golden/g18_bigbird_<case>.npz / .json: what HuggingFace's own BigBirdModel computes for the cases of
tests/bigbird_encoder_ref.py, in float32 on the CPU, from the installed `transformers` alone.

Per case and mode ("eval"; "train" = train mode at dropout 0): the rand_attn HuggingFace actually used in every layer (the
argument its attention hands to _create_rand_mask_from_inputs), the sequence output at the sampled rows (every 37th and every
masked-query row), the pooled vector, and the gradients of sum(w o seq) + sum(w' o pooled) with respect to inputs_embeds
(a sample of those rows) and, row-sampled, the parameters of bigbird_encoder_ref.grad_names. Weights, inputs and w are regenerated from the case's
seed by bigbird_encoder_ref.case_data: the fixture keeps their SHA-256 only, plus the mask.

    python tools/make_bigbird_encoder_golden.py [case ...]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import bigbird_encoder_ref as er  # noqa: E402


def hf_run(name, mode):
    import transformers

    c = er.CASES[name]
    hf = er.huggingface_run(name, mode, torch.float32)
    H = c["hidden"]
    res = {"seq": hf["seq"].reshape(-1, H).numpy()[er.sample_rows(c).numpy()], "pooled": hf["pooled"].numpy(),
           "loss": np.float64(hf["loss"].item()),
           "grad.inputs_embeds": hf["grads"]["inputs_embeds"].reshape(-1, H).numpy()[er.grad_rows(c).numpy()]}
    for k in er.grad_names(c):
        g = hf["grads"][k]
        res["grad." + k] = er.grad_sample(g[:c["S"]] if k == "embeddings.position_embeddings.weight" else g).numpy()
    for i, ra in enumerate(hf["plans"]):
        res[f"plan.{i}"] = ra
    return res, transformers.__version__


def main(argv):
    os.makedirs(er.GOLDEN, exist_ok=True)
    for name in argv or list(er.CASES):
        c = er.CASES[name]
        arrays, version = {"mask": c["mask"].numpy().astype(np.int8)}, None
        for mode in er.case_modes(name):
            res, version = hf_run(name, mode)
            arrays.update({f"{mode}.{k}": v for k, v in res.items()})
        meta = dict(case=name, S=c["S"], B=c["B"], layers=c["layers"], hidden=c["hidden"], heads=c["heads"], inter=c["inter"],
                    seed=c["seed"], data_sha256=er.data_checksum(name), transformers_version=version,
                    torch_version=torch.__version__, sampled_rows=int(er.sample_rows(c).sum()), modes=list(er.case_modes(name)),
                    grad_names=er.grad_names(c))
        np.savez_compressed(os.path.join(er.GOLDEN, f"g18_bigbird_{name}.npz"), **arrays)
        with open(os.path.join(er.GOLDEN, f"g18_bigbird_{name}.json"), "w") as fh:
            json.dump(meta, fh, indent=2, sort_keys=True)
        size = os.path.getsize(os.path.join(er.GOLDEN, f"g18_bigbird_{name}.npz"))
        print(f"{name}: {len(arrays)} arrays, {size} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
