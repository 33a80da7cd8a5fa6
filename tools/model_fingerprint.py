"""Fingerprint of the three model classes at the smallest shape the kernels accept, for a refactor of the Python
layer: what one commit computes, to be compared with what another computes (profiles/model_layer.md).

  python tools/model_fingerprint.py --out DIR/NAME     writes NAME.json (keys, hashes, losses, norms, entry names) and
                                                       NAME.npz (the arrays behind the hashes that atomics may move)
  python tools/model_fingerprint.py --compare A B [..] --branch C [..]    runs of the parent against runs of the branch

For each of STonKGsForPreTraining, STonKGsForSequenceClassification and BertForSequenceClassification, with a fixed seed
and a fixed batch: the state-dict keys in order, the sha256 of every tensor right after construction, the sha256 of the
eval-mode forward outputs, the loss of one ``Trainer.training_step``, the L2 norm of every gradient view after it (the
fused AdamW has zeroed what it does not keep) and after one further ``forward_backward`` (the gradients themselves), the
sha256 of the flat parameter buffer after the step, and the names that went through ``_hip.call`` during the step.
``--compare``: a field all parent runs agree on must be identical on the branch (exit status 1 otherwise); where the
parent differs from itself, the parent-to-parent and the branch-to-parent differences are printed side by side. Two
runs can agree by chance on a value that atomics accumulate: a further parent run settles such a field."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = dict(vocab_size=512, kg_vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
            intermediate_size=128, max_position_embeddings=256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
B, NUM_LABELS, SEED = 3, 3, 11


def _sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()   # (fp32 / int64 tensors only)


def _flatten(out, prefix="out"):
    """(name, tensor) of every tensor in a nested tuple of forward outputs."""
    import torch

    if torch.is_tensor(out):
        yield prefix, out
    elif isinstance(out, (tuple, list)):
        for i, o in enumerate(out):
            yield from _flatten(o, f"{prefix}.{i}")


def _cases():
    import torch

    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.data import synthetic_batch
    from stonkgs_amd.nlp_baseline_model import BertForSequenceClassification
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining, STonKGsForSequenceClassification

    rows = torch.randn(300, 128, generator=torch.Generator().manual_seed(SEED + 1), dtype=torch.float64) * 0.3
    pre = synthetic_batch(B, 512, 300, 256, seed=SEED + 2, min_text=16)
    labels = torch.tensor([2, 0, 1])
    cls = {k: pre[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    cls["labels"] = labels
    g = torch.Generator().manual_seed(SEED + 3)
    lengths = torch.tensor([256, 100, 17])
    text = {"input_ids": torch.randint(1, 512, (B, 256), generator=g),
            "attention_mask": (torch.arange(256)[None, :] < lengths[:, None]).long(),
            "token_type_ids": torch.zeros(B, 256, dtype=torch.long), "labels": labels}
    text["input_ids"] = text["input_ids"] * text["attention_mask"]
    yield "STonKGsForPreTraining", lambda: STonKGsForPreTraining(STonKGsConfig(**DIMS), kg_embeddings=rows, seed=SEED), pre
    yield ("STonKGsForSequenceClassification",
           lambda: STonKGsForSequenceClassification(STonKGsConfig(**DIMS, num_labels=NUM_LABELS), kg_embeddings=rows,
                                                    seed=SEED), cls)
    yield ("BertForSequenceClassification",
           lambda: BertForSequenceClassification(STonKGsConfig(**DIMS), num_labels=NUM_LABELS, seed=SEED), text)


def fingerprint(out: str) -> None:
    import torch

    from stonkgs_amd import _hip
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    names = []
    real_call = _hip.call

    def recording_call(name, *args):
        names.append(name)
        return real_call(name, *args)

    res, arrays = {}, {}
    for cname, make, batch in _cases():
        model = make()
        r = res[cname] = {}
        sd = model.state_dict()
        r["keys"] = list(sd.keys())
        r["named_parameters"] = [n for n, _ in model.named_parameters()]
        r["init_sha256"] = {k: _sha(v) for k, v in sd.items()}
        model.eval()
        with torch.no_grad():
            outs = dict(_flatten(model(**batch)))
        r["eval_sha256"] = {k: _sha(v) for k, v in outs.items()}
        for k, v in outs.items():
            arrays[f"{cname}/eval/{k}"] = v.float().cpu().numpy()
        model.train()
        trainer = Trainer(model, TrainingArguments(per_device_train_batch_size=B, max_steps=10, learning_rate=1e-3))
        del names[:]
        _hip.call = recording_call
        try:
            loss = trainer.training_step(model, batch)
            torch.cuda.synchronize()
        finally:
            _hip.call = real_call
        model.engine.check_errors()
        r["step_entries"] = list(names)
        r["step_loss"] = float(loss).hex()
        r["grad_norms_after_step"] = {k: float(v.double().norm()).hex() for k, v in model.named_grad_views().items()}
        r["params_after_step_sha256"] = _sha(model._store.data)
        arrays[f"{cname}/params_after_step"] = model._store.data.cpu().numpy()
        loss2 = model.forward_backward(batch)
        torch.cuda.synchronize()
        model.engine.check_errors()
        r["second_loss"] = float(loss2).hex()
        r["grad_norms_after_forward_backward"] = {k: float(v.double().norm()).hex()
                                                  for k, v in model.named_grad_views().items()}
        del trainer, model
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    np.savez(out + ".npz", **arrays)
    print(f"wrote {out}.json and {out}.npz")


# ---------------------------------------------------------------------------------------------------- comparison
def _leaves(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _leaves(v, f"{prefix}{k}/")
        else:
            yield prefix + k, v


def _delta(field: str, x, y, ax, ay) -> tuple:
    """(how far two values of a field are apart, their size): floats by |x - y| and |x|, hashed arrays by max |x - y| and
    max |x| of the saved arrays."""
    cname, _, rest = field.partition("/")
    key = None
    if rest.startswith("eval_sha256/"):
        key = f"{cname}/eval/{rest[len('eval_sha256/'):]}"
    elif rest == "params_after_step_sha256":
        key = f"{cname}/params_after_step"
    if key is not None:
        a, b = ax[key].astype(np.float64), ay[key].astype(np.float64)
        return float(np.abs(a - b).max()), float(np.abs(a).max())
    if isinstance(x, str) and isinstance(y, str):
        fx, fy = float.fromhex(x), float.fromhex(y)
        return abs(fx - fy), abs(fx)
    return float("inf"), 1.0


def compare(parents, branches) -> int:
    def load(paths):
        return [(dict(_leaves(json.load(open(p + ".json")))), np.load(p + ".npz")) for p in paths]

    P, Br = load(parents), load(branches)
    same = moved = 0
    bad, groups = [], {}
    for field in sorted(set().union(*(r for r, _ in P + Br))):
        pv = [r.get(field) for r, _ in P]
        if all(v == pv[0] for v in pv):
            same += 1
            for (r, _), path in zip(Br, branches):
                if r.get(field) != pv[0]:
                    bad.append(field)
                    print(f"BRANCH DIFFERS where the parent runs agree: {field}: {pv[0]!r} -> {r.get(field)!r} ({path})")
        else:   # one row per class and kind of field. The gradient views of a class share one, measured against the
            moved += 1   # largest of their norms: a gradient that is zero but for rounding (a key bias) has no scale of its own
            parts = field.split("/")
            g = groups.setdefault("/".join(parts[:2]) + ("/*" if len(parts) > 2 else ""), [0, 0.0, 0.0, 0.0])
            g[0] += 1
            for col, pairs in ((1, [(x, y) for i, x in enumerate(P) for y in P[i + 1:]]), (2, [(x, y) for x in P for y in Br])):
                for x, y in pairs:
                    d, size = _delta(field, x[0].get(field), y[0].get(field), x[1], y[1])
                    g[col], g[3] = max(g[col], d), max(g[3], size)
    print(f"{same} fields identical in the {len(P)} parent runs; the {len(Br)} branch run(s) differ in {len(set(bad))} of them")
    print(f"{moved} fields differ among the parent runs (atomic accumulation); largest difference per group:")
    print("| fields | count | largest value | parent - parent | branch - parent |\n|---|---|---|---|---|")
    for name, (n, pp, bp, size) in groups.items():
        print(f"| {name} | {n} | {size:.3e} | {pp:.2e} | {bp:.2e} |")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="path without extension: writes .json and .npz")
    ap.add_argument("--compare", nargs="+", metavar="PARENT", help="two or more runs of the parent (paths without extension)")
    ap.add_argument("--branch", nargs="+", metavar="BRANCH", help="with --compare: one or more runs of the branch")
    a = ap.parse_args()
    if a.compare:
        if len(a.compare) < 2 or not a.branch:
            ap.error("--compare takes at least two parent runs and --branch at least one branch run")
        sys.exit(compare(a.compare, a.branch))
    if not a.out:
        ap.error("--out or --compare")
    fingerprint(a.out)
