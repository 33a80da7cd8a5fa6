"""Evaluation without dense logits, measured (profiles/eval_topk.md):
 (1) stonk_row_topk_f16 alone at the benchmark's label-sparse shapes (fp16 logits [2432, 175104] for the entity head,
     [2432, 29056] for the text head), k = 1 / 10 / 16: us per launch and bytes per second of logits read (each once);
 (2) with --model: `model.evaluate_batch` against the only route there was before it - `model.eval(); model(**batch)`
     (dense fp32 logits) plus torch cross-entropy / top-k / rank on the labelled rows - interleaved in one process at the
     benchmark configuration (B 64, 12 layers, 768 wide, full vocabularies)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stonkgs_amd import _hip as hip  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_alone():
    R = 2432
    for ncols, npad in ((175094, 175104), (28996, 29056)):
        g = torch.Generator(device="cuda").manual_seed(1)
        logits = (torch.randn(R, npad, device="cuda", generator=g) * 3).to(torch.float16)
        tgt = torch.randint(0, ncols, (R,), device="cuda", generator=g, dtype=torch.int32)
        cnt = torch.tensor([R], dtype=torch.int32, device="cuda")
        for k in (1, 10, 16):
            tv, ti = torch.empty(R, k, device="cuda"), torch.empty(R, k, device="cuda", dtype=torch.int32)
            lse, tl = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
            rank = torch.empty(R, device="cuda", dtype=torch.int32)

            def run():
                hip.call("stonk_row_topk_f16", logits.data_ptr(), npad, ncols, tgt.data_ptr(), cnt.data_ptr(), R, k,
                         tv.data_ptr(), ti.data_ptr(), lse.data_ptr(), rank.data_ptr(), tl.data_ptr(), hip.stream_ptr())

            ms = timed(run, 10)
            ref = torch.topk(logits[:64, :ncols].float(), k, dim=1)
            ok = bool(torch.equal(ref.values, tv[:64]))
            print(f"topk alone: {ncols} columns, k {k}: {ms * 1e3:.0f} us, {R * ncols * 2 / ms / 1e9:.2f} TB/s of logits read; "
                  f"values equal torch.topk on 64 rows: {ok}", flush=True)


def model_ab(rounds=5):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.data import synthetic_batch
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    cfg = STonKGsConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = STonKGsForPreTraining(cfg, seed=0)
    batch = {k: v.cuda() for k, v in synthetic_batch(64, cfg.vocab_size, cfg.kg_vocab_size, 512, seed=1234).items()}
    model.eval()

    def new():
        return model.evaluate_batch(batch, k=10)

    def old():
        with torch.no_grad():
            (tl, el), _ = model(**batch)[1:]
        res = {}
        for nm, logits, lab in (("text", tl, batch["masked_lm_labels"]), ("ent", el, batch["ent_masked_lm_labels"])):
            sel = lab != -100
            x, t = logits[sel], lab[sel]
            lse = torch.logsumexp(x, 1)
            xt = x.gather(1, t[:, None])
            res[nm] = dict(nll=lse - xt[:, 0], topk=torch.topk(x, 10, dim=1), rank=(x > xt).sum(1))
        return res

    a, b = new(), old()
    torch.cuda.synchronize()
    for nm in ("text", "ent"):
        print(f"{nm}: nll mean new {float(a[nm]['nll'].mean()):.4f} old {float(b[nm]['nll'].mean()):.4f}; top-1 agreement "
              f"{float((a[nm]['topk_ids'][:, 0] == b[nm]['topk'].indices[:, 0]).float().mean()):.3f}", flush=True)
    tn, to = [], []
    for _ in range(rounds):       # interleaved: A, B, A, B ...
        tn.append(timed(new, 3))
        to.append(timed(old, 3))
    print("evaluate_batch ms per batch of 64:", ["%.2f" % x for x in tn])
    print("eval-mode dense forward + torch CE / top-k / rank on labelled rows, ms:", ["%.2f" % x for x in to], flush=True)


if __name__ == "__main__":
    kernel_alone()
    if "--model" in sys.argv:
        model_ab()
