"""The whole training step with dropout ON (p = 0.1: what bench.py measures and a user trains in) against the oracle with the
step's exact keep-masks, element by element: every loss term and every gradient tensor.

The per-kernel parity tests pin what a kernel drops given (seed, row, column). What they cannot see is the bookkeeping the
engine owns: which (layer, site) seed a launch gets, whether the backward re-draws the forward's mask, which row index keys
the mask once rows are packed or pruned, the prefetched backbone forward drawing the consuming step's masks, and the counter
across optimizer steps. tests/step_dropout_ref.py restates that contract without importing the engine;
oracle/stonkgs_oracle.py (`dropout=`) multiplies the masks in where the engine does, and torch autograd gives the exact
gradients. tests/test_step_dropout_ref_cpu.py proves on the CPU that ten single mistakes in that bookkeeping each move at
least one compared quantity by three times its tolerance here.

Tolerances. Loss terms: |d| < 1e-2 (tests/test_model_gpu.py). Gradients: relative L2 per tensor (absolute scale for an
analytically zero reference, as test_model_gpu._rel), as a multiple of the oracle's OWN bf16-autocast error under the same
masks (r16, against its fp64 run) - held to ENVELOPE, the project's recorded multiple (test_shape_true_gpu._GRAD_ENVELOPE).
profiles/step_dropout_parity.md holds the figures this file prints on MI355X at p = 0.1 and p = 0."""
import numpy as np
import pytest
import torch

from oracle import stonkgs_oracle as orc
from tests import step_dropout_ref as R
from tests.golden_util import load_case

pytestmark = pytest.mark.gpu

# err_HIP / r16 per gradient tensor: the median over tensors and the worst tensor (test_shape_true_gpu._GRAD_ENVELOPE)
ENVELOPE = {"median": 2.8, "max": 3.6}
P = 0.1
SEED_BASE = 0x2468          # the counter BEFORE the step; the step runs under SEED_BASE + 1
B = 4
_CFG_KEYS = ("vocab_size", "kg_vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size",
             "max_position_embeddings", "type_vocab_size", "layer_norm_eps")


def _build(cfg, sd, tsv_rows, p, cls=None, **kw):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    c = STonKGsConfig(**{k: getattr(cfg, k) for k in _CFG_KEYS}, hidden_dropout_prob=p, attention_probs_dropout_prob=p, **kw)
    model = (cls or STonKGsForPreTraining)(c, kg_embeddings=tsv_rows)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("decoder" in k for k in missing), (missing, unexpected)
    return model


@pytest.fixture(scope="module")
def case(hip):
    from tests.test_unpad_gpu import _batches

    cfg, sd, tsv_rows, _, _, _ = load_case("g2_hipsmall")
    with torch.no_grad():
        table = orc.build_kg_table(tsv_rows, orc.special_vectors(sd, cfg))
    return dict(cfg=cfg, sd=sd, sd64=R.to64(sd), tsv_rows=tsv_rows, table=table, batches=_batches(cfg, B), refs={})


def _reference(case, bi, layout, p, seed_base=SEED_BASE + 1):
    """(fp64 loss terms, fp64 gradients, r16 per tensor) of batch `bi` under the masks of `layout` - computed once."""
    key = (bi, layout, p, seed_base)
    if key not in case["refs"]:
        cfg, batch = case["cfg"], case["batches"][bi]
        prov = R.StepDropout(cfg, batch, seed_base, layout, p, p) if p > 0 else None
        terms, g64 = R.oracle_step(case["sd64"], cfg, case["table"], batch, prov)
        _, g16 = R.oracle_step(case["sd"], cfg, case["table"], batch, prov, autocast=True)
        case["refs"][key] = (terms, g64, {k: R.rel(g16[k], g64[k]) for k in g64})
    return case["refs"][key]


def _step(model, batch, layout, seed_base=SEED_BASE):
    e = model.engine
    e.unpad, e.prune_last_ffn, e.prune_last_attn = layout
    e.seed_base = seed_base
    model.train()
    model.zero_grad()
    loss = float(model.forward_backward(batch))
    e.join_wgrad()
    e.check_errors()
    torch.cuda.synchronize()
    assert e.seed_base == seed_base + 1
    terms = dict(zip(R.TERMS, [loss] + [float(t) for t in model.last_loss_terms]))
    return terms, {k: v.detach().cpu().clone() for k, v in model.named_grad_views().items()}


@pytest.fixture(scope="module")
def models(case):
    return {p: _build(case["cfg"], case["sd"], case["tsv_rows"], p) for p in (P, 0.0)}


# ------------------------------------------------------------------------------------------ (a) one step, four layouts
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=lambda l: "".join("FT"[int(x)] for x in l))
def test_step_with_dropout_matches_the_masked_oracle(case, models, layout):
    """forward_backward at p_hid = p_att = 0.1 in the layout (unpad, prune_last_ffn, prune_last_attn), both batches of
    test_unpad_gpu._batches (a hole in a text mask, masked entity positions, a sequence without a live key, one all live):
    loss terms and every gradient tensor against the fp64 oracle under the step's own masks. The p = 0 figures of the same
    layout are printed beside them: dropout must not cost precision."""
    fails = {}
    for bi, batch in enumerate(case["batches"]):
        for p in (0.0, P):
            ref_terms, g64, r16 = _reference(case, bi, layout, p)
            terms, grads = _step(models[p], batch, layout)
            assert set(grads) <= set(g64), set(grads) - set(g64)
            print(R.describe(f"layout {layout} batch {bi} p {p}", grads, g64, r16),
                  "| loss terms |d|", [f"{abs(terms[k] - ref_terms[k]):.2e}" for k in R.TERMS])
            bad = R.compare(terms, grads, ref_terms, g64, r16, ENVELOPE)
            if bad:
                fails[(bi, p)] = bad
    assert not fails, fails


def test_the_comparison_rejects_wrong_masks(case, models):
    """The harness can fail: the real GPU step (default layout) against an oracle whose masks make ONE mistake - the counter
    off by one, padded row indices in the packed layout, a backward mask at site 2 that is not the forward's."""
    layout, batch = (True, True, True), case["batches"][1]
    terms, grads = _step(models[P], batch, layout)
    ref_terms, g64, r16 = _reference(case, 1, layout, P)
    assert not R.compare(terms, grads, ref_terms, g64, r16, ENVELOPE)
    for name, kw in (("seed_base + 1", dict(seed_base=SEED_BASE + 2)), ("padded rows", dict(rows="padded")),
                     ("backward mask, site 2", dict(backward_seed_delta={(0, 2): 1}))):
        sb = kw.pop("seed_base", SEED_BASE + 1)
        mutant = R.StepDropout(case["cfg"], batch, sb, layout, P, P, **kw)
        m_terms, m64 = R.oracle_step(case["sd64"], case["cfg"], case["table"], batch, mutant)
        bad = R.compare(terms, grads, m_terms, m64, r16, ENVELOPE)
        print(name, "->", len(bad), "violations, e.g.", bad[:2])
        assert bad, name


# ------------------------------------------------------------------------------------------ (b) the autograd bridge
def test_autograd_bridge_with_dropout_matches_the_masked_oracle(case):
    """loss = model(**batch)[0]; loss.backward() at p = 0.1 with dense logits: the padded layout."""
    batch, layout = case["batches"][0], (False, False, False)
    model = _build(case["cfg"], case["sd"], case["tsv_rows"], P)
    model.materialize_logits = True
    model.train()
    model.zero_grad()
    model.engine.seed_base = SEED_BASE
    before = list(model.engine.rows_executed)
    out = model(**batch)
    after = model.engine.rows_executed
    assert after[0] - before[0] == after[1] - before[1] == B * case["cfg"].max_position_embeddings   # padded
    assert out[1][0].shape == (B, case["cfg"].half_length, case["cfg"].vocab_size)
    out[0].backward()
    model.engine.join_wgrad()
    model.engine.check_errors()
    torch.cuda.synchronize()
    assert model.engine.seed_base == SEED_BASE + 1
    terms = dict(zip(R.TERMS, [float(out[0].detach())] + [float(t) for t in model.last_loss_terms]))
    grads = {k: v.detach().cpu().clone() for k, v in model.named_grad_views().items()}
    ref_terms, g64, r16 = _reference(case, 0, layout, P)
    print(R.describe("autograd bridge, padded, p 0.1", grads, g64, r16))
    bad = R.compare(terms, grads, ref_terms, g64, r16, ENVELOPE)
    assert not bad, bad


# ------------------------------------------------------------------------------------------ (c) three Trainer steps
def test_three_trainer_steps_with_dropout_match_the_masked_oracle(case):
    """Trainer steps at p = 0.1 with the optimizer on its own stream and the next batch hinted (steps 2 and 3 consume a
    prefetched backbone forward, drawn one step early with the CONSUMING step's masks) against orc.train_step under the
    masks of step 1, 2, 3; then the same run without prefetch."""
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    cfg, sd, batches = case["cfg"], case["sd"], case["batches"]
    runs = {}
    for prefetch in (True, False):
        model = _build(cfg, sd, case["tsv_rows"], P)
        model.engine.seed_base = SEED_BASE
        layout = (model.engine.unpad, model.engine.prune_last_ffn, model.engine.prune_last_attn)
        assert layout == (True, True, True)
        tr = Trainer(model, TrainingArguments(max_steps=10, learning_rate=1e-3, per_device_train_batch_size=B,
                                              optimizer_overlap=True, prefetch_backbone=prefetch))
        dev = [{k: v.cuda() for k, v in b.items()} for b in batches]
        losses = []
        for i in range(3):
            nxt = dev[(i + 1) % 2] if prefetch and i < 2 else None
            if prefetch and i > 0:
                assert model.engine._prefetch is not None      # this step consumes a prefetched backbone forward
            losses.append(float(tr.training_step(model, dev[i % 2], next_inputs=nxt)))
        model.engine.check_errors()
        assert model.engine.seed_base == SEED_BASE + 3
        runs[prefetch] = (losses, {k: v.detach().cpu().clone() for k, v in model.named_parameters()})
    osd = {k: v.clone() for k, v in case["sd64"].items()}
    state = orc.AdamState()
    ref = []
    for i in range(3):
        prov = R.StepDropout(cfg, batches[i % 2], SEED_BASE + 1 + i, (True, True, True), P, P)
        ref.append(float(orc.train_step(osd, cfg, case["table"], batches[i % 2], state, base_lr=1e-3, max_steps=10,
                                        dropout=prov)["loss"]))
    got, params = runs[True]
    print("trainer losses", got, "oracle", ref, "without prefetch", runs[False][0])
    assert np.abs(np.array(got) - np.array(ref)).max() < 1e-2, (got, ref)
    for k in ("bert.encoder.layer.0.attention.self.query.weight", "bert.embeddings.position_embeddings.weight",
              "cls.predictions.entity_decoder.weight", "bert.pooler.dense.weight"):
        d_got, d_ref = params[k].double() - sd[k].double(), osd[k] - sd[k].double()
        cos = torch.nn.functional.cosine_similarity(d_got.flatten(), d_ref.flatten(), dim=0).item()
        assert cos > 0.97, (k, cos)
    assert runs[False][0] == pytest.approx(got, rel=1e-4)


# ------------------------------------------------------------------------------------------ (d) classification
def test_classification_step_with_dropout_matches_the_masked_oracle(hip):
    """STonKGsForSequenceClassification on g6_classification at p = 0.1: the pooled vector's dropout (site (300, 0), flat
    form) and backward_cls, on the packed rows with position 0 as the only read row. Loss, classifier.*, bert.pooler.* and
    every encoder gradient against forward_classification(..., dropout=...)."""
    from stonkgs_amd.stonkgs_model import STonKGsForSequenceClassification
    from tests.test_finetune_gpu import _g6

    cfg, sd, rows, gold, meta = _g6()
    batch = {k: torch.from_numpy(gold[k]) for k in ("input_ids", "attention_mask", "token_type_ids", "labels")}
    inputs = {k: batch[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    with torch.no_grad():
        table = orc.build_kg_table(rows, orc.special_vectors(sd, cfg))
    model = _build(cfg, sd, rows, P, cls=STonKGsForSequenceClassification, num_labels=meta["num_labels"])
    e = model.engine
    layout = (e.unpad, e.prune_last_ffn, e.prune_last_attn)
    assert layout == (True, True, True)
    for p, m in ((0.0, _build(cfg, sd, rows, 0.0, cls=STonKGsForSequenceClassification, num_labels=meta["num_labels"])),
                 (P, model)):
        m.train()
        m.zero_grad()
        m.engine.seed_base = SEED_BASE
        loss = float(m.forward_backward(dict(batch)))
        m.engine.join_wgrad()
        m.engine.check_errors()
        torch.cuda.synchronize()
        assert m.engine.seed_base == SEED_BASE + 1
        grads = {k: v.detach().cpu().clone() for k, v in m.named_grad_views().items()}
        prov = R.StepDropout(cfg, batch, SEED_BASE + 1, layout, p, p, labels=(None, None)) if p > 0 else None
        ref_terms, g64 = R.oracle_cls_step(R.to64(sd), cfg, table, inputs, batch["labels"], prov)
        _, g16 = R.oracle_cls_step(sd, cfg, table, inputs, batch["labels"], prov, autocast=True)
        r16 = {k: R.rel(g16[k], g64[k]) for k in g64}
        assert set(grads) <= set(g64) and {"classifier.weight", "classifier.bias", "bert.pooler.dense.weight"} <= set(grads)
        print(R.describe(f"classification p {p}", grads, g64, r16), "| loss |d|", f"{abs(loss - ref_terms['loss']):.2e}")
        bad = R.compare({"loss": loss}, grads, ref_terms, g64, r16, ENVELOPE)
        assert not bad, (p, bad)
