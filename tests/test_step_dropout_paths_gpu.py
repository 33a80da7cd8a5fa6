"""GPU: three dropout-on paths where the engine or the trainer could draw the wrong mask and the whole-step comparison
(tests/test_step_dropout_gpu.py) would not notice - each against the fp64 oracle under the step's exact masks.

  A  the frozen backbone's own output (`Engine.backbone_fwd`), inline and prefetched, per sequence against the oracle under
     the masks of the step that CONSUMES it: relative L2 <= 3 x r16, the bf16-autocast oracle's own error on that sequence
     (the block rule of profiles/bigbird_attention.md with 3 for its 2: the engine's bf16 residual stream alone costs 2.4 x
     r16, see BACKBONE_FACTOR in the CPU file). Seven wrong seeds on the real engine must each fail that comparison.
  B  the text-only classifier (`TextEngine`) at p = 0.1: loss and every gradient tensor, the word table's included, in the
     four row layouts; the structure of the word-table gradient; five wrong-mask oracles rejected; three Trainer steps.
  C  gradient accumulation over two micro-batches at p = 0.1 with a backbone forward prefetched across the micro-batch
     boundary: the accumulated gradient against the mean of two masked oracle gradients, on two optimizer steps.

References, mutants and their CPU distances: tests/test_step_dropout_paths_cpu.py. Figures of one MI355X run:
profiles/step_dropout_paths.md."""
import numpy as np
import pytest
import torch

from tests import step_dropout_ref as R
from tests import test_step_dropout_paths_cpu as C
from tests.test_step_dropout_gpu import ENVELOPE, P, SEED_BASE, _build
from tests.test_text_embed_cpu import PAD, WORD

pytestmark = pytest.mark.gpu

STEP = SEED_BASE + 1
B = 4


# ====================================================================================== A. the frozen backbone's output
@pytest.fixture(scope="module")
def bcase(hip):
    return C.backbone_case()


@pytest.fixture(scope="module")
def backbone_model(bcase):
    model = _build(bcase["cfg"], bcase["sd"], bcase["tsv_rows"], P)
    model.train()
    return model


def _spy_backbone(eng):
    """Record the counter every backbone forward is drawn under and a copy of the rows it returns."""
    seen, inner = [], eng.backbone_fwd

    def backbone_fwd(*a, **kw):
        x = inner(*a, **kw)
        seen.append((eng.seed_base, x.clone()))
        return x

    eng.backbone_fwd = backbone_fwd
    return seen, inner


def _check_backbone(bcase, tag, bi, counter, y):
    y64, r16 = C.backbone_reference(bcase, bi, counter)
    q = C.backbone_ratios(y, y64, r16)
    print(f"PARITY backbone {tag}: batch {bi} counter {counter:#x} per-sequence err / r16 {np.round(q, 2).tolist()} "
          f"worst {q.max():.2f} of {C.BACKBONE_FACTOR}")
    assert y.dtype == torch.bfloat16 and y.shape == (B * bcase["cfg"].half_length, bcase["cfg"].hidden_size)
    return C.backbone_violations(y, y64, r16)


def test_backbone_output_inline_and_prefetched_matches_the_masked_oracle(bcase, backbone_model):
    """One forward_backward (inline backbone forward) and three Trainer steps with the next batch hinted (steps 2 and 3
    consume forwards drawn one step early, under seed_base + 1 inside `prefetch_backbone`): every backbone output against
    the fp64 oracle under the masks of the step that consumes it."""
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    model, eng, batches = backbone_model, backbone_model.engine, bcase["batches"]
    seen, inner = _spy_backbone(eng)
    try:
        eng.seed_base = SEED_BASE
        model.zero_grad()
        model.forward_backward(batches[1])
        eng.join_wgrad()
        torch.cuda.synchronize()
        assert [s for s, _ in seen] == [STEP] and eng._prefetch is None
        eng.seed_base = SEED_BASE
        tr = Trainer(model, TrainingArguments(max_steps=10, learning_rate=1e-3, per_device_train_batch_size=B,
                                              optimizer_overlap=True, prefetch_backbone=True))
        dev = [{k: v.cuda() for k, v in b.items()} for b in batches]
        for i in range(3):
            assert (eng._prefetch is not None) == (i > 0)      # steps 2 and 3 consume a prefetched forward
            tr.training_step(model, dev[i % 2], next_inputs=dev[(i + 1) % 2] if i < 2 else None)
        eng.check_errors()
        torch.cuda.synchronize()
    finally:
        eng.backbone_fwd = inner
    assert eng.seed_base == SEED_BASE + 3 and eng._prefetch is None
    # step 1 ran its forward inline; the forwards of steps 2 and 3 were queued while the step before them was running
    assert [s for s, _ in seen] == [STEP, STEP, STEP + 1, STEP + 2]
    fails = {}
    for tag, bi, (counter, y) in zip(("inline, forward_backward", "inline, trainer step 1", "prefetched, trainer step 2",
                                      "prefetched, trainer step 3"), (1, 0, 1, 0), seen):
        bad = _check_backbone(bcase, tag, bi, counter, y)
        if bad:
            fails[tag] = bad
    assert not fails, fails


def _backbone_alone(bcase, model, bi, seed_base, slip=None):
    """The engine's backbone forward alone on batch `bi` with the counter at `seed_base`; `slip` = the (layer, site) whose
    seed is off by one."""
    eng, cfg = model.engine, bcase["cfg"]
    ids = bcase["batches"][bi]["input_ids"].cuda().contiguous()
    model._sync_derived()
    inner, before = eng.seed, eng.seed_base
    if slip is not None:
        eng.seed = lambda layer, site: (inner(layer, site) + int((layer, site) == slip)) & 0xFFFFFFFF
    try:
        eng.seed_base = seed_base
        y = eng.backbone_fwd(ids, cfg.max_position_embeddings, B, cfg.half_length, True).clone()
    finally:
        eng.seed, eng.seed_base = inner, before
    torch.cuda.synchronize()
    eng.check_errors()
    return y


def test_the_real_backbone_fails_the_comparison_under_a_wrong_seed(bcase, backbone_model):
    """The comparison can fail on the real engine: `engine.seed` patched so that ONE interior (layer, site) draws with its
    seed + 1, and the forward run under the previous counter (what a prefetch without its `seed_base + 1` would do), each
    violate the bound that the unpatched forward on the same batch keeps."""
    y64, r16 = C.backbone_reference(bcase, 1, STEP)
    assert not C.backbone_violations(_backbone_alone(bcase, backbone_model, 1, STEP), y64, r16)
    mutants = [(f"seed of {s} + 1", dict(slip=s, seed_base=STEP)) for s in C.INTERIOR]
    mutants.append(("drawn under seed_base, not seed_base + 1", dict(seed_base=STEP - 1)))
    assert len(mutants) == 7
    for name, kw in mutants:
        y = _backbone_alone(bcase, backbone_model, 1, **kw)
        q = C.backbone_ratios(y, y64, r16)
        bad = C.backbone_violations(y, y64, r16)
        print(f"engine mutant, {name}: per-sequence err / r16 {np.round(q, 1).tolist()} -> {len(bad)} violations")
        assert bad, name


# ====================================================================================== B. the text baseline at p = 0.1
@pytest.fixture(scope="module")
def tcase(hip):
    return C.text_case()


def _build_text(tc, p, num_labels=3):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.nlp_baseline_model import BertForSequenceClassification

    cfg = tc["cfg"]
    c = STonKGsConfig(**{k: getattr(cfg, k) for k in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads",
                                                      "intermediate_size", "max_position_embeddings", "type_vocab_size",
                                                      "layer_norm_eps")},
                      hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    model = BertForSequenceClassification(c, num_labels=num_labels)
    missing, unexpected = model.load_state_dict(tc["sd"], strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.train()
    return model


@pytest.fixture(scope="module")
def text_models(tcase):
    return {p: _build_text(tcase, p) for p in (0.0, P)}


def _text_step(model, batch, layout, seed_base=SEED_BASE):
    e = model.engine
    e.unpad, e.prune_last_ffn, e.prune_last_attn = layout
    e.seed_base = seed_base
    model.zero_grad()
    loss = float(model.forward_backward(batch))
    e.join_wgrad()
    e.check_errors()
    torch.cuda.synchronize()
    assert e.seed_base == seed_base + 1
    return {"loss": loss}, {k: v.detach().cpu().clone() for k, v in model.named_grad_views().items()}


@pytest.mark.parametrize("layout", R.LAYOUTS, ids=lambda l: "".join("FT"[int(x)] for x in l))
def test_text_step_matches_the_masked_restatement(tcase, text_models, layout):
    """forward_backward of the text-only classifier at p = 0 and p = 0.1 in the layout (unpad, prune_last_ffn,
    prune_last_attn): the loss and every gradient tensor - the word table's, which passes back through the embedding
    dropout at site (200, 0), included - against the fp64 restatement under the step's masks."""
    fails = {}
    for p in (0.0, P):
        ref_terms, g64, r16 = C.text_reference(tcase, layout, p)
        terms, grads = _text_step(text_models[p], tcase["batch"], layout)
        assert set(grads) == set(g64) and WORD in grads
        print(R.describe(f"text layout {layout} p {p}", grads, g64, r16), "| loss |d|",
              f"{abs(terms['loss'] - ref_terms['loss']):.2e}", "| word table err / r16",
              f"{R.rel(grads[WORD], g64[WORD]) / r16[WORD]:.2f}")
        bad = R.compare(terms, grads, ref_terms, g64, r16, ENVELOPE)
        if bad:
            fails[p] = bad
    assert not fails, fails


def test_text_word_table_gradient_keeps_its_structure_under_dropout(tcase, text_models):
    """At p = 0.1: the [PAD] row (a [PAD] id stands at an attended position) and the rows of ids the batch does not hold
    are exactly zero, every other row is not."""
    cfg, ids = tcase["cfg"], tcase["batch"]["input_ids"]
    _, grads = _text_step(text_models[P], tcase["batch"], C.FULL)
    dword = grads[WORD]
    assert (ids[tcase["batch"]["attention_mask"] == 1] == PAD).any() and torch.count_nonzero(dword[PAD]) == 0
    absent = torch.ones(cfg.vocab_size, dtype=torch.bool)
    absent[ids.unique()] = False
    assert absent.sum() >= 20 and torch.count_nonzero(dword[absent]) == 0
    present = ~absent
    present[PAD] = False
    assert present.sum() > 100 and (dword[present].abs().amax(dim=1) > 0).all()


def test_the_text_comparison_rejects_wrong_masks(tcase, text_models):
    """The real step (default layout) against the restatement under masks with ONE mistake each (their CPU distances:
    test_text_mutants_move_a_quantity_by_three_times_its_gpu_tolerance)."""
    terms, grads = _text_step(text_models[P], tcase["batch"], C.FULL)
    ref_terms, g64, r16 = C.text_reference(tcase, C.FULL, P)
    assert not R.compare(terms, grads, ref_terms, g64, r16, ENVELOPE)
    assert len(C.TEXT_MUTANTS) >= 4
    for name, kw in C.TEXT_MUTANTS.items():
        m_terms, m64 = C.text_mutant(tcase, kw)
        bad = R.compare(terms, grads, m_terms, m64, r16, ENVELOPE)
        print("text mutant,", name, "->", len(bad), "violations, e.g.", bad[:2])
        assert bad, name


def test_three_text_trainer_steps_match_the_masked_restatement(tcase):
    """Three Trainer steps at p = 0.1 (optimizer on its own stream, a next batch hinted although nothing can be
    prefetched) against the fp64 restatement trained with torch.optim.AdamW under the masks of counters +1, +2, +3."""
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    model = _build_text(tcase, P)
    eng, batch = model.engine, tcase["batch"]
    assert (eng.unpad, eng.prune_last_ffn, eng.prune_last_attn) == C.FULL
    eng.seed_base = SEED_BASE
    tr = Trainer(model, TrainingArguments(learning_rate=C.TEXT_LR, max_steps=C.TEXT_MAX_STEPS, per_device_train_batch_size=5,
                                          optimizer_overlap=True))
    got = []
    for i in range(3):
        got.append(float(tr.training_step(model, batch, next_inputs=batch)))
        assert eng._prefetch is None and eng.next_input_ids is None     # TextEngine has no backbone to run ahead
    eng.check_errors()
    torch.cuda.synchronize()
    ref = C.text_training_losses(tcase)
    print("text trainer losses", got, "restatement", ref)
    assert eng.seed_base == SEED_BASE + 3 and tr.optimizer.step_count == 3
    assert np.abs(np.array(got) - np.array(ref)).max() < R.LOSS_ATOL, (got, ref)


# ====================================================================================== C. accumulation at p = 0.1
def test_two_micro_batches_per_step_with_dropout_match_the_masked_oracle(hip):
    """Four Trainer calls = two optimizer steps of two micro-batches, each call hinting the next batch: the counter advances
    once per micro-batch, the forward prefetched across the micro-batch (and the optimizer-step) boundary draws the
    consuming micro-batch's masks, gscale = 1 / 2, and the decoders' spans are stored by the first micro-batch and
    accumulated into by the second. The accumulated gradient, taken where the optimizer's update starts, against
    (g(batch 0; c) + g(batch 1; c + 1)) / 2 of the fp64 oracle on the weights as they are before that step."""
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    ac = C.accumulation_case()
    model = _build(ac["cfg"], ac["sd"], ac["tsv_rows"], P)
    eng = model.engine
    assert (eng.unpad, eng.prune_last_ffn, eng.prune_last_attn) == C.FULL
    eng.seed_base = SEED_BASE
    tr = Trainer(model, TrainingArguments(gradient_accumulation_steps=C.GAS, learning_rate=C.ACC_LR, max_steps=C.ACC_MAX_STEPS,
                                          per_device_train_batch_size=B, optimizer_overlap=True, prefetch_backbone=True))
    opt, seen = tr.optimizer, []
    inner = opt.apply_update

    def apply_update(lr, grad_scale=1.0, **kw):
        seen.append(dict(g={k: v.detach().clone() for k, v in model.named_grad_views().items()}, lr=lr, step=opt.step_count))
        return inner(lr, grad_scale, **kw)

    opt.apply_update = apply_update
    dev = [{k: v.cuda() for k, v in b.items()} for b in ac["batches"]]
    terms, logs = [], []
    for i in range(4):
        assert (eng._prefetch is not None) == (i > 0)      # calls 2, 3 and 4 consume a prefetched backbone forward
        eng.store_log.clear()
        loss = float(tr.training_step(model, dev[i % 2], next_inputs=dev[(i + 1) % 2]))
        terms.append(dict(zip(R.TERMS, [loss] + [float(t) for t in model.last_loss_terms])))
        logs.append(list(eng.store_log))
        assert eng.seed_base == SEED_BASE + 1 + i and opt.step_count == (i + 1) // 2
    eng.check_errors()
    torch.cuda.synchronize()
    assert eng.seed_base == SEED_BASE + 4 and opt.step_count == 2 and len(seen) == 2
    assert [s["step"] for s in seen] == [1, 2] and seen[0]["lr"] == pytest.approx(C.ACC_LR) and seen[1]["lr"] == pytest.approx(0.9 * C.ACC_LR)
    print("store_log per call", logs)
    ref = C.accumulation_reference(ac)
    fails = {}
    for s in range(2):
        grads = {k: v.cpu() for k, v in seen[s]["g"].items()}
        assert set(grads) <= set(ref[s]["g64"])
        loss_d = [max(abs(terms[2 * s + j][k] - ref[s]["terms"][j][k]) for k in R.TERMS) for j in range(2)]
        print(R.describe(f"accumulation, optimizer step {s + 1}", grads, ref[s]["g64"], ref[s]["r16"]),
              "| loss terms max |d| per micro-batch", [f"{d:.2e}" for d in loss_d])
        bad = R.compare({}, grads, {}, ref[s]["g64"], ref[s]["r16"], ENVELOPE)
        for j in range(2):
            got, want = terms[2 * s + j], ref[s]["terms"][j]
            bad += [f"micro-batch {j} {k}: {got[k]:.5f} vs {want[k]:.5f}" for k in R.TERMS
                    if not abs(got[k] - want[k]) < R.LOSS_ATOL]
        if bad:
            fails[s] = bad
    assert not fails, fails
    # the comparison rejects an oracle with one mistake (CPU distances: test_accumulation_mutants_move_...)
    grads = {k: v.cpu() for k, v in seen[0]["g"].items()}
    for name in C.ACC_MUTANTS:
        m_terms, m64 = C.accumulation_mutant(ac, name)
        bad = R.compare(terms[1], grads, m_terms, m64, ref[0]["r16"], ENVELOPE)
        print("accumulation mutant,", name, "->", len(bad), "violations, e.g.", bad[:2])
        assert bad, name
    # the route on record: only the first micro-batch of a step tries to store. At this model's 512 x 128 and 384 x 128
    # decoder gradients over 512 rows the routing splits K eight ways, the store entry refuses both and they accumulate -
    # on step 2 into spans the optimizer left unzeroed and marked stale (the stored route: tests/test_wgrad_store_gpu.py)
    text, ent = "cls.predictions.text_decoder.weight", "cls.predictions.entity_decoder.weight"
    assert logs[1] == logs[3] == [] and logs[0] == logs[2] == [(ent, hip.ESHAPE), (text, hip.ESHAPE)], logs
