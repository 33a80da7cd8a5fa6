"""CPU: the references of tests/test_step_dropout_paths_gpu.py and their discriminating power - three dropout-on paths that
the whole-step comparison (tests/test_step_dropout_gpu.py) cannot see or does not run:

  A  the frozen backbone's own output, site by site. The whole step sees the backbone through the encoder's gradients only
     and a seed slip at five of its six interior sites stays below tolerance there (profiles/step_dropout_parity.md). Here
     the output itself is the compared quantity, per sequence, as a multiple of the bf16-autocast oracle's own error.
  B  the text-only classifier (TextEngine) at p = 0.1: the restatement that transformers pins at p = 0
     (tests/test_text_embed_cpu.py) with the oracle's dropout hooks, the word table's gradient included.
  C  two micro-batches per optimizer step at p = 0.1: the mean of two masked gradients under consecutive counters.

What is proven here without a GPU: the restatement with `dropout=None` is the code it was, the text batch's row counts,
that the hand-made AdamW equals `orc.train_step`'s, and that every single mistake the GPU tests reject moves a compared
quantity by at least 3 x its GPU tolerance (fp64 oracle under the mistake against the fp64 oracle under the contract)."""
import contextlib
import re

import numpy as np
import pytest
import torch

from oracle import stonkgs_oracle as orc
from oracle.masking_oracle import unpad_plan
from tests import step_dropout_ref as R
from tests.golden_util import load_case
from tests.test_step_dropout_gpu import ENVELOPE, P, SEED_BASE
from tests.test_text_embed_cpu import PAD, WORD, restatement_grads, text_batch, text_classifier, text_state_dict, tiny_config

STEP = SEED_BASE + 1
FULL = (True, True, True)


@pytest.fixture
def deterministic():
    """Index-adds into the embedding tables are split among threads in an order of torch's own: bit-for-bit comparisons
    of two oracle runs need the deterministic kernels."""
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(before)


# ====================================================================================== A. the frozen backbone's output
SHARPEN = 16.0          # a power of two: the sharpened weights stay bf16-exact
# GPU bound per sequence: relative L2 <= BACKBONE_FACTOR x r16, r16 = the bf16-AUTOCAST oracle's error. The block rule of
# profiles/bigbird_attention.md has 2 here, against an emulation that rounds where the kernel rounds. Autocast does not: it
# keeps the residual stream in fp32 where `layer_fwd` stores bf16 (five more roundings per layer pair on stream-sized
# values), and `backbone_rounding_model` - fp64 arithmetic with the engine's bf16 stores, no GPU involved - already stands at
# 2.35 .. 2.57 x r16 (test_the_bf16_residual_stream_alone_costs_more_than_twice_r16). 2 cannot be kept by a correct engine;
# 3 is the next whole factor, and the largest for which every wrong seed still lies at 3 x the bound (the weakest, site
# (101, 3), moves a sequence by 9.8 x r16: 9.8 / 3 = 3.27).
BACKBONE_FACTOR = 3.0
CPU_FACTOR = 3.0        # a mistake must move a compared quantity by 3 x its GPU tolerance
INTERIOR = tuple((R.BACKBONE_LAYER0 + i, s) for i in range(2) for s in (1, 2, 3))
_QK = re.compile(r"lm_backbone\.encoder\.layer\.\d+\.attention\.self\.(query|key)\.weight")


def sharpened(sd):
    """`sd` with the backbone's query and key weights x 16. At the stored (random-initialised) weights the scores are
    small, attention is near uniform and the dropout mask on the probabilities averages out: a slip at site 1 moves the
    output by 1.3 .. 1.4 x r16 and cannot be told from rounding."""
    out = dict(sd)
    hit = [k for k in sd if _QK.fullmatch(k)]
    assert len(hit) == 4, hit
    for k in hit:
        out[k] = sd[k] * SHARPEN
        assert torch.equal(out[k].to(torch.bfloat16).to(out[k].dtype), out[k])
    return out


def backbone_case():
    """g2_hipsmall (H 128, 2 backbone layers, half 128, vocab 512) with the sharpened backbone, the two batches of
    tests/test_unpad_gpu._batches at B = 4."""
    from tests.test_unpad_gpu import _batches

    cfg, sd, tsv_rows, _, _, _ = load_case("g2_hipsmall")
    sharp = sharpened(sd)
    return dict(cfg=cfg, stored=sd, stored64=R.to64(sd), sd=sharp, sd64=R.to64(sharp), tsv_rows=tsv_rows,
                batches=_batches(cfg, 4), refs={})


def backbone_oracle(sd, cfg, batch, counter, autocast=False, **mutant):
    """The backbone's output [B, half, H] as fp64 under the masks of the step `counter`; `autocast`: the bf16-autocast
    oracle on fp32 weights with its output rounded to bf16 (what the engine hands to the encoder)."""
    prov = R.StepDropout(cfg, batch, counter, FULL, P, P, **mutant)
    ids = batch["input_ids"][:, :cfg.half_length]
    with torch.no_grad(), (torch.autocast("cpu", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()):
        y = orc.lm_backbone_forward(sd, cfg, ids, dropout=prov)
    return (y.to(torch.bfloat16) if autocast else y).double()


def backbone_rounding_model(sd64, cfg, batch, counter):
    """The same forward in fp64, rounded to bf16 wherever `Engine.layer_fwd` writes a bf16 buffer and the autocast oracle
    keeps fp32: the embeddings' output, both residual sums in front of a LayerNorm (s1, s2) and both LayerNorm outputs
    (h1, y) - the residual stream is bf16 from end to end - besides the roundings autocast has too (q, k, v, the
    probabilities, ctx, the GELU output). No tile order, no fp32 accumulation: what the number format alone costs."""
    import torch.nn.functional as F

    prov = R.StepDropout(cfg, batch, counter, FULL, P, P)
    ids = batch["input_ids"][:, :cfg.half_length]
    r = lambda t: t.to(torch.bfloat16).double()   # noqa: E731
    nh, eps = cfg.num_attention_heads, cfg.layer_norm_eps
    with torch.no_grad():
        x = r(orc.bert_embeddings(sd64, "lm_backbone.embeddings", cfg, input_ids=ids, dropout=prov))
        Bn, S, H = x.shape
        heads = lambda t: t.view(Bn, S, nh, H // nh).transpose(1, 2)   # noqa: E731
        for i in range(cfg.n_backbone_layers):
            p = f"lm_backbone.encoder.layer.{i}"
            q, k, v = (heads(r(orc._linear(x, sd64, f"{p}.attention.self.{n}"))) for n in ("query", "key", "value"))
            probs = torch.softmax(q @ k.transpose(-1, -2) / (H // nh) ** 0.5, dim=-1)
            ctx = r((r(orc._drop(probs, prov, (p, 1))) @ v).transpose(1, 2).reshape(Bn, S, H))
            s1 = r(orc._drop(orc._linear(ctx, sd64, p + ".attention.output.dense"), prov, (p, 2)) + x)
            h1 = r(orc._ln(s1, sd64, p + ".attention.output.LayerNorm", eps))
            g = r(F.gelu(orc._linear(h1, sd64, p + ".intermediate.dense")))
            s2 = r(orc._drop(orc._linear(g, sd64, p + ".output.dense"), prov, (p, 3)) + h1)
            x = r(orc._ln(s2, sd64, p + ".output.LayerNorm", eps))
    return x


def seq_rel(y, ref):
    """Relative L2 of every sequence of `y` ([B, half, H] or the engine's [B * half, H] rows) from `ref`: float64 [B]."""
    y = torch.as_tensor(y).detach().double().cpu().reshape(ref.shape)
    return ((y - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).numpy()


def backbone_reference(case, bi, counter, weights="sd"):
    """(fp64 output, r16 per sequence) of batch `bi` under the masks of `counter` - computed once."""
    key = (bi, counter, weights)
    if key not in case["refs"]:
        cfg, batch = case["cfg"], case["batches"][bi]
        y64 = backbone_oracle(case[weights + "64"], cfg, batch, counter)
        case["refs"][key] = (y64, seq_rel(backbone_oracle(case[weights], cfg, batch, counter, autocast=True), y64))
    return case["refs"][key]


def backbone_ratios(y, y64, r16):
    return seq_rel(y, y64) / r16


def backbone_violations(y, y64, r16, factor=BACKBONE_FACTOR) -> list:
    """The GPU test's comparison of one backbone forward: every violated condition as a string."""
    y = torch.as_tensor(y)
    bad = [] if bool(torch.isfinite(y.float()).all()) else ["not finite"]
    q = backbone_ratios(y, y64, r16)
    return bad + [f"sequence {b}: {q[b]:.2f} x r16 {r16[b]:.3e}" for b in range(len(q)) if not q[b] <= factor]


BACKBONE_MUTANTS = {f"seed of ({l}, {s}) + 1": dict(seed_delta={(l, s): 1}) for l, s in INTERIOR}
BACKBONE_MUTANTS["backbone under the previous counter"] = dict(backbone_base=STEP - 1)


@pytest.fixture(scope="module")
def bcase():
    return backbone_case()


def test_r16_of_the_sharpened_backbone(bcase):
    """The yardstick is what the issue measured: about 2e-3 per sequence, sharpened or not, and the sharpened weights did
    change the output."""
    for bi in range(2):
        y64, r16 = backbone_reference(bcase, bi, STEP)
        y64s, r16s = backbone_reference(bcase, bi, STEP, "stored")
        print(f"batch {bi}: r16 sharpened {np.round(r16, 5)}, stored {np.round(r16s, 5)}; "
              f"sharpened against stored output {np.round(seq_rel(y64, y64s), 3)}")
        assert (r16 > 5e-4).all() and (r16 < 5e-3).all() and (r16s > 5e-4).all() and (r16s < 5e-3).all()
        assert (seq_rel(y64, y64s) > 0.05).all()
        assert y64.shape == (4, 128, 128)


def test_the_bf16_residual_stream_alone_costs_more_than_twice_r16(bcase):
    """Where the factor 3 comes from. The forward in fp64 with nothing but the engine's bf16 stores stands at 2.3 .. 2.6 x
    the autocast oracle's error, on every sequence under the masks of the three counters the GPU test runs: the block
    rule's 2 is out of reach for any implementation with a bf16 residual stream, 3 is kept with room."""
    for bi in range(2):
        for counter in (STEP, STEP + 1, STEP + 2):
            y64, r16 = backbone_reference(bcase, bi, counter)
            q = backbone_ratios(backbone_rounding_model(bcase["sd64"], bcase["cfg"], bcase["batches"][bi], counter), y64, r16)
            print(f"rounding model, batch {bi} counter {counter:#x}: per-sequence err / r16 {np.round(q, 2)}")
            assert (q > 2.0).all() and (q < 0.9 * BACKBONE_FACTOR).all(), (bi, counter, q)


@pytest.mark.parametrize("name", sorted(BACKBONE_MUTANTS))
def test_backbone_mutants_move_a_sequence_by_three_times_the_gpu_bound(bcase, name):
    """Each of the six interior seed slips and the backbone drawn under counter - 1 moves at least one sequence's relative
    L2 to >= 3 x the GPU bound, that is 9 x r16, on both batches (no site had to be pinned on batch 1 alone)."""
    for bi in range(2):
        y64, r16 = backbone_reference(bcase, bi, STEP)
        q = backbone_ratios(backbone_oracle(bcase["sd64"], bcase["cfg"], bcase["batches"][bi], STEP, **BACKBONE_MUTANTS[name]),
                            y64, r16)
        print(f"{name}, batch {bi}: per-sequence distance / r16 {np.round(q, 1)}")
        assert q.max() >= CPU_FACTOR * BACKBONE_FACTOR, (name, bi, q)


def test_site_one_slips_are_invisible_at_the_stored_weights(bcase):
    """Why the query / key weights are sharpened: at the stored weights a seed slip at the probabilities' site moves every
    sequence of both batches by less than 2 x r16 - inside the GPU bound, and below what the engine's own bf16 stores cost
    there: a test on those weights would pass a wrong seed."""
    for bi in range(2):
        y64, r16 = backbone_reference(bcase, bi, STEP, "stored")
        for layer in (101, 102):
            q = backbone_ratios(backbone_oracle(bcase["stored64"], bcase["cfg"], bcase["batches"][bi], STEP,
                                                seed_delta={(layer, 1): 1}), y64, r16)
            print(f"stored weights, ({layer}, 1) + 1, batch {bi}: per-sequence distance / r16 {np.round(q, 2)}")
            assert q.max() < 2.0 < BACKBONE_FACTOR, (bi, layer, q)


# ====================================================================================== B. the text baseline at p = 0.1
LENGTHS = [1, 16, 100, 256, 60]
TEXT_MUTANTS = {
    "counter + 1": dict(seed_base=STEP + 1),
    "padded rows in the packed layout": dict(rows="padded"),
    "backward mask != forward mask, embeddings (200, 0)": dict(backward_seed_delta={(R.JOINT_EMB, 0): 1}),
    "classifier seed (300, 0) + 1": dict(seed_delta={(R.CLASSIFIER, 0): 1}),
    "packed row for the read row, site 3": dict(read_rows=(3,)),
}
TEXT_LR, TEXT_MAX_STEPS = 1e-3, 10


def text_case():
    cfg = tiny_config()
    sd = text_state_dict(cfg)
    return dict(cfg=cfg, sd=sd, sd64=R.to64(sd), batch=text_batch(cfg, LENGTHS), refs={})


def text_provider(tc, layout, p, counter=STEP, **mutant):
    if p == 0:
        return None
    return R.StepDropout(tc["cfg"], tc["batch"], counter, layout, p, p, labels=(None, None), **mutant)


def text_reference(tc, layout, p, counter=STEP):
    """(fp64 loss, fp64 gradients, r16 per tensor) of the text step under the masks of `layout` - computed once."""
    key = (layout if p > 0 else None, p, counter)
    if key not in tc["refs"]:
        prov = text_provider(tc, layout, p, counter)
        terms, g64 = R.oracle_text_step(tc["sd64"], tc["cfg"], tc["batch"], prov)
        _, g16 = R.oracle_text_step(tc["sd"], tc["cfg"], tc["batch"], prov, autocast=True)
        tc["refs"][key] = (terms, g64, {k: R.rel(g16[k], g64[k]) for k in g64})
    return tc["refs"][key]


def text_mutant(tc, kw, layout=FULL):
    """(fp64 loss, fp64 gradients) of the text step under the mutant masks `kw`."""
    kw = dict(kw)
    prov = text_provider(tc, layout, P, kw.pop("seed_base", STEP), **kw)
    return R.oracle_text_step(tc["sd64"], tc["cfg"], tc["batch"], prov)


def text_training_losses(tc, n=3, first_counter=STEP, advance=1):
    """Losses of `n` optimizer steps of the fp64 restatement under the masks of counters first_counter, +1, ... with
    torch.optim.AdamW as TrainingArguments sets it: no weight decay, clip at 1.0, linear schedule over TEXT_MAX_STEPS.
    `advance` 0: the counter stands still (what the reference must be told from)."""
    params = {k: v.clone().requires_grad_(True) for k, v in tc["sd64"].items()}
    opt = torch.optim.AdamW(list(params.values()), lr=TEXT_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    b, losses = tc["batch"], []
    for i in range(n):
        for g in opt.param_groups:
            g["lr"] = orc.linear_schedule_lr(TEXT_LR, i, TEXT_MAX_STEPS)
        opt.zero_grad()
        out = text_classifier(params, tc["cfg"], b["input_ids"], b["attention_mask"], b["token_type_ids"], b["labels"],
                              dropout=text_provider(tc, FULL, P, first_counter + advance * i))
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
        opt.step()
        losses.append(float(out["loss"].detach()))
    return losses


@pytest.fixture(scope="module")
def tcase():
    return text_case()


def test_restatement_without_a_provider_is_the_code_it_was(tcase, deterministic):
    """`dropout=None`, the argument absent, and a provider with p = 0 give the same loss, logits and gradients bit for bit
    (test_restatement_equals_transformers_bert_for_sequence_classification pins the absent form to transformers)."""
    cfg, sd, b = tcase["cfg"], tcase["sd"], tcase["batch"]
    loss0, logits0, g0 = restatement_grads(sd, cfg, b)          # (calls text_classifier without the argument)
    zero = R.StepDropout(cfg, b, STEP, FULL, 0.0, 0.0, labels=(None, None))
    for prov in (None, zero):
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        out = text_classifier(p, cfg, b["input_ids"], b["attention_mask"], b["token_type_ids"], b["labels"], dropout=prov)
        out["loss"].backward()
        assert torch.equal(out["loss"].detach(), loss0) and torch.equal(out["logits"].detach(), logits0)
        for k in g0:
            assert torch.equal(p[k].grad, g0[k]), k
    terms, grads = R.oracle_text_step(sd, cfg, b, None)
    assert terms["loss"] == float(loss0) and set(grads) == set(sd)
    for k in g0:
        assert torch.equal(grads[k], g0[k]), k


def test_text_batch_rows_and_the_sites_the_provider_is_asked_for(tcase):
    """433 packed rows and 5 read rows (position 0 of every sequence); the step asks for the encoder's sites and the
    classifier's, never for a backbone site; a length-1 sequence, a full one, a [PAD] id at an attended position, both
    token types."""
    cfg, b = tcase["cfg"], tcase["batch"]
    rop, _, offs, _, _, read_of_pos, _ = unpad_plan(np.asarray(b["attention_mask"]), None, None, read=True)
    assert int((rop >= 0).sum()) == sum(LENGTHS) == 433 and int(offs[5]) == 433
    S = cfg.max_position_embeddings
    assert int((read_of_pos >= 0).sum()) == 5 and (np.nonzero(read_of_pos >= 0)[0] == np.arange(5) * S).all()
    am, ids = b["attention_mask"], b["input_ids"]
    assert sorted(am.sum(1).tolist()) == sorted(LENGTHS) and (ids[am == 1] == PAD).any()
    assert set(b["token_type_ids"][am == 1].unique().tolist()) == {0, 1}

    class Spy(R.StepDropout):
        asked = []

        def _mask(self, site_key, shape, backward):
            self.asked.append(site_key)
            return super()._mask(site_key, shape, backward)

    prov = Spy(cfg, b, STEP, FULL, P, P, labels=(None, None))
    R.oracle_text_step(tcase["sd64"], cfg, b, prov)
    want = {("bert.embeddings", 0), ("classifier", 0)} | {(f"bert.encoder.layer.{i}", s) for i in range(2) for s in (1, 2, 3)}
    assert set(prov.asked) == want
    assert prov.launch(("bert.embeddings", 0))[1:3] == (R.JOINT_EMB, 0) and prov.launch(("classifier", 0))[1:3] == (R.CLASSIFIER, 0)


def test_text_losses_and_the_word_table_gradient_move_with_the_masks(tcase):
    """The recorded fp64 losses (p = 0, and the masks of two consecutive counters), and how far the word table's gradient
    moves: dropout is not a perturbation that a tolerance could swallow."""
    t0, g0, _ = text_reference(tcase, FULL, 0.0)
    t1, g1, r16 = text_reference(tcase, FULL, P)
    t2, g2 = text_mutant(tcase, TEXT_MUTANTS["counter + 1"])
    print("fp64 loss p 0", t0["loss"], "counter", hex(STEP), t1["loss"], "counter + 1", t2["loss"],
          "| word table moves", R.rel(g1[WORD], g0[WORD]), R.rel(g2[WORD], g1[WORD]), "r16", r16[WORD])
    assert t0["loss"] == pytest.approx(1.11986, abs=1e-5) and t1["loss"] == pytest.approx(1.09608, abs=1e-5)
    assert t2["loss"] == pytest.approx(1.13008, abs=1e-5)
    assert R.rel(g1[WORD], g0[WORD]) > 0.4 and R.rel(g2[WORD], g1[WORD]) > 0.5
    for g in (g0, g1, g2):
        assert torch.count_nonzero(g[WORD][PAD]) == 0 and torch.count_nonzero(g[WORD]) > 0


def text_mutant_distances(tc, kw):
    """[(quantity, distance, GPU tolerance)] of a text mutant from the contract (default layout)."""
    terms, g64, r16 = text_reference(tc, FULL, P)
    m_terms, m64 = text_mutant(tc, kw)
    rows = [("loss", abs(m_terms["loss"] - terms["loss"]), R.LOSS_ATOL)]
    for k, g in g64.items():
        zero = float(g.norm()) < 1e-5
        rows.append((k, R.rel(m64[k], g), R.ZERO_REF_TOL if zero else ENVELOPE["max"] * r16[k]))
    return rows


@pytest.mark.parametrize("name", sorted(TEXT_MUTANTS))
def test_text_mutants_move_a_quantity_by_three_times_its_gpu_tolerance(tcase, name):
    rows = text_mutant_distances(tcase, TEXT_MUTANTS[name])
    k, d, tol = max(rows, key=lambda r: r[1] / r[2])
    caught = sum(1 for r in rows if r[1] >= CPU_FACTOR * r[2])
    print(f"{name}: worst {k} distance {d:.3e} = {d / tol:.1f} x tolerance {tol:.3e}; {caught} of {len(rows)} quantities at "
          f">= 3 x; loss moves {rows[0][1]:.3e}")
    assert d / tol >= CPU_FACTOR, (name, k, d, tol)


def test_text_training_reference(tcase):
    """Three AdamW steps of the restatement under the masks of counters +1, +2, +3: the first loss is the single step's,
    and the losses under the masks of ONE counter repeated differ from them by more than the GPU tolerance - a counter that
    stood still would be seen."""
    losses = text_training_losses(tcase)
    assert losses[0] == pytest.approx(text_reference(tcase, FULL, P)[0]["loss"], abs=1e-12)
    stuck = text_training_losses(tcase, advance=0)
    print("text trainer reference", losses, "with the counter standing still", stuck)
    assert max(abs(a - b) for a, b in zip(losses[1:], stuck[1:])) >= CPU_FACTOR * R.LOSS_ATOL


# ====================================================================================== C. accumulation at p = 0.1
GAS, ACC_LR, ACC_MAX_STEPS = 2, 1e-3, 10
ACC_MUTANTS = ("second micro-batch under the first's counter", "sum instead of the mean",
               "second micro-batch's backbone under the previous counter")


def accumulation_case():
    from tests.test_unpad_gpu import _batches

    cfg, sd, tsv_rows, _, _, _ = load_case("g2_hipsmall")
    with torch.no_grad():
        table = orc.build_kg_table(tsv_rows, orc.special_vectors(sd, cfg))
    return dict(cfg=cfg, sd=sd, sd64=R.to64(sd), tsv_rows=tsv_rows, table=table, batches=_batches(cfg, 4), refs=None)


def _micro(ac, sd64, bi, counter, **mutant):
    cfg, batch = ac["cfg"], ac["batches"][bi]
    prov = R.StepDropout(cfg, batch, counter, FULL, P, P, **mutant)
    terms, g64 = R.oracle_step(sd64, cfg, ac["table"], batch, prov)
    return prov, terms, g64


def _mean(a, b, scale=0.5):
    return {k: (a[k] + b[k]) * scale for k in a}


def accumulation_reference(ac, n_steps=2):
    """Per optimizer step: dict(terms = the two micro-batches' fp64 loss terms, g64 = (g(batch 0; c) + g(batch 1; c + 1)) / 2
    on the weights as they are before the step, r16 = the same mean from the autocast oracle against it, micro = the two
    fp64 gradients, sd64 = those weights). The weights move by AdamW on the fp64 mean (`R.adamw_update`)."""
    if ac["refs"] is None:
        sd64 = {k: v.clone() for k, v in ac["sd64"].items()}
        state, steps = orc.AdamState(), []
        for s in range(n_steps):
            c = STEP + GAS * s
            sd32 = {k: v.float() for k, v in sd64.items()}
            micro, micro16, terms = [], [], []
            for j in range(GAS):
                prov, t, g = _micro(ac, sd64, j, c + j)
                _, g16 = R.oracle_step(sd32, ac["cfg"], ac["table"], ac["batches"][j], prov, autocast=True)
                micro.append(g), micro16.append(g16), terms.append(t)
            g64, g16 = _mean(*micro), _mean(*micro16)
            steps.append(dict(terms=terms, g64=g64, r16={k: R.rel(g16[k], g64[k]) for k in g64}, micro=micro,
                              sd64={k: v.clone() for k, v in sd64.items()}, counter=c))
            R.adamw_update(sd64, g64, state, ACC_LR, ACC_MAX_STEPS)
        ac["refs"] = steps
    return ac["refs"]


def accumulation_mutant(ac, name, step=0):
    """(the second micro-batch's loss terms, the step's gradient) of the oracle with the mistake `name`."""
    ref = accumulation_reference(ac)[step]
    c = ref["counter"]
    if name == ACC_MUTANTS[0]:
        _, t, g = _micro(ac, ref["sd64"], 1, c)
        return t, _mean(ref["micro"][0], g)
    if name == ACC_MUTANTS[1]:
        return ref["terms"][1], _mean(*ref["micro"], scale=1.0)
    assert name == ACC_MUTANTS[2]
    _, t, g = _micro(ac, ref["sd64"], 1, c + 1, backbone_base=c)
    return t, _mean(ref["micro"][0], g)


@pytest.fixture(scope="module")
def acase():
    return accumulation_case()


def test_adamw_by_hand_is_train_steps(acase, deterministic):
    """`R.adamw_update` from one micro-batch's gradient is `orc.train_step`, bit for bit, over two steps."""
    cfg, table, batch = acase["cfg"], acase["table"], acase["batches"][0]
    a = {k: v.clone() for k, v in acase["sd64"].items()}
    b = {k: v.clone() for k, v in acase["sd64"].items()}
    sa, sb = orc.AdamState(), orc.AdamState()
    for i in range(2):
        prov = R.StepDropout(cfg, batch, STEP + i, FULL, P, P)
        orc.train_step(a, cfg, table, batch, sa, base_lr=ACC_LR, max_steps=ACC_MAX_STEPS, dropout=prov)
        _, g = R.oracle_step(b, cfg, table, batch, prov)
        R.adamw_update(b, g, sb, ACC_LR, ACC_MAX_STEPS)
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)
    assert sa.step == sb.step == 2


@pytest.mark.parametrize("name", ACC_MUTANTS)
def test_accumulation_mutants_move_a_quantity_by_three_times_its_gpu_tolerance(acase, name):
    ref = accumulation_reference(acase)[0]
    t, g = accumulation_mutant(acase, name)
    rows = [(k, abs(t[k] - ref["terms"][1][k]), R.LOSS_ATOL) for k in R.TERMS]
    for k, g64 in ref["g64"].items():
        zero = float(g64.norm()) < 1e-5
        rows.append((k, R.rel(g[k], g64), R.ZERO_REF_TOL if zero else ENVELOPE["max"] * ref["r16"][k]))
    k, d, tol = max(rows, key=lambda r: r[1] / r[2])
    caught = sum(1 for r in rows if r[1] >= CPU_FACTOR * r[2])
    print(f"{name}: worst {k} distance {d:.3e} = {d / tol:.1f} x tolerance {tol:.3e}; {caught} of {len(rows)} quantities at "
          ">= 3 x")
    assert d / tol >= CPU_FACTOR, (name, k, d, tol)


def test_the_second_step_runs_on_moved_weights(acase):
    """Step 2's reference stands on step 1's AdamW result: the weights moved by lr per element at most, and step 2's
    gradient on the stored weights would be told from the one on the moved weights."""
    s0, s1 = accumulation_reference(acase)
    k = "bert.encoder.layer.0.attention.self.query.weight"
    moved = (s1["sd64"][k] - s0["sd64"][k]).abs()
    assert 0 < float(moved.max()) <= ACC_LR * 1.0001
    assert s1["counter"] == s0["counter"] + GAS == STEP + 2
