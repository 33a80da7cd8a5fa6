"""Which elements one TRAINING STEP drops, restated from the engine's contract - numpy / torch only, nothing imported from
``stonkgs_amd.engine``. ``oracle/dropout_oracle.py`` says what a kernel drops given (seed, row, column); this module says
which seed and which row index every launch of a step is given, so that ``oracle/stonkgs_oracle.py`` (``dropout=``) can
replay the step's masks element by element and torch autograd yields the exact gradients under dropout.

The contract (``StepDropout`` is its statement; tests/test_step_dropout_gpu.py holds the engine to it):

  seed(layer, site) = (seed_base * 0x9E3779B1 + layer * 64 + site) mod 2^32, seed_base = the step's counter: the value
    AFTER the increment that opens the step's ``encode``.
  frozen backbone (dropout live, quirk Q6): always padded, B x half rows, no key mask. Embeddings (100, 0); layer i is
    101 + i with sites 1 (softmax probabilities), 2 (attention.output.dense), 3 (output.dense).
  trainable encoder: joint embeddings (200, 0); layer i is i, sites 1, 2, 3; classifier (300, 0) in the flat form (row 0,
    column b * H + c).
  element form (sites 0, 2, 3): row = the launch's output row, column = the hidden index. Padded layout: b * S + pos.
    Packed layout: row_of_pos[b * S + pos] of ``masking_oracle.unpad_plan``. Pruned last layer: the READ-row index
    read_of_pos[b * S + pos] - site 3 whenever `prune_last_ffn`, site 2 too when `prune_last_attn`.
  block form (site 1): row = (b * NH + h) * S_launch + q, key = k; S_launch = half in the backbone, S in the encoder; q and k
    are counted inside the sequence's packed rows (padded layout: the position).
  a position without a row in the layout at a site: mask 1 (nothing reads it - test_step_dropout_ref_cpu.py proves that by
    dropping everything there instead).

Every departure from the contract that a test wants to see caught is a keyword of ``StepDropout`` (the mutants of
tests/test_step_dropout_ref_cpu.py); all of them default to the contract."""
from __future__ import annotations

import contextlib
import re
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import dropout_oracle as do
from oracle import stonkgs_oracle as orc
from oracle.masking_oracle import unpad_plan

GOLDEN_RATIO = 0x9E3779B1
BACKBONE_EMB, BACKBONE_LAYER0, JOINT_EMB, CLASSIFIER = 100, 101, 200, 300
LAYOUTS = ((False, False, False), (True, False, False), (True, True, False), (True, True, True))
TERMS = ("loss", "masked_lm_loss", "ent_masked_lm_loss", "next_sentence_loss")


def seed_of(seed_base: int, layer: int, site: int) -> int:
    return (int(seed_base) * GOLDEN_RATIO + layer * 64 + site) & 0xFFFFFFFF


def drop_scale(p: float) -> float:
    """1 / (1 - p) as the launchers compute it: in float32, from p rounded to float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


class StepDropout:
    """The keep-masks of one step (``keep(site_key, shape)`` of ``stonkgs_oracle._drop``), scaled by 1 / (1 - float32(p)).

    cfg, batch: the oracle's config and the batch (``attention_mask`` None = every key live, padded layout only).
    seed_base: the counter the step runs under. layout: (unpad, prune_last_ffn, prune_last_attn) of the engine.
    labels: "batch" = the pre-training labels of `batch` decide the read rows; (None, None) = a head that reads position 0
    only (sequence classification).

    Mutant keywords (default = the contract):
      seed_delta       {(layer, site): d} - that launch's seed is off by d
      backbone_base    the counter the frozen backbone's launches use instead of seed_base
      rows             "contract" | "padded": padded row indices where the packed row belongs
      read_rows        sites (subset of {2, 3}) of the pruned last layer that use the PACKED row where the read row belongs
      attn_index       "packed" | "position": query / key counted by original position in the packed layout
      backward_seed_delta  {(layer, site): d} - that site's BACKWARD mask is drawn with a seed off by d
      norow            "ones" | "zeros": the mask of positions without a row (zeros: everything there is dropped)"""

    def __init__(self, cfg, batch, seed_base: int, layout=(True, True, True), p_hid: float = 0.1, p_att: float = 0.1, *,
                 labels="batch", seed_delta: Optional[Dict[Tuple[int, int], int]] = None,
                 backbone_base: Optional[int] = None, rows: str = "contract", read_rows=(), attn_index: str = "packed",
                 backward_seed_delta: Optional[Dict[Tuple[int, int], int]] = None, norow: str = "ones"):
        self.cfg, self.seed_base, self.p_hid, self.p_att = cfg, int(seed_base), float(p_hid), float(p_att)
        self.seed_delta = dict(seed_delta or {})
        self.backward_seed_delta = dict(backward_seed_delta or {})
        self.backbone_base = self.seed_base if backbone_base is None else int(backbone_base)
        self.rows_rule, self.read_sites_wrong, self.attn_index, self.norow = rows, set(read_rows), attn_index, norow
        ids = np.asarray(batch["input_ids"])
        self.B, self.S = ids.shape
        self.half, self.H, self.NH = cfg.half_length, cfg.hidden_size, cfg.num_attention_heads
        self.last = cfg.num_hidden_layers - 1
        unpad, prune_ffn, prune_attn = layout
        am = batch.get("attention_mask")
        self.packed = bool(unpad) and am is not None
        self.prune_ffn = self.packed and bool(prune_ffn)
        self.prune_attn = self.prune_ffn and bool(prune_attn)
        B, S = self.B, self.S
        self.padded_row = np.arange(B * S, dtype=np.int64)
        if self.packed:
            tl, el = (batch["masked_lm_labels"], batch["ent_masked_lm_labels"]) if labels == "batch" else labels
            rop, _, offs, _, _, read_of_pos, _ = unpad_plan(np.asarray(am), None if tl is None else np.asarray(tl),
                                                            None if el is None else np.asarray(el), read=True)
            self.row_of_pos = rop.astype(np.int64)
            self.read_of_pos = read_of_pos.astype(np.int64)
            # a position's index inside its sequence's packed rows (-1: no row)
            first = np.repeat(offs[:B].astype(np.int64), S)
            self.local = np.where(self.row_of_pos >= 0, self.row_of_pos - first, -1)
        else:
            self.row_of_pos = self.padded_row
            self.read_of_pos = None
            self.local = np.tile(np.arange(S, dtype=np.int64), B)
        self._cache: Dict[tuple, torch.Tensor] = {}

    # ------------------------------------------------------------------ (layer, site) of an oracle site key
    def launch(self, site_key):
        """(tower, layer index of the seed, site, encoder layer number or None) of `site_key` = (HF module prefix, site)."""
        prefix, site = site_key
        if prefix == "classifier":
            return "cls", CLASSIFIER, 0, None
        tower = "bb" if prefix.startswith("lm_backbone.") else "enc"
        if prefix.endswith(".embeddings"):
            return tower, BACKBONE_EMB if tower == "bb" else JOINT_EMB, 0, None
        i = int(re.search(r"\.layer\.(\d+)$", prefix).group(1))
        return tower, (BACKBONE_LAYER0 + i) if tower == "bb" else i, site, i

    def seed(self, tower, layer, site, backward=False) -> int:
        base = self.backbone_base if tower == "bb" else self.seed_base
        d = self.seed_delta.get((layer, site), 0)
        if backward:
            d += self.backward_seed_delta.get((layer, site), 0)
        return (seed_of(base, layer, site) + d) & 0xFFFFFFFF

    # ------------------------------------------------------------------ rows
    def element_rows(self, tower, site, i) -> np.ndarray:
        """int64 [B * S_tower]: the row index that keys every position's mask at an element-form site (-1: no row)."""
        if tower == "bb":
            return np.arange(self.B * self.half, dtype=np.int64)
        if not self.packed:
            return self.padded_row
        pruned = i == self.last and ((site == 3 and self.prune_ffn) or (site == 2 and self.prune_attn))
        if pruned:
            if site in self.read_sites_wrong:      # (mutant: the packed row - of the positions that have a read row)
                return np.where(self.read_of_pos >= 0, self.row_of_pos, -1)
            return self.read_of_pos
        if self.rows_rule == "padded":             # (mutant)
            return np.where(self.row_of_pos >= 0, self.padded_row, -1)
        return self.row_of_pos

    # ------------------------------------------------------------------ masks
    def _fill(self):
        return 1.0 if self.norow == "ones" else 0.0

    def _element(self, tower, layer, site, i, shape, backward) -> np.ndarray:
        B, S, H = shape
        rows = self.element_rows(tower, site, i)
        assert rows.shape[0] == B * S and H == self.H, (shape, rows.shape)
        out = np.full((B * S, H), self._fill())
        has = rows >= 0
        k = do.keep(rows[has], np.arange(H), self.seed(tower, layer, site, backward), self.p_hid)
        out[has] = k * drop_scale(self.p_hid)
        return out.reshape(B, S, H)

    def _attention(self, tower, layer, i, shape, backward) -> np.ndarray:
        B, NH, S, S2 = shape
        assert S == S2 and NH == self.NH
        seed = self.seed(tower, layer, 1, backward)
        out = np.full(shape, self._fill())
        for b in range(B):
            if tower == "bb" or not self.packed:
                pos, idx = np.arange(S), np.arange(S)
            else:
                loc = self.local[b * S:(b + 1) * S]
                pos = np.nonzero(loc >= 0)[0]
                idx = pos if self.attn_index == "position" else loc[pos]
            for h in range(NH):
                k = do.keep_block((b * NH + h) * S + idx, idx, seed, self.p_att)
                out[b, h][np.ix_(pos, pos)] = k * drop_scale(self.p_att)
        return out

    def _mask(self, site_key, shape, backward: bool) -> torch.Tensor:
        tower, layer, site, i = self.launch(site_key)
        key = (site_key, tuple(shape), self.seed(tower, layer, site, backward))
        m = self._cache.get(key)
        if m is None:
            if tower == "cls":
                B, H = shape
                m = do.keep_flat(B * H, self.seed(tower, layer, site, backward), self.p_hid).reshape(B, H) * drop_scale(self.p_hid)
            elif site == 1:
                m = self._attention(tower, layer, i, shape, backward)
            else:
                m = self._element(tower, layer, site, i, shape, backward)
            m = self._cache[key] = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64))
        return m

    def keep(self, site_key, shape) -> torch.Tensor:
        return self._mask(site_key, shape, False)

    def keep_backward(self, site_key, shape) -> torch.Tensor:
        return self._mask(site_key, shape, True)

    def keep_bool(self, site_key, shape) -> np.ndarray:
        """The forward mask as booleans (for the tests of the masks themselves)."""
        return self.keep(site_key, shape).numpy() != 0

    def sites(self, classifier: bool = False):
        """(site key, shape) of every dropout site of one step, in execution order."""
        cfg, B, S, half, H, NH = self.cfg, self.B, self.S, self.half, self.H, self.NH
        out = [(("lm_backbone.embeddings", 0), (B, half, H))]
        for i in range(cfg.n_backbone_layers):
            p = f"lm_backbone.encoder.layer.{i}"
            out += [((p, 1), (B, NH, half, half)), ((p, 2), (B, half, H)), ((p, 3), (B, half, H))]
        out.append((("bert.embeddings", 0), (B, S, H)))
        for i in range(cfg.num_hidden_layers):
            p = f"bert.encoder.layer.{i}"
            out += [((p, 1), (B, NH, S, S)), ((p, 2), (B, S, H)), ((p, 3), (B, S, H))]
        if classifier:
            out.append((("classifier", 0), (B, H)))
        return out


# ---------------------------------------------------------------------------------------- the oracle's step
def to64(sd):
    return {k: v.double() for k, v in sd.items()}


def oracle_step(sd, cfg, table, batch, dropout, autocast: bool = False):
    """(loss terms {name: float}, gradients {name: tensor}) of the pre-training step on the weights `sd` (fp64 weights: an
    fp64 step) with the masks of `dropout`; `autocast`: under torch.autocast("cpu", bfloat16), the reference's own reduced
    precision (tests/test_losscurve_gpu.py)."""
    names = orc.trainable_names(sd)
    params = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    work = dict(sd)
    work.update(params)
    with torch.autocast("cpu", dtype=torch.bfloat16) if autocast else contextlib.nullcontext():
        out = orc.forward(work, cfg, table, **batch, dropout=dropout)
    grads = torch.autograd.grad(out["loss"], [params[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(sd[k]) if g is None else g.detach()) for k, g in zip(names, grads)}
    return {k: float(out[k].detach()) for k in TERMS}, grads


def oracle_cls_step(sd, cfg, table, inputs, labels, dropout, autocast: bool = False):
    """The same for the sequence-classification step: ({"loss": float}, gradients of `bert.*` and `classifier.*`)."""
    names = [k for k in sd if (k.startswith("bert.") and "word_embeddings" not in k) or k.startswith("classifier.")]
    params = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    work = dict(sd)
    work.update(params)
    with torch.autocast("cpu", dtype=torch.bfloat16) if autocast else contextlib.nullcontext():
        out = orc.forward_classification(work, cfg, table, **inputs, labels=labels, dropout=dropout)
    grads = torch.autograd.grad(out["loss"], [params[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(sd[k]) if g is None else g.detach()) for k, g in zip(names, grads)}
    return {"loss": float(out["loss"].detach())}, grads


def oracle_text_step(sd, cfg, batch, dropout, autocast: bool = False):
    """The same for the text-only classifier (tests/test_text_embed_cpu.text_classifier, which transformers'
    BertForSequenceClassification pins at p = 0): ({"loss": float}, gradients of EVERY parameter, the word table included -
    its pad row is read detached and stays zero)."""
    from tests.test_text_embed_cpu import text_classifier

    names = list(sd)
    params = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    with torch.autocast("cpu", dtype=torch.bfloat16) if autocast else contextlib.nullcontext():
        out = text_classifier(params, cfg, batch["input_ids"], batch["attention_mask"], batch["token_type_ids"],
                              batch["labels"], dropout=dropout)
    grads = torch.autograd.grad(out["loss"], [params[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(sd[k]) if g is None else g.detach()) for k, g in zip(names, grads)}
    return {"loss": float(out["loss"].detach())}, grads


def adamw_update(sd, grads, state, base_lr: float, max_steps: int, max_grad_norm: float = 1.0, betas=(0.9, 0.999),
                 eps: float = 1e-8) -> None:
    """The optimizer half of ``orc.train_step`` (clip by the global norm, AdamW without weight decay, linear schedule) from
    gradients the caller has: the mean over the micro-batches of an accumulation window, or a model ``train_step`` does not
    know. Updates `sd` and `state` (``orc.AdamState``) in place."""
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).float())
    coef = min(1.0, max_grad_norm / (total + 1e-6)) if max_grad_norm and max_grad_norm > 0 else 1.0
    lr = orc.linear_schedule_lr(base_lr, state.step, max_steps)
    state.step += 1
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** state.step, 1 - b2 ** state.step
    with torch.no_grad():
        for k, g in grads.items():
            g = g * coef
            m = state.m.setdefault(k, torch.zeros_like(sd[k]))
            v = state.v.setdefault(k, torch.zeros_like(sd[k]))
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            sd[k].addcdiv_(m, (v.sqrt() / (bc2 ** 0.5)).add_(eps), value=-lr / bc1)


def rel(a, b) -> float:
    """Relative L2 distance of `a` from the reference `b`; a reference that is analytically zero (key.bias) is compared on
    the absolute scale tests/test_model_gpu.py uses."""
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).detach().double().cpu().flatten()
    if float(b.norm()) < 1e-5:
        return float((a - b).norm()) / 1e-2
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------------------- the comparison
LOSS_ATOL = 1e-2   # |loss term - oracle|: the project's bound (tests/test_model_gpu.py)
ZERO_REF_TOL = 1.0  # an analytically zero tensor: |d| < 1e-2 in `rel`'s absolute scale


def grad_ratios(grads, ref64, r16):
    """[(name, err, r16, err / r16)] over the tensors of `ref64` that `grads` has, key.bias-like zero references left out
    of the ratios (they are held on the absolute scale by `compare`)."""
    rows = []
    for k, g in ref64.items():
        if k not in grads:
            continue
        e = rel(grads[k], g)
        if float(g.double().norm()) < 1e-5:
            continue
        rows.append((k, e, r16[k], e / max(r16[k], 1e-6)))
    return rows


def compare(terms, grads, ref_terms, ref64, r16, envelope) -> list:
    """The GPU tests' comparison: every violated condition as a string (empty: the step agrees with the oracle).
    Conditions: every loss term within LOSS_ATOL; median over tensors of err / r16 <= envelope["median"]; every tensor's
    err / r16 <= envelope["max"]; zero-reference tensors within 1e-2 absolute."""
    bad = [f"{k}: {terms[k]:.5f} vs {ref_terms[k]:.5f}" for k in ref_terms if abs(terms[k] - ref_terms[k]) >= LOSS_ATOL]
    rows = grad_ratios(grads, ref64, r16)
    med = float(np.median([r[3] for r in rows]))
    if med > envelope["median"]:
        bad.append(f"median ratio {med:.2f} > {envelope['median']}")
    bad += [f"{k}: err {e:.3e} = {q:.2f} x r16 {r:.3e}" for k, e, r, q in rows if q > envelope["max"]]
    for k, g in ref64.items():
        if k in grads and float(g.double().norm()) < 1e-5 and rel(grads[k], g) >= ZERO_REF_TOL:
            bad.append(f"{k}: zero reference, |d| {rel(grads[k], g) * 1e-2:.3e}")
    return bad


def describe(tag, grads, ref64, r16) -> str:
    rows = grad_ratios(grads, ref64, r16)
    q = np.array([r[3] for r in rows])
    worst = sorted(rows, key=lambda r: -r[3])[:5]
    return (f"{tag}: {len(q)} tensors, err/r16 median {np.median(q):.2f} p90 {np.percentile(q, 90):.2f} max {q.max():.2f}; "
            f"worst {[(k, f'{e:.2e}', f'{r:.2e}', f'{x:.2f}') for k, e, r, x in worst]}")
