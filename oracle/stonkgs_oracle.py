"""CPU oracle for the STonKGs pre-training hot path  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Only ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline`` leg of ``bench.py`` may import this
module; the product (``stonkgs_amd``) never does and has no CPU fallback.

What it is: a plain-PyTorch fp32 restatement (no ``transformers`` import, no reference import) of
  * ``STonKGsForPreTraining.forward``            ref:src/stonkgs/models/stonkgs_model.py:149-258
  * ``STonKGsELMPredictionHead.forward``         ref:src/stonkgs/models/stonkgs_model.py:62-73
  * the KG-backbone index space / special vectors ref:src/stonkgs/models/stonkgs_model.py:123-141
  * the BERT arithmetic the reference delegates to HuggingFace (third-party dependency, NOT vendored under
    /root/reference; reference pins ``transformers>=4.6.1`` in ref:setup.cfg:80, 5.15.0 installed here):
    hf:models/bert/modeling_bert.py BertEmbeddings :98-108, BertSelfAttention :164-203 (eager :111-136),
    BertSelfOutput :289-293, BertIntermediate :334-337, BertOutput :347-351, BertPooler :457-463,
    BertPredictionHeadTransform :476-480, seq_relationship :523-527
  * the optimizer step the reference's driver runs through HF ``Trainer``
    (ref:src/stonkgs/models/stonkgs_pretraining.py:171-223 -> hf:trainer.py:1780-1796): clip_grad_norm_(1.0),
    AdamW(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0), linear decay to 0 with no warm-up
  * the offline masking that defines the batch schema
    ref:src/stonkgs/data/indra_for_pretraining.py:33-77 (replace_mlm_tokens), :80-126 (NSP negatives).

Dropout: off by default (every `dropout=None`: no operation is added, the golden vectors are replayed bit for bit). With a
mask provider (`_drop`; tests/step_dropout_ref.py) the keep-masks are multiplied in where hf drops and the engine does:
behind both embeddings LayerNorms, on the softmax probabilities, on the two output projections before their residual, on
the pooled vector before the classifier - torch autograd then gives the exact gradients of a step under THOSE masks.

Pinning: the reference's own test-suite holds no vectors for this path, so the oracle is
pinned against the reference ITSELF, imported in the authoring container by ``oracle/make_golden.py`` (reference
``forward`` unmodified + HF BERT, local config, random weights); the resulting inputs/outputs are committed under
``tests/golden/`` and ``tests/test_oracle_golden.py`` replays them without the reference.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor


@dataclass
class OracleConfig:
    vocab_size: int = 28996
    kg_vocab_size: int = 175094
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    layer_norm_eps: float = 1e-12
    # the LM backbone may be shaped differently from the trainable encoder only in depth / position count
    backbone_layers: Optional[int] = None

    @property
    def half_length(self) -> int:  # ref:stonkgs_model.py:52
        return self.max_position_embeddings // 2

    @property
    def n_backbone_layers(self) -> int:
        return self.num_hidden_layers if self.backbone_layers is None else self.backbone_layers


SPECIAL_IDS = (102, 103, 100)  # [SEP], [MASK], [UNK] of BioBERT's vocab (ref:stonkgs_model.py:116-118)


# --------------------------------------------------------------------------------------------- index space
def kg_row_of_entity_id(e: int) -> Optional[int]:
    """Quirk Q1: model index -> TSV row.  numeric_indices = [0..K+2] \\ {100,102,103} (ref:stonkgs_model.py:123-129).

    Returns None for the three reserved ids (they map to LM special-token vectors instead)."""
    if e in SPECIAL_IDS:
        return None
    return e - sum(1 for s in SPECIAL_IDS if s < e)


def build_kg_table(tsv_rows: Tensor, special_vectors: Dict[int, Tensor]) -> Tensor:
    """Dense [K+3, H] table indexed by the MODEL's entity id (what ``self.kg_backbone[i]`` returns).

    tsv_rows: [K, H] float64 as read by prepare_df (ref:kg_baseline_model.py:270-280); the reference casts the
    gathered fp64 rows to CPU fp32 (ref:stonkgs_model.py:193-200), i.e. round-to-nearest, done here once."""
    K, H = tsv_rows.shape
    table = torch.empty(K + 3, H, dtype=torch.float32)
    for e in range(K + 3):
        r = kg_row_of_entity_id(e)
        table[e] = special_vectors[e].to(torch.float32) if r is None else tsv_rows[r].to(torch.float32)
    return table


# --------------------------------------------------------------------------------------------- BERT pieces
def _ln(x: Tensor, sd: Dict[str, Tensor], prefix: str, eps: float) -> Tensor:
    return F.layer_norm(x, (x.shape[-1],), sd[prefix + ".weight"], sd[prefix + ".bias"], eps)


def _linear(x: Tensor, sd: Dict[str, Tensor], prefix: str) -> Tensor:
    return F.linear(x, sd[prefix + ".weight"], sd.get(prefix + ".bias"))


class _MaskMul(torch.autograd.Function):
    """y = x * fwd, dx = dy * bwd. The two masks are one tensor in normal use; a test that wants to know what a backward
    with ANOTHER mask than the forward's would compute hands in two."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.save_for_backward(bwd)
        return x * fwd

    @staticmethod
    def backward(ctx, g):
        (bwd,) = ctx.saved_tensors
        return g * bwd, None, None


def _drop(x: Tensor, dropout, site_key) -> Tensor:
    """Dropout at the site `site_key` = (HF module prefix, site): 0 = behind an embeddings LayerNorm / on the pooled
    vector, 1 = the softmax probabilities, 2 = attention.output.dense, 3 = output.dense.
    `dropout` None: x itself (p = 0, no operation added). Else an object with `keep(site_key, shape) -> Tensor`, the {0, 1}
    keep-mask already scaled by 1 / (1 - float32(p)) (tests/step_dropout_ref.py derives it from the engine's seed and row
    contract and oracle/dropout_oracle.py); an optional `keep_backward(site_key, shape)` gives the mask of the backward."""
    if dropout is None:
        return x
    dt = torch.promote_types(x.dtype, torch.float32)   # (under autocast x may be bf16: the product is taken in fp32)
    fwd = dropout.keep(site_key, tuple(x.shape)).to(dt)
    kb = getattr(dropout, "keep_backward", None)
    bwd = fwd if kb is None else kb(site_key, tuple(x.shape)).to(dt)
    return _MaskMul.apply(x, fwd, bwd)


def bert_embeddings(sd, prefix, cfg, *, input_ids=None, inputs_embeds=None, token_type_ids=None, dropout=None) -> Tensor:
    """hf BertEmbeddings.forward :98-108 (absolute positions; `dropout` None: p = 0 / eval, else see `_drop`)."""
    if inputs_embeds is None:
        inputs_embeds = sd[prefix + ".word_embeddings.weight"][input_ids]
    B, S = inputs_embeds.shape[:2]
    if token_type_ids is None:
        token_type_ids = torch.zeros(B, S, dtype=torch.long)
    pos = sd[prefix + ".position_embeddings.weight"][:S][None]
    typ = sd[prefix + ".token_type_embeddings.weight"][token_type_ids]
    return _drop(_ln(inputs_embeds + typ + pos, sd, prefix + ".LayerNorm", cfg.layer_norm_eps), dropout, (prefix, 0))


def bert_layer(x: Tensor, sd, prefix: str, cfg: OracleConfig, mask_bias: Optional[Tensor], dropout=None) -> Tensor:
    """hf BertLayer. Dropout (`_drop`) where hf has it: on the softmax probabilities (BertSelfAttention :195) and on
    dense(x) + bias of BertSelfOutput :291 / BertOutput :349, before the residual is added."""
    B, S, H = x.shape
    nh = cfg.num_attention_heads
    d = H // nh

    def heads(t):
        return t.view(B, S, nh, d).transpose(1, 2)

    q = heads(_linear(x, sd, prefix + ".attention.self.query"))
    k = heads(_linear(x, sd, prefix + ".attention.self.key"))
    v = heads(_linear(x, sd, prefix + ".attention.self.value"))
    scores = q @ k.transpose(-1, -2) / math.sqrt(d)
    if mask_bias is not None:
        scores = scores + mask_bias
    ctx = (_drop(torch.softmax(scores, dim=-1), dropout, (prefix, 1)) @ v).transpose(1, 2).reshape(B, S, H)
    h1 = _ln(_drop(_linear(ctx, sd, prefix + ".attention.output.dense"), dropout, (prefix, 2)) + x, sd,
             prefix + ".attention.output.LayerNorm", cfg.layer_norm_eps)
    inter = F.gelu(_linear(h1, sd, prefix + ".intermediate.dense"))  # exact erf GELU (hidden_act="gelu")
    return _ln(_drop(_linear(inter, sd, prefix + ".output.dense"), dropout, (prefix, 3)) + h1, sd,
               prefix + ".output.LayerNorm", cfg.layer_norm_eps)


def bert_encoder(x, sd, prefix, cfg, n_layers, attention_mask=None, collect: Optional[list] = None,
                 dropout=None) -> Tensor:
    mask_bias = None
    if attention_mask is not None:  # additive key-padding mask [B,1,1,S]
        mask_bias = (1.0 - attention_mask[:, None, None, :].to(x.dtype)) * torch.finfo(x.dtype).min
    for i in range(n_layers):
        x = bert_layer(x, sd, f"{prefix}.layer.{i}", cfg, mask_bias, dropout)
        if collect is not None:
            collect.append(x)
    return x


def lm_backbone_forward(sd, cfg: OracleConfig, input_ids: Tensor, dropout=None) -> Tensor:
    """`self.lm_backbone(ids)[0]`: full BERT forward, NO attention mask (quirk Q5, ref:stonkgs_model.py:178). In training
    mode its dropout is live although it is frozen (quirk Q6): `dropout` reaches every site of it."""
    x = bert_embeddings(sd, "lm_backbone.embeddings", cfg, input_ids=input_ids, dropout=dropout)
    return bert_encoder(x, sd, "lm_backbone.encoder", cfg, cfg.n_backbone_layers, dropout=dropout)


def special_vectors(sd, cfg: OracleConfig) -> Dict[int, Tensor]:
    """Quirk Q2: kg_backbone[sid] = lm_backbone([[sid]])[0][0][0] (ref:stonkgs_model.py:138-141)."""
    return {sid: lm_backbone_forward(sd, cfg, torch.tensor([[sid]]))[0, 0] for sid in SPECIAL_IDS}


# --------------------------------------------------------------------------------------------- the hot function
def _embeds_dtype(token_embeddings: Tensor) -> torch.dtype:
    """fp32, as the reference casts the concatenation (ref:stonkgs_model.py:193-200) - unless the oracle is run in fp64 as a
    whole (fp64 weights: a higher-precision yardstick for the tests), which then stays fp64."""
    return torch.float64 if token_embeddings.dtype == torch.float64 else torch.float32


def forward(sd: Dict[str, Tensor], cfg: OracleConfig, kg_table: Tensor, input_ids: Tensor,
            attention_mask: Optional[Tensor] = None, token_type_ids: Optional[Tensor] = None,
            masked_lm_labels: Optional[Tensor] = None, ent_masked_lm_labels: Optional[Tensor] = None,
            next_sentence_labels: Optional[Tensor] = None, collect_layers: bool = False,
            dropout=None) -> Dict[str, Tensor]:
    """ref:src/stonkgs/models/stonkgs_model.py:149-258, step numbers as in SURVEY.md section 3.2. `dropout`: see `_drop`
    (the pooler and the head transform have none)."""
    half = cfg.half_length
    # 1. frozen LM backbone on the text half
    token_embeddings = lm_backbone_forward(sd, cfg, input_ids[:, :half], dropout)
    # 2. KG gather (KeyError for ids outside the table, like the reference's dict lookup)
    ent_ids = input_ids[:, half:]
    if ent_ids.numel() and (int(ent_ids.min()) < 0 or int(ent_ids.max()) >= kg_table.shape[0]):
        raise KeyError(int(ent_ids.max()))
    ent_embeddings = kg_table[ent_ids]
    # 3. concat, fp32
    inputs_embeds = torch.cat([token_embeddings, ent_embeddings], dim=1).to(_embeds_dtype(token_embeddings))
    # 4. trainable encoder + pooler
    emb = bert_embeddings(sd, "bert.embeddings", cfg, inputs_embeds=inputs_embeds, token_type_ids=token_type_ids,
                          dropout=dropout)
    layers: Optional[list] = [] if collect_layers else None
    seq = bert_encoder(emb, sd, "bert.encoder", cfg, cfg.num_hidden_layers, attention_mask, layers, dropout)
    pooled = torch.tanh(_linear(seq[:, 0], sd, "bert.pooler.dense"))
    # 6. heads
    t = _ln(F.gelu(_linear(seq, sd, "cls.predictions.transform.dense")), sd, "cls.predictions.transform.LayerNorm",
            cfg.layer_norm_eps)
    text_logits = F.linear(t[:, :half], sd["cls.predictions.text_decoder.weight"])
    ent_logits = F.linear(t[:, half:], sd["cls.predictions.entity_decoder.weight"])
    nsp_logits = _linear(pooled, sd, "cls.seq_relationship")
    out = {"inputs_embeds": inputs_embeds, "embedding_output": emb, "hidden_states": seq, "pooler_output": pooled,
           "transform_output": t, "text_logits": text_logits, "ent_logits": ent_logits, "nsp_logits": nsp_logits}
    if collect_layers:
        out["layers"] = layers
    # 7. loss
    if masked_lm_labels is not None and ent_masked_lm_labels is not None and next_sentence_labels is not None:
        lt = F.cross_entropy(text_logits.reshape(-1, cfg.vocab_size), masked_lm_labels.reshape(-1))
        le = F.cross_entropy(ent_logits.reshape(-1, cfg.kg_vocab_size), ent_masked_lm_labels.reshape(-1))
        ln = F.cross_entropy(nsp_logits.reshape(-1, 2), next_sentence_labels.reshape(-1))
        out.update(loss=lt + le + ln, masked_lm_loss=lt, ent_masked_lm_loss=le, next_sentence_loss=ln)
    return out


def encode(sd, cfg: OracleConfig, kg_table: Tensor, input_ids, attention_mask=None, token_type_ids=None, dropout=None):
    """Shared front of both models: steps 1-4 of `forward` (sequence_output, pooled_output)."""
    half = cfg.half_length
    token_embeddings = lm_backbone_forward(sd, cfg, input_ids[:, :half], dropout)
    ent_ids = input_ids[:, half:]
    if ent_ids.numel() and (int(ent_ids.min()) < 0 or int(ent_ids.max()) >= kg_table.shape[0]):
        raise KeyError(int(ent_ids.max()))
    inputs_embeds = torch.cat([token_embeddings, kg_table[ent_ids]], dim=1).to(_embeds_dtype(token_embeddings))
    emb = bert_embeddings(sd, "bert.embeddings", cfg, inputs_embeds=inputs_embeds, token_type_ids=token_type_ids,
                          dropout=dropout)
    seq = bert_encoder(emb, sd, "bert.encoder", cfg, cfg.num_hidden_layers, attention_mask, dropout=dropout)
    return seq, torch.tanh(_linear(seq[:, 0], sd, "bert.pooler.dense"))


def forward_classification(sd, cfg: OracleConfig, kg_table: Tensor, input_ids, attention_mask=None, token_type_ids=None,
                           labels=None, problem_type: str = "single_label_classification",
                           dropout=None) -> Dict[str, Tensor]:
    """STonKGsForSequenceClassification.forward (ref:src/stonkgs/models/stonkgs_finetuning.py:259-346): same embedding
    front and encoder, pooled -> dropout (`dropout` None: p = 0; else `_drop` at ("classifier", 0)) -> classifier -> the
    loss of `problem_type` (:328-338): CrossEntropyLoss / MSELoss on logits.view(-1, num_labels) (torch's own broadcasting
    included) / BCEWithLogitsLoss."""
    seq, pooled = encode(sd, cfg, kg_table, input_ids, attention_mask, token_type_ids, dropout)
    logits = _linear(_drop(pooled, dropout, ("classifier", 0)), sd, "classifier")
    out = {"logits": logits, "pooler_output": pooled, "hidden_states": seq}
    if labels is not None:
        nl = logits.shape[-1]
        if problem_type == "regression":
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")   # ([B,1] against [B]: broadcast to [B,B], as in the reference)
                out["loss"] = F.mse_loss(logits.view(-1, nl), labels)
        elif problem_type == "multi_label_classification":
            out["loss"] = F.binary_cross_entropy_with_logits(logits, labels)
        else:
            out["loss"] = F.cross_entropy(logits.view(-1, nl), labels.view(-1))
    return out


# --------------------------------------------------------------------------------------------- parameters
def trainable_names(sd: Dict[str, Tensor]) -> List[str]:
    """Parameters that receive a gradient in the reference (quirk Q4 removes the dead ones, lm_backbone is frozen)."""
    dead = ("bert.embeddings.word_embeddings.weight", "cls.predictions.bias", "cls.predictions.decoder.weight",
            "cls.predictions.decoder.bias", "cls.predictions.text_bias", "cls.predictions.entity_bias",
            "cls.predictions.decoder.text_bias", "cls.predictions.decoder.entity_bias")
    return [k for k in sd if not k.startswith("lm_backbone.") and k not in dead]


def init_state_dict(cfg: OracleConfig, seed: int = 0, std: float = 0.02, bf16_exact: bool = True) -> Dict[str, Tensor]:
    """Random-init weights in HF layout (N(0, std) matrices/embeddings, zero biases, unit LayerNorm), optionally
    rounded to bf16-representable values so a bf16 implementation starts from bit-identical weights."""
    g = torch.Generator().manual_seed(seed)
    H, I = cfg.hidden_size, cfg.intermediate_size
    sd: Dict[str, Tensor] = {}

    def mat(*shape):
        w = torch.randn(*shape, generator=g) * std
        return w.to(torch.bfloat16).to(torch.float32) if bf16_exact else w

    def vec(n, noise=0.0, base=0.0):
        w = base + torch.randn(n, generator=g) * noise
        return w.to(torch.bfloat16).to(torch.float32) if bf16_exact else w

    def bert(prefix, n_layers, with_pooler=True):
        sd[prefix + ".embeddings.word_embeddings.weight"] = mat(cfg.vocab_size, H)
        sd[prefix + ".embeddings.position_embeddings.weight"] = mat(cfg.max_position_embeddings, H)
        sd[prefix + ".embeddings.token_type_embeddings.weight"] = mat(cfg.type_vocab_size, H)
        sd[prefix + ".embeddings.LayerNorm.weight"] = vec(H, 0.05, 1.0)
        sd[prefix + ".embeddings.LayerNorm.bias"] = vec(H, 0.02)
        for i in range(n_layers):
            p = f"{prefix}.encoder.layer.{i}"
            for n in ("query", "key", "value"):
                sd[f"{p}.attention.self.{n}.weight"] = mat(H, H)
                sd[f"{p}.attention.self.{n}.bias"] = vec(H, 0.02)
            sd[f"{p}.attention.output.dense.weight"] = mat(H, H)
            sd[f"{p}.attention.output.dense.bias"] = vec(H, 0.02)
            sd[f"{p}.attention.output.LayerNorm.weight"] = vec(H, 0.05, 1.0)
            sd[f"{p}.attention.output.LayerNorm.bias"] = vec(H, 0.02)
            sd[f"{p}.intermediate.dense.weight"] = mat(I, H)
            sd[f"{p}.intermediate.dense.bias"] = vec(I, 0.02)
            sd[f"{p}.output.dense.weight"] = mat(H, I)
            sd[f"{p}.output.dense.bias"] = vec(H, 0.02)
            sd[f"{p}.output.LayerNorm.weight"] = vec(H, 0.05, 1.0)
            sd[f"{p}.output.LayerNorm.bias"] = vec(H, 0.02)
        if with_pooler:
            sd[prefix + ".pooler.dense.weight"] = mat(H, H)
            sd[prefix + ".pooler.dense.bias"] = vec(H, 0.02)

    bert("bert", cfg.num_hidden_layers)
    sd["cls.predictions.bias"] = torch.zeros(cfg.vocab_size)
    sd["cls.predictions.transform.dense.weight"] = mat(H, H)
    sd["cls.predictions.transform.dense.bias"] = vec(H, 0.02)
    sd["cls.predictions.transform.LayerNorm.weight"] = vec(H, 0.05, 1.0)
    sd["cls.predictions.transform.LayerNorm.bias"] = vec(H, 0.02)
    sd["cls.predictions.text_decoder.weight"] = mat(cfg.vocab_size, H)
    sd["cls.predictions.entity_decoder.weight"] = mat(cfg.kg_vocab_size, H)
    sd["cls.predictions.text_bias"] = torch.zeros(cfg.vocab_size)
    sd["cls.predictions.entity_bias"] = torch.zeros(cfg.kg_vocab_size)
    sd["cls.seq_relationship.weight"] = mat(2, H)
    sd["cls.seq_relationship.bias"] = vec(2, 0.02)
    bert("lm_backbone", cfg.n_backbone_layers)
    return sd


# --------------------------------------------------------------------------------------------- optimizer step
def linear_schedule_lr(base_lr: float, step: int, max_steps: int, warmup: int = 0) -> float:
    """hf get_linear_schedule_with_warmup as configured by the reference (0 warm-up): lr used BY optimizer step
    number `step` (0-based) = base * max(0, (max_steps - step) / max_steps)."""
    if step < warmup:
        return base_lr * step / max(1, warmup)
    return base_lr * max(0.0, (max_steps - step) / max(1, max_steps - warmup))


@dataclass
class AdamState:
    step: int = 0
    m: Dict[str, Tensor] = field(default_factory=dict)
    v: Dict[str, Tensor] = field(default_factory=dict)


def train_step(sd: Dict[str, Tensor], cfg: OracleConfig, kg_table: Tensor, batch: Dict[str, Tensor], state: AdamState,
               base_lr: float = 1e-4, max_steps: int = 200, max_grad_norm: float = 1.0, betas=(0.9, 0.999),
               eps: float = 1e-8, weight_decay: float = 0.0, return_outputs: bool = False,
               dropout=None) -> Dict[str, Tensor]:
    """One Trainer optimizer step (forward, backward, clip, AdamW, schedule); updates `sd` in place.
    Returns loss terms, the pre-clip global grad norm and the gradients (for parity checks). `dropout`: see `_drop`."""
    names = trainable_names(sd)
    params = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    work = dict(sd)
    work.update(params)
    out = forward(work, cfg, kg_table, **batch, dropout=dropout)
    grads = torch.autograd.grad(out["loss"], [params[k] for k in names], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(sd[k])) for k, g in zip(names, grads)}
    total_norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).float()
    coef = float(min(1.0, max_grad_norm / (float(total_norm) + 1e-6))) if max_grad_norm and max_grad_norm > 0 else 1.0
    lr = linear_schedule_lr(base_lr, state.step, max_steps)
    state.step += 1
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** state.step, 1 - b2 ** state.step
    with torch.no_grad():
        for k in names:
            g = grads[k] * coef
            m = state.m.setdefault(k, torch.zeros_like(sd[k]))
            v = state.v.setdefault(k, torch.zeros_like(sd[k]))
            p = sd[k]
            # hf:trainer.py get_decay_parameter_names: biases and LayerNorm parameters are not decayed
            if weight_decay and not (k.endswith(".bias") or "LayerNorm" in k):
                p.mul_(1 - lr * weight_decay)
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
            p.addcdiv_(m, denom, value=-lr / bc1)
    res = {k: out[k].detach() for k in ("loss", "masked_lm_loss", "ent_masked_lm_loss", "next_sentence_loss")}
    res.update(grad_norm=total_norm, lr=lr, grads=grads)
    if return_outputs:
        res["outputs"] = {k: v.detach() for k, v in out.items() if torch.is_tensor(v)}
    return res


# --------------------------------------------------------------------------------------------- masking (integer-exact)
def replace_mlm_tokens(tokens: Sequence[int], vocab_len: int, mask_id: int = 103, masked_tokens_percentage: float = 0.15,
                       unmasked_label_id: int = -100, rng=random) -> Tuple[List[int], List[int]]:
    """ref:src/stonkgs/data/indra_for_pretraining.py:33-77; consumes `rng` (Python's Mersenne Twister) in the same
    call order: one sample() of int(n*0.15) positions, then per position random() [<0.8 -> mask], else random()
    [<0.5 -> keep] else randint(0, vocab_len-1)."""
    inp = list(tokens)
    labels = [unmasked_label_id] * len(inp)
    positions = rng.sample(range(len(inp)), int(len(inp) * masked_tokens_percentage))
    for pos in positions:
        if rng.random() < 0.8:
            tok = mask_id
        elif rng.random() < 0.5:
            tok = tokens[pos]
        else:
            tok = rng.randint(0, vocab_len - 1)
        inp[pos] = tok
        labels[pos] = tokens[pos]
    return inp, labels


def negative_nsp_index_pairs(n_rows: int, proportion: float = 0.25, rng=random) -> List[Tuple[int, int]]:
    """ref:indra_for_pretraining.py:80-126: (text row i, entity row j) pairs of the appended negatives."""
    k = int(n_rows * proportion)
    a = rng.sample(range(n_rows), k)
    b = rng.sample(range(n_rows), k)
    return list(zip(a, b))
