"""MI355X-native ``STonKGsForPreTraining``: the reference's module contract on top of the HIP engine.

Mirror of ref:src/stonkgs/models/stonkgs_model.py (same class names, constructor arguments, ``forward`` signature,
return packing, attributes other code touches, state-dict keys), so that ``stonkgs.models.stonkgs_pretraining``'s
``Trainer(model=..., ...)`` loop, ``from_pretrained`` and the bs=1 inference helpers work unchanged - but no
arithmetic runs in torch: ``forward`` hands raw device pointers to ``libstonk_hip.so`` (see ``engine.py``).

Differences a user of the reference will notice (all forced by the offline, GPU-only setting):
  * ``nlp_model_type`` / ``from_pretrained`` take LOCAL directories, never hub names;
  * the model is built directly on the GPU (``.to(device)`` to the same device is a no-op);
  * in training mode the dense logits ([B,256,V] and [B,256,K] = 13 GB at B=64) are not materialised unless
    asked for (``model.materialize_logits = True``): loss and gradients are identical.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from . import _hip as hip
from .config import STonKGsConfig
from .engine import Engine
from .flat_model import (FlatBufferModel, SequenceClassifierFront, SequenceClassifierOutput,  # noqa: F401
                         _load_weights_file, _StepFunction)
from .params import (FlatStore, _Node, _linear, _param, backbone_specs, build_bert_tree, pretraining_head_specs,
                     trainable_specs)

SEP_ID, MASK_ID, UNK_ID = 102, 103, 100  # BioBERT vocabulary (ref:stonkgs_model.py:116-118)
# state-dict keys a checkpoint may lack (see from_pretrained)
_DROPPED_ALIASES = ("position_ids", "cls.predictions.decoder.", "cls.predictions.bias", "cls.predictions.text_bias",
                    "cls.predictions.entity_bias", "bert.embeddings.word_embeddings.weight")
_FRESH_HEAD_PREFIXES = ("classifier.",)
_TERM_KEYS = ("masked_lm_loss", "ent_masked_lm_loss", "next_sentence_loss")


@dataclass
class BertForPreTrainingOutputWithPooling:
    """ref:stonkgs_model.py:30-34 (HF BertForPreTrainingOutput + pooler_output). Indexable like a ModelOutput."""

    loss: Optional[torch.Tensor] = None
    prediction_logits: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
    seq_relationship_logits: Optional[torch.Tensor] = None
    hidden_states: Optional[torch.Tensor] = None
    attentions: Optional[tuple] = None
    pooler_output: Optional[torch.Tensor] = None

    def to_tuple(self):
        return tuple(v for v in (self.loss, self.prediction_logits, self.seq_relationship_logits, self.hidden_states,
                                 self.attentions, self.pooler_output) if v is not None)

    def __getitem__(self, k):
        return getattr(self, k) if isinstance(k, str) else self.to_tuple()[k]


def prepare_df(embedding_path: str, sep: str = "\t") -> Dict[object, "object"]:
    """ref:src/stonkgs/models/kg_baseline_model.py:270-280: TSV (first column = node name, no header) ->
    {name: float64 vector}, in file order. Read with pandas like the reference, so that the parsed values (its C
    float parser) and the key types (an all-numeric name column becomes an integer index) are the reference's:
    pinned by tests/golden/g8_table.* made with the reference's own function."""
    import pandas as pd

    df = pd.read_csv(embedding_path, sep=sep, header=None, index_col=0)
    return dict(zip(df.index.tolist(), df.to_numpy()))   # (= {index: row.values for index, row in df.iterrows()})


class KGBackbone:
    """Dict-like view of the dense entity table: ``kg_backbone[i]`` is row i (a device tensor), KeyError outside
    the table - what ref:stonkgs_model.py:131-141 builds as a Python dict of 175 097 tensors."""

    def __init__(self, table: torch.Tensor):
        self.table = table

    def __getitem__(self, i: int) -> torch.Tensor:
        if not 0 <= int(i) < self.table.shape[0]:
            raise KeyError(i)
        return self.table[int(i)]

    def __len__(self):
        return self.table.shape[0]

    def __contains__(self, i):
        return 0 <= int(i) < self.table.shape[0]

    def keys(self):
        return range(self.table.shape[0])


class STonKGsELMPredictionHead(_Node):
    """Naming mirror of ref:stonkgs_model.py:37-73 (transform, split text/entity decoders, dead biases)."""

    def __init__(self, config: STonKGsConfig, store: FlatStore, device, trainable: bool = True):
        super().__init__()
        H = config.hidden_size
        tr = _Node()
        tr.dense = _linear(store, "cls.predictions.transform.dense", trainable)
        tr.LayerNorm = _linear(store, "cls.predictions.transform.LayerNorm", trainable)
        self.transform = tr
        self.text_decoder = _linear(store, "cls.predictions.text_decoder", trainable, bias=False)
        self.entity_decoder = _linear(store, "cls.predictions.entity_decoder", trainable, bias=False)
        self.half_length = config.max_position_embeddings // 2
        # dead parameters (quirk Q4): declared, serialised, never used by forward, never updated
        self.bias = nn.Parameter(torch.zeros(config.vocab_size, device=device), requires_grad=False)
        self.text_bias = nn.Parameter(torch.zeros(config.vocab_size, device=device), requires_grad=False)
        self.entity_bias = nn.Parameter(torch.zeros(config.kg_vocab_size, device=device), requires_grad=False)
        dec = _Node()
        dec.bias = self.bias
        dec.text_bias = self.text_bias
        dec.entity_bias = self.entity_bias
        self.decoder = dec


class STonKGsForPreTraining(FlatBufferModel):
    _TRAIN_PRETRAINING_HEADS = True

    def __init__(self, config=None, nlp_model_type: Optional[str] = None, kg_embedding_dict_path: Optional[str] = None,
                 *, kg_embeddings: Optional[torch.Tensor] = None, kg_names=None, device=None, seed: int = 0,
                 backbone_layers: Optional[int] = None):
        """:param config: STonKGsConfig / dict / BertConfig-like (the reference ignores its ``config`` and reads the hub;
            here it is honoured unless ``nlp_model_type`` is a local directory holding config.json)
        :param nlp_model_type: LOCAL directory of the LM backbone (config.json + pytorch_model.bin|model.safetensors)
        :param kg_embedding_dict_path: TSV of node2vec embeddings (prepare_df format)
        :param kg_embeddings: alternative to the TSV: [K, H] tensor in TSV row order (synthetic tables)"""
        super().__init__(device)
        if nlp_model_type is not None and os.path.isdir(nlp_model_type):
            cfg = STonKGsConfig.from_pretrained(nlp_model_type)
            if config is not None:  # keep run-time knobs (dropout) of an explicit config
                c2 = STonKGsConfig.from_any(config)
                cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = c2.hidden_dropout_prob, c2.attention_probs_dropout_prob
        elif config is not None:
            cfg = STonKGsConfig.from_any(config)
        else:
            raise ValueError("pass a local config, or nlp_model_type = local directory with config.json "
                             "(hub names cannot be fetched offline)")
        names = None
        if kg_embedding_dict_path is not None:
            d = prepare_df(kg_embedding_dict_path)  # ref:stonkgs_model.py:93
            names = list(d.keys())
            import numpy as np

            kg_embeddings = torch.from_numpy(np.stack(list(d.values())))
        if kg_embeddings is not None:
            cfg.update({"kg_vocab_size": int(kg_embeddings.shape[0])})  # ref:stonkgs_model.py:97
            if kg_embeddings.shape[1] != cfg.hidden_size:
                raise ValueError("KG embedding width must equal hidden_size")
        self.config = cfg
        cfg.validate_for_hip()
        dev = self._device
        n_bb = cfg.num_hidden_layers if backbone_layers is None else backbone_layers
        self._store = FlatStore(self._head_specs(cfg) + trainable_specs(cfg, self._TRAIN_PRETRAINING_HEADS), dev,
                                trainable=True)
        # the fine-tuning subclass inherits the MLM/ELM/NSP heads (they stay in its checkpoints) but never uses them:
        # there they live in a frozen side store - no gradient buffer, no optimizer state, no all-reduce bytes
        heads = self._store if self._TRAIN_PRETRAINING_HEADS else FlatStore(pretraining_head_specs(cfg), dev, False)
        self._heads_store = heads
        self._bb_store = FlatStore(backbone_specs(cfg, n_bb), dev, trainable=False)
        # ---- module tree (names only)
        dead_we = nn.Parameter(torch.zeros(cfg.vocab_size, cfg.hidden_size, device=dev), requires_grad=False)
        self.bert = build_bert_tree(self._store, "bert", cfg, cfg.num_hidden_layers, True, dead_we)
        cls = _Node()
        cls.predictions = STonKGsELMPredictionHead(cfg, heads, dev, self._TRAIN_PRETRAINING_HEADS)
        cls.predictions.decoder.weight = dead_we  # tied: cls.predictions.decoder.weight <-> word_embeddings (both dead)
        cls.seq_relationship = _linear(heads, "cls.seq_relationship", self._TRAIN_PRETRAINING_HEADS)
        self.cls = cls
        self.lm_backbone = build_bert_tree(self._bb_store, "lm_backbone", cfg, n_bb, False, None)
        self.lm_sep_id, self.lm_mask_id, self.lm_unk_id = SEP_ID, MASK_ID, UNK_ID
        self.engine = Engine(cfg, self._store, self._bb_store, n_bb, dev)
        self.materialize_logits: Optional[bool] = None  # None = "only when not training"
        # ---- init weights, KG table
        self._init_weights(seed)
        if nlp_model_type is not None and os.path.isdir(nlp_model_type):
            sd = _load_weights_file(nlp_model_type)
            if sd is not None:
                sd = {("lm_backbone." + k[len("bert."):] if k.startswith("bert.") else "lm_backbone." + k): v
                      for k, v in sd.items() if not k.startswith("cls.")}
                self.load_state_dict(sd, strict=False, _refresh=False)
        K = cfg.kg_vocab_size
        if kg_embeddings is None:
            g = torch.Generator().manual_seed(seed + 1)
            kg_embeddings = torch.randn(K, cfg.hidden_size, generator=g, dtype=torch.float64) * 0.3
        self._kg_rows = kg_embeddings.to(torch.float32).to(dev)  # fp64 -> fp32 RN, as ref:stonkgs_model.py:193-200
        # (a table of fewer than 101 rows ends below the special ids: the reference's zip stops after K indices)
        numeric_indices = [i for i in range(K + 3) if i not in (SEP_ID, MASK_ID, UNK_ID)][:K]
        names = names if names is not None else [f"node{r}" for r in range(K)] if K <= 4096 else None
        self.kg_idx_to_name = dict(zip(numeric_indices, names)) if names is not None else _LazyNames(numeric_indices)
        self._numeric_indices = torch.tensor(numeric_indices, device=dev)
        self._bind_grad_views()
        self.refresh()

    # -------------------------------------------------------------- construction helpers
    @staticmethod
    def _head_specs(cfg):
        """Extra trainable tensors a subclass puts in FRONT of the flat buffer (their gradients are final first)."""
        return []

    def refresh(self) -> None:
        """Recompute everything derived from the fp32 masters: bf16 mirrors, W^T copies, the entity table with its
        three LM special-token rows (quirks Q1/Q2). Called after init / load_state_dict."""
        eng = self.engine
        eng.refresh_derived(bf16_mirror=True)
        K, H = self.config.kg_vocab_size, self.config.hidden_size
        table = torch.zeros(max(K + 3, MASK_ID + 1), H, dtype=torch.float32, device=self._device)
        table[self._numeric_indices] = self._kg_rows  # TSV row r -> model index numeric_indices[r]  (Q1)
        eng.kg_table = table
        sv = eng.special_vectors()  # (Q2)
        for sid, vec in sv.items():
            if sid < table.shape[0]:
                table[sid] = vec
        self.kg_backbone = KGBackbone(table)
        self._mark_synced()

    def _stores(self) -> tuple:
        return self._store, self._bb_store, self._heads_store

    def _rederive(self, written: list) -> None:
        if any(s is self._bb_store for s in written):
            self.refresh()              # backbone changed: special vectors of the entity table too (quirk Q2)
        else:
            super()._rederive(written)

    def _backward(self, gscale: float, on_segment_done) -> None:
        self.engine.backward(gscale, on_segment_done)

    # -------------------------------------------------------------- loaders
    @classmethod
    def from_pretrained(cls, path: str, **kwargs) -> "STonKGsForPreTraining":
        """Local directory in HF layout (config.json + weights). ``kwargs`` go to the constructor, as in HF."""
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path!r}: only local checkpoints can be loaded (no network)")
        cfg = STonKGsConfig.from_pretrained(path)
        model = cls(cfg, **kwargs)
        sd = _load_weights_file(path)
        if sd is None:
            raise FileNotFoundError(f"no pytorch_model.bin / model.safetensors under {path!r}")
        missing, unexpected = model.load_state_dict(sd, strict=False)
        # what HF's from_pretrained tolerates for this architecture: buffers that are not parameters here, the tied / dead
        # aliases a safetensors checkpoint drops (quirk Q4: word_embeddings <-> cls.predictions.decoder.weight,
        # cls.predictions.bias <-> decoder.bias, text_bias / entity_bias <-> decoder.*), and the heads the checkpoint's
        # architecture does not have - `STonKGsForSequenceClassification.from_pretrained(pretraining_dir, num_labels=n)`
        # (ref:stonkgs_finetuning.py:404-407) keeps the freshly initialised classifier, as HF does, and says so
        fresh = [k for k in missing if k.startswith(_FRESH_HEAD_PREFIXES)]
        bad = [k for k in missing if k not in fresh and not any(t in k for t in _DROPPED_ALIASES)]
        if bad:
            raise KeyError(f"checkpoint misses {bad[:5]}...")
        if fresh:
            import warnings

            warnings.warn(f"Some weights of {cls.__name__} were not initialized from the checkpoint at {path} and are "
                          f"newly initialized: {fresh}. You should probably TRAIN this model on a down-stream task.")
        return model

    @classmethod
    @lru_cache(maxsize=32)
    def from_default_pretrained(cls, **kwargs) -> "STonKGsForPreTraining":
        """ref:stonkgs_model.py:143-147 fetches 'stonkgs/stonkgs-150k' from the hub; offline, the checkpoint must be
        provided locally through $STONKGS_PRETRAINED_DIR."""
        path = os.environ.get("STONKGS_PRETRAINED_DIR")
        if not path:
            raise FileNotFoundError("set STONKGS_PRETRAINED_DIR to a local copy of stonkgs/stonkgs-150k")
        return cls.from_pretrained(path, **kwargs)

    # -------------------------------------------------------------- forward
    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, masked_lm_labels=None,
                ent_masked_lm_labels=None, next_sentence_labels=None, return_dict=None, head_mask=None):
        """ref:stonkgs_model.py:149-258. ``head_mask`` is accepted and ignored (quirk Q8)."""
        cfg = self.config
        if input_ids is None:
            raise ValueError("input_ids is required")
        if getattr(cfg, "output_attentions", False):   # (set after construction: the constructor refuses it already)
            cfg.validate_for_hip()
        input_ids, attention_mask, token_type_ids = (self._long(t) for t in (input_ids, attention_mask, token_type_ids))
        mlm, elm, nsp = (self._long(t) for t in (masked_lm_labels, ent_masked_lm_labels, next_sentence_labels))
        if input_ids.dim() != 2 or input_ids.shape[1] != cfg.max_position_embeddings:
            raise ValueError(f"input_ids must be [B, {cfg.max_position_embeddings}] (text half | entity half)")
        have_labels = mlm is not None and elm is not None and nsp is not None
        training = self.training
        self._sync_derived()
        need_bwd = have_labels and torch.is_grad_enabled() and training
        dense = self.materialize_logits if self.materialize_logits is not None else not training
        # (hidden states leave only in the dataclass: a tuple-returning training forward may run the encoder unpadded)
        out = self.engine.forward(input_ids, attention_mask, token_type_ids, mlm if have_labels else None,
                                  elm if have_labels else None, nsp if have_labels else None, training, dense, need_bwd,
                                  want_hidden=bool(return_dict) or not need_bwd)
        total_loss = None
        if have_labels:
            total_loss = out["loss"]
            self.last_loss_terms = tuple(out[k].clone() for k in _TERM_KEYS)
            total_loss = _StepFunction.apply(self._anchor, self, total_loss) if need_bwd else total_loss.clone()
        prediction_scores = (out.get("text_logits"), out.get("ent_logits"))
        nsp_logits = out["nsp_logits"].clone()
        if not return_dict:
            output = (prediction_scores, nsp_logits)
            return ((total_loss,) + output) if total_loss is not None else output
        return BertForPreTrainingOutputWithPooling(
            loss=total_loss, prediction_logits=prediction_scores, seq_relationship_logits=nsp_logits,
            hidden_states=out["hidden_states"].float(), attentions=None, pooler_output=out["pooler_output"].clone())


    # -------------------------------------------------------------- forward-only encoder (embedding extraction)
    @torch.no_grad()
    def encode(self, input_ids, attention_mask=None, token_type_ids=None, pooled_only: bool = False):
        """(sequence_output bf16 [B, S, H], pooler_output fp32 [B, H]) without the pre-training heads: what
        ``model(**row, return_dict=True).pooler_output`` costs in ref:stonkgs_for_embeddings.py:179 minus the two
        vocabulary-wide decoders, whose logits that caller throws away. Dropout is off (the reference's
        ``from_pretrained`` models are in eval mode); any batch size. ``pooled_only``: the caller reads the pooled vector
        only (embedding extraction does): the encoder runs on the rows that are live keys or position 0, its last layer on
        position 0 alone behind the QKV projection (Engine.unpad), and the first element returned is None."""
        cfg = self.config
        input_ids, attention_mask, token_type_ids = (self._long(t) for t in (input_ids, attention_mask, token_type_ids))
        if input_ids.dim() != 2 or input_ids.shape[1] != cfg.max_position_embeddings:
            raise ValueError(f"input_ids must be [B, {cfg.max_position_embeddings}] (text half | entity half)")
        self._sync_derived()
        seq_out, pooled, _ = self.engine.encode(input_ids, attention_mask, token_type_ids, False, None,
                                                (None, None) if pooled_only else None)
        self.engine.check_errors()
        B = input_ids.shape[0]
        if pooled_only:
            return None, pooled.clone()
        return seq_out.view(B, cfg.max_position_embeddings, cfg.hidden_size).clone(), pooled.clone()

    # -------------------------------------------------------------- attention maps (on request only)
    @torch.no_grad()
    def attention_maps(self, input_ids, attention_mask=None, token_type_ids=None, layers=None, output: str = "probs",
                       max_bytes: int = 4 << 30) -> dict:
        """The encoder's attention probabilities, what the reference hands through as ``outputs.attentions``
        (ref:stonkgs_model.py:256) - here an explicit forward-only call, because the training and inference kernels never
        hold the S x S scores. Dropout is OFF (p = 0) in either module mode, which is left as it was: the reference's
        training-mode ``attentions`` are post-dropout, these are not.

        ``layers``: None = all, or layer indices (negative ones count from the end; no duplicates). ``output``:
        "probs", "modal_mass" or "both". Returns a dict: ``layers`` (the resolved indices, ascending), ``attentions`` (a
        tuple of fp32 [B, heads, S, S], one per selected layer, HuggingFace layout; absent for "modal_mass"),
        ``modal_mass`` (fp32 [len(layers), B, heads, S, 2]: per query row the probability mass on the text half and on the
        entity half of the keys - see ``stonkgs_for_embeddings.summarize_modal_mass``; absent for "probs") and
        ``pooler_output`` (fp32 [B, H], as ``encode`` returns it). A masked key has probability exactly 0; padded
        positions still have a row as queries. The result tensors are allocated up front: more than ``max_bytes`` of them
        is refused before anything runs."""
        cfg = self.config
        S, NH, L = cfg.max_position_embeddings, cfg.num_attention_heads, cfg.num_hidden_layers
        if output not in ("probs", "modal_mass", "both"):
            raise ValueError(f'output must be "probs", "modal_mass" or "both" (got {output!r})')
        wanted = list(range(L)) if layers is None else [int(i) for i in layers]
        resolved = []
        for i in wanted:
            if not -L <= i < L:
                raise ValueError(f"layer index {i} is out of range for {L} layers")
            resolved.append(i % L)
        if len(set(resolved)) != len(resolved):
            raise ValueError(f"duplicate layer in {wanted}")
        if not resolved:
            raise ValueError("no layer selected")
        resolved = tuple(sorted(resolved))
        input_ids, attention_mask, token_type_ids = (self._long(t) for t in (input_ids, attention_mask, token_type_ids))
        if input_ids.dim() != 2 or input_ids.shape[1] != S:
            raise ValueError(f"input_ids must be [B, {S}] (text half | entity half)")
        B = input_ids.shape[0]
        want_p, want_m = output != "modal_mass", output != "probs"
        need = len(resolved) * B * NH * S * 4 * ((S if want_p else 0) + (2 if want_m else 0))
        if need > max_bytes:
            raise ValueError(
                f"attention_maps would allocate {need} bytes ({need / 2 ** 30:.2f} GiB) for {len(resolved)} layer(s) of "
                f"[{B}, {NH}, {S}, {S}] fp32, more than max_bytes = {max_bytes}: select fewer layers (layers=...), ask for "
                'output="modal_mass", or pass a smaller batch')
        dev = self._device
        probs = tuple(torch.empty(B, NH, S, S, device=dev, dtype=torch.float32) for _ in resolved) if want_p else None
        modal = torch.empty(len(resolved), B, NH, S, 2, device=dev, dtype=torch.float32) if want_m else None
        self._sync_derived()
        sel = {l: (probs[j] if want_p else None, modal[j] if want_m else None) for j, l in enumerate(resolved)}
        pooled = self.engine.attention_maps(input_ids, attention_mask, token_type_ids, sel)
        self.engine.check_errors()
        res = dict(layers=resolved, pooler_output=pooled.clone())
        if want_p:
            res["attentions"] = probs
        if want_m:
            res["modal_mass"] = modal
        return res

    # -------------------------------------------------------------- input attributions (on request only)
    def _attribution_buffers(self, input_ids, return_gradient: bool, max_bytes: int):
        """Shape check and the result tensors of `input_attributions`, allocated up front."""
        cfg = self.config
        S, H = cfg.max_position_embeddings, cfg.hidden_size
        if input_ids.dim() != 2 or input_ids.shape[1] != S:
            raise ValueError(f"input_ids must be [B, {S}] (text half | entity half)")
        B = input_ids.shape[0]
        need = B * S * H * 4 if return_gradient else 0
        if need > max_bytes:
            raise ValueError(f"return_gradient would allocate {need} bytes ({need / 2 ** 30:.2f} GiB) for [{B}, {S}, {H}] "
                             f"fp32, more than max_bytes = {max_bytes}: pass a smaller batch or raise max_bytes")
        dev = self._device
        gxi = torch.empty(B, S, device=dev, dtype=torch.float32)
        gn = torch.empty(B, S, device=dev, dtype=torch.float32)
        grad = torch.empty(B, S, H, device=dev, dtype=torch.float32) if return_gradient else None
        return gxi, gn, grad

    @torch.no_grad()
    def input_attributions(self, input_ids, attention_mask=None, token_type_ids=None, labels=None,
                           return_gradient: bool = False, max_bytes: int = 1 << 30) -> dict:
        """Which evidence tokens and which walk entities drive a masked prediction: the gradient of
        F = sum of log p(label) with respect to the input embeddings (the `inputs_embeds` of ref:stonkgs_model.py:193-210:
        the frozen backbone's output for the text half, the entity table's rows for the other), per position.

        ``labels``: a dict with any non-empty subset of ``masked_lm_labels`` [B, S/2], ``ent_masked_lm_labels`` [B, S/2],
        ``next_sentence_labels`` [B]; F sums over the labels that are not -100. Sequences are independent: row b of the
        result is the gradient of sequence b's own terms. Returns ``score`` (fp32 scalar tensor: F), ``grad_x_input``
        (fp32 [B, S]: <dF/dx_p, x_p>), ``grad_norm`` (fp32 [B, S]: |dF/dx_p|, saliency) and, with ``return_gradient``,
        ``gradient`` (fp32 [B, S, H]; allocated up front, refused beyond ``max_bytes``). A padded position that carries no
        label and is not position 0 is read by nothing: its entries are exactly 0.

        Dropout is off in either module mode, which is left as it was; no parameter gradient is computed and a training
        run around the call does not notice it (Engine.input_gradients) - but it may not run between a training-mode
        forward and its backward (RuntimeError). See ``stonkgs_for_embeddings.summarize_attributions``."""
        names = ("masked_lm_labels", "ent_masked_lm_labels", "next_sentence_labels")
        if labels is not None and set(labels) - set(names):
            raise ValueError(f"labels: unknown key(s) {sorted(set(labels) - set(names))}; expected a subset of {names}")
        lab = {k: self._long(v) for k, v in (labels or {}).items() if v is not None}
        if not lab:
            raise ValueError(f"labels: give a dict with at least one of {names}")
        input_ids, attention_mask, token_type_ids = (self._long(t) for t in (input_ids, attention_mask, token_type_ids))
        gxi, gn, grad = self._attribution_buffers(input_ids, return_gradient, max_bytes)
        B, half = input_ids.shape[0], self.config.half_length
        for k, v in lab.items():
            if (v.numel() != B) if k == "next_sentence_labels" else (tuple(v.shape) != (B, half)):
                raise ValueError(f"labels[{k!r}] must have shape {(B,) if k == 'next_sentence_labels' else (B, half)}")
        self._sync_derived()
        out = self.engine.input_gradients(input_ids, attention_mask, token_type_ids, gxi, gn, grad, labels=lab)
        self.engine.check_errors()
        res = dict(score=out["score"].clone(), grad_x_input=gxi, grad_norm=gn)
        if return_gradient:
            res["gradient"] = grad
        return res

    # -------------------------------------------------------------- evaluation / masked prediction (no dense logits)
    def _evaluate(self, input_ids, attention_mask, token_type_ids, mlm, elm, nsp, k: int):
        """Engine.evaluate + the trim to the true label counts: one device-to-host copy (the two counts and the
        engine's error word) on top of the packed encoder's own wait for its row count."""
        cfg = self.config
        S, half = cfg.max_position_embeddings, cfg.half_length
        if input_ids.dim() != 2 or input_ids.shape[1] != S:
            raise ValueError(f"input_ids must be [B, {S}] (text half | entity half)")
        if not 1 <= int(k) <= 16 or k > min(cfg.vocab_size, cfg.kg_vocab_size):
            raise ValueError("k must be in [1, 16] and at most the smaller vocabulary")
        self._sync_derived()
        eng = self.engine
        out = eng.evaluate(input_ids, attention_mask, token_type_ids, mlm, elm, nsp, int(k))
        n_text, n_ent, err = torch.cat([out["text"]["count"], out["ent"]["count"], eng.err]).tolist()
        if err:
            eng.check_errors()
        res = {key: out[key].clone() for key in ("loss",) + _TERM_KEYS + ("nsp_logits",)}
        for nm, n, off in (("text", n_text, 0), ("ent", n_ent, half)):
            h = out[nm]
            rows = h["rows"][:n].long()
            lse = h["lse"][:n]
            res[nm] = dict(batch_index=rows // S, position=rows % S - off, label=h["targets"][:n].long(),
                           rank=h["rank"][:n].long(), topk_ids=h["top_idx"][:n].long(),
                           topk_logprobs=h["top_val"][:n] - lse[:, None], nll=lse - h["tgt_logit"][:n])
        return res

    @torch.no_grad()
    def evaluate_batch(self, inputs: Dict[str, torch.Tensor], k: int = 10) -> Dict[str, object]:
        """Held-out evaluation of one labelled batch (the six schema columns) WITHOUT dense logits: the decoders run on
        the labelled rows only, as in training, and a top-k kernel reads the logits the loss reads. Works in either
        module mode; always without dropout and without gradients; leaves no trace in a training run around it.

        Returns `loss`, `masked_lm_loss`, `ent_masked_lm_loss`, `next_sentence_loss` (means over their own labels, as
        the training loss), `nsp_logits` [B, 2], and under "text" and "ent" one dict per head, rows in row-major order of
        `labels != -100`, trimmed to the true label count n: `batch_index`, `position` (within the half), `label`, `rank`
        (zero-based: classes with a larger logit, plus classes with an equal logit and a lower id), `topk_ids` [n, k],
        `topk_logprobs` [n, k] (logit - logsumexp; non-increasing, ties by lower id) and `nll` [n] (logsumexp - the
        label's logit). Class ids are in the label space the decoders are trained against - for entities the
        PREPROCESSING ids 0..K-1 (quirk Q1), not rows of the entity table (`entity_names` maps them)."""
        t = {key: self._long(v) for key, v in inputs.items()}
        return self._evaluate(t["input_ids"], t.get("attention_mask"), t.get("token_type_ids"), t["masked_lm_labels"],
                              t["ent_masked_lm_labels"], t["next_sentence_labels"], k)

    @torch.no_grad()
    def predict_masked(self, input_ids, attention_mask=None, token_type_ids=None, positions=None, k: int = 10):
        """"Fill this mask": the k most probable classes at the wanted positions. `positions`: bool [B, S], or None =
        wherever `input_ids == self.lm_mask_id`, in either half. Returns {"text": (batch_index, position, topk_ids,
        topk_logprobs), "ent": (...)} - `position` within the half, ids in the decoders' label space (see
        `evaluate_batch`, whose path this is: labels of 0 at the wanted positions, loss and rank dropped)."""
        input_ids = self._long(input_ids)
        half = self.config.half_length
        want = input_ids == self.lm_mask_id if positions is None else torch.as_tensor(positions).to(self._device) != 0
        if want.shape != input_ids.shape:
            raise ValueError("positions must be a bool [B, S] like input_ids")
        lab = torch.where(want, 0, -100)
        nsp = torch.zeros(input_ids.shape[0], dtype=torch.long, device=self._device)
        res = self._evaluate(input_ids, self._long(attention_mask), self._long(token_type_ids),
                             lab[:, :half].contiguous(), lab[:, half:].contiguous(), nsp, k)
        return {nm: tuple(res[nm][key] for key in ("batch_index", "position", "topk_ids", "topk_logprobs"))
                for nm in ("text", "ent")}

    def entity_names(self, ids) -> list:
        """Names of entity class ids (label space, quirk Q1): id e is the node the model embeds for input id e -
        `kg_idx_to_name[e]` - and 100 / 102 / 103 are the LM's [UNK] / [SEP] / [MASK] rows. Nested lists in, nested out."""
        special = {self.lm_unk_id: "[UNK]", self.lm_sep_id: "[SEP]", self.lm_mask_id: "[MASK]"}
        ids = ids.tolist() if torch.is_tensor(ids) else ids
        if isinstance(ids, (list, tuple)):
            return [self.entity_names(i) for i in ids]
        return special[ids] if ids in special else self.kg_idx_to_name[ids]

    # -------------------------------------------------------------- fused training path (no autograd)
    def forward_backward(self, inputs: Dict[str, torch.Tensor], gscale: float = 1.0, on_segment_done=None):
        """forward + hand-written backward in one call: what ``Trainer.training_step`` does through
        ``loss = model(**inputs)[0]; loss.backward()`` (hf:trainer.py:1892-1963), minus the autograd graph and the
        host sync on ``dloss``. Gradients are accumulated into the flat buffer; returns the (detached) loss."""
        t = {k: self._long(v) for k, v in inputs.items()}
        self._sync_derived()
        out = self.engine.forward(t["input_ids"], t.get("attention_mask"), t.get("token_type_ids"),
                                  t["masked_lm_labels"], t["ent_masked_lm_labels"], t["next_sentence_labels"],
                                  self.training, False, True, want_hidden=False)
        terms = out["loss_terms"].clone()          # [total, text MLM, entity MLM, NSP]: one copy out of the workspace
        loss, self.last_loss_terms = terms[0], (terms[1], terms[2], terms[3])
        self.engine.backward(gscale, on_segment_done)
        return loss


class STonKGsForSequenceClassification(SequenceClassifierFront, STonKGsForPreTraining):
    """Fine-tuning model of BASELINE config 5 (relation-type etc. classification): mirror of
    ref:src/stonkgs/models/stonkgs_finetuning.py:237-346. Same frozen LM backbone + KG table front, same encoder,
    pooled [CLS] -> dropout -> Linear(hidden, num_labels) -> CrossEntropyLoss. Like the reference it inherits from the
    pre-training class (its MLM/ELM heads stay in the state dict, unused). The three loss branches of the reference
    (:328-338) run on the HIP path: CrossEntropyLoss, MSELoss (regression) and BCEWithLogitsLoss (multi-label)."""

    _TRAIN_PRETRAINING_HEADS = False

    def __init__(self, config, **kwargs):
        cfg = STonKGsConfig.from_any(config) if config is not None else None
        if "num_labels" in kwargs:  # from_pretrained(model_path, num_labels=n) as the reference calls it (:404-407)
            n = kwargs.pop("num_labels")
            if cfg is not None:
                cfg.num_labels = n
        super().__init__(cfg, **kwargs)
        self.num_labels = self.config.num_labels
        self.dropout = nn.Dropout(self.config.hidden_dropout_prob)  # naming only; the engine applies it
        self.classifier = _linear(self._store, "classifier", True)
        self._bind_grad_views()

    @staticmethod
    def _head_specs(cfg):
        return [("classifier.weight", (cfg.num_labels, cfg.hidden_size), None), ("classifier.bias", (cfg.num_labels,), None)]

    def _labels_and_mode(self, labels):
        """ref:stonkgs_finetuning.py:316-338: infer `problem_type` once from num_labels and the label dtype, as the
        reference does, and bring the labels to what the loss kernels read. Returns (labels on the device, loss mode):
        None = CrossEntropyLoss on int64 [B]; hip.LOSS_MSE / LOSS_MSE_BROADCAST (regression: MSELoss on
        logits.view(-1, num_labels) - with num_labels = 1 and 1-D labels torch broadcasts [B,1] x [B] to [B,B], and the
        reference inherits that) / hip.LOSS_BCE (multi-label: BCEWithLogitsLoss) on fp32 labels."""
        if labels is None:
            return None, None
        lt = torch.as_tensor(labels)
        pt = self.config.problem_type
        if pt is None:
            if self.num_labels == 1:
                pt = "regression"
            elif self.num_labels > 1 and lt.dtype in (torch.long, torch.int):
                pt = "single_label_classification"
            else:
                pt = "multi_label_classification"
            self.config.problem_type = pt
        if pt == "single_label_classification":
            return self._long(lt.reshape(-1)), None
        if pt not in ("regression", "multi_label_classification"):
            raise ValueError(f"unknown problem_type {pt!r}")
        f = lt.to(device=self._device, dtype=torch.float32).contiguous()
        n, C = f.numel(), self.num_labels
        if pt == "regression" and C == 1 and f.dim() == 1 and n > 1:
            return f, hip.LOSS_MSE_BROADCAST
        B = n // max(C, 1)
        if n != B * C or (f.dim() > 1 and f.shape[-1] != C):
            raise ValueError(f"labels of shape {tuple(f.shape)} do not match logits [B, {C}]")
        return f.view(B, C), hip.LOSS_MSE if pt == "regression" else hip.LOSS_BCE

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, head_mask=None,
                inputs_embeds=None, labels=None, output_attentions=None, output_hidden_states=None, return_dict=None):
        return self._classify(*self._cls_inputs(input_ids, attention_mask, token_type_ids, labels), return_dict)

    def _cls_inputs(self, input_ids, attention_mask, token_type_ids, labels):
        if input_ids is None:
            raise ValueError("input_ids is required")
        lab, mode = self._labels_and_mode(labels)
        return self._long(input_ids), self._long(attention_mask), self._long(token_type_ids), lab, mode

    @torch.no_grad()
    def input_attributions(self, input_ids, attention_mask=None, token_type_ids=None, target=None,
                           return_gradient: bool = False, max_bytes: int = 1 << 30) -> dict:
        """Which evidence tokens and which walk entities drive this classification: the gradient of the logit of class
        ``target`` with respect to the input embeddings (the frozen backbone's output for the text half, the entity
        table's rows for the other), per position.

        ``target``: None = the predicted class of every sequence (argmax), an int (one class for all), or int64 [B]; a
        class outside [0, num_labels) raises IndexError. Returns ``logits`` (fp32 [B, num_labels], the eval-mode forward's),
        ``target`` (int64 [B]), ``grad_x_input`` (fp32 [B, S]: <dF/dx_p, x_p>), ``grad_norm`` (fp32 [B, S]: |dF/dx_p|,
        saliency) and, with ``return_gradient``, ``gradient`` (fp32 [B, S, H]; allocated up front, refused beyond
        ``max_bytes``). Padded positions other than position 0 are read by nothing: their entries are exactly 0.
        Dropout is off in either module mode; see the pre-training class's method for what the call leaves alone."""
        input_ids, attention_mask, token_type_ids = (self._long(t) for t in (input_ids, attention_mask, token_type_ids))
        gxi, gn, grad = self._attribution_buffers(input_ids, return_gradient, max_bytes)
        B, C = input_ids.shape[0], self.num_labels
        if target is not None:
            if torch.is_tensor(target) and target.dim() > 0:
                if target.dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool) or \
                        tuple(target.shape) != (B,):
                    raise ValueError(f"target must be None, an int, or an integer tensor of shape [{B}]")
                target = self._long(target)
                lo, hi = (int(v) for v in torch.stack([target.min(), target.max()]).tolist()) if B else (0, 0)
            else:
                lo = hi = int(target)
                target = torch.full((B,), lo, dtype=torch.long, device=self._device)
            if lo < 0 or hi >= C:
                raise IndexError(f"target class {lo if lo < 0 else hi} is out of range for {C} labels")
        self._sync_derived()
        out = self.engine.input_gradients(input_ids, attention_mask, token_type_ids, gxi, gn, grad, num_labels=C,
                                          target=target)
        self.engine.check_errors()
        res = dict(logits=out["logits"].clone(), target=out["target"].clone(), grad_x_input=gxi, grad_norm=gn)
        if return_gradient:
            res["gradient"] = grad
        return res


class _LazyNames:
    """kg_idx_to_name for synthetic tables too large to name eagerly."""

    def __init__(self, numeric_indices):
        self._idx = {i: r for r, i in enumerate(numeric_indices)}

    def __getitem__(self, i):
        return f"node{self._idx[i]}"

    def keys(self):
        return self._idx.keys()

    def __len__(self):
        return len(self._idx)
