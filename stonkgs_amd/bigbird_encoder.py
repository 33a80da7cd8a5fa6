"""BigBird encoder on the HIP path: the trainable stack of ProtSTonKGs (ref:src/stonkgs/models/protstonkgs_model.py:301,
``self.bert(inputs_embeds=..., attention_mask=...)``), HuggingFace's ``BigBirdModel`` with ``attention_type="block_sparse"``
run on given ``inputs_embeds``.

    BigBirdEncoderConfig   the fields of hf BigBirdConfig the encoder reads, and what the kernels are built for
    BigBirdEngine          layer_engine.LayerEngine with the block-sparse attention core (masked queries as HuggingFace has
                           them) and gelu_new behind the FFN-up GEMM in the place of its four layer methods, plus what this
                           encoder puts around the layers: BigBird's embeddings (dropout BEFORE the LayerNorm) and the
                           pooler. No attention-probability dropout; the GEMM / LayerNorm chain of a layer, the workspace,
                           the streams and the derived weights are the base class's
    BigBirdEncoderModel    FlatBufferModel that loads a BigBirdModel state dict (plain, or under ``bert.``), differentiable:
                           forward(inputs_embeds, attention_mask, token_type_ids) -> (sequence_output, pooler_output)

What differs from HuggingFace: sequence lengths it would pad (S % 64) or run with full attention (S <= (5 + 2 r) * 64) are
refused; ``.train()`` plans are drawn per layer from this package's generator (``set_rand_attn`` installs HuggingFace's, or a
checkpoint's); activations are bf16 between the kernels. Not here: the two frozen backbones, the projection, the PELM head and
the loss of ProtSTonKGs, gradient checkpointing, the packed row layout. No CPU fallback: the constructor raises without the
library or a GPU."""
from __future__ import annotations

import json
import math
import os
import warnings
from dataclasses import asdict, dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _hip as hip
from .bigbird_attention import BLOCK, BlockSparsePlan, bigbird_rand_attn
from .layer_engine import F32, LayerEngine, padded_rows
from .flat_model import FlatBufferModel, _load_weights_file
from .params import FlatStore, _linear, build_bert_tree, trainable_specs


@dataclass
class BigBirdEncoderConfig:
    """Defaults: HuggingFace's ``BigBirdConfig()``."""
    vocab_size: int = 50358
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    hidden_act: str = "gelu_new"
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    max_position_embeddings: int = 4096
    type_vocab_size: int = 2
    initializer_range: float = 0.02
    layer_norm_eps: float = 1e-12
    attention_type: str = "block_sparse"
    use_bias: bool = True
    rescale_embeddings: bool = False
    block_size: int = 64
    num_random_blocks: int = 3
    model_type: str = "big_bird"

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def min_blocksparse_length(self) -> int:
        """HuggingFace runs FULL attention up to and including this length (hf:modeling_big_bird.py:1574-1589)."""
        return (5 + 2 * self.num_random_blocks) * self.block_size

    def validate_for_hip(self) -> None:
        """What the gfx950 kernels are built for; anything else is refused (no fallback)."""
        if self.hidden_size % self.num_attention_heads or self.head_dim != 64:
            raise ValueError(f"head_dim must be 64 (got hidden {self.hidden_size} / heads {self.num_attention_heads})")
        if self.block_size != BLOCK:
            raise ValueError(f"block_size must be {BLOCK}: the block-sparse kernels are built for 64-row blocks")
        if self.rescale_embeddings:
            raise ValueError("rescale_embeddings=True is not implemented (the embeddings kernel adds inputs_embeds unscaled)")
        if self.attention_type != "block_sparse":
            raise ValueError(f"attention_type must be 'block_sparse', got {self.attention_type!r}: BigBird's 'original_full' "
                             "is BERT's attention - use the STonKGs classes for it")
        if self.hidden_act != "gelu_new":
            raise ValueError(f"hidden_act must be 'gelu_new' (BigBird's tanh form), got {self.hidden_act!r}")
        if not self.use_bias:
            raise ValueError("use_bias=False is not implemented: the fused q | k | v projection carries its bias")
        if self.hidden_size % 128 or self.intermediate_size % 128:
            raise ValueError("hidden_size and intermediate_size must be multiples of 128 (GEMM tiles)")
        if self.hidden_size > 1024:
            raise ValueError("hidden_size must be <= 1024 (the embeddings kernels hold a row in one wavefront)")
        if self.type_vocab_size not in (1, 2):
            raise ValueError("type_vocab_size must be 1 or 2 (stonk_embed_grad keeps sums for two token types)")
        if not 0 <= self.num_random_blocks <= 8:
            raise ValueError("num_random_blocks must be in [0, 8]")
        if self.max_position_embeddings > 64 * BLOCK:
            raise ValueError(f"max_position_embeddings must be <= {64 * BLOCK}: the kernels take at most 64 blocks a sequence")
        if not 0.0 <= self.hidden_dropout_prob < 1.0:
            raise ValueError("hidden_dropout_prob must be in [0, 1)")

    def validate_length(self, S: int) -> None:
        """The sequence lengths the encoder runs; the others are refused with what HuggingFace would have done instead."""
        if S % self.block_size:
            raise ValueError(f"sequence length {S} is no multiple of block_size {self.block_size}: HuggingFace pads such a batch "
                             "to the next multiple (with masked positions) and cuts its output back; pad the batch before the call")
        if S <= self.min_blocksparse_length:
            raise ValueError(f"sequence length {S} <= (5 + 2 * num_random_blocks) * block_size = {self.min_blocksparse_length}: "
                             "HuggingFace silently switches to full attention there (attention_type 'original_full'); this "
                             "encoder has no second code path")
        if S > self.max_position_embeddings:
            raise ValueError(f"sequence length {S} > max_position_embeddings {self.max_position_embeddings}")

    def to_dict(self) -> dict:
        return asdict(self)

    @classmethod
    def from_any(cls, obj) -> "BigBirdEncoderConfig":
        """A BigBirdEncoderConfig, a dict, or any object with BigBirdConfig-like attributes."""
        if isinstance(obj, cls):
            return obj
        src = obj if isinstance(obj, dict) else {k: getattr(obj, k) for k in cls.__dataclass_fields__ if hasattr(obj, k)}
        return cls(**{k: v for k, v in src.items() if k in cls.__dataclass_fields__})

    @classmethod
    def from_pretrained(cls, path: str) -> "BigBirdEncoderConfig":
        """Local directory (or config.json path) only."""
        f = os.path.join(path, "config.json") if os.path.isdir(path) else path
        if not os.path.exists(f):
            raise FileNotFoundError(f"{path!r} is not a local model directory: pass a directory holding config.json")
        with open(f) as fh:
            return cls.from_any(json.load(fh))

    def save_pretrained(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as fh:
            json.dump(self.to_dict(), fh, indent=2, sort_keys=True)


# ------------------------------------------------------------------------------------------------ state-dict keys
WORD = "embeddings.word_embeddings.weight"


def encoder_keys(cfg: BigBirdEncoderConfig) -> List[str]:
    """The state-dict keys of hf BigBirdModel that the encoder owns, in HuggingFace's layout (no prefix)."""
    keys = [WORD, "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
            "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layer.{i}."
        for lin in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                    "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm"):
            keys += [p + lin + ".weight", p + lin + ".bias"]
    return keys + ["pooler.weight", "pooler.bias"]


def map_state_dict(state_dict: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], List[str]]:
    """(tensors under the encoder's own keys, keys that were ignored). Two layouts: hf ``BigBirdModel``'s own, and the same
    under ``bert.`` - a ``BigBirdForPreTraining`` / ProtSTonKGs checkpoint, whose ``cls.*`` heads and backbones
    (everything outside ``bert.``) are ignored. HuggingFace's non-persistent ``position_ids`` / ``token_type_ids`` buffers
    are ignored in both. Works on any tensors (meta included): nothing is read."""
    prefixed = any(k.startswith("bert.") for k in state_dict)
    out, ignored = {}, []
    for k, v in state_dict.items():
        if prefixed and not k.startswith("bert."):
            ignored.append(k)
            continue
        name = k[len("bert."):] if prefixed else k
        if name in ("embeddings.position_ids", "embeddings.token_type_ids"):
            ignored.append(k)
            continue
        out[name] = v
    return out, ignored


# ------------------------------------------------------------------------------------------------ engine
class BigBirdEngine(LayerEngine):
    """The encoder's launches. A layer is `LayerEngine.layer_fwd` / `layer_bwd` in the padded layout with four methods replaced:
    the attention core (stonk_block_sparse_attention_*_ex with STONK_BSA_ZERO_MASKED_QUERIES, no probability dropout) and
    the FFN activation (bias-only GEMM, then stonk_gelu_new_*: the GEMM epilogues carry the erf form only)."""

    ERR_BITS = {1: "a block list entry, multiplicity or count of an attention plan is out of range"}
    KEY_ERROR_BITS = 0

    def __init__(self, cfg: BigBirdEncoderConfig, store: FlatStore, device):
        super().__init__(cfg, store, device)
        self.plans: List[BlockSparsePlan] = []   # one per layer, for the sequence length of the call in flight
        self.generation = 0                      # training forwards so far: a backward must belong to the latest

    # ---- the four methods
    def _attention_fwd(self, qkv, mask, cu, qoff, ctx, lse, B, NH, seq, p_att, lidx, st) -> None:
        H = self.cfg.hidden_size
        lists, _ = self.plans[lidx].on(self.device)
        p = qkv.data_ptr()
        hip.call("stonk_block_sparse_attention_fwd_ex", p, p + 2 * H, p + 4 * H, 3 * H, hip.ptr(mask),
                 *(t.data_ptr() for t in lists[:3]), ctx.data_ptr(), H, lse.data_ptr(), B, NH, seq, 64, 1.0 / math.sqrt(64.0),
                 self.err.data_ptr(), hip.BSA_ZERO_MASKED_QUERIES, st)

    def _attention_bwd(self, qkv, mask, cu, qoff, ctx, dctx, lse, delta, dqkv, B, NH, seq, p_att, lidx, st) -> None:
        H = self.cfg.hidden_size
        lists, _ = self.plans[lidx].on(self.device)
        ws = self.buf("b.bbws", (2, B, NH, seq), F32)
        p, g = qkv.data_ptr(), dqkv.data_ptr()
        hip.call("stonk_block_sparse_attention_bwd_ex", p, p + 2 * H, p + 4 * H, 3 * H, hip.ptr(mask),
                 *(t.data_ptr() for t in lists), ctx.data_ptr(), H, dctx.data_ptr(), H, lse.data_ptr(), ws.data_ptr(), g, g + 2 * H,
                 3 * H, g + 4 * H, B, NH, seq, 64, 1.0 / math.sqrt(64.0), self.err.data_ptr(), hip.BSA_ZERO_MASKED_QUERIES, st)

    def _ffn_up(self, S: FlatStore, prefix: str, hf, g, u, Tf) -> None:
        H, I = self.cfg.hidden_size, self.cfg.intermediate_size
        if u is None:   # (forward-only: the pre-activation still needs a place)
            u = self.buf("tmp.u", (g.shape[0], I))
        self.gemm(hf, S.bf16_view(prefix + ".intermediate.dense.weight"), u, Tf, I, H, flags=hip.EPI_BIAS,
                  bias=S.view(prefix + ".intermediate.dense.bias"), kernel=self._kernel("ffn_up"))
        hip.call("stonk_gelu_new_fwd_bf16", u.data_ptr(), g.data_ptr(), Tf * I, hip.stream_ptr())

    def _ffn_down_dgrad(self, prefix: str, df, du, u, Tf) -> None:
        H, I = self.cfg.hidden_size, self.cfg.intermediate_size
        self.gemm(df, self.P.wt[prefix + ".output.dense.weight"], du, Tf, I, H, kernel=self._kernel("dgrad_gelu", True))
        hip.call("stonk_gelu_new_bwd_bf16", du.data_ptr(), u.data_ptr(), du.data_ptr(), Tf * I, hip.stream_ptr())   # in place

    # ---- the whole encoder
    def encode_embeds(self, inputs_embeds, attention_mask, token_type_ids, plans, training: bool, save: Optional[dict]):
        """inputs_embeds fp32 [B, S, H] contiguous, attention_mask / token_type_ids int64 [B, S] or None, one plan per layer.
        Returns (sequence output bf16 [B*S, H], pooled fp32 [B, H]) - workspace views; `save` (None: forward-only, scratch
        buffers of its own) keeps what `backward_embeds` reads."""
        cfg = self.cfg
        H = cfg.hidden_size
        B, S = inputs_embeds.shape[0], inputs_embeds.shape[1]
        T = B * S
        st = hip.stream_ptr()
        f = self.P.view
        self.wait_params()
        self.seed_base += 1
        if save is not None:
            self.generation += 1
        p_hid = cfg.hidden_dropout_prob if training else 0.0
        e = "e" if save is not None else "et"
        sum0, x = self.buf(f"{e}.sum0", (T, H)), self.buf(f"{e}.x0", (T, H))
        st0 = self.buf(f"{e}.st0", (2, T), F32)
        hip.call("stonk_embeds_ln_fwd", inputs_embeds.data_ptr(), H, hip.ptr(token_type_ids),
                 f("bert.embeddings.position_embeddings.weight").data_ptr(),
                 f("bert.embeddings.token_type_embeddings.weight").data_ptr(), f("bert.embeddings.LayerNorm.weight").data_ptr(),
                 f("bert.embeddings.LayerNorm.bias").data_ptr(), sum0.data_ptr(), x.data_ptr(), st0[0].data_ptr(),
                 st0[1].data_ptr(), B, S, H, cfg.type_vocab_size, cfg.layer_norm_eps, p_hid, self.seed(200, 0), st)
        L = padded_rows(B, S, attention_mask)
        self.plans = list(plans)
        for i in range(cfg.num_hidden_layers):
            x = self.layer_fwd(self.P, f"bert.encoder.layer.{i}", x, L, p_hid, 0.0, i, save)
        pooled = self.buf(f"{e}.pooled", (B, H), F32)
        hip.call("stonk_small_linear_fwd", x.data_ptr(), S * H, f("bert.pooler.dense.weight").data_ptr(),
                 f("bert.pooler.dense.bias").data_ptr(), pooled.data_ptr(), B, H, H, hip.SMALL_TANH, st)
        if save is not None:
            save.update(layout=L, token_type_ids=token_type_ids, sum0=sum0, st0=st0, seq_out=x, pooled=pooled, p_hid=p_hid,
                        plans=self.plans, seed_base=self.seed_base, generation=self.generation)
        return x, pooled

    def backward_embeds(self, dseq, dpooled, sv: dict, d_inputs_embeds) -> None:
        """dseq fp32 [B, S, H] and dpooled fp32 [B, H] (contiguous): the gradients of the two outputs. Parameter gradients are
        ACCUMULATED into the store's gradient buffer; d(inputs_embeds) is written to `d_inputs_embeds` (fp32 [B, S, H])."""
        if sv["generation"] != self.generation:
            raise RuntimeError("backward through a BigBirdEncoderModel forward that a later training forward has replaced: the "
                               "saved activations live in one workspace - run forward and backward in pairs")
        cfg = self.cfg
        H = cfg.hidden_size
        L = sv["layout"]
        B, S, T = L.B, L.S, L.T
        st = hip.stream_ptr()
        f, g_ = self.P.view, self.P.grad_view
        seed_now, self.seed_base = self.seed_base, sv["seed_base"]   # the forward's dropout masks
        self.plans = sv["plans"]
        try:
            dy = self.buf("b.dseq", (T, H))
            hip.call("stonk_cast_f32_to_bf16", dseq.data_ptr(), dy.data_ptr(), T * H, st)
            # pooler (tanh) backward: into position 0 of every sequence's row of d(sequence output)
            hip.call("stonk_small_linear_bwd", dpooled.data_ptr(), sv["pooled"].data_ptr(), sv["seq_out"].data_ptr(), S * H,
                     f("bert.pooler.dense.weight").data_ptr(), g_("bert.pooler.dense.weight").data_ptr(),
                     g_("bert.pooler.dense.bias").data_ptr(), 0, dy.data_ptr(), S * H, B, H, H, hip.SMALL_TANH, st)
            for i in reversed(range(cfg.num_hidden_layers)):
                prefix = f"bert.encoder.layer.{i}"
                dy = self.layer_bwd(prefix, dy, L, sv["p_hid"], 0.0, i, sv[prefix])
            # embeddings: LayerNorm, then the dropout in front of it, then the position / token-type tables
            dsum = self.buf("b.dsum0", (T, H))
            self.ln_bwd(dy, sv["sum0"], sv["st0"][0], sv["st0"][1], f("bert.embeddings.LayerNorm.weight"), dsum, None,
                        g_("bert.embeddings.LayerNorm.weight"), g_("bert.embeddings.LayerNorm.bias"), T, H, 0, 0.0, 0, 0.0, 0)
            dxm = self.buf("b.dxm", (T, H))
            hip.call("stonk_embeds_ln_bwd_finish", dsum.data_ptr(), H, d_inputs_embeds.data_ptr(), H, dxm.data_ptr(), T, H,
                     sv["p_hid"], self.seed(200, 0), st)
            hip.call("stonk_embed_grad", dxm.data_ptr(), hip.ptr(sv["token_type_ids"]),
                     g_("bert.embeddings.position_embeddings.weight").data_ptr(),
                     g_("bert.embeddings.token_type_embeddings.weight").data_ptr(), B, S, H, cfg.type_vocab_size, 0, st)
            self.join_wgrad()
        finally:
            self.seed_base = seed_now


# ------------------------------------------------------------------------------------------------ autograd bridge
class _EncoderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs_embeds, anchor, model, attention_mask, token_type_ids, plans):
        save: dict = {}
        seq, pooled = model.engine.encode_embeds(inputs_embeds, attention_mask, token_type_ids, plans, model.training, save)
        ctx.model, ctx.saved = model, save
        B, S, H = inputs_embeds.shape
        return seq.view(B, S, H).float(), pooled.clone()

    @staticmethod
    def backward(ctx, dseq, dpooled):
        model, sv = ctx.model, ctx.saved
        L = sv["layout"]
        H = model.config.hidden_size
        dev = model.device
        dseq = torch.zeros(L.B, L.S, H, device=dev) if dseq is None else dseq.to(torch.float32).contiguous()
        dpooled = torch.zeros(L.B, H, device=dev) if dpooled is None else dpooled.to(torch.float32).contiguous()
        d_in = torch.empty(L.B, L.S, H, device=dev, dtype=torch.float32)
        model._prepare_grads_for_autograd()
        model.engine.backward_embeds(dseq, dpooled, sv, d_in)
        model._reattach_grads()
        model._external_step_pending = True   # whoever called backward() steps the masters with its own optimizer
        return d_in, None, None, None, None, None


# ------------------------------------------------------------------------------------------------ model
class BigBirdEncoderModel(FlatBufferModel):
    """hf ``BigBirdModel(inputs_embeds=..., attention_mask=..., token_type_ids=...)`` with block-sparse attention:
    ``forward`` returns ``(sequence_output fp32 [B, S, H], pooler_output fp32 [B, H])``, computed in bf16 between the
    kernels. Differentiable: ``loss.backward()`` gives ``inputs_embeds.grad`` and accumulates the parameter gradients into
    the flat gradient buffer the parameters' ``.grad`` views name, so a torch optimizer or ``FusedAdamW(model._store)``
    trains it. One training forward is alive at a time (its activations live in one workspace): backward belongs to the
    latest one.

    Plans: ``.eval()`` uses the zeros plan (HuggingFace's at 1024, 3072 and 4096 tokens), ``.train()`` one plan per layer
    drawn from ``bigbird_rand_attn(..., seed=layer index)``; ``set_rand_attn(layer, array)`` installs an explicit one.
    ``embeddings.word_embeddings.weight`` is a dead parameter (the encoder takes ``inputs_embeds``): kept so that a
    checkpoint round-trips."""

    def __init__(self, config, *, device=None, seed: int = 0):
        super().__init__(device)
        cfg = BigBirdEncoderConfig.from_any(config)
        cfg.validate_for_hip()
        self.config = cfg
        dev = self._device
        self._store = FlatStore(trainable_specs(cfg, False), dev, trainable=True)
        word = torch.nn.Parameter(torch.zeros(cfg.vocab_size, cfg.hidden_size, device=dev), requires_grad=False)
        bert = build_bert_tree(self._store, "bert", cfg, cfg.num_hidden_layers, True, word)
        self.embeddings, self.encoder = bert.embeddings, bert.encoder
        self.pooler = _linear(self._store, "bert.pooler.dense", True)      # (hf BigBirdModel.pooler is the Linear itself)
        self.engine = BigBirdEngine(cfg, self._store, dev)
        self._plans: Dict[tuple, BlockSparsePlan] = {}       # (layer, blocks, training) -> plan
        self.ignored_keys: List[str] = []                    # what the latest load_state_dict ignored
        self._init_weights(seed)
        self._bind_grad_views()
        self.refresh()

    def _stores(self) -> tuple:
        return (self._store,)

    # -------------------------------------------------------------- plans
    def set_rand_attn(self, layer: int, rand_attn, training: Optional[bool] = None) -> None:
        """Install the random blocks of layer `layer`: int [num_heads, nb - 2, r] as ``bigbird_rand_attn`` returns them (what
        HuggingFace's ``rand_attn`` holds per sequence), for sequences of nb blocks. `training` None: for both modes."""
        ra = np.asarray(rand_attn)
        if not 0 <= int(layer) < self.config.num_hidden_layers:
            raise ValueError(f"layer must be in [0, {self.config.num_hidden_layers}), got {layer}")
        if ra.ndim != 3 or ra.shape[0] != self.config.num_attention_heads:
            raise ValueError(f"rand_attn must be [num_heads = {self.config.num_attention_heads}, nb - 2, r], got {ra.shape}")
        nb = ra.shape[1] + 2
        plan = BlockSparsePlan(nb, ra)      # (validates the values)
        for mode in ((False, True) if training is None else (bool(training),)):
            self._plans[(int(layer), nb, mode)] = plan

    def plan_for(self, layer: int, num_blocks: int) -> BlockSparsePlan:
        key = (int(layer), int(num_blocks), bool(self.training))
        if key not in self._plans:
            cfg = self.config
            ra = bigbird_rand_attn(num_blocks, cfg.num_random_blocks, cfg.num_attention_heads,
                                   "train" if self.training else "eval", seed=int(layer))
            self._plans[key] = BlockSparsePlan(num_blocks, ra)
        return self._plans[key]

    def set_dropout_seed(self, seed: int) -> None:
        """The base of the next forward's dropout masks (every launch site derives its own seed from it; every forward moves
        the base on by one, so two calls repeat each other only behind the same ``set_dropout_seed``)."""
        self.engine.seed_base = int(seed)

    # -------------------------------------------------------------- state dict
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False, _refresh: bool = True):
        """Takes hf ``BigBirdModel``'s layout, or the same under ``bert.`` (``map_state_dict``); what was ignored is kept in
        ``self.ignored_keys`` and warned about."""
        sd, self.ignored_keys = map_state_dict(state_dict)
        if self.ignored_keys:
            warnings.warn(f"BigBirdEncoderModel.load_state_dict ignored {len(self.ignored_keys)} keys outside the encoder: "
                          f"{self.ignored_keys[:4]}{'...' if len(self.ignored_keys) > 4 else ''}")
        return super().load_state_dict(sd, strict=strict, _refresh=_refresh)

    @classmethod
    def from_pretrained(cls, path: str, **kwargs) -> "BigBirdEncoderModel":
        """Local directory in HF layout (config.json + pytorch_model.bin / model.safetensors)."""
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path!r}: only local checkpoints can be loaded")
        model = cls(BigBirdEncoderConfig.from_pretrained(path), **kwargs)
        sd = _load_weights_file(path)
        if sd is None:
            raise FileNotFoundError(f"no pytorch_model.bin / model.safetensors under {path!r}")
        missing, unexpected = model.load_state_dict(sd, strict=False)
        bad = [k for k in missing if k != WORD]
        if bad or unexpected:
            raise KeyError(f"checkpoint misses {bad[:5]} / holds unknown keys {list(unexpected)[:5]}")
        return model

    # -------------------------------------------------------------- forward
    def forward(self, inputs_embeds, attention_mask=None, token_type_ids=None):
        cfg = self.config
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[2] != cfg.hidden_size:
            raise ValueError(f"inputs_embeds must be [B, S, {cfg.hidden_size}], got {tuple(inputs_embeds.shape)}")
        B, S, _ = inputs_embeds.shape
        cfg.validate_length(S)
        x = inputs_embeds
        if x.device != self._device or x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(device=self._device, dtype=torch.float32).contiguous()
        am, tt = self._long(attention_mask), self._long(token_type_ids)
        for name, t in (("attention_mask", am), ("token_type_ids", tt)):
            if t is not None and tuple(t.shape) != (B, S):
                raise ValueError(f"{name} must be [{B}, {S}], got {tuple(t.shape)}")
        if tt is not None and B and (int(tt.min()) < 0 or int(tt.max()) >= cfg.type_vocab_size):
            raise IndexError("token_type_id outside [0, type_vocab_size)")     # (the kernel has no error word for it)
        self._sync_derived()
        plans = [self.plan_for(i, S // BLOCK) for i in range(cfg.num_hidden_layers)]
        if torch.is_grad_enabled():
            return _EncoderFunction.apply(x, self._anchor, self, am, tt, plans)
        seq, pooled = self.engine.encode_embeds(x, am, tt, plans, self.training, None)
        return seq.view(B, S, cfg.hidden_size).float(), pooled.clone()
