"""HIP execution engines of the STonKGs hot path: what STonKGs puts around the layers of `layer_engine.LayerEngine` (which
owns the workspace, the streams, the GEMM and weight-gradient wrappers, the derived weights and one BERT layer).

`Engine(LayerEngine)` owns the frozen LM backbone and its prefetch stream, the row plan of the unpadded encoder, `encode`,
the label-sparse heads, `forward` / `backward`, the calls training must not notice (`evaluate`, `attention_maps`,
`input_gradients`) and the classification head. `TextEngine(Engine)` is the text-only baseline: a trainable word table in
the backbone's place.

Call structure mirrors SURVEY.md section 3.2 (ref:src/stonkgs/models/stonkgs_model.py:149-258):
  F1 frozen LM backbone on the text half  ->  F2 KG gather + concat + embeddings LayerNorm  ->  F3 encoder layers
  ->  F4 pooler / NSP  ->  F5 head transform  ->  F6 label-sparse decoders + fused cross-entropy
and the mirrored backward.
"""
from __future__ import annotations

import collections
import contextlib
from typing import Callable, Dict, Optional

import torch

from . import _hip as hip
from .config import STonKGsConfig
from .layer_engine import BF16, F32, I32, GemmTimer, LayerEngine, ReadRows, Rows, padded_rows  # noqa: F401 (re-exported)
from .params import FlatStore, pad128

ERR_BITS = {1: "entity id outside the KG table (the reference raises KeyError, stonkgs_model.py:185)",
            2: "token_type_id outside [0, type_vocab_size)", 4: "text token id outside the LM vocabulary",
            8: "MLM/ELM label outside the decoder's class range", 16: "NSP label outside [0, 2)"}

Decoder = collections.namedtuple("Decoder", "name label_key weight classes offset")


def decoders(cfg: STonKGsConfig):
    """The two label-sparse decoders of the pre-training head, in the order of the loss terms (backward runs them in
    reverse: the flat gradient buffer's order). `offset`: the first sequence position a decoder predicts."""
    return (Decoder("text", "masked_lm_labels", "cls.predictions.text_decoder.weight", cfg.vocab_size, 0),
            Decoder("ent", "ent_masked_lm_labels", "cls.predictions.entity_decoder.weight", cfg.kg_vocab_size,
                    cfg.half_length))


class Engine(LayerEngine):
    ERR_BITS = ERR_BITS      # the bits STonKGs' embedding and loss kernels set in the error word ...
    KEY_ERROR_BITS = 1       # ... of which the entity id is a KeyError, as in the reference

    def __init__(self, cfg: STonKGsConfig, store: FlatStore, backbone: FlatStore, n_backbone_layers: int, device):
        super().__init__(cfg, store, device)
        self.BB = backbone
        self.n_bb = n_backbone_layers
        self.kg_table: Optional[torch.Tensor] = None  # fp32 [K+3, H]
        self.saved = None
        self.f16_logits = True      # label-sparse decoder logits in fp16 (False: fp32, 4 more bytes of HBM traffic per logit)
        # Unpadded trainable encoder (csrc/unpad.hip): rows that are neither live keys, nor labelled, nor position 0 are
        # dropped before the embeddings LayerNorm - no loss term and no gradient reads them - and every per-row kernel,
        # GEMM and the attention run on the packed rows. Used by the training paths that hand out neither hidden states
        # nor dense logits (`forward_backward`, `forward(..., return_dict=False)` in training mode); costs one host wait
        # per step for the packed row count, taken while the frozen backbone's forward is already queued.
        self.unpad = True
        # ... and, in the packed layout, the LAST layer's feed-forward block, the pooler and the head transform run on the
        # READ rows only (labelled positions + position 0: ~77 of a sequence's ~410 rows) - they are row-wise, and nothing
        # reads the last layer's output at any other row. Attention and its projections still see every row (keys).
        self.prune_last_ffn = True
        # ... and so does the last layer's attention block behind the QKV projection: the row plan puts a sequence's read
        # rows first, the attention kernels compute the first rows of every sequence as queries only (`q_offsets`; keys and
        # values: every row), and the output projection + LayerNorm run on the gathered read rows.
        self.prune_last_attn = True
        # The frozen backbone's forward depends on the batch's token ids and on frozen weights only: given a hint of the NEXT
        # batch (`next_input_ids`, set by the trainer) it is queued on a stream of its own at the start of the current step and
        # runs beside the current step's encoder forward, where no weight-gradient stream competes for the CUs.
        self.next_input_ids: Optional[torch.Tensor] = None
        self._prefetch: Optional[dict] = None
        self._bb_stream: Optional[torch.cuda.Stream] = None
        self._pref_par = 0
        # what ran: [rows, padded rows they stand for, encoder passes, sum over sequences of rows^2, of S^2] - bench.py prices
        # the step on the FLOPs actually executed (linear layers ~ rows, attention ~ rows^2 per sequence)
        # (sixth: rows of the last layer's feed-forward block / pooler / head; seventh: query rows x key rows of the last
        # layer's attention, summed over sequences)
        self.rows_executed = [0, 0, 0, 0, 0, 0, 0]
        self._plan_host: Optional[torch.Tensor] = None

    def _mirrored_stores(self) -> tuple:
        return self.P, self.BB

    # ------------------------------------------------------------------ frozen backbone
    def backbone_fwd(self, input_ids, ld_ids, B, seq, training: bool, mask=None):
        cfg = self.cfg
        H = cfg.hidden_size
        p_hid = cfg.hidden_dropout_prob if training else 0.0  # quirk Q6: dropout is live inside the frozen LM
        p_att = cfg.attention_probs_dropout_prob if training else 0.0
        f = self.BB.view
        x = self.buf("bb.x", (B * seq, H))
        hip.call("stonk_text_embed_ln_fwd", input_ids.data_ptr(), ld_ids,
                 f("lm_backbone.embeddings.word_embeddings.weight").data_ptr(),
                 f("lm_backbone.embeddings.position_embeddings.weight").data_ptr(),
                 f("lm_backbone.embeddings.token_type_embeddings.weight").data_ptr(),
                 f("lm_backbone.embeddings.LayerNorm.weight").data_ptr(),
                 f("lm_backbone.embeddings.LayerNorm.bias").data_ptr(), x.data_ptr(), B, seq, H, cfg.vocab_size,
                 cfg.layer_norm_eps, hip.LN_DROPOUT if p_hid > 0 else 0, p_hid, self.seed(100, 0), self.err.data_ptr(),
                 hip.stream_ptr())
        L = padded_rows(B, seq, mask)
        for i in range(self.n_bb):
            x = self.layer_fwd(self.BB, f"lm_backbone.encoder.layer.{i}", x, L, p_hid, p_att, 101 + i, None)
        return x

    def prefetch_backbone(self, input_ids, training: bool) -> None:
        """Queue the frozen backbone's forward for a FUTURE batch on the backbone stream (ordered after everything queued so
        far on the current stream: the ids are there, the previous prefetch's consumer has read its buffer). The result is
        kept in one of two buffers until `encode` is called with the same ids."""
        cfg = self.cfg
        H, S, half = cfg.hidden_size, cfg.max_position_embeddings, cfg.half_length
        B = input_ids.shape[0]
        self._pref_par ^= 1
        out = self.buf(f"bb.pref{self._pref_par}", (B * half, H))   # (allocated, if it has to be, on the current stream)
        with self._fork("_bb_stream"):
            # dropout masks are a function of (step counter, layer, site, element): the prefetched forward draws the masks
            # of the step that will CONSUME it (the counter advances once per encode), so a run that prefetches and one
            # that does not - or a resumed one - see the same masks
            self.seed_base += 1
            try:
                x = self.backbone_fwd(input_ids, S, B, half, training)
            finally:
                self.seed_base -= 1
            out.copy_(x)
            done = torch.cuda.Event()
            done.record()
        self._prefetch = dict(ids=input_ids, ptr=input_ids.data_ptr(), ver=input_ids._version, shape=tuple(input_ids.shape),
                              out=out, done=done, training=training)

    def _take_prefetched(self, input_ids, training: bool):
        """The prefetched backbone output for exactly these ids (same storage, same version, same mode), or None. Either
        way the current stream is ordered after the prefetch: its scratch buffers are the inline forward's too."""
        pf, self._prefetch = self._prefetch, None
        if pf is None:
            return None
        torch.cuda.current_stream().wait_event(pf["done"])
        hit = (pf["ptr"] == input_ids.data_ptr() and pf["ver"] == input_ids._version and
               pf["shape"] == tuple(input_ids.shape) and pf["training"] == training)
        return pf["out"] if hit else None

    def special_vectors(self) -> Dict[int, torch.Tensor]:
        """Quirk Q2: kg_backbone[sid] = lm_backbone([[sid]])[0][0][0], eval mode. A 1-token sequence is run as a
        128-token sequence whose only unmasked key is position 0 - identical arithmetic for that position."""
        ids = torch.zeros(3, 128, dtype=torch.long, device=self.device)
        ids[:, 0] = torch.tensor([102, 103, 100], device=self.device)
        mask = torch.zeros(3, 128, dtype=torch.long, device=self.device)
        mask[:, 0] = 1
        out = self.backbone_fwd(ids, 128, 3, 128, False, mask=mask).view(3, 128, -1)[:, 0].float()
        return {102: out[0].clone(), 103: out[1].clone(), 100: out[2].clone()}

    # ------------------------------------------------------------------ forward
    def _plan_rows(self, attention_mask, mlm_labels, ent_labels, B, S, half, keep: bool):
        """Launch the row plan of the unpadded encoder (csrc/unpad.hip) on the current stream and start the copy of the
        packed row count to the host; returns (plan dict, event). The caller queues the frozen backbone's forward - which
        does not depend on the plan - and only then waits for the event, so the GPU has work while the host learns the
        count. `keep`: the plan belongs to a forward whose backward will read it (its maps live in buffers of their own,
        which a forward-only call in between - evaluation, embedding extraction - does not touch)."""
        n = B * S
        u = "u" if keep else "ut"
        row_of_pos = self.buf(f"{u}.row_of_pos", (n,), I32)
        pos_of_row = self.buf(f"{u}.pos_of_row", (n,), I32)
        row_mask = self.buf(f"{u}.row_mask", (n,), torch.int64)
        offs = self.buf(f"{u}.offsets", (2 * (B + 1),), I32)     # [sequence offsets | read-row offsets]: one copy to the host
        cu, cu_rd = offs[:B + 1], offs[B + 1:]
        read_rows = self.buf(f"{u}.read_rows", (n,), I32)
        read_of_pos = self.buf(f"{u}.read_of_pos", (n,), I32)
        ws = self.buf("u.ws", (int(hip.lib().stonk_unpad_workspace_ints(B)),), I32)
        hip.call("stonk_unpad_plan", attention_mask.data_ptr(), hip.ptr(mlm_labels), hip.ptr(ent_labels), B, S, half,
                 row_of_pos.data_ptr(), pos_of_row.data_ptr(), cu.data_ptr(), row_mask.data_ptr(), read_rows.data_ptr(),
                 read_of_pos.data_ptr(), cu_rd.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream_ptr())
        if self._plan_host is None or self._plan_host.numel() < 2 * (B + 1):
            self._plan_host = torch.empty(2 * (B + 1), dtype=I32).pin_memory()
        self._plan_host[:2 * (B + 1)].copy_(offs, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return dict(row_of_pos=row_of_pos, pos_of_row=pos_of_row, cu=cu, row_mask=row_mask, read_rows=read_rows,
                    read_of_pos=read_of_pos, cu_rd=cu_rd), ev

    @property
    def half_length(self) -> int:
        """Positions of a sequence the embeddings kernel takes from `_text_half`'s rows; the rest are table lookups."""
        return self.cfg.half_length

    def _text_half(self, input_ids, B, training: bool):
        """F1 frozen backbone (no attention mask: quirk Q5; always padded - its padding positions ARE attended). Returns
        (text_hidden, hint): `hint` = the next batch's ids when their prefetch is still to be queued by the caller."""
        S, half = self.cfg.max_position_embeddings, self.half_length
        with self.block("K1 frozen backbone fwd"):
            text_hidden = self._take_prefetched(input_ids, training)
            hit = text_hidden is not None
            if not hit:
                text_hidden = self.backbone_fwd(input_ids, S, B, half, training)
            # The next batch's backbone forward, if the trainer named the batch. After a hit it is queued HERE, before the
            # wait for the optimizer: it then runs beside AdamW (HBM-bound) and the encoder forward below. After a miss the
            # inline forward's scratch buffers are still to be read by the embedding kernel: queued behind that kernel.
            hint, self.next_input_ids = self.next_input_ids, None
            if hint is not None and hit:
                self.prefetch_backbone(hint, training)
                hint = None
        return text_hidden, hint

    def encode(self, input_ids, attention_mask, token_type_ids, training: bool, save: dict, unpad_labels=None,
               attn_maps: Optional[dict] = None):
        """F1-F4: frozen backbone, KG gather + embeddings LayerNorm, encoder layers, pooler. Shared by the pre-training
        and the sequence-classification models (ref:stonkgs_model.py:178-212, ref:stonkgs_finetuning.py:277-310).
        `unpad_labels`: None = padded layout (every position a row: callers that hand out hidden states or dense
        logits); a (text_labels, entity_labels) pair (either may be None) = packed layout, see `Engine.unpad`.
        `attn_maps` (forward-only, padded layout, dropout off): {layer index: (probs or None, modal_mass or None)} - the
        selected layers write their attention probabilities into these tensors (`layer_fwd`).
        Returns (sequence output, pooled, the row layout `Rows`); `save` keeps the layout too (`save["layout"]`)."""
        cfg = self.cfg
        H, S, half = cfg.hidden_size, cfg.max_position_embeddings, self.half_length
        B = input_ids.shape[0]
        cap = B * S
        if attn_maps and (training or save is not None or unpad_labels is not None):
            raise ValueError("attention maps need a forward-only call in the padded layout with dropout off")
        st = hip.stream_ptr()
        P = self.P
        f = P.view
        self.seed_base += 1
        p_hid = cfg.hidden_dropout_prob if training else 0.0
        p_att = cfg.attention_probs_dropout_prob if training else 0.0
        plan = ev = None
        if unpad_labels is not None and attention_mask is not None and self.unpad and B > 0:
            plan, ev = self._plan_rows(attention_mask, unpad_labels[0], unpad_labels[1], B, S, half, keep=save is not None)
        text_hidden, hint = self._text_half(input_ids, B, training)
        self.wait_params()   # everything above read frozen weights only; from here on the trainable ones
        if plan is None:
            L = padded_rows(B, S, attention_mask)
            sq = sq_last = B * S * S
        else:
            self.mark("plan_wait")
            ev.synchronize()                       # (a backbone forward - this batch's or the next one's - is queued: the GPU has work)
            self.mark("plan_known")
            host = self._plan_host[:2 * (B + 1)].tolist()
            offs, n_read = host[:B + 1], host[2 * B + 1]
            rd = None
            if self.prune_last_ffn:
                rd = ReadRows(rows=plan["read_rows"], cnt=plan["cu_rd"][B:B + 1], n=n_read, offsets=plan["cu_rd"],
                              T=min(cap, (n_read + 63) // 64 * 64), attn=self.prune_last_attn)
            # T: whole 64-row K tiles for the weight gradients; the tail rows are zeros
            L = Rows(B, S, T=min(cap, (offs[B] + 63) // 64 * 64), rows=offs[B], mask=plan["row_mask"], cu=plan["cu"],
                     row_of_pos=plan["row_of_pos"], pos_of_row=plan["pos_of_row"], read_of_pos=plan["read_of_pos"], rd=rd)
            sq = sq_last = sum((offs[i + 1] - offs[i]) ** 2 for i in range(B))
            if rd is not None and rd.attn:
                sq_last = sum((host[B + 2 + i] - host[B + 1 + i]) * (offs[i + 1] - offs[i]) for i in range(B))
        for i, v in enumerate((L.T, cap, 1, sq, B * S * S, L.Th, sq_last)):
            self.rows_executed[i] += v
        # F2 gather + concat + embeddings LayerNorm
        # (a forward-only call - save is None - works in scratch buffers of its own throughout: it may run between a
        # training forward and its backward without touching what that backward reads)
        e = "e" if save is not None else "et"
        sum0 = self.buf(f"{e}.sum0", (cap, H))
        x = self.buf(f"{e}.x0", (cap, H))
        st0 = self.buf(f"{e}.st0", (2, cap), F32)
        hip.call("stonk_joint_embed_ln_fwd", input_ids.data_ptr(), hip.ptr(token_type_ids), text_hidden.data_ptr(),
                 self.kg_table.data_ptr(), f("bert.embeddings.position_embeddings.weight").data_ptr(),
                 f("bert.embeddings.token_type_embeddings.weight").data_ptr(),
                 f("bert.embeddings.LayerNorm.weight").data_ptr(), f("bert.embeddings.LayerNorm.bias").data_ptr(),
                 sum0.data_ptr(), x.data_ptr(), st0[0].data_ptr(), st0[1].data_ptr(), B, S, half, H,
                 self.kg_table.shape[0], cfg.type_vocab_size, cfg.layer_norm_eps, hip.LN_DROPOUT if p_hid > 0 else 0,
                 p_hid, self.seed(200, 0), self.err.data_ptr(), hip.ptr(L.pos_of_row), L.T if L.packed else 0, st)
        if hint is not None:   # (after an inline backbone forward: behind the kernel above, the last reader of its scratch)
            self.prefetch_backbone(hint, training)
        # F3 encoder
        self.mark("encoder_fwd_begin")
        span = self._span_begin()
        last = cfg.num_hidden_layers - 1
        for i in range(cfg.num_hidden_layers):
            with self.block(f"K4-K8 encoder layer {i} fwd"):
                am = attn_maps.get(i) if attn_maps else None
                x = self.layer_fwd(P, f"bert.encoder.layer.{i}", x, L, p_hid, p_att, i, save, last=i == last,
                                   attn_maps=None if am is None else (am[0], am[1], half))
        self._span_end("encoder_fwd", span)
        seq_out = x                                # [L.Th rows]: every packed row, or the read rows only
        # F4 pooler (fp32 master weights) on position 0 of every sequence
        pooled = self.buf(f"{e}.pooled", (B, H), F32)
        if not L.packed:
            first, ld_first = seq_out, S * H
        else:   # packed: position 0 of sequence b is row cu[b] (among the read rows: read_offsets[b])
            nb = self.buf(f"{e}.nb", (1,), I32)
            nb.fill_(B)
            first, ld_first = self.buf(f"{e}.first", ((B + 127) // 128 * 128, H)), H
            self._gather_rows(seq_out, L.first_rows, nb, first, first.shape[0])
        hip.call("stonk_small_linear_fwd", first.data_ptr(), ld_first, f("bert.pooler.dense.weight").data_ptr(),
                 f("bert.pooler.dense.bias").data_ptr(), pooled.data_ptr(), B, H, H, hip.SMALL_TANH, st)
        if save is not None:   # (None: forward-only callers - embedding extraction, batched inference)
            save.update(layout=L, input_ids=input_ids, token_type_ids=token_type_ids, sum0=sum0, st0=st0, seq_out=seq_out,
                        pooled=pooled, p_hid=p_hid, p_att=p_att, first=first, ld_first=ld_first, text_hidden=text_hidden)
        return seq_out, pooled, L

    def _sparse_head(self, pre, dec: Decoder, labels, t, row_of_pos, cnt, loss_sum, B, need_backward,
                     grad_scale: float = 1.0):
        """One label-sparse decoder + fused cross-entropy (F6), shared by the training forward (`pre` = "l") and `evaluate`
        ("ev": small buffers of its own, so that it may run between a forward and its backward): compaction of the labelled
        positions into rows of `t` (through `row_of_pos` in the packed layout), row gather, decoder GEMM over the
        device-side count, cross-entropy into `loss_sum` (+ dlogits when `need_backward`). The logits buffer is the same
        for both callers - nothing reads it after the call that filled it. `grad_scale`: dlogits = (softmax - onehot) *
        grad_scale / count. Returns dict(rows, tg, cnt, hs, logits, dl)."""
        H, S, half = self.cfg.hidden_size, self.cfg.max_position_embeddings, self.cfg.half_length
        nm, N = dec.name, dec.classes
        cap, npad, st = B * half, pad128(N), hip.stream_ptr()
        rows = self.buf(f"{pre}.{nm}.rows", (cap,), I32)
        tg = self.buf(f"{pre}.{nm}.tg", (cap,), I32)
        hip.call("stonk_label_compact", labels.data_ptr(), cap, half, S, dec.offset, rows.data_ptr(), tg.data_ptr(),
                 cnt.data_ptr(), hip.ptr(row_of_pos), st)
        hs = self.buf(f"{pre}.{nm}.hs", (cap, H))
        self._gather_rows(t, rows, cnt, hs, cap)
        # logits of the labelled rows only, in fp16 (11 significant bits; the softmax arithmetic stays fp32): the
        # decoder GEMM writes and the cross-entropy reads 2 bytes per logit instead of 4 - both are HBM-bound on them
        f16 = self.f16_logits
        logits = self.buf(f"l.{nm}.logits", (cap, npad), torch.float16 if f16 else F32)
        self.gemm(hs, self.P.bf16_view(dec.weight), logits, cap, npad, H, flags=hip.EPI_OUT_F16 if f16 else hip.EPI_OUT_F32,
                  m_dev=cnt)
        dl = self.buf(f"{pre}.{nm}.dl", (cap, npad)) if need_backward else None
        hip.call("stonk_softmax_xent_f16_fwd_bwd" if f16 else "stonk_softmax_xent_fwd_bwd", logits.data_ptr(), npad,
                 N, npad, tg.data_ptr(), cnt.data_ptr(), loss_sum.data_ptr(), hip.ptr(dl), npad, grad_scale, cap,
                 self.err.data_ptr(), st)
        return dict(rows=rows, tg=tg, cnt=cnt, hs=hs, logits=logits, dl=dl)

    def _pooled_linear(self, name, out, x, B, C):
        """The fp32 linear layer `name` (H -> C: the NSP head, the classifier) on the B pooled rows `x`, into the buffer
        `out` (fp32 [B, C], returned)."""
        H, f = self.cfg.hidden_size, self.P.view
        y = self.buf(out, (B, C), F32)
        hip.call("stonk_small_linear_fwd", x.data_ptr(), H, f(name + ".weight").data_ptr(), f(name + ".bias").data_ptr(),
                 y.data_ptr(), B, C, H, hip.SMALL_X_F32, hip.stream_ptr())
        return y

    def _head_transform(self, pre, seq_out, pooled, L: Rows, save_preact: bool):
        """F4b / F5 on the rows of the sequence output: NSP logits from the pooled vector, then dense + GELU + LayerNorm of
        the prediction head, in buffers named by `pre` ("h": training forward, "ev": `evaluate`). Returns (nsp, what the
        backward reads: dict(gt, ut, t, stt)); `ut` (the saved pre-activation) only with `save_preact`."""
        H, cap_rows, T = self.cfg.hidden_size, L.B * L.S, L.Th
        f, w = self.P.view, self.P.bf16_view
        nsp = self._pooled_linear("cls.seq_relationship", f"{pre}.nsp", pooled, L.B, 2)
        gt = self.buf(f"{pre}.gt", (cap_rows, H))
        ut = self.buf(f"{pre}.ut", (cap_rows, H)) if save_preact else None
        self.gemm(seq_out, w("cls.predictions.transform.dense.weight"), gt, T, H, H,
                  flags=hip.EPI_BIAS | hip.EPI_GELU | (hip.EPI_SAVE_PREACT if save_preact else 0),
                  bias=f("cls.predictions.transform.dense.bias"), aux=ut)
        t = self.buf(f"{pre}.t", (cap_rows, H))
        stt = self.buf(f"{pre}.stt", (2, cap_rows), F32)
        self.ln_fwd(gt, f("cls.predictions.transform.LayerNorm.weight"), f("cls.predictions.transform.LayerNorm.bias"), t, stt, T)
        return nsp, dict(gt=gt, ut=ut, t=t, stt=stt)

    def _loss_tail(self, nsp, nsp_labels, acc, cnts, dnsp, B) -> dict:
        """NSP cross-entropy (+ dlogits into `dnsp` unless None), then the four loss terms from the sums and counts in
        `acc` [text_sum, ent_sum, nsp_sum, nsp_cnt, loss x4] / `cnts`. Returns the loss entries of a forward's result."""
        st = hip.stream_ptr()
        hip.call("stonk_nsp_xent_fwd_bwd", nsp.data_ptr(), nsp_labels.data_ptr(), B, 2, acc[2:4].data_ptr(),
                 hip.ptr(dnsp), 1.0, self.err.data_ptr(), st)
        hip.call("stonk_loss_finalize", acc[0:1].data_ptr(), cnts[0:1].data_ptr(), acc[1:2].data_ptr(),
                 cnts[1:2].data_ptr(), acc[2:4].data_ptr(), acc[4:8].data_ptr(), st)
        return dict(loss=acc[4], masked_lm_loss=acc[5], ent_masked_lm_loss=acc[6], next_sentence_loss=acc[7],
                    loss_terms=acc[4:8])

    def forward(self, input_ids, attention_mask, token_type_ids, mlm_labels, ent_labels, nsp_labels, training: bool,
                dense_logits: bool, need_backward: bool, want_hidden: bool = True):
        """`want_hidden=False` (with labels, without dense logits): nobody will read `hidden_states`, so the trainable
        encoder may run on the packed rows (`Engine.unpad`); `hidden_states` is then None."""
        cfg = self.cfg
        H, S, half = cfg.hidden_size, cfg.max_position_embeddings, cfg.half_length
        B = input_ids.shape[0]
        save: dict = {}
        labels = dict(masked_lm_labels=mlm_labels, ent_masked_lm_labels=ent_labels)
        have_labels = mlm_labels is not None and ent_labels is not None and nsp_labels is not None
        packed = have_labels and not dense_logits and not want_hidden
        seq_out, pooled, L = self.encode(input_ids, attention_mask, token_type_ids, training, save,
                                         (mlm_labels, ent_labels) if packed else None)
        # F5 head transform: dense + GELU, LayerNorm
        nsp, ht = self._head_transform("h", seq_out, pooled, L, True)
        t = ht["t"]
        out = dict(hidden_states=None if L.packed else seq_out.view(B, S, H), pooler_output=pooled, nsp_logits=nsp)
        # F6 label-sparse decoders + fused softmax cross-entropy (value and logits-gradient in one sweep)
        if have_labels:
            acc = self.buf("l.acc", (8,), F32)  # [text_sum, ent_sum, nsp_sum, nsp_cnt, loss x4]
            acc.zero_()
            cnts = self.buf("l.cnt", (2,), I32)
            for hi, dec in enumerate(decoders(cfg)):
                save[dec.name] = self._sparse_head("l", dec, labels[dec.label_key], t, L.head_map, cnts[hi:hi + 1],
                                                   acc[hi:hi + 1], B, need_backward)
            dnsp = self.buf("l.dnsp", (B, 2), F32) if need_backward else None
            out.update(self._loss_tail(nsp, nsp_labels, acc, cnts, dnsp, B))
            save["dnsp"] = dnsp
        # F7 dense logits (what the reference always materialises: stonkgs_model.py:70-71)
        if dense_logits:
            cap = B * half
            full = self.buf("d.cnt", (1,), I32)
            full.fill_(cap)
            for dec in decoders(cfg):
                N, npad = dec.classes, pad128(dec.classes)
                rows = self.buf(f"d.{dec.name}.rows", (cap,), I32)
                rows.copy_((torch.arange(cap, device=self.device, dtype=I32) // half) * S + dec.offset +
                           torch.arange(cap, device=self.device, dtype=I32) % half)
                hs = self.buf("d.hs", (cap, H))
                self._gather_rows(t, rows, full, hs, cap)
                # fresh tensor: handed to the caller, must not alias the workspace
                logits = torch.empty(cap, npad, dtype=F32, device=self.device)
                self.gemm(hs, self.P.bf16_view(dec.weight), logits, cap, npad, H, flags=hip.EPI_OUT_F32)
                out[f"{dec.name}_logits"] = logits[:, :N].view(B, half, N)
        if need_backward:
            save.update(ht)
            self.saved = save
        return out

    # ------------------------------------------------------------------ calls that training must not notice
    @contextlib.contextmanager
    def _detached(self, restore_rows: bool, inputs_only: bool = False):
        """Run the body detached from training: an `encode` in it neither consumes nor queues a frozen-backbone prefetch
        nor advances the dropout counter for good - the prefetched forward, the hint for the next one, `seed_base` and
        (`restore_rows`) `rows_executed` are put back on exit, whether the body returns or raises. The body's inline
        backbone forward shares the prefetch's scratch buffers, so the stream is ordered behind a prefetch in flight.
        `inputs_only`: `_inputs_only` is set for the body."""
        seed_base, prefetch, hint, rows = self.seed_base, self._prefetch, self.next_input_ids, list(self.rows_executed)
        self._prefetch = self.next_input_ids = None
        if prefetch is not None:
            torch.cuda.current_stream().wait_event(prefetch["done"])
        self._inputs_only = inputs_only
        try:
            yield
        finally:
            self._inputs_only = False
            self.seed_base, self._prefetch, self.next_input_ids = seed_base, prefetch, hint
            if restore_rows:
                self.rows_executed[:] = rows

    # ------------------------------------------------------------------ attention maps (forward-only, on request)
    def attention_maps(self, input_ids, attention_mask, token_type_ids, attn_maps: dict):
        """`encode` in the padded layout, eval mode, with the layers named in `attn_maps` writing their attention
        probabilities (see `encode`). Returns the pooled output (a workspace view). Invisible to training as `evaluate`
        is: scratch buffers of its own (save = None), the prefetched frozen-backbone forward, the hint for the next one
        and the dropout counter are as they were; `rows_executed` counts the call."""
        with self._detached(restore_rows=False):
            return self.encode(input_ids, attention_mask, token_type_ids, False, None, None, attn_maps=attn_maps)[1]

    # ------------------------------------------------------------------ evaluation (forward-only, label-sparse)
    def evaluate(self, input_ids, attention_mask, token_type_ids, mlm_labels, ent_labels, nsp_labels, k: int = 10):
        """Held-out evaluation of one batch without dense logits: the training forward's own route - packed encoder rows,
        last layer on labelled rows + position 0, head transform, stonk_label_compact, row gather, label-sparse decoder
        GEMM (`m_dev` = the device-side count) into the SAME logits buffers and dtype training uses - with dropout off,
        the cross-entropy entry called for its loss sums only (null dlogits), and stonk_row_topk_* on the logits it read.
        Returns device tensors only (views of the workspace, valid until the next call; entries at or past a head's
        `count` are unspecified): per head ("text", "ent") `rows` (flat b*S + position), `targets`, `count` [1], `top_idx`
        / `top_val` [cap, k], `lse`, `rank`, `tgt_logit` [cap]; `loss_terms` (total, text, entity, NSP), the four terms by
        name, `nsp_logits`, `nsp_sum_cnt` (sum of the NSP losses, number of NSP labels).
        Invisible to training: `saved`, the prefetched frozen-backbone forward and the hint for the next one, the
        store-mode gradient state, the gradient buffer and the dropout counter are as they were; every buffer a pending
        backward reads is left alone (own head buffers; the logits buffers are not saved for backward)."""
        cfg = self.cfg
        S, half = cfg.max_position_embeddings, cfg.half_length
        B = input_ids.shape[0]
        cap = B * half
        st = hip.stream_ptr()
        labels = dict(masked_lm_labels=mlm_labels, ent_masked_lm_labels=ent_labels)
        with self._detached(restore_rows=True):
            seq_out, pooled, L = self.encode(input_ids, attention_mask, token_type_ids, False, None,
                                             (mlm_labels, ent_labels))
        nsp, ht = self._head_transform("ev", seq_out, pooled, L, False)
        acc = self.buf("ev.acc", (8,), F32)   # [text_sum, ent_sum, nsp_sum, nsp_cnt, loss x4]
        acc.zero_()
        cnts = self.buf("ev.cnt", (2,), I32)
        out = dict(nsp_logits=nsp)
        f16 = self.f16_logits
        for hi, dec in enumerate(decoders(cfg)):
            nm, N, npad = dec.name, dec.classes, pad128(dec.classes)
            h = self._sparse_head("ev", dec, labels[dec.label_key], ht["t"], L.head_map, cnts[hi:hi + 1], acc[hi:hi + 1], B,
                                  False)
            tg, cnt = h["tg"], h["cnt"]
            # the caller wants flat positions b*S + off + p; in the packed layout the compaction above produced rows of the
            # sequence output instead (what the gather reads), so it runs once more without the map: one workgroup, ~20 us
            pos = h["rows"]
            if L.packed:
                pos = self.buf(f"ev.{nm}.pos", (cap,), I32)
                hip.call("stonk_label_compact", labels[dec.label_key].data_ptr(), cap, half, S, dec.offset, pos.data_ptr(),
                         tg.data_ptr(), cnt.data_ptr(), 0, st)
            top_val = self.buf(f"ev.{nm}.top_val", (cap, k), F32)
            top_idx = self.buf(f"ev.{nm}.top_idx", (cap, k), I32)
            lse = self.buf(f"ev.{nm}.lse", (cap,), F32)
            rank = self.buf(f"ev.{nm}.rank", (cap,), I32)
            tl = self.buf(f"ev.{nm}.tgt_logit", (cap,), F32)
            hip.call("stonk_row_topk_f16" if f16 else "stonk_row_topk_f32", h["logits"].data_ptr(), npad, N, tg.data_ptr(),
                     cnt.data_ptr(), cap, k, top_val.data_ptr(), top_idx.data_ptr(), lse.data_ptr(), rank.data_ptr(),
                     tl.data_ptr(), st)
            out[nm] = dict(rows=pos, targets=tg, count=cnt, top_idx=top_idx, top_val=top_val, lse=lse, rank=rank,
                           tgt_logit=tl)
        out.update(self._loss_tail(nsp, nsp_labels, acc, cnts, None, B), nsp_sum_cnt=acc[2:4])
        return out

    # ------------------------------------------------------------------ input gradients (inputs-only backward)
    def input_gradients(self, input_ids, attention_mask, token_type_ids, grad_x_input, grad_norm, grad_out=None, *,
                        num_labels: Optional[int] = None, target=None, labels: Optional[dict] = None):
        """d F / d inputs_embeds per position, reduced by stonk_input_attribution into `grad_x_input` / `grad_norm` (fp32
        [B, S], either may be None) and written out as `grad_out` (fp32 [B, S, H]) when given. Dropout is off. The forward is
        the training forward (packed rows of `Engine.unpad`, last layer on the read rows, activations saved); the backward is
        the training backward's own chain under `_inputs_only`: no weight gradient is computed and the gradient buffer is
        not touched.
          classification model (`num_labels`): F_b = logits[b, target_b]; `target` None = the predicted class (one host
            sync), else int64 [B] on the device. Returns dict(logits, target).
          pre-training model (`labels`: masked_lm_labels / ent_masked_lm_labels / next_sentence_labels, any non-empty
            subset): F = sum of log p(label) over the given labels; a head without labels is not run. One host sync for the
            label counts. Returns dict(score).
        Returned tensors are workspace views. Between steps the call leaves no trace: the prefetched frozen-backbone
        forward, the hint for the next one, the dropout counter, `rows_executed`, the store-mode gradient state, the
        gradient buffer and the parameters are as they were. It uses the training forward's activation buffers, so it refuses
        to run while a forward is waiting for its backward."""
        if self.saved is not None:
            raise RuntimeError("input_gradients() while a training forward is waiting for its backward: the call uses that "
                               "forward's activation buffers - run the backward first")
        cfg = self.cfg
        H, S, half = cfg.hidden_size, cfg.max_position_embeddings, cfg.half_length
        B = input_ids.shape[0]
        st = hip.stream_ptr()
        counts = {}
        if num_labels is None:
            given = {k: v for k, v in (labels or {}).items() if v is not None}
            if not given:
                raise ValueError("labels: give at least one of masked_lm_labels, ent_masked_lm_labels, next_sentence_labels")
            n = torch.stack([(v != -100).sum() for v in given.values()]).tolist()   # (the host sync)
            counts = {k: c for k, c in zip(given, n) if c > 0}
            if not counts:
                raise ValueError("labels: every given label is -100 - there is no prediction to attribute")
            # per decoder: its labels, or None for a head that is not run
            dec_labels = [given[d.label_key] if d.label_key in counts else None for d in decoders(cfg)]
        with self._detached(restore_rows=True, inputs_only=True):
            save: dict = {}
            out: dict = {}
            # (encode orders the stream behind the optimizer's last parameter write before it reads a trainable weight)
            if num_labels is not None:
                _, pooled, L = self.encode(input_ids, attention_mask, token_type_ids, False, save, (None, None))
                logits = self._pooled_linear("classifier", "ia.logits", pooled, B, num_labels)
                if target is None:
                    target = logits.argmax(dim=1)
                dl = self.buf("ia.dl", (B, num_labels), F32)
                dl.zero_()
                dl.scatter_(1, target.view(B, 1), 1.0)
                dpooled = self._pooled_linear_bwd("classifier", dl, pooled, B, num_labels)
                dseq = self._zero_rows("b.dseq", L)   # only position 0 of a sequence receives a gradient (from the pooler)
                out.update(logits=logits, target=target)
            else:
                seq_out, pooled, L = self.encode(input_ids, attention_mask, token_type_ids, False, save, tuple(dec_labels))
                if any(lab is not None for lab in dec_labels):
                    nsp, ht = self._head_transform("h", seq_out, pooled, L, True)
                    save.update(ht)
                    t = ht["t"]
                else:   # NSP labels alone: no decoder runs, so neither does the head transform
                    t = None
                    nsp = self._pooled_linear("cls.seq_relationship", "h.nsp", pooled, B, 2)
                acc = self.buf("l.acc", (8,), F32)   # [text_sum, ent_sum, nsp_sum, nsp_cnt, -]
                acc.zero_()
                cnts = self.buf("l.cnt", (2,), I32)
                heads = []
                for hi, (dec, lab) in enumerate(zip(decoders(cfg), dec_labels)):
                    if lab is None:
                        continue
                    # (softmax - onehot) * grad_scale / count with grad_scale = -count: onehot - softmax, d log p / d logits
                    h = self._sparse_head("l", dec, lab, t, L.head_map, cnts[hi:hi + 1], acc[hi:hi + 1], B, True,
                                          grad_scale=-float(counts[dec.label_key]))
                    heads.append((dec, h))
                dnsp = None
                if "next_sentence_labels" in counts:
                    dnsp = self.buf("l.dnsp", (B, 2), F32)
                    hip.call("stonk_nsp_xent_fwd_bwd", nsp.data_ptr(), given["next_sentence_labels"].data_ptr(), B, 2,
                             acc[2:4].data_ptr(), dnsp.data_ptr(), -float(counts["next_sentence_labels"]),
                             self.err.data_ptr(), st)
                # the backward: the training chain's pieces with the default split-K decoder dgrad; without a decoder
                # d(sequence_output) is zero, without NSP labels so is d(pooled)
                if heads:
                    dt = self._zero_rows("b.dt", L)
                    for dec, h in heads:
                        self._decoder_dgrad(dec, h, dt, B, B * half)
                    dseq = self._head_transform_bwd(save, dt)
                else:
                    dseq = self._zero_rows("b.dseq", L)
                if dnsp is not None:
                    dpooled = self._pooled_linear_bwd("cls.seq_relationship", dnsp, pooled, B, 2)
                else:
                    dpooled = self.buf("b.dpooled", (B, H), F32)
                    dpooled.zero_()
                out.update(score=-acc[0:3].sum())
            dsum = self.backward_encoder(dpooled, dseq, save, None)
            hip.call("stonk_input_attribution", dsum.data_ptr(), dsum.stride(0), input_ids.data_ptr(),
                     save["text_hidden"].data_ptr(), self.kg_table.data_ptr(), self.kg_table.shape[0],
                     hip.ptr(L.row_of_pos), 1.0, hip.ptr(grad_x_input), hip.ptr(grad_norm), hip.ptr(grad_out), H, B, S, half,
                     H, st)
        return out

    # ------------------------------------------------------------------ backward
    def _zero_rows(self, name, L: Rows):
        """The [B * S, H] gradient buffer `name` with the rows of the sequence output cleared."""
        x = self.buf(name, (L.B * L.S, self.cfg.hidden_size))
        x[:L.Th].zero_()
        return x

    def _decoder_dgrad(self, dec: Decoder, h, dt, B, clear_rows, alpha: float = 1.0, wave8: bool = False) -> None:
        """One decoder's dHs = alpha * dlogits . W over the device-side count of `h` (`_sparse_head`), scattered into the
        head transform's output gradient `dt`. Few output tiles (count/128 x H/128), very long contraction (the
        vocabulary): split-K into fp32, whose first `clear_rows` rows are cleared. `wave8`: the persistent 256x256 kernel
        with 8 splits instead of 128x128 tiles with up to 16 - the caller's choice."""
        H, cap, npad = self.cfg.hidden_size, B * self.cfg.half_length, pad128(dec.classes)
        dhs = self.buf("b.dhs32", (cap, H), F32)
        dhs[:clear_rows].zero_()
        if wave8:
            self.gemm(h["dl"], self.P.wt[dec.weight], dhs, cap, H, npad, flags=hip.EPI_OUT_F32_ATOMIC, split_k=8,
                      m_dev=h["cnt"], alpha=alpha, kernel=hip.GEMM_WAVE8)
        else:
            self.gemm(h["dl"], self.P.wt[dec.weight], dhs, cap, H, npad, flags=hip.EPI_OUT_F32_ATOMIC,
                      split_k=max(1, min(16, npad // 2048)), m_dev=h["cnt"], alpha=alpha)
        hip.call("stonk_scatter_rows_f32_to_bf16", dhs.data_ptr(), H, h["rows"].data_ptr(), h["cnt"].data_ptr(),
                 dt.data_ptr(), H, H, hip.stream_ptr())

    def _head_transform_bwd(self, sv, dt):
        """LayerNorm and GELU backward of the head transform, its weight gradients, and the dgrad into d(sequence_output)
        (the "b.dseq" buffer, returned)."""
        H = self.cfg.hidden_size
        L = sv["layout"]
        T, cap_rows = L.Th, L.B * L.S
        f, g_ = self.P.view, self.P.grad_view
        dgt = self.buf("b.dgt", (cap_rows, H))
        self.ln_bwd(dt, sv["gt"], sv["stt"][0], sv["stt"][1], f("cls.predictions.transform.LayerNorm.weight"), dgt, None,
                    g_("cls.predictions.transform.LayerNorm.weight"), g_("cls.predictions.transform.LayerNorm.bias"), T, H, 0,
                    0.0, 0, 0.0, 0)
        dut = self.buf("b.dut", (cap_rows, H))
        hip.call("stonk_gelu_bwd_bf16", dgt.data_ptr(), sv["ut"].data_ptr(), dut.data_ptr(), T * H, hip.stream_ptr())
        self.wgrad(dut, sv["seq_out"], g_("cls.predictions.transform.dense.weight"),
                   g_("cls.predictions.transform.dense.bias"), H, H, T)
        dseq = self.buf("b.dseq", (cap_rows, H))
        self.gemm(dut, self.P.wt["cls.predictions.transform.dense.weight"], dseq, T, H, H,
                  kernel=self._kernel("dgrad_head", True))
        return dseq

    def _pooled_linear_bwd(self, name, dy, x, B, C):
        """Backward of `_pooled_linear`: the layer's weight gradients, and d(x) (the "b.dpooled" buffer, returned)."""
        H = self.cfg.hidden_size
        dpooled = self.buf("b.dpooled", (B, H), F32)
        dW, db = self._small_wgrad(name, C, H)
        hip.call("stonk_small_linear_bwd", dy.data_ptr(), 0, x.data_ptr(), H, self.P.view(name + ".weight").data_ptr(),
                 dW.data_ptr(), db.data_ptr(), dpooled.data_ptr(), 0, 0, B, C, H, hip.SMALL_X_F32, hip.stream_ptr())
        return dpooled

    def backward(self, gscale: float = 1.0, on_segment_done: Optional[Callable[[str], None]] = None) -> None:
        """Accumulate d(loss * gscale)/d(param) into the flat gradient buffer. `on_segment_done(name)` fires as
        soon as the gradients of a contiguous region of the flat buffer are final (DP all-reduce overlap)."""
        sv = self.saved
        if sv is None:
            raise RuntimeError("backward() without a training forward (labels are required)")
        self.saved = None
        cfg = self.cfg
        H = cfg.hidden_size
        L = sv["layout"]
        B = L.B
        cap = B * cfg.half_length
        notify = self._make_notify(on_segment_done)
        # ---- decoders (label-sparse): dHs = dlogits . W ; dW += dlogits^T . Hs
        dt = self._zero_rows("b.dt", L)
        # (labelled rows of a head <= read rows, known to the host in the packed layout: the split-K atomics and the
        # scatter touch no row of dHs beyond them)
        clear = cap if L.rd is None else min(cap, (L.rd.n + 255) // 256 * 256)
        for dec in reversed(decoders(cfg)):
            npad, h = pad128(dec.classes), sv[dec.name]
            # the persistent 256x256 kernel with 8 splits (<= 30 live tiles x 8 = one round of the CUs) against 128x128
            # tiles with 16: 734 us against 951 for the entity decoder (tools/bench_decoder_dgrad.py)
            # (not beside a running all-reduce - the entity decoder's bucket is in flight when the text decoder's dgrad is
            # launched: a persistent launch would wait for the CUs RCCL holds, tools/hog_test.py)
            # (the written-out four-wave kernel on 256x192 tiles is the slower one here: DESIGN.md section 4.3)
            wave8 = npad >= 16384 and cap >= 1024 and H % 256 == 0 and not (self.comm_overlap and dec.name != "ent")
            self._decoder_dgrad(dec, h, dt, B, clear, alpha=gscale, wave8=wave8)
            self.wgrad(h["dl"], h["hs"], self.P.grad_view(dec.weight, padded=True), None, npad, H, cap, k_dev=h["cnt"],
                       alpha=gscale, name=dec.weight)
            notify(dec.weight)
        # ---- head transform backward
        dseq = self._head_transform_bwd(sv, dt)
        # ---- NSP + pooler (fp32), pooler gradient lands on position 0 of d(sequence_output)
        dnsp = sv["dnsp"]
        if gscale != 1.0:
            hip.call("stonk_scale_f32", dnsp.data_ptr(), dnsp.numel(), gscale, hip.stream_ptr())
        dpooled = self._pooled_linear_bwd("cls.seq_relationship", dnsp, sv["pooled"], B, 2)
        self.backward_encoder(dpooled, dseq, sv, notify)

    def backward_encoder(self, dpooled, dseq, sv, notify):
        """Pooler (tanh) backward into position 0 of d(sequence_output), encoder layers last to first, embeddings.
        Returns `dsum`, the gradient of the embedding sum (bf16, the forward's row layout; a workspace view)."""
        if self._inputs_only:
            notify = lambda name: None   # noqa: E731
        cfg = self.cfg
        H, S = cfg.hidden_size, cfg.max_position_embeddings
        L = sv["layout"]
        B, T = L.B, L.T
        cap = B * S
        st = hip.stream_ptr()
        f, g_ = self.P.view, self.P.grad_view
        if not L.packed:
            acc, ld_acc = dseq, S * H
        else:   # packed: position 0 of sequence b is row first_rows[b] - its gradient rows are gathered, added to, scattered back
            nb = self.buf("e.nb", (1,), I32)
            nb.fill_(B)
            acc, ld_acc = self.buf("b.dfirst", ((B + 127) // 128 * 128, H)), H
            self._gather_rows(dseq, L.first_rows, nb, acc, acc.shape[0])
        dWp, dbp = self._small_wgrad("bert.pooler.dense", H, H)
        hip.call("stonk_small_linear_bwd", dpooled.data_ptr(), sv["pooled"].data_ptr(), sv["first"].data_ptr(),
                 sv["ld_first"], f("bert.pooler.dense.weight").data_ptr(), dWp.data_ptr(), dbp.data_ptr(), 0,
                 acc.data_ptr(), ld_acc, B, H, H, hip.SMALL_TANH, st)
        if L.packed:
            hip.call("stonk_scatter_rows_bf16", acc.data_ptr(), H, L.first_rows.data_ptr(), nb.data_ptr(), dseq.data_ptr(),
                     H, H, st)
        notify("bert.pooler.dense.bias")
        # ---- encoder layers, last to first
        dy = dseq
        last = cfg.num_hidden_layers - 1
        if L.packed and L.rows < T:   # what an earlier step left in the rows no sequence owns must not reach dW
            for par in (0, 1):
                self.buf(f"b.dqkv.{par}", (cap, 3 * H))[L.rows:T].zero_()
        span = self._span_begin()
        for i in reversed(range(cfg.num_hidden_layers)):
            prefix = f"bert.encoder.layer.{i}"
            with self.block(f"K15 encoder layer {i} bwd"):
                dy = self.layer_bwd(prefix, dy, L, sv["p_hid"], sv["p_att"], i, sv[prefix], last=i == last)
            notify(prefix)
        if span is not None and self._wstream is not None:   # (timing only) the span ends when the layers' weight gradients have
            torch.cuda.current_stream().wait_stream(self._wstream)
        self._span_end("encoder_bwd", span)
        # ---- embeddings LayerNorm, position / token-type embeddings
        dsum = self.buf("b.dsum0", (cap, H))
        p_hid = sv["p_hid"]
        self.ln_bwd(dy, sv["sum0"], sv["st0"][0], sv["st0"][1], f("bert.embeddings.LayerNorm.weight"), dsum, None,
                    g_("bert.embeddings.LayerNorm.weight"), g_("bert.embeddings.LayerNorm.bias"), T, H,
                    hip.LN_DROPOUT if p_hid > 0 else 0, p_hid, self.seed(200, 0), 0.0, 0)
        if not self._inputs_only:
            hip.call("stonk_embed_grad", dsum.data_ptr(), hip.ptr(sv["token_type_ids"]),
                     g_("bert.embeddings.position_embeddings.weight").data_ptr(),
                     g_("bert.embeddings.token_type_embeddings.weight").data_ptr(), B, S, H, cfg.type_vocab_size,
                     hip.ptr(L.row_of_pos), st)
            self._word_embed_grad(dsum, sv)
        notify("bert.embeddings")
        self.mark("backward_end")
        self.join_wgrad()
        return dsum

    def _word_embed_grad(self, dsum, sv) -> None:
        """Gradient of the looked-up input rows, where they are trainable (`TextEngine`); STonKGs' entity table and its
        frozen backbone are not."""

    # ------------------------------------------------------------------ sequence classification head (config 5)
    def forward_cls(self, input_ids, attention_mask, token_type_ids, labels, num_labels: int, training: bool,
                    need_backward: bool, loss_mode: Optional[int] = None):
        """pooled -> dropout -> Linear(H, num_labels) -> loss (ref:stonkgs_finetuning.py:310-338). `loss_mode` None:
        CrossEntropyLoss on int64 labels [B]; hip.LOSS_MSE / LOSS_MSE_BROADCAST / LOSS_BCE: the regression and
        multi-label branches on fp32 labels."""
        cfg = self.cfg
        H = cfg.hidden_size
        B = input_ids.shape[0]
        st = hip.stream_ptr()
        save: dict = {}
        # (the classification head hands out no per-position output: the encoder runs on the packed rows, training or not)
        seq_out, pooled, L = self.encode(input_ids, attention_mask, token_type_ids, training, save, (None, None))
        p = cfg.hidden_dropout_prob if training else 0.0
        dropped = pooled
        if p > 0:
            dropped = self.buf("c.dropped", (B, H), F32)
            hip.call("stonk_dropout_f32", pooled.data_ptr(), dropped.data_ptr(), B * H, p, self.seed(300, 0), st)
        logits = self._pooled_linear("classifier", "c.logits", dropped, B, num_labels)
        out = dict(logits=logits, pooler_output=pooled,
                   hidden_states=None if L.packed else seq_out.view(B, cfg.max_position_embeddings, H))
        if labels is not None:
            dl = self.buf("c.dl", (B, num_labels), F32) if need_backward else None
            loss = self.buf("c.loss", (1,), F32)
            if loss_mode is None:
                acc = self.buf("c.acc", (2,), F32)
                acc.zero_()
                hip.call("stonk_nsp_xent_fwd_bwd", logits.data_ptr(), labels.data_ptr(), B, num_labels, acc.data_ptr(),
                         hip.ptr(dl), 1.0, self.err.data_ptr(), st)
                hip.call("stonk_ratio_f32", acc[0:1].data_ptr(), acc[1:2].data_ptr(), loss.data_ptr(), st)
            else:
                hip.call("stonk_elementwise_loss_fwd_bwd", logits.data_ptr(), labels.data_ptr(), B, num_labels, loss_mode,
                         loss.data_ptr(), hip.ptr(dl), 1.0, st)
            out["loss"] = loss[0]
            if need_backward:
                save.update(dl=dl, dropped=dropped, p_cls=p, num_labels=num_labels)
                self.saved = save
        return out

    def backward_cls(self, gscale: float = 1.0, on_segment_done: Optional[Callable[[str], None]] = None) -> None:
        sv = self.saved
        if sv is None:
            raise RuntimeError("backward_cls() without a training forward (labels are required)")
        self.saved = None
        L = sv["layout"]
        B, H = L.B, self.cfg.hidden_size
        st = hip.stream_ptr()
        notify = self._make_notify(on_segment_done)
        dl = sv["dl"]
        if gscale != 1.0:
            hip.call("stonk_scale_f32", dl.data_ptr(), dl.numel(), gscale, st)
        dpooled = self._pooled_linear_bwd("classifier", dl, sv["dropped"], B, sv["num_labels"])
        if sv["p_cls"] > 0:  # same (seed, index) mask as the forward
            hip.call("stonk_dropout_f32", dpooled.data_ptr(), dpooled.data_ptr(), B * H, sv["p_cls"], self.seed(300, 0), st)
        notify("classifier.bias")
        dseq = self._zero_rows("b.dseq", L)  # only position 0 of every sequence receives a gradient (from the pooler)
        self.backward_encoder(dpooled, dseq, sv, notify)


TEXT_ERR_BITS = {**ERR_BITS, 1: "token id outside [0, vocab_size)", 16: "class label outside [0, num_labels)"}


class TextEngine(Engine):
    """Text-only front and tail for a plain BERT classifier (the NLP baseline, ref:src/stonkgs/models/nlp_baseline_model.py):
    the input is token ids alone. No frozen backbone, no entity table, no special vectors - every position's input row is a
    lookup in the TRAINABLE word table `bert.embeddings.word_embeddings.weight`, which stonk_joint_embed_ln_fwd reads as its
    table with half = 0 (word + position + token-type -> LayerNorm -> dropout, packed layout included) and whose gradient
    stonk_word_embed_grad adds behind stonk_embed_grad, before the "bert.embeddings" notification: the table is the last
    segment of the flat buffer. Encoder layers, pooler, `forward_cls` / `backward_cls` and the optimizer tables are the
    base class's. Only the gather reads the table: it has no W^T copy, and its bf16 mirror is never read."""

    WORD = "bert.embeddings.word_embeddings.weight"
    ERR_BITS = TEXT_ERR_BITS
    KEY_ERROR_BITS = 0   # an out-of-range token id is an IndexError: what torch's embedding raises
    PADDING_IDX = 0  # BertEmbeddings: nn.Embedding(vocab_size, hidden_size, padding_idx=config.pad_token_id = 0)

    def __init__(self, cfg: STonKGsConfig, store: FlatStore, device):
        super().__init__(cfg, store, None, 0, device)
        self.kg_table = store.view(self.WORD)   # fp32 [vocab, H]: a view of the master, so it is always current

    def _mirrored_stores(self) -> tuple:
        return (self.P,)   # (no backbone store)

    @property
    def half_length(self) -> int:
        return 0

    def _text_half(self, input_ids, B, training: bool):
        """Nothing runs ahead of the embeddings kernel; with half = 0 it reads no text row (the pointer must be non-null)."""
        self.next_input_ids = None
        return self.kg_table, None

    def _word_embed_grad(self, dsum, sv) -> None:
        cfg, L = self.cfg, sv["layout"]
        dword = self.P.grad_view(self.WORD)
        hip.call("stonk_word_embed_grad", dsum.data_ptr(), dsum.stride(0), sv["input_ids"].data_ptr(),
                 hip.ptr(L.row_of_pos), dword.data_ptr(), dword.stride(0), cfg.vocab_size, self.PADDING_IDX, L.B,
                 cfg.max_position_embeddings, cfg.hidden_size, self.err.data_ptr(), hip.stream_ptr())
