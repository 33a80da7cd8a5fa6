"""HIP execution engine for the STonKGs hot path: schedules the C-ABI kernels (include/stonk_hip.h) for
forward, backward and the derived-weight refresh.  No torch arithmetic on the data path: torch tensors are
device memory, ``torch.cuda.current_stream()`` is the stream every launcher is given.

Call structure mirrors SURVEY.md section 3.2 (ref:src/stonkgs/models/stonkgs_model.py:149-258):
  F1 frozen LM backbone on the text half  ->  F2 KG gather + concat + embeddings LayerNorm  ->  F3 encoder layers
  ->  F4 pooler / NSP  ->  F5 head transform  ->  F6 label-sparse decoders + fused cross-entropy
and the mirrored backward.  Activations needed by backward are kept in a persistent workspace (HBM is 288 GB;
B=64 needs ~12 GB), nothing is recomputed except attention probabilities.
"""
from __future__ import annotations

import collections
import contextlib
import dataclasses
import math
import os
import struct
import time
from typing import Callable, Dict, Optional

import torch

from . import _hip as hip
from .config import STonKGsConfig
from .params import FlatStore, pad128

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32

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


@dataclasses.dataclass(frozen=True)
class ReadRows:
    """The READ rows of the packed layout (labelled positions + position 0), on which the last encoder layer's
    feed-forward block, the pooler and the head transform run (`Engine.prune_last_ffn`)."""
    rows: torch.Tensor      # int32: packed row of every read row
    cnt: torch.Tensor       # int32 [1]: their number, on the device ...
    n: int                  # ... and on the host
    offsets: torch.Tensor   # int32 [B + 1]: a sequence's read rows (its FIRST packed rows) among all read rows
    T: int                  # n rounded up to 64
    attn: bool              # the last layer's attention computes them alone as queries (`Engine.prune_last_attn`)


@dataclasses.dataclass(frozen=True)
class Rows:
    """What one step knows about its rows. Padded layout: every position is a row, T = rows = B * S, `mask` = the
    attention mask [B, S] (or None). Packed layout (csrc/unpad.hip, `Engine.unpad`): `cu` = sequence offsets, `mask` = one
    word per row, the three maps of the row plan, and `rd` where the last layer runs on the read rows only."""
    B: int
    S: int
    T: int                  # rows the layers run on (packed: the packed row count rounded up to 64)
    rows: int               # rows that belong to a sequence
    mask: Optional[torch.Tensor]
    cu: Optional[torch.Tensor] = None
    row_of_pos: Optional[torch.Tensor] = None
    pos_of_row: Optional[torch.Tensor] = None
    read_of_pos: Optional[torch.Tensor] = None
    rd: Optional[ReadRows] = None

    @property
    def packed(self) -> bool:
        return self.cu is not None

    @property
    def Th(self) -> int:
        """Rows of the sequence output (and of everything the heads run on)."""
        return self.T if self.rd is None else self.rd.T

    @property
    def first_rows(self) -> Optional[torch.Tensor]:
        """Packed: row of position 0 of every sequence in the sequence output."""
        return self.cu if self.rd is None else self.rd.offsets

    @property
    def head_map(self) -> Optional[torch.Tensor]:
        """Packed: position -> row of the sequence output."""
        return self.row_of_pos if self.rd is None else self.read_of_pos


def padded_rows(B: int, S: int, mask) -> Rows:
    return Rows(B, S, B * S, B * S, mask)


class GemmTimer:
    """Optional per-launch HIP-event timing of the GEMM kernel (bench.py roofline leg)."""

    def __init__(self):
        self.records = []  # (kind, start_event, end_event, M, N, K, m_dev, k_dev)
        self.spans = {}    # name -> [(start_event, end_event)]: stream-order spans (the encoder's forward / backward)

    def kinds(self):
        return sorted({r[0] for r in self.records})

    def span_seconds(self, name) -> float:
        torch.cuda.synchronize()
        return sum(s.elapsed_time(e) for s, e in self.spans.get(name, [])) * 1e-3

    def summarize(self, kind=None):
        """Algorithmic FLOPs use the rows / contraction length that exist at run time (device-side counts of the
        label-sparse decoders), not the launch capacity. kind: "tn_a4" / "tn" (weight-gradient kernels: four-wave 256x256, written-out loop /
        128x128), "nt", or None = all."""
        torch.cuda.synchronize()
        tot_t = tot_f = 0.0
        n = 0
        for k, s, e, M, N, K, m_dev, k_dev in self.records:
            if kind is not None and k != kind:
                continue
            n += 1
            tot_t += s.elapsed_time(e) * 1e-3
            if m_dev is not None:
                M = min(M, int(m_dev.item()))
            if k_dev is not None:
                K = min(K, int(k_dev.item()))
            tot_f += 2.0 * M * N * K
        return {"launches": n, "seconds": tot_t, "flops": tot_f}


class Engine:
    ERR_BITS = ERR_BITS      # what check_errors says for each bit of the kernels' error word ...
    KEY_ERROR_BITS = 1       # ... and which of them make it a KeyError instead of an IndexError

    def __init__(self, cfg: STonKGsConfig, store: FlatStore, backbone: FlatStore, n_backbone_layers: int, device):
        cfg.validate_for_hip()
        hip.lib()  # fail loudly, now, if the extension is missing
        self.cfg = cfg
        self.P = store
        self.BB = backbone
        self.n_bb = n_backbone_layers
        self.device = device
        self.ws: Dict[str, torch.Tensor] = {}
        self.kg_table: Optional[torch.Tensor] = None  # fp32 [K+3, H]
        self.err = torch.zeros(1, dtype=I32, device=device)
        self.gemm_timer: Optional[GemmTimer] = None
        self.saved = None
        self.seed_base = 0x5710
        # Weight-gradient GEMMs are off the critical path of backward (nothing downstream reads dW until the optimizer):
        # they are launched on a second HIP stream and overlap the dgrad / LayerNorm / attention chain on the main one.
        self.overlap_wgrad = True
        # Set by the trainer when gradients are all-reduced while backward runs (world size > 1): RCCL's kernels then hold
        # some CUs for the length of a collective, and a PERSISTENT one-workgroup-per-CU kernel with a static tile split
        # would wait for them (its late workgroups own a share of the tiles). Backward's persistent launches on the main
        # stream (the dgrad GEMMs of every layer, `_kernel(site, True)`) are then launched STONK_GEMM_DISPATCHED2: the
        # same four-wave kernel with two work items per workgroup, so the hardware dispatcher hands out the tiles and
        # every second tile boundary keeps its prefetch (what it costs with nothing beside it: DESIGN.md section 6).
        self.comm_overlap = False
        # Which of the library's three NT kernels runs a launch is the LIBRARY's choice (STONK_GEMM_AUTO: from shape and
        # epilogue, stonk_gemm_nt_bf16) - except where the engine knows what the library cannot: that an all-reduce is
        # running beside backward (comm_overlap -> the dispatcher-scheduled form for the persistent launches).
        # `kernel_for` lets a tool pin a site for an A/B (tools/ab_step.py): "qkv", "attn_out", "ffn_up", "ffn_down",
        # "dgrad_gelu", "dgrad_resid", "dgrad_attn_out", "dgrad_head" -> hip.GEMM_*.
        self.kernel_for: Dict[str, int] = {}
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
        self._wstream: Optional[torch.cuda.Stream] = None
        # The optimizer (grad-norm, AdamW, W^T refresh: ~2 ms of HBM-bound work) runs on a third stream; the next step's
        # frozen-backbone forward reads none of what it writes and starts beside it. `wait_params()` orders the current
        # stream after the last parameter write - called before the first trainable weight is read and by every accessor.
        self._opt_stream: Optional[torch.cuda.Stream] = None
        self._params_ready: Optional[torch.cuda.Event] = None
        # tools/step_marks.py: a list to collect (name, host time, event on the current stream, was the optimizer's
        # "parameters final" event already complete) at a few points of the step; None (default) = nothing is recorded
        self.marks: Optional[list] = None
        self._wgrad_done: Dict[int, torch.cuda.Event] = {}   # layer parity -> side-stream event after its last wgrad
        self._wt_desc = None   # (device table, entries, tiles) of the batched W^T refresh
        self._adamw_tables = None   # device tables of stonk_adamw_step_tiled (adamw_tables())
        # Store-mode weight gradients (stonk_gemm_tn_bf16_store). `store_names`: the weights whose unsplit gradient GEMM may
        # WRITE its result - set by a trainer whose optimizer then leaves those spans unzeroed; `store_first`: this backward is
        # the first contribution of the optimizer step (first micro-batch); `grad_stale`: spans that still hold the previous
        # step's gradient - a launch that cannot store (the routing splits K at this shape) zeroes its span first.
        self.store_names: tuple = ()
        self.store_first = False
        self.grad_stale: set = set()
        self.store_log = collections.deque(maxlen=64)   # (name, status) of the latest store-mode attempts (tests, debugging)
        # Sums of squares from the store epilogue (stonk_gemm_tn_bf16_store_sumsq): while `store_sumsq`
        # is set (by a trainer whose gradient norm is the norm of ONE backward on ONE rank) a store launch also leaves its
        # output tiles' sums of squares in its region of one slot buffer, and the gradient-norm pass need not read that
        # gradient back. `sumsq_valid`: the weights whose slots are THIS step's - set by the store launch that returned OK,
        # dropped by any other launch into the same gradient and when the optimizer has taken them (`take_wgrad_sumsq`).
        # `norm_from_epilogue` = False: store launches never write slots (the norm reads the whole buffer, as it did).
        self.norm_from_epilogue = True
        self.store_sumsq = False
        self.sumsq_valid: set = set()
        self._sumsq_tiles: Dict[str, int] = {}
        self._sumsq_buf: Optional[torch.Tensor] = None
        # Inputs-only backward (`input_gradients` alone sets it, through `_detached`): the chain of dgrad GEMMs, LayerNorm and attention
        # backward runs down to d(embedding sum) and nothing is written to the gradient buffer - `wgrad` returns at once,
        # `ln_bwd` passes null dgamma / dbeta, the small linear layers' weight gradients go to scratch, stonk_embed_grad
        # and the `notify` hooks are skipped. False: every path issues exactly the launches it issued before the flag.
        self._inputs_only = False
        self.tn_cus = 160         # CU share of the side-stream weight gradients (tools/sweep_engine_int.py)
        # Weight gradients of a layer that leave as ONE launch of the grouped kernel (stonk_gemm_tn_bf16_group), the earlier
        # one held until the later one's operands are ready: "attn" = attention output + fused QKV, "ffn" = FFN down + FFN
        # up. Together they fill the CU share with fewer K splits each: half the float-atomic bytes, one launch
        # (DESIGN.md section 4.3). "attn" is 0.24 ms of the step; "ffn" measured 0.01 ms on top of it and is off
        # (profiles/wgrad_groups.md).
        self.wgrad_groups: frozenset = frozenset({"attn"})
        self.group_log = collections.deque(maxlen=64)   # (members, status) of the latest grouped launches (tests, debugging)
        # roctx ranges around the blocks of SURVEY section 2.3 (K1 backbone ... K16 optimizer), so that a
        # `rocprofv3 --marker-trace --kernel-trace` timeline reads by block. Off unless STONK_ROCTX=1 (read once, here).
        self.roctx = bool(os.environ.get("STONK_ROCTX"))
        self.tn_min_k = 16384     # contraction length (rows) from which the four-wave kernel takes a weight gradient
        self.tn_min_tiles = 36    # 128x128 tiles of an output from which the four-wave kernel takes the gradient: 36 = the
                                  # 768 x 768 ones too (35.67 against 35.79 ms per step with 100, tools/sweep_engine_int.py)

    # ------------------------------------------------------------------ plumbing
    def buf(self, name: str, shape, dtype=BF16, zero=False) -> torch.Tensor:
        n = 1
        for d in shape:
            n *= d
        t = self.ws.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = (torch.zeros if zero else torch.empty)(max(n, 1), dtype=dtype, device=self.device)
            self.ws[name] = t
        return t[:n].view(shape)

    @contextlib.contextmanager
    def optimizer_stream(self, enabled: bool = True):
        """Run the body on the optimizer stream, ordered after everything enqueued so far on the current stream; on
        exit the engine remembers the event that marks the parameters as final (see `wait_params`)."""
        if not enabled:
            yield
            return
        with self._fork("_opt_stream") as stream:
            yield
            ev = torch.cuda.Event()
            ev.record(stream)
        self._params_ready = ev

    @contextlib.contextmanager
    def _fork(self, attr: str):
        """Run the body on the side stream kept in `self.<attr>` (created on first use), ordered after everything enqueued
        so far on the current stream. Yields the side stream."""
        side = getattr(self, attr)
        if side is None:
            side = torch.cuda.Stream(device=self.device)
            setattr(self, attr, side)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            yield side

    @contextlib.contextmanager
    def _timed(self, kind: str, M, N, K, m_dev=None, k_dev=None):
        """(GemmTimer only) bracket the body's launch with two timing events on the current stream and record it."""
        if self.gemm_timer is None:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        self.gemm_timer.records.append((kind, e0, e1, M, N, K, m_dev, k_dev))

    @contextlib.contextmanager
    def block(self, name: str):
        """roctx range (torch.cuda.nvtx maps to roctx on ROCm) around one block of the step; a no-op unless `roctx`."""
        if not self.roctx:
            yield
            return
        torch.cuda.nvtx.range_push(name)
        try:
            yield
        finally:
            torch.cuda.nvtx.range_pop()

    def mark(self, name: str) -> None:
        if self.marks is None:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        pr = self._params_ready
        self.marks.append((name, time.perf_counter(), ev, None if pr is None else pr.query()))

    def wait_params(self) -> None:
        """Order the current stream after the last optimizer step, if it ran on the optimizer stream (no host
        synchronisation). The event is kept until the next step replaces it: callers on different streams each wait."""
        ev = self._params_ready
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def _span_begin(self):
        """(GemmTimer only) start of a stream-order span on the current stream."""
        if self.gemm_timer is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _span_end(self, name, start) -> None:
        if start is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.gemm_timer.spans.setdefault(name, []).append((start, e))

    def ln_ws(self) -> torch.Tensor:
        """Partial-sum workspace of the LayerNorm backward kernels, sized by the library's own query for the largest row
        count it can be asked for (every token of the largest batch seen so far)."""
        n = int(hip.lib().stonk_layernorm_bwd_workspace_floats(1 << 30, self.cfg.hidden_size))
        return self.buf("ln.ws", (n,), F32)

    def ln_bwd(self, dy, x, mean, rstd, gamma, dx, dx_drop, dgamma, dbeta, rows, H, flags, p_in, seed_in, p_out, seed_out):
        """stonk_layernorm_bwd on the current stream, with the shared partial-sum workspace."""
        ws = self.ln_ws()
        if self._inputs_only:
            dgamma = dbeta = None
        hip.call("stonk_layernorm_bwd", hip.ptr(dy), hip.ptr(x), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma), hip.ptr(dx),
                 hip.ptr(dx_drop), hip.ptr(dgamma), hip.ptr(dbeta), rows, H, flags, p_in, seed_in, p_out, seed_out,
                 ws.data_ptr(), ws.numel(), hip.stream_ptr())

    def check_errors(self) -> None:
        """Raise for any flag the kernels set (one tiny D2H copy; call where a sync is acceptable)."""
        e = int(self.err.item())
        if e:
            self.err.zero_()
            msgs = [m for b, m in self.ERR_BITS.items() if e & b]
            if e & self.KEY_ERROR_BITS:
                raise KeyError("; ".join(msgs))
            raise IndexError("; ".join(msgs))

    def gemm(self, A, B, C, M, N, K, flags=0, bias=None, resid=None, aux=None, alpha=1.0, split_k=1, m_dev=None,
             k_dev=None, drop_p=0.0, seed=0, kernel=hip.GEMM_AUTO):
        with self._timed("nt", M, N, K, m_dev, k_dev):
            hip.call("stonk_gemm_nt_bf16", A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0),
                     M, N, K, flags, hip.ptr(bias), hip.ptr(resid), 0 if resid is None else resid.stride(0), hip.ptr(aux),
                     0 if aux is None else aux.stride(0), alpha, split_k, hip.ptr(m_dev), hip.ptr(k_dev), drop_p,
                     seed & 0xFFFFFFFF, kernel, hip.stream_ptr())

    def _split_k(self, M, N, K, side_stream=False) -> int:
        # 128x128 tiles, two workgroups co-resident per CU = 512 slots on 256 CUs: the sweep in tools/sweep_wgrad.py
        # is fastest when tiles x split fills ONE co-resident wave without a tail (432-480 workgroups)
        tiles = ((M + 127) // 128) * (N // 128)
        # the large weight gradients (FFN up / down, fused QKV) go to the four-wave 256x256 kernel, which splits K itself
        # (split_k = 0): -1.4 ms per step in an interleaved A/B; 768 x 768 (36 tiles) and the text decoder's
        # gradient (29 056 rows: not a multiple of 256) stay on the 128x128 kernel. Beside the dgrad chain (second
        # stream) the kernel is held to 160 CUs' worth of workgroups (split_k = -160): another -1.5 ms
        # ... and so does the entity decoder's 175 104 x 768 gradient (2052 unsplit tiles, device-side token count, 5.7 GB
        # operand extent - the kernel re-bases its buffer resources per K tile): 863 us against 966 alone, -0.27 ms in the step
        if tiles >= self.tn_min_tiles and K >= self.tn_min_k and M % 256 == 0 and N % 256 == 0:
            return -self.tn_cus if side_stream else 0
        return max(1, min(32, 480 // tiles, K // 64))

    def wgrad(self, dy, x, dW, db, M_out, N_in, T, k_dev=None, alpha=1.0, name=None):
        """dW[M_out, N_in] += dy[T, M_out]^T . x[T, N_in];  db[M_out] += colsum(dy)   (fp32 atomics, split-K).
        With `overlap_wgrad` the launch goes to the second stream, ordered after everything enqueued so far on the
        current one; a GemmTimer brackets it with events on THAT stream, in the same launch configuration.
        `name` (a weight in `store_names`, first contribution of the optimizer step): the result is STORED when the launch
        has one K split - no atomics, and the optimizer does not zero the span afterwards."""
        if self._inputs_only:   # (before the store-mode bookkeeping: `store_log`, `grad_stale`, `store_first` do not move)
            return
        self.sumsq_valid.discard(name)   # whatever this launch does to the gradient, an earlier launch's sums are not its norm
        side = self.overlap_wgrad
        split = self._split_k(M_out, N_in, T, side)
        # (the fork: dy and x are complete on the main stream at this point)
        with (self._fork("_wstream") if side else contextlib.nullcontext()), \
                self._timed("tn_a4" if split <= 0 else "tn", M_out, N_in, T, None, k_dev):
            args = (dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dW.data_ptr(), dW.stride(0), hip.ptr(db), M_out,
                    N_in, T, alpha, split, hip.ptr(k_dev), hip.stream_ptr())
            # what the store entry asks beyond the accumulating one is decided HERE (no bias, ld >= cols, 32-bit byte offsets):
            # a launch outside it takes the accumulating route by this test, and the entry's STONK_ESHAPE can then only mean
            # "the routing splits K at this shape" (anything else both entries refuse alike, and the call below raises)
            can_store = db is None and dW.stride(0) >= N_in and M_out * dW.stride(0) * 4 < 1 << 31
            if name is not None and self.store_first and name in self.store_names and can_store:
                slots = self._sumsq_slots(name, M_out, N_in, T, split) if self.store_sumsq and self.norm_from_epilogue else None
                if slots is None:
                    rc = hip.lib().stonk_gemm_tn_bf16_store(*args)
                else:
                    rc = hip.lib().stonk_gemm_tn_bf16_store_sumsq(*args[:-1], slots.data_ptr(), slots.numel(), args[-1])
                self.store_log.append((name, rc))
                if rc == hip.OK:
                    self.grad_stale.discard(name)
                    if slots is not None:
                        self.sumsq_valid.add(name)
                    return
                if rc != hip.ESHAPE:
                    hip.check(rc, "stonk_gemm_tn_bf16_store")
            if name in self.grad_stale:   # the optimizer left the previous step's gradient in place
                dW.zero_()
                self.grad_stale.discard(name)
            hip.call("stonk_gemm_tn_bf16", *args)

    def _groupable(self, kind: str, shapes) -> bool:
        """Whether the weight gradients `shapes` = [(M_out, N_in, T), ...] of one layer go out as ONE grouped launch
        (stonk_gemm_tn_bf16_group) once the operands of the last are ready: the group is switched on, the launches go to the
        second stream, the members share one row count (not the pruned last layer's attention pair) and each of them
        is one the four-wave kernel takes today. Decided BEFORE the first member is held back, so that everything else is
        launched exactly where it was."""
        if kind not in self.wgrad_groups or not self.overlap_wgrad or self._inputs_only:
            return False
        return len({T for _, _, T in shapes}) == 1 and all(self._split_k(M, N, T, True) <= 0 for M, N, T in shapes)

    def wgrad_group(self, members) -> None:
        """`wgrad` for members = [(dy, x, dW, db, M_out, N_in, T), ...] that `_groupable` admitted, as one launch on the
        second stream, ordered after everything enqueued so far on the current one: every member's operands must be
        complete by now and must stay as they are until the side stream is done with them (the caller's business). A
        GemmTimer sees one launch with the members' summed FLOPs. A group the library refuses for its shape goes out as
        single launches, here. (Members carry no store-mode name - the layers' gradients have none - so `grad_stale`,
        `sumsq_valid` and `store_log` have nothing to record; a named gradient goes through `wgrad`.)"""
        T = members[0][6]
        probs = hip.tn_problems([(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dW.data_ptr(), dW.stride(0), hip.ptr(db),
                                  M, N, T, 1.0, 0) for dy, x, dW, db, M, N, T in members])
        with self._fork("_wstream"), self._timed("tn_a4", sum(m[4] * m[5] for m in members), 1, T):
            rc = hip.lib().stonk_gemm_tn_bf16_group(probs, len(members), self.tn_cus, hip.stream_ptr())
        self.group_log.append((len(members), rc))
        if rc == hip.ESHAPE:
            if self.gemm_timer is not None:
                self.gemm_timer.records.pop()   # (nothing ran between its two events)
            for m in members:
                self.wgrad(*m)
            return
        hip.check(rc, "stonk_gemm_tn_bf16_group")

    def _sumsq_slots(self, name, M, N, K, split) -> Optional[torch.Tensor]:
        """The region of the slot buffer that the store launch of weight `name` fills (one float per output tile), or None
        when the store entry refuses the shape (the plain attempt then records its status). Regions lie in the order of
        `store_names`, so that all of them together are ONE contiguous array of extras for stonk_sumsq_f32_plus."""
        n = int(hip.lib().stonk_gemm_tn_store_tiles(M, N, K, split))
        if n <= 0:
            return None
        at = self.store_names.index(name)
        if self._sumsq_tiles.get(name) != n:   # (first use, or another shape: the regions behind this one move)
            self._sumsq_tiles[name] = n
            self.sumsq_valid.difference_update(self.store_names[at + 1:])
        total = sum(self._sumsq_tiles.values())
        if self._sumsq_buf is None or self._sumsq_buf.numel() < total:
            self._sumsq_buf = torch.zeros(max(total, 16384), dtype=F32, device=self.device)
            self.sumsq_valid.clear()
        first = sum(self._sumsq_tiles.get(k, 0) for k in self.store_names[:at])
        return self._sumsq_buf[first:first + n]

    def take_wgrad_sumsq(self):
        """([lo, hi) spans of the flat gradient buffer whose sum of squares is already known, those sums: one device array) when
        EVERY weight of `store_names` was stored with its sums by this step's backward, else None. Either way the slots are
        used up: a later step must write its own."""
        ok = bool(self.store_names) and self.sumsq_valid == set(self.store_names)
        self.sumsq_valid.clear()
        if not ok:
            return None
        total = sum(self._sumsq_tiles[k] for k in self.store_names)
        return sorted(self.P.span(k) for k in self.store_names), self._sumsq_buf[:total]

    def _gather_rows(self, src, rd_rows, cnt, dst, cap) -> None:
        """dst[i] = src[rd_rows[i]] for the first cnt[0] rows (a device-side count); rows from the count up to the next
        multiple of 128, at most `cap`, are zero-filled."""
        H = self.cfg.hidden_size
        hip.call("stonk_gather_rows_bf16", src.data_ptr(), H, rd_rows.data_ptr(), cnt.data_ptr(), dst.data_ptr(), H, H, cap,
                 hip.stream_ptr())

    def _scatter_rows_into_zeros(self, src, rd_rows, cnt, dst, T) -> None:
        """dst[:T] = 0, then dst[rd_rows[i]] = src[i] for the first cnt[0] rows."""
        H = self.cfg.hidden_size
        dst[:T].zero_()
        hip.call("stonk_scatter_rows_bf16", src.data_ptr(), H, rd_rows.data_ptr(), cnt.data_ptr(), dst.data_ptr(), H, H,
                 hip.stream_ptr())

    def _kernel(self, site: str, persistent_in_backward: bool = False) -> int:
        """NT kernel of a launch site: a tool's pin, else the dispatcher-scheduled form for a backward launch that
        would otherwise be persistent while a collective holds CUs, else the library's own choice."""
        k = self.kernel_for.get(site)
        if k is not None:
            return k
        if persistent_in_backward and self.comm_overlap:
            return hip.GEMM_DISPATCHED2
        return hip.GEMM_AUTO

    def seed(self, layer: int, site: int) -> int:
        return (self.seed_base * 0x9E3779B1 + layer * 64 + site) & 0xFFFFFFFF

    # ------------------------------------------------------------------ derived weights
    def refresh_derived(self, bf16_mirror: bool = True) -> None:
        """bf16 mirrors (if the optimizer has not just written them) and W^T copies for dgrad."""
        st = hip.stream_ptr()
        if bf16_mirror:
            for s in (self.P,) if self.BB is None else (self.P, self.BB):
                hip.call("stonk_cast_f32_to_bf16", s.data.data_ptr(), s.bf16.data_ptr(), s.numel, st)
        self._refresh_wt(st)

    def _refresh_wt(self, st) -> None:
        if self._wt_desc is None or self._wt_desc[3] != self.P.bf16.data_ptr():   # (the table holds raw addresses)
            self._wt_desc = self._build_wt_table()
        desc, n, tiles, _ = self._wt_desc
        hip.call("stonk_transpose_bf16_batched", desc.data_ptr(), n, tiles, st)

    def _wt_weights(self):
        """(name, offset, rows, padded rows, cols, W^T copy) of every weight a dgrad GEMM reads transposed, in the flat
        buffer's order. The table kernels move 16-byte vectors and cannot validate a device-side table: what they assume is
        checked here."""
        for name, (off, shape, pshape) in self.P.index.items():
            if len(shape) != 2 or not name.endswith(".weight") or shape[0] < 64:
                continue
            if "embeddings" in name or "pooler" in name or "seq_relationship" in name:
                continue
            rows, cols = shape
            rpad = pshape[0] if pshape[0] % 64 == 0 else (pshape[0] + 63) // 64 * 64
            wt = self.P.wt.get(name)
            if wt is None:
                wt = torch.zeros(cols, rpad, dtype=BF16, device=self.device)
                self.P.wt[name] = wt
            src = self.P.bf16_view(name, padded=False)
            if cols % 8 or src.data_ptr() % 16 or wt.data_ptr() % 16 or rpad % 8 or wt.shape[1] < (rows + 63) // 64 * 64 \
                    or off % 4 or wt.stride(0) != rpad:
                raise ValueError(f"{name}: [{rows}, {cols}] cannot take the batched W^T refresh (needs cols % 8 == 0, "
                                 "16-byte aligned slices and a destination of roundup64(rows) columns)")
            yield name, off, rows, pshape[0], cols, rpad, src, wt

    def _build_wt_table(self):
        """Descriptor table of the batched W^T refresh (stonk_transpose_bf16_batched): one entry per dgrad weight - source =
        its slice of the bf16 mirror (bit-identical to casting the fp32 master), destination = the [in, out_padded] copy.
        Addresses are stable for the life of the store, so the table is built once."""
        entries, first = [], 0
        for _, _, rows, _, cols, rpad, src, wt in self._wt_weights():
            col_tiles = (cols + 63) // 64
            entries.append(struct.pack("<QQqqqiiii", src.data_ptr(), wt.data_ptr(), cols, rpad, rows, cols, first, col_tiles, 0))
            first += ((rows + 63) // 64) * col_tiles
        raw = torch.frombuffer(bytearray(b"".join(entries)), dtype=torch.uint8).to(self.device)
        return raw, len(entries), first, self.P.bf16.data_ptr()

    def adamw_tables(self):
        """Device tables of stonk_adamw_step_tiled over the trainable store, built once: (tile descriptors, entries, tiles,
        flat spans, entries, chunks). The tile table holds the weights of `_wt_weights` (all their padded rows); the flat
        spans are the complement in [0, numel) - biases, LayerNorm, embeddings, pooler, NSP head and the alignment gaps."""
        key = (self.P.data.data_ptr(), self.P.bf16.data_ptr())
        if self._adamw_tables is not None and self._adamw_tables[-1] == key:
            return self._adamw_tables[:-1]
        entries, first, spans, chunks, pos = [], 0, [], 0, 0
        for name, off, rows, prows, cols, rpad, _, wt in self._wt_weights():
            if off < pos or (prows * cols) % 4:
                raise ValueError(f"{name}: the flat buffer's order or alignment does not fit the tiled optimizer step")
            if off > pos:
                spans.append((pos, off, chunks))
                chunks += (off - pos + 1023) // 1024
            col_tiles = (cols + 63) // 64
            entries.append(struct.pack("<qQqqqiiii", off, wt.data_ptr(), rpad, rows, prows, cols, first, col_tiles, 0))
            first += ((prows + 63) // 64) * col_tiles
            pos = off + prows * cols
        if pos < self.P.numel:
            spans.append((pos, self.P.numel, chunks))
            chunks += (self.P.numel - pos + 1023) // 1024
        if not entries or self.P.numel % 4:
            raise ValueError("no weight with a W^T copy: the tiled optimizer step does not apply")
        desc = torch.frombuffer(bytearray(b"".join(entries)), dtype=torch.uint8).to(self.device)
        flat = torch.tensor(spans, dtype=torch.int64, device=self.device).reshape(-1, 3)
        self._adamw_tables = (desc, len(entries), first, flat, len(spans), chunks, key)
        return self._adamw_tables[:-1]

    # ------------------------------------------------------------------ one BERT layer
    def layer_fwd(self, S: FlatStore, prefix: str, x, L: Rows, p_hid, p_att, lidx, save: Optional[dict],
                  last: bool = False, attn_maps: Optional[tuple] = None):
        """One BERT layer on the L.T rows of the layout `L` (`Rows`).
        `last` (the layer whose output only the pooler and the heads read) with read rows in the layout: the feed-forward
        block runs on the READ rows only - gathered after the attention block's LayerNorm, or (`rd.attn`) behind the
        attention core - and the layer's output has L.rd.T rows.
        `attn_maps` (padded layout only): (probs fp32 [B, NH, seq, seq] or None, modal_mass fp32 [B, NH, seq, 2] or None,
        half) - this layer's attention probabilities at p = 0 are written there (stonk_attention_probs), from the `qkv`
        buffer right behind the projection: a forward-only pass reuses that buffer from layer to layer."""
        cfg = self.cfg
        H, I, NH = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
        B, seq, T, mask, cu = L.B, L.S, L.T, L.mask, L.cu
        rd = L.rd if last else None
        cap = B * seq
        st = hip.stream_ptr()
        tag = prefix if save is not None else "tmp"
        w = S.bf16_view
        f = S.view
        qkv = self.buf(f"{tag}.qkv", (cap, 3 * H))
        self.gemm(x, w(prefix + ".attention.self.qkv.weight"), qkv, T, 3 * H, H, flags=hip.EPI_BIAS,
                  bias=f(prefix + ".attention.self.qkv.bias"), kernel=self._kernel("qkv"))
        if attn_maps is not None:
            if cu is not None:
                raise ValueError("attention maps are written in the padded layout only")
            probs, modal, half = attn_maps
            hip.call("stonk_attention_probs", qkv.data_ptr(), qkv.data_ptr() + 2 * H, 3 * H, hip.ptr(mask), hip.ptr(probs),
                     hip.ptr(modal), B, NH, seq, 64, half, 1.0 / math.sqrt(64.0), st)
        # (zeroed when allocated: in the packed layout the rows between the last sequence and T are never written by the
        # attention kernel and must stay finite for the projections that run over them)
        ctx = self.buf(f"{tag}.ctx", (cap, H), zero=True)
        lse = self.buf(f"{tag}.lse", (B, NH, seq), F32)
        qattn = rd is not None and rd.attn   # queries = the read rows only (a sequence's first rows)
        qoff = rd.offsets if qattn else None
        self._attention_fwd(qkv, mask, cu, qoff, ctx, lse, B, NH, seq, p_att, lidx, st)
        Ta, a_in, res = T, ctx, x                  # rows / input / residual of the output projection
        if qattn:
            Ta = rd.T
            a_in, res = self.buf(f"{tag}.ctxrd", (cap, H)), self.buf(f"{tag}.xrd", (cap, H))
            self._gather_rows(ctx, rd.rows, rd.cnt, a_in, cap)
            self._gather_rows(x, rd.rows, rd.cnt, res, cap)
        s1 = self.buf(f"{tag}.s1", (cap, H))
        fl = hip.EPI_BIAS | hip.EPI_RESID | (hip.EPI_DROPOUT if p_hid > 0 else 0)
        self.gemm(a_in, w(prefix + ".attention.output.dense.weight"), s1, Ta, H, H, flags=fl,
                  bias=f(prefix + ".attention.output.dense.bias"), resid=res, drop_p=p_hid, seed=self.seed(lidx, 2),
                  kernel=self._kernel("attn_out"))
        h1 = self.buf(f"{tag}.h1", (cap, H))
        st1 = self.buf(f"{tag}.st1", (2, cap), F32)
        hip.call("stonk_layernorm_fwd", s1.data_ptr(), f(prefix + ".attention.output.LayerNorm.weight").data_ptr(),
                 f(prefix + ".attention.output.LayerNorm.bias").data_ptr(), h1.data_ptr(), st1[0].data_ptr(),
                 st1[1].data_ptr(), Ta, H, cfg.layer_norm_eps, 0, 0.0, 0, st)
        hf, Tf = h1, Ta                            # input rows of the feed-forward block
        if rd is not None and not qattn:
            hf, Tf = self.buf(f"{tag}.h1rd", (cap, H)), rd.T
            self._gather_rows(h1, rd.rows, rd.cnt, hf, cap)
        g = self.buf(f"{tag}.g", (cap, I))
        u = self.buf(f"{tag}.u", (cap, I)) if save is not None else None
        self._ffn_up(S, prefix, hf, g, u, Tf)
        s2 = self.buf(f"{tag}.s2", (cap, H))
        fl = hip.EPI_BIAS | hip.EPI_RESID | (hip.EPI_DROPOUT if p_hid > 0 else 0)
        self.gemm(g, w(prefix + ".output.dense.weight"), s2, Tf, H, I, flags=fl, bias=f(prefix + ".output.dense.bias"),
                  resid=hf, drop_p=p_hid, seed=self.seed(lidx, 3), kernel=self._kernel("ffn_down"))
        y = self.buf(f"{prefix}.y" if save is not None else f"tmp.y{lidx & 1}", (cap, H))
        st2 = self.buf(f"{tag}.st2", (2, cap), F32)
        hip.call("stonk_layernorm_fwd", s2.data_ptr(), f(prefix + ".output.LayerNorm.weight").data_ptr(),
                 f(prefix + ".output.LayerNorm.bias").data_ptr(), y.data_ptr(), st2[0].data_ptr(), st2[1].data_ptr(), Tf,
                 H, cfg.layer_norm_eps, 0, 0.0, 0, st)
        if save is not None:
            save[prefix] = dict(x=x, qkv=qkv, ctx=ctx, ctx_in=a_in, lse=lse, s1=s1, h1=hf, st1=st1, g=g, u=u, s2=s2, st2=st2)
        return y

    # What a layer does between its GEMMs and LayerNorms, as methods: the dense attention core and the erf GELU carried by
    # the FFN GEMMs' epilogues. A subclass with another attention family or activation (bigbird_encoder.BigBirdEngine)
    # overrides these four and inherits the chain.
    def _attention_fwd(self, qkv, mask, cu, qoff, ctx, lse, B, NH, seq, p_att, lidx, st) -> None:
        H = self.cfg.hidden_size
        hip.call("stonk_attention_fwd", qkv.data_ptr(), qkv.data_ptr() + 2 * H, qkv.data_ptr() + 4 * H, 3 * H,
                 hip.ptr(mask), hip.ptr(cu), hip.ptr(qoff), ctx.data_ptr(), H, lse.data_ptr(), B, NH, seq, 64,
                 1.0 / math.sqrt(64.0), p_att, self.seed(lidx, 1), st)

    def _attention_bwd(self, qkv, mask, cu, qoff, ctx, dctx, lse, delta, dqkv, B, NH, seq, p_att, lidx, st) -> None:
        H = self.cfg.hidden_size
        aargs = (qkv.data_ptr(), qkv.data_ptr() + 2 * H, qkv.data_ptr() + 4 * H, 3 * H, hip.ptr(mask), hip.ptr(cu),
                 hip.ptr(qoff), ctx.data_ptr(), H, dctx.data_ptr(), H, lse.data_ptr(), delta.data_ptr(),
                 dqkv.data_ptr(), dqkv.data_ptr() + 2 * H, 3 * H, dqkv.data_ptr() + 4 * H, B, NH, seq, 64,
                 1.0 / math.sqrt(64.0), p_att, self.seed(lidx, 1))
        hip.call("stonk_attention_bwd", *aargs, st)

    def _ffn_up(self, S: FlatStore, prefix: str, hf, g, u, Tf) -> None:
        """g = act(hf . W^T + b); `u` (None in a forward-only pass): what the backward's `_ffn_down_dgrad` reads."""
        H, I = self.cfg.hidden_size, self.cfg.intermediate_size
        fl = hip.EPI_BIAS | hip.EPI_GELU | ((hip.EPI_SAVE_PREACT | hip.EPI_AUX_GRAD) if u is not None else 0)
        self.gemm(hf, S.bf16_view(prefix + ".intermediate.dense.weight"), g, Tf, I, H, flags=fl,
                  bias=S.view(prefix + ".intermediate.dense.bias"), aux=u, kernel=self._kernel("ffn_up"))

    def _ffn_down_dgrad(self, prefix: str, df, du, u, Tf) -> None:
        """du = (df . W_down) o act'(pre-activation), from what `_ffn_up` left in `u`."""
        H, I = self.cfg.hidden_size, self.cfg.intermediate_size
        self.gemm(df, self.P.wt[prefix + ".output.dense.weight"], du, Tf, I, H, flags=hip.EPI_GELU_BWD | hip.EPI_AUX_GRAD,
                  aux=u, kernel=self._kernel("dgrad_gelu", True))

    def layer_bwd(self, prefix: str, dy, L: Rows, p_hid, p_att, lidx, sv, last: bool = False):
        """dy: bf16 [T,H] gradient of the layer output. Returns the gradient of the layer input. `L`, `last`: the
        forward's (`layer_fwd`). Where the feed-forward block ran on the read rows, dy has L.rd.T rows and its input
        gradient is scattered back to all rows."""
        cfg = self.cfg
        H, I, NH = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
        B, seq, T, mask, cu = L.B, L.S, L.T, L.mask, L.cu
        rd = L.rd if last else None
        cap = B * seq
        st = hip.stream_ptr()
        P = self.P
        g_ = P.grad_view
        f = P.view
        wt = P.wt
        # dY buffers alternate by layer parity: the side stream may still be reading layer i+1's while layer i writes;
        # before reusing the buffers of layer i+2 the main stream waits for that layer's last weight-gradient GEMM
        par = lidx & 1
        ev = self._wgrad_done.pop(par, None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
        # ---- LN2 backward: ds2 (residual branch) and df (through the FFN-output dropout)
        ds2 = self.buf(f"b.ds2.{par}", (cap, H))
        df = self.buf(f"b.df.{par}", (cap, H)) if p_hid > 0 else None
        Tf = T if rd is None else rd.T             # rows the feed-forward block ran on
        self.ln_bwd(dy, sv["s2"], sv["st2"][0], sv["st2"][1], f(prefix + ".output.LayerNorm.weight"), ds2, df,
                    g_(prefix + ".output.LayerNorm.weight"), g_(prefix + ".output.LayerNorm.bias"), Tf, H, 0, 0.0, 0, p_hid,
                    self.seed(lidx, 3))
        if df is None:
            df = ds2
        # ---- FFN down: wgrad, bias grad, dgrad fused with GELU'
        # (a held weight gradient: its operands - df / da of this parity, a saved activation - are written by nothing else in
        # this layer, and the next writer of this parity's buffers, layer i-2, first waits for `_wgrad_done[par]`, which is
        # recorded behind the grouped launch below)
        w_down = (df, sv["g"], g_(prefix + ".output.dense.weight"), g_(prefix + ".output.dense.bias"), H, I, Tf)
        group_ffn = self._groupable("ffn", [(H, I, Tf), (I, H, Tf)])
        if not group_ffn:
            self.wgrad(*w_down)
        du = self.buf(f"b.du.{par}", (cap, I))
        self._ffn_down_dgrad(prefix, df, du, sv["u"], Tf)
        # ---- FFN up
        w_up = (du, sv["h1"], g_(prefix + ".intermediate.dense.weight"), g_(prefix + ".intermediate.dense.bias"), I, H, Tf)
        if group_ffn:
            self.wgrad_group([w_down, w_up])
        else:
            self.wgrad(*w_up)
        qattn = rd is not None and rd.attn
        Ta = Tf if qattn else T                    # rows the attention block's projection / LayerNorm ran on
        dh1 = self.buf("b.dh1", (cap, H))
        gathered = rd is not None and not qattn    # the feed-forward block alone ran on gathered rows
        dh1f = self.buf("b.dh1rd", (cap, H)) if gathered else dh1
        self.gemm(du, wt[prefix + ".intermediate.dense.weight"], dh1f, Tf, H, I, flags=hip.EPI_RESID, resid=ds2,
                  kernel=self._kernel("dgrad_resid", True))
        if gathered:   # their gradient, scattered into an otherwise zero gradient of the attention block's output
            self._scatter_rows_into_zeros(dh1f, rd.rows, rd.cnt, dh1, T)
        # ---- LN1 backward
        ds1 = self.buf(f"b.ds1.{par}", (cap, H))
        da = self.buf(f"b.da.{par}", (cap, H)) if p_hid > 0 else None
        self.ln_bwd(dh1, sv["s1"], sv["st1"][0], sv["st1"][1], f(prefix + ".attention.output.LayerNorm.weight"), ds1, da,
                    g_(prefix + ".attention.output.LayerNorm.weight"), g_(prefix + ".attention.output.LayerNorm.bias"), Ta, H, 0,
                    0.0, 0, p_hid, self.seed(lidx, 2))
        if da is None:
            da = ds1
        # ---- attention output projection
        w_out = (da, sv["ctx_in"], g_(prefix + ".attention.output.dense.weight"),
                 g_(prefix + ".attention.output.dense.bias"), H, H, Ta)
        group_attn = self._groupable("attn", [(3 * H, H, T), (H, H, Ta)])
        if not group_attn:
            self.wgrad(*w_out)
        dctx = self.buf("b.dctx", (cap, H))
        dctxa = self.buf("b.dctxrd", (cap, H)) if qattn else dctx
        self.gemm(da, wt[prefix + ".attention.output.dense.weight"], dctxa, Ta, H, H,
                  kernel=self._kernel("dgrad_attn_out", True))
        if qattn:   # the read rows' gradients go back to their packed rows: into zeros (the kernels read whole query tiles)
            ds1rd, ds1 = ds1, self.buf("b.ds1full", (cap, H))
            self._scatter_rows_into_zeros(dctxa, rd.rows, rd.cnt, dctx, T)
            self._scatter_rows_into_zeros(ds1rd, rd.rows, rd.cnt, ds1, T)
        # ---- attention core
        qkv = sv["qkv"]
        dqkv = self.buf(f"b.dqkv.{par}", (cap, 3 * H))
        delta = self.buf("b.delta", (B, NH, seq), F32)
        qoff = rd.offsets if qattn else None
        if qattn:
            # dQ of the rows that were not queries (the kernel does not write them) feeds the projection's gradients; their dK and
            # dV are the dK/dV kernel's to write (every key row of a sequence), so only the dQ third is cleared: 40 of 122 MB
            dqkv[:T, :H].zero_()
        # (packed layout: the rows between the last sequence and T are not the attention kernel's to write, and the weight
        # gradient below contracts over all T rows - backward_encoder zeroes them in both dqkv buffers once per step)
        self._attention_bwd(qkv, mask, cu, qoff, sv["ctx"], dctx, sv["lse"], delta, dqkv, B, NH, seq, p_att, lidx, st)
        # ---- QKV projection
        w_qkv = (dqkv, sv["x"], g_(prefix + ".attention.self.qkv.weight"), g_(prefix + ".attention.self.qkv.bias"), 3 * H, H, T)
        if group_attn:
            self.wgrad_group([w_qkv, w_out])
        else:
            self.wgrad(*w_qkv)
        dx = self.buf(f"b.dx{lidx & 1}", (cap, H))
        self.gemm(dqkv, wt[prefix + ".attention.self.qkv.weight"], dx, T, H, 3 * H, flags=hip.EPI_RESID, resid=ds1,
                  kernel=self._kernel("dgrad_resid", True))
        if self._wstream is not None and self.overlap_wgrad:
            done = torch.cuda.Event()
            done.record(self._wstream)
            self._wgrad_done[par] = done
        return dx

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
        cfg = self.cfg
        H, cap_rows, T, st = cfg.hidden_size, L.B * L.S, L.Th, hip.stream_ptr()
        f, w = self.P.view, self.P.bf16_view
        nsp = self._pooled_linear("cls.seq_relationship", f"{pre}.nsp", pooled, L.B, 2)
        gt = self.buf(f"{pre}.gt", (cap_rows, H))
        ut = self.buf(f"{pre}.ut", (cap_rows, H)) if save_preact else None
        self.gemm(seq_out, w("cls.predictions.transform.dense.weight"), gt, T, H, H,
                  flags=hip.EPI_BIAS | hip.EPI_GELU | (hip.EPI_SAVE_PREACT if save_preact else 0),
                  bias=f("cls.predictions.transform.dense.bias"), aux=ut)
        t = self.buf(f"{pre}.t", (cap_rows, H))
        stt = self.buf(f"{pre}.stt", (2, cap_rows), F32)
        hip.call("stonk_layernorm_fwd", gt.data_ptr(), f("cls.predictions.transform.LayerNorm.weight").data_ptr(),
                 f("cls.predictions.transform.LayerNorm.bias").data_ptr(), t.data_ptr(), stt[0].data_ptr(),
                 stt[1].data_ptr(), T, H, cfg.layer_norm_eps, 0, 0.0, 0, st)
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

    def _small_wgrad(self, name: str, N: int, K: int):
        """(dW [N, K], db [N]) for stonk_small_linear_bwd of the linear layer `name`: its gradient views - in the
        inputs-only backward one scratch buffer, never read, because the kernel cannot be told to skip them."""
        if not self._inputs_only:
            return self.P.grad_view(name + ".weight"), self.P.grad_view(name + ".bias")
        w = self.buf("ia.dw", (N * K + N,), F32)
        return w[:N * K], w[N * K:]

    def _make_notify(self, hook):
        """Gradients of a segment are final once the SIDE stream has run its weight-gradient GEMMs: the DP hook (RCCL
        all-reduce) is therefore issued under the side stream, which it then orders itself after."""
        if hook is None:
            return lambda name: None
        if not self.overlap_wgrad:
            return hook

        def notify(name):
            if self._wstream is None:
                hook(name)
                return
            with self._fork("_wstream"):        # (behind the bias / LayerNorm gradients written by main-stream kernels)
                hook(name)
        return notify

    def join_wgrad(self) -> None:
        """Main stream waits for every outstanding weight-gradient GEMM (before the optimizer reads the gradients)."""
        if self._wstream is not None:
            torch.cuda.current_stream().wait_stream(self._wstream)
        self._wgrad_done.clear()

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
