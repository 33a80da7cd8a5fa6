"""The model-independent core of the HIP engines: `LayerEngine` schedules the C-ABI kernels (include/stonk_hip.h) of ONE
BERT layer, forward and backward, and owns what any stack of such layers needs around them. No torch arithmetic on the data
path: torch tensors are device memory, ``torch.cuda.current_stream()`` is the stream every launcher is given.

`LayerEngine` owns
  - the workspace (`buf`) and the side streams: weight gradients, optimizer (`optimizer_stream`, `wait_params`);
  - the GEMM and weight-gradient launch wrappers: `gemm`, `wgrad`, `wgrad_group`, store mode and its sum-of-squares slots;
  - the derived weights: bf16 mirrors, W^T copies, the AdamW device tables (`refresh_derived`, `adamw_tables`);
  - `layer_fwd` / `layer_bwd`, with the attention core and the FFN activation as four overridable methods (defaults: dense
    attention, erf GELU in the GEMM epilogues), on a row layout `Rows`;
  - the kernels' error word (`check_errors`; a subclass names the bits its kernels set).
It knows no model: no embeddings, no pooler, no head, no backbone. A model's engine subclasses it and adds its front and
its heads around the layers: `engine.Engine` (STonKGs), `engine.TextEngine` (the text baseline),
`bigbird_encoder.BigBirdEngine`. What `FlatBufferModel`, `FusedAdamW` and `Trainer` call on an engine is all here.

Activations needed by backward are kept in the persistent workspace (HBM is 288 GB; B=64 needs ~12 GB), nothing is
recomputed except attention probabilities.
"""
from __future__ import annotations

import collections
import contextlib
import dataclasses
import math
import os
import struct
import time
from typing import Dict, Optional

import torch

from . import _hip as hip
from .params import FlatStore

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


# The row layouts `layer_fwd` / `layer_bwd` run on. The core takes a layout as it is given one; who packs rows and prunes the
# last layer is the caller: `Engine.unpad`, `Engine.prune_last_ffn`, `Engine.prune_last_attn` below are the STonKGs engine's
# switches (engine.py), which builds the packed layouts in `encode`.
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


class LayerEngine:
    """Workspace, streams, GEMM / weight-gradient wrappers, derived weights and one BERT layer over the trainable store
    `store`. `cfg`: anything with `validate_for_hip()`, hidden_size, intermediate_size, num_attention_heads and
    layer_norm_eps (STonKGsConfig, BigBirdEncoderConfig)."""

    ERR_BITS: Dict[int, str] = {}   # what check_errors says for each bit of the kernels' error word (the layer chain sets none) ...
    KEY_ERROR_BITS = 0              # ... and which of them make it a KeyError instead of an IndexError

    def __init__(self, cfg, store: FlatStore, device):
        cfg.validate_for_hip()
        hip.lib()  # fail loudly, now, if the extension is missing
        self.cfg = cfg
        self.P = store
        self.device = device
        self.ws: Dict[str, torch.Tensor] = {}
        self.err = torch.zeros(1, dtype=I32, device=device)
        self.gemm_timer: Optional[GemmTimer] = None
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
        # Inputs-only backward (`Engine.input_gradients` alone sets it, through `_detached`): the chain of dgrad GEMMs, LayerNorm
        # and attention backward runs down to d(embedding sum) and nothing is written to the gradient buffer - `wgrad` returns
        # at once, `ln_bwd` passes null dgamma / dbeta, the small linear layers' weight gradients go to scratch,
        # stonk_embed_grad and the `notify` hooks are skipped. False: every path issues exactly the launches it issued
        # before the flag.
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

    def ln_fwd(self, x, gamma, beta, y, stats, rows) -> None:
        """stonk_layernorm_fwd on the current stream, without dropout: y = LayerNorm(x) on `rows` rows of hidden_size, their
        mean / reciprocal deviation into stats[0] / stats[1] (what `ln_bwd` reads)."""
        hip.call("stonk_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), stats[0].data_ptr(),
                 stats[1].data_ptr(), rows, self.cfg.hidden_size, self.cfg.layer_norm_eps, 0, 0.0, 0, hip.stream_ptr())

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
            for s in self._mirrored_stores():
                hip.call("stonk_cast_f32_to_bf16", s.data.data_ptr(), s.bf16.data_ptr(), s.numel, st)
        self._refresh_wt(st)

    def _mirrored_stores(self) -> tuple:
        """The stores whose bf16 mirror `refresh_derived` casts from the fp32 master: the trainable one; an engine with a
        store of its own beside it (a frozen backbone) overrides this and adds it."""
        return (self.P,)

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
        self._dense_drop_resid(S, prefix + ".attention.output.dense", "attn_out", a_in, res, s1, Ta, H, p_hid,
                               self.seed(lidx, 2))
        h1 = self.buf(f"{tag}.h1", (cap, H))
        st1 = self.buf(f"{tag}.st1", (2, cap), F32)
        self.ln_fwd(s1, f(prefix + ".attention.output.LayerNorm.weight"), f(prefix + ".attention.output.LayerNorm.bias"), h1,
                    st1, Ta)
        hf, Tf = h1, Ta                            # input rows of the feed-forward block
        if rd is not None and not qattn:
            hf, Tf = self.buf(f"{tag}.h1rd", (cap, H)), rd.T
            self._gather_rows(h1, rd.rows, rd.cnt, hf, cap)
        g = self.buf(f"{tag}.g", (cap, I))
        u = self.buf(f"{tag}.u", (cap, I)) if save is not None else None
        self._ffn_up(S, prefix, hf, g, u, Tf)
        s2 = self.buf(f"{tag}.s2", (cap, H))
        self._dense_drop_resid(S, prefix + ".output.dense", "ffn_down", g, hf, s2, Tf, I, p_hid, self.seed(lidx, 3))
        y = self.buf(f"{prefix}.y" if save is not None else f"tmp.y{lidx & 1}", (cap, H))
        st2 = self.buf(f"{tag}.st2", (2, cap), F32)
        self.ln_fwd(s2, f(prefix + ".output.LayerNorm.weight"), f(prefix + ".output.LayerNorm.bias"), y, st2, Tf)
        if save is not None:
            save[prefix] = dict(x=x, qkv=qkv, ctx=ctx, ctx_in=a_in, lse=lse, s1=s1, h1=hf, st1=st1, g=g, u=u, s2=s2, st2=st2)
        return y

    def _dense_drop_resid(self, S: FlatStore, name: str, site: str, x, resid, out, rows, K, p_hid, seed) -> None:
        """out = dropout(x . W^T + b) + resid in one GEMM: the linear layer `name` (K -> hidden_size) of store `S` that closes
        the attention block and the feed-forward block. `site`: its name for `_kernel`."""
        fl = hip.EPI_BIAS | hip.EPI_RESID | (hip.EPI_DROPOUT if p_hid > 0 else 0)
        self.gemm(x, S.bf16_view(name + ".weight"), out, rows, self.cfg.hidden_size, K, flags=fl, bias=S.view(name + ".bias"),
                  resid=resid, drop_p=p_hid, seed=seed, kernel=self._kernel(site))

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
