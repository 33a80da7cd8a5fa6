"""What the model classes share: an ``nn.Module`` whose parameters are views of flat HBM buffers (``params.FlatStore``).

``FlatBufferModel`` owns the device, the gradient views and their torch semantics, the tracking of master weights against
their derived copies, the weight init, the input conversion, the state-dict wrappers and the autograd bridge; a subclass
adds its stores, its engine (``self.engine``), its module tree and its ``forward``. ``SequenceClassifierFront`` is the
classification tail the two fine-tuning classes share."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, Optional

import torch
from torch import nn

from . import _hip as hip


def as_long(t, device):
    """``t`` as a contiguous int64 tensor on ``device``; the very same tensor if it is one already. None passes through."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    if t.device != device or t.dtype != torch.long or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.long).contiguous()
    return t


def _load_weights_file(path: str) -> Optional[Dict[str, torch.Tensor]]:
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file

        return load_file(st)
    pb = os.path.join(path, "pytorch_model.bin")
    if os.path.exists(pb):
        return torch.load(pb, map_location="cpu", weights_only=True)
    return None


class _StepFunction(torch.autograd.Function):
    """Makes ``loss.backward()`` (HF Trainer / accelerate) drive the engine's hand-written backward."""

    @staticmethod
    def forward(ctx, anchor, model, loss):
        ctx.model = model
        return loss.clone()

    @staticmethod
    def backward(ctx, dloss):
        model = ctx.model
        model._prepare_grads_for_autograd()
        model._backward(float(dloss), model._segment_hook)
        model._reattach_grads()
        model._external_step_pending = True   # whoever called loss.backward() steps the masters with its own optimizer
        return None, None, None


class FlatBufferModel(nn.Module):
    """A subclass's constructor builds ``self._store`` (the trainable store: its ``grad`` is THE gradient buffer),
    ``self.engine`` and the module tree, then calls ``_init_weights``, ``_bind_grad_views`` and ``refresh``."""

    def __init__(self, device=None):
        super().__init__()
        if not torch.cuda.is_available():
            raise hip.StonkHipError(f"{type(self).__name__} needs an MI355X: the hot path has no CPU fallback")
        self._device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._segment_hook = None
        self._anchor = torch.zeros((), device=self._device, requires_grad=True)

    # -------------------------------------------------------------- what a subclass provides
    def _stores(self) -> tuple:
        """The stores whose version counters are watched (and whose tensors are initialised), in init order."""
        raise NotImplementedError

    def _backward(self, gscale: float, on_segment_done) -> None:
        """The engine's backward that belongs to this class's forward."""
        raise NotImplementedError

    def _after_init_weights(self) -> None:
        """Hook: what the init sets apart from the three rules of ``_init_weights``."""

    # -------------------------------------------------------------- construction helpers
    def _init_weights(self, seed: int) -> None:
        """BERT init (hf _init_weights: N(0, initializer_range) matrices/embeddings, zero bias, unit LayerNorm)."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        std = self.config.initializer_range
        with torch.no_grad():
            for store in {id(x): x for x in self._stores()}.values():
                for name, (off, shape, _) in store.index.items():
                    v = store.view(name)
                    if "LayerNorm.weight" in name:
                        v.fill_(1.0)
                    elif name.endswith(".bias") or "LayerNorm.bias" in name:
                        v.zero_()
                    else:
                        v.copy_((torch.randn(shape, generator=g) * std).to(v.device))
            self._after_init_weights()

    def _bind_grad_views(self) -> None:
        self._grad_views = {n: p.grad for n, p in self.named_parameters() if p.requires_grad}

    def _long(self, t):
        return as_long(t, self._device)

    # -------------------------------------------------------------- masters <-> derived copies
    # The GEMMs read bf16 mirrors and bf16 W^T copies of the fp32 master weights; the fused optimizer refreshes them itself.
    # Anything ELSE that writes the masters is noticed here as far as torch lets it be noticed:
    #  * in-place writes THROUGH the parameters (a torch optimizer's step, `p.copy_` / `p.add_` under no_grad,
    #    `load_state_dict`) bump the version counter the parameter views share with their flat buffer;
    #  * an autograd-driven backward sets `_external_step_pending`: whoever called loss.backward() is about to step the
    #    masters, possibly through `p.data` - which has a version counter of its OWN and is invisible above. The flag stays
    #    set until a version change is seen (the ordinary optimizer) or `refresh()` is called: while it is set, every forward
    #    re-derives the copies (0.5 ms), so a `.data`-writing optimizer is never read stale;
    #  * a write through `p.data` that no backward preceded (weight surgery before eval / encode) CANNOT be seen:
    #    call `model.refresh()` after it.
    def refresh(self) -> None:
        """Recompute everything derived from the fp32 masters: bf16 mirrors and W^T copies. Called after init /
        load_state_dict."""
        self.engine.refresh_derived(bf16_mirror=True)
        self._mark_synced()

    def _versions(self) -> tuple:
        return tuple(s.data._version for s in self._stores())

    def _mark_synced(self, clear_pending: bool = True) -> None:
        self._synced_versions = self._versions()
        if clear_pending:
            self._external_step_pending = False

    def _sync_derived(self) -> None:
        """Called at the top of every forward: bring the derived copies up to date with externally modified masters."""
        v = self._versions()
        if v == self._synced_versions and not self._external_step_pending:
            return
        self._wait_params()
        self._rederive([s for s, new, old in zip(self._stores(), v, self._synced_versions) if new != old])

    def _rederive(self, written: list) -> None:
        """Hook: `written` = the stores whose masters changed (none: an external step is pending and may still come via
        `.data`, so the flag stays). A subclass overrides it where a store feeds more than the engine's own copies."""
        self.engine.refresh_derived(bf16_mirror=True)
        self._mark_synced(clear_pending=bool(written))

    # -------------------------------------------------------------- gradients
    def zero_grad(self, set_to_none: bool = True) -> None:
        """nn.Module.zero_grad on the flat gradient buffer: the engine's backward ACCUMULATES into it (+= / atomics), so
        dropping the `.grad` attributes alone would leave last step's gradients in place. The buffer is zeroed for both
        values of `set_to_none`; with True the attributes are dropped as torch does and re-attached by the next backward."""
        self._wait_params()
        self._store.grad.zero_()
        for p in self.parameters():
            if p.requires_grad:
                p.grad = None if set_to_none else p.grad
        if not set_to_none:
            self._reattach_grads(force=True)

    def _prepare_grads_for_autograd(self) -> None:
        """torch semantics for `loss.backward()`: a parameter whose `.grad` is None starts from zero (an optimizer's
        zero_grad(set_to_none=True) only drops the attributes), one that still has its view accumulates."""
        params = [(n, p) for n, p in nn.Module.named_parameters(self) if p.requires_grad]
        dropped = [n for n, p in params if p.grad is None]
        if not dropped:
            return
        if len(dropped) == len(params):
            self._store.grad.zero_()
        else:
            for n in dropped:
                self._grad_views[n].zero_()

    def _reattach_grads(self, force: bool = False) -> None:
        for name, p in nn.Module.named_parameters(self):
            if p.requires_grad and (force or p.grad is None):
                p.grad = self._grad_views[name]

    def named_grad_views(self) -> Dict[str, torch.Tensor]:
        """name -> view into the flat gradient buffer (stable across zero_grad(set_to_none=True))."""
        self._wait_params()
        return self._grad_views

    # -------------------------------------------------------------- nn.Module plumbing
    @property
    def device(self) -> torch.device:
        return self._device

    def _apply(self, fn, recurse=True):
        probe = fn(torch.zeros(1, device=self._device))
        if probe.device != self._device or probe.dtype != torch.float32:
            raise NotImplementedError(f"construct {type(self).__name__} on its target GPU; parameters are views of flat "
                                      "HBM buffers and cannot be moved or cast")
        return self

    # Accessors order the caller's stream after an optimizer step still running on the optimizer stream
    # (Engine.wait_params): whatever they hand out is final for work enqueued on the current stream.
    def _wait_params(self) -> None:
        eng = self.__dict__.get("engine")
        if eng is not None:
            eng.wait_params()

    def state_dict(self, *args, **kwargs):
        self._wait_params()
        return super().state_dict(*args, **kwargs)

    def named_parameters(self, *args, **kwargs):
        self._wait_params()
        return super().named_parameters(*args, **kwargs)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False, _refresh: bool = True):
        self._wait_params()
        res = super().load_state_dict(state_dict, strict=strict)
        if _refresh:
            self.refresh()
        return res

    def save_pretrained(self, path: str, safe_serialization: bool = False) -> None:
        """HF layout: config.json + pytorch_model.bin, or model.safetensors with ``safe_serialization=True`` (what newer
        HF versions write by default; `from_pretrained` reads either)."""
        self.config.save_pretrained(path)
        sd = {k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}
        if safe_serialization:
            from safetensors.torch import save_file

            save_file(sd, os.path.join(path, "model.safetensors"), metadata={"format": "pt"})
        else:
            torch.save(sd, os.path.join(path, "pytorch_model.bin"))


@dataclass
class SequenceClassifierOutput:
    """hf:modeling_outputs.SequenceClassifierOutput as returned by ref:stonkgs_finetuning.py:340-345."""

    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    hidden_states: Optional[tuple] = None
    attentions: Optional[tuple] = None

    def __getitem__(self, k):
        if isinstance(k, str):
            return getattr(self, k)
        return tuple(v for v in (self.loss, self.logits, self.hidden_states, self.attentions) if v is not None)[k]


class SequenceClassifierFront:
    """pooled [CLS] -> dropout -> Linear(hidden, num_labels) -> loss on ``engine.forward_cls`` / ``backward_cls``: mixed
    into a ``FlatBufferModel`` that has ``num_labels`` and prepares its inputs in
    ``_cls_inputs(input_ids, attention_mask, token_type_ids, labels) -> (ids, am, tt, labels, loss mode)``."""

    def _backward(self, gscale: float, on_segment_done) -> None:
        self.engine.backward_cls(gscale, on_segment_done)

    def _classify(self, ids, am, tt, labels, mode, return_dict):
        training = self.training
        self._sync_derived()
        need_bwd = labels is not None and torch.is_grad_enabled() and training
        out = self.engine.forward_cls(ids, am, tt, labels, self.num_labels, training, need_bwd, mode)
        loss = None
        if labels is not None:
            loss = _StepFunction.apply(self._anchor, self, out["loss"]) if need_bwd else out["loss"].clone()
        logits = out["logits"].clone()
        if not return_dict:
            return (loss, logits) if loss is not None else (logits,)
        return SequenceClassifierOutput(loss=loss, logits=logits, hidden_states=None, attentions=None)

    def forward_backward(self, inputs, gscale: float = 1.0, on_segment_done=None):
        ids, am, tt, labels, mode = self._cls_inputs(inputs["input_ids"], inputs.get("attention_mask"),
                                                     inputs.get("token_type_ids"), inputs.get("labels"))
        self._sync_derived()
        out = self.engine.forward_cls(ids, am, tt, labels, self.num_labels, self.training, True, mode)
        loss = out["loss"].clone()
        self.engine.backward_cls(gscale, on_segment_done)
        return loss
