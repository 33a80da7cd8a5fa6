"""BigBird block-sparse self-attention on the HIP kernels of ``csrc/bigbird_attention.hip``.

The encoder of ProtSTonKGs (ref:src/stonkgs/models/protstonkgs_model.py) is HuggingFace BigBird with
``attention_type="block_sparse"``: block size 64, 3 random blocks, 4096 tokens. Its attention
(hf:models/big_bird/modeling_big_bird.py:295-744) is expressed here as LISTS: for every head and query block the key blocks
it attends to, each with a multiplicity. HuggingFace concatenates the blocks it gathers and does not remove duplicates, so
a block gathered twice counts twice in the softmax; in eval mode its random plan is all zeros at 1024, 3072 and 4096 tokens
and every inner query block then sees block 0 ``1 + r`` times. The lists keep that as a multiplicity.

    bigbird_rand_attn(...)      the random part of a plan: zeros (eval) or a seeded draw (train)
    bigbird_block_lists(...)    forward and inverse lists of a plan, numpy int32, on the host
    BlockSparsePlan             the lists, uploaded once per device
    block_sparse_attention(...) the autograd op over stonk_block_sparse_attention_fwd / _bwd
    BigBirdBlockSparseSelfAttention   an nn.Module that loads HuggingFace's BigBirdBlockSparseAttention state dict

Like every product path of this package there is no fallback: without the library or a GPU the op raises.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from . import _hip as hip

BLOCK = 64        # rows per block (and the head dimension): the only size the kernels are built for
MIN_BLOCKS, MAX_BLOCKS = 5, 64
MAX_RANDOM_BLOCKS = 8


def _fixed_blocks(i: int, nb: int) -> list[int]:
    """The key blocks HuggingFace gives query block 1 <= i <= nb-2 besides the random ones, in its order."""
    if i == 1:
        return [0, 1, 2, nb - 1]
    if i == nb - 2:
        return [0, nb - 3, nb - 2, nb - 1]
    return [i - 1, i, i + 1, 0, nb - 1]


def _check_num_blocks(num_blocks) -> int:
    nb = int(num_blocks)
    if nb != num_blocks or not MIN_BLOCKS <= nb <= MAX_BLOCKS:
        raise ValueError(f"num_blocks must be an integer in [{MIN_BLOCKS}, {MAX_BLOCKS}], got {num_blocks!r}")
    return nb


def bigbird_rand_attn(num_blocks, num_rand_blocks, num_heads, mode, seed=None) -> np.ndarray:
    """The random blocks of a plan, int32 [num_heads, num_blocks - 2, num_rand_blocks]; row i-1 belongs to query block i.

    mode "eval": zeros - HuggingFace's eval-mode plan at 1024, 3072 and 4096 tokens, what a loaded ProtSTonKGs checkpoint
    runs at inference. mode "train": per head and query block, ``num_rand_blocks`` distinct blocks outside that block's
    fixed set, from ``numpy.random.default_rng(seed)`` (not HuggingFace's own np.random stream). Where fewer blocks than
    that lie outside the fixed set (num_blocks < 6 + num_rand_blocks), the shortfall is drawn, distinct again, from the
    fixed set - those blocks then count twice, as any duplicate does."""
    nb = _check_num_blocks(num_blocks)
    r, nh = int(num_rand_blocks), int(num_heads)
    if not 0 <= r <= MAX_RANDOM_BLOCKS:
        raise ValueError(f"num_rand_blocks must be in [0, {MAX_RANDOM_BLOCKS}], got {num_rand_blocks!r}")
    if nh <= 0:
        raise ValueError(f"num_heads must be positive, got {num_heads!r}")
    out = np.zeros((nh, nb - 2, r), dtype=np.int32)
    if mode == "eval":
        return out
    if mode != "train":
        raise ValueError(f"mode must be 'eval' or 'train', got {mode!r}")
    rng = np.random.default_rng(seed)
    for h in range(nh):
        for i in range(1, nb - 1):
            fixed = sorted(set(_fixed_blocks(i, nb)))
            free = [j for j in range(nb) if j not in fixed]
            take = min(r, len(free))
            if r - take > len(fixed):
                raise ValueError(f"{r} random blocks cannot be drawn from {nb} blocks")
            picks = list(rng.choice(free, size=take, replace=False)) if take else []
            picks += list(rng.choice(fixed, size=r - take, replace=False)) if r > take else []
            out[h, i - 1] = picks
    return out


def bigbird_block_lists(num_blocks, rand_attn) -> dict:
    """Forward and inverse lists of a BigBird plan, int32 numpy arrays:

    key_blocks / key_mult [NH, nb, nb], key_count [NH, nb]: the key blocks of (head, query block), ascending, each with its
    multiplicity (entries past the count are zero); query_blocks / query_mult / query_count: for (head, key block) the query
    blocks that list it, with the same multiplicities - what dK / dV walk. Query blocks 0 and nb-1 list every block once."""
    nb = _check_num_blocks(num_blocks)
    ra = np.asarray(rand_attn)
    if ra.ndim != 3 or ra.shape[1] != nb - 2 or ra.shape[0] < 1 or ra.shape[2] > MAX_RANDOM_BLOCKS:
        raise ValueError(f"rand_attn must have shape [num_heads, {nb - 2}, r <= {MAX_RANDOM_BLOCKS}], got {ra.shape}")
    if not np.issubdtype(ra.dtype, np.integer):
        raise ValueError(f"rand_attn must hold integers, got {ra.dtype}")
    if ra.size and (ra.min() < 0 or ra.max() >= nb):
        raise ValueError(f"rand_attn values must lie in [0, {nb})")
    nh = ra.shape[0]
    mult = np.zeros((nh, nb, nb), dtype=np.int32)      # mult[h, i, j]: how often query block i of head h sees key block j
    mult[:, 0, :] = 1
    mult[:, nb - 1, :] = 1
    for i in range(1, nb - 1):
        for j in _fixed_blocks(i, nb):
            mult[:, i, j] += 1
        for h in range(nh):
            np.add.at(mult[h, i], ra[h, i - 1], 1)
    out = {}
    for prefix, m in (("key", mult), ("query", mult.transpose(0, 2, 1))):
        blocks, mults = np.zeros_like(mult), np.zeros_like(mult)
        count = (m > 0).sum(-1).astype(np.int32)
        for h in range(nh):
            for a in range(nb):
                idx = np.nonzero(m[h, a])[0]
                blocks[h, a, :len(idx)] = idx
                mults[h, a, :len(idx)] = m[h, a, idx]
        out[prefix + "_blocks"], out[prefix + "_mult"], out[prefix + "_count"] = blocks, mults, count
    return out


class BlockSparsePlan:
    """The lists of one plan (bigbird_block_lists) and their device copies, uploaded once per device."""

    NAMES = ("key_blocks", "key_mult", "key_count", "query_blocks", "query_mult", "query_count")

    def __init__(self, num_blocks, rand_attn):
        self.lists = bigbird_block_lists(num_blocks, rand_attn)
        self.num_blocks = int(num_blocks)
        self.num_heads = int(self.lists["key_count"].shape[0])
        self._device = {}

    @classmethod
    def from_lists(cls, lists: dict):
        """A plan from ready-made lists (arrays of the shapes bigbird_block_lists returns); their VALUES are checked on the
        device, by the kernels (an entry out of range sets the error word and block_sparse_attention raises)."""
        self = cls.__new__(cls)
        kc = np.asarray(lists["key_count"])
        if kc.ndim != 2:
            raise ValueError(f"key_count must have shape [num_heads, num_blocks], got {kc.shape}")
        nh, nb = kc.shape
        _check_num_blocks(nb)
        self.lists = {}
        for name in cls.NAMES:
            a = np.ascontiguousarray(lists[name], dtype=np.int32)
            want = (nh, nb) if name.endswith("count") else (nh, nb, nb)
            if a.shape != want:      # (the kernels index a full [NH, nb, nb] / [NH, nb] extent)
                raise ValueError(f"{name} must have shape {want}, got {a.shape}")
            self.lists[name] = a
        self.num_blocks, self.num_heads, self._device = nb, nh, {}
        return self

    def on(self, device):
        """(the six lists, the error word) on `device`."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            tensors = tuple(torch.from_numpy(self.lists[n]).to(device) for n in self.NAMES)
            self._device[device] = (tensors, torch.zeros(1, dtype=torch.int32, device=device))
        return self._device[device]

    def tiles(self):
        """Visited (query block, key block) tiles per head, forward."""
        return self.lists["key_count"].sum(-1)


class _BlockSparseAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, attention_mask, plan, num_heads, scale, flags):
        H = num_heads * BLOCK
        S = plan.num_blocks * BLOCK
        if not qkv.is_cuda:
            raise hip.StonkHipError("block_sparse_attention needs a GPU tensor: there is no CPU path")
        if qkv.dtype != torch.bfloat16 or qkv.dim() != 2 or qkv.shape[1] != 3 * H or not qkv.is_contiguous():
            raise ValueError(f"qkv must be a contiguous bf16 [B*S, {3 * H}] tensor, got {qkv.dtype} {tuple(qkv.shape)}")
        if plan.num_heads != num_heads:
            raise ValueError(f"the plan has {plan.num_heads} heads, the call {num_heads}")
        if qkv.shape[0] % S:
            raise ValueError(f"{qkv.shape[0]} rows are no multiple of the plan's sequence length {S}")
        B = qkv.shape[0] // S
        if attention_mask is not None:
            if attention_mask.shape != (B, S):
                raise ValueError(f"attention_mask must have shape {(B, S)}, got {tuple(attention_mask.shape)}")
            attention_mask = attention_mask.to(device=qkv.device, dtype=torch.int64).contiguous()
        lists, err = plan.on(qkv.device)
        out = torch.empty(B * S, H, device=qkv.device, dtype=torch.bfloat16)
        lse = torch.empty(B, num_heads, S, device=qkv.device, dtype=torch.float32)
        p = hip.ptr(qkv)
        hip.call("stonk_block_sparse_attention_fwd_ex", p, p + 2 * H, p + 4 * H, 3 * H, hip.ptr(attention_mask),
                 *(hip.ptr(t) for t in lists[:3]), hip.ptr(out), H, hip.ptr(lse), B, num_heads, S, BLOCK, scale, hip.ptr(err),
                 flags, hip.stream_ptr())
        if int(err.item()):
            err.zero_()
            raise IndexError("block_sparse_attention: a list entry, multiplicity or count of the plan is out of range")
        ctx.save_for_backward(qkv, attention_mask, out, lse)
        ctx.plan, ctx.num_heads, ctx.scale, ctx.flags = plan, num_heads, scale, flags
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, attention_mask, out, lse = ctx.saved_tensors
        num_heads, scale, plan = ctx.num_heads, ctx.scale, ctx.plan
        H = num_heads * BLOCK
        B, _, S = lse.shape
        dout = dout.to(torch.bfloat16).contiguous()
        lists, err = plan.on(qkv.device)
        dqkv = torch.empty_like(qkv)
        ws = torch.empty(2, B, num_heads, S, device=qkv.device, dtype=torch.float32)
        p, g = hip.ptr(qkv), hip.ptr(dqkv)
        hip.call("stonk_block_sparse_attention_bwd_ex", p, p + 2 * H, p + 4 * H, 3 * H, hip.ptr(attention_mask),
                 *(hip.ptr(t) for t in lists), hip.ptr(out), H, hip.ptr(dout), H, hip.ptr(lse), hip.ptr(ws), g, g + 2 * H, 3 * H,
                 g + 4 * H, B, num_heads, S, BLOCK, scale, hip.ptr(err), ctx.flags, hip.stream_ptr())
        return dqkv, None, None, None, None, None


def block_sparse_attention(qkv, attention_mask, plan, num_heads, scale=None, zero_masked_queries=False):
    """softmax over the plan's listed key blocks (with multiplicities) . V, per head.

    zero_masked_queries: HuggingFace's ``context_layer * from_mask`` (modeling_big_bird.py:617) - the output row of a
    position whose own mask word is 0 is exact zeros and no gradient passes through it (STONK_BSA_ZERO_MASKED_QUERIES, applied
    inside the kernels). Off, such a row is the list formulation's row.

    qkv: bf16 [B*S, 3H] contiguous (q | k | v, head h at columns h*64..), S = 64 * plan.num_blocks; attention_mask int64
    [B, S] (0 = masked key) or None; returns bf16 [B*S, H]. Differentiable with respect to qkv. Raises IndexError when the
    kernels find a list entry out of range (one device-to-host word per call, as Engine.check_errors reads)."""
    if scale is None:
        scale = 1.0 / math.sqrt(BLOCK)
    flags = hip.BSA_ZERO_MASKED_QUERIES if zero_masked_queries else 0
    return _BlockSparseAttention.apply(qkv, attention_mask, plan, int(num_heads), float(scale), flags)


class BigBirdBlockSparseSelfAttention(nn.Module):
    """Stands in for HuggingFace's BigBirdBlockSparseAttention (block size 64, head dimension 64): the same ``query`` / ``key`` /
    ``value`` linears, so ``load_state_dict`` takes its state dict unchanged. What "drop-in" means depends on
    ``zero_masked_queries``: True, every row is HuggingFace's - the context row of a position whose own mask word is 0 is exact
    zeros (its ``context_layer * from_mask``, :617) and takes no gradient; False (the default), only the rows whose own mask
    word is 1 are HuggingFace's, and a masked position's row is the list formulation's row (its block's softmax over the live
    listed keys), which HuggingFace never returns. The projections run in torch in bf16; the
    attention is block_sparse_attention. ``.eval()`` uses the zeros plan, ``.train()`` a plan drawn once per module from
    ``layer_seed`` (HuggingFace's is fixed per layer by its seed as well, but from another random stream). No dropout and no
    attention-probability output."""

    def __init__(self, hidden_size, num_heads, num_random_blocks=3, layer_seed=0, zero_masked_queries=False):
        super().__init__()
        if hidden_size != num_heads * BLOCK:
            raise ValueError(f"hidden_size must be num_heads * {BLOCK}: the kernels are built for head dimension {BLOCK}")
        self.hidden_size, self.num_heads = int(hidden_size), int(num_heads)
        self.num_random_blocks, self.layer_seed = int(num_random_blocks), int(layer_seed)
        self.zero_masked_queries = bool(zero_masked_queries)
        self.query = nn.Linear(hidden_size, hidden_size, bias=True)
        self.key = nn.Linear(hidden_size, hidden_size, bias=True)
        self.value = nn.Linear(hidden_size, hidden_size, bias=True)
        self._plans = {}

    def plan_for(self, num_blocks) -> BlockSparsePlan:
        """The plan of the module's current mode at this sequence length (built once)."""
        key = (int(num_blocks), bool(self.training))
        if key not in self._plans:
            ra = bigbird_rand_attn(num_blocks, self.num_random_blocks, self.num_heads, "train" if self.training else "eval",
                                   seed=self.layer_seed)
            self._plans[key] = BlockSparsePlan(num_blocks, ra)
        return self._plans[key]

    def project(self, hidden_states):
        """q | k | v of hidden_states [B, S, H]: bf16 [B*S, 3H], what the attention kernels read."""
        B, S, H = hidden_states.shape
        w = torch.cat([self.query.weight, self.key.weight, self.value.weight], 0).to(torch.bfloat16)
        bias = torch.cat([self.query.bias, self.key.bias, self.value.bias], 0).to(torch.bfloat16)
        return nn.functional.linear(hidden_states.reshape(B * S, H).to(torch.bfloat16), w, bias)

    def forward(self, hidden_states, attention_mask=None):
        B, S, H = hidden_states.shape
        if H != self.hidden_size or S % BLOCK:
            raise ValueError(f"hidden_states must be [B, S, {self.hidden_size}] with S a multiple of {BLOCK}, got {tuple(hidden_states.shape)}")
        hip.lib()   # (raises if the library has not been built)
        ctx = block_sparse_attention(self.project(hidden_states), attention_mask, self.plan_for(S // BLOCK), self.num_heads,
                                     zero_masked_queries=self.zero_masked_queries)
        return ctx.view(B, S, H).to(hidden_states.dtype)
