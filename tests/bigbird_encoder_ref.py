"""Reference, cases and fixtures' readers of the BigBird encoder tests (test_bigbird_encoder_gpu.py,
test_bigbird_encoder_ref_cpu.py, test_bigbird_encoder_cpu.py; tools/make_bigbird_encoder_golden.py writes the fixtures).

The encoder of hf:models/big_bird/modeling_big_bird.py BigBirdModel (block-sparse attention, inputs_embeds in), restated on
the CPU from a HuggingFace-layout state dict:

    e   = inputs_embeds + token_type_embeddings[tt] + position_embeddings[:S]          (dropout 0)
    x   = LayerNorm(e)
    per layer:  qkv = x W_qkv^T + b     ctx = list-form block-sparse attention (tests/bigbird_ref.compute) o from_mask
                h1 = LayerNorm(ctx W_o^T + b + x)     g = gelu_new(h1 W_i^T + b)     x = LayerNorm(g W_d^T + b + h1)
    pooled = tanh(x[:, 0] W_p^T + b)

in three modes: "r64" (float64: the reference r), "r32" (float32) and "r16" (float32 with the kernels' bf16 rounding points:
every activation a kernel stores in bf16 is rounded where it is stored - and, in the backward, the gradient that flows through
the same point is rounded too, since the kernels keep their gradient activations in bf16 as well; the attention is
bigbird_ref's own r16, tile order included). Gradients come from torch autograd over the restatement; the attention is one
autograd Function over bigbird_ref.compute (its out, and its dq / dk / dv for a given dout).

`zero_masked_queries=False` and `act="gelu"` are the two MUTANTS the tests must be able to tell from the feature: today's
kernels' rule for a masked query (the list formulation's row), and BERT's erf GELU.

The fixed scalar of the gradient checks: sum(w o seq) + sum(w' o pooled), w / w' seeded normals (`loss_weights`).
Weights and inputs_embeds are bf16-exact and regenerated from seeds (the fixtures hold checksums, masks, HuggingFace's
plans and HuggingFace's float32 results)."""
import functools
import hashlib
import json
import math
import os

import numpy as np
import torch

from tests import bigbird_ref as br

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GELU_NEW_C = math.sqrt(2.0 / math.pi)
BF16_MAX = 3.3895313892515355e38
TAIL_IN_STD, TAIL_BIAS_MEAN, TAIL_BIAS_STD, TAIL_OUT_STD = 0.04, -4.5, 0.3, 32.0     # init_state_dict's tail units
# What HuggingFace's FLOAT32 run (the fixtures) may be off by, relative norm, from its own arithmetic: its NewGELU forms
# 1 + tanh(a) in float32, one ulp of 1 = 2^-24 off in absolute terms, so a tail unit's value 0.5 u (1 + tanh) is off by about
# 0.5 * 4.5 * 2^-24 = 1.3e-7; 128 such units through output weights of size 32 add up to sqrt(128) * 32 * 1.3e-7 = 5e-5 on a
# feed-forward output of size 1. Ten times that for two layers, the LayerNorms' gain and the backward: 5e-4 - a sixtieth of
# what the erf mutant misses by, a twentieth of the GPU bound.
HF_FLOAT32_ERROR = 5e-4


# ------------------------------------------------------------------ cases
def _mask(B, S, edits):
    m = torch.ones(B, S, dtype=torch.long)
    for b, lo, hi in edits:
        m[b, lo:hi] = 0
    return m


def _case(name, S, B, L, edits, seed):
    return dict(name=name, S=S, B=B, nb=S // 64, hidden=128, heads=2, layers=L, inter=256, mask=_mask(B, S, edits), seed=seed,
                type_split=S // 2)


# masked positions: inside a block, a whole inner block, in block 0, in block nb - 1 (position 0, the pooler's row, stays live)
CASES = {c["name"]: c for c in (
    _case("s768", 768, 2, 2, [(0, 3, 9), (0, 200, 230), (0, 320, 384), (1, 768 - 100, 768)], 41),
    _case("s1024", 1024, 2, 2, [(0, 5, 20), (0, 130, 140), (0, 448, 512), (0, 1000, 1024), (1, 1024 - 150, 1024)], 42),
    _case("s4096", 4096, 1, 1, [(0, 2, 7), (0, 700, 760), (0, 1024, 1088), (0, 4096 - 300, 4096)], 43),
)}
MODES = ("eval", "train")     # train: dropout 0, HuggingFace's train-mode plans


def case_modes(name):
    """The modes a case has a fixture for (the 4096-token case: the eval plan only)."""
    return ("eval",) if name == "s4096" else MODES


def config_dict(c):
    """hf BigBirdConfig keyword arguments of a case (dropout 0: the fixtures' train mode differs by its plans only)."""
    return dict(vocab_size=64, hidden_size=c["hidden"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                intermediate_size=c["inter"], hidden_act="gelu_new", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                max_position_embeddings=4096, type_vocab_size=2, layer_norm_eps=1e-12, attention_type="block_sparse",
                use_bias=True, rescale_embeddings=False, block_size=64, num_random_blocks=3)


def grad_names(c):
    """(no key bias: a softmax does not see a shift common to all its keys - that gradient is zero up to rounding)"""
    last = c["layers"] - 1
    return ["encoder.layer.0.attention.self.query.weight", "encoder.layer.0.attention.self.value.bias",
            f"encoder.layer.{last}.attention.self.value.weight", "encoder.layer.0.attention.output.dense.weight",
            f"encoder.layer.{last}.intermediate.dense.weight", f"encoder.layer.{last}.output.dense.bias",
            "encoder.layer.0.output.LayerNorm.weight", "embeddings.LayerNorm.bias", "embeddings.token_type_embeddings.weight",
            "embeddings.position_embeddings.weight", "pooler.weight"]


# ------------------------------------------------------------------ seeded, bf16-exact data
def _bf_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def init_state_dict(cfg: dict, seed: int):
    """A state dict in hf BigBirdModel's key layout, float32 values that bf16 holds exactly (the GEMMs' bf16 mirrors then
    equal the masters): matrices N(0, 0.08), biases N(0, 0.05), LayerNorm weights 1 + N(0, 0.1).

    The second half of every layer's intermediate units are TAIL units: input weights N(0, 0.04), bias N(-4.5, 0.3), output
    weights N(0, 32). Their pre-activations sit at -4.5 +- 0.6, where gelu_new and the erf GELU differ by a factor (at
    u = -4.5: -4.7e-6 against -1.5e-5) while both are tiny; the output weights are sized so that this tail carries as much of
    the feed-forward branch as the ordinary units do. An activation that is the wrong FORM then moves the encoder's output by
    more than bf16 rounding does, which ordinary units alone cannot show (the two forms differ by at most 4.7e-4 where one
    rounding of their value is 2e-3): tests/test_bigbird_encoder_ref_cpu.py measures both."""
    g = torch.Generator().manual_seed(seed)
    H, I = cfg["hidden_size"], cfg["intermediate_size"]

    def mat(*shape, std=0.08):
        return _bf_exact(torch.randn(*shape, generator=g) * std)

    sd = {"embeddings.word_embeddings.weight": mat(cfg["vocab_size"], H),
          "embeddings.position_embeddings.weight": mat(cfg["max_position_embeddings"], H, std=0.3),
          "embeddings.token_type_embeddings.weight": mat(cfg["type_vocab_size"], H, std=0.3),
          "embeddings.LayerNorm.weight": _bf_exact(1.0 + 0.1 * torch.randn(H, generator=g)),
          "embeddings.LayerNorm.bias": mat(H, std=0.05)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        for lin, (o, n) in (("attention.self.query", (H, H)), ("attention.self.key", (H, H)), ("attention.self.value", (H, H)),
                            ("attention.output.dense", (H, H)), ("intermediate.dense", (I, H)), ("output.dense", (H, I))):
            sd[p + lin + ".weight"] = mat(o, n)
            sd[p + lin + ".bias"] = mat(o, std=0.05)
        t = I // 2      # the tail units
        sd[p + "intermediate.dense.weight"][t:] = mat(I - t, H, std=TAIL_IN_STD)
        sd[p + "intermediate.dense.bias"][t:] = _bf_exact(TAIL_BIAS_MEAN + TAIL_BIAS_STD * torch.randn(I - t, generator=g))
        sd[p + "output.dense.weight"][:, t:] = mat(H, I - t, std=TAIL_OUT_STD)
        for ln in ("attention.output.LayerNorm", "output.LayerNorm"):
            sd[p + ln + ".weight"] = _bf_exact(1.0 + 0.1 * torch.randn(H, generator=g))
            sd[p + ln + ".bias"] = mat(H, std=0.05)
    sd["pooler.weight"] = mat(H, H)
    sd["pooler.bias"] = mat(H, std=0.05)
    return sd


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(state dict, inputs_embeds fp32 [B, S, H] bf16-exact, token_type_ids [B, S], (w [B, S, H], w' [B, H])) of a case."""
    c = CASES[name]
    sd = init_state_dict(config_dict(c), c["seed"])
    g = torch.Generator().manual_seed(c["seed"] + 1000)
    x = _bf_exact(torch.randn(c["B"], c["S"], c["hidden"], generator=g))
    tt = torch.zeros(c["B"], c["S"], dtype=torch.long)
    tt[:, c["type_split"]:] = 1
    w = torch.randn(c["B"], c["S"], c["hidden"], generator=g)
    wp = torch.randn(c["B"], c["hidden"], generator=g)
    return sd, x, tt, (w, wp)


def checksum(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def data_checksum(name):
    sd, x, tt, (w, wp) = case_data(name)
    return checksum([sd[k] for k in sorted(sd)] + [x, tt, w, wp])


def sample_rows(c):
    """The rows of [B*S] whose sequence output the fixtures keep: every 37th, and every masked-query row."""
    keep = torch.zeros(c["B"] * c["S"], dtype=torch.bool)
    keep[::37] = True
    keep |= c["mask"].view(-1) == 0
    return keep


def grad_rows(c):
    """The rows whose d(inputs_embeds) the fixtures keep: every 37th, and every 8th masked-query row."""
    keep = torch.zeros(c["B"] * c["S"], dtype=torch.bool)
    keep[::37] = True
    masked = torch.nonzero(c["mask"].view(-1) == 0).view(-1)
    keep[masked[::8]] = True
    return keep


def grad_sample(g):
    """What the fixtures keep of a parameter gradient: every 7th row of a matrix of more than 32 rows, else all of it."""
    return g[::7] if g.dim() == 2 and g.shape[0] > 32 else g


# ------------------------------------------------------------------ fixtures
def load_fixture(name):
    """The fixture of a case: dict(meta=json, plus per mode: plans [L][NH, nb-2, r] and HuggingFace's float32 results)."""
    with open(os.path.join(GOLDEN, f"g18_bigbird_{name}.json")) as fh:
        meta = json.load(fh)
    z = np.load(os.path.join(GOLDEN, f"g18_bigbird_{name}.npz"))
    return dict(meta=meta, arrays={k: z[k] for k in z.files})


def fixture_plans(fx, mode):
    return [fx["arrays"][f"{mode}.plan.{i}"] for i in range(fx["meta"]["layers"])]


# ------------------------------------------------------------------ HuggingFace itself
def huggingface_run(name, mode, dtype=torch.float32):
    """hf BigBirdModel on a case, on the CPU in `dtype` (needs `transformers`): dict(seq, pooled, loss, grads = {name: tensor}
    with "inputs_embeds", plans = the rand_attn [NH, nb - 2, r] each layer actually used - the argument its attention hands
    to _create_rand_mask_from_inputs)."""
    from transformers.models.big_bird.modeling_big_bird import BigBirdConfig, BigBirdModel

    c = CASES[name]
    sd, x, tt, (w, wp) = case_data(name)
    model = BigBirdModel(BigBirdConfig(**config_dict(c)))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    model = model.to(dtype)
    model.train(mode == "train")
    used = {}
    for i, layer in enumerate(model.encoder.layer):
        attn = layer.attention.self
        inner = attn._create_rand_mask_from_inputs

        def spy(from_blocked_mask, to_blocked_mask, rand_attn, *a, _i=i, _inner=inner, **k):
            assert bool((rand_attn == rand_attn[:1]).all())      # the same for every sequence
            used[_i] = rand_attn[0].detach().cpu().numpy().astype(np.int32)
            return _inner(from_blocked_mask, to_blocked_mask, rand_attn, *a, **k)

        attn._create_rand_mask_from_inputs = spy
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    out = model(inputs_embeds=xin, attention_mask=c["mask"], token_type_ids=tt)
    assert model.encoder.layer[0].attention.attention_type == "block_sparse"     # (no silent switch to full attention)
    seq, pooled = out.last_hidden_state, out.pooler_output
    assert seq.shape == x.shape
    loss = (w.to(dtype) * seq).sum() + (wp.to(dtype) * pooled).sum()
    loss.backward()
    params = dict(model.named_parameters())
    grads = {"inputs_embeds": xin.grad, **{k: params[k].grad for k in grad_names(c)}}
    return dict(seq=seq.detach(), pooled=pooled.detach(), loss=loss.detach(), grads=grads,
                plans=[used[i] for i in range(c["layers"])])


# ------------------------------------------------------------------ the restatement
def gelu_new(u):
    """0.5 u (1 + tanh(a)), a = c (u + 0.044715 u^3), written as u * sigmoid(2a) - the same function, without the
    cancellation of 1 + tanh on the negative side (in float32 that form has lost every digit by u = -4)."""
    return u * torch.sigmoid(2.0 * GELU_NEW_C * (u + 0.044715 * u ** 3))


def gelu_new_grad(u):
    """The issue's closed form, evaluated so that it is finite for every finite u: the second term is dropped where 1 - t^2
    has underflowed to 0 (there u (1 + 3 k u^2) may be inf)."""
    t = torch.tanh(GELU_NEW_C * (u + 0.044715 * u ** 3))
    sech2 = 1.0 - t * t
    poly = GELU_NEW_C * (1.0 + 3 * 0.044715 * u * u)
    second = torch.where(sech2 == 0, torch.zeros_like(u), 0.5 * u * sech2 * poly)
    return 0.5 * (1.0 + t) + second


class _RoundBoth(torch.autograd.Function):
    """A bf16 storage point: the value is rounded on the way forward, the gradient on the way back."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class _ListAttention(torch.autograd.Function):
    """tests/bigbird_ref.compute as an autograd op on qkv [T, 3H] -> out [T, H]."""

    @staticmethod
    def forward(ctx, qkv, c, lists, mode):
        ctx.c, ctx.lists, ctx.mode = c, lists, mode
        ctx.save_for_backward(qkv)
        dt = qkv.dtype
        res = br.compute(c, lists, qkv.detach(), torch.zeros(c["T"], c["NH"] * 64, dtype=dt), mode)
        return res["out"].to(dt)

    @staticmethod
    def backward(ctx, dout):
        (qkv,) = ctx.saved_tensors
        res = br.compute(ctx.c, ctx.lists, qkv.detach(), dout, ctx.mode)
        return torch.cat([res["dq"], res["dk"], res["dv"]], 1).to(qkv.dtype), None, None, None


def _layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def encoder(sd, cfg, inputs_embeds, mask, token_type_ids, plans, mode, zero_masked_queries=True, act="gelu_new",
            loss_w=None, grads=()):
    """The restatement. sd: HuggingFace-layout state dict; cfg: config_dict(); plans: per layer rand_attn [NH, nb-2, r];
    mode "r64" / "r32" / "r16". Returns dict(seq [B, S, H], pooled [B, H]) and, with `loss_w` = (w, w'), the gradients of
    sum(w o seq) + sum(w' o pooled): "inputs_embeds" and every state-dict name in `grads`."""
    from stonkgs_amd.bigbird_attention import bigbird_block_lists

    dt = torch.float64 if mode == "r64" else torch.float32
    rb = _RoundBoth.apply if mode == "r16" else (lambda t: t)
    B, S, H = inputs_embeds.shape
    NH, nb, eps = cfg["num_attention_heads"], S // 64, cfg["layer_norm_eps"]
    P = {k: v.detach().to(dt).clone().requires_grad_(k in grads) for k, v in sd.items()}
    x_in = inputs_embeds.detach().to(dt).clone().requires_grad_(loss_w is not None)
    tt = torch.zeros(B, S, dtype=torch.long) if token_type_ids is None else token_type_ids
    c = dict(B=B, NH=NH, S=S, nb=nb, T=B * S, scale=0.125, mask=mask)
    live = torch.ones(B * S, 1, dtype=dt) if mask is None else (mask.view(-1, 1) != 0).to(dt)

    e = x_in + P["embeddings.token_type_embeddings.weight"][tt]
    e = e + P["embeddings.position_embeddings.weight"][:S]
    x = rb(_layer_norm(e, P["embeddings.LayerNorm.weight"], P["embeddings.LayerNorm.bias"], eps)).view(B * S, H)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        wqkv = torch.cat([P[p + f"attention.self.{n}.weight"] for n in ("query", "key", "value")], 0)
        bqkv = torch.cat([P[p + f"attention.self.{n}.bias"] for n in ("query", "key", "value")], 0)
        qkv = rb(x @ wqkv.T + bqkv)
        ctx = _ListAttention.apply(qkv, c, bigbird_block_lists(nb, plans[i]), mode)
        if zero_masked_queries:
            ctx = ctx * live
        s1 = rb(ctx @ P[p + "attention.output.dense.weight"].T + P[p + "attention.output.dense.bias"] + x)
        h1 = rb(_layer_norm(s1, P[p + "attention.output.LayerNorm.weight"], P[p + "attention.output.LayerNorm.bias"], eps))
        u = rb(h1 @ P[p + "intermediate.dense.weight"].T + P[p + "intermediate.dense.bias"])
        g = rb(gelu_new(u) if act == "gelu_new" else torch.nn.functional.gelu(u))
        s2 = rb(g @ P[p + "output.dense.weight"].T + P[p + "output.dense.bias"] + h1)
        x = rb(_layer_norm(s2, P[p + "output.LayerNorm.weight"], P[p + "output.LayerNorm.bias"], eps))
    seq = x.view(B, S, H)
    pooled = torch.tanh(seq[:, 0] @ P["pooler.weight"].T + P["pooler.bias"])
    out = dict(seq=seq.detach(), pooled=pooled.detach())
    if loss_w is not None:
        w, wp = loss_w
        loss = (w.to(dt) * seq).sum() + (wp.to(dt) * pooled).sum()
        loss.backward()
        out["loss"] = loss.detach()
        out["grads"] = {"inputs_embeds": x_in.grad, **{k: P[k].grad for k in grads}}
    return out


@functools.lru_cache(maxsize=None)
def reference(name, mode_name, mode, zero_masked_queries=True, act="gelu_new"):
    """encoder() for a case with the fixture's plans of `mode_name` ("eval" / "train"), gradients included; made once."""
    c = CASES[name]
    sd, x, tt, lw = case_data(name)
    plans = fixture_plans(load_fixture(name), mode_name)
    return encoder(sd, config_dict(c), x, c["mask"], tt, plans, mode, zero_masked_queries, act, loss_w=lw,
                   grads=tuple(grad_names(c)))


def rel(a, r):
    """||a - r|| / ||r|| in float64."""
    a, r = a.detach().double().cpu(), r.detach().double().cpu()
    return float((a - r).norm() / r.norm())
