"""The BigBird encoder's host side without a GPU: the new launchers' refusals through the C ABI (they happen before any
launch; the library loads without a GPU), symbol registration, the state-dict key mapping in both layouts, config and
sequence-length validation, and a BlockSparsePlan from a fixture's rand_attn."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from stonkgs_amd import _hip
from stonkgs_amd import bigbird_encoder as be
from stonkgs_amd.bigbird_attention import BlockSparsePlan
from tests import bigbird_encoder_ref as er

P = 0x10000      # (never dereferenced: every call below is refused, or returns for an empty launch, before any launch)
NEW = ("stonk_block_sparse_attention_fwd_ex", "stonk_block_sparse_attention_bwd_ex", "stonk_gelu_new_fwd_bf16",
       "stonk_gelu_new_bwd_bf16", "stonk_embeds_ln_fwd", "stonk_embeds_ln_bwd_finish")


def test_symbols_are_registered_and_the_abi_number_stays():
    lib = _hip.lib()
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "stonk_hip.h")).read()
    for name in NEW:
        assert name in _hip._SIGNATURES and name in _hip.exported_symbols() and hasattr(lib, name)
        assert f"int {name}(" in header
    assert lib.stonk_abi_version() == 5
    vp, i32, i64, f32, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint32
    old = _hip._SIGNATURES
    for sfx in ("fwd", "bwd"):      # today's signatures plus `int flags` in front of the stream
        base = old["stonk_block_sparse_attention_" + sfx]
        assert old[f"stonk_block_sparse_attention_{sfx}_ex"] == base[:-1] + [i32, vp]
    assert old["stonk_gelu_new_fwd_bf16"] == [vp, vp, i64, vp] and old["stonk_gelu_new_bwd_bf16"] == [vp, vp, vp, i64, vp]
    assert old["stonk_embeds_ln_fwd"] == [vp, i64] + [vp] * 9 + [i32] * 4 + [f32, f32, u32, vp]
    assert old["stonk_embeds_ln_bwd_finish"] == [vp, i64, vp, i64, vp, i64, i32, f32, u32, vp]
    flags = open(os.path.join(_hip._HERE, "csrc", "stonk_flags.h")).read()
    assert "#define STONK_BSA_ZERO_MASKED_QUERIES (1 << 0)" in flags and _hip.BSA_ZERO_MASKED_QUERIES == 1


# ------------------------------------------------------------------ block-sparse _ex entries
def _fwd_ex(**kw):
    a = dict(q=P, k=P + 256, v=P + 512, ld=384, mask=P, kb=P, km=P, kc=P, out=P, ldo=128, lse=P, B=1, NH=2, S=384, D=64,
             scale=0.125, err=P, flags=_hip.BSA_ZERO_MASKED_QUERIES, stream=0)
    a.update(kw)
    return [a[k] for k in ("q", "k", "v", "ld", "mask", "kb", "km", "kc", "out", "ldo", "lse", "B", "NH", "S", "D", "scale", "err",
                           "flags", "stream")]


def _bwd_ex(**kw):
    a = dict(q=P, k=P + 256, v=P + 512, ld=384, mask=P, kb=P, km=P, kc=P, qb=P, qm=P, qc=P, out=P, ldo=128, dout=P, lddo=128,
             lse=P, ws=P, dq=P, dk=P + 256, ldd=384, dv=P + 512, B=1, NH=2, S=384, D=64, scale=0.125, err=P,
             flags=_hip.BSA_ZERO_MASKED_QUERIES, stream=0)
    a.update(kw)
    return [a[k] for k in ("q", "k", "v", "ld", "mask", "kb", "km", "kc", "qb", "qm", "qc", "out", "ldo", "dout", "lddo", "lse", "ws",
                           "dq", "dk", "ldd", "dv", "B", "NH", "S", "D", "scale", "err", "flags", "stream")]


EX_REFUSALS = [(dict(flags=2), _hip.EINVAL), (dict(flags=-1), _hip.EINVAL), (dict(flags=3), _hip.EINVAL),
               (dict(D=32), _hip.ESHAPE), (dict(S=256), _hip.ESHAPE), (dict(S=4160), _hip.ESHAPE), (dict(S=400), _hip.ESHAPE),
               (dict(ld=128), _hip.ESHAPE), (dict(ld=388), _hip.EALIGN), (dict(q=0), _hip.EINVAL), (dict(err=0), _hip.EINVAL),
               (dict(out=0), _hip.EINVAL), (dict(scale=0.0), _hip.EINVAL), (dict(q=P + 8), _hip.EALIGN)]


@pytest.mark.parametrize("kw,code", EX_REFUSALS, ids=[f"{next(iter(k))}={next(iter(k.values()))}" for k, _ in EX_REFUSALS])
def test_ex_entries_refuse_what_the_old_ones_refuse_and_unknown_flags(kw, code):
    lib = _hip.lib()
    assert lib.stonk_block_sparse_attention_fwd_ex(*_fwd_ex(**kw)) == code
    assert lib.stonk_block_sparse_attention_bwd_ex(*_bwd_ex(**kw)) == code


def test_ex_entries_empty_batch_and_flag_without_mask():
    lib = _hip.lib()
    for flags in (0, _hip.BSA_ZERO_MASKED_QUERIES):
        for mask in (0, P):      # (the flag without a mask is accepted: every query is live)
            assert lib.stonk_block_sparse_attention_fwd_ex(*_fwd_ex(B=0, flags=flags, mask=mask)) == _hip.OK
            assert lib.stonk_block_sparse_attention_bwd_ex(*_bwd_ex(B=0, flags=flags, mask=mask)) == _hip.OK
    for name in ("qb", "dout", "ws", "dv"):
        assert lib.stonk_block_sparse_attention_bwd_ex(*_bwd_ex(**{name: 0})) == _hip.EINVAL


# ------------------------------------------------------------------ gelu_new
def test_gelu_new_refusals():
    lib = _hip.lib()
    f, b = lib.stonk_gelu_new_fwd_bf16, lib.stonk_gelu_new_bwd_bf16
    assert f(P, P, 0, 0) == _hip.OK and b(P, P, P, 0, 0) == _hip.OK
    assert f(0, P, 8, 0) == _hip.EINVAL and f(P, 0, 8, 0) == _hip.EINVAL
    assert b(0, P, P, 8, 0) == _hip.EINVAL and b(P, 0, P, 8, 0) == _hip.EINVAL and b(P, P, 0, 8, 0) == _hip.EINVAL
    assert f(P, P, 12, 0) == _hip.EINVAL and b(P, P, P, 12, 0) == _hip.EINVAL and f(P, P, -8, 0) == _hip.EINVAL
    assert f(P + 8, P, 8, 0) == _hip.EALIGN and f(P, P + 2, 8, 0) == _hip.EALIGN
    assert b(P + 8, P, P, 8, 0) == _hip.EALIGN and b(P, P + 8, P, 8, 0) == _hip.EALIGN and b(P, P, P + 8, 8, 0) == _hip.EALIGN


# ------------------------------------------------------------------ embeddings
def _emb_fwd(**kw):
    a = dict(x=P, ld=128, tt=0, pos=P, typ=P, gamma=P, beta=P, sum_out=P, y=P, mean=P, rstd=P, B=1, S=768, H=128, types=2,
             eps=1e-12, p=0.1, seed=1, stream=0)
    a.update(kw)
    return [a[k] for k in ("x", "ld", "tt", "pos", "typ", "gamma", "beta", "sum_out", "y", "mean", "rstd", "B", "S", "H", "types",
                           "eps", "p", "seed", "stream")]


def _emb_bwd(**kw):
    a = dict(dsum=P, ld=128, d_in=P, ld_out=128, dxm=P, rows=768, H=128, p=0.1, seed=1, stream=0)
    a.update(kw)
    return [a[k] for k in ("dsum", "ld", "d_in", "ld_out", "dxm", "rows", "H", "p", "seed", "stream")]


def test_embeds_ln_refusals():
    lib = _hip.lib()
    f = lib.stonk_embeds_ln_fwd
    assert f(*_emb_fwd(B=0)) == _hip.OK
    for name in ("x", "pos", "typ", "gamma", "beta", "sum_out", "y", "mean", "rstd"):
        assert f(*_emb_fwd(**{name: 0})) == _hip.EINVAL, name
    for kw, code in ((dict(p=1.0), _hip.EINVAL), (dict(p=-0.1), _hip.EINVAL), (dict(H=132), _hip.ESHAPE), (dict(H=1032), _hip.ESHAPE),
                     (dict(H=0), _hip.ESHAPE), (dict(ld=120), _hip.ESHAPE), (dict(S=0), _hip.ESHAPE), (dict(B=-1), _hip.ESHAPE),
                     (dict(types=0), _hip.ESHAPE), (dict(ld=130), _hip.EALIGN), (dict(x=P + 4), _hip.EALIGN),
                     (dict(y=P + 8), _hip.EALIGN), (dict(sum_out=P + 8), _hip.EALIGN), (dict(gamma=P + 4), _hip.EALIGN),
                     (dict(B=0, H=132), _hip.ESHAPE)):
        assert f(*_emb_fwd(**kw)) == code, kw
    assert f(*_emb_fwd(B=0, H=1024, ld=1028)) == _hip.OK


def test_embeds_ln_bwd_finish_refusals():
    lib = _hip.lib()
    f = lib.stonk_embeds_ln_bwd_finish
    assert f(*_emb_bwd(rows=0)) == _hip.OK
    for name in ("dsum", "d_in", "dxm"):
        assert f(*_emb_bwd(**{name: 0})) == _hip.EINVAL, name
    for kw, code in ((dict(p=1.0), _hip.EINVAL), (dict(H=132), _hip.ESHAPE), (dict(H=2048, ld=2048, ld_out=2048), _hip.ESHAPE),
                     (dict(ld=120), _hip.ESHAPE), (dict(ld_out=64), _hip.ESHAPE), (dict(rows=-1), _hip.ESHAPE),
                     (dict(ld=132), _hip.EALIGN), (dict(ld_out=130), _hip.EALIGN), (dict(dsum=P + 8), _hip.EALIGN),
                     (dict(d_in=P + 4), _hip.EALIGN), (dict(dxm=P + 8), _hip.EALIGN)):
        assert f(*_emb_bwd(**kw)) == code, kw


# ------------------------------------------------------------------ state-dict keys
def test_state_dict_key_mapping_in_both_layouts():
    cfg = be.BigBirdEncoderConfig(**er.config_dict(er.CASES["s768"]))
    keys = be.encoder_keys(cfg)
    sd = er.init_state_dict(er.config_dict(er.CASES["s768"]), 1)
    assert sorted(keys) == sorted(sd) and be.WORD in keys
    meta = {k: torch.empty(v.shape, device="meta") for k, v in sd.items()}
    plain, ignored = be.map_state_dict({**meta, "embeddings.position_ids": torch.empty(1, 4096, device="meta")})
    assert sorted(plain) == sorted(keys) and ignored == ["embeddings.position_ids"]
    assert all(plain[k] is meta[k] for k in keys)
    extra = {"cls.predictions.bias": torch.empty(3), "cls.seq_relationship.weight": torch.empty(2, 4),
             "lm_backbone.encoder.layer.0.output.dense.bias": torch.empty(4), "prot_backbone.pooler.dense.weight": torch.empty(4, 4),
             "bert.embeddings.position_ids": torch.empty(1, 8)}
    pref, ignored = be.map_state_dict({**{"bert." + k: v for k, v in meta.items()}, **extra})
    assert sorted(pref) == sorted(keys) and sorted(ignored) == sorted(extra)
    assert all(pref[k] is meta[k] for k in keys)
    # a plain-layout dict with a foreign key keeps it: load_state_dict(strict=True) then names it as unexpected
    odd, ignored = be.map_state_dict({**meta, "classifier.weight": torch.empty(2, 2)})
    assert "classifier.weight" in odd and not ignored


# ------------------------------------------------------------------ config
def test_config_defaults_are_huggingfaces_and_validation_refuses_the_rest():
    cfg = be.BigBirdEncoderConfig()
    want = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=4096,
                type_vocab_size=2, block_size=64, num_random_blocks=3, hidden_act="gelu_new", layer_norm_eps=1e-12,
                hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, rescale_embeddings=False, attention_type="block_sparse")
    assert all(getattr(cfg, k) == v for k, v in want.items())
    try:
        from transformers import BigBirdConfig

        hf = BigBirdConfig()
        assert all(getattr(hf, k) == getattr(cfg, k) for k in list(want) + ["vocab_size", "use_bias", "initializer_range"])
        assert be.BigBirdEncoderConfig.from_any(hf) == cfg
    except ImportError:
        pass
    cfg.validate_for_hip()
    for kw, what in ((dict(num_attention_heads=8), "head_dim"), (dict(block_size=32), "block_size"),
                     (dict(rescale_embeddings=True), "rescale_embeddings"), (dict(attention_type="original_full"), "attention_type"),
                     (dict(hidden_act="gelu"), "hidden_act"), (dict(hidden_act="relu"), "hidden_act")):
        with pytest.raises(ValueError, match=what):
            be.BigBirdEncoderConfig(**kw).validate_for_hip()


def test_sequence_lengths_704_and_800_are_refused_with_their_reasons(tmp_path):
    cfg = be.BigBirdEncoderConfig()
    with pytest.raises(ValueError, match="full attention"):
        cfg.validate_length(704)
    with pytest.raises(ValueError, match="pads"):
        cfg.validate_length(800)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        cfg.validate_length(4160)
    for S in (768, 1024, 3072, 4096):
        cfg.validate_length(S)
    with pytest.raises(ValueError, match="full attention"):      # the threshold moves with the number of random blocks
        be.BigBirdEncoderConfig(num_random_blocks=4).validate_length(832)
    cfg.save_pretrained(str(tmp_path))
    assert be.BigBirdEncoderConfig.from_pretrained(str(tmp_path)) == cfg


def test_model_raises_without_a_gpu():
    if not torch.cuda.is_available():
        with pytest.raises(_hip.StonkHipError):
            be.BigBirdEncoderModel(be.BigBirdEncoderConfig(**er.config_dict(er.CASES["s768"])))


# ------------------------------------------------------------------ plans from a fixture
@pytest.mark.parametrize("name,mode", [("s768", "eval"), ("s768", "train"), ("s1024", "eval"), ("s4096", "eval")])
def test_block_sparse_plan_from_a_fixtures_rand_attn(name, mode):
    c = er.CASES[name]
    plans = er.fixture_plans(er.load_fixture(name), mode)
    assert len(plans) == c["layers"]
    for ra in plans:
        assert ra.shape == (c["heads"], c["nb"] - 2, 3) and ra.dtype == np.int32
        plan = BlockSparsePlan(c["nb"], ra)
        assert plan.num_heads == c["heads"] and plan.num_blocks == c["nb"]
        # every query block's total multiplicity: 8 for a middle row (5 fixed + 3 random), 7 for rows 1 and nb - 2, nb at the ends
        total = plan.lists["key_mult"].sum(-1)
        assert [int(v) for v in total[0]] == [c["nb"], 7] + [8] * (c["nb"] - 4) + [7, c["nb"]]
    if name in ("s1024", "s4096") and mode == "eval":      # HuggingFace's eval plan at these lengths is the zeros plan
        assert not any(ra.any() for ra in plans)
    if mode == "train":
        assert any(ra.any() for ra in plans)
