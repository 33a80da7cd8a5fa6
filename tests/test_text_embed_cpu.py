"""CPU (no GPU): stonk_word_embed_grad refuses bad arguments with the documented status codes before anything is launched,
the symbol is declared everywhere, and the fp32 restatement of the text-only classifier that the GPU tests compare against
(tests/test_text_baseline_gpu.py) equals transformers' BertForSequenceClassification."""
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from oracle import stonkgs_oracle as orc
from stonkgs_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESHAPE, EALIGN = _hip.OK, _hip.EINVAL, _hip.ESHAPE, _hip.EALIGN
WORD = "bert.embeddings.word_embeddings.weight"
PAD = 0


# ---------------------------------------------------------------------------------------------------- the restatement
def tiny_config(num_hidden_layers=2):
    """The configuration of the text-baseline tests: hidden 128, 2 heads, intermediate 256, vocab 160, 256 positions."""
    return orc.OracleConfig(vocab_size=160, kg_vocab_size=8, hidden_size=128, num_hidden_layers=num_hidden_layers,
                            num_attention_heads=2, intermediate_size=256, max_position_embeddings=256, backbone_layers=0)


def text_state_dict(cfg, num_labels=3, seed=11):
    """bf16-representable weights in HF's BertForSequenceClassification layout (the pad row is NOT zero: a loaded checkpoint
    need not have one, and the forward reads the row as it is)."""
    sd = {k: v for k, v in orc.init_state_dict(cfg, seed=seed).items() if k.startswith("bert.")}
    g = torch.Generator().manual_seed(seed + 1)
    sd["classifier.weight"] = (torch.randn(num_labels, cfg.hidden_size, generator=g) * 0.05).to(torch.bfloat16).float()
    sd["classifier.bias"] = (torch.randn(num_labels, generator=g) * 0.02).to(torch.bfloat16).float()
    return sd


def text_classifier(sd, cfg, input_ids, attention_mask=None, token_type_ids=None, labels=None, dropout=None):
    """BertForSequenceClassification.forward from the oracle's pieces: embeddings of token ids, the encoder, the pooler line
    and a classifier. nn.Embedding(padding_idx=0) never accumulates a gradient into the pad row: the row is read detached.
    `dropout` None: dropout off, no operation added; else a mask provider (`orc._drop`; tests/step_dropout_ref.py) for the
    embeddings, every encoder site and the pooled vector."""
    w = sd[WORD]
    sd = dict(sd)
    sd[WORD] = torch.cat([w[:PAD], w[PAD:PAD + 1].detach(), w[PAD + 1:]])
    x = orc.bert_embeddings(sd, "bert.embeddings", cfg, input_ids=input_ids, token_type_ids=token_type_ids, dropout=dropout)
    seq = orc.bert_encoder(x, sd, "bert.encoder", cfg, cfg.num_hidden_layers, attention_mask, dropout=dropout)
    pooled = torch.tanh(F.linear(seq[:, 0], sd["bert.pooler.dense.weight"], sd["bert.pooler.dense.bias"]))
    logits = F.linear(orc._drop(pooled, dropout, ("classifier", 0)), sd["classifier.weight"], sd["classifier.bias"])
    out = {"logits": logits, "pooler_output": pooled}
    if labels is not None:
        out["loss"] = F.cross_entropy(logits, labels.view(-1))
    return out


def text_batch(cfg, lengths, L=None, seed=5, num_labels=3):
    """Right-padded token batch [B, L]: ids in [1, vocab) on the attended positions with a [PAD] id placed at an ATTENDED
    position of every text longer than 2, [PAD] and mask 0 behind the text; both token types."""
    g = torch.Generator().manual_seed(seed)
    B, L = len(lengths), L or cfg.max_position_embeddings
    ids = torch.zeros(B, L, dtype=torch.long)
    am = torch.zeros(B, L, dtype=torch.long)
    tt = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lengths):
        ids[b, :n] = torch.randint(1, cfg.vocab_size - 20, (n,), generator=g)   # (the last 20 ids never occur)
        am[b, :n] = 1
        tt[b, n // 2:n] = 1
        if n > 2:
            ids[b, n // 2] = PAD
    labels = torch.randint(0, num_labels, (B,), generator=g)
    return {"input_ids": ids, "attention_mask": am, "token_type_ids": tt, "labels": labels}


def restatement_grads(sd, cfg, batch):
    """(loss, logits, {name: gradient}) of the restatement, fp32 on the CPU."""
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = text_classifier(p, cfg, batch["input_ids"], batch["attention_mask"], batch["token_type_ids"], batch["labels"])
    out["loss"].backward()
    return out["loss"].detach(), out["logits"].detach(), {k: v.grad for k, v in p.items()}


def test_restatement_equals_transformers_bert_for_sequence_classification():
    try:
        from transformers import BertConfig, BertForSequenceClassification
    except Exception as e:   # pragma: no cover
        pytest.skip(f"transformers cannot be imported: {e}")
    cfg = tiny_config()
    sd = text_state_dict(cfg)
    batch = text_batch(cfg, [256, 100, 16, 1])
    assert (batch["input_ids"][batch["attention_mask"] == 1] == PAD).sum() >= 3
    hf = BertForSequenceClassification(BertConfig(
        vocab_size=160, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
        max_position_embeddings=256, type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
        layer_norm_eps=cfg.layer_norm_eps, num_labels=3, pad_token_id=PAD))
    res = hf.load_state_dict(sd, strict=False)
    params = dict(hf.named_parameters())
    assert not res.unexpected_keys and not [k for k in res.missing_keys if k in params], res
    assert set(params) == set(sd)
    hf.train()   # (p = 0: training mode is eval mode with gradients)
    out = hf(**batch)
    out.loss.backward()
    loss, logits, grads = restatement_grads(sd, cfg, batch)
    assert abs(float(loss) - float(out.loss.detach())) < 1e-5
    assert (logits - out.logits.detach()).abs().max() < 1e-5
    for k, p in params.items():
        ref = p.grad
        if k.endswith("attention.self.key.bias"):
            # a key bias shifts every score of a query by the same amount and the softmax does not see it: this gradient is
            # exactly zero in exact arithmetic, both sides hold rounding residue (~1e-11), and the difference is measured
            # against the layer's query-bias gradient instead of against that residue
            ref = params[k.replace(".key.", ".query.")].grad
        rel = float((grads[k] - p.grad).norm() / ref.norm())
        assert rel < 1e-5, (k, rel)
    assert torch.count_nonzero(params[WORD].grad[PAD]) == 0
    assert torch.count_nonzero(grads[WORD][PAD]) == 0 and torch.count_nonzero(grads[WORD]) > 0


# ---------------------------------------------------------------------------------------------------- the launcher
def _weg(**kw):
    a = dict(dsum=4096, ld=768, ids=8192, row_of_pos=0, dword=16384, ld_w=768, vocab=1000, padding_idx=0, B=2, S=256, H=768,
             err=64, stream=0)
    a.update(kw)
    return _hip.lib().stonk_word_embed_grad(*a.values())


def test_word_embed_grad_argument_checks():
    """Every call here is refused (or has nothing to do) before a launch: no GPU is touched."""
    for null in ("dsum", "ids", "dword", "err"):
        assert _weg(**{null: 0, "B": 0}) == EINVAL, null
    assert _weg(H=100, B=0) == ESHAPE and _weg(H=4104, ld=4104, ld_w=4104, B=0) == ESHAPE and _weg(H=0, B=0) == ESHAPE
    assert _weg(ld=760, B=0) == ESHAPE and _weg(ld_w=767, B=0) == ESHAPE
    assert _weg(vocab=0, B=0) == ESHAPE and _weg(vocab=-3, padding_idx=-5, B=0) == ESHAPE
    assert _weg(padding_idx=1000, B=0) == ESHAPE and _weg(padding_idx=999, B=0) == OK and _weg(padding_idx=-1, B=0) == OK
    assert _weg(B=1 << 23, S=256) == ESHAPE and _weg(B=-1) == ESHAPE and _weg(S=0, B=0) == ESHAPE
    assert _weg(dsum=4104, B=0) == EALIGN and _weg(ld=772, B=0) == EALIGN and _weg(dword=16386, B=0) == EALIGN
    assert _weg(ld=776, ld_w=769, B=0) == OK                    # ld % 8 only; the fp32 rows need no vector alignment
    assert _weg(B=0) == OK                                       # nothing to do, nothing launched


def test_word_embed_grad_is_declared_everywhere_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "stonk_hip.h")).read()
    assert "int stonk_word_embed_grad(const void* dsum, int64_t ld, const int64_t* input_ids, const int* row_of_pos," in header
    assert "stonk_word_embed_grad" in _hip._SIGNATURES and "stonk_word_embed_grad" in _hip.exported_symbols()
    assert len(_hip._SIGNATURES["stonk_word_embed_grad"]) == 13
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T stonk_word_embed_grad" in nm
    assert hasattr(_hip.lib(), "stonk_word_embed_grad")
    assert _hip.lib().stonk_abi_version() == 5
