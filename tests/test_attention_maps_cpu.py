"""CPU (no GPU): the host side of the attention-map feature - the C-ABI entry stonk_attention_probs is exported, declared
and bound; its argument checks answer without a launch; the analysis helper summarize_modal_mass; and the config flag
output_attentions is still refused, now pointing at the method that does produce the maps."""
import ctypes
import os

import pytest
import torch

from stonkgs_amd import _hip
from stonkgs_amd.config import STonKGsConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_exported_declared_and_bound():
    handle = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(handle, "stonk_attention_probs")
    header = open(os.path.join(ROOT, "include", "stonk_hip.h")).read()
    assert "int stonk_attention_probs(" in header and "modeling_bert.py:111-136" in header
    assert "stonk_attention_probs" in _hip.exported_symbols()
    assert _hip.lib().stonk_abi_version() == 5            # an addition: no caller breaks


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    f = _hip.lib().stonk_attention_probs

    def call(q=16, k=16, ld=192, mask=0, probs=16, modal=16, B=1, NH=1, S=256, D=64, half=128, scale=0.125):
        return f(q, k, ld, mask, probs, modal, B, NH, S, D, half, scale, 0)

    assert call(S=100, half=64) == _hip.ESHAPE
    assert call(S=4224, half=2112) == _hip.ESHAPE          # > 4096 keys
    assert call(S=64, half=32) == _hip.ESHAPE              # < 128
    assert call(D=32) == _hip.ESHAPE
    assert call(probs=0, modal=0) == _hip.EINVAL           # nothing to write
    assert call(half=0) == _hip.EINVAL and call(half=256) == _hip.EINVAL
    assert call(half=96) == _hip.EINVAL                    # not a multiple of the 64-key tile
    assert call(q=0) == _hip.EINVAL and call(k=0) == _hip.EINVAL
    assert call(q=24) == _hip.EALIGN and call(k=8) == _hip.EALIGN
    assert call(probs=20) == _hip.EALIGN
    assert call(B=0) == _hip.OK                            # an empty batch: no launch
    assert call(B=0, modal=0) == _hip.OK and call(B=0, probs=0) == _hip.OK


def test_summarize_modal_mass_on_a_hand_made_tensor():
    from stonkgs_amd.stonkgs_for_embeddings import summarize_modal_mass

    L, B, NH, S, half = 2, 2, 3, 8, 4
    g = torch.Generator().manual_seed(0)
    text = torch.rand(L, B, NH, S, generator=g)
    mm = torch.stack([text, 1.0 - text], -1)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[0, 2:4] = 0                                       # two padded text positions in sequence 0
    mask[1, 1:4] = 0
    got = summarize_modal_mass(mm, mask, half)
    assert got.shape == (L, NH, 2, 2) and got.dtype == torch.float32
    assert float((got.sum(-1) - 1.0).abs().max()) < 1e-6
    for l in range(L):
        for h in range(NH):
            tq = torch.cat([mm[l, 0, h, 0:2], mm[l, 1, h, 0:1]])       # the three unmasked text queries
            eq = torch.cat([mm[l, 0, h, 4:8], mm[l, 1, h, 4:8]])       # every entity query
            torch.testing.assert_close(got[l, h, 0], tq.mean(0), rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(got[l, h, 1], eq.mean(0), rtol=1e-6, atol=1e-7)
    # no mask: every position counts
    torch.testing.assert_close(summarize_modal_mass(mm, None, half)[:, :, 0], mm[:, :, :, :half].mean(dim=(1, 3)),
                               rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        summarize_modal_mass(mm[0], mask, half)
    with pytest.raises(ValueError):
        summarize_modal_mass(mm, mask, S)


def test_output_attentions_is_still_refused_and_names_the_method():
    with pytest.raises(NotImplementedError, match="output_attentions") as ei:
        STonKGsConfig(output_attentions=True).validate_for_hip()
    assert "attention_maps" in str(ei.value)
    assert "CPU path" not in str(ei.value)


def test_the_method_is_inherited_by_the_classification_model():
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining, STonKGsForSequenceClassification

    assert callable(STonKGsForPreTraining.attention_maps)
    assert STonKGsForSequenceClassification.attention_maps is STonKGsForPreTraining.attention_maps
