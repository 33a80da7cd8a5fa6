"""CPU (no GPU): the host side of the input-attribution feature - the C-ABI entry stonk_input_attribution is exported,
declared and bound; every argument check answers without a launch; the analysis helper summarize_attributions; and the
classification model has a method of its own."""
import ctypes
import os

import pytest
import torch

from stonkgs_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_exported_declared_and_bound():
    handle = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(handle, "stonk_input_attribution")
    header = open(os.path.join(ROOT, "include", "stonk_hip.h")).read()
    assert "int stonk_input_attribution(" in header and "stonkgs_model.py:193-210" in header
    assert "stonk_input_attribution" in _hip.exported_symbols()
    assert _hip.lib().stonk_abi_version() == 5            # an addition: no caller breaks


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    f = _hip.lib().stonk_input_attribution

    def call(dsum=16, ld=128, ids=16, text=16, kg=16, kg_rows=10, row_of_pos=0, scale=1.0, gxi=16, gn=16, gout=0, ld_out=0,
             B=1, S=256, half=128, H=128):
        return f(dsum, ld, ids, text, kg, kg_rows, row_of_pos, scale, gxi, gn, gout, ld_out, B, S, half, H, 0)

    for name in ("dsum", "ids", "text", "kg"):
        assert call(**{name: 0}) == _hip.EINVAL, name
    assert call(gxi=0, gn=0) == _hip.EINVAL                # nothing to write
    assert call(gxi=0, gn=0, gout=16, ld_out=128) == _hip.EINVAL   # the gradient alone is not enough either
    assert call(H=124, ld=128) == _hip.ESHAPE              # H % 8
    assert call(H=4104, ld=4104) == _hip.ESHAPE            # H > 4096
    assert call(half=257) == _hip.ESHAPE and call(half=-1) == _hip.ESHAPE
    assert call(kg_rows=0) == _hip.ESHAPE and call(kg_rows=-3) == _hip.ESHAPE
    assert call(ld=120) == _hip.ESHAPE                     # ld < H
    assert call(gout=16, ld_out=120) == _hip.ESHAPE        # ld_out < H with grad_out
    for name in ("dsum", "text", "kg"):
        assert call(**{name: 24}) == _hip.EALIGN, name
    assert call(gout=24, ld_out=128) == _hip.EALIGN
    assert call(ld=132) == _hip.EALIGN                     # ld % 8
    assert call(half=0, B=0) == _hip.OK and call(half=256, B=0) == _hip.OK   # the ends of the range are shapes like any other
    assert call(B=0) == _hip.OK                            # an empty batch: no launch
    assert call(B=0, gxi=0) == _hip.OK and call(B=0, gn=0) == _hip.OK
    assert call(B=0, gout=16, ld_out=136, row_of_pos=16) == _hip.OK


def test_summarize_attributions_on_a_hand_made_tensor():
    from stonkgs_amd.stonkgs_for_embeddings import summarize_attributions

    half = 4
    attr = torch.tensor([[1.0, -2.0, 5.0, 7.0, 0.5, -0.5, 3.0, 0.0],
                         [-4.0, 9.0, 9.5, 1.0, 2.0, -6.0, 0.0, 0.0]])
    mask = torch.ones(2, 8, dtype=torch.long)
    mask[0, 2:4] = 0                                       # two masked text positions in sequence 0 (|attr| 5 and 7)
    mask[1, 1:4] = 0                                       # three in sequence 1 (9, 9.5, 1)
    got = summarize_attributions(attr, mask, half, top=3)
    assert got["shares"].shape == (2, 2) and got["shares"].dtype == torch.float32
    # sequence 0: text 1 + 2 = 3, entities 0.5 + 0.5 + 3 = 4; sequence 1: text 4, entities 2 + 6 = 8
    torch.testing.assert_close(got["shares"], torch.tensor([[3 / 7, 4 / 7], [4 / 12, 8 / 12]]), rtol=1e-6, atol=1e-7)
    assert float((got["shares"].sum(1) - 1.0).abs().max()) < 1e-6
    # the top positions rank |attr| over the whole sequence, largest first, and report the signed values
    assert got["top_positions"].tolist() == [[3, 2, 6], [2, 1, 5]]
    assert got["top_values"].tolist() == [[7.0, 5.0, 3.0], [9.5, 9.0, -6.0]]
    # no mask: every text position counts (sequence 0: 15 against 4)
    torch.testing.assert_close(summarize_attributions(attr, None, half)["shares"][0], torch.tensor([15 / 19, 4 / 19]),
                               rtol=1e-6, atol=1e-7)
    assert summarize_attributions(attr, None, half, top=100)["top_positions"].shape == (2, 8)
    with pytest.raises(ValueError):
        summarize_attributions(attr[0], mask, half)
    with pytest.raises(ValueError):
        summarize_attributions(attr, mask, 8)
    with pytest.raises(ValueError):
        summarize_attributions(attr, mask, 0)


def test_the_classification_model_has_a_method_of_its_own():
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining, STonKGsForSequenceClassification

    assert callable(STonKGsForPreTraining.input_attributions)
    assert callable(STonKGsForSequenceClassification.input_attributions)
    assert STonKGsForSequenceClassification.input_attributions is not STonKGsForPreTraining.input_attributions
