"""The model classes' layering, checked on imported objects only (no GPU): one flat-buffer base under the three classes,
the text model outside the STonKGs hierarchy, and one definition of the int64 input conversion."""
import torch

from stonkgs_amd import flat_model, nlp_baseline_model, stonkgs_model, stonkgs_pretraining
from stonkgs_amd.flat_model import FlatBufferModel, SequenceClassifierFront, as_long
from stonkgs_amd.nlp_baseline_model import BertForSequenceClassification
from stonkgs_amd.stonkgs_model import STonKGsForPreTraining, STonKGsForSequenceClassification

STONKGS_ONLY = ("encode", "attention_maps", "input_attributions", "evaluate_batch", "predict_masked", "entity_names")
CPU = torch.device("cpu")


def test_hierarchy():
    for cls in (STonKGsForPreTraining, STonKGsForSequenceClassification, BertForSequenceClassification):
        assert issubclass(cls, FlatBufferModel) and issubclass(cls, torch.nn.Module)
    assert issubclass(STonKGsForSequenceClassification, STonKGsForPreTraining)
    assert not issubclass(BertForSequenceClassification, STonKGsForPreTraining)
    for name in STONKGS_ONLY:
        assert hasattr(STonKGsForPreTraining, name), name
        assert not hasattr(BertForSequenceClassification, name), name
    assert not hasattr(BertForSequenceClassification, "from_default_pretrained")
    # both classifiers take their front from the one mixin, the pre-training class does not
    for cls in (STonKGsForSequenceClassification, BertForSequenceClassification):
        assert issubclass(cls, SequenceClassifierFront)
        assert cls._classify is SequenceClassifierFront._classify
        assert cls.forward_backward is SequenceClassifierFront.forward_backward
        assert cls._backward is SequenceClassifierFront._backward
    assert not issubclass(STonKGsForPreTraining, SequenceClassifierFront)
    assert STonKGsForPreTraining._backward is not FlatBufferModel._backward


def test_shared_plumbing_is_the_base_class_own():
    """What the issue moves into the base is defined there and nowhere below it."""
    moved = ("_apply", "_init_weights", "_mark_synced", "_sync_derived", "zero_grad", "_prepare_grads_for_autograd",
             "_reattach_grads", "named_grad_views", "_wait_params", "state_dict", "named_parameters", "load_state_dict",
             "save_pretrained", "_long")
    for cls in (STonKGsForPreTraining, STonKGsForSequenceClassification, BertForSequenceClassification):
        for name in moved:
            assert getattr(cls, name) is getattr(FlatBufferModel, name), (cls.__name__, name)
    assert isinstance(FlatBufferModel.__dict__["device"], property)
    assert stonkgs_model._load_weights_file is flat_model._load_weights_file    # (still importable from stonkgs_model)
    assert stonkgs_model.SequenceClassifierOutput is flat_model.SequenceClassifierOutput


def test_as_long_identity_and_conversion():
    ok = torch.arange(6).reshape(2, 3)
    assert as_long(ok, CPU) is ok                                    # int64, contiguous, on the device: the same tensor
    assert as_long(None, CPU) is None
    from_list = as_long([[1, 2], [3, 4]], CPU)
    assert from_list.dtype == torch.long and from_list.tolist() == [[1, 2], [3, 4]]
    i32 = torch.tensor([5, -100, 7], dtype=torch.int32)
    got = as_long(i32, CPU)
    assert got is not i32 and got.dtype == torch.long and got.tolist() == [5, -100, 7]
    view = ok.t()                                                    # [3, 2], strides (1, 3)
    assert not view.is_contiguous()
    got = as_long(view, CPU)
    assert got.is_contiguous() and got.dtype == torch.long and torch.equal(got, view)
    assert got.data_ptr() != ok.data_ptr()
    sliced = torch.arange(10)[::2]
    got = as_long(sliced, CPU)
    assert got.is_contiguous() and got.tolist() == [0, 2, 4, 6, 8]


def test_one_definition_of_the_long_helper():
    assert as_long.__module__ == "stonkgs_amd.flat_model"
    assert stonkgs_pretraining.as_long is as_long                    # Trainer._on_device converts with the same function
    for mod in (stonkgs_model, nlp_baseline_model, stonkgs_pretraining):
        own = [n for n, v in vars(mod).items() if callable(v) and getattr(v, "__module__", None) == mod.__name__
               and n.lstrip("_") in ("prep", "prep_long", "long", "as_long")]
        assert not own, (mod.__name__, own)
    for cls in (STonKGsForPreTraining, STonKGsForSequenceClassification, BertForSequenceClassification):
        for name in ("_prep", "_prep_long", "_long"):
            assert name not in vars(cls), (cls.__name__, name)
    assert not hasattr(STonKGsForPreTraining, "_prep_long") and not hasattr(BertForSequenceClassification, "_prep")
    # the method is the module-level helper bound to the model's device
    code = FlatBufferModel._long.__code__
    assert "as_long" in code.co_names and FlatBufferModel._long.__globals__["as_long"] is as_long
