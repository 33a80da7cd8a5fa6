"""CPU (no GPU): stonk_row_topk_f32 / _f16 refuse bad arguments with the documented status codes before anything is
launched, and the evaluation surface exists where the issue puts it."""
import inspect

import pytest

from stonkgs_amd import _hip

OK, EINVAL, ESHAPE = _hip.OK, _hip.EINVAL, _hip.ESHAPE


def _topk(entry, **kw):
    a = dict(logits=4096, ld=384, ncols=300, targets=8192, count=12288, cap=40, k=5, top_val=16384, top_idx=20480, lse=24576,
             rank=28672, tgt_logit=32768, stream=0)
    a.update(kw)
    return getattr(_hip.lib(), entry)(*a.values())


@pytest.mark.parametrize("entry", ["stonk_row_topk_f32", "stonk_row_topk_f16"])
def test_row_topk_argument_checks(entry):
    assert (EINVAL, ESHAPE) == (-1, -2)
    assert _topk(entry, k=0) == ESHAPE and _topk(entry, k=17) == ESHAPE and _topk(entry, k=-1) == ESHAPE
    assert _topk(entry, ncols=4, ld=8, k=5) == ESHAPE                       # k > ncols
    assert _topk(entry, ncols=0, ld=8) == ESHAPE
    assert _topk(entry, ld=299) == EINVAL                                   # ld < ncols
    for null in ("logits", "count", "top_val", "top_idx", "lse"):
        assert _topk(entry, **{null: 0}) == EINVAL, null
    assert _topk(entry, rank=0) == EINVAL and _topk(entry, tgt_logit=0) == EINVAL   # required with targets ...
    assert _topk(entry, cap=-1) == EINVAL
    assert _topk(entry, cap=0) == OK                                        # nothing to do, nothing launched
    assert _topk(entry, cap=0, targets=0, rank=0, tgt_logit=0) == OK        # ... and nullable without


def test_evaluation_surface():
    from stonkgs_amd.engine import Engine
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    assert list(inspect.signature(Engine.evaluate).parameters)[1:] == [
        "input_ids", "attention_mask", "token_type_ids", "mlm_labels", "ent_labels", "nsp_labels", "k"]
    assert inspect.signature(STonKGsForPreTraining.evaluate_batch).parameters["k"].default == 10
    p = inspect.signature(STonKGsForPreTraining.predict_masked).parameters
    assert list(p)[1:] == ["input_ids", "attention_mask", "token_type_ids", "positions", "k"] and p["k"].default == 10
    a = TrainingArguments()
    assert a.eval_steps == 0 and a.per_device_eval_batch_size == 8
    assert inspect.signature(Trainer.__init__).parameters["eval_dataset"].default is None
    p = inspect.signature(Trainer.evaluate).parameters
    assert (p["eval_dataset"].default, p["k"].default, p["max_batches"].default) == (None, 10, None)
