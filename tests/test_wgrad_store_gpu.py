"""GPU: stonk_gemm_tn_bf16_store - the weight gradient of a launch with one K split, WRITTEN instead of accumulated. One
producer per element, so it must equal stonk_gemm_tn_bf16 into a zeroed buffer exactly, whatever the destination held."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(shape, scale, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


def _pair(hip, Mo, No, cap, split, count, seed, bias=False, alpha=0.5):
    """(atomic form into zeros, store form into garbage) for dY [cap, Mo], X [cap, No]; `count`: device-side token count
    (None: the capacity). Rows from the count up to the next multiple of 64 are zero, as the contract asks."""
    dY, X = _rand((cap, Mo), 0.5, seed), _rand((cap, No), 0.5, seed + 1)
    cnt = None
    if count is not None:
        dY[count:(count + 63) // 64 * 64] = 0
        X[count:(count + 63) // 64 * 64] = 0
        cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    res = []
    for store in (False, True):
        dW = torch.full((Mo, No), float("nan") if store else 0.0, device="cuda")
        db = torch.full((Mo,), 123.0 if store else 0.0, device="cuda") if bias else None
        hip.call("stonk_gemm_tn_bf16_store" if store else "stonk_gemm_tn_bf16", hip.ptr(dY), Mo, hip.ptr(X), No, hip.ptr(dW),
                 No, hip.ptr(db), Mo, No, cap, alpha, split, hip.ptr(cnt), hip.stream_ptr())
        res.append((dW, db))
    torch.cuda.synchronize()
    return res, dY, X


# (rows, cols, token capacity, split_k, device-side count): the 256x256 kernel unsplit on a CU share (-160: the engine's
# side-stream form; 42 * 256 rows x 768 = 126 tiles would split on 160 CUs, 60 * 3 = 180 tiles do not) and on all CUs; the
# 128x128 kernel with split_k = 1; counts: full, ragged last K tile (not a multiple of 64), zero
CASES = [
    (15360, 768, 1024, -160, None), (15360, 768, 1024, -160, 1000), (15360, 768, 1024, -160, 37), (15360, 768, 1024, -160, 0),
    (22016, 768, 512, 0, 451), (22016, 768, 512, 0, 0),
    (3200, 768, 1024, 1, None), (3200, 768, 1024, 1, 999), (3200, 768, 1024, 1, 0), (29056, 768, 256, 1, 130),
]


@pytest.mark.parametrize("Mo,No,cap,split,count", CASES)
def test_store_mode_equals_the_atomic_form_into_zeros(hip, Mo, No, cap, split, count):
    ((ref, _), (got, _)), dY, X = _pair(hip, Mo, No, cap, split, count, seed=Mo % 97 + (count or 0))
    assert torch.isfinite(got).all()                      # every element defined: nothing of the garbage is left
    assert torch.equal(got, ref), int((got != ref).sum())
    if count == 0:
        assert float(got.abs().max()) == 0.0
    else:
        assert float(got.abs().max()) > 0.0
        k = cap if count is None else count
        want = 0.5 * (dY[:k, :256].float().t() @ X[:k, :128].float())
        assert float((got[:256, :128] - want).abs().max()) < 2e-3 * float(want.abs().max()) + 1e-3   # (fp32 accumulation order)


@pytest.mark.parametrize("Mo,No,cap,split,count", [(46080, 256, 512, -160, 300), (46080, 256, 512, -160, 0),
                                                   (1024, 768, 512, 1, 300), (1024, 768, 512, 1, 0)])
def test_store_mode_bias_sums(hip, Mo, No, cap, split, count):
    """The bias gradient is stored too. One column tile (256x256 kernel) or the first column tile alone (128x128 kernel)
    produces it in both forms, in the same order: exact equality."""
    ((ref, rb), (got, gb)), dY, _ = _pair(hip, Mo, No, cap, split, count, seed=5, bias=True)
    assert torch.equal(got, ref) and torch.equal(gb, rb)
    want = 0.5 * dY[:count].float().sum(0)
    assert float((gb - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


def test_store_mode_refuses_a_split_launch(hip):
    """A shape the launcher would split has several producers per element: refused with STONK_ESHAPE, nothing launched."""
    lib = hip.lib()
    dY, X = _rand((4096, 768), 0.5, 1), _rand((4096, 768), 0.5, 2)
    dW = torch.full((768, 768), 5.0, device="cuda")
    a = (hip.ptr(dY), 768, hip.ptr(X), 768, hip.ptr(dW), 768, 0, 768, 768, 4096, 1.0)
    assert lib.stonk_gemm_tn_bf16_store(*a, 4, 0, hip.stream_ptr()) == hip.ESHAPE      # explicit split
    assert lib.stonk_gemm_tn_bf16_store(*a, 0, 0, hip.stream_ptr()) == hip.ESHAPE      # 9 tiles on 256 CUs: automatic split
    assert lib.stonk_gemm_tn_bf16_store(*a, -160, 0, hip.stream_ptr()) == hip.ESHAPE
    assert lib.stonk_gemm_tn_bf16_store(*a, -1, 0, hip.stream_ptr()) == hip.ESHAPE     # the eight-wave form has no store mode
    db = torch.zeros(15360, device="cuda")
    dY2 = _rand((1024, 15360), 0.5, 3)
    dW2 = torch.zeros(15360, 768, device="cuda")
    assert lib.stonk_gemm_tn_bf16_store(hip.ptr(dY2), 15360, hip.ptr(X), 768, hip.ptr(dW2), 768, hip.ptr(db), 15360, 768, 1024,
                                        1.0, -160, 0, hip.stream_ptr()) == hip.ESHAPE  # bias over three column tiles
    torch.cuda.synchronize()
    assert (dW == 5.0).all()


def test_trainer_steps_match_with_and_without_stored_gradients(hip):
    """Three optimizer steps with two micro-batches each, through the Trainer (stored decoder gradients on the first
    micro-batch, tiled AdamW, spans left unzeroed) against the same steps with the store mode switched off (atomics into the
    buffer AdamW zeroed). The two runs must agree to the noise of the remaining fp32 atomics and the W^T copies must equal
    the transposed bf16 mirror after every step."""
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.data import synthetic_batch
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    # (31 000 x 128: 243 x 1 tiles of 128x128 - the text decoder's gradient is unsplit and takes the store mode, as at full
    # size; the 300-row entity decoder splits K, is refused and goes through the stale-span path)
    dims = dict(vocab_size=31000, kg_vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                intermediate_size=256, max_position_embeddings=256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    rows = torch.randn(300, 128, generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 0.3
    finals = []
    for store in (True, False):
        torch.manual_seed(3)
        model = STonKGsForPreTraining(STonKGsConfig(**dims), kg_embeddings=rows)
        tr = Trainer(model, TrainingArguments(per_device_train_batch_size=4, gradient_accumulation_steps=2, learning_rate=1e-3))
        assert model.engine.store_names
        if not store:
            model.engine.store_names = ()
            tr._keep_grad = None
        eng, st = model.engine, model._store
        text, ent = "cls.predictions.text_decoder.weight", "cls.predictions.entity_decoder.weight"
        for i in range(6):
            eng.store_log.clear()
            loss = tr.training_step(model, synthetic_batch(4, 31000, 300, 256, seed=20 + i, min_text=16))
            assert eng.store_first is False                        # only the trainer's own backward may store
            # the route each decoder took: first micro-batch - the unsplit text decoder stores, the entity decoder (split K)
            # is refused and accumulates; second micro-batch, or store mode off - no attempt at all
            want = [(ent, hip.ESHAPE), (text, hip.OK)] if store and i % 2 == 0 else []
            assert list(eng.store_log) == want, (i, list(eng.store_log))
            if i % 2 == 1:
                eng.wait_params()
                torch.cuda.synchronize()
                for name, wt in st.wt.items():
                    w = st.bf16_view(name, padded=False)
                    assert torch.equal(wt[:, :w.shape[0]], w.t()), name
                # after the optimizer step: the decoders' spans hold the step's gradient (kept), every other element is zero
                g = st.grad.clone()
                for name in (text, ent):
                    lo, hi = st.span(name)
                    assert (float(g[lo:hi].abs().max()) > 0.0) == store, name
                    g[lo:hi] = 0
                assert float(g.abs().max()) == 0.0
                assert eng.grad_stale == (set((text, ent)) if store else set())
        model.engine.check_errors()
        finals.append((float(loss), model._store.data.clone()))
    (la, a), (lb, b) = finals
    print("loss", la, lb, "max |dp|", float((a - b).abs().max()), "mean |dp|", float((a - b).abs().mean()))
    # both arms carry the split-K atomics' order noise; Adam turns a sign flip of a near-zero gradient into up to 2 lr per
    # step, so single elements may differ by 6e-3 - the loss (smoke()'s bound against the oracle) and the mean may not
    assert abs(la - lb) < 1e-2 and float((a - b).abs().max()) <= 6e-3 + 1e-6 and float((a - b).abs().mean()) < 1e-4


def test_backwards_outside_the_trainer_accumulate_after_a_trainer_step(hip):
    """A Trainer step leaves the decoders' gradient spans unzeroed and marked stale. Two backwards driven by somebody else on
    the same model afterwards (torch's way of accumulating: backward twice, no zeroing in between) must ADD: the first one
    zeroes the stale spans before accumulating, neither stores. The text decoder's gradient is unsplit - one atomic add per
    element and backward - so after two identical backwards it is exactly twice the gradient of one."""
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.data import synthetic_batch
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    dims = dict(vocab_size=31000, kg_vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                intermediate_size=256, max_position_embeddings=256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    rows = torch.randn(300, 128, generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 0.3
    model = STonKGsForPreTraining(STonKGsConfig(**dims), kg_embeddings=rows)
    tr = Trainer(model, TrainingArguments(per_device_train_batch_size=4, learning_rate=1e-3))
    eng, st = model.engine, model._store
    text, ent = "cls.predictions.text_decoder.weight", "cls.predictions.entity_decoder.weight"
    tr.training_step(model, synthetic_batch(4, 31000, 300, 256, seed=1, min_text=16))
    eng.wait_params()
    assert eng.store_first is False and eng.grad_stale == {text, ent}
    assert float(st.grad_view(text).abs().max()) > 0.0             # the trainer step's gradient is still there
    batch = synthetic_batch(4, 31000, 300, 256, seed=2, min_text=16)
    eng.store_log.clear()
    model.forward_backward(batch)
    torch.cuda.synchronize()
    assert not eng.store_log and not eng.grad_stale
    once = {n: st.grad_view(n, padded=True).clone() for n in (text, ent)}
    model.forward_backward(batch)
    torch.cuda.synchronize()
    assert not eng.store_log
    assert torch.equal(st.grad_view(text, padded=True), 2 * once[text])
    twice = st.grad_view(ent, padded=True)
    assert float((twice - 2 * once[ent]).abs().max()) <= 1e-5 * float(once[ent].abs().max())   # (split K: fp32 atomics' order)
    # and against a model that never saw a trainer: the same single-backward gradient
    model2 = STonKGsForPreTraining(STonKGsConfig(**dims), kg_embeddings=rows)
    model2.train()
    model2._store.data.copy_(st.data)
    model2._bb_store.data.copy_(model._bb_store.data)
    model2.engine.refresh_derived(bf16_mirror=True)
    model2.zero_grad()
    model2.forward_backward(batch)
    torch.cuda.synchronize()
    assert torch.equal(model2._store.grad_view(text, padded=True), once[text])
