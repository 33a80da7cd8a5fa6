"""GPU: STonKGsForPreTraining.attention_maps on g2_hipsmall (2 layers, H 128, 2 heads, S 256, B 3) - against the
oracle's per-layer softmax(Q K^T / sqrt(d) + mask), the interface (layer selection, output modes, the size guard), that a
call leaves no trace in the encoder or in a training step around it, and the analysis helper on its output.

The bound on the total-variation distance to the oracle is a measurement (profiles/attention_maps.md): TV_BOUND is three
times the largest value seen on the MI355X, rounded up to one significant digit - the margin covers bf16 hidden states
whose rounding moves with launch geometry - and may never exceed 0.05: a map that misplaces more than 5 % of a row's mass
is wrong whatever the hardware does."""
import math

import pytest
import torch

from oracle import stonkgs_oracle as orc
from tests.golden_util import load_case
from tests.test_finetune_gpu import _build_cls, _g6
from tests.test_model_gpu import _build

pytestmark = pytest.mark.gpu

TV_MEASURED = 2.565e-4   # first run on the MI355X: layer 0 2.164e-4, layer 1 2.565e-4 (row means 1.2e-4 / 1.5e-4)
TV_BOUND = 8e-4          # 3 x 2.565e-4 = 7.7e-4, rounded up to one significant digit
assert 3 * TV_MEASURED <= TV_BOUND <= 0.05


@pytest.fixture(scope="module")
def g2(hip):
    cfg, sd, tsv_rows, batch, gold, meta = load_case("g2_hipsmall")
    model = _build(cfg, sd, tsv_rows)
    model.eval()
    inputs = {k: batch[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    full = model.attention_maps(**inputs, output="both")
    torch.cuda.synchronize()
    return dict(cfg=cfg, sd=sd, tsv_rows=tsv_rows, batch=batch, inputs=inputs, model=model, full=full)


def _oracle_maps(cfg, sd, tsv_rows, inputs):
    """fp32 torch, per layer: softmax(Q K^T / sqrt(d) + mask) from the layer's input as the oracle computes it."""
    with torch.no_grad():
        table = orc.build_kg_table(tsv_rows, orc.special_vectors(sd, cfg))
        out = orc.forward(sd, cfg, table, inputs["input_ids"], inputs["attention_mask"], inputs["token_type_ids"],
                          collect_layers=True)
        xs = [out["embedding_output"]] + out["layers"][:-1]
        B, S, H = xs[0].shape
        nh = cfg.num_attention_heads
        d = H // nh
        bias = (1.0 - inputs["attention_mask"][:, None, None, :].float()) * torch.finfo(torch.float32).min
        maps = []
        for i, x in enumerate(xs):
            pre = f"bert.encoder.layer.{i}.attention.self."
            q = torch.nn.functional.linear(x, sd[pre + "query.weight"], sd[pre + "query.bias"]).view(B, S, nh, d).transpose(1, 2)
            k = torch.nn.functional.linear(x, sd[pre + "key.weight"], sd[pre + "key.bias"]).view(B, S, nh, d).transpose(1, 2)
            maps.append(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d) + bias, -1))
    return maps, out["pooler_output"]


def test_maps_match_the_oracle(g2):
    cfg, full = g2["cfg"], g2["full"]
    ref, pooled = _oracle_maps(cfg, g2["sd"], g2["tsv_rows"], g2["inputs"])
    assert full["layers"] == (0, 1) and len(full["attentions"]) == 2
    worst = 0.0
    for i, (p, r) in enumerate(zip(full["attentions"], ref)):
        tv = 0.5 * (p.cpu() - r).abs().sum(-1)             # per query row
        print(f"layer {i}: max total-variation distance to the oracle {float(tv.max()):.3e} (mean {float(tv.mean()):.3e})")
        worst = max(worst, float(tv.max()))
        dead = (g2["inputs"]["attention_mask"] == 0)[:, None, None, :].expand_as(p)
        assert float(p.cpu()[dead].abs().max()) == 0.0
    print(f"max over layers {worst:.3e}; bound {TV_BOUND}")
    assert worst <= TV_BOUND, worst
    rel = float((full["pooler_output"].cpu() - pooled).norm() / pooled.norm())
    assert rel < 2e-2, rel


def test_shapes_dtypes_and_layer_selection(g2):
    cfg, model, inputs, full = g2["cfg"], g2["model"], g2["inputs"], g2["full"]
    B, S, NH, L, H = 3, cfg.max_position_embeddings, cfg.num_attention_heads, cfg.num_hidden_layers, cfg.hidden_size
    assert set(full) == {"layers", "attentions", "modal_mass", "pooler_output"}
    assert all(a.shape == (B, NH, S, S) and a.dtype == torch.float32 and a.is_contiguous() for a in full["attentions"])
    assert full["modal_mass"].shape == (L, B, NH, S, 2) and full["modal_mass"].dtype == torch.float32
    assert full["pooler_output"].shape == (B, H) and full["pooler_output"].dtype == torch.float32
    _, pooled = model.encode(**inputs)
    assert torch.equal(pooled, full["pooler_output"])
    by_range = model.attention_maps(**inputs, layers=range(L), output="both")
    assert by_range["layers"] == full["layers"]
    assert all(torch.equal(a, b) for a, b in zip(by_range["attentions"], full["attentions"]))
    assert torch.equal(by_range["modal_mass"], full["modal_mass"])
    last = model.attention_maps(**inputs, layers=[-1])
    assert set(last) == {"layers", "attentions", "pooler_output"} and last["layers"] == (L - 1,)
    assert len(last["attentions"]) == 1 and torch.equal(last["attentions"][0], full["attentions"][-1])
    both = model.attention_maps(**inputs, layers=[-1, 0], output="modal_mass")
    assert both["layers"] == (0, 1) and "attentions" not in both and torch.equal(both["modal_mass"], full["modal_mass"])
    half = cfg.half_length
    for i, a in enumerate(full["attentions"]):
        mm = full["modal_mass"][i]
        assert float((mm[..., 0] - a[..., :half].sum(-1)).abs().max()) < 1e-5
        assert float((mm[..., 1] - a[..., half:].sum(-1)).abs().max()) < 1e-5
    for bad in ([0, 0], [0, -2], [2], [-3], []):
        with pytest.raises(ValueError):
            model.attention_maps(**inputs, layers=bad)
    with pytest.raises(ValueError):
        model.attention_maps(**inputs, output="logits")
    model.engine.check_errors()


def test_modal_mass_mode_allocates_no_map(g2):
    cfg, model, inputs = g2["cfg"], g2["model"], g2["inputs"]
    S, NH = cfg.max_position_embeddings, cfg.num_attention_heads
    one_map = 3 * NH * S * S * 4
    model.attention_maps(**inputs, output="modal_mass")    # (the encoder's scratch buffers exist from here on)
    dev_inputs = {k: v.cuda() for k, v in inputs.items()}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    res = model.attention_maps(**dev_inputs, output="modal_mass")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"modal_mass mode: peak memory grew by {grown} bytes; one map is {one_map}")
    assert grown < one_map and "attentions" not in res


def test_size_guard_refuses_before_anything_runs(g2):
    model, inputs = g2["model"], g2["inputs"]
    rows = list(model.engine.rows_executed)
    with pytest.raises(ValueError, match="modal_mass"):
        model.attention_maps(**inputs, max_bytes=1)
    assert list(model.engine.rows_executed) == rows
    one_map = 3 * 2 * 256 * 256 * 4
    with pytest.raises(ValueError, match="layers="):
        model.attention_maps(**inputs, max_bytes=2 * one_map - 1)
    assert list(model.engine.rows_executed) == rows
    model.attention_maps(**inputs, layers=[0], max_bytes=one_map)
    assert list(model.engine.rows_executed) != rows


def test_module_mode_is_left_alone_and_dropout_stays_off(hip):
    cfg, sd, tsv_rows, batch, _, _ = load_case("g2_hipsmall")
    model = _build(cfg, sd, tsv_rows, dropout=0.1)
    inputs = {k: batch[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    model.train()
    seed = model.engine.seed_base
    a = model.attention_maps(**inputs, layers=[1])
    assert model.training and model.engine.seed_base == seed
    model.eval()
    b = model.attention_maps(**inputs, layers=[1])
    assert not model.training
    assert torch.equal(a["attentions"][0], b["attentions"][0]) and torch.equal(a["pooler_output"], b["pooler_output"])


def test_classification_model_returns_the_same_shapes(hip):
    cfg, sd, rows, gold, meta = _g6()
    model = _build_cls(cfg, sd, rows, meta["num_labels"])
    inputs = {k: torch.from_numpy(gold[k]) for k in ("input_ids", "attention_mask", "token_type_ids")}
    B, S, NH, L = inputs["input_ids"].shape[0], cfg.max_position_embeddings, cfg.num_attention_heads, cfg.num_hidden_layers
    res = model.attention_maps(**inputs, output="both")
    assert res["layers"] == tuple(range(L)) and len(res["attentions"]) == L
    assert all(a.shape == (B, NH, S, S) and a.dtype == torch.float32 for a in res["attentions"])
    assert res["modal_mass"].shape == (L, B, NH, S, 2) and res["pooler_output"].shape == (B, cfg.hidden_size)
    assert float((res["attentions"][-1].sum(-1) - 1.0).abs().max()) < 1e-5
    model.engine.check_errors()


def test_encode_is_the_same_before_and_after(g2):
    model, inputs = g2["model"], g2["inputs"]
    s0, p0 = model.encode(**inputs)
    model.attention_maps(**inputs, output="both")
    s1, p1 = model.encode(**inputs)
    assert torch.equal(s0, s1) and torch.equal(p0, p1)


def _bits(t):
    return t.reshape(-1).contiguous().view(torch.uint8)     # (workspace buffers may hold NaN bit patterns: compare the bytes)


def test_a_call_between_forward_and_backward_leaves_no_trace(hip):
    """Dropout 0, forward -> attention_maps -> backward against forward -> backward.

    What is bitwise, and asserted bitwise: the loss of the forward, and EVERYTHING the backward reads - every workspace
    buffer that existed after the forward except the forward-only scratch ("tmp.", "et.", "bb."), the saved-activation
    table, the gradient buffer, the parameters, the dropout counter and the prefetch state - is byte for byte what it was
    before the call, and the call creates scratch buffers only. The backward then is the same computation on the same
    inputs.

    The gradients (and the loss) of two SEPARATE runs cannot be compared bitwise on this code base, with or without the
    call: the loss sums and the split weight gradients are float atomics, equal up to their arrival order. Measured on
    the MI355X, six fresh models against the first: plain run against plain run, 27 or 28 of 46 gradient tensors differ in
    some last bits (worst 1.2e-6, 2.4e-6 and 4.8e-6 of the tensor's maximum in three pairs) and the loss differs in one of
    the three pairs; with the call in between, 27 and 28 tensors, worst 2.4e-6 and 4.8e-6, the loss in one of the two
    pairs - the plain pairs' own figures. The two runs are therefore held to the bounds
    the suite already uses for "the same kernels on the same data": 1e-5 relative on the loss
    (test_unpad_gpu.py::test_backbone_prefetch_changes_nothing) and 1e-4 relative L2 per gradient tensor
    (test_evaluate_gpu.py::test_evaluation_is_invisible_to_training)."""
    cfg, sd, tsv_rows, batch, _, _ = load_case("g2_hipsmall")
    inputs = {k: batch[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    scratch = ("tmp.", "et.", "bb.")
    runs = []
    for with_maps in (False, True):
        model = _build(cfg, sd, tsv_rows)
        eng = model.engine
        model.train()
        model.zero_grad()
        loss = model(**batch)[0]
        if with_maps:
            torch.cuda.synchronize()
            held = {k: (t, _bits(t).clone()) for k, t in eng.ws.items() if not k.startswith(scratch)}
            state = (eng.seed_base, eng._prefetch, eng.next_input_ids, eng.saved)
            loss0, grad0, data0 = _bits(loss.detach()).clone(), _bits(model._store.grad).clone(), _bits(model._store.data).clone()
            res = model.attention_maps(**inputs, output="both")
            torch.cuda.synchronize()
            assert bool(torch.isfinite(res["modal_mass"]).all())
            for k, (t, bits) in held.items():
                assert eng.ws[k] is t and torch.equal(_bits(t), bits), k
            assert all(k in held or k.startswith(scratch) for k in eng.ws), [k for k in eng.ws if k not in held]
            after = (eng.seed_base, eng._prefetch, eng.next_input_ids, eng.saved)
            assert state[0] == after[0] and all(a is b for a, b in zip(state[1:], after[1:]))
            assert torch.equal(_bits(loss.detach()), loss0)
            assert torch.equal(_bits(model._store.grad), grad0) and torch.equal(_bits(model._store.data), data0)
            assert model.training
        loss.backward()
        eng.join_wgrad()
        torch.cuda.synchronize()
        runs.append((float(loss.detach()), {k: v.detach().clone() for k, v in model.named_grad_views().items()}))
    (l0, g0), (l1, g1) = runs
    assert abs(l0 - l1) <= 1e-5 * abs(l0), (l0, l1)
    worst = max((float((g0[k] - g1[k]).norm() / g0[k].norm().clamp_min(1e-30)), k) for k in g0)
    print(f"loss {l0!r} / {l1!r}; worst relative L2 between the two runs' gradients {worst}")
    assert worst[0] < 1e-4, worst


def test_summarize_modal_mass_equals_the_plain_computation(g2):
    from stonkgs_amd.stonkgs_for_embeddings import summarize_modal_mass

    cfg, full, inputs = g2["cfg"], g2["full"], g2["inputs"]
    half = cfg.half_length
    got = summarize_modal_mass(full["modal_mass"], inputs["attention_mask"], half)
    assert got.shape == (cfg.num_hidden_layers, cfg.num_attention_heads, 2, 2)
    assert float((got.sum(-1) - 1.0).abs().max()) < 1e-5
    live = inputs["attention_mask"].cuda() != 0                          # [B, S]
    for i, a in enumerate(full["attentions"]):
        for h in range(cfg.num_attention_heads):
            for qm, qs in enumerate((slice(0, half), slice(half, None))):
                rows = a[:, h, qs][live[:, qs]]                          # [unmasked queries of that half, S]
                want = torch.stack([rows[:, :half].sum(-1).mean(), rows[:, half:].sum(-1).mean()])
                assert float((got[i, h, qm].cuda() - want).abs().max()) < 1e-5, (i, h, qm)
