"""GPU: one training step of a small model (hidden 256, intermediate 1024 - the smallest the four-wave weight-gradient kernel
takes once `tn_min_k` / `tn_min_tiles` are lowered) with `Engine.wgrad_groups` empty, {"attn"}, {"ffn"} and both.

Grouping changes which launch adds a layer's weight gradients and in how many K shares - nothing else: the loss is
bit-equal, the operands of every weight gradient are bit-equal (captured where the launch forks from the main stream:
a held operand that something overwrote would show here), GemmTimer's FLOPs are equal, and every gradient of a grouped
weight lies within tests/gemm_ref.py's bound of float64 dY^T X on the captured operands and of the ungrouped run. K = the
rows of the contraction; adds = the most K shares the routing can choose (K tiles / 8) + 1, for a bias times the column
tiles that share the bias duty.
Every other gradient tensor runs the same launches in all four runs; they add fp32 terms over at most R = B x S rows in
no fixed order, so two runs may differ by R x 2^-23 x (sum of |terms|); the test allows R x 2^-23 x max |gradient| - the
sum of |terms| is not smaller."""
import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

DIMS = dict(vocab_size=2048, kg_vocab_size=300, hidden_size=256, num_hidden_layers=3, num_attention_heads=4,
            intermediate_size=1024, max_position_embeddings=256, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
B, S = 8, 256
PAIRS = {"attn": (".attention.self.qkv", ".attention.output.dense"), "ffn": (".output.dense", ".intermediate.dense")}
GROUPS = ((), ("attn",), ("ffn",), ("attn", "ffn"))


def _model(hip, groups):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    rows = torch.randn(300, 256, generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 0.3
    torch.manual_seed(3)
    model = STonKGsForPreTraining(STonKGsConfig(**DIMS), kg_embeddings=rows)
    model.train()
    eng = model.engine
    eng.tn_min_k, eng.tn_min_tiles = 512, 4
    eng.wgrad_groups = frozenset(groups)
    return model


def _step(hip, monkeypatch, groups):
    from stonkgs_amd.data import synthetic_batch
    from stonkgs_amd.engine import GemmTimer

    model = _model(hip, groups)
    eng, st = model.engine, model._store
    names, ops = [], {}
    call = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    wgrad, wgrad_group = eng.wgrad, eng.wgrad_group

    def capture(dy, x, dW, db, M, N, T, k_dev=None, **kw):
        if k_dev is None:
            ops[dW.data_ptr()] = (dy[:T, :M].clone(), x[:T, :N].clone(), T, db is not None)

    def one(*a, **kw):
        capture(*a, **kw)
        return wgrad(*a, **kw)

    def many(members):
        for m in members:
            capture(*m)
        return wgrad_group(members)

    eng.wgrad, eng.wgrad_group = one, many
    eng.gemm_timer = GemmTimer()
    model.zero_grad()
    batch = synthetic_batch(B, DIMS["vocab_size"], DIMS["kg_vocab_size"], S, seed=20, min_text=16)
    loss = model.forward_backward(batch)
    torch.cuda.synchronize()
    eng.check_errors()
    flops = {k: eng.gemm_timer.summarize(k)["flops"] for k in (None, "tn_a4", "tn")}
    launches = eng.gemm_timer.summarize("tn_a4")["launches"]
    eng.gemm_timer = None
    layer = {}
    for i in range(DIMS["num_hidden_layers"]):
        for suffix in PAIRS["attn"] + PAIRS["ffn"]:
            name = f"bert.encoder.layer.{i}{suffix}"
            dy, x, T, _ = ops[st.grad_view(name + ".weight").data_ptr()]
            layer[name] = (dy, x, T, st.grad_view(name + ".weight").clone(), st.grad_view(name + ".bias").clone())
    return dict(model=model, loss=loss.clone(), grad=st.grad.clone(), flops=flops, launches=launches, names=list(names),
                log=list(eng.group_log), layer=layer, batch=batch)


@pytest.fixture(scope="module")
def runs(hip):
    mp = pytest.MonkeyPatch()
    try:
        out = {g: _step(hip, mp, g) for g in GROUPS}
    finally:
        mp.undo()
    return out


def _expected_groups(eng, base, kind):
    """Layers whose pair the documented rule groups: one row count, both members the four-wave kernel's."""
    n = 0
    for i in range(DIMS["num_hidden_layers"]):
        a, b = (base["layer"][f"bert.encoder.layer.{i}{s}"] for s in PAIRS[kind])
        shapes = [(t[3].shape[0], t[3].shape[1], t[2]) for t in (a, b)]
        n += shapes[0][2] == shapes[1][2] and all(eng._split_k(M, N, T, True) <= 0 for M, N, T in shapes)
    return n


def test_launches_taken(hip, runs):
    """Which entry ran: grouped launches where the members share a row count, single launches for the pruned last layer's
    attention pair (its output projection runs on the read rows, the QKV projection on all rows) and for everything when
    the switch is off; the timer sees one launch per group and the same FLOPs."""
    base = runs[()]
    eng = base["model"].engine
    last = DIMS["num_hidden_layers"] - 1
    qkv, out = (base["layer"][f"bert.encoder.layer.{last}{s}"] for s in PAIRS["attn"])
    assert qkv[2] != out[2], "the last layer's attention pair must differ in rows for this test"
    n_single = base["names"].count("stonk_gemm_tn_bf16")
    assert not base["log"] and "stonk_gemm_tn_bf16_group" not in base["names"]
    want = {k: _expected_groups(eng, base, k) for k in PAIRS}
    assert want["attn"] == last and 1 <= want["ffn"] <= last + 1, want
    for g in GROUPS[1:]:
        r = runs[g]
        n = sum(want[k] for k in g)
        assert r["log"] == [(2, hip.OK)] * n, (g, r["log"])
        assert r["names"].count("stonk_gemm_tn_bf16") == n_single - 2 * n, g
        assert r["launches"] == base["launches"] - n, g
        assert r["flops"] == base["flops"], (g, r["flops"], base["flops"])
    print("GROUPS", want, "single TN launches ungrouped:", n_single, "FLOPs", base["flops"])


def test_loss_and_operands_are_bit_equal(hip, runs):
    base = runs[()]
    for g in GROUPS[1:]:
        r = runs[g]
        assert torch.equal(r["loss"], base["loss"]), g
        for name, (dy, x, T, _, _) in r["layer"].items():
            bdy, bx, bT, _, _ = base["layer"][name]
            assert T == bT and torch.equal(dy, bdy) and torch.equal(x, bx), (g, name)


def test_gradients_within_the_bound(hip, runs):
    base = runs[()]
    st = base["model"]._store
    used = 0.0
    spans = []
    for name, (dy, x, T, _, _) in base["layer"].items():
        dyd, xd = dy.double(), x.double()
        dW, db = (dyd.t() @ xd).cpu(), dyd.sum(0).cpu()
        Sw, Sb = (dyd.abs().t() @ xd.abs()).cpu(), dyd.abs().sum(0).cpu()
        shares = max(1, ((T + 63) // 64) // 8)
        ntn = (x.shape[1] + 255) // 256
        spans += [st.span(name + ".weight"), st.span(name + ".bias")]
        for g in GROUPS:
            _, _, _, gw, gb = runs[g]["layer"][name]
            nm = f"{name} groups {g}"
            used = max(used, gr.check_bound(nm + " dW", gw, dW, Sw, T, shares + 1, torch.float32))
            used = max(used, gr.check_bound(nm + " db", gb, db, Sb, T, shares * ntn + 1, torch.float32))
            if g:
                _, _, _, bw, bb = base["layer"][name]
                used = max(used, gr.check_bound(nm + " dW against ungrouped", gw, bw.double().cpu(), Sw, T, shares + 1, torch.float32))
                used = max(used, gr.check_bound(nm + " db against ungrouped", gb, bb.double().cpu(), Sb, T, shares * ntn + 1,
                                                torch.float32))
    assert used <= 1.0
    # every other gradient tensor: the same launches in all four runs
    others = [name for name in st.index if st.span(name) not in spans]
    assert len(others) + len(spans) == len(st.index) and len(others) > 10
    for g in GROUPS[1:]:
        for name in others:
            lo, hi = st.span(name)
            a, b = runs[g]["grad"][lo:hi], base["grad"][lo:hi]
            tol = B * S * 2.0 ** -23 * float(b.abs().max())
            assert float((a - b).abs().max()) <= tol, (g, name, float((a - b).abs().max()), tol)


def test_inputs_only_backward_launches_no_weight_gradient(hip, runs, monkeypatch):
    """`_inputs_only` (input_attributions): no weight gradient at all with both groups on - no grouped launch, no single one,
    the gradient buffer untouched."""
    r = runs[("attn", "ffn")]
    model, batch = r["model"], r["batch"]
    eng = model.engine
    names = []
    call = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    eng.group_log.clear()
    before = model._store.grad.clone()
    labels = {k: batch[k] for k in ("masked_lm_labels", "ent_masked_lm_labels", "next_sentence_labels")}
    inputs = {k: batch[k] for k in ("input_ids", "attention_mask", "token_type_ids") if k in batch}
    model.input_attributions(**inputs, labels=labels)
    torch.cuda.synchronize()
    eng.check_errors()
    assert "stonk_attention_bwd" in names                     # the backward chain ran
    assert not eng.group_log and not [n for n in names if n.startswith("stonk_gemm_tn")]
    assert torch.equal(model._store.grad, before)
