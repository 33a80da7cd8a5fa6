"""GPU: the three integer kernels every training step runs before its first GEMM - csrc/unpad.hip (stonk_unpad_plan) and
csrc/data.hip (stonk_mlm_mask, stonk_assemble_rows) - through the C ABI, on the paths their first tests do not reach.

Cases, checks and the launch constants they are sized by live in tests/batch_ref.py; tests/test_batch_ref_cpu.py shows
without a GPU that every case reaches its branch and tells a restatement with one mistake apart. Integer work: every
comparison is EQUALITY with the restatement (oracle/masking_oracle.py), plus invariants that do not go through it. Every
output (and the row plan's workspace) sits at its exact length inside a sentinel frame and is filled with garbage before the
call; every launch is run twice, from different garbage, and the two results are compared bit for bit.
profiles/batch_parity.md records the run on an MI355X, with the mutation table."""
import numpy as np
import pytest
import torch

from oracle import masking_oracle as mo
from tests import batch_ref as br

pytestmark = pytest.mark.gpu

FRAME = 64                                   # sentinel words on either side of an output
SENTINEL = {torch.int32: 0x5EA1ED, torch.int64: 0x5EA1ED5EA1ED}
GARBAGE = (0x0BADF00D, -3)                   # what the outputs hold before the first / the second run


class Framed:
    """`n` words of `dtype` filled with `garbage`, with FRAME sentinel words before and behind them."""

    def __init__(self, n, dtype, garbage):
        self.n, self.sentinel = n, SENTINEL[dtype]
        self.whole = torch.full((n + 2 * FRAME,), self.sentinel, dtype=dtype, device="cuda")
        self.view = self.whole[FRAME:FRAME + n]
        self.view.fill_(garbage)

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        """The output - after asserting that nothing was written outside it."""
        w = self.whole.cpu().numpy()
        assert (w[:FRAME] == self.sentinel).all() and (w[FRAME + self.n:] == self.sentinel).all(), "a write outside the output"
        return w[FRAME:FRAME + self.n].copy()


def _dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ row plan
def _plan_launch(hip, c, read, garbage, inputs):
    B, S = c["am"].shape
    n = B * S
    d_am, d_tl, d_el = inputs
    specs = [(n, torch.int32), (n, torch.int32), (B + 1, torch.int32), (n, torch.int64)]
    if read:
        specs += [(n, torch.int32), (n, torch.int32), (B + 1, torch.int32)]
    outs = [Framed(k, dt, garbage) for k, dt in specs]
    ws_ints = int(hip.lib().stonk_unpad_workspace_ints(B))
    assert ws_ints == br.geometry()["ws_per_seq"] * B
    ws = Framed(ws_ints, torch.int32, garbage)
    ptrs = [o.ptr() for o in outs] + ([] if read else [0, 0, 0])
    hip.call("stonk_unpad_plan", hip.ptr(d_am), hip.ptr(d_tl), hip.ptr(d_el), B, S, c["half"], *ptrs, ws.ptr(), ws_ints,
             hip.stream_ptr())
    torch.cuda.synchronize()
    ws.numpy()
    return [o.numpy() for o in outs]


@pytest.mark.parametrize("name", sorted(br.plan_cases()))
def test_unpad_plan_case(hip, name):
    c = br.plan_cases()[name]
    want = br.plan_expected(name)
    inputs = (_dev(c["am"]), _dev(c["tl"]), _dev(c["el"]))
    facts = br.plan_facts(name)
    print(f"BATCH plan {name}: B {c['am'].shape[0]} S {c['am'].shape[1]} half {c['half']} chunk {facts['per']} idle threads "
          f"{facts['idle']} kept {facts['total']} tail trips {facts['tail_trips']}")
    for read in (True, False):
        first = _plan_launch(hip, c, read, GARBAGE[0], inputs)
        second = _plan_launch(hip, c, read, GARBAGE[1], inputs)
        for key, a, b, w in zip(br.PLAN_NAMES, first, second, want):
            assert a.dtype == w.dtype and a.tobytes() == b.tobytes(), (key, "two runs differ")
            assert np.array_equal(a, w), (key, read, int((a != w).sum()), "elements differ from the restatement")
        assert br.plan_invariants(c, first, read=read) == facts["total"]


def _plan_inputs(S, half, seed):
    c = br._plan_random(5, S, half, seed)
    c["am"][1] = 0                                          # a sequence without a live key
    return c


def _check_engine_plan(engine, c, half):
    B, S = c["am"].shape
    d_am, d_tl, d_el = _dev(c["am"]), _dev(c["tl"]), _dev(c["el"])
    plan, ev = engine._plan_rows(d_am, d_tl, d_el, B, S, half, keep=False)
    ev.synchronize()
    want = mo.unpad_plan(c["am"], c["tl"], c["el"], read=True, half=half)
    got = [plan[k].cpu().numpy() for k in ("row_of_pos", "pos_of_row", "cu", "row_mask", "read_rows", "read_of_pos", "cu_rd")]
    for key, a, w in zip(br.PLAN_NAMES, got, want):
        assert np.array_equal(a, w), key
    br.plan_invariants(dict(c, half=half), got)
    assert engine._plan_host[:2 * (B + 1)].tolist() == want[2].tolist() + want[6].tolist()       # what the host learns
    return got


def test_text_engine_plans_rows_with_half_zero(hip):
    """The text baseline's call: TextEngine.half_length is 0, so no label is read and only mask words and position 0 keep
    a row - against unpad_plan(..., half=0)."""
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.nlp_baseline_model import BertForSequenceClassification

    cfg = STonKGsConfig(vocab_size=160, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                        max_position_embeddings=256)
    engine = BertForSequenceClassification(cfg, num_labels=3).engine
    assert engine.half_length == 0
    c = _plan_inputs(256, 0, 31)
    got = _check_engine_plan(engine, c, engine.half_length)
    assert int(got[6][-1]) == 5                                 # one read row per sequence: its position 0
    engine.check_errors()


def test_joint_engine_plans_rows_with_its_half(hip):
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    cfg = STonKGsConfig(vocab_size=640, kg_vocab_size=400, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                        intermediate_size=256, max_position_embeddings=256)
    table = torch.randn(400, 128, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 0.3
    engine = STonKGsForPreTraining(cfg, kg_embeddings=table, backbone_layers=1).engine
    assert engine.half_length == 128
    _check_engine_plan(engine, _plan_inputs(256, 128, 32), engine.half_length)
    engine.check_errors()


# ------------------------------------------------------------------------------------------------ masking
def _mask_launch(hip, c, garbage, d_ids):
    B, S = c["ids"].shape
    outs = [Framed(B * S, torch.int64, garbage), Framed(B * c["half"], torch.int64, garbage),
            Framed(B * c["half"], torch.int64, garbage)]
    hip.call("stonk_mlm_mask", hip.ptr(d_ids), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), B, S, c["half"], c["vocab_text"],
             c["vocab_ent"], c["mask_id"], c["k_text"], c["k_ent"], c["seed"], hip.stream_ptr())
    torch.cuda.synchronize()
    return [o.numpy().reshape(B, -1) for o in outs]


@pytest.mark.parametrize("name", sorted(br.mask_cases()))
def test_mlm_mask_case(hip, name):
    c = br.mask_cases()[name]
    want = br.mask_expected(name)
    d_ids = _dev(c["ids"])
    first, second = _mask_launch(hip, c, GARBAGE[0], d_ids), _mask_launch(hip, c, GARBAGE[1], d_ids)
    print(f"BATCH mask {name}: B {c['ids'].shape[0]} half {c['half']} k {c['k_text']}/{c['k_ent']} vocab {c['vocab_text']}/"
          f"{c['vocab_ent']} changed ids {int((first[0] != c['ids']).sum())}")
    for key, a, b, w in zip(("ids", "text_labels", "ent_labels"), first, second, want):
        assert a.dtype == np.int64 and a.tobytes() == b.tobytes(), (key, "two runs differ")
        assert np.array_equal(a, w), (key, int((a != w).sum()), "elements differ from the restatement")
    br.mask_invariants(c, first)
    assert np.array_equal(d_ids.cpu().numpy(), c["ids"])         # the input is read, never written


# ------------------------------------------------------------------------------------------------ assembly
def _assemble_launch(hip, c, garbage, inputs):
    B, half = c["text"].shape
    S = 2 * half
    outs = [Framed(B * S, torch.int64, garbage) for _ in range(3)] + [Framed(B, torch.int64, garbage)]
    err = torch.zeros(1 + 2 * FRAME, dtype=torch.int32, device="cuda")
    d_text, d_att, d_src, d_tgt, d_walks = inputs
    hip.call("stonk_assemble_rows", hip.ptr(d_text), hip.ptr(d_att), hip.ptr(d_src), hip.ptr(d_tgt), hip.ptr(d_walks),
             c["walks"].shape[0], c["walks"].shape[1], outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), outs[3].ptr(), B, S, half,
             br.SEP, c["rate"], c["seed"], err[FRAME:].data_ptr(), hip.stream_ptr())
    torch.cuda.synchronize()
    e = err.cpu().numpy()
    assert not e[:FRAME].any() and not e[FRAME + 1:].any(), "a write beside the error word"
    return [o.numpy().reshape(B, -1) for o in outs[:3]] + [outs[3].numpy(), int(e[FRAME])]


@pytest.mark.parametrize("name", sorted(br.assemble_cases()))
def test_assemble_rows_case(hip, name):
    c = br.assemble_cases()[name]
    want = br.assemble_expected(name)
    inputs = tuple(_dev(c[k]) for k in ("text", "att", "source", "target", "walks"))
    first, second = _assemble_launch(hip, c, GARBAGE[0], inputs), _assemble_launch(hip, c, GARBAGE[1], inputs)
    print(f"BATCH assemble {name}: B {c['text'].shape[0]} half {c['half']} rate {c['rate']} seed {c['seed']:#x} nsp "
          f"{first[3].tolist()} rows {[r[2] for r in br.assemble_rows_of(c)]} error bit {first[4]}")
    for key, a, b, w in zip(("ids", "attention", "types", "nsp"), first, second, want):
        assert a.tobytes() == b.tobytes(), (key, "two runs differ")
        assert np.array_equal(a, w), (key, int((a != w).sum()), "elements differ from the restatement")
    assert first[4] == second[4] == want[4] == int(c["bad"])
    if c["bad"]:                                               # zeros: one walk's length per read of a bad node, no more
        n_nodes, W = c["walks"].shape
        reads = sum(int(not 0 <= int(nodes[row]) < n_nodes) for _, _, row in br.assemble_rows_of(c)
                    for nodes in (c["source"], c["target"]))
        assert reads >= 1 and int((first[0][:, c["half"]:] == 0).sum()) == W * reads
    else:
        br.assemble_invariants(c, first)


# ------------------------------------------------------------------------------------------------ DeviceBatcher
@pytest.mark.parametrize("half", [4, 100])
def test_device_batcher_hands_k_and_the_float_rate_to_the_kernels(hip, half):
    """DeviceBatcher at halves other than 128 / 256: k = int(half * 0.15) - 0 at half 4, 15 at half 100 - must reach
    stonk_mlm_mask, the rate crosses the ABI as a float, and the batch equals the restatement."""
    from stonkgs_amd.data import DeviceBatcher

    c = br.assemble_cases()["h4" if half == 4 else "h100"]
    B, V, K = c["text"].shape[0], 28996, 175094
    bat = DeviceBatcher(torch.tensor(c["walks"]), V, K, half=half, seed=11)
    assert bat.k == int(half * 0.15) == {4: 0, 100: 15}[half]
    for step in (0, 3):
        got = {k: v.cpu().numpy() for k, v in bat(*(torch.tensor(c[k]) for k in ("text", "att", "source", "target")), step).items()}
        seed = bat.step_seed(step)
        raw, a, t, nsp = mo.assemble_rows(c["text"], c["att"], c["source"], c["target"], c["walks"], negative_rate=0.2, seed=seed)
        ids, tl, el = mo.mlm_mask(raw, half, V, K, seed=seed ^ 0x5BD1E995)
        assert np.array_equal(got["input_ids"], ids)
        assert np.array_equal(got["masked_lm_labels"], tl) and np.array_equal(got["ent_masked_lm_labels"], el)
        assert np.array_equal(got["attention_mask"], a) and np.array_equal(got["token_type_ids"], t)
        assert np.array_equal(got["next_sentence_labels"], nsp)
        assert ((tl != -100).sum(axis=1) == bat.k).all() and ((el != -100).sum(axis=1) == bat.k).all()
        br.mask_invariants(dict(ids=raw, half=half, k_text=bat.k, k_ent=bat.k, vocab_text=V, vocab_ent=K, mask_id=103),
                           (got["input_ids"], got["masked_lm_labels"], got["ent_masked_lm_labels"]))
    bat.check_errors()
