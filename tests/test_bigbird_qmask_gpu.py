"""stonk_block_sparse_attention_fwd_ex / _bwd_ex with STONK_BSA_ZERO_MASKED_QUERIES on the GPU: HuggingFace's rule for a
masked query (context_layer * from_mask, modeling_big_bird.py:617). Reference, bounds and the per-block rule are those of
tests/bigbird_ref.py, with out o mask and dout o mask: the masked rows of out and dq must be EXACT zeros, nothing of them may
reach dk / dv, the live rows of the forward must equal the flag-less run bit for bit, every launch must repeat bit for bit,
outputs sit between sentinel rows, and the entries without `flags` must still give what they gave."""
import pytest
import torch

from stonkgs_amd import _hip as hip
from stonkgs_amd.bigbird_attention import BlockSparsePlan, bigbird_rand_attn, block_sparse_attention
from tests import bigbird_ref as br
from tests.parity_util import gen

pytestmark = pytest.mark.gpu
ZQ = hip.BSA_ZERO_MASKED_QUERIES
GUARD = 64     # sentinel rows in front of and behind every output


def _mask(B, S, edits):
    m = torch.ones(B, S, dtype=torch.long)
    for b, lo, hi in edits:
        m[b, lo:hi] = 0
    return m


def _cases():
    cs = [
        # the kernels' minimum: 5 blocks; holes inside blocks 1 and 3
        br._case("s320", 1, 2, 320, 1, "train", 31, plan_seed=3, mask=_mask(1, 320, [(0, 70, 90), (0, 200, 230)])),
        # holes inside a block, a fully masked inner query block (block 2), masked rows in blocks 0 and nb - 1
        br._case("s384-holes", 2, 2, 384, 3, "train", 32, plan_seed=4,
                 mask=_mask(2, 384, [(0, 3, 9), (0, 70, 90), (0, 128, 192), (0, 370, 384), (1, 384 - 100, 384)])),
        # one sequence of two without any live key
        br._case("s384-nokey", 2, 1, 384, 3, "train", 33, plan_seed=5, mask=_mask(2, 384, [(0, 0, 384), (1, 200, 230)])),
        # 64 blocks, once
        br._case("s4096", 1, 1, 4096, 3, "eval", 34, mask=_mask(1, 4096, [(0, 5, 9), (0, 1024, 1088), (0, 4096 - 1000, 4096)])),
    ]
    return {c["name"]: c for c in cs}


CASES = _cases()
_cache = {}


def _setup(name):
    """plan, inputs and the three references with out o mask / dout o mask - made once per case."""
    if name not in _cache:
        c = CASES[name]
        plan = BlockSparsePlan(c["nb"], bigbird_rand_attn(c["nb"], c["r"], c["NH"], c["mode"], seed=c["plan_seed"]))
        H = c["NH"] * 64
        g = gen(c["data_seed"])
        qkv = (torch.randn(c["T"], 3 * H, generator=g) * 1.5).to(torch.bfloat16)
        dout = torch.randn(c["T"], H, generator=g).to(torch.bfloat16)
        live = (c["mask"].view(-1, 1) != 0)
        refs = []
        for mode in ("r64", "r32", "r16"):
            r = br.compute(c, plan.lists, qkv, dout * live.to(dout.dtype), mode)
            r["out"] = r["out"] * live.to(r["out"].dtype)
            if mode == "r64":
                r["E_out"] = r["E_out"] * live.to(r["E_out"].dtype)
            refs.append(r)
        _cache[name] = (c, plan, qkv, dout, live.view(-1), tuple(refs))
    return _cache[name]


def _guarded(rows, cols, dev):
    t = torch.full((rows + 2 * GUARD, cols), br.OUT_SENTINEL, dtype=torch.bfloat16, device=dev)
    return t, t[GUARD:GUARD + rows]


def _guards_intact(t):
    return bool((t[:GUARD] == br.OUT_SENTINEL).all()) and bool((t[-GUARD:] == br.OUT_SENTINEL).all())


def _run(c, plan, qkv_cpu, dout_cpu, flags, ex=True):
    """Forward and backward through the C ABI; returns CPU tensors (out, lse, dqkv). Guards are asserted."""
    dev = torch.device("cuda")
    B, NH, S, T = c["B"], c["NH"], c["S"], c["T"]
    H = NH * 64
    qkv, dout = qkv_cpu.to(dev), dout_cpu.to(dev)
    mask = c["mask"].to(dev)
    lists, err = plan.on(dev)
    full_out, out = _guarded(T, H, dev)
    full_dqkv, dqkv = _guarded(T, 3 * H, dev)
    lse = torch.full((B, NH, S), float("nan"), device=dev)
    ws = torch.empty(2, B, NH, S, device=dev)
    p, g, st = qkv.data_ptr(), dqkv.data_ptr(), hip.stream_ptr()
    tail = (flags, st) if ex else (st,)
    sfx = "_ex" if ex else ""
    hip.call("stonk_block_sparse_attention_fwd" + sfx, p, p + 2 * H, p + 4 * H, 3 * H, mask.data_ptr(),
             *(t.data_ptr() for t in lists[:3]), out.data_ptr(), H, lse.data_ptr(), B, NH, S, 64, c["scale"], err.data_ptr(), *tail)
    hip.call("stonk_block_sparse_attention_bwd" + sfx, p, p + 2 * H, p + 4 * H, 3 * H, mask.data_ptr(),
             *(t.data_ptr() for t in lists), out.data_ptr(), H, dout.data_ptr(), H, lse.data_ptr(), ws.data_ptr(), g, g + 2 * H,
             3 * H, g + 4 * H, B, NH, S, 64, c["scale"], err.data_ptr(), *tail)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    assert _guards_intact(full_out) and _guards_intact(full_dqkv), "a kernel wrote outside its output"
    return dict(out=out.cpu(), lse=lse.cpu(), dqkv=dqkv.cpu(), delta=ws[0].cpu())


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int16) if a[k].dtype == torch.bfloat16 else a[k].view(torch.int32),
                           b[k].view(torch.int16) if b[k].dtype == torch.bfloat16 else b[k].view(torch.int32)) for k in a)


@pytest.mark.parametrize("name", list(CASES))
def test_masked_queries_are_zero_and_the_rest_is_the_reference(name):
    c, plan, qkv, dout, live, refs = _setup(name)
    H = c["NH"] * 64
    got = _run(c, plan, qkv, dout, ZQ)
    again = _run(c, plan, qkv, dout, ZQ)
    assert _same(got, again), "two launches on the same inputs differ"
    # masked rows: exact zeros in out and dq, a zero delta, a finite lse
    assert int((~live).sum()) > 0
    assert not bool(got["out"][~live].float().abs().max() > 0)
    assert not bool(got["dqkv"][~live][:, :H].float().abs().max() > 0)
    delta = got["delta"].permute(0, 2, 1).reshape(c["T"], c["NH"])
    assert not bool(delta[~live].abs().max() > 0)
    assert bool(torch.isfinite(got["lse"]).all())
    # a sequence without any live key: everything zero
    for b in range(c["B"]):
        if not bool(c["mask"][b].any()):
            rows = slice(b * c["S"], (b + 1) * c["S"])
            assert not bool(got["out"][rows].float().abs().max() > 0) and not bool(got["dqkv"][rows].float().abs().max() > 0)
    # everything against r (out o mask, dout o mask): per element, per (sequence, head) block against r16
    br.check(c, plan.lists, refs, dict(out=got["out"], lse=got["lse"], dqkv=got["dqkv"]), name, label="bigbird_qmask")


@pytest.mark.parametrize("name", ["s320", "s384-holes", "s384-nokey"])
def test_flagless_runs_are_unchanged_and_live_rows_do_not_see_the_flag(name):
    c, plan, qkv, dout, live, _ = _setup(name)
    H = c["NH"] * 64
    zq = _run(c, plan, qkv, dout, ZQ)
    plain = _run(c, plan, qkv, dout, 0)
    old = _run(c, plan, qkv, dout, 0, ex=False)
    assert _same(plain, old), "the entries without `flags` no longer equal flags = 0"
    assert _same(old, _run(c, plan, qkv, dout, 0, ex=False))
    # the flag-less run is the list formulation's: its masked rows are NOT zero (what tells the feature from it) ...
    some_key_live = torch.tensor([bool(c["mask"][b].any()) for b in range(c["B"])]).repeat_interleave(c["S"])
    assert bool(plain["out"][~live & some_key_live].float().abs().max() > 0)
    # ... and the forward's live rows, and the whole lse, are the same bits with and without the flag
    assert torch.equal(zq["out"][live].view(torch.int16), plain["out"][live].view(torch.int16))
    assert torch.equal(zq["lse"].view(torch.int32), plain["lse"].view(torch.int32))
    # the flag-less results still satisfy the flag-less reference
    refs = tuple(br.compute(c, plan.lists, qkv, dout, m) for m in ("r64", "r32", "r16"))
    br.check(c, plan.lists, refs, dict(out=old["out"], lse=old["lse"], dqkv=old["dqkv"]), name, label="bigbird_flagless")
    # dq of a live row depends on that row alone (its q, dO, delta, lse and the keys): the same bits with and without the flag
    assert torch.equal(zq["dqkv"][live][:, :H].contiguous().view(torch.int16),
                       plain["dqkv"][live][:, :H].contiguous().view(torch.int16))


def test_autograd_op_and_module_take_the_flag():
    c, plan, qkv, dout, live, refs = _setup("s384-holes")
    dev = torch.device("cuda")
    q = qkv.to(dev).requires_grad_(True)
    out = block_sparse_attention(q, c["mask"].to(dev), plan, c["NH"], scale=c["scale"], zero_masked_queries=True)
    out.backward(dout.to(dev))
    direct = _run(c, plan, qkv, dout, ZQ)
    assert torch.equal(out.detach().cpu().view(torch.int16), direct["out"].view(torch.int16))
    assert torch.equal(q.grad.cpu().view(torch.int16), direct["dqkv"].view(torch.int16))
    # without a mask the flag changes nothing
    a = block_sparse_attention(q.detach(), None, plan, c["NH"], zero_masked_queries=True)
    b = block_sparse_attention(q.detach(), None, plan, c["NH"])
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
