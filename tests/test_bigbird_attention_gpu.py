"""GPU parity of the block-sparse attention kernels (stonk_block_sparse_attention_fwd / _bwd), the autograd op and the module
over them against a float64 reference, element by element: out, lse, dQ, dK and dV of every case of tests/bigbird_ref.py -
every row kind of BigBird's pattern at the smallest sizes that have them, the minimum and maximum number of blocks, drawn and
eval-mode plans (multiplicity 4 on block 0), masked keys, a dead global block, a sequence with no live key, exact
probability masses. Operands and outputs are strided views inside sentinel-filled allocations. Reference, bounds and cases:
tests/bigbird_ref.py (its CPU self-check: test_bigbird_ref_cpu.py); figures of one run: profiles/bigbird_attention.md."""
import pytest
import torch

from stonkgs_amd import bigbird_attention as bb
from tests import bigbird_ref as br

pytestmark = pytest.mark.gpu

PAD_R, PAD_C = 1, 8      # rows above / below and columns left / right of a view inside its allocation
_RESULTS = {}


def _framed(rows, cols, fill, dtype=torch.bfloat16, src=None):
    """A [rows, cols] view (row stride cols + 16, 16-byte aligned) inside an allocation filled with `fill`."""
    full = torch.full((rows + 2 * PAD_R, cols + 2 * PAD_C), fill, device="cuda", dtype=dtype)
    view = full[PAD_R:PAD_R + rows, PAD_C:PAD_C + cols]
    if src is not None:
        view.copy_(src)
    return full, view


def _flat_framed(n, fill):
    full = torch.full((n + 128,), fill, device="cuda", dtype=torch.float32)
    return full, full[64:64 + n]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _frame_intact(full, view_slices, fill):
    probe = full.clone()
    probe[view_slices] = fill
    return torch.equal(_bits(probe), _bits(torch.full_like(full, fill)))


def _launch(hip, c, lists_dev, err, qkv_v, mask, dout_v):
    """One forward and one backward into fresh sentinel-filled allocations; returns the views and the allocations."""
    B, NH, S, T = c["B"], c["NH"], c["S"], c["T"]
    H = NH * 64
    N = B * NH * S
    out_f, out = _framed(T, H, br.OUT_SENTINEL)
    lse_f, lse = _flat_framed(N, float("nan"))
    ws_f, ws = _flat_framed(2 * N, float("nan"))
    dqkv_f, dqkv = _framed(T, 3 * H, br.OUT_SENTINEL)
    ld = qkv_v.stride(0)
    q = qkv_v.data_ptr()
    head = (q, q + 2 * H, q + 4 * H, ld, hip.ptr(mask))
    tail = (B, NH, S, 64, c["scale"], hip.ptr(err), hip.stream_ptr())
    hip.call("stonk_block_sparse_attention_fwd", *head, *(hip.ptr(t) for t in lists_dev[:3]), out.data_ptr(), out.stride(0),
             lse.data_ptr(), *tail)
    g = dqkv.data_ptr()
    hip.call("stonk_block_sparse_attention_bwd", *head, *(hip.ptr(t) for t in lists_dev), out.data_ptr(), out.stride(0),
             dout_v.data_ptr(), dout_v.stride(0), lse.data_ptr(), ws.data_ptr(), g, g + 2 * H, dqkv.stride(0), g + 4 * H, *tail)
    rows = slice(PAD_R, PAD_R + T)
    frames = dict(out=(out_f, (rows, slice(PAD_C, PAD_C + H)), br.OUT_SENTINEL),
                  dqkv=(dqkv_f, (rows, slice(PAD_C, PAD_C + 3 * H)), br.OUT_SENTINEL),
                  lse=(lse_f, (slice(64, 64 + N),), float("nan")), ws=(ws_f, (slice(64, 64 + 2 * N),), float("nan")))
    return dict(out=out, lse=lse.view(B, NH, S), dqkv=dqkv), frames


def _run(hip, name):
    """The case's forward and backward, twice: the outputs on the CPU, what the frames and the repeat showed."""
    if name in _RESULTS:
        return _RESULTS[name]
    c = br.CASES[name]
    H = c["NH"] * 64
    qkv, dout = br.inputs(name)
    qkv_f, qkv_v = _framed(c["T"], 3 * H, 3.0, src=qkv.cuda())
    dout_f, dout_v = _framed(c["T"], H, 3.0, src=dout.cuda())
    operands = (qkv_f.clone(), dout_f.clone())
    mask = None if c["mask"] is None else c["mask"].cuda()
    lists_dev, err = br.plan(name).on("cuda")
    first, frames = _launch(hip, c, lists_dev, err, qkv_v, mask, dout_v)
    second, _ = _launch(hip, c, lists_dev, err, qkv_v, mask, dout_v)
    torch.cuda.synchronize()
    got = {k: v.cpu().contiguous() for k, v in first.items()}
    got["err"] = int(err.item())
    got["repeat_differs"] = {k: int((_bits(first[k]) != _bits(second[k])).sum()) for k in first}
    got["frames_intact"] = {k: _frame_intact(*f) for k, f in frames.items()}
    got["operands_intact"] = torch.equal(_bits(qkv_f), _bits(operands[0])) and torch.equal(_bits(dout_f), _bits(operands[1]))
    _RESULTS[name] = got
    return got


@pytest.mark.parametrize("name", list(br.CASES))
def test_block_sparse_attention_against_float64(hip, name):
    got = _run(hip, name)
    assert got["err"] == 0
    br.check_case(name, got)      # every element of out, lse, dq, dk, dv (all of them are written); finiteness
    assert got["frames_intact"] == dict(out=True, dqkv=True, lse=True, ws=True), got["frames_intact"]
    assert got["operands_intact"]
    assert got["repeat_differs"] == dict(out=0, lse=0, dqkv=0), got["repeat_differs"]      # bitwise repeatable


@pytest.mark.parametrize("name", ["exact-s512-drawn", "exact-s512-eval"])
def test_probability_masses_are_exact(hip, name):
    """q = 0 and V[key, c] = [c == key // 64]: out[row, c] is the probability mass on key block c - exactly 0.0 for a block
    that is not in the row's list, m / L bit for bit where the row's total multiplicity L is a power of two (8 on the middle
    and the global rows), within one bf16 rounding on the others (7 on rows of blocks 1 and nb-2)."""
    c = br.CASES[name]
    nb, NH = c["nb"], c["NH"]
    out = _run(hip, name)["out"].double().view(c["T"], NH, 64)
    want, pow2 = br.exact_masses(name)
    mass = out[:, :, :nb]
    assert bool((out[:, :, nb:] == 0).all())
    assert bool((mass[want == 0] == 0).all()), "mass on a block that is not listed"
    assert int(pow2.sum()) >= c["T"] * NH // 2 and not bool(pow2.all())
    exact = pow2[:, :, None].expand_as(want)
    assert torch.equal(mass[exact], want[exact]), f"{int((mass[exact] != want[exact]).sum())} masses differ from m / L"
    err = (mass - want).abs()
    assert bool((err[~exact] <= br.U * want[~exact]).all()), float((err[~exact] / want[~exact].clamp(min=1e-30)).max())
    print(f"EXACT {name}: {int(exact.sum())} masses bit for bit, {int((~exact).sum())} within 2^-8 relative "
          f"(largest {float((err[~exact] / want[~exact].clamp(min=1e-30)).max()):.2e})")


def test_out_of_range_list_entries_set_the_error_bit_and_touch_nothing_else(hip):
    """One corrupted entry on a copy of a valid plan at S = 384: the forward sets bit 0 of the error word, the other
    (head, block) outputs are bitwise the valid run's, nothing faults. bb_list() (csrc/bigbird_attention.hip) reads a count,
    clamps it to [0, nb], reads that many entries of a row of nb and uses a block index only after comparing it with nb: the
    bad value never becomes an address. The same for an entry of the inverse lists in the backward, and through the op."""
    name = "s384-drawn"
    c = br.CASES[name]
    H, S = c["NH"] * 64, c["S"]
    good = _run(hip, name)
    qkv, dout = (t.cuda() for t in br.inputs(name))
    _, qkv_v = _framed(c["T"], 3 * H, 3.0, src=qkv)
    _, dout_v = _framed(c["T"], H, 3.0, src=dout)
    lists = {k: v.copy() for k, v in br.plan(name).lists.items()}
    lists["key_blocks"][0, 2, 1] = 99            # head 0, query block 2
    lists["query_mult"][1, 3, 0] = 0             # head 1, key block 3
    plan = bb.BlockSparsePlan.from_lists(lists)
    lists_dev, err = plan.on("cuda")
    got, frames = _launch(hip, c, lists_dev, err, qkv_v, None, dout_v)
    torch.cuda.synchronize()
    assert int(err.item()) & 1
    err.zero_()
    assert all(_frame_intact(*f) for f in frames.values())
    out, dqkv = got["out"].cpu(), got["dqkv"].cpu()
    rows = torch.ones(c["T"], dtype=torch.bool)
    rows.view(c["B"], S)[:, 2 * 64:3 * 64] = False
    assert torch.equal(_bits(out[rows]), _bits(good["out"][rows]))                   # every query block but 2 ...
    assert torch.equal(_bits(out[:, 64:]), _bits(good["out"][:, 64:]))               # ... and all of head 1
    assert not torch.equal(_bits(out[~rows, :64]), _bits(good["out"][~rows, :64]))   # (block 2 of head 0 lost an entry)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    assert torch.equal(_bits(dqkv[:, 64:H]), _bits(good["dqkv"][:, 64:H]))           # dq of head 1: the forward lists of head 1 are intact
    krows = torch.ones(c["T"], dtype=torch.bool)
    krows.view(c["B"], S)[:, 3 * 64:4 * 64] = False
    for lo in (H + 64, 2 * H + 64):      # dk, dv of head 1: every key block but 3
        assert torch.equal(_bits(dqkv[krows, lo:lo + 64]), _bits(good["dqkv"][krows, lo:lo + 64]))
    with pytest.raises(IndexError):
        bb.block_sparse_attention(qkv, None, plan, c["NH"], scale=c["scale"])
    assert int(err.item()) == 0          # (the op cleared the word it raised for)


def test_autograd_op_gradient_is_the_references(hip):
    name = "s384-mask"
    c = br.CASES[name]
    qkv, dout = (t.cuda() for t in br.inputs(name))
    x = qkv.clone().requires_grad_(True)
    out = bb.block_sparse_attention(x, c["mask"].cuda(), br.plan(name), c["NH"], scale=c["scale"])
    assert out.dtype == torch.bfloat16 and out.shape == (c["T"], c["NH"] * 64)
    out.backward(dout)
    torch.cuda.synchronize()
    br.check_case(name, dict(out=out.detach().cpu(), dqkv=x.grad.cpu()), label="bigbird-op")
    direct = _run(hip, name)
    assert torch.equal(_bits(out.detach().cpu()), _bits(direct["out"])) and torch.equal(_bits(x.grad.cpu()), _bits(direct["dqkv"]))
    assert len(br.plan(name)._device) == 1      # the lists were uploaded once, not per call


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_module_with_huggingface_state_dict(hip, mode):
    """Weights under HuggingFace's key names, built here; the float64 reference applied to the module's own bf16 projections;
    compared on the query rows whose own mask is 1, where the list semantics are HuggingFace's."""
    B, S, NH, H = 2, 384, 2, 128
    g = br.gen(31)
    sd = {}
    for n in ("query", "key", "value"):
        sd[n + ".weight"] = torch.randn(H, H, generator=g) * (1.5 / H ** 0.5)
        sd[n + ".bias"] = torch.randn(H, generator=g) * 0.1
    mod = bb.BigBirdBlockSparseSelfAttention(H, NH, num_random_blocks=3, layer_seed=3).cuda()
    mod.load_state_dict(sd)      # strict: the key names are HuggingFace's
    mod.train(mode == "train")
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1, 70:90] = 0
    mask[1, S - 100:] = 0
    x = torch.randn(B, S, H, generator=g).cuda().requires_grad_(True)
    out = mod(x, mask.cuda())
    assert out.shape == (B, S, H) and out.dtype == x.dtype
    plan = mod.plan_for(S // 64)
    ra_free = bool((plan.lists["key_mult"][:, 1:-1, 0] == 4).all())
    assert ra_free == (mode == "eval")          # eval: the zeros plan (block 0 four times); train: a drawn one
    assert mod.plan_for(S // 64) is plan          # fixed per module and mode
    qkv = mod.project(x).detach().cpu()
    c = dict(B=B, NH=NH, S=S, nb=S // 64, T=B * S, scale=0.125, mask=mask)
    zeros = torch.zeros(B * S, H, dtype=torch.bfloat16)
    refs = tuple(br.compute(c, plan.lists, qkv, zeros, m) for m in ("r64", "r32", "r16"))
    br.check(c, plan.lists, refs, dict(out=out.detach().reshape(B * S, H).to(torch.bfloat16).cpu()), name=f"module-{mode}",
             rows=mask.view(-1) != 0, keys=("out",))
    out.float().square().sum().backward()
    for p in list(mod.parameters()) + [x]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
