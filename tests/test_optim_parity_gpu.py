"""GPU: the optimizer boundary kernels (csrc/optim.hip) against float64, element by element, and bit for bit where the
answer is a bit pattern. Method and tolerances are tests/parity_util.py's: the kernel against the operation in float64 on the
CPU from the same fp32 inputs, A = max(8 e32, 2^-20 max |r|) from the same formula in torch float32 on the CPU, no element
left out, a PARITY line before every assert (run with -s; profiles/optimizer_parity.md is such a collection). The reference,
the cases and the layout are tests/optim_ref.py's; tests/test_optim_ref_cpu.py pins them without a GPU.

Denormals are not what the AdamW comparisons measure: every case keeps (1 - b2) g~^2 a normal fp32 number or exactly zero
(optim_ref.CASES). The conversions to bf16 ARE tested on denormals, ties, carries and overflow (the cast test below)."""
import functools
import struct

import pytest
import torch

from tests import optim_ref as orf
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENT = 7.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _guarded(rows, ld, dtype=BF16):
    """A [rows, ld] output between two guard rows, all of it sentinels: (whole buffer, view)."""
    buf = torch.full(((rows + 2) * ld,), SENT, device="cuda", dtype=dtype)
    return buf, buf[ld:ld + rows * ld].view(rows, ld)


def _guards_intact(buf, ld):
    return bool((buf[:ld] == SENT).all() and (buf[-ld:] == SENT).all())


def _i64(rows, width):
    return torch.tensor(rows, dtype=torch.int64, device="cuda").reshape(-1, width)


def _scalars(hip, kw, norm):
    return (kw["lr"], kw["b1"], kw["b2"], kw["eps"], kw["wd"], kw["bc1"], kw["bc2"], hip.ptr(norm), kw["max_norm"], kw["grad_scale"])


def _norm(kw):
    return None if kw["gnorm_sq"] is None else torch.tensor([kw["gnorm_sq"]], dtype=torch.float32, device="cuda")


def _run_flat(hip, p, g, m, v, kw, pieces=None):
    """stonk_adamw_step over the whole buffer, or over `pieces` (off, soff, n) with span_base = off and m / v packed."""
    n = p.numel()
    p, g = p.cuda(), g.cuda()
    pb = torch.full((n,), SENT, device="cuda", dtype=BF16)
    pieces = pieces or [(0, 0, n)]
    ms, vs = (torch.cat([x[off:off + k] for off, _, k in pieces]).cuda() for x in (m, v))
    norm, tab = _norm(kw), None if kw["decay_spans"] is None else _i64(kw["decay_spans"], 2)
    for off, soff, k in pieces:
        hip.call("stonk_adamw_step", p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, ms.data_ptr() + 4 * soff, vs.data_ptr() + 4 * soff,
                 pb.data_ptr() + 2 * off, k, *_scalars(hip, kw, norm), hip.ptr(tab), 0 if tab is None else tab.shape[0], off,
                 hip.stream_ptr())
    torch.cuda.synchronize()
    mo, vo = m.clone(), v.clone()
    for off, soff, k in pieces:
        mo[off:off + k], vo[off:off + k] = ms[soff:soff + k].cpu(), vs[soff:soff + k].cpu()
    return p.cpu(), mo, vo, g.cpu(), pb.cpu()


def _run_tiled(hip, index, p, g, m, v, kw, host=None):
    """stonk_adamw_step_tiled over `index` (tables built as Engine.adamw_tables builds them, or `host`). Returns the
    outputs and the W^T copies {name: (guarded buffer, [cols, ld_out] view)}."""
    n = p.numel()
    p, g, m, v = (x.cuda() for x in (p, g, m, v))
    pb = torch.full((n,), SENT, device="cuda", dtype=BF16)
    wts = {name: _guarded(index[name][1][1], (index[name][2][0] + 63) // 64 * 64) for name in orf.tiled(index)}
    tiles, n_tiles, spans, chunks = host or orf.host_tables(index, n, lambda name: wts[name][1].data_ptr())
    orf.check_tables(n, tiles, n_tiles, spans, chunks)
    desc = torch.frombuffer(bytearray(orf.pack_tiles(tiles)), dtype=torch.uint8).cuda()
    flat = _i64(spans, 3)
    norm, tab = _norm(kw), None if kw["decay_spans"] is None else _i64(kw["decay_spans"], 2)
    keep = _i64(kw["keep_grad"], 2) if kw.get("keep_grad") else None
    hip.call("stonk_adamw_step_tiled", hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(pb), n, *_scalars(hip, kw, norm),
             hip.ptr(tab), 0 if tab is None else tab.shape[0], hip.ptr(keep), 0 if keep is None else keep.shape[0],
             hip.ptr(desc), len(tiles), n_tiles, hip.ptr(flat), len(spans), chunks, hip.stream_ptr())
    torch.cuda.synchronize()
    return (p.cpu(), m.cpu(), v.cpu(), g.cpu(), pb.cpu()), wts


def _keep_spans(index):
    """Gradient spans the tiled step leaves in place: a tile tensor with its gap (as the trainer passes the decoders'), a
    piece in the middle of another, and a bias of the span kernel."""
    d, b, cb = index["d.weight"], index["b.weight"], index["c.bias"]
    return sorted([(d[0], d[0] + (d[3] + 255) // 256 * 256), (b[0] + 72 * 3, b[0] + 72 * 5), (cb[0], cb[0] + 64)])


@functools.lru_cache(maxsize=None)
def _refs(name, keep):
    """The references of a case, computed once and shared (never written to)."""
    index, numel = orf.layout()
    return orf.references(name, numel, orf.decay_spans(index), keep_grad=_keep_spans(index) if keep else None)


@pytest.mark.parametrize("name", list(orf.CASES))
def test_flat_adamw_against_float64(hip, name):
    (p, g, m, v, kw), r, r32 = _refs(name, False)
    got = _run_flat(hip, p, g, m, v, kw)
    orf.check_step(name, g, got, r, r32, "flat")


@pytest.mark.parametrize("name", list(orf.CASES))
def test_tiled_adamw_against_float64_with_mirror_and_wt_copies(hip, name):
    index, numel = orf.layout()
    (p, g, m, v, kw), r, r32 = _refs(name, True)
    got, wts = _run_tiled(hip, index, p, g, m, v, kw)
    orf.check_step(name, g, got, r, r32, "tiled")
    assert (r[3] != 0).any() and (r[3] == 0).any()    # some gradients survive, most do not
    # every W^T copy is the transposed mirror: zeros from the logical rows up to the tile edge, untouched past it
    for wname, (buf, wt) in wts.items():
        off, (rows, cols), (prows, _), _ = index[wname]
        r64, ld = (rows + 63) // 64 * 64, wt.shape[1]
        mirror = got[4][off:off + prows * cols].view(prows, cols)
        w = wt.cpu()
        assert torch.equal(_bits(w[:, :rows]), _bits(mirror[:rows].t())), wname
        assert (w[:, rows:r64] == 0).all() and (w[:, r64:] == SENT).all() and _guards_intact(buf, ld), wname


# ---- which elements are decayed and which gradients survive, exactly. p = 1, g = 0, m = v = 0 and lr * wd = 2^-7: p' is
# exactly 1 - 2^-7 on a decayed element and exactly 1 elsewhere; a gradient sentinel survives or becomes 0.
MASK_N = 12288
# [0, 4096) a 64x64 tile tensor | [4096, 5632) flat: ends in the MIDDLE of its second chunk of 1024 | [5632, 10240) a 64x72
# tile tensor | [10240, 12288) flat: ends at the last group of its second chunk
MASK_INDEX = {"t0.weight": (0, (64, 64), (64, 64), 4096), "f0.bias": (4096, (1536,), (1536,), 1536),
              "t1.weight": (5632, (64, 72), (64, 72), 4608), "f1.bias": (10240, (2048,), (2048,), 2048)}


def _table40(seed):
    """40 sorted spans over [0, MASK_N): every fifth adjacent to its predecessor, every seventh four elements long, the last
    one ending with the buffer."""
    gen, pos, spans = pu.gen(seed), 0, []
    for i in range(40):
        gap = 0 if i % 5 == 1 else 4 * int(torch.randint(1, 50, (1,), generator=gen))
        length = 4 if i % 7 == 0 else 4 * int(torch.randint(1, 80, (1,), generator=gen))
        spans.append((pos + gap, pos + gap + length))
        pos += gap + length
    assert pos < MASK_N - 8
    spans[-1] = (spans[-1][0], MASK_N)
    return spans


MASK_TABLES = {
    "one": [(4100, 5000)],                         # begins and ends inside a flat span
    "two": [(0, 4), (4, 4608)],                    # starts at 0, four elements, adjacent, crosses from the tile tensor into the span
    "one-group-at-the-end": [(MASK_N - 4, MASK_N)],
    "forty": _table40(1),
    "forty-b": _table40(2),
}


def _edge_elements(spans):
    """the element before the first span, first and last of each span, the one behind it, the last of the buffer"""
    e = {MASK_N - 1}
    for lo, hi in spans:
        e |= {lo - 1, lo, hi - 1, hi}
    return sorted(x for x in e if 0 <= x < MASK_N)


def _mask_kw(decay, keep=None, grad_scale=1.0):
    return dict(lr=2.0 ** -7, b1=orf.B1, b2=orf.B2, eps=orf.EPS, wd=1.0, bc1=1.0, bc2=1.0, gnorm_sq=None, max_norm=0.0,
                grad_scale=grad_scale, decay_spans=decay, keep_grad=keep)


def _assert_mask(what, got, want):
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, f"{what}: {len(bad)} elements wrong, first at {bad[:8]}"


@pytest.mark.parametrize("table", list(MASK_TABLES))
def test_flat_kernel_decays_exactly_the_elements_of_the_table(hip, table):
    spans = MASK_TABLES[table]
    orf.check_spans(spans, MASK_N)
    want = torch.where(orf.span_mask(MASK_N, spans), 1.0 - 2.0 ** -7, 1.0).float()
    one, zero = torch.ones(MASK_N), torch.zeros(MASK_N)
    p, m, v, g, pb = _run_flat(hip, one, zero, zero, zero, _mask_kw(spans))
    _assert_mask("p'", p, want)
    assert torch.equal(p[_edge_elements(spans)], want[_edge_elements(spans)])
    assert not m.any() and not v.any() and not g.any() and torch.equal(_bits(pb), _bits(want.to(BF16)))
    # the sharded form sees the same table through span_base: pieces that start inside and outside spans
    cuts = [0, 4, 4104, 4608, 4996, 5004, 8000, MASK_N - 4, MASK_N]
    pieces, acc = [], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        pieces.append((lo, acc, hi - lo))
        acc += hi - lo
    p2 = _run_flat(hip, one, zero, zero, zero, _mask_kw(spans), pieces=pieces)[0]
    _assert_mask("p' in pieces", p2, want)


@pytest.mark.parametrize("decay,keep", [("one", "two"), ("two", "forty"), ("forty", "forty-b"), ("forty-b", "one"),
                                        ("one-group-at-the-end", "one-group-at-the-end")])
def test_tiled_and_span_kernels_decay_and_keep_exactly_the_elements_of_the_tables(hip, decay, keep):
    dspans, kspans = MASK_TABLES[decay], MASK_TABLES[keep]
    want = torch.where(orf.span_mask(MASK_N, dspans), 1.0 - 2.0 ** -7, 1.0).float()
    kmask = orf.span_mask(MASK_N, kspans)
    one, zero = torch.ones(MASK_N), torch.zeros(MASK_N)
    # g = 0, as the case is stated; then a gradient of sentinels with grad_scale = 0 (g~ = 0 all the same), so that one run
    # shows both which parameters are decayed and which gradients survive
    for g_in, scale in ((zero, 1.0), (torch.full((MASK_N,), 3.0), 0.0)):
        (p, m, v, g, pb), wts = _run_tiled(hip, MASK_INDEX, one, g_in, zero, zero, _mask_kw(dspans, kspans, scale))
        _assert_mask("p'", p, want)
        _assert_mask("g'", g, torch.where(kmask, g_in, zero))
        for e in _edge_elements(dspans):
            assert p[e] == want[e], e
        for e in _edge_elements(kspans):
            assert g[e] == (g_in[e] if kmask[e] else 0.0), e
        assert not m.any() and not v.any() and torch.equal(_bits(pb), _bits(want.to(BF16)))
        for name, (buf, wt) in wts.items():
            off, (rows, cols), _, n = MASK_INDEX[name]
            assert torch.equal(_bits(wt.cpu()), _bits(want[off:off + n].view(rows, cols).t().to(BF16))) and _guards_intact(buf, 64)


# ---- the sharded form: stonk_adamw_step on pieces (off, soff, n) as FusedAdamW._pieces makes them
def _shard_pieces(index, numel):
    """Two ranks' pieces; the cuts lie inside decayed tensors, inside gaps, inside a bias and at a tensor's start."""
    a, ab, b, ln, d, tw = (index[k] for k in ("a.weight", "a.bias", "b.weight", "ln.LayerNorm.weight", "d.weight", "tiny.weight"))
    cuts = [0, 1000, ab[0] + 200, b[0] + 4444, ln[0] + 40, ln[0] + 100, d[0], d[0] + 12, d[0] + 39996, d[0] + d[3] + 64,
            tw[0] + 64, numel]
    assert cuts == sorted(set(cuts)) and all(c % 4 == 0 for c in cuts)
    assert ab[0] + ab[3] <= cuts[2] < b[0] and d[0] + d[3] < cuts[9] < tw[0]      # (two cuts inside alignment gaps)
    ranks = [[], []]
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        ranks[i % 2].append((lo, hi))
    out = []
    for spans in ranks:
        acc, pieces = 0, []
        for lo, hi in spans:
            pieces.append((lo, acc, hi - lo))
            acc += hi - lo
        out.append(pieces)
    return out


@pytest.mark.parametrize("name", ["long-step1-loose-gs0.125-wd10-table", "long-step3-below-gs0.5-table"])
def test_sharded_pieces_equal_the_unsharded_step_bit_for_bit(hip, name):
    index, numel = orf.layout()
    (p, g, m, v, kw), r, r32 = _refs(name, False)
    assert kw["decay_spans"] is not None and kw["wd"] > 0
    whole = _run_flat(hip, p, g, m, v, kw)
    pc, gc, mc, vc = p.clone(), g.clone(), m.clone(), v.clone()
    pb = torch.full((numel,), SENT, dtype=BF16)
    for pieces in _shard_pieces(index, numel):        # each rank from the step's inputs; its pieces' outputs are collected
        po, mo, vo, go, pbo = _run_flat(hip, p, g, m, v, kw, pieces=pieces)
        for off, _, k in pieces:
            for dst, src in ((pc, po), (gc, go), (mc, mo), (vc, vo), (pb, pbo)):
                dst[off:off + k] = src[off:off + k]
        rest = ~orf.span_mask(numel, [(off, off + k) for off, _, k in pieces])
        assert torch.equal(po[rest], p[rest]) and torch.equal(go[rest], g[rest]) and (pbo[rest] == SENT).all()
    for what, a, b in zip(("p", "m", "v", "g"), (pc, mc, vc, gc), whole):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, int((a != b).sum()))
    assert torch.equal(_bits(pb), _bits(whole[4]))
    orf.check_step(name, g, (pc, mc, vc, gc, pb), r, r32, "pieces")


# ---- the Python caller: FusedAdamW replicated (flat kernel) and sharded (pieces), over three steps
def test_fused_adamw_replicated_and_sharded_against_float64_step_by_step(hip):
    """Each step from the state the kernel itself left: p', m', v' against adamw_ref with the bias corrections of that step
    and the clip coefficient from the optimizer's own fp32 sum of squares; that sum against float64 within the bound of its
    addition order; two ranks' sharded optimizers, given the same norm, bit for bit the replicated one on their pieces."""
    from stonkgs_amd.params import FlatStore
    from stonkgs_amd.stonkgs_pretraining import FusedAdamW

    index, numel = orf.layout()
    lr, wd, u = 1e-3, 10.0, 2.0 ** -24
    p0 = pu.randn(numel, 71, 0.05)

    def make(spans=None):
        store = FlatStore(orf.SPECS, torch.device("cuda"), True)
        assert store.numel == numel and all(store.index[k][0] == index[k][0] for k in index)
        store.data.copy_(p0)
        return store, FusedAdamW(store, weight_decay=wd, max_grad_norm=1.0, spans=spans)

    store, opt = make()
    rank_pieces = _shard_pieces(index, numel)
    shards = [make([(off, off + k) for off, _, k in pieces]) for pieces in rank_pieces]
    assert [s[1]._pieces() for s in shards] == rank_pieces
    for step in (1, 2, 3):
        g = pu.randn(numel, 80 + step, 0.02 * step)
        p, m, v = store.data.cpu(), opt.m.cpu(), opt.v.cpu()
        for st, _ in [(store, opt)] + shards:
            st.grad.copy_(g)
        opt.step(lr)
        torch.cuda.synchronize()
        # the norm: one launch over the whole buffer
        exact = float((g.double() ** 2).sum())
        depth, bound = orf.sumsq_bound(numel)
        err = abs(float(opt.gnorm_sq) - exact) / exact
        print(f"PARITY fused-adamw step {step} sumsq G={depth} bound={bound:.3e} rel_err={err:.3e} used={err / bound:.3f}")
        assert err <= bound and opt.step_count == step
        kw = dict(lr=orf.f32(lr), b1=orf.B1, b2=orf.B2, eps=orf.EPS, wd=orf.f32(wd), bc1=orf.f32(1.0 - 0.9 ** step),
                  bc2=orf.f32(1.0 - 0.999 ** step), gnorm_sq=float(opt.gnorm_sq), max_norm=1.0, decay_spans=orf.decay_spans(index))
        r, r32 = (orf.adamw_ref(p, g, m, v, dtype=d, **kw) for d in (torch.float64, torch.float32))
        for k, (what, got) in enumerate((("p", store.data), ("m", opt.m), ("v", opt.v))):
            pu.check_f32(f"fused-adamw step {step} {what}'", got.cpu(), r[k], r32[k])
        pu.check_bf16(f"fused-adamw step {step} mirror", store.bf16.cpu(), r[0], r32[0])
        assert not store.grad.any() and torch.equal(_bits(store.bf16), _bits(store.data.to(BF16)))
        # sharded: the ranks' sums of squares add up to the whole (each piece a launch into one accumulator), and with
        # the replicated norm the pieces are the replicated step bit for bit
        total, worst = 0.0, 0.0
        for (st, so), pieces in zip(shards, rank_pieces):
            before = st.data.clone()
            so.step_count += 1
            so.accumulate_grad_norm_sq()
            torch.cuda.synchronize()
            mine = float(sum((g[off:off + k].double() ** 2).sum() for off, _, k in pieces))
            k_max = max(orf.sumsq_bound(k)[0] for _, _, k in pieces) + 24 + len(pieces)   # (+ one rounding per accumulation)
            worst = max(worst, k_max * u / (1 - k_max * u))
            assert abs(float(so.gnorm_sq) - mine) <= k_max * u / (1 - k_max * u) * mine
            total += float(so.gnorm_sq)
            so.gnorm_sq.copy_(opt.gnorm_sq)
            so.apply_update(lr)
            torch.cuda.synchronize()
            own = orf.span_mask(numel, [(off, off + k) for off, _, k in pieces]).cuda()
            assert torch.equal(st.data[own].view(torch.int32), store.data[own].view(torch.int32))
            assert torch.equal(st.bf16[own].view(torch.int16), store.bf16[own].view(torch.int16))
            assert torch.equal(st.data[~own], before[~own]) and not st.grad[own].any() and torch.equal(st.grad[~own], g.cuda()[~own])
            assert torch.equal(so.m.view(torch.int32), opt.m[own].view(torch.int32)) and torch.equal(so.v.view(torch.int32), opt.v[own].view(torch.int32))
            st.data.copy_(store.data)            # (the all-gather of the parameters)
        assert abs(total - exact) <= worst * exact       # (the ranks' sums added in float64 here: no further rounding)


# ---- the tables of a real model
def test_tables_of_a_real_model_keep_the_tiled_entrys_contract(hip):
    import math

    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    dims = dict(vocab_size=31000, kg_vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                intermediate_size=256, max_position_embeddings=256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    rows = torch.randn(300, 128, generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 0.3
    model = STonKGsForPreTraining(STonKGsConfig(**dims), kg_embeddings=rows)
    tr = Trainer(model, TrainingArguments(per_device_train_batch_size=4, weight_decay=0.01))
    store, eng = model._store, model.engine
    desc, n_desc, n_tiles, flat, n_flat, chunks = eng.adamw_tables()
    tiles = orf.unpack_tiles(bytes(desc.cpu().numpy().tobytes()))
    spans = [tuple(s) for s in flat.cpu().tolist()]
    assert len(tiles) == n_desc and len(spans) == n_flat
    ext = orf.check_tables(store.numel, tiles, n_tiles, spans, chunks)
    # the tile table: every 2-D weight a dgrad GEMM reads transposed, all its stored rows, its own W^T copy
    want = [name for name, (off, shape, pshape) in store.index.items()
            if len(shape) == 2 and shape[0] >= 64 and name.endswith(".weight")
            and not any(k in name for k in ("embeddings", "pooler", "seq_relationship"))]
    assert len(want) == 4 * 2 + 3
    for name, (off, wt, ld_out, r, prows, cols, _, _) in zip(want, tiles):
        o, shape, pshape = store.index[name]
        assert (off, r, prows, cols) == (o, shape[0], pshape[0], shape[1]), name
        assert wt == store.wt[name].data_ptr() and ld_out == store.wt[name].stride(0) and store.wt[name].shape[0] == cols, name
    assert len(tiles) == len(want)
    # every tensor lies wholly in one table; a tile entry holds exactly one tensor's stored rows
    for name, (off, _, pshape) in store.index.items():
        n = math.prod(pshape)
        kinds = [k for lo, hi, k in ext if lo <= off and off + n <= hi]
        assert kinds == (["tile"] if name in want else ["flat"]), (name, kinds)
    # the decay table: the stored extents of the .weight tensors without LayerNorm, sorted and disjoint
    dec = [tuple(s) for s in tr.optimizer._decay_table().cpu().tolist()]
    assert dec == sorted((off, off + math.prod(pshape)) for name, (off, _, pshape) in store.index.items()
                         if name.endswith(".weight") and "LayerNorm" not in name)
    orf.check_spans(dec, store.numel)
    # the gradients the step leaves in place: the two decoders' spans (their alignment gaps included), sorted
    keep = [tuple(s) for s in tr._keep_grad.cpu().tolist()]
    assert keep == sorted(store.span(n) for n in ("cls.predictions.entity_decoder.weight", "cls.predictions.text_decoder.weight"))
    orf.check_spans(keep, store.numel)


# ---- sum of squares
def _sumsq(hip, x, n, out=None, extra=None, n_extra=0):
    out = torch.zeros(1, device="cuda") if out is None else out
    ws = torch.zeros(int(hip.lib().stonk_sumsq_workspace_floats()), device="cuda")
    hip.call("stonk_sumsq_f32_plus", hip.ptr(x), n, hip.ptr(out), hip.ptr(ws), ws.numel(), hip.ptr(extra), n_extra, hip.stream_ptr())
    torch.cuda.synchronize()
    assert float(ws[-1]) == 0.0     # the ticket word is back at zero
    return out


SUMSQ_SIZES = [0, 1, 3, 4, 1023, 1024, 1027, 262147, 1050003]


def _small_ints(n, seed):
    return torch.randint(-2, 3, (max(n, 4),), generator=pu.gen(seed)).float()


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_of_small_integers_is_the_integer_sum(hip, n):
    """x in {-2 .. 2}: every square is at most 4 and every partial sum an integer of at most 4 n <= 4 200 012 < 2^24, so
    every addition in fp32 is exact whatever its order, and the result must EQUAL the integer sum."""
    x = _small_ints(n, n)
    want = int((x[:n].long() ** 2).sum())
    assert 4 * n < 2 ** 24 and want <= 4 * n and (n < 1000 or want > n)
    got = _sumsq(hip, x.cuda(), n)
    assert float(got) == float(want), (n, float(got), want)


@pytest.mark.parametrize("n", [262147, 1050003])
def test_sumsq_counts_one_planted_element_wherever_it_lies(hip, n):
    """A single 2 in a zero buffer: at the last element (block 0's scalar tail), at the last element of the vector part, and
    at index 4 * stride (the second load of thread 0; at 262 147 elements the first element behind the vector part)."""
    stride = 256 * orf.sumsq_grid(n)
    assert orf.sumsq_grid(n) == 256 and n % 4 == 3 and (n == 262147 or n > 12 * 256 * 256)
    for at in (n - 1, (n // 4) * 4 - 1, 4 * stride, 0):
        x = torch.zeros(n + 1, device="cuda")
        x[at] = 2.0
        x[n] = 64.0                     # (one past the end: never read)
        assert float(_sumsq(hip, x, n)) == 4.0, (n, at)


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1024, 1027, 70001, 262147, 1050003])
def test_sumsq_of_random_data_within_the_bound_of_its_own_addition_order(hip, n):
    """|got - r| <= gamma(G + 24) r: optim_ref.sumsq_bound derives it from the kernel's addition depth (all addends are
    non-negative, so the bound is relative). r is the float64 sum of the float64 squares."""
    x = pu.randn(max(n, 4), 300 + n % 97)
    r = float((x[:n].double() ** 2).sum())
    got = float(_sumsq(hip, x.cuda(), n))
    depth, bound = orf.sumsq_bound(n)
    err = abs(got - r) / r
    print(f"PARITY sumsq n={n} grid={orf.sumsq_grid(n)} G={depth} bound={bound:.3e} rel_err={err:.3e} used={err / bound:.3f}")
    assert err <= bound, (n, got, r, err, bound)


def test_sumsq_plus_over_pieces_and_extras_on_exact_data(hip):
    x = _small_ints(70003, 5).cuda()
    out = torch.zeros(1, device="cuda")
    cut = 1028                                                 # (a multiple of 4: the second piece is 16-byte aligned)
    _sumsq(hip, x, cut, out=out)
    extra = torch.randint(0, 50, (1500,), generator=pu.gen(6)).float().cuda()
    _sumsq(hip, x[cut:], 70003 - cut, out=out, extra=extra, n_extra=1500)
    want = int((x.cpu().long() ** 2).sum()) + int(extra.cpu().long().sum())
    assert want < 2 ** 24 and float(out) == float(want)
    # extras alone (n = 0: nothing of x is read), few and many
    for k in (1, 63, 64, 65, 1500):
        got = _sumsq(hip, x, 0, extra=extra, n_extra=k)
        assert float(got) == float(int(extra[:k].cpu().long().sum())), k
    assert float(_sumsq(hip, x, 0)) == 0.0


# ---- transposes and cast: exact by nature
def _transpose(hip, x, rows, cols, live=None, colsum=False):
    """stonk_transpose_bf16 of x[:rows] into a guarded [cols, roundup64(rows)] output; `live` = a device-side row count."""
    ld = (rows + 63) // 64 * 64
    buf, out = _guarded(cols, ld)
    cs = torch.zeros(cols + 8, device="cuda") if colsum else None
    cnt = None if live is None else torch.tensor([live], device="cuda", dtype=torch.int32)
    hip.call("stonk_transpose_bf16", hip.ptr(x), x.stride(0), hip.ptr(out), ld, rows, cols, hip.ptr(cs), hip.ptr(cnt), hip.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(buf, ld)
    return out.cpu(), None if cs is None else cs.cpu()


def _assert_transposed(out, x, live):
    """out[:, :live] = x[:live]^T, zeros up to the 64-row round-up of live, sentinels past it"""
    r64 = (live + 63) // 64 * 64
    assert torch.equal(_bits(out[:, :live]), _bits(x[:live].t().cpu()))
    assert (out[:, live:r64] == 0).all() and (_bits(out[:, live:r64]) == 0).all()
    assert (out[:, r64:] == SENT).all()


@pytest.mark.parametrize("live", [4131, 4097, 0, 4160 + 5])
def test_transpose_under_a_device_side_row_count(hip, live):
    """rows = 4160 = 65 row tiles on a grid bounded to 64: workgroups stride. 4131 and 4097 live rows need the 65th tile."""
    rows, cols = 4160, 128
    x = pu.randn((rows, cols), 21, dtype=BF16).cuda()
    out, _ = _transpose(hip, x, rows, cols, live=live)
    _assert_transposed(out, x, min(live, rows))


@pytest.mark.parametrize("cols", [72, 200])
@pytest.mark.parametrize("rows,live", [(130, None), (4160, 4131), (4160, 0)])
def test_transpose_column_sums(hip, rows, cols, live):
    x = pu.randn((rows, cols), 22 + cols, dtype=BF16)
    n = rows if live is None else live
    out, cs = _transpose(hip, x.cuda(), rows, cols, live=live, colsum=True)
    _assert_transposed(out, x, n)
    assert not cs[cols:].any()
    pu.check_f32(f"transpose colsum rows={rows} live={live} cols={cols}", cs[:cols], x[:n].double().sum(0), x[:n].float().sum(0))


@pytest.mark.parametrize("rows", [1, 63, 65])
@pytest.mark.parametrize("cols", [8, 72])
def test_transpose_f32_to_bf16(hip, rows, cols):
    w = pu.randn((rows, cols), 23 + rows, 0.02)
    ld = (rows + 63) // 64 * 64
    buf, out = _guarded(cols, ld)
    wd = w.cuda()
    hip.call("stonk_transpose_f32_to_bf16", hip.ptr(wd), hip.ptr(out), rows, cols, ld, hip.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(buf, ld)
    _assert_transposed(out.cpu(), w.to(BF16), rows)


def test_batched_transpose_of_short_and_narrow_entries(hip):
    shapes = [(30, 64), (130, 8), (64, 72), (65, 200)]
    srcs, outs, entries, first = [], [], [], 0
    for i, (rows, cols) in enumerate(shapes):
        x = pu.randn((rows, cols), 50 + i, dtype=BF16).cuda()
        ld = (rows + 63) // 64 * 64
        buf, out = _guarded(cols, ld)
        col_tiles = (cols + 63) // 64
        entries.append(struct.pack("<QQqqqiiii", hip.ptr(x), hip.ptr(out), cols, ld, rows, cols, first, col_tiles, 0))
        first += ((rows + 63) // 64) * col_tiles
        srcs.append(x)
        outs.append((buf, out))
    table = torch.frombuffer(bytearray(b"".join(entries)), dtype=torch.uint8).cuda()
    hip.call("stonk_transpose_bf16_batched", hip.ptr(table), len(shapes), first, hip.stream_ptr())
    torch.cuda.synchronize()
    for x, (buf, out), (rows, cols) in zip(srcs, outs, shapes):
        assert _guards_intact(buf, out.shape[1])
        _assert_transposed(out.cpu(), x, rows)


def _all_patterns():
    """Every high half of an fp32 word with the low halves that decide a rounding: exact, just below a tie, a tie, just
    above, all ones - ties to even both ways, the carry into the exponent, overflow to infinity, denormals, both zeros,
    infinities and NaNs."""
    hi = torch.arange(65536, dtype=torch.int64).repeat_interleave(5)
    lo = torch.tensor([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64).repeat(65536)
    word = (hi << 16) | lo
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)
    return word.view(torch.float32)


def _assert_same_bf16(got, x, what):
    """bits equal to torch's conversion wherever the input is no NaN; a NaN stays a NaN"""
    want = x.to(BF16)
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(got.float()), nan), what
    bad = ((_bits(got) != _bits(want)) & ~nan).nonzero().flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {x.numel()} patterns differ from round-to-nearest-even, first "
                              f"{[hex(int(x.view(torch.int32)[i]) & 0xFFFFFFFF) for i in bad[:6]]} -> "
                              f"{[hex(int(_bits(got)[i]) & 0xFFFF) for i in bad[:6]]}")


def test_the_three_bf16_conversions_round_every_pattern_as_torch_does(hip):
    x = _all_patterns()
    n, xd = x.numel(), x.cuda()
    # stonk_cast_f32_to_bf16 (n - 3 elements as well: the scalar tail)
    for k in (n, n - 3):
        y = torch.full((n + 8,), SENT, device="cuda", dtype=BF16)
        hip.call("stonk_cast_f32_to_bf16", hip.ptr(xd), hip.ptr(y), k, hip.stream_ptr())
        torch.cuda.synchronize()
        assert (y[k:] == SENT).all()
        _assert_same_bf16(y[:k].cpu(), x[:k], "cast")
    # the transpose's conversion: all of them as a [5120, 64] matrix
    buf, out = _guarded(64, 5120)
    hip.call("stonk_transpose_f32_to_bf16", hip.ptr(xd), hip.ptr(out), 5120, 64, 5120, hip.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(buf, 5120)
    _assert_same_bf16(out.cpu().t().contiguous().flatten(), x, "transpose f32 -> bf16")
    # the mirror of stonk_adamw_step with lr = 0, wd = 0 and nothing to add: p' = p, for every finite parameter
    p = x[torch.isfinite(x)]
    assert p.numel() % 4 == 0 and p.numel() == 5 * (65536 - 256)   # (256 high halves have an all-ones exponent)
    zero = torch.zeros_like(p)
    kw = dict(_mask_kw(None), lr=0.0, wd=0.0)
    p2, m, v, g, pb = _run_flat(hip, p, zero, zero, zero, kw)
    assert torch.equal(p2.view(torch.int32), p.view(torch.int32)) and not m.any() and not v.any()
    _assert_same_bf16(pb, p, "adamw mirror")
