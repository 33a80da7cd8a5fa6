"""GPU: stonk_adamw_step_tiled against what it replaces - stonk_adamw_step over the whole flat buffer followed by
stonk_transpose_bf16_batched - from identical inputs. Every output must be equal BIT FOR BIT: the fp32 parameters, both Adam
moments, the zeroed gradient, the bf16 mirror and every W^T copy."""
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

ALIGN = 256
H, I = 768, 3072
# the tensors of one encoder layer in the flat buffer's order, then a decoder-like tall matrix whose logical row count is
# not a multiple of 64 and whose slab carries pad rows (name, logical shape, rows stored in the flat buffer)
SPECS = [
    ("qkv.weight", (3 * H, H), 3 * H), ("qkv.bias", (3 * H,), None), ("attn_out.weight", (H, H), H), ("attn_out.bias", (H,), None),
    ("ln1.weight", (H,), None), ("ln1.bias", (H,), None), ("ffn_up.weight", (I, H), I), ("ffn_up.bias", (I,), None),
    ("ffn_down.weight", (H, I), H), ("ffn_down.bias", (H,), None), ("ln2.weight", (H,), None), ("ln2.bias", (H,), None),
    ("decoder.weight", (4131, H), 4224), ("odd.weight", (100, 72), 100), ("nsp.weight", (2, H), None), ("nsp.bias", (2,), None),
]


def _layout():
    index, off = {}, 0
    for name, shape, prows in SPECS:
        pshape = shape if prows is None else (prows,) + shape[1:]
        n = 1
        for d in pshape:
            n *= d
        index[name] = (off, shape, pshape, n)
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    return index, off


def _tables(hip, index, numel, bf16, wts):
    """(transpose table, entries, tiles), (tile table, entries, tiles, flat spans, entries, chunks)"""
    tr, first_tr, tiles, first, spans, chunks, pos = [], 0, [], 0, [], 0, 0
    for name, (off, shape, pshape, n) in index.items():
        if len(shape) != 2 or shape[0] < 64:
            continue
        rows, cols = shape
        prows = pshape[0]
        rpad = (prows + 63) // 64 * 64
        wt = wts[name]
        col_tiles = (cols + 63) // 64
        tr.append(struct.pack("<QQqqqiiii", bf16.data_ptr() + 2 * off, wt.data_ptr(), cols, rpad, rows, cols, first_tr, col_tiles, 0))
        first_tr += ((rows + 63) // 64) * col_tiles
        if off > pos:
            spans.append((pos, off, chunks))
            chunks += (off - pos + 1023) // 1024
        tiles.append(struct.pack("<qQqqqiiii", off, wt.data_ptr(), rpad, rows, prows, cols, first, col_tiles, 0))
        first += ((prows + 63) // 64) * col_tiles
        pos = off + prows * cols
    if pos < numel:
        spans.append((pos, numel, chunks))
        chunks += (numel - pos + 1023) // 1024
    dev = lambda e: torch.frombuffer(bytearray(b"".join(e)), dtype=torch.uint8).cuda()
    flat = torch.tensor(spans, dtype=torch.int64, device="cuda").reshape(-1, 3)
    return (dev(tr), len(tr), first_tr), (dev(tiles), len(tiles), first, flat, len(spans), chunks)


@pytest.mark.parametrize("clip,wd,keep", [(0.0, 0.0, False), (1.0, 0.0, False), (1.0, 0.01, False), (1.0, 0.01, True),
                                          (1e9, 0.0, True)])
def test_tiled_adamw_is_bitwise_the_flat_step_plus_the_batched_transpose(hip, clip, wd, keep):
    """clip = 0: no clipping; 1.0: active (the gradient norm is far above 1); 1e9: a norm is given but does not clip. wd with
    decay spans on the weights only. keep: the decoder's gradient span is not zeroed - then the REFERENCE gradient is the
    flat kernel's zeroed buffer with that span's input values put back."""
    index, numel = _layout()
    gen = torch.Generator(device="cuda").manual_seed(11)
    p0 = torch.randn(numel, device="cuda", generator=gen) * 0.05
    g0 = torch.randn(numel, device="cuda", generator=gen) * 0.02
    m0 = torch.randn(numel, device="cuda", generator=gen) * 0.01
    v0 = torch.rand(numel, device="cuda", generator=gen) * 1e-4
    nrm = (g0.double() ** 2).sum().float().reshape(1)
    decay = sorted((off, off + n) for name, (off, _, _, n) in index.items() if name.endswith(".weight") and "ln" not in name)
    dtab = torch.tensor(decay, dtype=torch.int64, device="cuda").reshape(-1, 2)
    doff, _, _, dn = index["decoder.weight"]
    ktab = torch.tensor([(doff, doff + dn)], dtype=torch.int64, device="cuda") if keep else None
    scal = (1e-3, 0.9, 0.999, 1e-8, wd, 1.0 - 0.9 ** 3, 1.0 - 0.999 ** 3, hip.ptr(nrm) if clip else 0, clip, 0.5)
    out = []
    for tiled in (False, True):
        p, g, m, v = p0.clone(), g0.clone(), m0.clone(), v0.clone()
        pb = torch.full((numel,), 3.0, device="cuda", dtype=torch.bfloat16)
        wts = {name: torch.full((shape[1], (pshape[0] + 63) // 64 * 64), 7.0, device="cuda", dtype=torch.bfloat16)
               for name, (_, shape, pshape, _) in index.items() if len(shape) == 2 and shape[0] >= 64}
        (tr, n_tr, tiles_tr), (td, n_td, tiles_td, flat, n_flat, chunks) = _tables(hip, index, numel, pb, wts)
        if tiled:
            hip.call("stonk_adamw_step_tiled", hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(pb), numel, *scal,
                     hip.ptr(dtab), dtab.shape[0], hip.ptr(ktab), 1 if keep else 0, hip.ptr(td), n_td, tiles_td, hip.ptr(flat),
                     n_flat, chunks, hip.stream_ptr())
        else:
            hip.call("stonk_adamw_step", hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(pb), numel, *scal,
                     hip.ptr(dtab), dtab.shape[0], 0, hip.stream_ptr())
            hip.call("stonk_transpose_bf16_batched", hip.ptr(tr), n_tr, tiles_tr, hip.stream_ptr())
            if keep:
                g[doff:doff + dn] = g0[doff:doff + dn]
        torch.cuda.synchronize()
        out.append((p, g, m, v, pb, wts))
    (p, g, m, v, pb, wts), (p2, g2, m2, v2, pb2, wts2) = out
    assert not torch.equal(p, p0) and float(g.abs().max()) == (float(g0[doff:doff + dn].abs().max()) if keep else 0.0)
    for name, a, b in (("p", p, p2), ("g", g, g2), ("m", m, m2), ("v", v, v2), ("bf16", pb, pb2)):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    for name in wts:
        assert torch.equal(wts[name], wts2[name]), name
    # and the W^T copies are what they claim: the transposed mirror, zeros past the logical rows up to the tile edge
    off, shape, pshape, _ = index["decoder.weight"]
    w = pb2[off:off + shape[0] * shape[1]].view(shape)
    r64 = (shape[0] + 63) // 64 * 64
    assert torch.equal(wts2["decoder.weight"][:, :shape[0]], w.t()) and (wts2["decoder.weight"][:, shape[0]:r64] == 0).all()
    assert (wts2["decoder.weight"][:, r64:] == 7.0).all()   # pad-row tiles past the copy's last tile leave it alone
