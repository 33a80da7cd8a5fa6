"""Reference of the optimizer kernels (csrc/optim.hip) for tests/test_optim_parity_gpu.py, its cases, and the layout the
flat and the tiled AdamW kernels are run over. tests/test_optim_ref_cpu.py pins all of it without a GPU.

adamw_ref is what include/stonk_hip.h and adamw_consts promise, element by element, in float64 (the reference r) or in
float32 with one rounding per operation (r32, which gives the tolerance its e32: tests/parity_util.py):

    coef  = grad_scale * min(1, max_norm / (sqrt(gnorm_sq) * grad_scale + 1e-6))     (clip_grad_norm_; 1 without a norm)
    keep  = 1 - lr * wd   on decayed elements (everywhere without a table), 1 elsewhere
    g~    = g * coef
    m'    = b1 m + (1 - b1) g~
    v'    = b2 v + (1 - b2) g~ g~
    p'    = p keep - (lr / bc1) * m' / (sqrt(v') / sqrt(bc2) + eps)
    g'    = 0, except inside keep_grad spans, where it stays

WHICH AdamW this is. The kernel computes sqrt(v') * rsqrt(bc2) + eps, torch.optim.AdamW computes
(sqrt(v') / sqrt(bc2)) + eps (its `denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)`), and both decay BEFORE the
Adam update (p *= 1 - lr wd, then p -= ...). The two differ in rounding only: eps is added AFTER the division by sqrt(bc2)
in both. The two look-alikes that differ in meaning - eps added before the division ((sqrt(v') + eps) / sqrt(bc2), what the
original Adam paper's "epsilon hat" form amounts to), and decay applied to the updated parameter - are the `variant`s
below; test_optim_ref_cpu.py shows that the checks refuse both.

Every scalar a case hands to the kernel is a float32 value already (f32()), because the C entry takes floats: the
reference reads the same number the kernel reads. That holds for gnorm_sq too: the clip coefficient comes from the GIVEN
fp32 sum of squares, so the norm kernel's own error stays out of the AdamW comparison.
"""
import math
import struct

import numpy as np
import torch

from tests import parity_util as pu

BF16 = torch.bfloat16


def f32(x):
    """The float32 nearest to x, as a Python float: what a c_float argument carries."""
    return float(np.float32(x))


def span_mask(n, spans, base=0):
    """bool[n]: element base + i lies in one of the [lo, hi) spans. None = everywhere."""
    mask = torch.zeros(n, dtype=torch.bool)
    if spans is None:
        return ~mask
    for lo, hi in spans:
        lo, hi = max(lo - base, 0), min(hi - base, n)
        if hi > lo:
            mask[lo:hi] = True
    return mask


def adamw_ref(p, g, m, v, *, lr, b1, b2, eps, wd, bc1, bc2, gnorm_sq=None, max_norm=0.0, grad_scale=1.0, decay_spans=None,
              span_base=0, keep_grad=None, dtype=torch.float64, variant=None):
    """(p', m', v', g', bf16(p')) of one step over flat CPU tensors. `gnorm_sq`: None (no norm pointer) or the fp32 value
    the kernel reads. `decay_spans`: None = decay everywhere, else sorted [lo, hi) spans of the flat buffer, of which this
    call's element i is element span_base + i. `variant` (None | "decay_after" | "eps_first"): deliberately wrong forms."""
    t = lambda x: torch.tensor(x, dtype=dtype)
    p, g, m, v = (x.detach().cpu().to(dtype) for x in (p, g, m, v))
    coef = t(grad_scale)
    if gnorm_sq is not None and max_norm > 0:
        total = torch.sqrt(t(gnorm_sq)) * t(grad_scale)
        cc = t(max_norm) / (total + t(1e-6))
        coef = coef * torch.clamp(cc, max=1.0)
    step = t(lr) / t(bc1)
    keep = torch.where(span_mask(p.numel(), decay_spans if wd != 0 else None, span_base), t(1.0) - t(lr) * t(wd), t(1.0))
    gr = g * coef
    m2 = t(b1) * m + (t(1.0) - t(b1)) * gr
    v2 = t(b2) * v + (t(1.0) - t(b2)) * gr * gr
    if variant == "eps_first":
        denom = (torch.sqrt(v2) + t(eps)) / torch.sqrt(t(bc2))
    else:
        denom = torch.sqrt(v2) / torch.sqrt(t(bc2)) + t(eps)
    if variant == "decay_after":
        p2 = (p - step * (m2 / denom)) * keep
    else:
        p2 = p * keep - step * (m2 / denom)
    g2 = torch.where(span_mask(p.numel(), keep_grad or [], span_base), g, torch.zeros_like(g))
    return p2, m2, v2, g2, p2.to(torch.float32).to(BF16)


# ---- the layout: a few 2-D weights, biases and the alignment gaps between them, in the flat buffer's order (tensors start
# at multiples of 256 elements, as params.FlatStore lays them out). (name, logical shape, rows held in the flat buffer)
ALIGN = 256
SPECS = [
    ("a.weight", (130, 64), 256),      # rows < prows, rows % 64 != 0: every stored row is updated, rows 130..191 reach W^T
                                       # as zeros and the row tile 192..255 does not touch it
    ("a.bias", (130,), None),
    ("b.weight", (128, 72), 128),      # cols % 64 != 0
    ("ln.LayerNorm.weight", (72,), None),
    ("ln.LayerNorm.bias", (72,), None),
    ("c.weight", (64, 128), 64),
    ("c.bias", (64,), None),
    ("d.weight", (200, 200), 200),     # neither a multiple of 64
    ("tiny.weight", (2, 64), None),    # fewer than 64 rows: no W^T copy, the span kernel's - but decayed
    ("tiny.bias", (2,), None),
]


def layout():
    """name -> (offset, shape, stored shape, stored elements), and the buffer's length."""
    index, off = {}, 0
    for name, shape, prows in SPECS:
        pshape = shape if prows is None else (prows,) + shape[1:]
        n = math.prod(pshape)
        index[name] = (off, shape, pshape, n)
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    return index, off


def tiled(index):
    return [name for name, (_, shape, _, _) in index.items() if len(shape) == 2 and shape[0] >= 64]


def decay_spans(index):
    """HF's grouping as FusedAdamW._decay_table makes it: the stored extent of every .weight that is no LayerNorm's."""
    return sorted((off, off + n) for name, (off, _, _, n) in index.items() if name.endswith(".weight") and "LayerNorm" not in name)


def host_tables(index, numel, wt_ptr):
    """Host form of the tables of stonk_adamw_step_tiled, built the way Engine.adamw_tables builds them: (tile entries as
    tuples (off, wt, ld_out, rows, prows, cols, first_tile, col_tiles), tiles, flat spans (lo, hi, first_chunk), chunks)."""
    tiles, first, spans, chunks, pos = [], 0, [], 0, 0
    for name in tiled(index):
        off, (rows, cols), pshape, _ = index[name]
        prows = pshape[0]
        if off > pos:
            spans.append((pos, off, chunks))
            chunks += (off - pos + 1023) // 1024
        col_tiles = (cols + 63) // 64
        tiles.append((off, wt_ptr(name), (prows + 63) // 64 * 64, rows, prows, cols, first, col_tiles))
        first += ((prows + 63) // 64) * col_tiles
        pos = off + prows * cols
    if pos < numel:
        spans.append((pos, numel, chunks))
        chunks += (numel - pos + 1023) // 1024
    return tiles, first, spans, chunks


TILE_FMT = "<qQqqqiiii"   # AdamwTileDesc: off, wt, ld_out, rows, prows, cols, first_tile, col_tiles, pad (56 bytes)


def pack_tiles(tiles):
    return b"".join(struct.pack(TILE_FMT, *e, 0) for e in tiles)


def unpack_tiles(raw):
    return [struct.unpack_from(TILE_FMT, raw, i)[:8] for i in range(0, len(raw), struct.calcsize(TILE_FMT))]


def check_tables(numel, tiles, n_tiles, spans, n_chunks):
    """The contract stonk_adamw_step_tiled leaves to its caller, in integers: the tile entries and the flat spans cover
    [0, numel) exactly once, first_tile / first_chunk and the totals are consistent, and every alignment the header lists
    holds. Returns the sorted extents [(lo, hi, "tile" | "flat")]."""
    assert numel % 4 == 0
    ext, first = [], 0
    for off, wt, ld_out, rows, prows, cols, first_tile, col_tiles in tiles:
        assert first_tile == first and col_tiles == (cols + 63) // 64, (off, first_tile, first)
        assert 0 < rows <= prows and cols > 0 and cols % 8 == 0 and off % 4 == 0 and (prows * cols) % 4 == 0, off
        assert wt % 16 == 0 and ld_out % 8 == 0 and ld_out >= (rows + 63) // 64 * 64, off
        first += ((prows + 63) // 64) * col_tiles
        ext.append((off, off + prows * cols, "tile"))
    assert first == n_tiles
    chunk = 0
    for lo, hi, first_chunk in spans:
        assert first_chunk == chunk and 0 <= lo < hi and lo % 4 == 0 and hi % 4 == 0, (lo, hi, first_chunk)
        chunk += (hi - lo + 1023) // 1024
        ext.append((lo, hi, "flat"))
    assert chunk == n_chunks
    assert [e[0] for e in tiles] == sorted(e[0] for e in tiles) and [s[0] for s in spans] == sorted(s[0] for s in spans)
    ext.sort()
    pos = 0
    for lo, hi, _ in ext:
        assert lo == pos, f"[{pos}, {lo}) is " + ("covered twice" if lo < pos else "in neither table: it would not train")
        pos = hi
    assert pos == numel, (pos, numel)
    return ext


def check_spans(spans, numel):
    """sorted, disjoint, non-empty, inside [0, numel), multiples of 4 (a group of four elements shares the answer)"""
    pos = 0
    for lo, hi in spans:
        assert pos <= lo < hi <= numel and lo % 4 == 0 and hi % 4 == 0, (lo, hi, pos)
        pos = hi


# ---- cases of the per-element comparison. Each key is there for a reason (test_optim_ref_cpu.py checks the coverage):
#   p:     "normal" ~ 0.05 | "zero": the output is then the update itself, its relative error not hidden under |p|
#   state: "zero" (first step) | "long": m ~ 1e-2, v ~ 1e-4, what a long run leaves | "mixed": long, with a third of the
#          elements at m = v = 0 and another third at g = 0 beside non-zero state
#   step:  bias corrections of step 1, 3 and 100 000 (where bc1 = 1 - 0.9^step rounds to 1 in fp32)
#   clip:  "off" (max_norm = 0, no norm pointer) | "active" (norm about 30) | "loose" (a norm is given, max_norm = 1e9) |
#          "below" / "above": the scaled norm within 1e-6 of max_norm = 1 on either side
#   g:     "normal" | "wide": |g| log-uniform in [1e-15, 1e4]. g^2 (1 - b2) coef^2 stays a NORMAL fp32 number (above
#          1e-15^2 * 1e-3 / 30^2 = 1.1e-36, coef >= 1 / 30 in every wide case) or is exactly zero (g = 0), so that denormal handling is not what the test measures
B1, B2, EPS, LR = f32(0.9), f32(0.999), f32(1e-8), f32(1e-3)


def _case(p="normal", state="long", step=3, clip="off", gs=1.0, wd=0.0, table=False, g="normal", seed=0):
    return dict(p=p, state=state, step=step, clip=clip, gs=gs, wd=wd, table=table, g=g, seed=seed)


CASES = {
    "first-step": _case(state="zero", step=1, seed=1),
    "p0-first-step-clip": _case(p="zero", state="zero", step=1, clip="active", seed=2),
    "p0-long-step3-loose-gs0.5-wd": _case(p="zero", step=3, clip="loose", gs=0.5, wd=0.01, seed=3),
    "p0-long-step100000": _case(p="zero", step=100000, seed=4),
    "long-step100000-clip-gs0.125-table": _case(step=100000, clip="active", gs=0.125, wd=0.01, table=True, seed=5),
    "long-step3-clip-table": _case(clip="active", wd=0.01, table=True, seed=6),
    "long-step3-below-gs0.5-table": _case(clip="below", gs=0.5, wd=0.01, table=True, seed=7),
    "long-step3-above-gs0.125": _case(clip="above", gs=0.125, seed=8),
    "long-step1-below": _case(step=1, clip="below", seed=9),
    "long-step1-above-gs0.5": _case(step=1, clip="above", gs=0.5, seed=10),
    "long-step1-loose-gs0.125-wd10-table": _case(step=1, clip="loose", gs=0.125, wd=10.0, table=True, seed=11),
    "wide-mixed-wd10-table": _case(state="mixed", g="wide", wd=10.0, table=True, seed=12),
    "p0-wide-mixed-clip-gs0.5-wd": _case(p="zero", state="mixed", g="wide", clip="active", gs=0.5, wd=0.01, seed=13),
    "long-step100000-wd10-table": _case(step=100000, wd=10.0, table=True, seed=14),
}


def inputs(name, numel):
    """Seeded CPU inputs of a case: p, g, m, v (fp32) and the keyword arguments of adamw_ref / the kernel's scalars."""
    c = CASES[name]
    s = c["seed"] * 10
    p = torch.zeros(numel) if c["p"] == "zero" else pu.randn(numel, s + 1, 0.05)
    if c["g"] == "wide":
        gen = pu.gen(s + 2)
        mag = 10.0 ** (torch.rand(numel, generator=gen, dtype=torch.float64) * 19 - 15)
        sign = torch.where(torch.rand(numel, generator=gen) < 0.5, -1.0, 1.0)
        g = (mag * sign).to(torch.float32)
    else:
        g = pu.randn(numel, s + 2, 30.0 / math.sqrt(numel) if c["clip"] == "active" else 0.02)
    if c["state"] == "zero":
        m, v = torch.zeros(numel), torch.zeros(numel)
    else:
        m, v = pu.randn(numel, s + 3, 0.01), torch.rand(numel, generator=pu.gen(s + 4)) * 1e-4
        if c["state"] == "mixed":
            third = torch.arange(numel) % 3
            m, v = torch.where(third == 0, 0.0, m), torch.where(third == 0, 0.0, v)
            g = torch.where(third == 1, 0.0, g)
    gs = c["gs"]
    kw = dict(lr=LR, b1=B1, b2=B2, eps=EPS, wd=f32(c["wd"]), bc1=f32(1.0 - 0.9 ** c["step"]), bc2=f32(1.0 - 0.999 ** c["step"]),
              gnorm_sq=None, max_norm=0.0, grad_scale=gs)
    if c["clip"] in ("active", "loose"):
        # (a wide gradient's own norm is 3e5 and would scale its smallest elements' squares into the denormals: the norm
        # GIVEN to the kernel is 30 there - the kernel and the reference read the given value, whatever the gradient's is)
        nsq = 900.0 if c["g"] == "wide" else float((g.double() ** 2).sum())
        kw.update(gnorm_sq=f32(nsq), max_norm=1.0 if c["clip"] == "active" else f32(1e9))
    elif c["clip"] in ("below", "above"):   # sqrt(gnorm_sq) * gs = 1 -+ 5e-7: the clip factor 1 / (1 + 5e-7) or exactly 1
        kw.update(gnorm_sq=f32(((1.0 + (-5e-7 if c["clip"] == "below" else 5e-7)) / gs) ** 2), max_norm=1.0)
    return p, g, m, v, kw


def bands(name, g):
    """Element sets a case is compared in. A wide-gradient case is cut by the decade of |g| (A then comes from the band's own
    reference values, and a small element is not measured against the largest one's ulp); together they are every element."""
    if CASES[name]["g"] != "wide":
        return [("", torch.ones_like(g, dtype=torch.bool))]
    a = g.abs()
    edges = [0.0, 1e-10, 1e-5, 1.0, float("inf")]
    out = [(f"|g| in [{lo:g}, {hi:g})", (a >= lo) & (a < hi)) for lo, hi in zip(edges[:-1], edges[1:])]
    assert int(sum(mask.sum() for _, mask in out)) == g.numel()
    return out


def references(name, numel, spans, **extra):
    """(inputs, r, r32) of a case: adamw_ref in float64 and in float32 from the same inputs."""
    p, g, m, v, kw = inputs(name, numel)
    kw = dict(kw, decay_spans=spans if CASES[name]["table"] else None, **extra)
    return (p, g, m, v, kw), adamw_ref(p, g, m, v, dtype=torch.float64, **kw), adamw_ref(p, g, m, v, dtype=torch.float32, **kw)


def check_step(name, g_in, got, r, r32, kernel="r32"):
    """A kernel's (p', m', v', g', mirror) against the references: p', m', v' with check_f32 and the mirror with check_bf16
    in every band, the gradient and mirror == bf16(own p') exactly."""
    for label, mask in bands(name, g_in):
        tag = f"[{kernel}] {name} {label}".strip()
        for k, what in enumerate(("p", "m", "v")):
            pu.check_f32(f"adamw {tag} {what}'", got[k].cpu()[mask], r[k][mask], r32[k][mask])
        pu.check_bf16(f"adamw {tag} mirror", got[4].cpu()[mask], r[0][mask], r32[0][mask])
    assert torch.equal(got[3].cpu(), r[3].to(torch.float32)), f"{name}: gradient after the step"
    assert torch.equal(got[4].cpu().view(torch.int16), got[0].cpu().to(BF16).view(torch.int16)), f"{name}: mirror != bf16(p')"


# ---- sum of squares
SUMSQ_SLOTS = 256


def sumsq_grid(n):
    return min(max((n // 4 + 255) // 256, 1), SUMSQ_SLOTS)


def sumsq_bound(n):
    """Relative error bound of sumsq_kernel over n non-negative addends x^2, from its addition order (optim.hip).
    Every addend is non-negative, so the computed sum is within gamma_k = k u / (1 - k u) of the exact one, u = 2^-24, where
    k is the largest number of roundings any one addend passes through on its way to the result:
        1       the product x * x (an FMA rounds less often, never more)
        3       the sum of the four squares of one 16-byte load
        G       acc += ... once per load of the thread, G = ceil(n / (1024 * grid)) loads at the most (the four-load loop and
                the single loop are the same chain: one addition per load)
        1       the scalar tail in block 0 (n % 4 <= 3 elements: one more addition for three threads)
        6 + 3   wave_sum's butterfly over 64 lanes, then part[0] + part[1] + part[2] + part[3]
        1       the last block's sum over the slots (grid <= 256 slots: one per thread)
        6 + 2   wave_sum again, then (part[0] + part[1]) + (part[2] + part[3])
        1       atomicAdd into the accumulator
    k = G + 24. (The issue proposed 4 G + 24: that counts four roundings per load on the chain, but the three additions inside a
    load are off the chain - an addend meets them once, whichever load it came with. The derived constant is the smaller one
    and is the one used.)"""
    g = -(-n // (1024 * sumsq_grid(n))) if n else 0
    k = g + 24
    u = 2.0 ** -24
    return g, k * u / (1 - k * u)
