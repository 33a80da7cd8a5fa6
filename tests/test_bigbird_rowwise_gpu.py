"""The BigBird encoder's row-wise kernels on the GPU, per element against float64 (tests/parity_util.py: a bf16 output may be
off by one rounding, 2^-8 |r|, plus A = tol_a of the same operation in float32; an fp32 output by A):

  stonk_gelu_new_fwd_bf16 / _bwd_bf16   at 0, -0.0, denormals, +-{1e-3, 1, 3, 10, 1e4, 1e20, bf16-max} and normal draws; one
        comparison per MAGNITUDE group (A has a floor relative to the group's largest |r|: a group that held 1e20 would let
        anything pass at 1); n = 8, an n with a grid-stride tail, an n just beyond one trip of the launcher's grid cap
  stonk_embeds_ln_fwd                   H 128 / 768 / 1024; 1, 3 and 2 x 768 rows; ld_in > H; token types null and mixed; p = 0,
        and p = 0.1 under the EXACT mask oracle/dropout_oracle.py predicts
  stonk_embeds_ln_bwd_finish            the same shapes, and stonk_embed_grad on its bf16 output."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import dropout_oracle
from stonkgs_amd import _hip as hip
from tests import bigbird_encoder_ref as er
from tests.parity_util import check_bf16, check_f32, gen

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"


def _grid_cap():
    src = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "bigbird_rowwise.hip")).read()
    m = re.search(r"constexpr long GN_GRID_CAP = (\d+);", src)
    assert m and src.count("grid_cap(n8, 256, GN_GRID_CAP)") == 2, "the launcher's lines are not what this test reads"
    return int(m.group(1))


SPECIAL = [0.0, -0.0, 1e-40, -1e-40, 2.0 ** -130, -(2.0 ** -130)]
GROUPS = {"small": SPECIAL + [1e-3, -1e-3, 1.0, -1.0, 3.0, -3.0], "ten": [10.0, -10.0], "1e4": [1e4, -1e4],
          "1e20": [1e20, -1e20], "max": [er.BF16_MAX, -er.BF16_MAX]}


def _gelu_input(n, group, seed):
    """n bf16 values: the group's special values repeated through the array (first, last and around the middle included),
    normal draws of the group's scale elsewhere ("small": N(0, 2))."""
    vals = torch.tensor(GROUPS[group], dtype=torch.float32)
    if group == "small":
        u = torch.randn(n, generator=gen(seed)) * 2.0
        for start in (0, n // 2, n - len(vals)):
            if 0 <= start and start + len(vals) <= n:
                u[start:start + len(vals)] = vals
        if n < len(vals):
            u = vals[:n].clone()
    else:
        u = vals.repeat((n + len(vals) - 1) // len(vals))[:n].clone()
    return u.to(BF16)


def _gelu_refs(u_bf, dg_bf):
    """(r, r32) of the forward and of the backward: the closed forms of tests/bigbird_encoder_ref.py, which
    test_bigbird_encoder_ref_cpu.py pins to torch's own tanh GELU and its autograd in float64 (torch's float32 backward is
    NaN at 1e20: (1 - t^2) * inf)."""
    u64, u32 = u_bf.double(), u_bf.float()
    return er.gelu_new(u64), er.gelu_new(u32), dg_bf.double() * er.gelu_new_grad(u64), dg_bf.float() * er.gelu_new_grad(u32)


def _launch_gelu(u_bf, dg_bf):
    n = u_bf.numel()
    u, dg = u_bf.to(DEV), dg_bf.to(DEV)
    g = torch.full((n + 8,), 7.0, dtype=BF16, device=DEV)
    du = torch.full((n + 8,), 7.0, dtype=BF16, device=DEV)
    hip.call("stonk_gelu_new_fwd_bf16", u.data_ptr(), g.data_ptr(), n, hip.stream_ptr())
    hip.call("stonk_gelu_new_bwd_bf16", dg.data_ptr(), u.data_ptr(), du.data_ptr(), n, hip.stream_ptr())
    inplace = dg.clone()
    hip.call("stonk_gelu_new_bwd_bf16", inplace.data_ptr(), u.data_ptr(), inplace.data_ptr(), n, hip.stream_ptr())
    torch.cuda.synchronize()
    assert bool((g[n:] == 7.0).all()) and bool((du[n:] == 7.0).all()), "written past the end"
    assert torch.equal(inplace.view(torch.int16), du[:n].view(torch.int16)), "the in-place backward differs"
    return g[:n].cpu(), du[:n].cpu()


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("n", [8, 8 * (256 * 3 + 5)])
def test_gelu_new_per_element(group, n):
    u = _gelu_input(n, group, 5)
    dg = (torch.randn(n, generator=gen(6))).to(BF16)
    g, du = _launch_gelu(u, dg)
    r_g, g32, r_du, du32 = _gelu_refs(u, dg)
    assert bool(torch.isfinite(r_g).all()) and bool(torch.isfinite(r_du).all())
    assert bool(torch.isfinite(g.float()).all()) and bool(torch.isfinite(du.float()).all()), "NaN or inf for finite input"
    check_bf16(f"gelu_new.fwd.{group}.n{n}", g, r_g, g32)
    check_bf16(f"gelu_new.bwd.{group}.n{n}", du, r_du, du32)


def test_gelu_new_beyond_one_trip_of_the_grid_cap():
    """Every thread of the capped grid takes its first element, a few take a second: the stride and the tail."""
    n = _grid_cap() * 256 * 8 + 8 * 37
    u = _gelu_input(n, "small", 7)
    dg = torch.randn(n, generator=gen(8)).to(BF16)
    g, du = _launch_gelu(u, dg)
    r_g, g32, r_du, du32 = _gelu_refs(u, dg)
    assert bool(torch.isfinite(g.float()).all()) and bool(torch.isfinite(du.float()).all())
    check_bf16("gelu_new.fwd.cap", g, r_g, g32)
    check_bf16("gelu_new.bwd.cap", du, r_du, du32)


def test_gelu_new_is_not_the_erf_form():
    """At u = -3 the two forms differ by 10 % of the value, forty roundings: the bound tells them apart."""
    u = torch.full((8,), -3.0).to(BF16)
    g, _ = _launch_gelu(u, torch.ones(8).to(BF16))
    erf = torch.nn.functional.gelu(u.double())
    assert float((g.double() - er.gelu_new(u.double())).abs().max()) <= 2.0 ** -8 * float(er.gelu_new(u.double()).abs().max())
    assert float((g.double() - erf).abs().min()) > 20 * 2.0 ** -8 * float(erf.abs().max())


# ------------------------------------------------------------------ embeddings
def _embed_case(H, B, S, mixed_tt, seed):
    g = gen(seed)
    ld = H + 4
    x = torch.randn(B * S, ld, generator=g)
    pos = torch.randn(max(S, 4), H, generator=g) * 0.5
    typ = torch.randn(2, H, generator=g) * 0.5
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    tt = None
    if mixed_tt:
        tt = (torch.rand(B, S, generator=g) < 0.4).long()
    return x, ld, pos, typ, gamma, beta, tt


def _embed_ref(x, pos, typ, gamma, beta, tt, B, S, H, keep, p, dt):
    e = x[:, :H].to(dt).view(B, S, H) + typ.to(dt)[tt if tt is not None else torch.zeros(B, S, dtype=torch.long)]
    e = (e + pos.to(dt)[:S]).view(B * S, H)
    if keep is not None:
        scale = torch.tensor(1.0, dtype=dt) / (1.0 - torch.tensor(np.float32(p), dtype=dt))
        e = torch.where(keep, e * scale, torch.zeros_like(e))
    mean = e.mean(-1)
    var = ((e - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + 1e-12)
    y = (e - mean[:, None]) * rstd[:, None] * gamma.to(dt) + beta.to(dt)
    return e, y, mean, rstd


EMBED_CASES = [(H, B, S, mixed, p) for H in (128, 768, 1024)
               for B, S, mixed, p in ((1, 1, False, 0.0), (1, 3, True, 0.0), (2, 768, False, 0.0), (2, 768, True, 0.1))]


@pytest.mark.parametrize("H,B,S,mixed,p", EMBED_CASES)
def test_embeds_ln_fwd(H, B, S, mixed, p):
    seed = 77
    x, ld, pos, typ, gamma, beta, tt = _embed_case(H, B, S, mixed, 100 + H + S)
    T = B * S
    d = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    xd, posd, typd, gd, bd, ttd = d(x), d(pos), d(typ), d(gamma), d(beta), d(tt)
    so = torch.full((T + 2, H), 7.0, dtype=BF16, device=DEV)
    y = torch.full((T + 2, H), 7.0, dtype=BF16, device=DEV)
    mean, rstd = torch.zeros(T, device=DEV), torch.zeros(T, device=DEV)
    hip.call("stonk_embeds_ln_fwd", xd.data_ptr(), ld, hip.ptr(ttd), posd.data_ptr(), typd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
             so.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, S, H, 2, 1e-12, p, seed, hip.stream_ptr())
    torch.cuda.synchronize()
    assert bool((so[T:] == 7.0).all()) and bool((y[T:] == 7.0).all()), "written past the last row"
    keep = torch.from_numpy(dropout_oracle.keep(np.arange(T), np.arange(H), seed, p)) if p > 0 else None
    r = _embed_ref(x, pos, typ, gamma, beta, tt, B, S, H, keep, p, torch.float64)
    r32 = _embed_ref(x, pos, typ, gamma, beta, tt, B, S, H, keep, p, torch.float32)
    tag = f"embeds_ln.H{H}.{B}x{S}.p{p}"
    check_bf16(tag + ".sum_out", so[:T].cpu(), r[0], r32[0])
    check_bf16(tag + ".y", y[:T].cpu(), r[1], r32[1])
    check_f32(tag + ".mean", mean.cpu(), r[2], r32[2])
    check_f32(tag + ".rstd", rstd.cpu(), r[3], r32[3])
    if keep is not None:
        zero = so[:T].cpu().float() == 0
        assert torch.equal(zero, ~keep), "the dropped elements are not the oracle's"
        share = float(zero.double().mean())
        assert abs(share - p) < 5 * (p * (1 - p) / zero.numel()) ** 0.5, share
        print(f"PARITY {tag}.zeros share={share:.5f}")


@pytest.mark.parametrize("H,B,S,mixed,p", EMBED_CASES)
def test_embeds_ln_bwd_finish_and_embed_grad(H, B, S, mixed, p):
    seed = 78
    T = B * S
    g = gen(200 + H + S)
    ld, ld_out = H + 8, H + 4
    dsum = torch.randn(T, ld, generator=g).to(BF16)
    tt = (torch.rand(B, S, generator=g) < 0.4).long() if mixed else None
    dsd = dsum.to(DEV)
    d_in = torch.full((T + 1, ld_out), 7.0, device=DEV)
    dxm = torch.full((T + 1, H), 7.0, dtype=BF16, device=DEV)
    hip.call("stonk_embeds_ln_bwd_finish", dsd.data_ptr(), ld, d_in.data_ptr(), ld_out, dxm.data_ptr(), T, H, p, seed,
             hip.stream_ptr())
    dpos, dtyp = torch.zeros(S, H, device=DEV), torch.zeros(2, H, device=DEV)
    ttd = None if tt is None else tt.to(DEV)
    hip.call("stonk_embed_grad", dxm.data_ptr(), hip.ptr(ttd), dpos.data_ptr(), dtyp.data_ptr(), B, S, H, 2, 0, hip.stream_ptr())
    torch.cuda.synchronize()
    assert bool((d_in[T:] == 7.0).all()) and bool((d_in[:T, H:] == 7.0).all()) and bool((dxm[T:] == 7.0).all())
    keep = torch.from_numpy(dropout_oracle.keep(np.arange(T), np.arange(H), seed, p)) if p > 0 else torch.ones(T, H, dtype=torch.bool)

    def ref(dt):
        scale = torch.tensor(1.0, dtype=dt) / (1.0 - torch.tensor(np.float32(p), dtype=dt))
        v = dsum[:, :H].to(dt)
        return torch.where(keep, v * scale if p > 0 else v, torch.zeros_like(v))

    tag = f"embeds_bwd_finish.H{H}.{B}x{S}.p{p}"
    check_f32(tag + ".d_inputs_embeds", d_in[:T, :H].cpu().contiguous(), ref(torch.float64), ref(torch.float32))
    check_bf16(tag + ".dx_masked", dxm[:T].cpu(), ref(torch.float64), ref(torch.float32))
    if p > 0:
        assert torch.equal(dxm[:T].cpu().float() == 0, ~keep | (dsum[:, :H].float() == 0))
    # stonk_embed_grad on that output: position and token-type sums of the bf16 rows the kernel wrote
    got = dxm[:T].cpu()
    types = torch.zeros(B, S, dtype=torch.long) if tt is None else tt

    def sums(dt):
        v = got.to(dt).view(B, S, H)
        t = torch.stack([(v * (types == k).to(dt)[:, :, None]).sum((0, 1)) for k in (0, 1)])
        return v.sum(0), t

    check_f32(tag + ".dpos", dpos.cpu(), sums(torch.float64)[0], sums(torch.float32)[0])
    check_f32(tag + ".dtype", dtyp.cpu(), sums(torch.float64)[1], sums(torch.float32)[1])
