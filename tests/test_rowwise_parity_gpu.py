"""fp64 parity of the row-wise kernels of csrc/norm.hip on the paths the step tests do not reach: several rows per wave
in the generic LayerNorm kernels, the wide-H instantiations (CPL = 4, 8), rstd, the three dgamma / dbeta routes, exact
dropout masks from oracle/dropout_oracle.py, the packed layout and null pointers of the embedding front-end, the batch loop
and the row map of the embedding gradient. Tolerances: tests/parity_util.py."""
import numpy as np
import pytest
import torch

from oracle import dropout_oracle as do
from tests.parity_util import check_bf16, check_f32, gen as _gen, leaf as _leaf, randn as _randn

pytestmark = pytest.mark.gpu

EPS = 1e-12
BF = torch.bfloat16




def _keep(rows, H, seed, p):
    return torch.from_numpy(do.keep(np.asarray(rows), np.arange(H), seed, p))


def _p32(p):
    return float(np.float32(p))   # the launchers take the probability as a C float


class _LnCase:
    """Inputs of one LayerNorm shape and the reference forward / backward in a given precision."""

    def __init__(self, rows, H):
        self.rows, self.H = rows, H
        self.x = _randn((rows, H), 1, 2.0, 0.5, BF)
        self.dy = _randn((rows, H), 2, 1.0, 0.0, BF)
        self.gamma = _randn((H,), 3, 0.5, 1.0)
        self.beta = _randn((H,), 4, 0.1)

    def ref(self, dtype, dy_mask=None, dy_scale=1.0):
        x, g, b = _leaf(self.x, dtype), _leaf(self.gamma, dtype), _leaf(self.beta, dtype)
        y, mean, rstd = torch.native_layer_norm(x, (self.H,), g, b, EPS)
        dy = self.dy.to(dtype)
        if dy_mask is not None:
            dy = torch.where(dy_mask, dy * dy_scale, torch.zeros((), dtype=dtype))
        y.backward(dy)
        return dict(y=y.detach(), mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1), dx=x.grad, dgamma=g.grad,
                    dbeta=b.grad)


def _ln_fwd(hip, c, x, gamma, beta, stats=True, flags=0, p=0.0, seed=0):
    y = torch.full_like(x, 7.0)
    mean = torch.full((c.rows,), -3.0, device="cuda") if stats else None
    rstd = torch.full((c.rows,), -3.0, device="cuda") if stats else None
    hip.call("stonk_layernorm_fwd", hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd),
             c.rows, c.H, EPS, flags, p, seed, hip.stream_ptr())
    return y, mean, rstd


def _ln_bwd(hip, c, dy, x, mean, rstd, gamma, dg, db, ws, flags=0, p_in=0.0, seed_in=0, p_out=0.0, seed_out=0, drop=False):
    dx = torch.full_like(x, 7.0)
    dxd = torch.full_like(x, 7.0) if drop else None
    hip.call("stonk_layernorm_bwd", hip.ptr(dy), hip.ptr(x), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma), hip.ptr(dx),
             hip.ptr(dxd), hip.ptr(dg), hip.ptr(db), c.rows, c.H, flags, p_in, seed_in, p_out, seed_out, hip.ptr(ws),
             0 if ws is None else ws.numel(), hip.stream_ptr())
    return dx, dxd


LN_SHAPES = [(1, 8), (3, 72), (8200, 72), (5, 520), (4100, 640), (7, 1032), (5, 1536), (4, 2048), (5, 2056), (6, 4096),
             (4100, 768), (2, 512), (1, 1024)]


@pytest.mark.parametrize("rows,H", LN_SHAPES)
def test_layernorm_fwd_bwd_fp64(hip, rows, H):
    """Several rows per wave. The backward grids stop at 1024 workgroups of four waves: (4100, 640) gives the generic backward
    a second row in every wave, (8200, 72) a third in 8 of them, (4100, 768) the lane backward a second. The forward grids
    stop at 2048 (generic) and 1024 (lane): the generic forward gets its second row only at (8200, 72), in 8 waves, the lane
    forward at (4100, 768). H > 1024: CPL = 4 and 8, with 8 H floats of LDS in the backward."""
    c = _LnCase(rows, H)
    r64, r32 = c.ref(torch.float64), c.ref(torch.float32)
    tag = f"ln[{rows}x{H}]"
    x, dy, gamma, beta = c.x.cuda(), c.dy.cuda(), c.gamma.cuda(), c.beta.cuda()
    y, mean, rstd = _ln_fwd(hip, c, x, gamma, beta)
    check_bf16(f"{tag}.y", y, r64["y"], r32["y"])
    check_f32(f"{tag}.mean", mean, r64["mean"], r32["mean"])
    check_f32(f"{tag}.rstd", rstd, r64["rstd"], r32["rstd"])
    y_nostats, _, _ = _ln_fwd(hip, c, x, gamma, beta, stats=False)
    assert torch.equal(y_nostats, y)

    # backward without dgamma / dbeta, then the three routes of the two column sums, each onto non-zero vectors
    dx0, _ = _ln_bwd(hip, c, dy, x, mean, rstd, gamma, None, None, None)
    check_bf16(f"{tag}.dx", dx0, r64["dx"], r32["dx"])
    dg0, db0 = _randn((H,), 5, 3.0), _randn((H,), 6, 3.0)
    want = {k: (i.double() + r64[k], i + r32[k]) for k, i in (("dgamma", dg0), ("dbeta", db0))}
    ws_floats = int(hip.lib().stonk_layernorm_bwd_workspace_floats(rows, H))
    assert ws_floats == min((rows + 3) // 4, 1024) * 2 * H
    for route in ("atomics", "workspace", "deferred"):
        dg, db = dg0.cuda(), db0.cuda()
        ws = None if route == "atomics" else torch.full((ws_floats,), float("nan"), device="cuda")
        dx, _ = _ln_bwd(hip, c, dy, x, mean, rstd, gamma, dg, db, ws, flags=hip.LN_DEFER_REDUCE if route == "deferred" else 0)
        if route == "deferred":
            torch.cuda.synchronize()
            assert torch.equal(dg.cpu(), dg0) and torch.equal(db.cpu(), db0)   # nothing added before the reduce
            hip.call("stonk_layernorm_bwd_reduce", hip.ptr(ws), rows, H, hip.ptr(dg), hip.ptr(db), hip.stream_ptr())
        assert torch.equal(dx, dx0)
        check_f32(f"{tag}.dgamma.{route}", dg, *want["dgamma"])
        check_f32(f"{tag}.dbeta.{route}", db, *want["dbeta"])


# (rows, H, p, which): which of the two dropouts of the backward is on - "in" = STONK_LN_DROPOUT (dy is the gradient of a
# dropped-out y), "out" = dx_drop is asked for, "both". The (4100, .) cases give a wave a second row; (9, .) = three
# workgroups, the last with one live wave, at the three lane widths (512 / 768 / 1024: every <EPL, in, out> instance of the
# lane backward and both of the lane forward) and at 640 for the generic kernels' run-time switches.
_LN_DROP_CASES = ([(rows, H, p, "both") for rows, H in [(4100, 768), (4100, 640), (5, 1536)] for p in (0.1, 0.5)]
                  + [(9, H, 0.1, which) for H in (512, 768, 1024, 640) for which in ("in", "out", "both")])


@pytest.mark.parametrize("rows,H,p,which", _LN_DROP_CASES,
                         ids=[f"{r}-{H}-{p}" + ("" if r != 9 else f"-{w}") for r, H, p, w in _LN_DROP_CASES])
def test_layernorm_dropout_exact_masks(hip, rows, H, p, which):
    c = _LnCase(rows, H)
    tag = f"lndrop[{rows}x{H},p={p},{which}]"
    seed_in, seed_out = 77, 78
    d_in, d_out = which in ("in", "both"), which in ("out", "both")
    k_in, k_out = _keep(range(rows), H, seed_in, p), _keep(range(rows), H, seed_out, p)
    inv = 1.0 / (1.0 - _p32(p))
    zero64, zero32 = torch.zeros((), dtype=torch.float64), torch.zeros(())
    x, dy, gamma, beta = c.x.cuda(), c.dy.cuda(), c.gamma.cuda(), c.beta.cuda()
    flags = hip.LN_DROPOUT if d_in else 0
    y, mean, rstd = _ln_fwd(hip, c, x, gamma, beta, flags=flags, p=p, seed=seed_in)
    if d_in:
        r64, r32 = c.ref(torch.float64, k_in, inv), c.ref(torch.float32, k_in, inv)
        assert (y.cpu()[~k_in] == 0).all(), "an element the generator drops is not zero"
        check_bf16(f"{tag}.y", y, torch.where(k_in, r64["y"] * inv, zero64), torch.where(k_in, r32["y"] * inv, zero32))
    else:
        r64, r32 = c.ref(torch.float64), c.ref(torch.float32)
        check_bf16(f"{tag}.y", y, r64["y"], r32["y"])
    check_f32(f"{tag}.mean", mean, r64["mean"], r32["mean"])
    check_f32(f"{tag}.rstd", rstd, r64["rstd"], r32["rstd"])

    dg0, db0 = _randn((H,), 5, 3.0), _randn((H,), 6, 3.0)
    dg, db = dg0.cuda(), db0.cuda()
    ws = torch.empty(int(hip.lib().stonk_layernorm_bwd_workspace_floats(rows, H)), device="cuda")
    dx, dxd = _ln_bwd(hip, c, dy, x, mean, rstd, gamma, dg, db, ws, flags=flags, p_in=p, seed_in=seed_in, p_out=p,
                      seed_out=seed_out, drop=d_out)
    check_bf16(f"{tag}.dx", dx, r64["dx"], r32["dx"])       # fp64 backward of dy, masked by the oracle (seed_in) with "in"
    if d_out:
        assert (dxd.cpu()[~k_out] == 0).all(), "dx_drop: an element the generator drops (seed_out) is not zero"
        check_bf16(f"{tag}.dx_drop", dxd, torch.where(k_out, r64["dx"] * inv, zero64),
                   torch.where(k_out, r32["dx"] * inv, zero32))
    check_f32(f"{tag}.dgamma", dg, dg0.double() + r64["dgamma"], dg0 + r32["dgamma"])
    check_f32(f"{tag}.dbeta", db, db0.double() + r64["dbeta"], db0 + r32["dbeta"])
    if which == "out":   # dx is the unmasked backward: the very bits of a call that asks for no dx_drop
        dx_plain, _ = _ln_bwd(hip, c, dy, x, mean, rstd, gamma, dg0.cuda(), db0.cuda(), ws)
        assert torch.equal(dx, dx_plain)


# ---- stonk_joint_embed_ln_fwd ----------------------------------------------------------------------------------------

KG, SENT = 53, 7.0


class _JointCase:
    def __init__(self, H, half, B=3, S=16):
        self.B, self.S, self.H, self.half = B, S, H, half
        self.ids = torch.randint(0, KG, (B, S), generator=_gen(20))
        self.tt = torch.randint(0, 2, (B, S), generator=_gen(21))
        self.text = _randn((max(B * half, 1), H), 22, 1.0, 0.0, BF)
        self.table = _randn((KG, H), 23, 0.3)
        self.pos = _randn((S, H), 24, 0.05)
        self.typ = _randn((2, H), 25, 0.05)
        self.gamma = _randn((H,), 26, 0.1, 1.0)
        self.beta = _randn((H,), 27, 0.1)

    def ref(self, dtype, tt=True):
        """Embedding sum and its LayerNorm for every padded position [B * S, H], and the statistics."""
        B, S, H, half = self.B, self.S, self.H, self.half
        src = torch.empty(B, S, H, dtype=dtype)
        if half > 0:
            src[:, :half] = self.text[: B * half].to(dtype).view(B, half, H)
        if half < S:
            src[:, half:] = self.table.to(dtype)[self.ids[:, half:]]
        typ = self.typ.to(dtype)[self.tt if tt else torch.zeros_like(self.tt)]
        emb = ((src + self.pos.to(dtype)[None]) + typ).view(B * S, H)
        y, mean, rstd = torch.native_layer_norm(emb, (H,), self.gamma.to(dtype), self.beta.to(dtype), EPS)
        return dict(sum=emb, y=y, mean=mean.reshape(-1), rstd=rstd.reshape(-1))

    def call(self, hip, ids=None, tt=True, ttv=None, sum_out=True, stats=True, p=0.0, seed=0, pos_of_row=None, n_rows=0,
             type_rows=2):
        B, S, H = self.B, self.S, self.H
        dev = lambda t: t.cuda()
        out = dict(sum=torch.full((B * S, H), SENT, device="cuda", dtype=BF) if sum_out else None,
                   y=torch.full((B * S, H), SENT, device="cuda", dtype=BF),
                   mean=torch.full((B * S,), SENT, device="cuda") if stats else None,
                   rstd=torch.full((B * S,), SENT, device="cuda") if stats else None,
                   err=torch.zeros(1, device="cuda", dtype=torch.int32))
        ids_d = dev(self.ids if ids is None else ids)
        tt_d = dev(self.tt if ttv is None else ttv) if tt else None
        por = None if pos_of_row is None else pos_of_row.to(torch.int32).cuda()
        args = [dev(self.text), dev(self.table), dev(self.pos), dev(self.typ), dev(self.gamma), dev(self.beta)]
        hip.call("stonk_joint_embed_ln_fwd", hip.ptr(ids_d), hip.ptr(tt_d), *[hip.ptr(a) for a in args], hip.ptr(out["sum"]),
                 hip.ptr(out["y"]), hip.ptr(out["mean"]), hip.ptr(out["rstd"]), B, S, self.half, H, KG, type_rows, EPS,
                 hip.LN_DROPOUT if p > 0 else 0, p, seed, hip.ptr(out["err"]), hip.ptr(por), n_rows, hip.stream_ptr())
        torch.cuda.synchronize()
        return out


def _packed_map(B, S):
    """A shuffled subset of the positions, then -1 entries; fewer rows than positions."""
    perm = torch.randperm(B * S, generator=_gen(30))
    live = perm[: B * S - 19]
    return torch.cat([live, torch.full((5,), -1, dtype=torch.long)])


def _rows_of(ref, pos_of_row, n_total, dtype):
    """Expected outputs per OUTPUT row: row i is position pos_of_row[i]; a -1 row is zeros with mean 0, rstd 1."""
    live = pos_of_row >= 0
    idx = pos_of_row.clamp(min=0)
    out = {}
    for k, v in ref.items():
        e = v[idx].to(dtype)
        if k == "rstd":
            e = torch.where(live, e, torch.ones((), dtype=dtype))
        else:
            e = torch.where(live if e.dim() == 1 else live[:, None], e, torch.zeros((), dtype=dtype))
        out[k] = e
    return out


@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("half", [0, 8, 16])
@pytest.mark.parametrize("H", [768, 1032])
def test_joint_embed_ln_fp64(hip, H, half, layout):
    c = _JointCase(H, half)
    n_pos = c.B * c.S
    por = _packed_map(c.B, c.S) if layout == "packed" else None
    n = n_pos if por is None else por.numel()
    row_pos = torch.arange(n_pos) if por is None else por
    kw = dict(pos_of_row=por, n_rows=0 if por is None else n)
    tag = f"joint[H={H},half={half},{layout}]"

    def expect(tt):
        return (_rows_of(c.ref(torch.float64, tt), row_pos, n, torch.float64),
                _rows_of(c.ref(torch.float32, tt), row_pos, n, torch.float32))

    def untouched(out):
        for k in ("sum", "y", "mean", "rstd"):
            if out[k] is not None:
                assert (out[k][n:] == SENT).all(), f"{k}: a row at or past n_rows was written"

    r64, r32 = expect(True)
    out = c.call(hip, **kw)
    assert out["err"].item() == 0
    check_bf16(f"{tag}.sum", out["sum"][:n], r64["sum"], r32["sum"])
    check_bf16(f"{tag}.y", out["y"][:n], r64["y"], r32["y"])
    check_f32(f"{tag}.mean", out["mean"][:n], r64["mean"], r32["mean"])
    check_f32(f"{tag}.rstd", out["rstd"][:n], r64["rstd"], r32["rstd"])
    untouched(out)
    if por is not None:
        dead = (por < 0).cuda()
        assert (out["y"][:n][dead] == 0).all() and (out["sum"][:n][dead] == 0).all()
        assert (out["mean"][:n][dead] == 0).all() and (out["rstd"][:n][dead] == 1).all()

    # null token_type_ids (every position type 0), null sum_out, null mean / rstd
    z64, z32 = expect(False)
    out0 = c.call(hip, tt=False, sum_out=False, stats=False, **kw)
    assert out0["err"].item() == 0
    check_bf16(f"{tag}.y.nulls", out0["y"][:n], z64["y"], z32["y"])
    untouched(out0)

    # dropout: the mask is keyed by the OUTPUT row (the packed row in the packed layout)
    p, seed = 0.25, 91
    keep = _keep(range(n), H, seed, p)
    inv = 1.0 / (1.0 - _p32(p))
    outd = c.call(hip, p=p, seed=seed, **kw)
    assert (outd["y"][:n].cpu()[~keep] == 0).all(), "an element the generator drops is not zero"
    check_bf16(f"{tag}.y.drop", outd["y"][:n], torch.where(keep, r64["y"] * inv, torch.zeros((), dtype=torch.float64)),
               torch.where(keep, r32["y"] * inv, torch.zeros(())))
    assert torch.equal(outd["sum"], out["sum"]) and torch.equal(outd["mean"], out["mean"])
    untouched(outd)


def test_joint_embed_ln_error_bits(hip):
    c = _JointCase(768, 8)
    half = c.half

    def err_of(**kw):
        return c.call(hip, **kw)["err"].item()

    for bad in (-1, KG):
        ids = c.ids.clone()
        ids[1, half + 3] = bad
        assert err_of(ids=ids) == 1                       # entity id outside the table
        ids = c.ids.clone()
        ids[2, half - 1] = bad
        ids[0, 0] = bad
        assert err_of(ids=ids) == 0                       # the text half's ids are not read
    for bad in (-1, 2):
        ttv = c.tt.clone()
        ttv[0, 5] = bad
        assert err_of(ttv=ttv) == 2                       # token type outside [0, type_rows)
    ids = c.ids.clone()
    ids[2, half] = KG + 100
    assert (c.tt == 1).any()
    assert err_of(ids=ids, type_rows=1) == 3             # type id 1 with a single type row and a bad entity id, one launch


# ---- stonk_text_embed_ln_fwd -----------------------------------------------------------------------------------------

def test_text_embed_ln_fp64(hip):
    B, S, H, V, ld = 4, 8, 768, 300, 21
    ids = torch.randint(0, V, (B, ld), generator=_gen(40))
    ids[:, S:] = V + 5                                    # past the S columns that are read: must not matter
    word, pos, typ = _randn((V, H), 41, 0.05), _randn((S + 3, H), 42, 0.05), _randn((2, H), 43, 0.05)
    gamma, beta = _randn((H,), 44, 0.1, 1.0), _randn((H,), 45, 0.1)

    def ref(dtype):
        emb = (word.to(dtype)[ids[:, :S]] + pos.to(dtype)[None, :S]) + typ.to(dtype)[0]
        return torch.native_layer_norm(emb.view(B * S, H), (H,), gamma.to(dtype), beta.to(dtype), EPS)[0]

    def run(ids_t, p, seed):
        y = torch.full((B * S + 2, H), SENT, device="cuda", dtype=BF)
        err = torch.zeros(1, device="cuda", dtype=torch.int32)
        t = [x.cuda() for x in (ids_t, word, pos, typ, gamma, beta)]
        hip.call("stonk_text_embed_ln_fwd", hip.ptr(t[0]), ld, *[hip.ptr(a) for a in t[1:]], hip.ptr(y), B, S, H, V, EPS,
                 hip.LN_DROPOUT if p > 0 else 0, p, seed, hip.ptr(err), hip.stream_ptr())
        torch.cuda.synchronize()
        assert (y[B * S:] == SENT).all()
        return y[: B * S], err.item()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    y, err = run(ids, 0.0, 0)
    assert err == 0
    check_bf16("text_embed.y", y, r64, r32)
    p, seed = 0.1, 17
    keep = _keep(range(B * S), H, seed, p)
    inv = 1.0 / (1.0 - _p32(p))
    yd, err = run(ids, p, seed)
    assert err == 0
    assert (yd.cpu()[~keep] == 0).all(), "an element the generator drops is not zero"
    check_bf16("text_embed.y.drop", yd, torch.where(keep, r64 * inv, torch.zeros((), dtype=torch.float64)),
               torch.where(keep, r32 * inv, torch.zeros(())))
    for bad in (-1, V):
        ids2 = ids.clone()
        ids2[3, S - 1] = bad
        assert run(ids2, 0.0, 0)[1] == 4


# ---- stonk_embed_grad ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("B,S,H", [(1, 3, 8), (7, 5, 768), (65, 4, 1024), (130, 3, 64)])
def test_embed_grad_fp64(hip, B, S, H, mapped):
    """B = 65 and 130: second and third trip of the batch loop (64 sequences per trip)."""
    n_pos = B * S
    tt = torch.randint(0, 2, (B, S), generator=_gen(50))
    if mapped:   # packed layout: some positions have no row, the others point into a shuffled dx
        live = torch.rand(n_pos, generator=_gen(51)) < 0.7
        live[0] = True
        n_dx = int(live.sum())
        rop = torch.full((n_pos,), -1, dtype=torch.long)
        rop[live] = torch.randperm(n_dx, generator=_gen(52))
    else:
        n_dx, rop = n_pos, torch.arange(n_pos)
    dx = _randn((n_dx, H), 53, 1.0, 0.0, BF)
    dpos0, dtyp0 = _randn((S, H), 54, 2.0), _randn((2, H), 55, 2.0)
    tag = f"embed_grad[{B}x{S}x{H},{'map' if mapped else 'nomap'}]"

    def ref(dtype, ttv):
        d = torch.where((rop >= 0)[:, None], dx.to(dtype)[rop.clamp(min=0)], torch.zeros((), dtype=dtype)).view(B, S, H)
        dpos = dpos0.to(dtype) + d.sum(0)
        dtyp = dtyp0.to(dtype) + torch.stack([(d * (ttv == t)[..., None].to(dtype)).sum((0, 1)) for t in (0, 1)])
        return dpos, dtyp

    def run(ttv, type_rows):
        dpos, dtyp = dpos0.cuda(), dtyp0.cuda()
        dx_d = dx.cuda()
        tt_d = None if ttv is None else ttv.cuda()
        rop_d = rop.to(torch.int32).cuda() if mapped else None
        hip.call("stonk_embed_grad", hip.ptr(dx_d), hip.ptr(tt_d), hip.ptr(dpos), hip.ptr(dtyp), B, S, H, type_rows,
                 hip.ptr(rop_d), hip.stream_ptr())
        torch.cuda.synchronize()
        return dpos, dtyp

    dpos, dtyp = run(tt, 2)
    (p64, t64), (p32, t32) = ref(torch.float64, tt), ref(torch.float32, tt)
    check_f32(f"{tag}.dpos", dpos, p64, p32)
    check_f32(f"{tag}.dtype", dtyp, t64, t32)
    # null type ids: everything is type 0
    zeros = torch.zeros_like(tt)
    (p64, t64), (p32, t32) = ref(torch.float64, zeros), ref(torch.float32, zeros)
    dpos, dtyp = run(None, 2)
    check_f32(f"{tag}.dpos.nulltt", dpos, p64, p32)
    check_f32(f"{tag}.dtype.nulltt", dtyp, t64, t32)
    assert torch.equal(dtyp[1].cpu(), dtyp0[1])
    # one type row: row 1 of the buffer is not the kernel's to touch
    dpos, dtyp = run(None, 1)
    check_f32(f"{tag}.dtype.rows1", dtyp[0], t64[0], t32[0])
    assert torch.equal(dtyp[1].cpu(), dtyp0[1])
    # a third type row would get no gradient: refused, nothing written
    with pytest.raises(hip.StonkHipError, match="-2"):
        run(tt, 3)
