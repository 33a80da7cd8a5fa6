"""Every exported entry point of the six row-wise sources (csrc/norm, loss, small, optim, topk, text_embed .hip: 34 of them)
called ONCE on fixed inputs, the outputs written to an .npz - to compare two BUILDS of the library bit for bit, each in a
process of its own:
  STONK_HIP_LIB=ab_ref/libstonk_hip.so python tools/rowwise_entries.py --out parent.npz
  python tools/rowwise_entries.py --out branch.npz
  python tools/rowwise_entries.py --compare parent.npz branch.npz
Equal bits are required of every array except the ones that fp32 atomics sum in arrival order (ATOMIC below): each of those
is held, in the run that produced it, to its fp64 reference with tests/parity_util.check_f32, as its GPU test holds it."""
import argparse
import os
import struct
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stonkgs_amd import _hip as hip  # noqa: E402
from tests.parity_util import check_f32, gen, randn  # noqa: E402
from oracle import dropout_oracle as do  # noqa: E402
from tests import optim_ref as orf  # noqa: E402

BF, F16, EPS = torch.bfloat16, torch.float16, 1e-12
# (all three dgamma / dbeta routes end in atomics: the workspace routes' ln_partial_reduce_kernel adds up to 32 partial sums per
# column in arrival order)
ATOMIC = {f"ln_bwd.{r}.{k}" for r in ("atomics", "workspace", "deferred") for k in ("dgamma", "dbeta")} | {"embed_grad.dtype", "word_embed_grad.dword", "transpose.colsum"}
OUT = {}


def put(name, t):
    t = t.detach().cpu().contiguous()
    OUT[name] = (t.view(torch.int16) if t.dtype in (BF, F16) else t).numpy()


def S():
    return hip.stream_ptr()


def norm_entries():
    rows, H = 9, 768
    x, dy = randn((rows, H), 1, 2.0, 0.5, BF).cuda(), randn((rows, H), 2, 1.0, 0.0, BF).cuda()
    gamma, beta = randn((H,), 3, 0.5, 1.0).cuda(), randn((H,), 4, 0.1).cuda()
    y, mean, rstd = torch.zeros_like(x), torch.zeros(rows, device="cuda"), torch.zeros(rows, device="cuda")
    hip.call("stonk_layernorm_fwd", hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), rows, H,
             EPS, hip.LN_DROPOUT, 0.1, 77, S())
    put("ln_fwd.y", y), put("ln_fwd.mean", mean), put("ln_fwd.rstd", rstd)
    n_ws = int(hip.lib().stonk_layernorm_bwd_workspace_floats(rows, H))
    OUT["ln_bwd_workspace_floats"] = np.asarray([n_ws, int(hip.lib().stonk_layernorm_bwd_workspace_floats(40000, 640))])
    # dgamma / dbeta in fp64 and fp32: the backward of native_layer_norm with dy under the oracle's keep-mask (seed 77)
    k_in = torch.from_numpy(do.keep(np.arange(rows), np.arange(H), 77, 0.1))
    inv = 1.0 / (1.0 - float(np.float32(0.1)))
    want = {}
    for dt in (torch.float64, torch.float32):
        gl, bl = gamma.cpu().to(dt).requires_grad_(True), beta.cpu().to(dt).requires_grad_(True)
        yl = torch.native_layer_norm(x.cpu().to(dt), (H,), gl, bl, EPS)[0]
        yl.backward(torch.where(k_in, dy.cpu().to(dt) * inv, torch.zeros((), dtype=dt)))
        want[dt] = (gl.grad, bl.grad)
    for route in ("workspace", "deferred", "atomics"):
        dx, dxd = torch.zeros_like(x), torch.zeros_like(x)
        dg, db = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
        ws = None if route == "atomics" else torch.zeros(n_ws, device="cuda")
        hip.call("stonk_layernorm_bwd", hip.ptr(dy), hip.ptr(x), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma), hip.ptr(dx),
                 hip.ptr(dxd), hip.ptr(dg), hip.ptr(db), rows, H, hip.LN_DROPOUT | (hip.LN_DEFER_REDUCE if route == "deferred" else 0),
                 0.1, 77, 0.1, 78, hip.ptr(ws), n_ws if ws is not None else 0, S())
        if route == "deferred":
            hip.call("stonk_layernorm_bwd_reduce", hip.ptr(ws), rows, H, hip.ptr(dg), hip.ptr(db), S())
        check_f32(f"ln_bwd.{route}.dgamma", dg, want[torch.float64][0], want[torch.float32][0])
        check_f32(f"ln_bwd.{route}.dbeta", db, want[torch.float64][1], want[torch.float32][1])
        put(f"ln_bwd.{route}.dx", dx), put(f"ln_bwd.{route}.dx_drop", dxd)
        put(f"ln_bwd.{route}.dgamma", dg), put(f"ln_bwd.{route}.dbeta", db)
    # the generic kernels (H = 640) once as well
    c = randn((5, 640), 5, 1.0, 0.0, BF).cuda()
    g2, b2, y2 = randn((640,), 6, 0.5, 1.0).cuda(), randn((640,), 7, 0.1).cuda(), torch.zeros(5, 640, device="cuda", dtype=BF)
    hip.call("stonk_layernorm_fwd", hip.ptr(c), hip.ptr(g2), hip.ptr(b2), hip.ptr(y2), 0, 0, 5, 640, EPS, 0, 0.0, 0, S())
    put("ln_fwd_generic.y", y2)

    B, Sq, half, KG = 3, 16, 8, 53
    ids = torch.randint(0, KG, (B, Sq), generator=gen(20)).cuda()
    tt = torch.randint(0, 2, (B, Sq), generator=gen(21)).cuda()
    text, table = randn((B * half, H), 22, 1.0, 0.0, BF).cuda(), randn((KG, H), 23, 0.3).cuda()
    pos, typ = randn((Sq, H), 24, 0.05).cuda(), randn((2, H), 25, 0.05).cuda()
    so, yo = torch.zeros(B * Sq, H, device="cuda", dtype=BF), torch.zeros(B * Sq, H, device="cuda", dtype=BF)
    mo, ro, err = torch.zeros(B * Sq, device="cuda"), torch.zeros(B * Sq, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
    hip.call("stonk_joint_embed_ln_fwd", hip.ptr(ids), hip.ptr(tt), hip.ptr(text), hip.ptr(table), hip.ptr(pos), hip.ptr(typ),
             hip.ptr(gamma), hip.ptr(beta), hip.ptr(so), hip.ptr(yo), hip.ptr(mo), hip.ptr(ro), B, Sq, half, H, KG, 2, EPS,
             hip.LN_DROPOUT, 0.1, 5, hip.ptr(err), 0, 0, S())
    put("joint.sum", so), put("joint.y", yo), put("joint.mean", mo), put("joint.rstd", ro), put("joint.err", err)
    yt = torch.zeros(B * Sq, H, device="cuda", dtype=BF)
    hip.call("stonk_text_embed_ln_fwd", hip.ptr(ids), Sq, hip.ptr(table), hip.ptr(pos), hip.ptr(typ), hip.ptr(gamma), hip.ptr(beta),
             hip.ptr(yt), B, Sq, H, KG, EPS, 0, 0.0, 0, hip.ptr(err), S())
    put("text_embed_ln.y", yt)
    dxe = randn((B * Sq, H), 26, 1.0, 0.0, BF).cuda()
    dpos, dtyp = torch.zeros(Sq, H, device="cuda"), torch.zeros(2, H, device="cuda")
    hip.call("stonk_embed_grad", hip.ptr(dxe), hip.ptr(tt), hip.ptr(dpos), hip.ptr(dtyp), B, Sq, H, 2, 0, S())
    d64 = dxe.double().cpu().view(B, Sq, H)
    want = lambda dt: torch.stack([(d64.to(dt) * (tt.cpu() == t)[..., None]).sum((0, 1)) for t in (0, 1)])
    check_f32("embed_grad.dtype", dtyp, want(torch.float64), want(torch.float32))
    put("embed_grad.dpos", dpos), put("embed_grad.dtype", dtyp)
    dword = torch.zeros(KG, H, device="cuda")
    hip.call("stonk_word_embed_grad", hip.ptr(dxe), H, hip.ptr(ids), 0, hip.ptr(dword), H, KG, -1, B, Sq, H, hip.ptr(err), S())
    wantw = lambda dt: torch.zeros(KG, H, dtype=dt).index_add_(0, ids.cpu().view(-1), dxe.cpu().to(dt))
    check_f32("word_embed_grad.dword", dword, wantw(torch.float64), wantw(torch.float32))
    put("word_embed_grad.dword", dword)


def loss_entries():
    B, Sq, half, H = 3, 16, 8, 72
    labels = torch.full((B * half,), -100, dtype=torch.int64)
    labels[torch.randperm(B * half, generator=gen(30))[:9]] = torch.randint(0, 50, (9,), generator=gen(31))
    labels = labels.cuda()
    rows, tgts = (torch.zeros(B * half, device="cuda", dtype=torch.int32) for _ in range(2))
    cnt = torch.zeros(1, device="cuda", dtype=torch.int32)
    hip.call("stonk_label_compact", hip.ptr(labels), B * half, half, Sq, 0, hip.ptr(rows), hip.ptr(tgts), hip.ptr(cnt), 0, S())
    put("label_compact.rows", rows[:9]), put("label_compact.targets", tgts[:9]), put("label_compact.count", cnt)
    src = randn((B * Sq, H), 32, 1.0, 0.0, BF).cuda()
    dst = torch.full((128, H), 3.0, device="cuda", dtype=BF)
    hip.call("stonk_gather_rows_bf16", hip.ptr(src), H, hip.ptr(rows), hip.ptr(cnt), hip.ptr(dst), H, H, 128, S())
    put("gather.dst", dst)
    back = torch.zeros(B * Sq, H, device="cuda", dtype=BF)
    hip.call("stonk_scatter_rows_bf16", hip.ptr(dst), H, hip.ptr(rows), hip.ptr(cnt), hip.ptr(back), H, H, S())
    put("scatter.dst", back)
    src32, back32 = randn((128, H), 33).cuda(), torch.zeros(B * Sq, H, device="cuda", dtype=BF)
    hip.call("stonk_scatter_rows_f32_to_bf16", hip.ptr(src32), H, hip.ptr(rows), hip.ptr(cnt), hip.ptr(back32), H, H, S())
    put("scatter_f32.dst", back32)
    ncols, npad = 1237, 1240
    for name, dt in (("xent", torch.float32), ("xent_f16", F16)):
        logits = randn((64, npad), 34, 2.0).to(dt).cuda()
        loss, dl = torch.zeros(1, device="cuda"), torch.full((64, npad), 3.0, device="cuda", dtype=BF)
        err = torch.zeros(1, device="cuda", dtype=torch.int32)
        hip.call(f"stonk_softmax_{name}_fwd_bwd", hip.ptr(logits), npad, ncols, npad, hip.ptr(tgts), hip.ptr(cnt), hip.ptr(loss),
                 hip.ptr(dl), npad, 0.5, 64, hip.ptr(err), S())
        put(f"{name}.loss", loss), put(f"{name}.dlogits", dl), put(f"{name}.err", err)
        for kname, k in (("topk", 5), ("topk1", 1)):
            tv, ti = torch.zeros(64, k, device="cuda"), torch.zeros(64, k, device="cuda", dtype=torch.int32)
            lse, rank, tl = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda", dtype=torch.int32), torch.zeros(64, device="cuda")
            hip.call("stonk_row_topk_f32" if dt == torch.float32 else "stonk_row_topk_f16", hip.ptr(logits), npad, ncols, hip.ptr(tgts),
                     hip.ptr(cnt), 64, k, hip.ptr(tv), hip.ptr(ti), hip.ptr(lse), hip.ptr(rank), hip.ptr(tl), S())
            n = int(cnt.item())
            put(f"{name}.{kname}.val", tv[:n]), put(f"{name}.{kname}.idx", ti[:n]), put(f"{name}.{kname}.lse", lse[:n])
            put(f"{name}.{kname}.rank", rank[:n]), put(f"{name}.{kname}.tgt", tl[:n])
    nl, lab = randn((5, 2), 35).cuda(), torch.tensor([0, 1, -100, 1, 0]).cuda()
    lsc, dnl, err = torch.zeros(2, device="cuda"), torch.zeros(5, 2, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
    hip.call("stonk_nsp_xent_fwd_bwd", hip.ptr(nl), hip.ptr(lab), 5, 2, hip.ptr(lsc), hip.ptr(dnl), 1.0, hip.ptr(err), S())
    put("nsp.sum_cnt", lsc), put("nsp.dlogits", dnl)
    one = torch.tensor([3], device="cuda", dtype=torch.int32)
    lo = torch.zeros(4, device="cuda")
    hip.call("stonk_loss_finalize", hip.ptr(lsc), hip.ptr(one), hip.ptr(lsc), hip.ptr(one), hip.ptr(lsc), hip.ptr(lo), S())
    put("loss_finalize", lo)


def small_entries():
    M, N, K = 70, 9, 300   # (a second piece of WG_MC rows, a partial block of 8 features, a partial block of 256 columns)
    x, W, b = randn((M, K), 40, 1.0, 0.0, BF).cuda(), randn((N, K), 41, 0.1).cuda(), randn((N,), 42, 0.1).cuda()
    y = torch.zeros(M, N, device="cuda")
    hip.call("stonk_small_linear_fwd", hip.ptr(x), K, hip.ptr(W), hip.ptr(b), hip.ptr(y), M, N, K, hip.SMALL_TANH, S())
    put("small_fwd.y", y)
    dy = randn((M, N), 43).cuda()
    dW, db, dxf = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(M, K, device="cuda")
    dxb = randn((M, K), 44, 1.0, 0.0, BF).cuda()
    hip.call("stonk_small_linear_bwd", hip.ptr(dy), hip.ptr(y), hip.ptr(x), K, hip.ptr(W), hip.ptr(dW), hip.ptr(db), hip.ptr(dxf),
             hip.ptr(dxb), K, M, N, K, hip.SMALL_TANH, S())
    put("small_bwd.dW", dW), put("small_bwd.db", db), put("small_bwd.dx", dxf), put("small_bwd.dx_bf16", dxb)
    M2 = 1600                  # (more rows than the tiled weight gradient stages: the untiled kernel)
    x2, y2, dy2 = randn((M2, K), 45).cuda(), torch.tanh(randn((M2, N), 46)).cuda(), randn((M2, N), 47).cuda()
    dW2, db2 = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
    hip.call("stonk_small_linear_bwd", hip.ptr(dy2), hip.ptr(y2), hip.ptr(x2), K, hip.ptr(W), hip.ptr(dW2), hip.ptr(db2), 0, 0, 0,
             M2, N, K, hip.SMALL_TANH | hip.SMALL_X_F32, S())
    put("small_bwd_untiled.dW", dW2), put("small_bwd_untiled.db", db2)
    dg, u, du = randn((808,), 48, 1.0, 0.0, BF).cuda(), randn((808,), 49, 1.0, 0.0, BF).cuda(), torch.zeros(808, device="cuda", dtype=BF)
    hip.call("stonk_gelu_bwd_bf16", hip.ptr(dg), hip.ptr(u), hip.ptr(du), 808, S())
    put("gelu_bwd", du)
    xd, yd = randn((777,), 50).cuda(), torch.zeros(777, device="cuda")
    hip.call("stonk_dropout_f32", hip.ptr(xd), hip.ptr(yd), 777, 0.1, 9, S())
    put("dropout_f32", yd)
    for mode in (hip.LOSS_MSE, hip.LOSS_BCE):
        lg, tg = randn((6, 3), 51).cuda(), torch.rand((6, 3), generator=gen(52)).cuda()
        lo, dl = torch.zeros(1, device="cuda"), torch.zeros(6, 3, device="cuda")
        hip.call("stonk_elementwise_loss_fwd_bwd", hip.ptr(lg), hip.ptr(tg), 6, 3, mode, hip.ptr(lo), hip.ptr(dl), 1.0, S())
        put(f"elementwise_loss.{mode}.loss", lo), put(f"elementwise_loss.{mode}.dlogits", dl)
    num, den, q = torch.tensor([3.0], device="cuda"), torch.tensor([7.0], device="cuda"), torch.zeros(1, device="cuda")
    hip.call("stonk_ratio_f32", hip.ptr(num), hip.ptr(den), hip.ptr(q), S())
    put("ratio", q)


def optim_entries():
    n_ws = int(hip.lib().stonk_sumsq_workspace_floats())
    OUT["sumsq_workspace_floats"] = np.asarray([n_ws])
    x, ws = randn((300007,), 60).cuda(), torch.zeros(n_ws, device="cuda")
    a, b, extra = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), torch.rand(130, generator=gen(61)).cuda()
    hip.call("stonk_sumsq_f32", hip.ptr(x), x.numel(), hip.ptr(a), hip.ptr(ws), n_ws, S())
    hip.call("stonk_sumsq_f32_plus", hip.ptr(x), x.numel(), hip.ptr(b), hip.ptr(ws), n_ws, hip.ptr(extra), 130, S())
    put("sumsq", a), put("sumsq_plus", b)
    hip.call("stonk_scale_f32", hip.ptr(x), x.numel(), 0.5, S())
    xb = torch.zeros(x.numel(), device="cuda", dtype=BF)
    hip.call("stonk_cast_f32_to_bf16", hip.ptr(x), hip.ptr(xb), x.numel(), S())
    put("scale", x), put("cast", xb)

    index, numel = orf.layout()   # (the small flat buffer of the optimizer parity tests: tiled and flat tensors, pad rows)
    g = torch.Generator(device="cpu").manual_seed(11)
    p0, g0 = (torch.randn(numel, generator=g) * 0.05).cuda(), (torch.randn(numel, generator=g) * 0.02).cuda()
    m0, v0 = (torch.randn(numel, generator=g) * 0.01).cuda(), (torch.rand(numel, generator=g) * 1e-4).cuda()
    nrm = (g0.double() ** 2).sum().float().reshape(1)
    dtab = torch.tensor(orf.decay_spans(index), dtype=torch.int64, device="cuda").reshape(-1, 2)
    doff, _, _, dn = index["d.weight"]
    ktab = torch.tensor([(doff, doff + dn)], dtype=torch.int64, device="cuda")
    scal = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0 - 0.9 ** 3, 1.0 - 0.999 ** 3, hip.ptr(nrm), 1.0, 0.5)
    dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    for tiled in (False, True):
        p, gr, m, v = p0.clone(), g0.clone(), m0.clone(), v0.clone()
        pb = torch.full((numel,), 3.0, device="cuda", dtype=BF)
        wts = {name: torch.full((index[name][1][1], (index[name][2][0] + 63) // 64 * 64), 7.0, device="cuda", dtype=BF)
               for name in orf.tiled(index)}
        tiles, n_tiles, spans, chunks = orf.host_tables(index, numel, lambda name: wts[name].data_ptr())
        if tiled:
            td, flat = dev(orf.pack_tiles(tiles)), torch.tensor(spans, dtype=torch.int64, device="cuda").reshape(-1, 3)
            hip.call("stonk_adamw_step_tiled", hip.ptr(p), hip.ptr(gr), hip.ptr(m), hip.ptr(v), hip.ptr(pb), numel, *scal, hip.ptr(dtab),
                     dtab.shape[0], hip.ptr(ktab), 1, hip.ptr(td), len(tiles), n_tiles, hip.ptr(flat), len(spans), chunks, S())
        else:
            hip.call("stonk_adamw_step", hip.ptr(p), hip.ptr(gr), hip.ptr(m), hip.ptr(v), hip.ptr(pb), numel, *scal, hip.ptr(dtab),
                     dtab.shape[0], 0, S())
            # TransposeDesc: in, out, ld_in, ld_out, rows, cols, first_tile, col_tiles, pad - the W^T copies from the mirror
            desc, first = [], 0
            for off, wt, ld_out, rows, _, cols, _, col_tiles in tiles:
                desc.append(struct.pack("<QQqqqiiii", pb.data_ptr() + 2 * off, wt, cols, ld_out, rows, cols, first, col_tiles, 0))
                first += (rows + 63) // 64 * col_tiles
            tr = dev(b"".join(desc))
            hip.call("stonk_transpose_bf16_batched", hip.ptr(tr), len(desc), first, S())
        tag = "adamw_tiled" if tiled else "adamw_flat"
        for k, t in (("p", p), ("g", gr), ("m", m), ("v", v), ("bf16", pb)):
            put(f"{tag}.{k}", t)
        for name, t in wts.items():
            put(f"{tag}.wt.{name}", t)

    rows, cols = 130, 72
    src, out = randn((rows, cols), 62, 1.0, 0.0, BF).cuda(), torch.full((cols, 192), 3.0, device="cuda", dtype=BF)
    colsum, live = torch.zeros(cols, device="cuda"), torch.tensor([100], device="cuda", dtype=torch.int32)
    hip.call("stonk_transpose_bf16", hip.ptr(src), cols, hip.ptr(out), 192, rows, cols, hip.ptr(colsum), hip.ptr(live), S())
    want = lambda dt: src[:100].cpu().to(dt).sum(0)
    check_f32("transpose.colsum", colsum, want(torch.float64), want(torch.float32))
    put("transpose.out", out[:, :128]), put("transpose.colsum", colsum)   # (row tiles past the live rows' round-up are not written)
    src32, out32 = randn((rows, cols), 63).cuda(), torch.full((cols, 192), 3.0, device="cuda", dtype=BF)
    hip.call("stonk_transpose_f32_to_bf16", hip.ptr(src32), hip.ptr(out32), rows, cols, 192, S())
    put("transpose_f32.out", out32)


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(Bz.files), set(A.files) ^ set(Bz.files)
    bad = []
    for k in sorted(A.files):
        same = A[k].shape == Bz[k].shape and A[k].tobytes() == Bz[k].tobytes()
        kind = "atomics (check_f32 in its own run)" if k in ATOMIC else "bits"
        print(f"{k:40s} {str(A[k].shape):16s} {kind:34s} {'equal' if same else 'DIFFERENT'}")
        if not same and k not in ATOMIC:
            bad.append(k)
    print(f"{len(A.files)} arrays, {len(bad)} differ where equal bits are required: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    torch.cuda.set_device(0)
    for f in (norm_entries, loss_entries, small_entries, optim_entries):
        f()
        torch.cuda.synchronize()
    np.savez(args.out, **OUT)
    print(f"{len(OUT)} arrays from {hip.LIB_PATH} -> {args.out}")
