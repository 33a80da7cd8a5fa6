"""Reference, bounds and cases of the attention parity tests (test_attention_parity_gpu.py, test_attention_ref_cpu.py).

Reference r: per sequence and head, in float64 on the CPU from the same bf16 inputs,

    s = q k^T * scale + bias      P = softmax(s)      Pd = P o keep / (1-p)      O = Pd V      lse = logsumexp(s)
    dV = Pd^T dO      dP = (dO V^T) o keep / (1-p)      dS = P o (dP - rowsum(dO o O))
    dQ = scale * dS K             dK = scale * dS^T Q

`keep` is oracle/dropout_oracle.attention_keep, never read off a kernel output. A masked key has P = 0 exactly; a sequence
with NO unmasked key attends uniformly over its own n rows (s = 0: what finfo.min does to the eager path's scores). With
query limits only the first nq rows of a sequence are queries: O, lse and dQ exist for them, dK / dV take their gradient.

Per-element bound E (first order, u = 2^-8 as in parity_util.check_bf16), from the kernels' known rounding points - P to
bf16 before P.V and P^T.dO, dS to bf16 before dS.K and dS^T.Q, the bf16 stores, delta taken from the stored bf16 O:

    E_O  = u (|O| + Pd |V|)                      (store; P's rounding through the product)
    d_i  = sum_d |dO_id| E_O[i,d]                (what delta_i inherits from the stored O)
    E_dV = u (|dV| + Pd^T |dO|)
    W    = u |dS| + P o d                        (dS's rounding; delta's error times P)
    E_dQ = u |dQ| + scale * W |K|
    E_dK = u |dK| + scale * W^T |Q|

Every element must satisfy |got - r| <= E + A, with A = parity_util.tol_a(r32, r) and r32 the same computation in torch
float32 on the CPU (A covers exp2, the fp32 summation order and elements whose E is exactly 0, e.g. masked keys).

Per-block noise level: r16 is the computation in float32 with P, dS and the four outputs rounded to bf16 at the points
above (and delta from the rounded O). For every (sequence, head) block of at least 64 rows whose reference is not
identically zero:  ||got - r|| / ||r||  <=  2 ||r16 - r|| / ||r||.  The kernel and r16 make statistically the same
rounding errors; the factor 2 covers the spread over a small block. r16 takes the forward as the kernel does, in 64-key
tiles with a running maximum (P is rounded relative to the maximum so far, the sums are rescaled): with one global
maximum instead, the dK block of a sequence with ONE query row (127 keys, query limit 1) is a single draw of delta's
error times a rank-one matrix, and the kernel's 6.94e-3 stood against 2 x 3.22e-3 - the tiled float32 emulation gives
that same 6.94e-3, so the kernel rounds correctly and the yardstick, not the factor, was what had to follow it.

check_case() prints one PARITY line per output before it asserts (run with -s; profiles/attention_parity.md collects them).
"""
import functools
import math

import numpy as np
import torch

from oracle import dropout_oracle as do
from tests.parity_util import _report, gen, tol_a

U = 2.0 ** -8
OUT_SENTINEL = 7.0


# ------------------------------------------------------------------ cases
def _padded_mask(B, S, seed):
    """The STonKGs layout (a padded text half, the entity half live) and a masked tail on the last sequence."""
    lens = torch.randint(S // 8, S // 2, (B,), generator=gen(seed))
    mask = torch.ones(B, S, dtype=torch.long)
    for b in range(B):
        mask[b, int(lens[b]): S // 2] = 0
    mask[B - 1, S - 5:] = 0
    return mask


def _case(name, B, NH, S, p, data_seed, scale=0.125, mask=None, lens=None, qlim=None, trailing=0, onehot=None):
    c = dict(name=name, B=B, NH=NH, S=S, p=p, scale=scale, seed=1000 + data_seed, data_seed=data_seed, mask=mask, lens=lens,
             qlim=qlim, onehot=onehot)
    c["T"] = B * S if lens is None else sum(lens) + trailing
    return c


def _packed_mask(lens, trailing, dead):
    """One word per packed row; `dead`: (sequence, first row, last row + 1) ranges of masked rows; trailing rows masked."""
    cu = np.concatenate([[0], np.cumsum(lens)])
    mask = torch.ones(int(cu[-1]) + trailing, dtype=torch.long)
    for b, lo, hi in dead:
        mask[int(cu[b]) + lo: int(cu[b]) + hi] = 0
    mask[int(cu[-1]):] = 0
    return mask


def _spread_keys(n):
    """64 distinct keys of a sequence of n >= 64 rows, spread over every key tile and both parities."""
    keys = sorted({(i * n) // 64 + (i % 2 if n >= 128 else 0) for i in range(64)})
    assert len(keys) == 64 and keys[-1] < n and len({k // 64 for k in keys}) == (n + 63) // 64 and len({k % 2 for k in keys}) == 2
    return keys


def _build_cases():
    cs = []
    # padded, each with and without a mask at p = 0 and p = 0.1 (2x3: the remainder branch of attn_block; 4x2: the
    # XCD-interleaved branch with two 128-row blocks per head)
    for i, (B, NH, S) in enumerate([(1, 1, 128), (2, 3, 256), (4, 2, 256)]):
        for masked in (False, True):
            for p in (0.0, 0.1):
                scale = 0.2 if (B, masked, p) == (2, True, 0.1) else 0.125
                cs.append(_case(f"pad{B}x{NH}x{S}-{'mask' if masked else 'nomask'}-p{p}", B, NH, S, p, 11 + i, scale=scale,
                                mask=_padded_mask(B, S, 50 + i) if masked else None))
    # tile skipping
    m = torch.ones(4, 512, dtype=torch.long)
    m[0, 40:256] = 0      # tiles 1-3 dead, the 128-key block 1 entirely
    m[1, :] = 0           # no live key
    m[2, 1:448] = 0       # [CLS] and the last tile only
    m[3, 100:130] = 0     # no dead tile
    cs.append(_case("skip4x2x512-p0.1", 4, 2, 512, 0.1, 21, mask=m))
    for S in (1024, 1152):   # the last size that computes live bits, the first that walks every tile: tile 0 and the last live
        m = torch.ones(1, S, dtype=torch.long)
        m[0, 1:S - 64] = 0
        cs.append(_case(f"skip1x1x{S}-p0.1", 1, 1, S, 0.1, 22, mask=m))
    # packed layout: ragged lengths, an empty sequence, masked rows in the middle of one sequence and at the tail of another,
    # trailing rows that belong to no sequence; then the same with query limits (the last larger than its sequence)
    lens = [1, 33, 63, 64, 65, 0, 127, 129, 256]
    pm = _packed_mask(lens, 29, [(8, 100, 117), (7, 109, 129)])
    for p in (0.0, 0.25):
        cs.append(_case(f"packed-p{p}", len(lens), 2, 256, p, 31, mask=pm, lens=lens, trailing=29))
        cs.append(_case(f"packed-qlim-p{p}", len(lens), 2, 256, p, 32, scale=0.2 if p else 0.125, mask=pm, lens=lens,
                        qlim=[1, 0, 63, 64, 65, 0, 1, 128, 300], trailing=29))
    # exact mask: 64 live keys per sequence with one-hot V rows
    keys = _spread_keys(256)
    m = torch.zeros(2, 256, dtype=torch.long)
    m[:, keys] = 1
    cs.append(_case("exact-pad-p0.25", 2, 2, 256, 0.25, 41, mask=m, onehot=[keys, keys]))
    lens = [200, 97, 256, 64]
    oh = [_spread_keys(n) for n in lens]
    cu = np.concatenate([[0], np.cumsum(lens)])
    m = torch.zeros(int(cu[-1]) + 13, dtype=torch.long)
    for b, ks in enumerate(oh):
        m[[int(cu[b]) + k for k in ks]] = 1
    cs.append(_case("exact-packed-p0.25", len(lens), 2, 256, 0.25, 42, mask=m, lens=lens, qlim=[70, 300, 256, 33], trailing=13,
                    onehot=oh))
    # no unmasked key in a whole sequence
    lens = [65, 128, 100]
    for p in (0.0, 0.25):
        cs.append(_case(f"nokey-packed-p{p}", 3, 2, 256, p, 51, mask=_packed_mask(lens, 7, [(0, 0, 65), (1, 0, 128), (2, 40, 57)]),
                        lens=lens, trailing=7))
    for S in (1152, 2048):
        m = torch.ones(2, S, dtype=torch.long)
        m[0, :] = 0
        m[1, 70:S // 2 + 5] = 0
        cs.append(_case(f"nokey-pad2x1x{S}-p0.1", 2, 1, S, 0.1, 52, mask=m))
    return {c["name"]: c for c in cs}


CASES = _build_cases()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """qkv bf16 [T, 3H] and dout bf16 [T, H], made on the CPU with a seeded generator."""
    c = CASES[name]
    H = c["NH"] * 64
    g = gen(c["data_seed"])
    qkv = (torch.randn(c["T"], 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dout = torch.randn(c["T"], H, generator=g).to(torch.bfloat16)
    if c["onehot"] is not None:
        v = qkv[:, 2 * H:]
        for b, lo, n, nq in sequences(c):
            rows = torch.tensor(c["onehot"][b]) + lo
            v[rows] = torch.eye(64, dtype=torch.bfloat16).repeat(1, c["NH"])
    return qkv, dout


def sequences(c):
    """(b, first row, rows, query rows) of every sequence."""
    if c["lens"] is None:
        return [(b, b * c["S"], c["S"], c["S"]) for b in range(c["B"])]
    cu = np.concatenate([[0], np.cumsum(c["lens"])])
    out = []
    for b, n in enumerate(c["lens"]):
        n = min(n, c["S"])
        out.append((b, int(cu[b]), n, n if c["qlim"] is None else min(c["qlim"][b], n)))
    return out


def key_live(c, b, lo, n):
    if c["mask"] is None:
        return torch.ones(n, dtype=torch.bool)
    return (c["mask"][b] if c["lens"] is None else c["mask"][lo:lo + n]) != 0


def offsets(c):
    """The launch's seq_offsets / q_offsets (int32 [B+1]) or None."""
    cu = None if c["lens"] is None else torch.tensor(np.concatenate([[0], np.cumsum(c["lens"])]), dtype=torch.int32)
    qo = None if c["qlim"] is None else torch.tensor(np.concatenate([[0], np.cumsum(c["qlim"])]), dtype=torch.int32)
    return cu, qo


def owned(c):
    """Which rows the kernels write: out / dq rows (queries), dk / dv rows (keys), lse entries; and the lse entries compared
    (those of a sequence with no unmasked key are -2^100-sized in the kernel, finfo.min-sized in eager: only finite)."""
    q = torch.zeros(c["T"], dtype=torch.bool)
    kv = torch.zeros(c["T"], dtype=torch.bool)
    lse = torch.zeros(c["B"], c["NH"], c["S"], dtype=torch.bool)
    lse_cmp = torch.zeros_like(lse)
    for b, lo, n, nq in sequences(c):
        q[lo:lo + nq] = True
        kv[lo:lo + n] = True
        lse[b, :, :nq] = True
        if n and bool(key_live(c, b, lo, n).any()):
            lse_cmp[b, :, :nq] = True
    return dict(q=q, kv=kv, lse=lse, lse_cmp=lse_cmp)


# ------------------------------------------------------------------ reference
def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """mode "r64": the float64 reference and its bounds E_*; "r32": the same in float32; "r16": float32 with the kernels'
    bf16 rounding points. Tensors in the kernels' layouts, zero where nothing is written (lse: NaN)."""
    c = CASES[name]
    dt = torch.float64 if mode == "r64" else torch.float32
    NH, S, T, p, scale = c["NH"], c["S"], c["T"], c["p"], c["scale"]
    H = NH * 64
    qkv, dout = inputs(name)
    qkv, dout = qkv.to(dt), dout.to(dt)
    res = {k: torch.zeros(T, H, dtype=dt) for k in ("out", "dq", "dk", "dv")}
    res["lse"] = torch.full((c["B"], NH, S), float("nan"), dtype=dt)
    if mode == "r64":
        res.update({"E_" + k: torch.zeros(T, H, dtype=dt) for k in ("out", "dq", "dk", "dv")})
    inv_keep = 1.0 / (1.0 - float(np.float32(p)))     # (the launchers take p as a C float)
    for b, lo, n, nq in sequences(c):
        if n == 0 or nq == 0:
            continue
        live = key_live(c, b, lo, n)
        for h in range(NH):
            cs = slice(h * 64, h * 64 + 64)
            q, dO = qkv[lo:lo + nq, cs], dout[lo:lo + nq, cs]
            k, v = qkv[lo:lo + n, H + h * 64: H + h * 64 + 64], qkv[lo:lo + n, 2 * H + h * 64: 2 * H + h * 64 + 64]
            keep = torch.ones(nq, n, dtype=dt)
            if p > 0:
                keep = torch.from_numpy(do.attention_keep(b, h, NH, S, nq, n, c["seed"], p)).to(dt)
            if bool(live.any()):
                s = (q @ k.T) * scale
                s[:, ~live] = -math.inf
            else:
                s = torch.zeros(nq, n, dtype=dt)
            m = s.max(-1, keepdim=True).values
            e = torch.exp(s - m)
            l = e.sum(-1, keepdim=True)
            lse = m + torch.log(l)
            res["lse"][b, h, :nq] = lse[:, 0]
            if mode == "r16":
                # the forward in 64-key tiles with a running maximum (P is rounded relative to the maximum SO FAR)
                m = torch.full((nq, 1), -1e30, dtype=dt)
                l, o = torch.zeros(nq, 1, dtype=dt), torch.zeros(nq, 64, dtype=dt)
                for t0 in range(0, n, 64):
                    st = s[:, t0:t0 + 64]
                    m_new = torch.maximum(m, st.max(-1, keepdim=True).values)
                    alpha = torch.exp(m - m_new)
                    e = torch.exp(st - m_new)
                    l = l * alpha + e.sum(-1, keepdim=True)
                    o = o * alpha + _bf(e * keep[:, t0:t0 + 64]) @ v[t0:t0 + 64]
                    m = m_new
                O = _bf(o / l * inv_keep)
                lse = m + torch.log(l)
                res["lse"][b, h, :nq] = lse[:, 0]
                P = torch.exp(s - lse)
                delta = (dO * O).sum(-1, keepdim=True)
                dV = _bf((_bf(P * keep).T @ dO) * inv_keep)
                dS = _bf(P * ((dO @ v.T) * keep - delta / inv_keep))
                dQ = _bf((dS @ k) * (scale * inv_keep))
                dK = _bf((dS.T @ q) * (scale * inv_keep))
            else:
                P = e / l
                Pd = P * keep * inv_keep
                O = Pd @ v
                dV = Pd.T @ dO
                dP = (dO @ v.T) * keep * inv_keep
                dS = P * (dP - (dO * O).sum(-1, keepdim=True))
                dQ = scale * (dS @ k)
                dK = scale * (dS.T @ q)
            res["out"][lo:lo + nq, cs], res["dq"][lo:lo + nq, cs] = O, dQ
            res["dk"][lo:lo + n, cs], res["dv"][lo:lo + n, cs] = dK, dV
            if mode == "r64":
                E_O = U * (O.abs() + Pd @ v.abs())
                d = (dO.abs() * E_O).sum(-1, keepdim=True)
                W = U * dS.abs() + P * d
                res["E_out"][lo:lo + nq, cs] = E_O
                res["E_dv"][lo:lo + n, cs] = U * (dV.abs() + Pd.T @ dO.abs())
                res["E_dq"][lo:lo + nq, cs] = U * dQ.abs() + scale * (W @ k.abs())
                res["E_dk"][lo:lo + n, cs] = U * dK.abs() + scale * (W.T @ q.abs())
    return res


def r16_as_kernel_output(name):
    """r16 in the form the kernels leave their outputs (bf16, the sentinels where nothing is written): what the CPU
    self-check feeds check_case() in place of a kernel's result."""
    c = CASES[name]
    r16, own = reference(name, "r16"), owned(c)
    H = c["NH"] * 64
    out = torch.where(own["q"][:, None], r16["out"], torch.full_like(r16["out"], OUT_SENTINEL)).to(torch.bfloat16)
    dqkv = torch.cat([r16["dq"], r16["dk"], r16["dv"]], 1).to(torch.bfloat16)
    assert dqkv.shape == (c["T"], 3 * H)
    return dict(out=out, lse=r16["lse"].clone(), dqkv=dqkv)


# ------------------------------------------------------------------ the check
def check_case(name, got):
    """got: out bf16 [T, H] (prefilled with OUT_SENTINEL), lse fp32 [B, NH, S] (prefilled with NaN), dqkv bf16 [T, 3H]
    (prefilled with 0), on the CPU. Every output of the case against r: per element, per block, sentinels, finiteness."""
    c = CASES[name]
    H = c["NH"] * 64
    r, r32, r16, own = reference(name, "r64"), reference(name, "r32"), reference(name, "r16"), owned(c)
    fails = []
    out, lse, dqkv = got["out"], got["lse"], got["dqkv"]
    assert out.dtype == torch.bfloat16 and dqkv.dtype == torch.bfloat16 and lse.dtype == torch.float32
    assert out.shape == (c["T"], H) and dqkv.shape == (c["T"], 3 * H) and lse.shape == (c["B"], c["NH"], c["S"])
    # rows that no sequence or query limit owns keep what they were prefilled with
    if not bool((out[~own["q"]].float() == OUT_SENTINEL).all()):
        fails.append("out: a row that is no query was written")
    if not bool((dqkv[~own["q"], :H].float() == 0).all()):
        fails.append("dq: a row that is no query was written")
    if not bool((dqkv[~own["kv"], H:].float() == 0).all()):
        fails.append("dk/dv: a row outside every sequence was written")
    if not bool(torch.isnan(lse[~own["lse"]]).all()):
        fails.append("lse: an entry that is no query was written")
    for t, what in ((out[own["q"]], "out"), (dqkv, "dqkv"), (lse[own["lse"]], "lse")):
        if not bool(torch.isfinite(t.float()).all()):
            fails.append(f"{what}: not finite")
    # lse of the sequences with a live key: parity_util.check_f32's rule, |got - r| <= A
    lr, lg = r["lse"][own["lse_cmp"]], lse[own["lse_cmp"]].double()
    e32, a = tol_a(r32["lse"][own["lse_cmp"]], lr)
    err = float(torch.nan_to_num((lg - lr).abs(), nan=math.inf).max()) if lr.numel() else 0.0
    _report(f"attn.{name}.lse", "f32", e32, a, err, err / a if a > 0 else 0.0)
    if err > a:
        fails.append(f"lse: max |got - r| = {err:.3e} > A = {a:.3e}")
    figures = {}
    for key, g, rows_of in (("out", out, "q"), ("dq", dqkv[:, :H], "q"), ("dk", dqkv[:, H:2 * H], "kv"), ("dv", dqkv[:, 2 * H:], "kv")):
        g = g.double()
        e32, a = tol_a(r32[key], r[key])
        diff = torch.nan_to_num((g - r[key]).abs(), nan=math.inf, posinf=math.inf)
        bound = r["E_" + key] + a
        m = own[rows_of]
        share = float((diff[m] / bound[m]).max()) if bool(m.any()) and a > 0 else float((diff > bound).any())
        bad = (diff > bound) & m[:, None]
        # per (sequence, head) block of at least 64 rows with a reference that is not identically zero
        worst, worst_blk, nblk = 0.0, None, 0
        for b, lo, n, nq in sequences(c):
            rows = nq if rows_of == "q" else n
            if rows < 64 or (rows_of == "kv" and nq == 0):
                continue
            for h in range(c["NH"]):
                blk = (slice(lo, lo + rows), slice(h * 64, h * 64 + 64))
                rn = float(r[key][blk].norm())
                if rn == 0.0:
                    continue
                nblk += 1
                kr = float(diff[blk].norm()) / rn
                rr = float((r16[key][blk].double() - r[key][blk]).norm()) / rn
                ratio = kr / rr if rr > 0 else (0.0 if kr == 0 else math.inf)
                if ratio > worst:
                    worst, worst_blk = ratio, (b, h, kr, rr)
                if kr > 2.0 * rr:
                    fails.append(f"{key}: block (sequence {b}, head {h}): ||got - r|| / ||r|| = {kr:.3e} > 2 x r16's {rr:.3e}")
        figures[key] = (share, worst)
        print(f"PARITY attn.{name}.{key} [bf16] e32={e32:.3e} A={a:.3e} max_err={float(diff[m].max()) if bool(m.any()) else 0.0:.3e} "
              f"share_of_E+A={share:.3f} blocks={nblk} worst_block_vs_r16={worst:.3f}"
              + (f" (sequence {worst_blk[0]}, head {worst_blk[1]}: {worst_blk[2]:.3e} vs {worst_blk[3]:.3e})" if worst_blk else ""))
        if bool(bad.any()):
            i = int(torch.argmax(torch.where(bad, diff / bound, torch.zeros_like(diff))))
            fails.append(f"{key}: {int(bad.sum())} of {int(m.sum()) * H} elements outside E + A (A = {a:.3e}); worst at row "
                         f"{i // H}, column {i % H}: |got - r| = {float(diff.flatten()[i]):.3e}, E + A = {float(bound.flatten()[i]):.3e}")
    assert not fails, f"{name}:\n  " + "\n  ".join(fails)
    return figures
