"""Reference, bounds and cases of the block-sparse attention tests (test_bigbird_attention_gpu.py, test_bigbird_ref_cpu.py),
in the manner of tests/attention_ref.py.

Reference r: per sequence, head and 64-row query block i with its list of (key block j, multiplicity m) entries, in
float64 on the CPU from the same bf16 inputs. K_i, V_i: the listed blocks' keys concatenated; w: m per key of an entry:

    s = q K_i^T * scale + bias     e = w o exp(s - max)     l = sum e     P = exp(s - max) / l     Pd = w o P
    O = Pd V_i     lse = max + log l     dV_i += Pd^T dO     dS = Pd o (dO V_i^T - rowsum(dO o O))
    dQ = scale * dS K_i            dK_i += scale * dS^T q

A masked key has P = 0 exactly; a block whose listed keys are ALL masked attends uniformly over them, weighted by
multiplicity (s = 0). No dropout: attention_ref's bounds with Pd := m P and p = 0 (u = 2^-8; P to bf16 before P.V and
P^T.dO, dS to bf16 before dS.K and dS^T.Q, the bf16 stores, delta from the stored bf16 O; dK / dV are summed over the
query blocks in fp32 and rounded once):

    E_O  = u (|O| + Pd |V_i|)           d = sum_d |dO| E_O           W = u |dS| + Pd o d
    E_dV = u (|dV| + sum_i Pd^T |dO|)   E_dQ = u |dQ| + scale W |K_i|     E_dK = u |dK| + scale sum_i W^T |q|

Every element must satisfy |got - r| <= E + A, A = parity_util.tol_a(r32, r), r32 the same computation in float32. lse is
within A where a listed key is live, only finite elsewhere. Per (sequence, head) block: ||got - r|| / ||r|| <= 2 ||r16 - r||
/ ||r||, r16 the float32 computation with the kernels' rounding points AND their tile order: a workgroup's waves split every
64-key tile into two 32-key halves, each half runs its own online softmax over the list in list order (m P rounded to bf16
relative to the maximum so far), and the two are merged at the end.

check_case() prints one PARITY line per output before it asserts (run with -s; profiles/bigbird_attention.md collects them).
"""
import functools
import math

import torch

from stonkgs_amd.bigbird_attention import BlockSparsePlan, bigbird_rand_attn
from tests.parity_util import _report, gen, tol_a

U = 2.0 ** -8
OUT_SENTINEL = 7.0
BLK = 64


# ------------------------------------------------------------------ cases
def _tail_mask(B, S, b, holes=((70, 90),), tail=100):
    m = torch.ones(B, S, dtype=torch.long)
    for lo, hi in holes:
        m[b, lo:hi] = 0
    m[b, S - tail:] = 0
    return m


def _case(name, B, NH, S, r, mode, data_seed, mask=None, plan_seed=0, exact=False, scale=0.125):
    return dict(name=name, B=B, NH=NH, S=S, nb=S // BLK, T=B * S, r=r, mode=mode, plan_seed=plan_seed, data_seed=data_seed,
                mask=mask, exact=exact, scale=scale)


def _build_cases():
    cs = [
        _case("s384-drawn", 2, 2, 384, 3, "train", 11, plan_seed=5),
        _case("s384-mask", 2, 2, 384, 3, "train", 12, plan_seed=5, mask=_tail_mask(2, 384, 1)),
        _case("s320-r1", 1, 2, 320, 1, "train", 13, plan_seed=6),
        _case("s768-eval", 1, 2, 768, 3, "eval", 14, mask=_tail_mask(1, 768, 0, holes=())),
        _case("s384-r0", 1, 1, 384, 0, "train", 16),
        _case("s4096-eval", 1, 1, 4096, 3, "eval", 17, mask=_tail_mask(1, 4096, 0, holes=(), tail=1000)),
        _case("s4096-drawn", 1, 1, 4096, 3, "train", 18, plan_seed=7, mask=_tail_mask(1, 4096, 0, holes=(), tail=1000)),
        _case("exact-s512-drawn", 1, 2, 512, 3, "train", 19, plan_seed=8, exact=True),
        _case("exact-s512-eval", 1, 2, 512, 3, "eval", 19, exact=True),
    ]
    m = torch.ones(2, 384, dtype=torch.long)
    m[0, :] = 0      # sequence 0: no unmasked key at all
    m[1, 200:230] = 0
    cs.insert(4, _case("s384-nokey", 2, 1, 384, 3, "train", 15, plan_seed=9, mask=m))
    return {c["name"]: c for c in cs}


CASES = _build_cases()


@functools.lru_cache(maxsize=None)
def plan(name):
    c = CASES[name]
    return BlockSparsePlan(c["nb"], bigbird_rand_attn(c["nb"], c["r"], c["NH"], c["mode"], seed=c["plan_seed"]))


def entries(lists, prefix, h, a):
    """[(block, multiplicity)] of row (h, a) of the forward ("key") or inverse ("query") lists."""
    n = int(lists[prefix + "_count"][h, a])
    return [(int(lists[prefix + "_blocks"][h, a, e]), int(lists[prefix + "_mult"][h, a, e])) for e in range(n)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """qkv bf16 [T, 3H] and dout bf16 [T, H], made on the CPU with a seeded generator. An `exact` case has q = 0 and
    V[key, c] = 1 if c == key // 64 else 0, so that out[row, c] is the probability mass on key block c."""
    c = CASES[name]
    H = c["NH"] * 64
    g = gen(c["data_seed"])
    qkv = (torch.randn(c["T"], 3 * H, generator=g) * 1.5).to(torch.bfloat16)
    dout = torch.randn(c["T"], H, generator=g).to(torch.bfloat16)
    if c["exact"]:
        qkv[:, :H] = 0
        v = torch.zeros(c["S"], 64)
        v[torch.arange(c["S"]), torch.arange(c["S"]) // BLK] = 1
        qkv[:, 2 * H:] = v.repeat(c["B"], c["NH"]).to(torch.bfloat16)
    return qkv, dout


def key_live(c, b):
    return torch.ones(c["S"], dtype=torch.bool) if c["mask"] is None else c["mask"][b] != 0


def lse_compared(c, lists):
    """[B, NH, S] bool: the lse entries compared with r - those of the blocks with a live listed key."""
    cmp = torch.zeros(c["B"], c["NH"], c["S"], dtype=torch.bool)
    for b in range(c["B"]):
        live = key_live(c, b).view(c["nb"], BLK).any(-1)
        for h in range(c["NH"]):
            for i in range(c["nb"]):
                cmp[b, h, i * BLK:(i + 1) * BLK] = any(bool(live[j]) for j, _ in entries(lists, "key", h, i))
    return cmp


# ------------------------------------------------------------------ reference
def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _forward_r16(s, ent, v, dt):
    """The kernels' forward for one query block: s [64, 64 n] (masked keys at -1e30: finite, as the kernels' -2^100 is), two
    32-key streams per tile, merged. Returns O (unrounded) and lse."""
    nq = s.shape[0]
    parts = []
    for kh in range(2):
        m = torch.full((nq, 1), -1e30, dtype=dt)
        l, o = torch.zeros(nq, 1, dtype=dt), torch.zeros(nq, 64, dtype=dt)
        for e, (j, mu) in enumerate(ent):
            cols = slice(e * BLK + kh * 32, e * BLK + kh * 32 + 32)
            st = s[:, cols]
            m_new = torch.maximum(m, st.max(-1, keepdim=True).values)
            alpha = torch.exp(m - m_new)
            ex = torch.exp(st - m_new)
            l = l * alpha + mu * ex.sum(-1, keepdim=True)
            o = o * alpha + _bf(mu * ex) @ v[cols]
            m = m_new
        parts.append((m, l, o))
    (m0, l0, o0), (m1, l1, o1) = parts
    mf = torch.maximum(m0, m1)
    a0, a1 = torch.exp(m0 - mf), torch.exp(m1 - mf)
    l = l0 * a0 + l1 * a1
    return (o0 * a0 + o1 * a1) / l, mf + torch.log(l)


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """compute() for a case of the table (made once, shared by the tests, never modified)."""
    return compute(CASES[name], plan(name).lists, *inputs(name), mode)


def compute(c, lists, qkv, dout, mode):
    """mode "r64": the float64 reference and its bounds E_*; "r32": the same in float32; "r16": float32 with the kernels'
    bf16 rounding points and tile order. c: B, NH, S, nb, T, scale, mask; qkv bf16 [T, 3H], dout bf16 [T, H]. Tensors in the
    kernels' layouts."""
    dt = torch.float64 if mode == "r64" else torch.float32
    NH, S, T, nb, scale = c["NH"], c["S"], c["T"], c["nb"], c["scale"]
    H = NH * 64
    qkv, dout = qkv.to(dt), dout.to(dt)
    res = {k: torch.zeros(T, H, dtype=dt) for k in ("out", "dq", "dk", "dv")}
    res["lse"] = torch.full((c["B"], NH, S), float("nan"), dtype=dt)
    if mode == "r64":
        res.update({"E_" + k: torch.zeros(T, H, dtype=dt) for k in ("out", "dq", "dk", "dv")})
    for b in range(c["B"]):
        lo = b * S
        live_all = key_live(c, b)
        for h in range(NH):
            cs = slice(h * 64, h * 64 + 64)
            K, V = qkv[lo:lo + S, H + h * 64: H + h * 64 + 64], qkv[lo:lo + S, 2 * H + h * 64: 2 * H + h * 64 + 64]
            dK, dV = torch.zeros(S, 64, dtype=dt), torch.zeros(S, 64, dtype=dt)
            eK, eV = torch.zeros(S, 64, dtype=dt), torch.zeros(S, 64, dtype=dt)
            for i in range(nb):
                ent = entries(lists, "key", h, i)
                rows = slice(lo + i * BLK, lo + (i + 1) * BLK)
                idx = torch.cat([torch.arange(j * BLK, (j + 1) * BLK) for j, _ in ent])
                w = torch.tensor([float(mu) for _, mu in ent], dtype=dt).repeat_interleave(BLK)[None, :]
                q, dO = qkv[rows, cs], dout[rows, cs]
                k, v = K[idx], V[idx]
                live = live_all[idx]
                degenerate = not bool(live.any())
                if degenerate:
                    s = torch.zeros(BLK, idx.numel(), dtype=dt)
                else:
                    s = (q @ k.T) * scale
                    s[:, ~live] = -math.inf
                mx = s.max(-1, keepdim=True).values
                ex = torch.exp(s - mx)
                l = (w * ex).sum(-1, keepdim=True)
                lse = mx + torch.log(l)
                if mode == "r16":
                    O, lse = _forward_r16(torch.nan_to_num(s, neginf=-1e30), ent, v, dt)
                    O = _bf(O)
                    if degenerate:
                        lse = torch.log(w.sum(-1, keepdim=True)).expand(BLK, 1)
                    P = torch.exp(s - lse)
                    delta = (dO * O).sum(-1, keepdim=True)
                    dV.index_add_(0, idx, _bf(w * P).T @ dO)
                    dS = _bf(w * P * (dO @ v.T - delta))
                    dQ = _bf((dS @ k) * scale)
                    dK.index_add_(0, idx, dS.T @ q)
                else:
                    P = ex / l
                    Pd = w * P
                    O = Pd @ v
                    dV.index_add_(0, idx, Pd.T @ dO)
                    dS = Pd * (dO @ v.T - (dO * O).sum(-1, keepdim=True))
                    dQ = scale * (dS @ k)
                    dK.index_add_(0, idx, dS.T @ q)
                res["out"][rows, cs], res["dq"][rows, cs] = O, dQ
                res["lse"][b, h, i * BLK:(i + 1) * BLK] = lse[:, 0]
                if mode == "r64":
                    E_O = U * (O.abs() + Pd @ v.abs())
                    d = (dO.abs() * E_O).sum(-1, keepdim=True)
                    W = U * dS.abs() + Pd * d
                    res["E_out"][rows, cs] = E_O
                    res["E_dq"][rows, cs] = U * dQ.abs() + scale * (W @ k.abs())
                    eV.index_add_(0, idx, Pd.T @ dO.abs())
                    eK.index_add_(0, idx, W.T @ q.abs())
            dK = dK * scale
            if mode == "r16":
                dK, dV = _bf(dK), _bf(dV)
            res["dk"][lo:lo + S, cs], res["dv"][lo:lo + S, cs] = dK, dV
            if mode == "r64":
                res["E_dk"][lo:lo + S, cs] = U * dK.abs() + scale * eK
                res["E_dv"][lo:lo + S, cs] = U * (dV.abs() + eV)
    return res


def r16_as_kernel_output(name):
    """r16 in the form the kernels leave their outputs: what the CPU self-check feeds check_case() in a kernel's place."""
    r16 = reference(name, "r16")
    return dict(out=r16["out"].to(torch.bfloat16), lse=r16["lse"].clone(),
                dqkv=torch.cat([r16["dq"], r16["dk"], r16["dv"]], 1).to(torch.bfloat16))


# ------------------------------------------------------------------ the check
def check_case(name, got, **kw):
    """check() for a case of the table."""
    refs = tuple(reference(name, mode) for mode in ("r64", "r32", "r16"))
    return check(CASES[name], plan(name).lists, refs, got, name=name, **kw)


def check(c, lists, refs, got, name, label="bigbird", rows=None, keys=("out", "dq", "dk", "dv")):
    """got: out bf16 [T, H], lse fp32 [B, NH, S], dqkv bf16 [T, 3H], on the CPU (lse / dqkv optional when `keys` leaves them
    out); refs: compute()'s r64, r32, r16. Every output against r: per element, per (sequence, head) block, finiteness.
    `rows` (bool [T], default all) restricts the comparison of out / dq to those query rows (the module test: the rows whose
    own mask is 1, where the list semantics ARE HuggingFace's)."""
    H = c["NH"] * 64
    r, r32, r16 = refs
    fails, figures = [], {}
    rows_q = torch.ones(c["T"], dtype=torch.bool) if rows is None else rows
    if "lse" in got:
        lse = got["lse"]
        assert lse.dtype == torch.float32 and lse.shape == (c["B"], c["NH"], c["S"])
        if not bool(torch.isfinite(lse).all()):
            fails.append("lse: not finite")
        cmp = lse_compared(c, lists)
        lr, lg = r["lse"][cmp], lse[cmp].double()
        e32, a = tol_a(r32["lse"][cmp], lr)
        err = float(torch.nan_to_num((lg - lr).abs(), nan=math.inf).max()) if lr.numel() else 0.0
        _report(f"{label}.{name}.lse", "f32", e32, a, err, err / a if a > 0 else 0.0)
        if err > a:
            fails.append(f"lse: max |got - r| = {err:.3e} > A = {a:.3e}")
    tensors = {"out": got["out"]}
    if "dqkv" in got:
        assert got["dqkv"].dtype == torch.bfloat16 and got["dqkv"].shape == (c["T"], 3 * H)
        tensors.update(dq=got["dqkv"][:, :H], dk=got["dqkv"][:, H:2 * H], dv=got["dqkv"][:, 2 * H:])
    assert got["out"].dtype == torch.bfloat16 and got["out"].shape == (c["T"], H)
    for key in keys:
        g = tensors[key].double()
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{key}: not finite")
        e32, a = tol_a(r32[key], r[key])
        diff = torch.nan_to_num((g - r[key]).abs(), nan=math.inf, posinf=math.inf)
        bound = r["E_" + key] + a
        m = rows_q if key in ("out", "dq") else torch.ones(c["T"], dtype=torch.bool)
        over = torch.where(diff[m] > 0, torch.full_like(diff[m], math.inf), torch.zeros_like(diff[m]))   # (a bound of exactly 0)
        share = float(torch.where(bound[m] > 0, diff[m] / bound[m], over).max())
        bad = (diff > bound) & m[:, None]
        worst, worst_blk, nblk = 0.0, None, 0
        for b in range(c["B"]):
            for h in range(c["NH"]):
                mb = m[b * c["S"]:(b + 1) * c["S"]]
                blk = (slice(b * c["S"], (b + 1) * c["S"]), slice(h * 64, h * 64 + 64))
                rn = float(r[key][blk][mb].norm())
                if rn == 0.0:
                    continue
                nblk += 1
                kr = float(diff[blk][mb].norm()) / rn
                rr = float((r16[key][blk].double() - r[key][blk])[mb].norm()) / rn
                ratio = kr / rr if rr > 0 else (0.0 if kr == 0 else math.inf)
                if ratio > worst:
                    worst, worst_blk = ratio, (b, h, kr, rr)
                if kr > 2.0 * rr:
                    fails.append(f"{key}: block (sequence {b}, head {h}): ||got - r|| / ||r|| = {kr:.3e} > 2 x r16's {rr:.3e}")
        figures[key] = (share, worst)
        print(f"PARITY {label}.{name}.{key} [bf16] e32={e32:.3e} A={a:.3e} max_err={float(diff[m].max()):.3e} "
              f"share_of_E+A={share:.3f} blocks={nblk} worst_block_vs_r16={worst:.3f}"
              + (f" (sequence {worst_blk[0]}, head {worst_blk[1]}: {worst_blk[2]:.3e} vs {worst_blk[3]:.3e})" if worst_blk else ""))
        if bool(bad.any()):
            i = int(torch.argmax(torch.where(bad, diff / bound, torch.zeros_like(diff))))
            fails.append(f"{key}: {int(bad.sum())} of {int(m.sum()) * H} elements outside E + A (A = {a:.3e}); worst at row "
                         f"{i // H}, column {i % H}: |got - r| = {float(diff.flatten()[i]):.3e}, E + A = {float(bound.flatten()[i]):.3e}")
    assert not fails, f"{name}:\n  " + "\n  ".join(fails)
    return figures


def exact_masses(name):
    """For an `exact` case: want [T, NH, nb] float64 (the mass m / L of every key block for every query row and head) and
    pow2 [T, NH] bool (rows whose total multiplicity L is a power of two)."""
    c = CASES[name]
    lists = plan(name).lists
    want = torch.zeros(c["T"], c["NH"], c["nb"], dtype=torch.float64)
    pow2 = torch.zeros(c["T"], c["NH"], dtype=torch.bool)
    for b in range(c["B"]):
        for h in range(c["NH"]):
            for i in range(c["nb"]):
                ent = entries(lists, "key", h, i)
                L = sum(mu for _, mu in ent)
                rows = slice(b * c["S"] + i * BLK, b * c["S"] + (i + 1) * BLK)
                for j, mu in ent:
                    want[rows, h, j] = mu / L
                pow2[rows, h] = (L & (L - 1)) == 0
    return want, pow2
