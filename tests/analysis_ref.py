"""References, case tables and launch geometry of the evaluation / analysis kernels for tests/test_analysis_parity_gpu.py:
row-wise top-k (csrc/topk.hip), input attributions (csrc/input_attribution.hip), attention probabilities
(csrc/attention_probs.hip), the word-table gradient (csrc/text_embed.hip) and the row movers of csrc/loss.hip.
tests/test_analysis_ref_cpu.py pins all of it without a GPU. CPU only: nothing here imports the package.

Every case is there for one branch of a kernel, named in its comment. The branch is taken or not according to constants of
the launchers (grid caps, positions per workgroup, which instantiation a k selects); `geometry()` reads those out of the
launchers' own source lines, so that a launcher edited without its case fails the CPU file by name.

References are the operation itself in float64 on the same bf16 / fp16 / fp32 inputs; the float32 twins (`r32`) give
tests/parity_util.py its e32. Inputs come from seeded CPU generators and are the same on every machine.
"""
import os
import re

import numpy as np
import torch

from oracle.masking_oracle import unpad_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stonkgs_amd", "csrc")
BF16 = torch.bfloat16
NEG_INF = float("-inf")


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# launch geometry, from the launchers' source
# ---------------------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the launcher's line is not what tests/analysis_ref.py reads - re-read it and re-size the case"
    return m


_GEOMETRY = None


def geometry():
    """The constants the cases are sized by: {name: int}, and `kc_chain` = [(largest k, KC)] in the launcher's order."""
    global _GEOMETRY
    if _GEOMETRY is not None:
        return _GEOMETRY
    g = {}
    topk = _src("topk.hip")
    g["topk_cap"] = int(_find(r"grid_cap\(cap_rows, 1, (\d+)\)", topk, "topk grid cap").group(1))
    g["topk_sweep"] = 8 * int(_find(r"for \(int i0 = 0; i0 < n8; i0 \+= (\d+)\)", topk, "topk sweep").group(1))
    chain = [(int(k), int(kc)) for _, k, kc in re.findall(r"if \(k (==|<=) (\d+)\) STONK_TOPK_LAUNCH\((\d+)\);", topk)]
    last = int(_find(r"\n\s*else STONK_TOPK_LAUNCH\((\d+)\);", topk, "topk instance chain").group(1))
    limit = int(_find(r"k >= 1 && k <= (\d+) && k <= ncols", topk, "topk k limit").group(1))
    g["kc_chain"] = chain + [(limit, last)]
    att = _src("input_attribution.hip")
    m = _find(r"const long g = \(npos \+ (\d+)\) / (\d+);", att, "attribution positions per workgroup")
    assert int(m.group(1)) + 1 == int(m.group(2))
    g["attr_per_block"] = int(m.group(2))
    m = _find(r"dim3\(\(unsigned\)\(g < (\d+) \? g : (\d+)\)\)", att, "attribution grid cap")
    assert m.group(1) == m.group(2)
    g["attr_cap"] = int(m.group(1))
    weg = _src("text_embed.hip")
    g["weg_cap"] = int(_find(r"grid_cap\(n_pos, WEG_WAVES, (\d+)\)", weg, "word-gradient grid cap").group(1))
    g["weg_per_block"] = int(_find(r"constexpr int WEG_WAVES = (\d+);", weg, "WEG_WAVES").group(1))
    g["weg_chunk"] = int(_find(r"constexpr int WEG_CHUNK = (\d+);", weg, "WEG_CHUNK").group(1))
    loss = _src("loss.hip")
    for name, kernel in (("gather", r"gather_rows_kernel"), ("scatter", r"scatter_rows_kernel<SrcT>")):
        m = _find(kernel + r", dim3\((\d+)\), dim3\((\d+)\)", loss, f"{name} grid")
        g[f"{name}_cap"], g[f"{name}_per_block"] = int(m.group(1)), int(m.group(2))
    g["gather_tile"] = int(_find(r"long lim = \(\(long\)\(cnt \+ 127\) / (\d+)\) \* (\d+);", loss, "gather clamp").group(1))
    g["compact_chunk"] = int(_find(r"constexpr int R = (\d+);", loss, "label compaction rounds").group(1)) * 1024
    probs = _src("attention_probs.hip")
    g["QB"] = int(_find(r"constexpr int QB = (\d+);", probs, "QB").group(1))
    g["probs_max_S"] = int(_find(r"S % 128 == 0 && S <= (\d+)", probs, "attention_probs S limit").group(1))
    g["TK"] = int(_find(r"constexpr int TK = (\d+);", _src("attn_tiles.h"), "TK").group(1))
    _GEOMETRY = g
    return g


def trips(work, cap, per_block):
    """Grid-stride trips of the busiest workgroup: ceil(work / (cap * per_block))."""
    return -(-work // (cap * per_block))


def kc_of(k):
    """The instantiation the top-k launcher picks for k."""
    for kmax, kc in geometry()["kc_chain"]:
        if k <= kmax:
            return kc
    raise AssertionError(k)


# ---------------------------------------------------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------------------------------------------------
TOPK_SENT = -7
TOPK_PAD = 1.0e4     # padding columns [ncols, ld): large and finite - must be ignored
# name -> (cap_rows, count, ncols, ld, ks). What each is there for:
#  trips      three grid-stride trips of the first count - 2 * cap workgroups; rows r, r + cap, r + 2 cap differ in kind and
#             level, so a list, a threshold or an LDS slot left over from the previous row changes ids, values or rank
#  instances  test_topk_gpu.py's `small` rows at the k that select KC = 4 and that sit on and just past every KC
#  special    -0.0 / +0.0, -inf, sorted rows, +-65504
#  sweep      a row longer than one 8192-column sweep whose best columns are its last
#  misaligned `small` again from a base pointer one element past a 16-byte boundary (the element-by-element sweep)
TOPK_CASES = {
    "trips": (4200, 4133, 40, 40, (1, 3, 8, 12, 16)),
    "instances": (40, 37, 300, 384, (2, 4, 8, 9, 12, 13)),
    "special": (16, 16, 300, 304, (1, 5, 16)),
    "sweep": (6, 5, 8200, 8200, (3, 16)),
    "misaligned": (40, 37, 300, 384, (5, 16)),
}
TRIP_LEVELS = (20.0, -20.0, 0.0)
_topk_cache = {}


def _kind_row(kind, ncols, g):
    if kind == 1:
        return torch.randint(-3, 4, (ncols,), generator=g).float()       # heavily tied
    if kind == 2:
        return torch.full((ncols,), 0.5)                                  # all equal
    row = torch.randn(ncols, generator=g) * 3.0
    if kind == 3:
        row[ncols - 1] = 50.0                                             # the maximum in the last valid column
    return row


def _f16_ramp(n, first_bits=0x3000):
    """n consecutive positive fp16 values (0.125 upwards): strictly ascending in fp16 and in fp32."""
    return torch.arange(first_bits, first_bits + n, dtype=torch.int32).to(torch.int16).view(torch.float16).float()


def topk_special_rows(ncols):
    """16 rows and their targets, and what each row is: {row: kind}."""
    g = gen(77)
    rows, tgt, kinds = [], [], {}

    def add(kind, row, t):
        kinds[len(rows)] = kind
        rows.append(row)
        tgt.append(t)

    sign = torch.where(torch.rand(ncols, generator=g) < 0.5, -1.0, 1.0)
    zeros = torch.zeros(ncols) * sign                                       # -0.0 and +0.0 mixed, nothing else
    neg = int((torch.signbit(zeros)).nonzero()[3])
    pos = int((~torch.signbit(zeros)).nonzero()[5])
    add("zeros", zeros.clone(), neg)                                        # the target on a -0.0
    add("zeros", zeros.clone(), pos)                                        # ... and on a +0.0 behind -0.0 columns
    mixed = -torch.rand(ncols, generator=g) * 4.0 - 0.5
    where = torch.randperm(ncols, generator=g)[:40]
    mixed[where] = zeros[where]                                             # 40 zeros of both signs above negatives
    add("zeros", mixed, int(where[7]))
    for n_fin, on_inf in ((16, True), (20, False), (17, False)):
        row = torch.full((ncols,), NEG_INF)
        cols = torch.randperm(ncols, generator=g)[:n_fin] if n_fin != 17 else torch.arange(ncols - 17, ncols)
        row[cols] = torch.randn(n_fin, generator=g) * 3.0 + 5.0
        inf_col = int((row == NEG_INF).nonzero()[11])
        add("neg_inf", row, inf_col if on_inf else int(cols[3]))
    ramp = _f16_ramp(ncols)
    add("ascending", ramp.clone(), 0)
    add("ascending", _f16_ramp(ncols, 0x4400), ncols - 1)                # (4.0 upwards)
    add("descending", ramp.flip(0).clone(), 0)
    add("descending", -ramp, ncols // 2)
    ext = torch.randn(ncols, generator=g) * 100.0
    ext[torch.randperm(ncols, generator=g)[:6]] = 65504.0
    ext[torch.randperm(ncols, generator=g)[:6]] = -65504.0
    add("extremes", ext, int((ext == 65504.0).nonzero()[2]))
    low = torch.full((ncols,), -65504.0)
    low[torch.randperm(ncols, generator=g)[:20]] = -65000.0 + torch.arange(20.0) * 32.0
    add("extremes", low, int((low == -65504.0).nonzero()[9]))
    add("zeros", -zeros, pos)
    both = torch.full((ncols,), NEG_INF)
    both[torch.randperm(ncols, generator=g)[:30]] = (torch.zeros(30) * torch.where(torch.rand(30, generator=g) < 0.5, -1.0, 1.0))
    add("neg_inf", both, int((both == 0).nonzero()[17]))                    # -inf below thirty zeros of both signs
    add("random", torch.randn(ncols, generator=g) * 3.0, 17)
    add("random", torch.randn(ncols, generator=g) * 3.0 + 9.0, ncols - 1)
    assert len(rows) == 16
    return torch.stack(rows), torch.tensor(tgt, dtype=torch.int32), kinds


def topk_trip_kind(r):
    """(kind, level) of row r of the `trips` case: both change with the trip r // cap."""
    trip = r // geometry()["topk_cap"]
    return (r + trip) % 4, TRIP_LEVELS[min(trip, 2)]


def topk_inputs(name, dtype):
    """(x [cap, ld] in `dtype`, targets int32 [cap]) on the CPU - built once per (case, dtype) and left unchanged."""
    key = (name, dtype)
    if key in _topk_cache:
        return _topk_cache[key]
    cap, count, ncols, ld, _ = TOPK_CASES[name]
    x = torch.full((cap, ld), TOPK_PAD)
    tgt = torch.zeros(cap, dtype=torch.int32)
    if name in ("instances", "misaligned"):          # test_topk_gpu.py's `small` rows
        g = gen(1234 + ncols)
        for r in range(cap):
            x[r, :ncols] = _kind_row(r % 5, ncols, g)
            tgt[r] = (0, ncols - 1, int(torch.randint(0, ncols, (1,), generator=g)))[r % 3]
    elif name == "trips":
        g = gen(4200)
        for r in range(cap):
            kind, level = topk_trip_kind(r)
            x[r, :ncols] = _kind_row(kind, ncols, g) + level
            tgt[r] = (0, ncols - 1, int(torch.randint(0, ncols, (1,), generator=g)))[r % 3]
    elif name == "special":
        rows, tgt, _ = topk_special_rows(ncols)
        x[:, :ncols] = rows
    elif name == "sweep":
        g = gen(8200)
        ramp = _f16_ramp(ncols)
        x[0, :ncols] = ramp                           # ascending across the sweep boundary: the best k are the last columns
        x[1, :ncols] = ramp.flip(0)                   # descending: nothing enters after the first k
        x[2, :ncols] = torch.randn(ncols, generator=g) * 3.0
        x[2, ncols - 3:ncols] = 40.0                  # three tied maxima behind the boundary
        x[3, :ncols] = NEG_INF
        x[3, geometry()["topk_sweep"] - 10:ncols] = ramp[:ncols - geometry()["topk_sweep"] + 10]   # finite only around the boundary
        x[4, :ncols] = torch.randint(-2, 3, (ncols,), generator=g).float()
        x[5, :ncols] = 3.0                            # (past the count)
        tgt = torch.tensor([ncols - 1, 0, ncols - 2, 5, geometry()["topk_sweep"], 0], dtype=torch.int32)
    else:
        raise KeyError(name)
    _topk_cache[key] = (x.to(dtype), tgt)
    return _topk_cache[key]


def topk_reference(x, tgt, count, ncols, variant=None):
    """The stated total order - larger value first, lower column first among equal values (-0.0 equals +0.0) - as a stable
    descending sort in float64; the rank of the target counted directly; the log-sum-exp in float64.
    `variant`: None | "ties_reversed" | "neg_zero_below" | "rank_ge" - one mistake each (test_analysis_ref_cpu.py)."""
    xs = x[:count, :ncols].double()
    key = xs
    if variant == "neg_zero_below":
        key = torch.where((xs == 0) & torch.signbit(xs), torch.full_like(xs, -1e-300), xs)
    if variant == "ties_reversed":
        _, si = torch.sort(key.flip(1), dim=1, descending=True, stable=True)
        si = ncols - 1 - si
    else:
        _, si = torch.sort(key, dim=1, descending=True, stable=True)
    sv = xs.gather(1, si)
    t = tgt[:count].long()[:, None]
    T = xs.gather(1, t)
    col = torch.arange(ncols)[None]
    if variant == "rank_ge":
        rank = (xs >= T).sum(1) - 1
    else:
        rank = (xs > T).sum(1) + ((xs == T) & (col < t)).sum(1)
    return dict(sv=sv[:, :16].float(), si=si[:, :16].int(), rank=rank.int(), tgt=T[:, 0].float(), lse=torch.logsumexp(xs, 1))


_topk_ref_cache = {}


def topk_expected(name, dtype):
    key = (name, dtype)
    if key not in _topk_ref_cache:
        cap, count, ncols, ld, _ = TOPK_CASES[name]
        x, tgt = topk_inputs(name, dtype)
        _topk_ref_cache[key] = topk_reference(x, tgt, count, ncols)
    return _topk_ref_cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# input attribution
# ---------------------------------------------------------------------------------------------------------------------
ATTR_SCALE = -19.0
ATTR_KG_ROWS = 333
# name -> B, S, half, H. Widths: 8 and 72 leave lanes idle in the only chunk of 64 lanes x 8 columns, 520 gives lane 0 alone
# a second chunk, 4096 is the largest the launcher accepts; `trips` has more positions than cap x 4; half = 0 / half = S
# put every position into one branch of the x lookup.
ATTR_CASES = {
    "H8": dict(B=2, S=128, half=64, H=8),
    "H72": dict(B=2, S=128, half=64, H=72),
    "H520": dict(B=2, S=128, half=64, H=520),
    "H4096": dict(B=2, S=128, half=64, H=4096),
    "trips": dict(B=33, S=512, half=256, H=64),
    "half0": dict(B=2, S=128, half=0, H=72),
    "halfS": dict(B=2, S=128, half=128, H=72),
}
ATTR_BAD_IDS = (-1, -(1 << 40), ATTR_KG_ROWS)     # entity ids outside the table: x counts as 0
_attr_cache = {}


def attr_plan(B, S, seed):
    """A mask with holes and labels through oracle.masking_oracle.unpad_plan: (row_of_pos int32 [B*S], attention mask).
    The plan puts a sequence's read rows (position 0, labelled positions) first: row_of_pos is not monotone."""
    g = gen(seed)
    h = S // 2
    am = torch.zeros(B, S, dtype=torch.int64)
    for b in range(B):
        nt = int(torch.randint(h // 4, h + 1, (1,), generator=g))
        ne = int(torch.randint(h // 4, h + 1, (1,), generator=g))
        am[b, :nt] = 1
        am[b, h:h + ne] = 1
        am[b, torch.randint(1, S, (6,), generator=g)] = 0          # holes (and some already dead)
    am[0, S - 4:] = 1                                              # (the out-of-table ids sit here: kept)
    lab = torch.full((B, S), -100, dtype=torch.int64)
    pick = torch.rand(B, S, generator=g) < 0.15
    lab[pick] = 5
    plan = unpad_plan(am.numpy(), lab[:, :h].numpy(), lab[:, h:].numpy())
    return torch.from_numpy(np.asarray(plan[0], dtype=np.int32)), am


def attr_inputs(name):
    if name in _attr_cache:
        return _attr_cache[name]
    c = ATTR_CASES[name]
    B, S, half, H = c["B"], c["S"], c["half"], c["H"]
    g = gen(3000 + H + S + half)
    dsum = (torch.randn(B * S, H, generator=g) * 0.05).to(BF16)
    text = torch.randn(max(B * half, 1), H, generator=g).to(BF16)
    kg = torch.randn(ATTR_KG_ROWS, H, generator=g) * 0.3
    ids = torch.randint(0, ATTR_KG_ROWS, (B, S), generator=g)
    ids[0, S - 4:] = torch.tensor(ATTR_BAD_IDS + (ATTR_KG_ROWS - 1,))
    row_of_pos, am = attr_plan(B, S, 50 + H)
    _attr_cache[name] = dict(c, dsum=dsum, text=text, kg=kg, ids=ids, row_of_pos=row_of_pos, mask=am)
    return _attr_cache[name]


def attr_reference(name, layout, dtype=torch.float64):
    """g = scale * dsum[row of p] (0 on a dropped position), x = the row the forward read (0 for an id outside the table):
    dict(live, g, gxi = <g, x>, gn = |g|, gx = |g| |x|)."""
    c = attr_inputs(name)
    B, S, half, H = c["B"], c["S"], c["half"], c["H"]
    n = B * S
    rows = torch.arange(n) if layout == "padded" else c["row_of_pos"].long()
    live = rows >= 0
    gd = torch.zeros(n, H, dtype=dtype)
    gd[live] = torch.tensor(ATTR_SCALE, dtype=dtype) * c["dsum"][rows[live]].to(dtype)
    x = torch.zeros(B, S, H, dtype=dtype)
    if half > 0:
        x[:, :half] = c["text"][:B * half].to(dtype).view(B, half, H)
    if half < S:
        ids = c["ids"][:, half:]
        ok = (ids >= 0) & (ids < ATTR_KG_ROWS)
        x[:, half:] = c["kg"].to(dtype)[ids.clamp(0, ATTR_KG_ROWS - 1)] * ok[..., None].to(dtype)
    x = x.view(n, H)
    return dict(live=live, g=gd, gxi=(gd * x).sum(1), gn=gd.norm(dim=1), gx=gd.norm(dim=1) * x.norm(dim=1))


# ---------------------------------------------------------------------------------------------------------------------
# attention probabilities
# ---------------------------------------------------------------------------------------------------------------------
# name -> B, NH, S, half, scale, mask kind. s1024 / s4096: lengths no test reaches (4096 is the launcher's limit, 16 KiB of
# dynamic LDS for the key bias); grid9: nine workgroups - an odd grid through xcd_linear - and an uneven split;
# grid9-sparse: per sequence one live key / live keys in the last key tile only / in the first tile only.
PROBS_CASES = {
    "s1024": dict(B=1, NH=2, S=1024, half=192, scale=0.125, mask="holes"),
    "s4096": dict(B=1, NH=1, S=4096, half=2048, scale=0.125, mask="holes"),
    "grid9": dict(B=3, NH=1, S=384, half=64, scale=0.2, mask="holes"),
    "grid9-sparse": dict(B=3, NH=1, S=384, half=192, scale=0.2, mask="sparse"),
}
ONE_LIVE_KEY = 200      # the single live key of sequence 0 of grid9-sparse
_probs_cache = {}
_probs_ref_cache = {}


def probs_inputs(name):
    """q, k bf16 [B*S, NH*64] and the key mask int64 [B, S]."""
    if name in _probs_cache:
        return _probs_cache[name]
    c = PROBS_CASES[name]
    B, NH, S = c["B"], c["NH"], c["S"]
    g = gen(9000 + S + NH + len(name))
    q = torch.randn(B * S, NH * 64, generator=g).to(BF16)
    k = torch.randn(B * S, NH * 64, generator=g).to(BF16)
    mask = torch.ones(B, S, dtype=torch.int64)
    tk = geometry()["TK"]
    if c["mask"] == "holes":
        for b in range(B):
            mask[b, torch.randperm(S, generator=g)[:S // 16]] = 0       # about 6 % of the keys, anywhere
            mask[b, S - 5 - b:] = 0                                       # and a padded tail
    else:
        mask[:] = 0
        mask[0, ONE_LIVE_KEY] = 1
        mask[1, S - tk + torch.randperm(tk, generator=g)[:40]] = 1       # the last key tile only
        mask[2, torch.randperm(tk, generator=g)[:40]] = 1                # the first key tile only
    _probs_cache[name] = dict(c, q=q, k=k, key_mask=mask)
    return _probs_cache[name]


def probs_reference(name, dtype=torch.float64, score_factor=1.0, split=None):
    """(probabilities [B, NH, S, S], masses [B, NH, S, 2]) of softmax(q k^T scale) over the live keys in `dtype`; a masked key
    has probability 0 (every sequence of the cases has a live key). `score_factor`, `split`: the mistakes of
    test_analysis_ref_cpu.py (another log2(e), the masses split at another key)."""
    c = probs_inputs(name)
    B, NH, S = c["B"], c["NH"], c["S"]
    q = c["q"].to(dtype).view(B, S, NH, 64).permute(0, 2, 1, 3)
    k = c["k"].to(dtype).view(B, S, NH, 64).permute(0, 2, 1, 3)
    s = (q @ k.transpose(-1, -2)) * torch.tensor(c["scale"] * score_factor, dtype=dtype)
    s = s.masked_fill((c["key_mask"] == 0)[:, None, None, :], NEG_INF)
    p = torch.softmax(s, -1)
    half = c["half"] if split is None else split
    return p, torch.stack([p[..., :half].sum(-1), p[..., half:].sum(-1)], -1)


def probs_expected(name):
    """((p64, m64), (p32, m32)), computed once."""
    if name not in _probs_ref_cache:
        _probs_ref_cache[name] = (probs_reference(name, torch.float64), probs_reference(name, torch.float32))
    return _probs_ref_cache[name]


PROBS_FLOOR = 1e-6          # the relative bound is taken on elements with r64 above this
PROBS_REL_FACTOR = 8.0      # x the r32-vs-r64 maximum relative error of the same case (parity_util's factor, for its reason)


def probs_rel(p, p64):
    """Maximum relative error of p against p64 over the elements with p64 > PROBS_FLOOR."""
    big = p64 > PROBS_FLOOR
    return float(((p.double() - p64).abs()[big] / p64[big]).max())


# ---------------------------------------------------------------------------------------------------------------------
# word-embedding gradient
# ---------------------------------------------------------------------------------------------------------------------
# name -> B, S, H, vocab. 72: `col < H` inside a group of 64 lanes; 520: a second chunk with one live lane; 1024: two whole
# chunks; trips: more positions than cap x WEG_WAVES.
WEG_CASES = {
    "H72": dict(B=3, S=256, H=72, vocab=160),
    "H520": dict(B=3, S=256, H=520, vocab=160),
    "H1024": dict(B=3, S=256, H=1024, vocab=1000),
    "trips": dict(B=65, S=512, H=8, vocab=1000),
}
WEG_HOT, WEG_N_HOT = 7, 220
_weg_cache = {}


def weg_inputs(name, packed):
    """test_word_embed_grad_gpu.py's construction: a hot row, the padding id, the table's last row, guard rows around the
    table, strides wider than H with a value behind H that would show in every sum."""
    key = (name, packed)
    if key in _weg_cache:
        return _weg_cache[key]
    c = WEG_CASES[name]
    B, S, H, vocab = c["B"], c["S"], c["H"], c["vocab"]
    g = gen(H + vocab + 31 * packed)
    n = B * S
    ids = torch.randint(1, vocab - 1, (n,), generator=g)
    where = torch.randperm(n, generator=g)
    ids[where[:WEG_N_HOT]] = WEG_HOT
    ids[where[WEG_N_HOT:WEG_N_HOT + 12]] = 0
    ids[where[WEG_N_HOT + 12:WEG_N_HOT + 17]] = vocab - 1
    ids[n - 1] = vocab - 1                                  # the last position (of the last trip) lands in the last row
    row_of_pos = None
    if packed:
        row_of_pos = torch.randperm(n, generator=g).to(torch.int32)
        row_of_pos[torch.randperm(n, generator=g)[:n // 3]] = -1
        row_of_pos[n - 1] = 0
    ld, ld_w = H + 8, H + 5
    dsum = torch.zeros(n, ld, dtype=BF16)
    dsum[:, :H] = torch.randn(n, H, generator=g).to(BF16)
    dsum[:, H:] = 1000.0
    table = torch.randn(vocab + 2, ld_w, generator=g)       # rows 0 and vocab + 1: guards
    _weg_cache[key] = dict(c, ids=ids.view(B, S), row_of_pos=row_of_pos, dsum=dsum, table=table, ld=ld, ld_w=ld_w)
    return _weg_cache[key]


def weg_reference(c, padding_idx, dtype=torch.float64):
    """index_add_ in `dtype`: (sums, sums of absolute values, contributions per destination row)."""
    H, vocab = c["H"], c["vocab"]
    flat = c["ids"].reshape(-1)
    rows = torch.arange(flat.numel()) if c["row_of_pos"] is None else c["row_of_pos"].long()
    live = (rows >= 0) & (flat != padding_idx)
    contrib = c["dsum"][rows[live], :H].to(dtype)
    ref = c["table"][1:vocab + 1, :H].to(dtype).clone()
    mag = ref.abs()
    ref.index_add_(0, flat[live], contrib)
    mag.index_add_(0, flat[live], contrib.abs())
    return ref, mag, torch.bincount(flat[live], minlength=vocab)


# ---------------------------------------------------------------------------------------------------------------------
# row movers
# ---------------------------------------------------------------------------------------------------------------------
# gather / scatter: (source rows, moved rows `count`, cap, cols, ld_src, ld_dst). trips: more 16-byte pieces than the fixed
# grid has threads (count x cols / 8 for the scatters, lim x cols / 8 for the gather: lim = cap here, with zero-filled rows
# in the second trip). The small shapes: every (count, cap) of the clamp lim = min(roundup(count, 128), cap).
MOVER_TRIPS = dict(n_src=2300, count=2060, cap=2100, cols=1024, ld_src=1032, ld_dst=1048)
MOVER_SMALL = dict(n_src=300, cols=64, ld_src=72, ld_dst=80)
MOVER_COUNTS, MOVER_CAPS = (0, 128, 190), (190, 200, 256)
MOVER_FILL = 9.0
# label compaction: (B, half, S, labelled share): several chunks of 16 384 labels with a ragged last one; fewer than 1024
COMPACT_CASES = {"chunks": (70, 256, 520, 0.15), "short": (3, 333, 700, 0.5)}


def gather_lim(count, cap):
    t = geometry()["gather_tile"]
    return min(-(-count // t) * t, cap)


def mover_rows(n_src, n_list, seed):
    """A row list of n_list distinct source rows in no order (longer than any count it is used with)."""
    return torch.randperm(n_src, generator=gen(seed))[:n_list].to(torch.int32)


def gather_reference(src, rows, count, cap, n_dst, cols, fill=MOVER_FILL):
    """dst[i] = src[rows[i]] for i < count, zero for count <= i < lim, untouched (fill) from lim on."""
    out = torch.full((n_dst, cols), fill, dtype=BF16)
    lim = gather_lim(count, cap)
    out[:lim] = 0
    out[:count] = src[rows[:count].long(), :cols].to(BF16)
    return out


def scatter_reference(src, rows, count, n_dst, cols, fill=MOVER_FILL):
    """dst[rows[i]] = bf16(src[i]) for i < count; every other row untouched."""
    out = torch.full((n_dst, cols), fill, dtype=BF16)
    out[rows[:count].long()] = src[:count, :cols].to(BF16)
    return out


def compact_labels(name):
    B, half, S, frac = COMPACT_CASES[name]
    g = gen(B * 1000 + half)
    labels = torch.full((B, half), -100, dtype=torch.int64)
    pick = torch.rand(B, half, generator=g) < frac
    labels[pick] = torch.randint(0, 5000, (int(pick.sum()),), generator=g)
    row_map = torch.randperm(B * S, generator=g).to(torch.int32)
    return labels, row_map


def compact_reference(labels, half, S, offset, row_map=None):
    """(rows, targets) of the labelled positions in order: row = b * S + offset + position, through the row map if any."""
    flat = labels.reshape(-1)
    idx = (flat != -100).nonzero().squeeze(1)
    pos = (idx // half) * S + offset + idx % half
    rows = pos if row_map is None else row_map[pos].long()
    return rows.int(), flat[idx].int()
