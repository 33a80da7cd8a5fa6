"""Case tables, input builders and launch constants of the graph-side kernels for tests/test_graph_parity_gpu.py:
csrc/node2vec.hip (skip-gram step), csrc/transe.hip (step, row normalisation, ranks), csrc/link_prediction.hip (loss /
gradient) and csrc/kg_baseline.hip (pooling, training, prediction). tests/test_graph_ref_cpu.py pins all of it without a
GPU. CPU only: nothing here touches a device.

Every case is there for one branch of a kernel, named where the case is built. Whether the branch is taken depends on
constants of the launchers (grid caps, the candidate split, which instantiation a D or C selects); `geometry()` reads those
out of the launchers' own source lines, so that a launcher edited without its case fails the CPU file by name.

References are the restatements the kernels' first tests were written against - `sgns_ref` (test_node2vec_cpu.py),
`transe_step_ref`, `normalize_ref`, `rank_ref` (test_transe_cpu.py), `integer_counts` (test_transe_rank_gpu.py),
`lossgrad_ref` (test_link_prediction_cpu.py), `Restatement`, `train_restated`, `pool_restated` (test_kg_baseline_cpu.py) -
in float64 for the reference and in float32 for the error of the number format. THE RULE (`compare`): per quantity, over an
array, the kernel may deviate from float64 by 4x what the float32 restatement deviates from it on the same inputs; where the
construction makes the arithmetic exact, bit equality. The builders also run restatements with ONE MISTAKE each (`wrong=`),
so that the CPU file can show that the cases tell them apart by at least 3x that tolerance."""
import functools
import os
import re

import numpy as np

from tests.test_node2vec_cpu import SGNS_SALT, _h, group_nodes, reduced_window, sgns_ref
from tests.test_transe_cpu import group_negatives, normalize_ref, transe_step_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stonkgs_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------
# launch geometry, from the launchers' source
# ---------------------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the launcher's line is not what tests/graph_ref.py reads - re-read it and re-size the case"
    return m


@functools.lru_cache(maxsize=None)
def geometry():
    """The constants the cases are sized by: {name: int or list}."""
    g = {}
    n2v, te, lp, kg = _src("node2vec.hip"), _src("transe.hip"), _src("link_prediction.hip"), _src("kg_baseline.hip")
    for key, text, var in (("sgns_cap", n2v, "ngroups"), ("transe_cap", te, "ngroups"), ("normalize_cap", te, "rows")):
        m = _find(rf"const int64_t blocks = {var} < (\d+) \? {var} : (\d+);", text, key)
        assert m.group(1) == m.group(2), key
        g[key] = int(m.group(1))
    _find(r"for \(long g = blockIdx\.x; g < ngroups; g \+= gridDim\.x\)", n2v, "sgns grid stride")
    _find(r"for \(long g = g_lo \+ blockIdx\.x; g < g_hi; g \+= gridDim\.x\)", te, "transe grid stride")
    _find(r"for \(long row = row_lo \+ blockIdx\.x; row < row_hi; row \+= gridDim\.x\)", te, "normalize grid stride")
    _find(r"return \(nctx \* D \+ nctx \* \(K \+ 1\) \+ nctx \+ \(K \+ 1\)\) \* 4;", n2v, "sgns LDS bytes")
    g["sgns_lds_limit"] = int(_find(r"sgns_lds_bytes\(D, window, negatives\) <= (\d+)", n2v, "sgns LDS limit").group(1))
    g["rank_qt"] = int(_find(r"#define RANK_QT (\d+)", te, "RANK_QT").group(1))
    g["rank_target"] = int(_find(r"split = \((\d+) \+ tiles - 1\) / tiles;", te, "rank split target").group(1))
    g["rank_rows_per_slice"] = int(_find(r"const int64_t most = \(N_e \+ 63\) / (\d+);", te, "rank slice floor").group(1))
    m = _find(r"split = split > (\d+) \? (\d+) : \(split < 1 \? 1 : split\);", te, "rank split cap")
    assert m.group(1) == m.group(2)
    g["rank_split_cap"] = int(m.group(1))
    _find(r"lo = lo < 0 \? 0 : lo;\s*\n\s*hi = hi > n_cand \? n_cand : hi;", te, "cand_ptr clamps")
    g["rank_lds_static_limit"] = int(_find(r"if \(rank_lds_bytes\(D\) > (\d+)\)", te, "rank LDS attribute").group(1))
    _find(r"switch \(D / 64\) \{", lp, "linkpred instance switch")
    g["linkpred_nf"] = sorted(int(x) for x in re.findall(r"STONK_LP_CASE\((\d+)\)", lp.split("switch (D / 64)")[1]))
    for name in ("MAX_STEPS", "THREADS", "COLS", "MAX_BATCH", "MAX_CLASSES", "CHUNK"):
        g["kgb_" + name.lower()] = int(_find(rf"#define STONK_KGB_{name} (\d+)", kg, name).group(1))
    _find(r"switch \(\(D \+ 255\) / 256\) \{", kg, "pooling instance switch")
    g["pool_nv"] = sorted(int(x) for x in re.findall(r"STONK_POOL_CASE\((\d+)\)", kg.split("switch ((D + 255) / 256)")[1]))
    chain = [(int(c), int(cm)) for c, cm in re.findall(r"if \(C <= (\d+)\) hipLaunchKernelGGL\(kgb_train_kernel<(\d+)>", kg)]
    last = int(_find(r"\n\s*else hipLaunchKernelGGL\(kgb_train_kernel<(\d+)>", kg, "kgb instance chain").group(1))
    g["kgb_chain"] = chain + [(g["kgb_max_classes"], last)]
    _find(r"constexpr int G = CM < 8 \? CM : CM == 8 \? 8 : 4;", kg, "classes per butterfly")
    _find(r"if \(c0 < C\) \{", kg, "butterfly skip")
    return g


def trips(work, cap):
    """Grid-stride trips of the busiest wavefront."""
    return -(-work // cap)


def sgns_lds_bytes(D, window, K):
    nctx = 2 * window
    return (nctx * D + nctx * (K + 1) + nctx + (K + 1)) * 4


def rank_split(n_q, n_e):
    """gridDim.y of stonk_transe_rank without candidate lists: the launcher's formula."""
    g = geometry()
    tiles = -(-n_q // g["rank_qt"])
    split = -(-g["rank_target"] // tiles)
    split = min(split, -(-n_e // g["rank_rows_per_slice"]))
    return max(1, min(split, g["rank_split_cap"]))


def rank_lds_bytes(D):
    qt = geometry()["rank_qt"]
    return (qt * D + qt + qt + qt * 2) * 4


def pool_nv(D):
    return (D + 255) // 256


def kgb_cm(C):
    """The instantiation stonk_kgb_train_steps picks for C classes."""
    for cmax, cm in geometry()["kgb_chain"]:
        if C <= cmax:
            return cm
    raise AssertionError(C)


def kgb_group(cm):
    return cm if cm < 8 else 8 if cm == 8 else 4


def kgb_butterflies(C):
    """(butterflies run, butterflies the instantiation has, live classes of the last one run)."""
    cm = kgb_cm(C)
    G = kgb_group(cm)
    run = [c0 for c0 in range(0, cm, G) if c0 < C]
    return len(run), cm // G, min(C - run[-1], G)


def kgb_columns(D):
    """Threads that own a feature in column k = 0 .. COLS - 1 (thread t owns d = t + THREADS k)."""
    g = geometry()
    return [max(0, min(g["kgb_threads"], D - k * g["kgb_threads"])) for k in range(g["kgb_cols"])]


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def deviations(names, got, r64, r32):
    """[(name, fp32-restatement deviation, deviation of `got`)], max |x - fp64| per quantity; NaN must sit where fp64 has it."""
    rows = []
    for name, g, a, b in zip(names, got, r64, r32):
        g, a, b = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (g, a, b))
        nan = np.isnan(a)
        assert np.array_equal(np.isnan(b), nan), name
        if not np.array_equal(np.isnan(g), nan):
            rows.append((name, float(np.abs(b[~nan] - a[~nan]).max()), float("inf")))
            continue
        rows.append((name, float(np.abs(b[~nan] - a[~nan]).max()), float(np.abs(g[~nan] - a[~nan]).max())))
    return rows


def compare(tag, names, got, r64, r32, factor=4.0):
    rows = deviations(names, got, r64, r32)
    for name, fmt, ker in rows:
        print(f"GRAPH {tag} {name}: fp32-restatement {fmt:.3e}  kernel {ker:.3e}  allowed {factor * fmt:.3e}")
    for name, fmt, ker in rows:
        assert np.isfinite(ker) and ker <= factor * fmt, (tag, name, ker, fmt)
    return rows


def told_apart(names, wrong, r64, r32, factor=12.0):
    """True if the result `wrong` of a restatement with one mistake misses the rule by 3x in at least one quantity."""
    return any(not ker <= factor * fmt for _, fmt, ker in deviations(names, wrong, r64, r32))


# ---------------------------------------------------------------------------------------------------------------------
# skip-gram: grid stride
# ---------------------------------------------------------------------------------------------------------------------
SGNS_NAMES = ("W_in", "W_out", "loss")
SGNS_STRIDE_EXTRA, SGNS_STRIDE_D, SGNS_STRIDE_LR, SGNS_STRIDE_SEED = 904, 64, 0.05, 5


def sgns_tables(n, d, seed):
    rng = np.random.RandomState(seed)
    s = np.sqrt(3.0) * d ** -0.25                   # dot products of two rows have unit variance
    return rng.uniform(-s, s, (n, d)).astype(np.float32), rng.uniform(-s, s, (n, d)).astype(np.float32)


def sgns_stride_ranges():
    """Walk ranges [lo, hi) of one launch each, all longer than the grid cap: everything, an inner range, cap + 1 groups (one
    wavefront with a second trip) and a range that ends one walk before the end."""
    cap = geometry()["sgns_cap"]
    W = cap + SGNS_STRIDE_EXTRA
    return [(0, W), (137, W - 267), (0, cap + 1), (450, W - 1)]


def sgns_stride_loss_bound(n_terms, total):
    """How far the kernel's loss sum of one launch may lie from float64. The sum is formed by fp32 additions of positive
    terms - a wavefront's own groups, then one atomic add per wavefront in no fixed order -, fewer than 2 n_terms additions,
    each rounding by at most 2^-24 of a partial sum that never exceeds the total; a term (softplus of a dot product of 64
    products, below 8) carries at most a few ulp of its own, 2^-20 to be safe. The float32 restatement's own deviation is
    ONE sample of such a rounding walk and the atomics' order changes from run to run, so 4x that sample would fail one
    run in ten here; the count, which the kernel accumulates at the same places, is compared exactly."""
    return 2 * n_terms * 2.0 ** -24 * total + n_terms * 2.0 ** -20


@functools.lru_cache(maxsize=None)
def sgns_stride_case():
    """The disjoint-rows construction of test_sgns_gpu.py beyond the grid cap: W = cap + 904 walks of two private nodes
    {2 w, 2 w + 1}, positions [0, 1), K 0, D 64. Walk w is group g = w - lo of a launch over [lo, hi): wavefront b takes
    g = b, b + cap. Every seventh walk below 904 has a centre outside the table (-1 and N in turn: `continue` in trip 1,
    real work in trip 2), every eleventh a context outside it (no context left: the other `continue`).
    Returns walks, (w_in0, w_out0) and, per dtype, (w_in, w_out, loss per walk, count per walk) after every walk's group -
    the groups touch disjoint rows, so any range's result is assembled from these (`sgns_stride_expected`)."""
    cap = geometry()["sgns_cap"]
    W = cap + SGNS_STRIDE_EXTRA
    walks = np.arange(2 * W, dtype=np.int32).reshape(W, 2)
    for i, w in enumerate(range(3, SGNS_STRIDE_EXTRA, 7)):
        walks[w, 0] = -1 if i % 2 else 2 * W
    for i, w in enumerate(range(5, SGNS_STRIDE_EXTRA, 11)):
        walks[w, 1] = -1 if i % 2 else 2 * W
    w_in0, w_out0 = sgns_tables(2 * W, SGNS_STRIDE_D, 8)
    runs = []
    for dtype in (np.float64, np.float32):
        a, b = w_in0.astype(dtype), w_out0.astype(dtype)
        loss, count = np.zeros(W, dtype=dtype), np.zeros(W, dtype=np.int64)
        for w in range(W):
            acc = [dtype(0), 0]
            sgns_ref(walks, a, b, [(w, 0)], 3, 0, None, None, SGNS_STRIDE_LR, SGNS_STRIDE_SEED, acc)
            loss[w], count[w] = acc
        runs.append((a, b, loss, count))
    return walks, (w_in0, w_out0), runs[0], runs[1]


def sgns_stride_expected(lo, hi, which, wrong=None):
    """(W_in, W_out, loss sum, count) of one launch over walks [lo, hi); which: 0 float64, 1 float32 (the loss a running
    fp32 sum). wrong: "trip2" - the groups of the second trip are lost; "stride" - wavefronts stride by cap - 1, so group
    cap - 1 is done twice (its update doubled: its rows are read before either add lands, or after - both are wrong)."""
    cap = geometry()["sgns_cap"]
    walks, (w_in0, w_out0), *runs = sgns_stride_case()
    a, b, loss, count = runs[which]
    dt = a.dtype
    live = np.zeros(len(walks), dtype=bool)
    live[lo:hi] = True
    if wrong == "trip2":
        live[lo + cap:] = False
    rows = np.repeat(live, 2)[:, None]
    w_in, w_out = np.where(rows, a, w_in0.astype(dt)), np.where(rows, b, w_out0.astype(dt))
    total = np.cumsum(loss[live], dtype=dt)[-1]
    if wrong == "stride":
        w = lo + cap - 1
        for t, t0, full in ((w_in, w_in0, a), (w_out, w_out0, b)):
            t[2 * w:2 * w + 2] += full[2 * w:2 * w + 2] - t0[2 * w:2 * w + 2].astype(dt)
    return w_in, w_out, float(total), int(count[live].sum())


def sgns_stride_untouched(lo, hi):
    """Rows no group of the launch adds into (outside the range, or of a skipped group): the kernel must leave their bits."""
    walks, (w_in0, w_out0), r64, _ = sgns_stride_case()
    w_in, w_out, _, _ = sgns_stride_expected(lo, hi, 0)
    return (w_in == w_in0).all(axis=1), (w_out == w_out0).all(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# skip-gram: the full window, ids outside the table
# ---------------------------------------------------------------------------------------------------------------------
SGNS_WINDOW, SGNS_WINDOW_K, SGNS_WINDOW_L, SGNS_WINDOW_N, SGNS_WINDOW_LR, SGNS_WINDOW_SEED = 7, 5, 15, 50, 0.025, 37
# (seed 37: the groups (0, 7), (1, 7) and (2, 7) draw b = 7 - the CPU file asserts it)
SGNS_WINDOW_POSITIONS = (6, 7, 8)


def _nodes_last_slot_dropped(walks, w, t, n, window, negatives, alias_thr, alias_idx, seedkey):
    ctx, tgt = group_nodes(walks, w, t, n, window, negatives, alias_thr, alias_idx, seedkey)
    return (ctx[:-1] if len(ctx) == 2 * window else ctx), tgt


def _nodes_window_one_short(walks, w, t, n, window, negatives, alias_thr, alias_idx, seedkey):
    """`<` for `<=` in the window's upper bound: u = t + b is not taken."""
    ctx, tgt = group_nodes(walks, w, t, n, window, negatives, alias_thr, alias_idx, seedkey)
    b = reduced_window(w, t, window, SGNS_WINDOW_SEED)
    row = walks[w]
    if t + b <= len(row) - 1 and 0 <= int(row[t + b]) < n and ctx:
        ctx = ctx[:-1]
    return ctx, tgt


def _nodes_skip_off_by_one(walks, w, t, n, window, negatives, alias_thr, alias_idx, seedkey):
    """The table's last node taken for one outside it: `id >= N - 1` where the kernel says `id >= N`."""
    ctx, tgt = group_nodes(walks, w, t, n, window, negatives, alias_thr, alias_idx, seedkey)
    if not tgt or tgt[0] == n - 1:
        return [], []
    return [x for x in ctx if x != n - 1], [x for x in tgt if x != n - 1]


SGNS_WRONG = {"last slot": _nodes_last_slot_dropped, "window": _nodes_window_one_short, "skip": _nodes_skip_off_by_one}


def sgns_window_inputs():
    """Walks of L = 15 over N = 50 nodes and two alias tables.
    row 0, 1: plain walks (row 1 with revisits)         row 2: -1 and N as contexts around valid centres
    row 3: -1, N and the last node N - 1 as CENTRES     row 4: all -1          row 5: the last node N - 1 among the contexts
    tables[1] sends a third of its slots to an alias outside the table (threshold 0: the alias is always taken)."""
    from stonkgs_amd.node2vec import alias_table

    n, L = SGNS_WINDOW_N, SGNS_WINDOW_L
    rng = np.random.RandomState(15)
    walks = rng.randint(0, n, (6, L)).astype(np.int32)
    walks[1, 4:11] = [9, 17, 9, 30, 17, 9, 30]
    walks[2, [1, 3, 5, 9, 10, 14]] = [-1, n, -1, n, -1, n]
    walks[2, 6:9] = [11, 12, 13]
    walks[3, 6:9] = [-1, n, n - 1]
    walks[4] = -1
    walks[5, [2, 5, 9, 13]] = n - 1
    walks[5, 6:9] = [20, 21, 22]
    thr0, idx0 = alias_table(rng.randint(1, 20, n))
    thr1, idx1 = thr0.copy(), idx0.copy()
    thr1[::3], idx1[::3] = 0, np.where(np.arange(n)[::3] % 2 == 0, n, -1)
    return walks, [(thr0, idx0), (thr1, idx1)]


@functools.lru_cache(maxsize=None)
def sgns_window_case(D, wrong=None):
    """One group per launch, the tables carried from launch to launch: walks x positions (6, 7, 8) x both alias tables.
    Returns (walks, alias tables, launches [(table, w, t)], (w_in0, w_out0), r64, r32); a run is (W_in, W_out, loss sum
    per launch, count per launch). wrong: a key of SGNS_WRONG."""
    walks, tables = sgns_window_inputs()
    launches = [(k, w, t) for k in range(2) for w in range(len(walks)) for t in SGNS_WINDOW_POSITIONS]
    w_in0, w_out0 = sgns_tables(SGNS_WINDOW_N, D, 5)
    nodes = SGNS_WRONG[wrong] if wrong else group_nodes
    runs = []
    for dtype in (np.float64, np.float32):
        a, b, losses, counts = w_in0.astype(dtype), w_out0.astype(dtype), [], []
        for k, w, t in launches:
            acc = [dtype(0), 0]
            sgns_ref(walks, a, b, [(w, t)], SGNS_WINDOW, SGNS_WINDOW_K, tables[k][0], tables[k][1], SGNS_WINDOW_LR,
                     SGNS_WINDOW_SEED, acc, nodes=nodes)
            losses.append(float(acc[0]))
            counts.append(int(acc[1]))
        runs.append((a, b, np.array(losses), counts))
    return walks, tables, launches, (w_in0, w_out0), runs[0], runs[1]


def sgns_window_facts():
    """What the draws of the case give, per launch: (table, w, t, b, contexts, targets, noise nodes lost to an alias outside
    the table)."""
    walks, tables = sgns_window_inputs()
    seedkey = _h(SGNS_WINDOW_SEED ^ SGNS_SALT)
    out = []
    for k, (thr, idx) in enumerate(tables):
        safe = np.where((idx >= 0) & (idx < SGNS_WINDOW_N), idx, 0)       # the same draws with every alias inside the table
        for w in range(len(walks)):
            for t in SGNS_WINDOW_POSITIONS:
                ctx, tgt = group_nodes(walks, w, t, SGNS_WINDOW_N, SGNS_WINDOW, SGNS_WINDOW_K, thr, idx, seedkey)
                full = group_nodes(walks, w, t, SGNS_WINDOW_N, SGNS_WINDOW, SGNS_WINDOW_K, thr, safe, seedkey)[1]
                out.append((k, w, t, reduced_window(w, t, SGNS_WINDOW, SGNS_WINDOW_SEED), ctx, tgt, len(full) - len(tgt)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# TransE step: grid stride under contention, bit-exact
# ---------------------------------------------------------------------------------------------------------------------
TRANSE_STRIDE_EXTRA, TRANSE_STRIDE_LR, TRANSE_STRIDE_MARGIN = 400, 2.0 ** -13, 256.0
TRANSE_STRIDE_SEED, TRANSE_STRIDE_EPOCH = 21, 2
TRANSE_STRIDE_NE, TRANSE_STRIDE_NR = 50, 40


@functools.lru_cache(maxsize=None)
def transe_stride_problem():
    """contention_problem of test_transe_step_gpu.py with cap + 400 triples: 50 entities on multiples of 4/8 (|k| <= 16), 40
    relations on k = 2 mod 4 (|k| <= 14): every component of every x has a numerator = 2 mod 4, so |x| >= 2/8.
    `order` is a permutation with four entries outside [0, n) inside the first cap groups (the wavefronts that skip in
    trip 1 have a second group); two triples name an entity / a relation outside its table."""
    n = geometry()["transe_cap"] + TRANSE_STRIDE_EXTRA
    rng = np.random.RandomState(7)
    n_e, n_r = TRANSE_STRIDE_NE, TRANSE_STRIDE_NR
    ent0 = (rng.randint(-4, 5, (n_e, 64)) * 4 / 8.0).astype(np.float32)
    rel0 = (rng.choice([-14, -10, -6, -2, 2, 6, 10, 14], (n_r, 64)) / 8.0).astype(np.float32)
    triples = np.stack([rng.randint(0, n_e, n), rng.randint(0, n_r, n), rng.randint(0, n_e, n)], axis=1).astype(np.int32)
    triples[::97, 2] = triples[::97, 0]                                    # h == t
    order = rng.permutation(n).astype(np.int32)
    order[[5, 100, 211, 340]] = [-1, n, n + 7, -2 ** 31]
    triples[order[17]] = (n_e, 0, 1)
    triples[order[300]] = (3, -1, 4)
    return ent0, rel0, triples, order


def transe_stride_ranges():
    n = geometry()["transe_cap"] + TRANSE_STRIDE_EXTRA
    return [(0, n), (3, n - 50)]


@functools.lru_cache(maxsize=None)
def transe_sign_safety(lo, hi, wrong=None):
    """sign_safety of test_transe_step_gpu.py for groups [lo, hi) of transe_stride_problem(), with the step size as a
    parameter. HYPOTHESIS: every x of every group has the signs it has at the initial tables. Under it a group's adds do
    not depend on what it read; B[row][i] = the sum over the launch of |add_i| into that row bounds how far component i
    can be from its initial value at any moment of any interleaving. Asserted: |x_i(initial)| > B_a[i] + B_r[i] + B_b[i]
    over the three rows of every x - no first sign flip can happen, so the hypothesis holds however the groups interleave,
    fully stale or sequential - and the margin exceeds every d(x) by more than the same drift: every term is active.
    Exactness: every table value is a multiple of lr below 8, every loss term at the initial tables a multiple of 1/8, and
    the sum of all of them stays below 2^24 eighths - so does every partial sum a wavefront or the atomics can form.
    Returns (ent, rel) of the sequential restatement as fp32, (loss, count) of the launch with lr = 0, and the figures.
    wrong: "trip2" - the groups of the second trip lost."""
    cap = geometry()["transe_cap"]
    ent0, rel0, triples, order = transe_stride_problem()
    K, margin, lr, seed, epoch = 1, TRANSE_STRIDE_MARGIN, TRANSE_STRIDE_LR, TRANSE_STRIDE_SEED, TRANSE_STRIDE_EPOCH
    groups = range(lo, min(hi, lo + cap) if wrong == "trip2" else hi)
    ent, rel, loss, log = ent0.astype(np.float64), rel0.astype(np.float64), [0.0, 0], []
    transe_step_ref(ent, rel, triples, order, groups, K, 1, margin, lr, seed, epoch, loss, log)
    still = [0.0, 0]
    transe_step_ref(ent0.astype(np.float64), rel0.astype(np.float64), triples, order, groups, K, 1, margin, 0.0, seed, epoch,
                    still)
    e64, r64 = ent0.astype(np.float64), rel0.astype(np.float64)
    bound_e, bound_r = np.zeros_like(e64), np.zeros_like(r64)
    xs_of, skipped_groups = [], 0
    for g, tri, signs, terms in log:
        if signs is None:
            skipped_groups += 1
            continue
        h, r, t = triples[tri]
        assert all(active for _, _, _, skipped, active, _ in terms if not skipped)
        xp = (e64[h] + r64[r]) - e64[t]
        st, sh, xs, live = np.zeros(64), np.zeros(64), [(xp, h, r, t)], 0
        for _, tail, e, skipped, _, _ in terms:
            if skipped:
                continue
            xj = (e64[h] + r64[r]) - e64[e] if tail else (e64[e] + r64[r]) - e64[t]
            xs.append((xj, h, r, e) if tail else (xj, e, r, t))
            bound_e[e] += lr * np.abs(np.sign(xj))
            if tail:
                st += np.sign(xj)
            else:
                sh += np.sign(xj)
            live += 1
        gp = live * np.sign(xp)
        bound_e[h] += lr * np.abs(gp - st)
        bound_r[r] += lr * np.abs((gp - st) - sh)
        bound_e[t] += lr * np.abs(sh - gp)
        xs_of.append(xs)
    d_max, slack = 0.0, np.inf
    for xs in xs_of:
        for x, a, r, b in xs:
            drift = bound_e[a] + bound_r[r] + bound_e[b]
            slack = min(slack, float((np.abs(x) - drift).min()))
            d_max = max(d_max, float(np.abs(x).sum() + drift.sum()))
    units = still[0] * 8
    facts = dict(slack=slack, d_max=d_max, margin=margin, loss_units=units, skipped_groups=skipped_groups,
                 largest=float(max(np.abs(ent).max(), np.abs(rel).max())),
                 on_grid=bool((ent / lr == np.round(ent / lr)).all() and (rel / lr == np.round(rel / lr)).all()),
                 moved=not np.array_equal(ent, e64) and not np.array_equal(rel, r64))
    return ent.astype(np.float32), rel.astype(np.float32), (still[0], still[1]), loss[1], facts


# ---------------------------------------------------------------------------------------------------------------------
# row normalisation: grid stride
# ---------------------------------------------------------------------------------------------------------------------
NORMALIZE_EXTRA, NORMALIZE_D, NORMALIZE_LD, NORMALIZE_LO, NORMALIZE_MARGIN = 300, 64, 80, 3, 5


@functools.lru_cache(maxsize=None)
def normalize_case(wrong=None):
    """cap + 300 rows [3, 3 + cap + 300) of a table with 5 more rows behind them, D 64, ld 80. Rows 3 + 7 i (i < 40) are zero
    or below the 1e-12 threshold: their wavefronts `continue` in trip 1 and have a row in trip 2.
    Returns (full [rows, ld] fp32, lo, hi, r64 [rows, D], r32). wrong: "trip2" - rows of the second trip left alone."""
    cap = geometry()["normalize_cap"]
    lo, hi = NORMALIZE_LO, NORMALIZE_LO + cap + NORMALIZE_EXTRA
    rows = hi + NORMALIZE_MARGIN
    rng = np.random.RandomState(64)
    full = (rng.randn(rows, NORMALIZE_LD) * rng.uniform(0.01, 30, (rows, 1))).astype(np.float32)
    for i in range(40):
        full[lo + 7 * i, :NORMALIZE_D] = 0 if i % 2 else 1e-20
    r64, r32 = full[:, :NORMALIZE_D].astype(np.float64), full[:, :NORMALIZE_D].copy()
    end = lo + cap if wrong == "trip2" else hi
    normalize_ref(r64, lo, end)
    normalize_ref(r32, lo, end)
    return full, lo, hi, r64, r32


# ---------------------------------------------------------------------------------------------------------------------
# TransE step: skipped groups and zero x
# ---------------------------------------------------------------------------------------------------------------------
TRANSE_NAMES = ("ent", "rel", "loss")
TRANSE_ZERO_K, TRANSE_ZERO_LR, TRANSE_ZERO_EPOCHS, TRANSE_ZERO_SEED = 5, 0.05, 4, 3
TRANSE_ZERO_NE, TRANSE_ZERO_NR = 8, 3


def transe_zero_inputs(D):
    """Tables on a grid of eighths (|k| <= 8) with planted equalities, 12 triples, an order of 12 entries.
      entity 1 = entity 0 + relation 0; entity 2 = a copy of entity 1; entity 7 = a copy of entity 0; entity 6 = a copy of
      entity 3; relation 1 = 0.
      triple 0 (0, 0, 1) and 3 (0, 0, 2): h + r == t exactly, x_p = 0. A tail replaced by 2 (or 1) and a head replaced by 7
        reproduce x_j = 0.
      triple 1 (3, 1, 3): h == t with the zero relation row, x_p = 0; replacement 6 on either side gives x_j = 0.
      triples 4 .. 7: h = N_e, r = N_r, t = -1, h = -1: an id outside its table.
      order entries 8, 9, 10: -1, n, 40: outside [0, n)."""
    rng = np.random.RandomState(D)
    ek, rk = rng.randint(-8, 9, (TRANSE_ZERO_NE, D)), rng.randint(-8, 9, (TRANSE_ZERO_NR, D))
    rk[1] = 0
    ek[1] = ek[0] + rk[0]
    ek[2], ek[7], ek[6] = ek[1], ek[0], ek[3]
    n_e, n_r = TRANSE_ZERO_NE, TRANSE_ZERO_NR
    triples = np.array([[0, 0, 1], [3, 1, 3], [4, 2, 5], [0, 0, 2], [n_e, 0, 1], [0, n_r, 1], [0, 0, -1], [-1, 2, 4],
                        [5, 2, 4], [6, 0, 2], [1, 2, 0], [7, 1, 5]], dtype=np.int32)
    order = np.array([0, 1, 2, 3, 4, 5, 6, 7, -1, 12, 40, 9], dtype=np.int32)
    return (ek / 8.0).astype(np.float32), (rk / 8.0).astype(np.float32), triples, order


def _x_of(ent, rel, h, r, t):
    return (ent[h] + rel[r]) - ent[t]


def transe_zero_margin(D, norm):
    """Half-way between two grid points next to the median d(x_j) over every negative the case draws: of the groups with
    x_p = 0 about half the terms are active. A function of the inputs alone."""
    ent0, rel0, triples, order = transe_zero_inputs(D)
    e, r = ent0.astype(np.float64), rel0.astype(np.float64)
    ds = []
    for epoch in range(TRANSE_ZERO_EPOCHS):
        for g in range(len(order)):
            tri = int(order[g])
            if not 0 <= tri < len(triples):
                continue
            h, rr, t = (int(v) for v in triples[tri])
            if not (0 <= h < len(e) and 0 <= t < len(e) and 0 <= rr < len(r)):
                continue
            for _, tail, c, skipped in group_negatives(g, epoch, h, t, len(e), TRANSE_ZERO_K, TRANSE_ZERO_SEED):
                if not skipped:
                    x = _x_of(e, r, h, rr, c) if tail else _x_of(e, r, c, rr, t)
                    ds.append(np.abs(x).sum() if norm == 1 else np.sqrt((x * x).sum()))
    return float(np.floor(np.median(ds) * 8) / 8 + 1 / 16)


@functools.lru_cache(maxsize=None)
def transe_zero_case(D, norm, wrong=None):
    """One group per launch, EVERY launch from the initial tables (an update would undo the planted equalities): groups 0 ..
    11 x 4 epochs. Returns (ent0, rel0, triples, order, margin, launches [(g, epoch)], r64, r32, logs); a run is (ent
    [launches, N_e, D], rel [launches, N_r, D], loss per launch, count per launch); logs = (fp64's, fp32's) decisions.
    wrong: "sign0" - sign(0) taken for 1 (norm 1); "eps" - no threshold on the norm: 0 / 0 (norm 2); "order" - an order
    entry equal to n accepted as the last triple."""
    import tests.test_transe_cpu as tc

    ent0, rel0, triples, order = transe_zero_inputs(D)
    margin = transe_zero_margin(D, norm)
    launches = [(g, epoch) for epoch in range(TRANSE_ZERO_EPOCHS) for g in range(len(order))]
    use_order = np.where(order == len(triples), len(triples) - 1, order).astype(np.int32) if wrong == "order" else order
    saved = tc._grad
    if wrong == "sign0":
        tc._grad = lambda x, d, nrm: np.where(x >= 0, 1.0, -1.0).astype(x.dtype)
    elif wrong == "eps":
        def no_threshold(x, d, nrm):
            with np.errstate(invalid="ignore", divide="ignore"):
                return x / d
        tc._grad = no_threshold
    try:
        runs, logs = [], []
        for dtype in (np.float64, np.float32):
            ents, rels, losses, counts, log = [], [], [], [], []
            for g, epoch in launches:
                ent, rel, acc = ent0.astype(dtype), rel0.astype(dtype), [dtype(0), 0]
                transe_step_ref(ent, rel, triples, use_order, [g], TRANSE_ZERO_K, norm, margin, TRANSE_ZERO_LR, TRANSE_ZERO_SEED,
                                epoch, acc, log)
                ents.append(ent)
                rels.append(rel)
                losses.append(float(acc[0]))
                counts.append(int(acc[1]))
            runs.append((np.stack(ents), np.stack(rels), np.array(losses), counts))
            logs.append(log)
    finally:
        tc._grad = saved
    return ent0, rel0, triples, order, margin, launches, runs[0], runs[1], tuple(logs)


def transe_zero_facts(D, norm):
    """Counts, from the fp64 restatement's log and the initial tables: groups skipped for their order entry / for an id,
    groups with x_p = 0 that have an active term, active terms with x_j = 0 (tail- and head-replaced), active and
    inactive terms, terms skipped because the replacement is the replaced entity."""
    ent0, rel0, triples, order, margin, launches, _, _, (log, _) = transe_zero_case(D, norm)
    e, r = ent0.astype(np.float64), rel0.astype(np.float64)
    f = dict(skip_order=0, skip_id=0, xp_zero_active=0, xj_zero_tail=0, xj_zero_head=0, active=0, inactive=0, same=0)
    for (g, tri, signs, terms) in log:
        if signs is None:
            f["skip_order" if not 0 <= tri < len(triples) else "skip_id"] += 1
            continue
        h, rr, t = (int(v) for v in triples[tri])
        xp_zero = not _x_of(e, r, h, rr, t).any()
        if xp_zero and any(a for _, _, _, s, a, _ in terms if not s):
            f["xp_zero_active"] += 1
        for _, tail, c, skipped, active, _ in terms:
            if skipped:
                f["same"] += 1
                continue
            f["active" if active else "inactive"] += 1
            x = _x_of(e, r, h, rr, c) if tail else _x_of(e, r, c, rr, t)
            if not x.any():
                assert active                                               # d(x_j) = 0: margin + d(x_p) > 0
                f["xj_zero_tail" if tail else "xj_zero_head"] += 1
    return f


# ---------------------------------------------------------------------------------------------------------------------
# ranks
# ---------------------------------------------------------------------------------------------------------------------
RANK_BIG_NE, RANK_BIG_D = 70001, 64


@functools.lru_cache(maxsize=None)
def rank_big_case():
    """Numerators (|k| <= 16) of a 70001 x 64 table on the grid of eighths, 3 relations, 17 queries (Q = 1 takes the first),
    duplicates of four true tails and heads planted far away - in other candidate slices than the originals."""
    rng = np.random.RandomState(70001)
    ek = rng.randint(-16, 17, (RANK_BIG_NE, RANK_BIG_D)).astype(np.int16)
    rk = rng.randint(-16, 17, (3, RANK_BIG_D)).astype(np.int16)
    queries = np.stack([rng.randint(0, RANK_BIG_NE, 17), rng.randint(0, 3, 17), rng.randint(0, RANK_BIG_NE, 17)], axis=1)
    queries = queries.astype(np.int32)
    queries[0] = (RANK_BIG_NE - 1, 1, 0)                                   # the last and the first row of the table
    for h, _, t in queries[:4].tolist():
        ek[(t + 35000) % RANK_BIG_NE] = ek[t]
        ek[(h + 23456) % RANK_BIG_NE] = ek[h]
    return ek, rk, queries


def rank_clamp_case(D):
    """grid_case(D, 63, 17) of test_transe_rank_gpu.py with candidate lists whose pointer array starts below 0 and ends
    beyond n_cand: the lists the kernel must use are the clamped ones. Returns (ek, rk, queries, ptr, cand, n_cand,
    clamped ptr): cand is as long as the largest pointer, n_cand smaller - a window on it."""
    from tests.test_transe_rank_gpu import grid_case

    ek, rk, queries = grid_case(D, 63, 17)
    queries = queries.copy()
    queries[9, 1] = -1                                                     # (an id out of range: -1 whatever its list)
    rng = np.random.RandomState(D + 1)
    lens = rng.randint(0, 30, 17)
    lens[0], lens[16], lens[15] = 9, 12, 8
    lens[1] = 7
    ptr = np.zeros(18, dtype=np.int64)
    ptr[1:] = np.cumsum(lens)
    total = int(ptr[-1])
    cand = rng.randint(-3, 70, total).astype(np.int32)
    cand[ptr[1]:ptr[1] + 7] = [int(queries[1, 2]), int(queries[1, 0])] * 3 + [(int(queries[1, 2]) + 7) % 63]
    cand[0] = queries[0, 2]                 # (the first entry of the list whose pointer is negative is a tie on side 0)
    n_cand = total - 16                     # the last list is cut away, the one before it cut short
    ptr[0] = -4
    clamped = np.clip(ptr, 0, n_cand)
    return ek, rk, queries, ptr, cand, n_cand, clamped


# ---------------------------------------------------------------------------------------------------------------------
# link prediction, KG baseline: case tables
# ---------------------------------------------------------------------------------------------------------------------
LINKPRED_DS = tuple(64 * k for k in range(1, 17))
LINKPRED_N, LINKPRED_PAD = 1000, 64

POOL_CASES = [(D, L) for D in (320, 512, 832, 1024) for L in (2, 4)]
# name -> (D, C, batch, steps, runs, ragged_to, dropout). What each is there for:
#  d1024    the fourth feature column per thread live in all 256 threads, every class, the largest batch: the shape the
#           register budget of the launch bound rests on
#  d320     column 1 partial (64 of 256 threads), C = 4 fills kgb_train_kernel<4>
#  d832     column 3 partial, C = 8 fills <8> (one butterfly of eight classes)
#  c9, c12  <16> with the fourth butterfly skipped (`c0 < C`); at C 9 the third carries one live class
#  batch1   one row: the loss is that row's term, the chunk has seven dead rows
#  batch9   one row in the second chunk (re-read for the backward pass)
KGB_TRAIN_CASES = {
    "d1024": (1024, 16, 64, 3, 2, 51, 0.1),
    "d320": (320, 4, 8, 3, 3, 5, 0.1),
    "d832": (832, 8, 8, 3, 3, 5, 0.1),
    "c9": (192, 9, 8, 3, 3, 5, 0.1),
    "c12": (192, 12, 8, 3, 3, None, 0.1),
    "batch1": (192, 5, 1, 6, 4, None, 0.1),
    "batch9": (192, 5, 9, 3, 3, 7, 0.1),
}
KGB_STRIDE_CASE = (192, 5, 8, 3, 3, 5, 0.1)     # `pooled` as a view with a row stride of D + 72
KGB_STRIDE_PAD = 72
KGB_SPAN_CASE = (64, 3, 8, 2, 0.1)              # D, C, batch, runs, dropout; max_steps() + 1 steps
KGB_PADDING_CASE = (192, 5, 8, 5, 3, 0.1)       # D, C, batch, steps, runs, dropout; step 2 of every run is all padding
KGB_PADDING_STEP = 2
KGB_PREDICT_CASES = [(64, 3), (832, 16)]
KGB_PREDICT_PAD = 40


def kgb_runs(D, C, R, n=40, seed=0):
    """test_kg_baseline_gpu.py's _runs: n pooled rows and labels, R runs with their own weights and class weights."""
    rng = np.random.RandomState(seed)
    pooled = rng.randn(n, D).astype(np.float32)
    labels = rng.randint(0, C, n).astype(np.int32)
    bound = 1 / np.sqrt(D)
    weights = [((rng.rand(C, D) * 2 - 1) * bound).astype(np.float32) for _ in range(R)]
    biases = [((rng.rand(C) * 2 - 1) * bound).astype(np.float32) for _ in range(R)]
    cws = [(1.0 / rng.randint(1, 9, C)).astype(np.float32) for _ in range(R)]
    return pooled, labels, weights, biases, cws


def kgb_orders(seed, n, steps, batch, runs, ragged_to=None):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(runs):
        order = rng.randint(0, n, (steps, batch)).astype(np.int32)
        if ragged_to is not None:
            order[-1, ragged_to:] = -1
        out.append(order)
    return out


def kgb_case(name):
    """(pooled, labels, weights, biases, cws, orders, batch, p) of a KGB_TRAIN_CASES entry (or "stride")."""
    D, C, batch, steps, runs, ragged_to, p = KGB_STRIDE_CASE if name == "stride" else KGB_TRAIN_CASES[name]
    seed = sum(ord(ch) for ch in name)
    pooled, labels, weights, biases, cws = kgb_runs(D, C, runs, n=90, seed=seed)
    return pooled, labels, weights, biases, cws, kgb_orders(seed + 1, 90, steps, batch, runs, ragged_to), batch, p


def kgb_padding_case():
    D, C, batch, steps, runs, p = KGB_PADDING_CASE
    pooled, labels, weights, biases, cws = kgb_runs(D, C, runs, n=60, seed=29)
    orders = kgb_orders(30, 60, steps, batch, runs)
    for o in orders:
        o[KGB_PADDING_STEP] = -1
    return pooled, labels, weights, biases, cws, orders, batch, p


def kgb_restated(pooled, labels, orders, weights, biases, cws, p, dtype, seed=11, lr=1e-3, wrong=None):
    """[losses of all runs, W, b, mW, vW, mb, vb] by train_restated, the runs stacked. wrong: "columns" - the features from
    768 on are not seen (a fourth column masked away); "counter" - an all-padding step does not count as a global step
    (bias corrections and dropout keys one step behind after it); "classes" - the logits of the classes from 8 on lose
    their dot product (a butterfly skipped that has live classes: `c0 + G <= C`)."""
    from tests.test_kg_baseline_cpu import train_restated

    if wrong == "columns":
        pooled = pooled.copy()
        pooled[:, 768:] = 0
    losses, states = [], []
    for r, order in enumerate(orders):
        order = np.asarray(order)
        if wrong == "counter":
            order = order[(order >= 0).any(axis=1)]
        if wrong == "classes":
            rs, ls = _train_classes_lost(pooled, labels, order, weights[r], biases[r], cws[r], lr, seed, r, p, dtype)
        else:
            rs, ls = train_restated(pooled, labels, order, weights[r], biases[r], cws[r], lr, seed, r, p, dtype=dtype)
        if wrong == "counter":
            ls = np.insert(ls, KGB_PADDING_STEP, np.nan)
        losses.append(ls)
        states.append(rs.state())
    return [np.concatenate(losses)] + [np.stack([s[k] for s in states]) for k in range(6)]


def _train_classes_lost(pooled, labels, order_steps, weight, bias, cw, lr, seed, run, p, dtype):
    import torch

    from stonkgs_amd import kg_baseline_model as kgb
    from tests.test_kg_baseline_cpu import Restatement

    rs = Restatement(weight, bias, cw, lr, dtype)
    plain = rs.forward

    def forward(x, mask=None, pp=0.0):
        h = torch.as_tensor(x, dtype=dtype)
        if mask is not None:
            h = h * torch.as_tensor(mask, dtype=dtype) * (1.0 / (1.0 - float(np.float32(pp))))
        keep = torch.ones(weight.shape[0], 1, dtype=dtype)
        keep[8:] = 0
        return torch.softmax(h @ (rs.linear.weight * keep).T + rs.linear.bias, dim=1)

    rs.forward = forward
    losses = []
    for s, row in enumerate(np.asarray(order_steps)):
        live = row >= 0
        mask = kgb.dropout_keep_mask(seed, run, s, len(row), pooled.shape[1], p)[live] if p > 0 else None
        losses.append(rs.step(pooled[row[live]], labels[row[live]], mask, p))
    rs.forward = plain
    return rs, np.array(losses)


KGB_NAMES = ("loss", "W", "b", "mW", "vW", "mb", "vb")
