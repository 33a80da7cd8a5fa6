"""GPU: stonk_transe_step against the numpy restatement of tests/test_transe_cpu.py (transe_step_ref).

(1) Single groups, one per launch: exact by construction. ent, rel and the loss sum are compared with the restatement in
fp64. Every launch has its own loss slot, as in TransE.train, and "the loss sum" is the vector of the launches' loss sums:
the largest deviation over the launches is what the rule below is applied to. (ONE fp32 accumulator over all launches makes
the figure a coin toss: at D 64, K 5, norm 2, N_e 3 the fp32 numpy restatement ends 0.36 ulp of the total from fp64, 2.7e-6 of
80.2, by luck of its roundings, and the kernel 1.8e-5, 2.4 ulp - a figure that fp32 numpy arithmetic in the kernel's
summation order, 64 lanes and a butterfly, reproduces to the last digit. A maximum over 16 sums does not depend on luck.) Tolerance (the rule of test_sgns_gpu.py): the same restatement run in fp32 numpy deviates from fp64 by the rounding of
the number format on these very inputs; the kernel (another reduction order over 64 lanes, fused multiply-adds) is allowed
4x that figure, per quantity; the count must be equal. Before the GPU is touched the test asserts that the fp32 and the
fp64 restatement took IDENTICAL decisions (hinge activity, skips, the signs of x for norm 1) - so no flipped hinge hides
inside the tolerance, and none is excused - and that active and inactive terms, a skip and (K > 1) two equal negatives
all occur. The figures are printed before they are asserted.
(2) Full contention, bit-exact: 1000 groups on 50 entities in ONE launch, norm 1, tables on a grid of eighths, lr = 2^-10,
a margin at which every term is active. No component of any x can change sign during the launch (asserted on the CPU, for
ANY interleaving: every |x_i| exceeds the sum of all adds its three rows can receive), so every gradient is a vector of
small integers that does not depend on what the group read, every add is exact in fp32 in any order, and the tables must be
BIT-EQUAL to the sequential restatement. The LOSS a group reports does depend on which adds of other groups had landed when
it read its rows, so the loss sum of a contended launch is no function of the inputs: it is asserted exactly - against its
exactly representable value - on a launch over the same groups with lr = 0, and for the lr > 0 launch to lie within the
envelope the same bound implies.
(3) Learning under contention: a 12 x 12 grid of entities with five translation relations, 10 % of the triples held out, D
64, 60 epochs of 64 launches (9 groups each), norm 1, margin 4, two negatives, lr 0.02 -> 0.002. The reference is the
restatement over the same launches, orders and learning rates. Measured on the CPU, held-out filtered MRR / hits@10 of the
restatement: 0.3120 / 0.984, 0.4030 / 1.0, 0.3842 / 1.0 for seeds 1, 2, 3 (untrained 0.025 .. 0.036 / 0.05 .. 0.08; chance is
10 / 144); the margin is that spread, 0.091, and the test runs seed 3. The schedule was chosen on the CPU with the
restatement in a second, fully stale mode (every group of a launch reads the tables as they were when the launch began -
the far end of what concurrency can do): 0.4222, 0.3700, 0.3924 for the three seeds, inside the seed spread. With only five
relation rows the number of launches matters: at 8 launches per epoch (70 groups each, 14 stale adds per relation row)
the fully stale mode drops to 0.27 / 0.944 against 0.41 / 1.0 sequential, and the kernel with it (0.29 / 0.944 measured) -
why the host cuts an epoch into many launches.
(4) A star: every group has the hub as head.

Measured on an MI355X, (1) over all 24 cases, max |x - fp64| after the whole sequence, fp32 numpy / kernel: ent 4.8e-08 ..
4.5e-07 / the same to three digits, rel 3.6e-08 .. 2.1e-07 / the same but for two cases (5.8e-08 / 5.1e-08, 1.28e-07 /
1.50e-07), loss (the largest over the 16 launches) 3.6e-07 .. 1.9e-04 / 5.9e-07 .. 1.6e-04, the kernel at most 1.8x numpy (D
1024, K 1, norm 1, N_e 3: 5.5e-05 / 1.0e-04). (2) tables bit-equal in all three launches; lr 0: loss sum 501751.5 = the
restatement's; lr 2^-10: 501751.5625 against 501748.79 sequential, envelope 14208; smallest |x_i| minus its drift bound
0.076. (3) filtered MRR / hits@10: kernel 0.3894 / 0.992, restatement 0.3842 / 1.0, untrained 0.0356 / 0.073."""
import numpy as np
import pytest
import torch

from stonkgs_amd import transe as tr
from tests.test_transe_cpu import normalize_ref, rank_ref, transe_step_ref

pytestmark = pytest.mark.gpu

SEED_SPREAD = 0.091     # filtered MRR of the restatement over seeds 1, 2, 3 (module docstring)


def _step(hip, ent, rel, tri, order, lo, hi, K, norm, margin, lr, seed, epoch, loss):
    hip.call("stonk_transe_step", hip.ptr(ent), hip.ptr(rel), ent.shape[0], rel.shape[0], ent.shape[1], hip.ptr(tri),
             tri.shape[0], hip.ptr(order), lo, hi, K, norm, margin, lr, seed, epoch, hip.ptr(loss), hip.stream_ptr())


def _compare(tag, got, ref64, ref32):
    """got / ref64 / ref32: (ent, rel, loss sums, counts). The kernel may deviate from fp64 by 4x what fp32 numpy does."""
    assert got[3] == ref64[3] == ref32[3], (tag, got[3], ref64[3], ref32[3])
    figures = []
    for name, g, r64, r32 in zip(("ent", "rel", "loss"), got, ref64, ref32):
        fmt = float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max())
        ker = float(np.abs(np.asarray(g, dtype=np.float64) - r64).max())
        print(f"{tag} {name}: fp32-numpy {fmt:.3e}  kernel {ker:.3e}  allowed {4 * fmt:.3e}")
        figures.append((name, fmt, ker))
    for name, fmt, ker in figures:
        assert np.isfinite(ker) and ker <= 4 * fmt, (tag, name, ker, fmt)


# ------------------------------------------------------------------------------------------------ (1) single groups
def single_group_case(D, K, norm, n_e, seed):
    """Tables, triples (h == t among them) and the two restatements with their decision logs, over 2 epochs of the triples."""
    rng = np.random.RandomState(100 * n_e + D + K + norm)
    ent0 = rng.uniform(-1, 1, (n_e, D)).astype(np.float32)
    rel0 = rng.uniform(-1, 1, (3, D)).astype(np.float32)
    triples = np.stack([rng.randint(0, n_e, 8), rng.randint(0, 3, 8), rng.randint(0, n_e, 8)], axis=1).astype(np.int32)
    triples[3, 2] = triples[3, 0]                                          # h == t
    runs = []
    for dtype in (np.float64, np.float32):
        ent, rel, losses, counts, log = ent0.astype(dtype), rel0.astype(dtype), [], [], []
        for epoch in range(2):
            for g in range(len(triples)):                                 # one group per launch: each has its own loss sum
                loss = [dtype(0), 0]
                transe_step_ref(ent, rel, triples, None, [g], K, norm, 0.5, 0.05, seed, epoch, loss, log)
                losses.append(float(loss[0]))
                counts.append(loss[1])
        runs.append((ent, rel, np.array(losses), counts, log))
    return ent0, rel0, triples, runs


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_single_groups_match_the_restatement(hip, D, K, norm):
    """40 entities (and 3, where a replacement often equals the replaced entity and negatives coincide), 3 relations, margin
    0.5, lr 0.05, two epochs over 8 triples, one group per launch."""
    for n_e, seed in ((40, 11), (3, 13)):      # (seeds at which every condition below holds in all twelve cases)
        ent0, rel0, triples, (r64, r32) = single_group_case(D, K, norm, n_e, seed)
        # conditions, on the CPU: identical decisions in both formats; every kind of term occurs
        assert r64[4] == r32[4], "the fp32 and fp64 restatements took different decisions: choose another seed"
        terms = [t for _, _, _, ts in r64[4] for t in ts]
        acts = [a for _, _, _, s, a, _ in terms if not s]
        assert any(acts) and not all(acts), (n_e, sum(acts), len(acts))
        if n_e == 3:
            assert any(s for _, _, _, s, _, _ in terms)
            if K > 1:
                assert any(len({(tail, e) for _, tail, e, s, _, _ in ts if not s}) < sum(not s for _, _, _, s, _, _ in ts)
                           for _, _, _, ts in r64[4])
        g_ent, g_rel = torch.from_numpy(ent0).cuda(), torch.from_numpy(rel0).cuda()
        g_tri, g_loss = torch.from_numpy(triples).cuda(), torch.zeros(2 * len(triples), 2, device="cuda")
        for epoch in range(2):
            for g in range(len(triples)):
                _step(hip, g_ent, g_rel, g_tri, None, g, g + 1, K, norm, 0.5, 0.05, seed, epoch, g_loss[epoch * len(triples) + g])
        loss = g_loss.cpu().numpy()
        got = (g_ent.cpu().numpy(), g_rel.cpu().numpy(), loss[:, 0], loss[:, 1].astype(np.int64).tolist())
        total = [float(np.asarray(x[2], dtype=np.float64).sum()) for x in (got, r64, r32)]
        print(f"D={D} K={K} norm={norm} N_e={n_e} sum over the launches: kernel - fp64 {total[0] - total[1]:.3e}  "
              f"fp32-numpy - fp64 {total[2] - total[1]:.3e}")
        assert np.abs(got[0] - ent0).max() > 1e-3 and np.abs(got[1] - rel0).max() > 1e-3       # the sequence did train
        _compare(f"D={D} K={K} norm={norm} N_e={n_e}", got, r64[:4], r32[:4])


# ------------------------------------------------------------------------------------------------ (2) full contention
LR_EXACT = 2.0 ** -10


def contention_problem():
    """50 entities on multiples of 4/8 (|k| <= 16), 40 relations on k = 2 mod 4 (|k| <= 14), 1000 triples: every component of
    every x = (h + r) - t, whatever the three rows, has a numerator = 2 mod 4, so |x| >= 2/8 and never zero; its sign is
    decided by the entities as often as by the relation."""
    rng = np.random.RandomState(7)
    ent0 = (rng.randint(-4, 5, (50, 64)) * 4 / 8.0).astype(np.float32)
    rel0 = (rng.choice([-14, -10, -6, -2, 2, 6, 10, 14], (40, 64)) / 8.0).astype(np.float32)
    triples = np.stack([rng.randint(0, 50, 1000), rng.randint(0, 40, 1000), rng.randint(0, 50, 1000)], axis=1).astype(np.int32)
    triples[::97, 2] = triples[::97, 0]                                    # h == t
    return ent0, rel0, triples


def sign_safety(ent0, rel0, triples, order, groups, K, margin, seed, epoch):
    """The CPU-side condition of the exact test; returns the sequential restatement's (fp64) tables and loss, and the loss
    envelope. HYPOTHESIS: every x of every group has the signs it has at the initial tables. Under it a group's adds do not
    depend on what it read; B[row][i] = the sum over the launch of |add_i| into that row bounds how far component i of the
    row can be from its initial value at any moment of any interleaving. Asserted: for every x, every component,
    |x_i(initial)| > B_a[i] + B_r[i] + B_b[i] over its three rows - then no first sign flip can happen, the hypothesis holds
    in every interleaving - and the margin exceeds every d(x) by more than the same drift, so every term is active.
    The envelope: whatever a group read, each of its terms differs from its value at the initial tables by at most the
    summed drift of x_p and x_j; the kernel's and the sequential loss sum both lie that close to the initial-table sum, so
    within twice the envelope of each other."""
    ent, rel, loss, log = ent0.astype(np.float64), rel0.astype(np.float64), [0.0, 0], []
    transe_step_ref(ent, rel, triples, order, groups, K, 1, margin, LR_EXACT, seed, epoch, loss, log)
    e64, r64 = ent0.astype(np.float64), rel0.astype(np.float64)
    bound_e, bound_r = np.zeros_like(e64), np.zeros_like(r64)
    xs_of = []
    for g, tri, _, terms in log:
        h, r, t = triples[tri]
        assert all(active for _, _, _, skipped, active, _ in terms if not skipped)
        xp = (e64[h] + r64[r]) - e64[t]
        st, sh, xs, live = np.zeros(64), np.zeros(64), [(xp, h, r, t)], 0
        for _, tail, e, skipped, _, _ in terms:
            if skipped:
                continue
            xj = (e64[h] + r64[r]) - e64[e] if tail else (e64[e] + r64[r]) - e64[t]
            xs.append((xj, h, r, e) if tail else (xj, e, r, t))
            bound_e[e] += LR_EXACT * np.abs(np.sign(xj))
            if tail:
                st += np.sign(xj)
            else:
                sh += np.sign(xj)
            live += 1
        gp = live * np.sign(xp)
        bound_e[h] += LR_EXACT * np.abs(gp - st)
        bound_r[r] += LR_EXACT * np.abs((gp - st) - sh)
        bound_e[t] += LR_EXACT * np.abs(sh - gp)
        xs_of.append(xs)
    envelope, d_max, slack = 0.0, 0.0, np.inf
    for xs in xs_of:
        drifts = []
        for x, a, r, b in xs:
            drift = bound_e[a] + bound_r[r] + bound_e[b]
            slack = min(slack, float((np.abs(x) - drift).min()))
            d_max = max(d_max, float(np.abs(x).sum() + drift.sum()))
            drifts.append(float(drift.sum()))
        envelope += sum(drifts[0] + d for d in drifts[1:])
    print(f"sign safety: smallest |x_i| - drift {slack:.4f}, largest d(x) + drift {d_max:.2f}, margin {margin}")
    assert slack > 0 and margin > d_max
    assert np.abs(ent).max() < 8 and np.abs(rel).max() < 8                 # multiples of 2^-10 below 8: exact in fp32
    assert not np.array_equal(ent, e64) and not np.array_equal(rel, r64)
    return ent.astype(np.float32), rel.astype(np.float32), loss, envelope


def test_one_launch_under_full_contention_is_bit_exact(hip):
    ent0, rel0, triples = contention_problem()
    K, margin, seed = 1, 512.0, 21
    g_tri = torch.from_numpy(triples).cuda()

    def launch(tri, order, lo, hi, lr, epoch=0):
        g_ent, g_rel, g_loss = torch.from_numpy(ent0).cuda(), torch.from_numpy(rel0).cuda(), torch.zeros(2, device="cuda")
        _step(hip, g_ent, g_rel, tri, order, lo, hi, K, 1, margin, lr, seed, epoch, g_loss)
        return g_ent.cpu().numpy(), g_rel.cpu().numpy(), g_loss.cpu().numpy()

    for lo, hi in ((0, 1000), (137, 802)):
        r_ent, r_rel, r_loss, envelope = sign_safety(ent0, rel0, triples, None, range(lo, hi), K, margin, seed, 0)
        # lr = 0: the loss is a function of the inputs - a sum of multiples of 1/8, every partial sum below 2^24 eighths
        still = [0.0, 0]
        transe_step_ref(ent0.astype(np.float64), rel0.astype(np.float64), triples, None, range(lo, hi), K, 1, margin, 0.0, seed,
                        0, still)
        assert still[0] * 8 == int(still[0] * 8) and still[0] * 8 < 2 ** 24 and float(np.float32(still[0])) == still[0]
        k_ent, k_rel, k_loss = launch(g_tri, None, lo, hi, 0.0)
        print(f"[{lo},{hi}) lr 0: loss sum kernel {k_loss[0]!r} restatement {still[0]!r}, count {k_loss[1]} / {still[1]}")
        assert float(k_loss[0]) == still[0] and int(k_loss[1]) == still[1]
        assert np.array_equal(k_ent, ent0) and np.array_equal(k_rel, rel0)
        # lr = 2^-10: bit-equal tables
        k_ent, k_rel, k_loss = launch(g_tri, None, lo, hi, LR_EXACT)
        print(f"[{lo},{hi}) lr 2^-10: max |ent - restatement| {np.abs(k_ent - r_ent).max():.3e}, rel {np.abs(k_rel - r_rel).max():.3e}; "
              f"loss sum kernel {k_loss[0]:.4f} sequential {r_loss[0]:.4f} envelope {envelope:.4f}")
        assert np.array_equal(k_ent, r_ent) and np.array_equal(k_rel, r_rel)
        assert not np.array_equal(k_ent, ent0) and not np.array_equal(k_rel, rel0)
        assert int(k_loss[1]) == r_loss[1] and abs(float(k_loss[0]) - r_loss[0]) <= 2 * envelope + 1e-5 * abs(r_loss[0])
    # a sub-launch with `order` given == the same launch over the permuted triples
    perm = np.random.RandomState(3).permutation(1000).astype(np.int32)
    r_ent, r_rel, r_loss, _ = sign_safety(ent0, rel0, triples, perm, range(137, 802), K, margin, seed, 5)
    a = launch(g_tri, torch.from_numpy(perm).cuda(), 137, 802, LR_EXACT, epoch=5)
    b = launch(torch.from_numpy(np.ascontiguousarray(triples[perm])).cuda(), None, 137, 802, LR_EXACT, epoch=5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and int(a[2][1]) == int(b[2][1]) == r_loss[1]
    assert np.array_equal(a[0], r_ent) and np.array_equal(a[1], r_rel)


# ------------------------------------------------------------------------------------------------ (3) learning
def grid_graph(side=12):
    """(source, relation, target) names: entities on a side x side grid, five translations - what TransE represents exactly."""
    moves = {"right": (1, 0), "up": (0, 1), "right2": (2, 0), "up2": (0, 2), "diagonal": (1, 1)}
    return [(f"n{x}_{y}", name, f"n{x + dx}_{y + dy}") for x in range(side) for y in range(side)
            for name, (dx, dy) in moves.items() if x + dx < side and y + dy < side]


def filtered_report_ref(ent, rel, test, known, norm):
    """The filtered evaluation of fp64 tables by rank_ref and the host arithmetic."""
    index = tr.known_index(known)
    ranks = []
    for side in (0, 1):
        less, equal = rank_ref(ent, rel, test, side, norm)
        ptr, cand = tr.candidate_lists(test, side, index)
        ranks.append(tr.realistic_rank(*tr.filtered_counts(less, equal, *rank_ref(ent, rel, test, side, norm, ptr, cand))))
    return tr.evaluation_report(*ranks)


def test_training_under_contention_learns_the_grid(hip):
    names_e, names_r, triples = tr.build_triples(*zip(*grid_graph()))
    assert len(names_e) == 144 and len(names_r) == 5 and len(triples) == 625
    train_pos, test_pos = tr.split_triples(len(triples), 0.1, 0)
    train, test = triples[train_pos], triples[test_pos]
    m = tr.TransE(n_components=64, epochs=60, negatives=2, margin=4.0, norm=1, lr=0.02, min_lr=0.002, seed=3)
    m.fit_ids(names_e, names_r, train)
    assert np.isfinite(m.entity_vectors).all() and np.isfinite(m.relation_vectors).all()
    assert np.abs(np.linalg.norm(m.entity_vectors, axis=1) - 1).max() < 1e-5
    assert m.loss_history[-1] < m.loss_history[0], m.loss_history
    gpu = m.evaluate(test, known_triples=triples)
    # the reference: the restatement over the same launches, orders and learning rates
    ent0, rel0 = m.initial_vectors(144, 5)
    ent, rel = ent0.numpy().astype(np.float64), rel0.numpy().astype(np.float64)
    plan = m.launch_plan(len(train))
    assert len(plan) == 64 * 60
    for i, (e, lo, hi) in enumerate(plan):
        transe_step_ref(ent, rel, train, m.epoch_order(len(train), e), range(lo, hi), 2, 1, 4.0, m.launch_lr(i, len(plan)), 3, e,
                        [0.0, 0])
        normalize_ref(ent, 0, 144)
    ref = filtered_report_ref(ent, rel, test, triples, 1)
    blank = filtered_report_ref(ent0.numpy().astype(np.float64), rel0.numpy().astype(np.float64), test, triples, 1)
    print(f"filtered MRR / hits@10: restatement {ref['mrr']:.4f} / {ref['hits@10']:.3f}  kernel {gpu['mrr']:.4f} / "
          f"{gpu['hits@10']:.3f}  untrained {blank['mrr']:.4f} / {blank['hits@10']:.3f}  margin {SEED_SPREAD}")
    assert ref["hits@10"] > 0.9 and blank["hits@10"] < 0.15               # the reference learned; untrained is near chance
    assert gpu["mrr"] >= ref["mrr"] - SEED_SPREAD


# ------------------------------------------------------------------------------------------------ (4) hub
def test_hub_contention_stays_finite(hip):
    """A star: one head, 64 tails, one relation, D 768, one epoch - every group adds into the hub's and the relation's row."""
    m = tr.TransE(n_components=768, epochs=1, seed=2, launches_per_epoch=1)     # all 64 groups in one launch
    triples = np.stack([np.zeros(64), np.zeros(64), np.arange(1, 65)], axis=1).astype(np.int32)
    ent, rel = m.train(triples, 65, 1)
    ent0, rel0 = m.initial_vectors(65, 1)
    assert torch.isfinite(ent).all() and torch.isfinite(rel).all()
    assert not torch.equal(ent.cpu(), ent0) and not torch.equal(rel.cpu(), rel0)
    assert np.isfinite(m.loss_history).all() and m.loss_history[0] > 0
