"""GPU: stonk_transe_rank and stonk_rows_l2_normalize.

(1) Exact grid: tables on k / 8 with |k| <= 16. Every |v_i - e_i| is a multiple of 1/8 below 8 and every square a multiple
of 1/64 below 64, so an L1 or squared-L2 distance over D <= 1024 elements is exact in fp32 in ANY summation order, and
less / equal must EQUAL integer arithmetic on the k. Duplicate rows of true entities are planted (equal > 1).
(2) Real-valued tables (N_e 1000, D 768) against the fp64 restatement with a band tau = 4x the largest deviation of the fp32
numpy restatement's distances from fp64 on these inputs:  #(d < d_true - tau) <= less <= #(d < d_true + tau), likewise for
less + equal with <=. Asserted on the CPU first: at most 1 % of the (query, candidate) pairs lie inside the band - else the
bound would test nothing. Planted duplicates of the true rows must come out as exact ties (one instruction sequence for
every distance).
(3) stonk_rows_l2_normalize against fp64 (4x the fp32-numpy deviation), ld > D, a zero row, an inner range.

Measured on an MI355X: (1) equal in all 27 + 2 cases; (2) largest |distance - fp64| of fp32 numpy 9.4e-05 .. 1.14e-04, tau
3.7e-04 .. 4.5e-04, 0.12 % of the pairs inside the band (the true entities and their twelve planted duplicates among them),
every count inside its bounds, every planted duplicate an exact tie; (3) fp32 numpy / kernel: D 64 4.2e-08 / 3.4e-08, D 768
1.24e-08 / 1.14e-08, D 1024 1.48e-08 / 9.5e-09."""
import functools

import numpy as np
import pytest
import torch

from stonkgs_amd import transe as tr
from tests.test_transe_cpu import normalize_ref, rank_distances, rank_ref

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ (1) the exact grid
def integer_counts(ek, rk, queries, side, norm, cand_ptr=None, cand=None):
    """less / equal by integer arithmetic on the numerators k of a k / 8 grid (L1: int16 differences summed in int32; L2:
    |v|^2 - 2 v.e + |e|^2 on integers below 2^53 in float64 - both exact)."""
    q = np.asarray(queries).reshape(-1, 3)
    n_e, n_r = len(ek), len(rk)
    valid = (q[:, 0] >= 0) & (q[:, 0] < n_e) & (q[:, 2] >= 0) & (q[:, 2] < n_e) & (q[:, 1] >= 0) & (q[:, 1] < n_r)
    qs = np.where(valid[:, None], q, 0)
    v = (ek[qs[:, 0]] + rk[qs[:, 1]] if side == 0 else ek[qs[:, 2]] - rk[qs[:, 1]]).astype(np.int16)
    true = qs[:, 2] if side == 0 else qs[:, 0]
    e16 = ek.astype(np.int16)
    if norm == 2:
        ef, vf = ek.astype(np.float64), v.astype(np.float64)
        dist = ((vf * vf).sum(1)[:, None] - 2.0 * (vf @ ef.T) + (ef * ef).sum(1)[None, :]).astype(np.int64)
    less, equal = np.full(len(q), -1, dtype=np.int32), np.full(len(q), -1, dtype=np.int32)
    for i in np.flatnonzero(valid):
        d = np.abs(v[i][None, :] - e16).sum(axis=1, dtype=np.int32) if norm == 1 else dist[i]
        dt = d[true[i]]
        if cand_ptr is not None:
            ids = np.asarray(cand[cand_ptr[i]:cand_ptr[i + 1]], dtype=np.int64)
            d = d[ids[(ids >= 0) & (ids < n_e)]]
        less[i], equal[i] = (d < dt).sum(), (d == dt).sum()
    return less, equal


@functools.lru_cache(maxsize=None)
def grid_case(D, n_e, n_q):
    rng = np.random.RandomState(D + 7 * n_e + 13 * n_q)
    ek, rk = rng.randint(-16, 17, (n_e, D)), rng.randint(-16, 17, (3, D))
    queries = np.stack([rng.randint(0, n_e, n_q), rng.randint(0, 3, n_q), rng.randint(0, n_e, n_q)], axis=1).astype(np.int32)
    for h, _, t in queries[:4].tolist():                                   # duplicates of true tails and true heads
        ek[(t + 7) % n_e] = ek[t]
        ek[(h + 11) % n_e] = ek[h]
    return ek, rk, queries


@pytest.mark.parametrize("n_q", [1, 17, 300])
@pytest.mark.parametrize("n_e", [1, 63, 1000])
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_counts_on_the_exact_grid_equal_integer_arithmetic(hip, D, n_e, n_q):
    ek, rk, queries = grid_case(D, n_e, n_q)
    ent, rel = (ek / 8.0).astype(np.float32), (rk / 8.0).astype(np.float32)
    d_ent, d_rel = torch.from_numpy(ent).cuda(), torch.from_numpy(rel).cuda()
    ties = 0
    for side in (0, 1):
        for norm in (1, 2):
            want = integer_counts(ek, rk, queries, side, norm)
            got = tr.transe_rank(d_ent, d_rel, queries, side, norm)
            assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), \
                (side, norm, np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))[:5])
            assert (want[1] >= 1).all()                                    # the true entity ties with itself
            ties += int((want[1] > 1).sum())
    assert ties > 0 or n_e == 1 or n_q == 1
    if n_e == 63 and n_q == 17:                                            # the integer arithmetic is the restatement's
        for side, norm in ((0, 1), (1, 2)):
            ref = rank_ref(ent.astype(np.float64), rel.astype(np.float64), queries, side, norm)
            want = integer_counts(ek, rk, queries, side, norm)
            assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[1], want[1])


@pytest.mark.parametrize("D", [64, 768])
def test_candidate_lists_on_the_exact_grid(hip, D):
    """Per-query lists: empty ones, ids outside [0, N_e), repeated ids, the true entity in a list, a list for a query whose
    own ids are out of range (-1 whatever the list says)."""
    ek, rk, queries = grid_case(D, 63, 17)
    queries = queries.copy()
    queries[5, 0], queries[9, 1], queries[12, 2] = 63, -1, 1000            # out-of-range head, relation, tail
    rng = np.random.RandomState(1)
    lists = [rng.randint(-3, 70, rng.randint(0, 40)).tolist() for _ in range(17)]
    lists[0], lists[16] = [], []
    lists[1] = [int(queries[1, 2]), int(queries[1, 0])] * 3 + [(int(queries[1, 2]) + 7) % 63]
    ptr = np.zeros(18, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    cand = np.array([c for x in lists for c in x], dtype=np.int32)
    assert (cand < 0).any() and (cand >= 63).any()
    ent, rel = (ek / 8.0).astype(np.float32), (rk / 8.0).astype(np.float32)
    for side in (0, 1):
        for norm in (1, 2):
            want = integer_counts(ek, rk, queries, side, norm, ptr, cand)
            got = tr.transe_rank(ent, rel, queries, side, norm, ptr, cand)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (side, norm, got, want)
            assert want[0][[5, 9, 12]].tolist() == [-1] * 3 and want[0][0] == want[1][0] == 0
            full = tr.transe_rank(ent, rel, queries, side, norm)
            assert full[0][[5, 9, 12]].tolist() == [-1] * 3 and full[1][[5, 9, 12]].tolist() == [-1] * 3
    assert integer_counts(ek, rk, queries, 0, 1, ptr, cand)[1][1] >= 4     # the true tail three times over, and its duplicate


# ------------------------------------------------------------------------------------------------ (2) real-valued tables
def band_counts(dist, true, valid, tau, mask=None):
    """``(less_lo, less_hi, le_lo, le_hi)`` per query from fp64 distances: the counts with the true distance moved by -+tau.
    ``mask`` (bool [Q, N_e], optional): the candidates that count."""
    out = np.full((4, len(true)), -1, dtype=np.int64)
    for i in np.flatnonzero(valid):
        d = dist[i] if mask is None else dist[i][mask[i]]
        dt = dist[i, true[i]]
        out[:, i] = (d < dt - tau).sum(), (d < dt + tau).sum(), (d <= dt - tau).sum(), (d <= dt + tau).sum()
    return out


@functools.lru_cache(maxsize=None)
def real_case():
    rng = np.random.RandomState(5)
    ent = rng.uniform(-1, 1, (1000, 768)).astype(np.float32)
    rel = rng.uniform(-1, 1, (4, 768)).astype(np.float32)
    queries = np.stack([rng.randint(0, 1000, 40), rng.randint(0, 4, 40), rng.randint(0, 1000, 40)], axis=1).astype(np.int32)
    for h, _, t in queries[:6].tolist():
        ent[(t + 7) % 1000] = ent[t]
        ent[(h + 11) % 1000] = ent[h]
    return ent, rel, queries


def test_counts_on_real_valued_tables_lie_in_the_fp32_band(hip):
    ent, rel, queries = real_case()
    d_ent, d_rel = torch.from_numpy(ent).cuda(), torch.from_numpy(rel).cuda()
    for side in (0, 1):
        for norm in (1, 2):
            d64, true, valid = rank_distances(ent.astype(np.float64), rel.astype(np.float64), queries, side, norm)
            d32 = rank_distances(ent, rel, queries, side, norm)[0]
            tau = 4 * float(np.abs(d32.astype(np.float64) - d64).max())
            inside = float((np.abs(d64 - d64[np.arange(40), true][:, None]) < tau).mean())
            # (the true entity itself and its planted duplicates are inside by construction: 40 + 12 pairs of 40 000)
            print(f"side {side} norm {norm}: fp32-numpy deviation {tau / 4:.3e}  tau {tau:.3e}  pairs inside the band {inside:.4%}")
            assert inside <= 0.01
            lo, hi, le_lo, le_hi = band_counts(d64, true, valid, tau)
            less, equal = tr.transe_rank(d_ent, d_rel, queries, side, norm)
            assert (lo <= less).all() and (less <= hi).all(), (side, norm)
            assert (le_lo <= less + equal).all() and (less + equal <= le_hi).all(), (side, norm)
            assert (equal >= 1).all()
            assert (equal[:6] >= 2).all()                                  # bit-equal rows give bit-equal distances


# ------------------------------------------------------------------------------------------------ (3) normalise
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_rows_l2_normalize(hip, D):
    ld, rows, lo, hi = D + 64, 50, 3, 40
    rng = np.random.RandomState(D)
    full = (rng.randn(rows, ld) * rng.uniform(0.01, 30, (rows, 1))).astype(np.float32)
    full[10, :D] = 0                                                       # a zero row inside the range
    full[11, :D] = 1e-20                                                   # norm below 1e-12: left as it is
    r64, r32 = full[:, :D].astype(np.float64), full[:, :D].copy()
    normalize_ref(r64, lo, hi)
    normalize_ref(r32, lo, hi)
    t = torch.from_numpy(full).cuda()
    hip.call("stonk_rows_l2_normalize", hip.ptr(t), ld, lo, hi, D, hip.stream_ptr())
    got = t.cpu().numpy()
    fmt = float(np.abs(r32.astype(np.float64) - r64).max())
    ker = float(np.abs(got[:, :D].astype(np.float64) - r64).max())
    print(f"D={D}: fp32-numpy {fmt:.3e}  kernel {ker:.3e}  allowed {4 * fmt:.3e}")
    assert ker <= 4 * fmt
    assert np.array_equal(got[:, D:], full[:, D:])                         # the padding of every row
    assert np.array_equal(got[:lo], full[:lo]) and np.array_equal(got[hi:], full[hi:])
    assert np.array_equal(got[10], full[10]) and np.array_equal(got[11], full[11])
    assert np.abs(np.linalg.norm(got[lo:hi, :D].astype(np.float64), axis=1)[[0, 1, 2, 3, 4, 5, 6, 9, 12]] - 1).max() < 1e-6
    assert not np.array_equal(got[lo:hi], full[lo:hi])
