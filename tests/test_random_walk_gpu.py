"""GPU: stonk_random_walks against the numpy restatement of tests/test_node2vec_cpu.py - bit for bit. The graph is the
smallest that reaches every branch of the kernel: N = 67 (not a multiple of the 64 walks of a wavefront), a hub adjacent to
every connected node (long adjacency list: the binary search, many rejections, the 32-attempt cap), a leaf of degree 1 (every
step out of it is a return), a triangle (common neighbours), a node of degree 0 (reached only as an explicit start: the walk
stays), and a sparse ring among the rest (candidates of the third class). L = 127 crosses three full 32-step tiles and a
31-step tail; L = 2 is the first-order step alone; L = 3 the first second-order step."""
import numpy as np
import pytest
import torch

from stonkgs_amd.node2vec import walk_thresholds
from tests.test_node2vec_cpu import walks_ref

pytestmark = pytest.mark.gpu

N, HUB, LEAF, ISOLATED = 67, 0, 65, 66
SENTINEL = -7


def _graph():
    edges = {(HUB, v) for v in range(1, 66)}               # the hub, the leaf's only edge included
    edges |= {(1, 2), (2, 3), (1, 3)}                        # a triangle away from the hub's spokes
    edges |= {(v, v + 1) for v in range(4, 64)} | {(4, 64)}  # a ring 4 .. 64
    edges |= {(10, 20), (20, 30), (10, 30), (7, 40)}
    both = sorted({(a, b) for a, b in edges} | {(b, a) for a, b in edges})
    rows = np.array([a for a, _ in both])
    col = np.array([b for _, b in both], dtype=np.int32)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=rowptr[1:])
    assert rowptr[LEAF + 1] - rowptr[LEAF] == 1 and rowptr[ISOLATED + 1] == rowptr[ISOLATED] and rowptr[1] == 65
    return rowptr, col


@pytest.fixture(scope="module")
def graph(hip):
    rowptr, col = _graph()
    return rowptr, col, torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()


def _launch(hip, rp, cl, starts, lo, hi, L, thr, seed, out):
    hip.call("stonk_random_walks", hip.ptr(rp), hip.ptr(cl), N, hip.ptr(starts), lo, hi, L, *thr, seed, hip.ptr(out),
             out.shape[1], hip.stream_ptr())


EXPLICIT = [ISOLATED, LEAF, HUB, 1, 2, 3, 64, 4, ISOLATED, 30]


@pytest.mark.parametrize("weights", [(1, 1, 1), (4, 1, 0.25), (0.25, 1, 4)])
@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("L", [2, 3, 127])
def test_walks_are_bit_exact_and_independent_of_the_launch_split(hip, graph, L, explicit, weights):
    rowptr, col, rp, cl = graph
    thr = walk_thresholds(*weights)
    seed = 1234 + L
    W = len(EXPLICIT) if explicit else 4 * N
    starts_np = np.array(EXPLICIT, dtype=np.int32) if explicit else None
    starts = torch.from_numpy(starts_np).cuda() if explicit else None
    ld = L + 3                                              # a row stride larger than the row
    want = walks_ref(rowptr, col, starts_np, W, L, thr, seed)
    one = torch.full((W, ld), SENTINEL, dtype=torch.int32, device="cuda")
    _launch(hip, rp, cl, starts, 0, W, L, thr, seed, one)
    got = one.cpu().numpy()
    assert np.array_equal(got[:, :L], want)                 # bit for bit
    assert (got[:, L:] == SENTINEL).all()                   # the padding of a row is not touched
    # every consecutive pair is an edge, or a node of degree 0 repeated
    keys = set((np.repeat(np.arange(N), np.diff(rowptr)) * N + col).tolist())
    a, b = want[:, :-1].ravel().astype(np.int64), want[:, 1:].ravel().astype(np.int64)
    deg = np.diff(rowptr)
    assert all((x * N + y) in keys or (x == y and deg[x] == 0) for x, y in zip(a.tolist(), b.tolist()))
    if explicit:
        assert (want[0] == ISOLATED).all() and want[1, 1] == HUB     # the walk stays / the leaf's only way out
    at_leaf = want[:, :-1] == LEAF
    assert (want[:, 1:][at_leaf] == HUB).all()              # every step out of the leaf goes back to the hub
    # three uneven ranges == one launch; rows outside a range keep the sentinel
    cuts = [0, W // 5, W // 5 + 1, W]
    parts = torch.full((W, ld), SENTINEL, dtype=torch.int32, device="cuda")
    for i in (2, 0):
        _launch(hip, rp, cl, starts, cuts[i], cuts[i + 1], L, thr, seed, parts)
    mid = parts.cpu().numpy()
    assert (mid[cuts[1]:cuts[2]] == SENTINEL).all() and np.array_equal(mid[:cuts[1], :L], want[:cuts[1]])
    _launch(hip, rp, cl, starts, cuts[1], cuts[2], L, thr, seed, parts)
    assert torch.equal(parts, one)
    # two launches are bit-identical
    again = torch.full((W, ld), SENTINEL, dtype=torch.int32, device="cuda")
    _launch(hip, rp, cl, starts, 0, W, L, thr, seed, again)
    assert torch.equal(again, one)


def test_a_start_outside_the_graph_gives_a_row_of_minus_one(hip, graph):
    rowptr, col, rp, cl = graph
    starts = torch.tensor([5, N, -3, 6], dtype=torch.int32, device="cuda")
    out = torch.full((4, 40), SENTINEL, dtype=torch.int32, device="cuda")
    _launch(hip, rp, cl, starts, 0, 4, 40, walk_thresholds(4, 1, 0.25), 9, out)
    got = out.cpu().numpy()
    assert (got[1] == -1).all() and (got[2] == -1).all() and got[0, 0] == 5 and got[3, 0] == 6 and (got[[0, 3]] >= 0).all()
