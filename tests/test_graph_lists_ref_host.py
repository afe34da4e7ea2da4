"""tests/graph_lists_ref.py checked on the CPU: the exact statement that test_gpu_graph_lists_exact.py holds the list builders
of csrc/graph_ops.hip to.

The reference against a plain per-target loop on tiny inputs (every special distance and every out-of-range target among them),
against GraphBatch._build_lists_host on host-resident batches (padded and CSR, valid targets only: that routine uses bincount),
and proof that an exact comparison with it tells a right list from three kinds of wrong ones."""
import numpy as np
import pytest

import graph_lists_ref as R

F32 = np.float32


def _is_live(e, t, N):
    """one entry, spelled out value by value"""
    if t < 0 or t >= N:
        return False
    if e is None:
        return True
    e = float(e)
    if e != e:                     # NaN
        return False
    return e > 0.0                 # 0.0, -0.0 and negative: False; +inf and the smallest normal: True


def _loop_lists(nlist, edges, N, K):
    n = len(nlist)
    ptr, out = [0], []
    for t in range(N):
        for eid in range(n):
            if int(nlist[eid]) == t and _is_live(None if edges is None else edges[eid], int(nlist[eid]), N):
                out.append(eid)
        ptr.append(len(out))
    nc = None
    if K > 0:
        nc = [int(nlist[eid]) if _is_live(None if edges is None else edges[eid], int(nlist[eid]), N) else eid // K
              for eid in range(n)]
    return ptr, out, nc


def _loop_partition(edges):
    live = [g for g, e in enumerate(edges) if _is_live(e, 0, 1)]
    dead = [g for g, e in enumerate(edges) if not _is_live(e, 0, 1)]
    pos = [-1] * len(edges)
    for r, g in enumerate(live):
        pos[g] = r
    return live + dead, pos, [edges[g] for g in live], len(live)


def test_every_special_value_one_by_one():
    N = 4
    for v in R.DEAD_VALUES:
        assert not R.live_mask(np.array([v], F32), [2], N)[0], v
    for v in R.LIVE_VALUES + (F32(0.05),):
        assert R.live_mask(np.array([v], F32), [2], N)[0], v
        for t in R.BAD_TARGETS:
            assert not R.live_mask(np.array([v], F32), [N if t is None else t], N)[0], (v, t)
    assert R.live_mask(None, [0, 3, -1, 4, -2 ** 31, 2 ** 31 - 1], N).tolist() == [True, True, False, False, False, False]
    assert not R.live_mask(np.array([0xffc00001, 0x7f800001], np.uint32).view(F32), [0, 0], N).any()   # NaNs with payloads


@pytest.mark.parametrize("with_edges", [True, False], ids=["edges", "no-edges"])
@pytest.mark.parametrize("N,K,seed", [(1, 1, 0), (5, 2, 1), (7, 9, 2), (13, 6, 3), (40, 0, 4)])
def test_reference_equals_a_per_target_loop(N, K, seed, with_edges):
    rng = np.random.default_rng(seed)
    if K > 0:
        nlist, edges = R.special_batch(rng, N, K, p_dead=0.25, p_bad=0.3)
        # small inputs: plant every special value by hand as well
        flat_n, flat_e = nlist.reshape(-1), edges.reshape(-1)
        vals = R.DEAD_VALUES + R.LIVE_VALUES
        for i in range(min(len(vals), flat_e.shape[0])):
            flat_e[-1 - i] = vals[i]
    else:
        flat_n = rng.integers(-2, N + 2, 150).astype(np.int32)        # CSR form: no K; out-of-range targets among them
        flat_e = R.special_edges(rng, 150, 0.25, 0.05)
    e = flat_e if with_edges else None
    ptr, eid, nc = R.incoming_lists(flat_n, e, N, K)
    lp, le, lc = _loop_lists(flat_n.tolist(), None if e is None else flat_e.tolist(), N, K)
    assert ptr.tolist() == lp and eid.tolist() == le
    assert (nc is None and lc is None) or nc.tolist() == lc
    assert ptr.dtype == np.int64 and eid.dtype == np.int64
    perm, pos, d_c, n_live = R.live_partition(flat_e)
    qp, qs, qd, qn = _loop_partition(flat_e.tolist())
    assert perm.tolist() == qp and pos.tolist() == qs and n_live == qn
    np.testing.assert_array_equal(d_c.view(np.uint32), np.array(qd, F32).view(np.uint32))


def test_all_dead_and_empty():
    ptr, eid, nc = R.incoming_lists(np.zeros(10, np.int32), R.dead_edges(np.random.default_rng(0), 10), 5, 2)
    assert ptr.tolist() == [0] * 6 and eid.shape == (0,) and nc.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    ptr, eid, nc = R.incoming_lists(np.zeros(0, np.int32), None, 0, 0)
    assert ptr.tolist() == [0] and eid.shape == (0,) and nc is None
    perm, pos, d_c, n_live = R.live_partition(np.zeros(0, F32))
    assert perm.shape == (0,) and pos.shape == (0,) and d_c.shape == (0,) and n_live == 0
    assert (R.live_edges(np.random.default_rng(1), 500) > 0).all()


def _valid_batch(rng, N, K, p_dead):
    nlist = rng.integers(0, N, (N, K)).astype(np.int32)
    edges = R.special_edges(rng, N * K, p_dead).reshape(N, K)
    return nlist, edges


@pytest.mark.parametrize("N,K,p_dead", [(1, 1, 0.0), (5, 2, 1.0), (300, 16, 0.3), (1100, 7, 0.05)])
def test_reference_equals_the_host_builder_padded(N, K, p_dead):
    from nmrgnn_amd.graph import GraphBatch
    rng = np.random.default_rng(N + K)
    nlist, edges = _valid_batch(rng, N, K, p_dead)
    if p_dead == 1.0:
        edges = R.dead_edges(rng, N * K).reshape(N, K)
    gb = GraphBatch(np.zeros((N, 3), F32), nlist, edges, np.ones(N, F32), device="cpu")
    ptr, eid, nc = R.incoming_lists(nlist, edges, N, K)
    cp, ce = gb.csc()
    np.testing.assert_array_equal(cp.numpy().astype(np.int64), ptr)
    np.testing.assert_array_equal(ce.numpy().astype(np.int64), eid)
    np.testing.assert_array_equal(gb.nlist_c.numpy().reshape(-1).astype(np.int64), nc)


@pytest.mark.parametrize("N,nnz", [(1, 0), (9, 40), (700, 5000)])
def test_reference_equals_the_host_builder_csr(N, nnz):
    from nmrgnn_amd.graph import GraphBatch
    rng = np.random.default_rng(N)
    deg = rng.multinomial(nnz, np.ones(N) / N)
    row_ptr = np.zeros(N + 1, np.int32)
    row_ptr[1:] = np.cumsum(deg)
    col = rng.integers(0, N, nnz).astype(np.int32)
    dist = rng.uniform(0.1, 0.4, nnz).astype(F32)
    gb = GraphBatch.from_csr(np.zeros((N, 3), F32), row_ptr, col, dist, inv_degree=np.ones(N, F32), device="cpu")
    ptr, eid, nc = R.incoming_lists(col, None, N, 0)
    cp, ce = gb.csc()
    np.testing.assert_array_equal(cp.numpy().astype(np.int64), ptr)
    np.testing.assert_array_equal(ce.numpy().astype(np.int64), eid)
    assert nc is None
    # distances are no part of the CSR lists
    assert all(np.array_equal(a, b) for a, b in zip(R.incoming_lists(col, dist, N, 0)[:2], (ptr, eid)))


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def test_an_exact_comparison_tells_right_from_wrong():
    """one fixed input; three wrong answers of the kinds a kernel could give, none of which may pass as the reference's"""
    rng = np.random.default_rng(11)
    N, K = 1100, 8                                   # two scan tiles of 1024 targets
    nlist, edges = R.special_batch(rng, N, K)
    ref = R.incoming_lists(nlist, edges, N, K)
    part = R.live_partition(edges)
    assert _same(ref, R.incoming_lists(nlist.copy(), edges.copy(), N, K))
    ptr, eid, nc = ref
    # 1. two entries of one target in the wrong order (an unstable sort)
    t = int(np.nonzero(np.diff(ptr) >= 2)[0][0])
    wrong = eid.copy()
    wrong[[ptr[t], ptr[t] + 1]] = wrong[[ptr[t] + 1, ptr[t]]]
    assert sorted(wrong.tolist()) == sorted(eid.tolist())
    assert not _same(ref, (ptr, wrong, nc))
    # 2. csc_ptr off by one from a scan tile's edge on (a lost carry)
    wrong = ptr.copy()
    wrong[1024:] -= 1
    assert not _same(ref, (wrong, eid, nc))
    assert np.array_equal(wrong[:1024], ptr[:1024])
    # 3. one dead slot counted as live
    g = int(np.nonzero((edges.reshape(-1) == 0) & (nlist.reshape(-1) >= 0) & (nlist.reshape(-1) < N))[0][5])
    e2 = edges.copy().reshape(-1)
    e2[g] = R.MIN_NORMAL
    got = R.incoming_lists(nlist, e2, N, K)
    assert got[0][-1] == ptr[-1] + 1 and not np.array_equal(got[0], ptr) and not np.array_equal(got[2], nc)
    assert not _same(ref, got)
    p2 = R.live_partition(e2)
    assert p2[3] == part[3] + 1 and not np.array_equal(p2[0], part[0]) and not np.array_equal(p2[1], part[1])
    # and a sign bit in d_c shows in the uint32 view only
    z = np.zeros(1, F32)
    assert np.array_equal(z, -z) and not np.array_equal(z.view(np.uint32), (-z).view(np.uint32))


def test_planted_segments_have_the_lengths_asked_for():
    rng = np.random.default_rng(2)
    N, K = 700, 16
    nlist, edges = R.special_batch(rng, N, K)
    want = {3: 0, 10: 1, 17: 15, 64: 16, 65: 17, 333: 32, 698: 33, 699: 64}
    R.plant_segments(rng, nlist, edges, N, want, spare=100)
    ptr = R.incoming_lists(nlist, edges, N, K)[0]
    assert {t: int(ptr[t + 1] - ptr[t]) for t in want} == want
