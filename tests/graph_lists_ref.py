"""Exact reference of the per-batch graph list builders (csrc/graph_ops.hip): NumPy, int64 inside, no import of the package.

What is stated (include/nmrgnn_hip.h: ng_build_incoming_lists, ng_build_live_edges, ng_build_graph_lists):
  live entry     edges[eid] > 0 (NaN, 0, -0 and negative distances are not; +inf is) AND 0 <= target < N; without edges
                 every entry with a target inside [0, N) is live
  incoming lists csc_ptr [N+1] and csc_edge [:csc_ptr[N]]: the live entry ids in a STABLE sort by target
  nlist_c        (padded form, K > 0) the target of a live entry, the atom's own index eid // K otherwise
  live partition of the slots by edges > 0 alone (it never sees the targets): perm = live slots ascending, then dead slots
                 ascending; pos = rank in the compacted order or -1; d_c [:n_live] = the distances of the live slots

The special values every test plants (special_edges, special_batch) are here too, so that the CPU test of this file and the
GPU tests draw from one helper."""
import numpy as np

F32 = np.float32
MIN_NORMAL = F32(1.17549435e-38)
DEAD_VALUES = (F32(0.0), F32(-0.0), F32(-0.3), F32(np.nan))       # not > 0
LIVE_VALUES = (F32(np.inf), MIN_NORMAL)                           # > 0, at the ends of the normal range
BAD_TARGETS = (-1, None, -2 ** 31, 2 ** 31 - 1)                   # None stands for N


def live_mask(edges, targets, N):
    t = np.asarray(targets).astype(np.int64).reshape(-1)
    ok = (t >= 0) & (t < int(N))
    if edges is None:
        return ok
    e = np.asarray(edges, F32).reshape(-1)
    assert e.shape == t.shape
    with np.errstate(invalid="ignore"):
        return (e > 0) & ok


def incoming_lists(nlist_flat, edges, N, K):
    """-> csc_ptr [N+1] int64, csc_edge [total] int64, nlist_c [n_entries] int64 (None when K == 0)"""
    t = np.asarray(nlist_flat).astype(np.int64).reshape(-1)
    live = live_mask(edges, t, N)
    eid = np.nonzero(live)[0].astype(np.int64)
    tgt = t[eid]
    count = np.zeros(int(N), np.int64)
    np.add.at(count, tgt, 1)
    csc_ptr = np.zeros(int(N) + 1, np.int64)
    csc_ptr[1:] = np.cumsum(count)
    csc_edge = eid[np.argsort(tgt, kind="stable")]
    nlist_c = None
    if K > 0:
        assert t.shape[0] == int(N) * K
        nlist_c = np.where(live, t, np.arange(t.shape[0], dtype=np.int64) // K)
    return csc_ptr, csc_edge, nlist_c


def live_partition(edges):
    """-> perm [n] int64, pos [n] int64, d_c [n_live] float32, n_live"""
    e = np.asarray(edges, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        live = e > 0
    li, de = np.nonzero(live)[0].astype(np.int64), np.nonzero(~live)[0].astype(np.int64)
    pos = np.full(e.shape[0], -1, np.int64)
    pos[li] = np.arange(li.shape[0])
    return np.concatenate([li, de]), pos, e[li].copy(), int(li.shape[0])


# ---- test data ----------------------------------------------------------------------------------------------------------

def special_edges(rng, n, p_dead=0.3, p_special=0.02):
    """[n] float32: uniform(0.05, 1) with a fraction p_dead of 0.0 and, each on a fraction p_special of the slots, -0.0, -0.3,
    NaN, +inf and the smallest normal float.  From 1000 slots on every value is present (asserted)."""
    e = rng.uniform(0.05, 1.0, n).astype(F32)
    u = rng.random(n)
    e[u < p_dead] = F32(0.0)
    lo = p_dead
    for v in DEAD_VALUES[1:] + LIVE_VALUES:
        e[(u >= lo) & (u < lo + p_special)] = v
        lo += p_special
    if n >= 1000 and p_dead > 0:
        bits = set(e.view(np.uint32).tolist())
        for v in DEAD_VALUES + LIVE_VALUES:
            assert int(np.array(v, F32).view(np.uint32)) in bits, v
    return e


def dead_edges(rng, n):
    """[n] float32, none of them > 0: every dead value in turn"""
    return np.array(DEAD_VALUES, F32)[rng.integers(0, len(DEAD_VALUES), n)]


def live_edges(rng, n):
    """[n] float32, every one > 0, +inf and the smallest normal float among them"""
    e = rng.uniform(0.05, 1.0, n).astype(F32)
    u = rng.random(n)
    e[u < 0.02] = LIVE_VALUES[0]
    e[(u >= 0.02) & (u < 0.04)] = LIVE_VALUES[1]
    return e


def special_batch(rng, N, K, p_dead=0.3, p_bad=0.02):
    """nlist [N, K] int32, edges [N, K] float32: random targets in [0, N), special_edges, and on a fraction p_bad of the slots
    that hold a positive edge a target of -1, N, -2^31 or 2^31 - 1"""
    n = N * K
    nlist = rng.integers(0, N, n).astype(np.int64)
    edges = special_edges(rng, n, p_dead)
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(edges > 0)[0]
    bad = cand[rng.random(cand.shape[0]) < p_bad]
    vals = np.array([N if v is None else v for v in BAD_TARGETS], np.int64)
    nlist[bad] = vals[np.arange(bad.shape[0]) % len(vals)]
    if n >= 1000 and p_bad > 0:
        assert set(vals.tolist()) <= set(nlist[bad].tolist())
    return nlist.astype(np.int32).reshape(N, K), edges.reshape(N, K)


def plant_segments(rng, nlist, edges, N, want, spare):
    """Give target t exactly want[t] live entries, in place: entries of `nlist` (flat, int) that point at one of the chosen
    targets are sent to `spare` first; then slots drawn from the live ones are pointed at the chosen targets.  With `edges`
    None every in-range entry counts as live."""
    flat = nlist.reshape(-1)
    assert spare not in want
    flat[np.isin(flat, list(want))] = spare
    cand = rng.permutation(np.nonzero(live_mask(None if edges is None else edges.reshape(-1), flat, N))[0])
    assert cand.shape[0] >= sum(want.values())
    at = 0
    for t, c in want.items():
        flat[cand[at:at + c]] = t
        at += c
    return nlist
