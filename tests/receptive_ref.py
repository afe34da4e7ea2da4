"""NumPy integer reference of receptive-field pruning (csrc/prune.hip): hops, kept atoms, the pruned
lists in both forms, the pruned graph_ptr and the expanded edge gradient.  Plain loops and index arithmetic, no shared
code with the library.  The GPU tests compare bit for bit against it; the host tests check it by hand cases and against
the float64 model."""
import numpy as np


def live_mask(nlist, edges, N):
    """the rule of ng_build_incoming_lists: edges > 0 and 0 <= target < N"""
    nlist = np.asarray(nlist, np.int64)
    return (np.asarray(edges) > 0) & (nlist >= 0) & (nlist < N)


def hops_padded(nlist, edges, seed, hops):
    """hop [N]: steps i -> nlist[i, k] along live entries from the nearest selected atom, -1 beyond ``hops``"""
    nlist = np.asarray(nlist, np.int64)
    N = nlist.shape[0]
    live = live_mask(nlist, edges, N)
    hop = np.where(np.asarray(seed) != 0, 0, -1).astype(np.int32)
    for d in range(1, hops + 1):
        rows = np.nonzero(hop == d - 1)[0]
        if len(rows) == 0:
            break
        t = nlist[rows][live[rows]]
        t = t[hop[t] == -1]
        hop[t] = d
    return hop


def to_csr(nlist, edges):
    """(row_ptr, col, dist, row_of) of the padded lists with the edges <= 0 slots dropped (GraphBatch.to_csr)"""
    keep = np.asarray(edges) > 0
    deg = keep.sum(1)
    row_ptr = np.zeros(len(deg) + 1, np.int32)
    row_ptr[1:] = np.cumsum(deg)
    return row_ptr, np.asarray(nlist)[keep].astype(np.int32), np.asarray(edges)[keep], np.repeat(np.arange(len(deg)), deg).astype(np.int32)


def hops_csr(row_ptr, col, dist, seed, hops):
    N = len(row_ptr) - 1
    hop = np.where(np.asarray(seed) != 0, 0, -1).astype(np.int32)
    for d in range(1, hops + 1):
        for i in np.nonzero(hop == d - 1)[0]:
            for e in range(row_ptr[i], row_ptr[i + 1]):
                t = int(col[e])
                if dist[e] > 0 and 0 <= t < N and hop[t] == -1:
                    hop[t] = d
    return hop


def _index(hop):
    flag = (hop >= 0).astype(np.int64)
    idx = np.zeros(len(hop) + 1, np.int64)
    idx[1:] = np.cumsum(flag)
    return idx


def _graphs(idx, graph_ptr):
    gp = np.asarray(graph_ptr, np.int64)
    counts = np.diff(idx[gp])
    gi = np.nonzero(counts > 0)[0].astype(np.int32)
    return np.concatenate([[0], np.cumsum(counts[gi])]).astype(np.int32), gi


def prune_padded(atoms, nlist, edges, inv_degree, graph_ptr, seed, hops):
    """dict of the pruned padded batch: hop_full, idx, keep, hop, atoms, nlist, edges, inv_degree, graph_ptr, graph_index"""
    nlist = np.asarray(nlist, np.int64)
    edges = np.asarray(edges, np.float32)
    N, K = nlist.shape
    hop = hops_padded(nlist, edges, seed, hops)
    idx = _index(hop)
    keep = np.nonzero(hop >= 0)[0]
    live = live_mask(nlist, edges, N)
    gp = np.asarray(graph_ptr, np.int64)
    # a slot stays when it is live and its row is closer than ``hops``; every other slot of a kept row is dead: (the first
    # kept atom of the row's graph, 0.0)
    stays = (hop[keep] < hops)[:, None] & live[keep]
    g = np.searchsorted(gp, keep, side="right") - 1
    dead = idx[gp[g]]
    nl = np.where(stays, idx[np.clip(nlist[keep], 0, N - 1)], dead[:, None]).astype(np.int32)
    ed = np.where(stays, edges[keep], np.float32(0)).astype(np.float32)
    assert not stays.any() or (hop[nlist[keep][stays]] >= 0).all()      # every target of a kept slot is a kept atom
    gp_p, gi = _graphs(idx, gp)
    return dict(hop_full=hop, idx=idx, keep=keep.astype(np.int32), hop=hop[keep], atoms=np.asarray(atoms, np.float32)[keep],
                nlist=nl, edges=ed, inv_degree=np.asarray(inv_degree, np.float32).reshape(-1)[keep], graph_ptr=gp_p,
                graph_index=gi, hops=hops)


def prune_csr(atoms, row_ptr, col, dist, inv_degree, graph_ptr, seed, hops):
    """the same for the CSR form: row_ptr, nlist (= col), edges (= dist), row_of of the pruned batch"""
    N = len(row_ptr) - 1
    hop = hops_csr(row_ptr, col, dist, seed, hops)
    idx = _index(hop)
    keep = np.nonzero(hop >= 0)[0]
    rp, cp, dp, ro = [0], [], [], []
    for r, i in enumerate(keep):
        if hop[i] < hops:
            for e in range(row_ptr[i], row_ptr[i + 1]):
                t = int(col[e])
                ok = dist[e] > 0 and 0 <= t < N
                cp.append(idx[t] if ok else r)
                dp.append(dist[e] if ok else 0.0)
                ro.append(r)
        rp.append(len(cp))
    gp_p, gi = _graphs(idx, graph_ptr)
    return dict(hop_full=hop, idx=idx, keep=keep.astype(np.int32), hop=hop[keep], atoms=np.asarray(atoms, np.float32)[keep],
                row_ptr=np.asarray(rp, np.int32), nlist=np.asarray(cp, np.int32), edges=np.asarray(dp, np.float32),
                row_of=np.asarray(ro, np.int32), inv_degree=np.asarray(inv_degree, np.float32).reshape(-1)[keep],
                graph_ptr=gp_p, graph_index=gi, hops=hops)


def expand_edge_grad_padded(p, nlist, edges, de_p):
    """parent-shaped [N, K]: the pruned value where the slot was kept, +0.0 elsewhere"""
    nlist = np.asarray(nlist, np.int64)
    N, K = nlist.shape
    live = live_mask(nlist, edges, N)
    de_p = np.asarray(de_p).reshape(-1, K)
    out = np.zeros((N, K), de_p.dtype)
    keep = np.asarray(p["keep"], np.int64)
    stays = (p["hop"] < p["hops"])[:, None] & live[keep]
    out[keep] = np.where(stays, de_p, 0)
    return out


def expand_edge_grad_csr(p, row_ptr, col, dist, de_p):
    N = len(row_ptr) - 1
    de_p = np.asarray(de_p).reshape(-1)
    out = np.zeros(len(col), de_p.dtype)
    for r, i in enumerate(p["keep"]):
        if p["hop"][r] < p["hops"]:
            for j, e in enumerate(range(row_ptr[i], row_ptr[i + 1])):
                if dist[e] > 0 and 0 <= col[e] < N:
                    out[e] = de_p[p["row_ptr"][r] + j]
    return out


def csr_to_padded(row_ptr, col, dist, K=None):
    """padded (nlist, edges) of CSR lists, rows padded with (0, 0.0) to the largest degree (the float64 model reads padded lists)"""
    row_ptr = np.asarray(row_ptr, np.int64)
    deg = np.diff(row_ptr)
    K = max(int(deg.max()) if len(deg) else 0, 1) if K is None else K
    N = len(deg)
    rows = np.repeat(np.arange(N), deg)
    slot = np.arange(len(col)) - row_ptr[rows]
    nlist = np.zeros((N, K), np.int64)
    edges = np.zeros((N, K), np.asarray(dist).dtype)
    nlist[rows, slot] = col
    edges[rows, slot] = dist
    return nlist, edges, rows, slot


# ---- hand cases ---------------------------------------------------------------------------------------------------------
def path_case(n=12):
    """a path 0 - 1 - ... - 11 with K = 2: atom i lists i - 1 and i + 1 (the ends one padded slot)"""
    nlist = np.zeros((n, 2), np.int32)
    edges = np.zeros((n, 2), np.float32)
    for i in range(n):
        k = 0
        for j in (i - 1, i + 1):
            if 0 <= j < n:
                nlist[i, k], edges[i, k] = j, 0.1 + 0.01 * abs(i - j) + 0.001 * i
                k += 1
    return nlist, edges


def asymmetric_case(n=8):
    """atom 5 lists atom 0; atom 0 lists only atom 1; nobody else lists anything"""
    nlist = np.zeros((n, 2), np.int32)
    edges = np.zeros((n, 2), np.float32)
    nlist[5, 0], edges[5, 0] = 0, 0.15
    nlist[0, 0], edges[0, 0] = 1, 0.12
    return nlist, edges


def padded_row_case(n=6):
    """atom 3 has only padded (0, 0.0) slots; atom 4 lists atom 3"""
    nlist = np.zeros((n, 2), np.int32)
    edges = np.zeros((n, 2), np.float32)
    nlist[4, 0], edges[4, 0] = 3, 0.11
    return nlist, edges


def hand_batch(nlist, edges, C=4, seed=0):
    """atoms / inv_degree around hand lists"""
    rng = np.random.default_rng(seed)
    N = nlist.shape[0]
    atoms = np.eye(C, dtype=np.float32)[rng.integers(0, C, N)]
    cnt = ((nlist > 0) & (edges > 0)).sum(1)
    inv = np.where(cnt > 0, 1.0 / np.maximum(cnt, 1), 0.0).astype(np.float32)
    return atoms, inv
