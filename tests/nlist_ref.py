"""Exact reference of the neighbour-list builders (knn.hip, knn_cells.hip, cutoff.hip, ragged.hip): NumPy and
integers only.

Every builder orders candidates by the float32 value fmaf(dz, dz, fmaf(dy, dy, dx * dx)) and then by index.  On positions that are
multiples of 1/8 with modest extent that value is exact however it is rounded or contracted, so the whole list can be stated
in integers: positions as int64 "eighths" q8 (float32 position = q8 / 8, exactly), boxes as the nine lower-triangular entries
in eighths, squared distances as integers in units of 1/64.  `check_exact_domain` states the conditions and every test calls
it on its own data.

Conventions (those of the kernels): (distance, index) ascending, self excluded, unused slots (0, 0.0), nlist = base + j,
edges = float32(sqrt(float32(d2 / 64))) * float32(scale), inv_degree = 1 / #(listed local j > 0) or 0, cutoff strict with the
square of the cutoff taken in float32, cutoff rows in ascending index."""
import numpy as np

F32 = np.float32
EXACT = 1 << 24            # integers below this are float32 values


def positions_f32(q8):
    """the float32 positions the kernels get: q8 / 8, exact under check_exact_domain"""
    return (np.asarray(q8, np.int64).astype(np.float64) / 8.0).astype(F32)


def box_f32(box8):
    return (np.asarray(box8, np.int64).astype(np.float64) / 8.0).astype(F32).reshape(9)


def _round_div(a, b):
    """the integer nearest to a / b (b > 0), halves up"""
    return (2 * a + b) // (2 * b)


def min_image_d2(d, box8=None):
    """d [..., 3] int64 displacements r_j - r_i in eighths -> squared length in units of 1/64 (int64).  Open boundaries: |d|^2.
    Periodic: fractional reduction along c, b, a, then the minimum over every translation of [-2, 2]^3 (test_gpu_pbc.py's
    _mic64 in integers).  Along a the minimum over i in [-2, 2] of (x + i ax)^2 is taken at the clipped nearest integer to
    -x / ax (a convex function of i); whole values of k, and of (k, j), are skipped only where z^2, or y^2 + z^2, alone
    already reaches the best found for every pair: nothing is assumed about the box.  The range [-2, 2]^3 is the definition's,
    not worked out from the box: it holds the minimum image for the boxes of these tests (a search over [-9, 9]^3 finds nothing
    shorter on any of them), and a box skewed or thin enough to need a wider range is outside what this file states."""
    d = np.asarray(d, np.int64)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    if box8 is None:
        return dx * dx + dy * dy + dz * dz
    ax, _, _, bx, by, _, cx, cy, cz = (int(v) for v in np.asarray(box8).reshape(9))
    s = _round_div(dz, cz)
    dx, dy, dz = dx - s * cx, dy - s * cy, dz - s * cz
    s = _round_div(dy, by)
    dx, dy = dx - s * bx, dy - s * by
    s = _round_div(dx, ax)
    dx = dx - s * ax
    assert max(np.abs(dx).max(initial=0), np.abs(dy).max(initial=0), np.abs(dz).max(initial=0)) + 2 * (abs(ax) + abs(bx) + abs(cx)
               + abs(by) + abs(cy) + abs(cz)) < 1 << 14          # squares and their sums fit int32
    dx, dy, dz = dx.astype(np.int32), dy.astype(np.int32), dz.astype(np.int32)
    best = None
    for k in (0, -1, 1, -2, 2):
        z = dz + np.int32(k * cz)
        z2 = z * z
        if best is not None and not (z2 < best).any():
            continue
        for j in (0, -1, 1, -2, 2):
            y = dy + np.int32(k * cy + j * by)
            yz = y * y + z2
            if best is not None and not (yz < best).any():
                continue
            x = dx + np.int32(k * cx + j * bx)
            i = np.clip((-2 * x + ax) // (2 * ax), -2, 2).astype(np.int32)
            x = x + i * np.int32(ax)
            cand = x * x + yz
            best = cand if best is None else np.minimum(best, cand)
    return best.astype(np.int64)


def d2_rows(q8, rows, box8=None):
    """[len(rows), n] int64: squared distance (1/64) from every requested row to every atom of the frame"""
    q8 = np.asarray(q8, np.int64)
    return min_image_d2(q8[None, :, :] - q8[np.asarray(rows), None, :], box8)


def d2_pairs(q8, i, j, box8=None):
    q8 = np.asarray(q8, np.int64)
    return min_image_d2(q8[j] - q8[i], box8)


def knn_top(q8, kmax, box8=None, rows=None, chunk=256):
    """the min(kmax, n - 1) smallest (d2, j), j != i, of every requested row, in that order -> (j, d2), both [rows, kk] int64"""
    q8 = np.asarray(q8, np.int64)
    n = q8.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    kk = min(kmax, n - 1)
    out_j = np.zeros((len(rows), kk), np.int64)
    out_d = np.zeros((len(rows), kk), np.int64)
    if kk == 0:
        return out_j, out_d
    big = np.iinfo(np.int64).max
    for r0 in range(0, len(rows), chunk):
        rr = rows[r0:r0 + chunk]
        key = d2_rows(q8, rr, box8) * n + np.arange(n)        # (d2, j) in one integer: d2 * n + j
        key[np.arange(len(rr)), rr] = big
        if kk < n - 1:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key = np.sort(key, axis=1)[:, :kk]
        out_j[r0:r0 + len(rr)] = key % n
        out_d[r0:r0 + len(rr)] = key // n
    return out_j, out_d


def edge_value(d2, scale):
    """sqrtf(d2) * scale as the kernels compute it: every step in float32, each correctly rounded"""
    return np.sqrt(np.asarray(d2).astype(F32) / F32(64.0)) * F32(scale)


def inv_degree_value(count):
    count = np.asarray(count)
    with np.errstate(divide="ignore"):
        return np.where(count > 0, F32(1.0) / count.astype(F32), F32(0.0)).astype(F32)


def knn_format(top_j, top_d2, K, base=0, scale=0.1):
    """(nlist [r, K] int32, edges [r, K] float32, inv_degree [r] float32) from the lists of knn_top (kmax >= K)"""
    r, kk = top_j.shape
    k = min(K, kk)
    nlist = np.zeros((r, K), np.int32)
    edges = np.zeros((r, K), F32)
    nlist[:, :k] = base + top_j[:, :k]
    edges[:, :k] = edge_value(top_d2[:, :k], scale)
    return nlist, edges, inv_degree_value((top_j[:, :k] > 0).sum(1))


def knn(q8, K, box8=None, rows=None, base=0, scale=0.1):
    j, d2 = knn_top(q8, K, box8, rows)
    return knn_format(j, d2, K, base, scale)


def cutoff2_f32(cutoff):
    """the float32 square cutoff_launch hands the kernels"""
    return F32(cutoff) * F32(cutoff)


def cutoff(q8, cutoff, box8=None, base=0, scale=0.1, chunk=256):
    """one frame: deg [n] int32, col [nnz] int32 (ascending in each row), dist [nnz] float32, inv_degree [n] float32"""
    q8 = np.asarray(q8, np.int64)
    n = q8.shape[0]
    c2 = cutoff2_f32(cutoff)
    deg = np.zeros(n, np.int32)
    pos_cnt = np.zeros(n, np.int64)
    cols, dists = [], []
    for r0 in range(0, n, chunk):
        rr = np.arange(r0, min(n, r0 + chunk))
        d2 = d2_rows(q8, rr, box8)
        hit = (d2.astype(F32) / F32(64.0)) < c2
        hit[np.arange(len(rr)), rr] = False
        deg[rr] = hit.sum(1)
        pos_cnt[rr] = hit[:, 1:].sum(1)
        ri, cj = np.nonzero(hit)                              # row-major: ascending j inside each row
        cols.append((base + cj).astype(np.int32))
        dists.append(edge_value(d2[ri, cj], scale))
    col = np.concatenate(cols) if cols else np.zeros(0, np.int32)
    dist = np.concatenate(dists) if dists else np.zeros(0, F32)
    return deg, col, dist.astype(F32), inv_degree_value(pos_cnt)


def cutoff_batch(frames, cutoff_, scale=0.1):
    """frames: a list of (q8, box8 or None), concatenated along the rows -> dict of deg, row_ptr, col, dist, inv_degree, row_of"""
    parts, base = [], 0
    for q8, box8 in frames:
        parts.append(cutoff(q8, cutoff_, box8, base, scale))
        base += len(q8)
    deg = np.concatenate([p[0] for p in parts])
    return dict(deg=deg, row_ptr=scan(deg), col=np.concatenate([p[1] for p in parts]),
                dist=np.concatenate([p[2] for p in parts]), inv_degree=np.concatenate([p[3] for p in parts]),
                row_of=np.repeat(np.arange(len(deg), dtype=np.int32), deg))


def scan(v):
    """ng_exclusive_scan_i32: out[0 .. n] exclusive prefix sums, out[n] the total; summed in int64, then cast"""
    out = np.zeros(len(v) + 1, np.int64)
    np.cumsum(np.asarray(v, np.int64), out=out[1:])
    assert out[-1] < 1 << 31
    return out.astype(np.int32)


def sample_rows(n, seed, count=2048):
    """the rows of a large frame that are checked for completeness: the first 256, the last 256 and 1536 seeded ones"""
    if n <= count:
        return np.arange(n)
    mid = np.random.default_rng(seed).choice(np.arange(256, n - 256), count - 512, replace=False)
    return np.concatenate([np.arange(256), np.sort(mid), np.arange(n - 256, n)])


def check_exact_domain(q8, box8=None, kth_d2=None, cutoff=None):
    """asserts the conditions under which the kernels' float32 chain equals the integers of this file:
      - every coordinate, every coordinate difference and every box entry is below 2^24 in eighths (float32 values; c - q
        exact);
      - diagonal box entries are powers of two (1 / L, d * (1 / L), rintf and the fused wrap steps are exact) and the box is
        orthorhombic or reduced;
      - the squared distance that decides a list (the K-th neighbour's of every checked row, 64 * cutoff^2) is below 2^24 in
        units of 1/64: all partial sums of the chain are then integers below 2^24.  A candidate beyond that bound stays
        beyond it, because fl(x * x) and fmaf are monotone and 2^24 is a float32 value."""
    q8 = np.asarray(q8)
    assert q8.dtype == np.int64 and q8.ndim == 2 and q8.shape[1] == 3
    if q8.size:
        assert np.abs(q8).max() < EXACT, "coordinate beyond 24 bits in eighths"
        assert (q8.max(0) - q8.min(0)).max() < EXACT, "coordinate difference beyond 24 bits in eighths"
    if box8 is not None:
        b = np.asarray(box8).reshape(9)
        assert b.dtype == np.int64 and np.abs(b).max() < EXACT
        ax, z0, z1, bx, by, z2, cx, cy, cz = (int(v) for v in b)
        assert z0 == z1 == z2 == 0, "box not lower-triangular"
        for L in (ax, by, cz):
            assert L > 0 and L & (L - 1) == 0, "box length not a power of two"
        assert 2 * abs(bx) <= ax and 2 * abs(cx) <= ax and 2 * abs(cy) <= by, "box not reduced"
    if kth_d2 is not None and np.size(kth_d2):
        assert int(np.max(kth_d2)) < EXACT, "K-th squared distance beyond 24 bits"
    if cutoff is not None:
        assert float(cutoff2_f32(cutoff)) * 64.0 < EXACT, "squared cutoff beyond 24 bits"
    return True


def check_knn_rows(q8, K, nlist, edges, inv_degree, box8=None, base=0, scale=0.1):
    """row-wise invariants of one frame's kNN lists, O(n K), every row: indices inside the frame, no self neighbour, no index
    twice, (d2, j) strictly ascending along the row, edges the expression above for the neighbour LISTED in the slot,
    inv_degree, padding only where n - 1 < K"""
    q8 = np.asarray(q8, np.int64)
    n = q8.shape[0]
    assert nlist.shape == (n, K) and edges.shape == (n, K) and inv_degree.shape == (n,)
    kk = min(K, n - 1)
    assert not nlist[:, kk:].any() and not edges[:, kk:].view(np.uint32).any(), "padding is (0, 0.0)"
    loc = nlist[:, :kk].astype(np.int64) - base
    assert ((loc >= 0) & (loc < n)).all(), "index outside the frame"
    i = np.arange(n)[:, None]
    assert (loc != i).all(), "self neighbour"
    d2 = d2_pairs(q8, np.broadcast_to(i, loc.shape), loc, box8)
    key = d2 * n + loc
    assert (np.diff(key, axis=1) > 0).all(), "(d2, j) not strictly ascending (an index twice, or out of order)"
    np.testing.assert_array_equal(edges[:, :kk], edge_value(d2, scale), err_msg="edges of the listed neighbours")
    np.testing.assert_array_equal(inv_degree, inv_degree_value((loc > 0).sum(1)), err_msg="inv_degree")
    return d2


# ------------------------------------------------------------------------------------------------ data families (eighths, seeded)
def _spread_side(n, density=0.1):
    return max(int(np.ceil(8.0 * (n / density) ** (1.0 / 3.0))), 8)


def family(kind, n, seed):
    """open-boundary positions q8 [n, 3] int64:
      ties    an integer grid (whole Angstrom) with about n / 4 sites: duplicates (d2 = 0) and equal-distance shells
      spread  a 1/8 grid at about 0.1 atoms per cubic Angstrom: few ties
      offset  spread shifted by (+4096, -2048, +512) Angstrom
      plane   spread's x and y over a square of 300 Angstrom, one z
      line    points over 8192 Angstrom of the x axis
      point   every atom on one point
      blobs   30 far-apart blobs (centres over 2000 Angstrom, 6 Angstrom wide)
      distinct  n different sites of a whole-Angstrom grid: no two atoms closer than 1 Angstrom
      atom0   ties, with atom 0 moved to the middle of the grid; atom0far: atom 0 moved 100 Angstrom away"""
    rng = np.random.default_rng([seed, n, sum(map(ord, kind))])
    if kind in ("ties", "atom0", "atom0far"):
        side = int(np.ceil((n / 4.0) ** (1.0 / 3.0))) + 1
        q = rng.integers(0, side, (n, 3)) * 8
        if kind == "atom0":
            q[0] = (side // 2) * 8
        elif kind == "atom0far":
            q[0] = -800
    elif kind == "distinct":
        side = int(np.ceil((2.0 * n) ** (1.0 / 3.0))) + 1
        pick = rng.choice(side ** 3, n, replace=False)
        q = np.stack([pick // (side * side), (pick // side) % side, pick % side], axis=1) * 8
    elif kind in ("spread", "offset"):
        q = rng.integers(0, _spread_side(n), (n, 3))
        if kind == "offset":
            q = q + np.array([4096, -2048, 512]) * 8
    elif kind == "plane":
        q = rng.integers(0, 300 * 8, (n, 3))
        q[:, 2] = 34
    elif kind == "line":
        q = np.zeros((n, 3), np.int64)
        q[:, 0] = rng.integers(0, 8192 * 8, n)
    elif kind == "point":
        q = np.tile(np.array([[1000, -24, 8]]), (n, 1))
    elif kind == "blobs":
        centres = rng.integers(0, 2000 * 8, (30, 3))
        q = centres[rng.integers(0, 30, n)] + np.rint(rng.standard_normal((n, 3)) * 48.0).astype(np.int64)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(q, dtype=np.int64)


def periodic_family(n, seed, diag, off=(0, 0, 0), kind="spread", moved=0.3, far=3):
    """(q8 [n, 3], box8 [9]) of a periodic frame: box diagonal ``diag`` (Angstrom, each from {8, 16, 32}), off-diagonals
    (b_x, c_x, c_y) ``off`` in eighths; atoms on the 1/8 grid of the cuboid [0, a_x) x [0, b_y) x [0, c_z) (``ties``: on its
    whole-Angstrom grid; ``cluster``: inside a cube of a quarter of the shortest edge, so that no wrapped pair reaches half the
    thinnest width), 30 % of them then moved by up to +-3 box vectors"""
    rng = np.random.default_rng([seed, n, int(diag[0]), int(diag[1]), int(diag[2])])
    d8 = np.array(diag, np.int64) * 8
    box8 = np.array([d8[0], 0, 0, off[0], d8[1], 0, off[1], off[2], d8[2]], np.int64)
    if kind == "ties":
        q = rng.integers(0, np.array(diag), (n, 3)) * 8
    elif kind == "cluster":
        q = rng.integers(0, int(d8.min()) // 4, (n, 3)) + d8 // 2
    else:
        q = rng.integers(0, d8, (n, 3))
    shift = rng.integers(-far, far + 1, (n, 3)) * (rng.random((n, 1)) < moved)
    return np.ascontiguousarray(q + shift @ box8.reshape(3, 3), dtype=np.int64), box8


def widths(box8):
    """perpendicular widths of the box along a, b, c in Angstrom (float64)"""
    v = np.asarray(box8, np.float64).reshape(3, 3) / 8.0
    vol = abs(np.linalg.det(v))
    return np.array([vol / np.linalg.norm(np.cross(v[1], v[2])), vol / np.linalg.norm(np.cross(v[2], v[0])),
                     vol / np.linalg.norm(np.cross(v[0], v[1]))])


def grid_cells(n, K, box8):
    """cells per axis of the periodic cell grid by the rule of knn_cells.hip: cell edge 0.5 (K V / n)^(1/3), cells per axis =
    floor(perpendicular width / edge), at least 1 (float64 here; the cases keep away from the rounding of the quotient)"""
    vol = abs(np.linalg.det(np.asarray(box8, np.float64).reshape(3, 3) / 8.0))
    quot = widths(box8) / (0.5 * (K * vol / n) ** (1.0 / 3.0))
    assert (np.abs(quot - np.rint(quot)) > 1e-3).all(), "cell count on a rounding edge"
    return tuple(int(max(np.floor(x), 1)) for x in quot)
