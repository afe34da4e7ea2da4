"""tests/nlist_ref.py checked on the CPU: the exact statement that test_gpu_nlist_exact.py holds the neighbour-list builders to.

The integer reference against a plain Python triple loop (open, orthorhombic and triclinic boundaries, duplicated points),
against nmrgnn_amd.structure.knn_graph (cKDTree) and a float64 minimum-image search on the rows without ties, and against an
emulation of the kernels' own float32 expression (dx * dx rounded, two fused steps, DispOrtho's and DispTric's wraps) on every
data family of the GPU tests; check_exact_domain refuses data outside the exact regime; the scan helper against a loop."""
import itertools

import numpy as np
import pytest

import nlist_ref as R

F32 = np.float32
BOXES = {"open": None, "ortho": ((8, 16, 8), (0, 0, 0)), "tric": ((16, 8, 8), (-64, 40, 32)), "thin": ((32, 16, 8), (128, -96, 64))}


def _frame(kind, n, seed, dup=False):
    if BOXES[kind] is None:
        q, box8 = R.family("ties" if dup else "spread", n, seed), None
    else:
        q, box8 = R.periodic_family(n, seed, BOXES[kind][0], BOXES[kind][1], kind="ties" if dup else "spread")
    if dup:
        q[n // 2:] = q[:n - n // 2]                       # every point twice
    return q, box8


def _loop_d2(q, box8):
    """[n][n] Python ints: the definition, pair by pair and translation by translation"""
    n = len(q)
    out = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            d = [int(q[j][a]) - int(q[i][a]) for a in range(3)]
            if box8 is None:
                out[i][j] = d[0] ** 2 + d[1] ** 2 + d[2] ** 2
                continue
            v = [[int(x) for x in box8[3 * r:3 * r + 3]] for r in range(3)]
            for r in (2, 1, 0):                            # fractional reduction along c, b, a
                s = (2 * d[r] + v[r][r]) // (2 * v[r][r])
                d = [d[a] - s * v[r][a] for a in range(3)]
            best = None
            for t in itertools.product(range(-2, 3), repeat=3):
                e = [d[a] + t[0] * v[0][a] + t[1] * v[1][a] + t[2] * v[2][a] for a in range(3)]
                e2 = e[0] ** 2 + e[1] ** 2 + e[2] ** 2
                best = e2 if best is None or e2 < best else best
            out[i][j] = best
    return out


@pytest.mark.parametrize("dup", [False, True], ids=["distinct", "duplicated"])
@pytest.mark.parametrize("kind", list(BOXES))
def test_reference_equals_a_python_loop(kind, dup):
    n, K, cut = 40, 7, 3.0
    q, box8 = _frame(kind, n, 5, dup)
    R.check_exact_domain(q, box8, cutoff=cut)
    d2 = _loop_d2(q, box8)
    np.testing.assert_array_equal(R.d2_rows(q, np.arange(n), box8), np.array(d2, np.int64))
    nl, ed, inv = R.knn(q, K, box8, base=80)
    co = R.cutoff_batch([(q, box8)], cut)
    c2 = F32(cut) * F32(cut)
    cols = []
    for i in range(n):
        order = sorted((d2[i][j], j) for j in range(n) if j != i)
        assert nl[i].tolist() == [80 + j for _, j in order[:K]]
        assert ed[i].tolist() == [F32(np.sqrt(F32(d / 64.0))) * F32(0.1) for d, _ in order[:K]]
        cnt = sum(1 for _, j in order[:K] if j > 0)
        assert inv[i] == (F32(1) / F32(cnt) if cnt else 0)
        row = [j for j in range(n) if j != i and F32(d2[i][j] / 64.0) < c2]
        assert co["deg"][i] == len(row)
        lo, hi = co["row_ptr"][i], co["row_ptr"][i + 1]
        assert co["col"][lo:hi].tolist() == row and (co["row_of"][lo:hi] == i).all()
        assert co["dist"][lo:hi].tolist() == [F32(np.sqrt(F32(d2[i][j] / 64.0))) * F32(0.1) for j in row]
        cp = sum(1 for j in row if j > 0)
        assert co["inv_degree"][i] == (F32(1) / F32(cp) if cp else 0)
        cols += row
    assert len(cols) == co["row_ptr"][-1] == len(co["col"])
    if dup:
        assert (np.array(d2) == 0).sum() > n            # the duplicates are there: d2 = 0 off the diagonal
    # the row-wise invariants accept the reference and notice a swap, a self neighbour and a wrong edge
    R.check_knn_rows(q, K, nl, ed, inv, box8, base=80)
    for breakit in ("swap", "self", "edge", "inv"):
        a, b, c = nl.copy(), ed.copy(), inv.copy()
        if breakit == "swap":
            a[3, [1, 2]] = a[3, [2, 1]]
        elif breakit == "self":
            a[3, 0] = 80 + 3
        elif breakit == "edge":
            b[3, 2] = np.nextafter(b[3, 2], F32(9))
        else:
            c[3] = np.nextafter(c[3], F32(9))
        with pytest.raises(AssertionError):
            R.check_knn_rows(q, K, a, b, c, box8, base=80)


def test_padding_and_small_frames():
    for n in (1, 2, 5):
        q = R.family("ties", n, 1)
        nl, ed, inv = R.knn(q, 6, base=10)
        assert nl.shape == (n, 6) and not nl[:, n - 1:].any() and not ed[:, n - 1:].any()
        assert (nl[:, :n - 1] >= 10).all()
        R.check_knn_rows(q, 6, nl, ed, inv, base=10)
        assert (inv == R.inv_degree_value(((nl[:, :n - 1] - 10) > 0).sum(1))).all()
    assert R.knn(R.family("ties", 1, 1), 4)[2].tolist() == [0.0]


def _tie_free(d2, K):
    s = np.sort(d2, axis=1)[:, :K + 2]                    # column 0 is the atom itself
    return (np.diff(s, axis=1) > 0).all(1)


def test_reference_equals_ckdtree_on_rows_without_ties():
    pytest.importorskip("scipy")
    from nmrgnn_amd.structure import inv_degree_of, knn_graph
    n, K = 500, 8
    q = R.family("spread", n, 2)
    free = _tie_free(R.d2_rows(q, np.arange(n)), K)
    assert free.mean() > 0.3
    nl, ed, inv = R.knn(q, K)
    ref_nl, ref_ed = knn_graph(R.positions_f32(q), K, 0.1)
    np.testing.assert_array_equal(nl[free], ref_nl[free])
    np.testing.assert_allclose(ed[free], ref_ed[free], rtol=3e-7, atol=0)
    np.testing.assert_array_equal(inv[free], inv_degree_of(ref_nl)[free])


@pytest.mark.parametrize("kind", ["ortho", "tric", "thin"])
def test_reference_equals_a_float64_minimum_image_search(kind):
    n, K = 300, 8
    q, box8 = _frame(kind, n, 3)
    vecs = box8.reshape(3, 3) / 8.0
    p = q / 8.0
    d = p[None, :, :] - p[:, None, :]
    d -= np.rint(d @ np.linalg.inv(vecs)) @ vecs
    best = np.full((n, n), np.inf)
    for t in itertools.product(range(-2, 3), repeat=3):
        best = np.minimum(best, ((d + np.array(t, float) @ vecs) ** 2).sum(-1))
    d2 = R.d2_rows(q, np.arange(n), box8)
    np.testing.assert_array_equal(d2, np.rint(best * 64.0).astype(np.int64))          # multiples of 1/64: exact in float64
    free = _tie_free(d2, K)
    assert free.mean() > 0.3
    np.fill_diagonal(best, np.inf)
    order = np.argsort(best, axis=1, kind="stable")[:, :K]
    np.testing.assert_array_equal(R.knn(q, K, box8)[0][free], order[free])


# ------------------------------------------------------------------------------------------------ the kernels' float32 chain
def _fma(a, b, c):
    """fmaf on float32 arrays: the product and sum in float64 (exact for these magnitudes or rounded once more: the chain is
    only claimed where it is exact), rounded to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _dist2(dx, dy, dz):
    return _fma(dz, dz, _fma(dy, dy, (dx * dx).astype(F32)))


def _chain_f32(q8, rows, box8, tric, reach=None):
    """the squared distances of pbc_dist2 after DispOpen / DispOrtho / DispTric, in NumPy float32.  ``reach``: (nk, nj, ni) of
    DispTric's image search instead of the reach DispTric::load works out from the box"""
    p = R.positions_f32(q8)
    dx, dy, dz = [(p[None, :, a] - p[rows, None, a]).astype(F32) for a in range(3)]
    if box8 is None:
        return _dist2(dx, dy, dz)
    b = R.box_f32(box8)
    ax, bx, by, cx, cy, cz = b[0], b[3], b[4], b[6], b[7], b[8]
    iax, iby, icz = F32(1) / ax, F32(1) / by, F32(1) / cz
    full = lambda v: np.full_like(dx, v)
    if not tric:
        dx = _fma(full(-ax), np.rint(dx * iax), dx)
        dy = _fma(full(-by), np.rint(dy * iby), dy)
        dz = _fma(full(-cz), np.rint(dz * icz), dz)
        return _dist2(dx, dy, dz)
    s = np.rint(dz * icz)
    dx, dy, dz = _fma(-s, full(cx), dx), _fma(-s, full(cy), dy), _fma(-s, full(cz), dz)
    s = np.rint(dy * iby)
    dx, dy = _fma(-s, full(bx), dx), _fma(-s, full(by), dy)
    s = np.rint(dx * iax)
    dx = _fma(-s, full(ax), dx)
    best = _dist2(dx, dy, dz)
    v = ax * by * cz
    bcx, bcy, bcz = by * cz, -bx * cz, bx * cy - by * cx
    wa = v / np.sqrt(bcx * bcx + bcy * bcy + bcz * bcz, dtype=F32)
    wb = by * cz / np.sqrt(cy * cy + cz * cz, dtype=F32)
    w = min(wa, wb, cz)
    search = best >= F32(0.25) * w * w
    out = best.copy()
    nk, nj, ni = _reach_f32(b) if reach is None else reach
    for k, j, i in itertools.product(range(-nk, nk + 1), range(-nj, nj + 1), range(-ni, ni + 1)):
        ex = _fma(full(k), full(cx), _fma(full(j), full(bx), _fma(full(i), full(ax), dx)))
        ey = _fma(full(k), full(cy), _fma(full(j), full(by), dy))
        ez = _fma(full(k), full(cz), dz)
        out = np.where(search, np.minimum(out, _dist2(ex, ey, ez)), out)
    return out, search


def _reach_f32(b):
    """DispTric::load: the reach of the image search along c, b, a, in float32 as the kernel computes it"""
    ax, bx, by, cx, cy, cz = b[0], b[3], b[4], b[6], b[7], b[8]
    iax, iby, icz = F32(1) / ax, F32(1) / by, F32(1) / cz
    r = F32(0.5) * np.sqrt(ax * ax + by * by + cz * cz, dtype=F32) * F32(1.0001)
    nk = int(r * icz + F32(0.5))
    nj = int(r * iby + F32(0.5) + F32(nk) * abs(cy) * iby)
    ni = max(int(np.ceil((F32(nj) * abs(bx) + F32(nk) * abs(cx)) * iax)), 1)
    return nk, nj, ni


def _assert_chain(q8, box8=None, tric=False, rows=None):
    n = len(q8)
    rows = np.arange(min(n, 200)) if rows is None else rows
    got = _chain_f32(q8, rows, box8, tric)
    search = None
    if tric:
        got, search = got
    d2 = R.d2_rows(q8, rows, box8)
    exact = d2 < R.EXACT
    np.testing.assert_array_equal(got[exact].astype(np.float64) * 64.0, d2[exact].astype(np.float64))
    assert (got[~exact].astype(np.float64) * 64.0 >= R.EXACT).all()          # beyond the bound stays beyond it
    return exact.mean(), search


@pytest.mark.parametrize("kind", ["ties", "spread", "offset", "plane", "line", "point", "blobs", "atom0", "atom0far"])
def test_float32_chain_is_exact_on_open_families(kind):
    q = R.family(kind, 4096, 7)                        # the size of the GPU cases that use every family
    R.check_exact_domain(q, kth_d2=R.knn_top(q, 64, rows=np.arange(200))[1][:, -1])
    frac, _ = _assert_chain(q)
    if kind in ("line", "blobs"):
        assert frac < 1.0                                  # these reach past 2^24: the monotone half of the argument is used


PERIODIC = {"ortho_8_16_32": ((8, 16, 32), (0, 0, 0)), "ortho_32": ((32, 32, 32), (0, 0, 0)),
            "tric_32": ((32, 32, 32), (64, -128, 48)), "tric_thin8": ((32, 32, 8), (64, -40, 24)),
            "tric_cluster": ((32, 32, 32), (64, -128, 48))}


@pytest.mark.parametrize("name", list(PERIODIC))
def test_float32_chain_is_exact_on_periodic_families(name):
    diag, off = PERIODIC[name]
    tric = any(off)
    q, box8 = R.periodic_family(700, 9, diag, off, kind="cluster" if name.endswith("cluster") else "spread")
    R.check_exact_domain(q, box8, kth_d2=R.knn_top(q, 64, box8, rows=np.arange(200))[1][:, -1])
    outside = ((q < 0) | (q >= box8.reshape(3, 3).diagonal())).any(1)
    assert 0.15 < outside.mean() < 0.6                     # atoms moved by box vectors take part
    frac, search = _assert_chain(q, box8, tric)
    assert frac == 1.0
    if name == "tric_thin8":
        assert search.mean() > 0.5                         # the 27-image search runs for most pairs
    if name == "tric_cluster":
        assert not search.any()                            # and here for none


def test_image_search_reach():
    """the usual cells need the 27 neighbouring images and get exactly those; in a box thin along c an image two cells up or
    down can be the nearest, which the reach of DispTric::load covers and a reach of one does not"""
    for diag, off in (((32, 32, 32), (64, -128, 48)), ((16, 16, 16), (32, -40, 24)), ((32, 16, 16), (-128, 64, 24))):
        assert _reach_f32(R.box_f32(R.periodic_family(4, 1, diag, off)[1])) == (1, 1, 1)
    d = 60.0                                               # rhombic dodecahedron, truncated octahedron, b_x = a_x / 4 ...
    for v in ([d, 0, 0, 0, d, 0, d / 2, d / 2, d / 2 ** 0.5], [d, 0, 0, d / 3, d * 8 ** 0.5 / 3, 0, -d / 3, d * 2 ** 0.5 / 3, d * 6 ** 0.5 / 3],
              [d, 0, 0, d / 4, d, 0, -d / 5, 0.3 * d, d], [20, 0, 0, 10, 18, 0, -10, 9, 16]):
        assert _reach_f32(np.array(v, F32)) == (1, 1, 1)
    q, box8 = R.periodic_family(700, 9, (32, 32, 8), (64, -40, 24))
    assert _reach_f32(R.box_f32(box8))[0] >= 2
    rows = np.arange(100)
    d2 = R.d2_rows(q, rows, box8)
    full, _ = _chain_f32(q, rows, box8, True)
    near, _ = _chain_f32(q, rows, box8, True, reach=(1, 1, 1))
    np.testing.assert_array_equal(full.astype(np.float64) * 64.0, d2)
    n64 = near.astype(np.float64) * 64.0
    long = n64 > d2                                        # the figures of DESIGN.md 7.8: 0.9 % of the pairs, up to 16 % in d2
    assert 0.005 < long.mean() < 0.015 and 0.10 < ((n64 - d2)[long] / d2[long]).max() < 0.20


def test_exact_domain_refuses_what_is_outside():
    q = R.family("spread", 50, 1)
    assert R.check_exact_domain(q)
    far = q.copy()
    far[0, 0] = (1 << 22) * 8                              # a coordinate of 2^22 Angstrom
    with pytest.raises(AssertionError):
        R.check_exact_domain(far)
    box = np.array([24 * 8, 0, 0, 0, 128, 0, 0, 0, 128], np.int64)          # a box length of 24: 1 / 24 is not a float32 value
    with pytest.raises(AssertionError):
        R.check_exact_domain(q, box)
    skew = np.array([128, 0, 0, 72, 128, 0, 0, 0, 128], np.int64)           # |b_x| > a_x / 2: not reduced
    with pytest.raises(AssertionError):
        R.check_exact_domain(q, skew)
    with pytest.raises(AssertionError):
        R.check_exact_domain(q, kth_d2=np.array([1 << 24]))
    with pytest.raises(AssertionError):
        R.check_exact_domain(q, cutoff=512.0)
    assert R.check_exact_domain(q, np.array([64, 0, 0, 32, 128, 0, -32, 64, 256], np.int64), kth_d2=[5], cutoff=3.2)


def test_scan_helper_equals_a_loop():
    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 1025):
        v = rng.integers(0, 41, n).astype(np.int32)
        want, run = [], 0
        for x in v.tolist():
            want.append(run)
            run += x
        want.append(run)
        got = R.scan(v)
        assert got.dtype == np.int32 and got.tolist() == want
    big = np.zeros(10, np.int32)
    big[3], big[9] = 2 ** 30, 2 ** 30 - 1 + 2 ** 30 - 2 ** 30       # total 2^31 - 1
    big[5] = 2 ** 31 - 1 - int(big.astype(np.int64).sum())
    assert R.scan(big)[-1] == 2 ** 31 - 1


def test_sample_rows_and_grid_cells():
    r = R.sample_rows(16384, 4)
    assert len(r) == 2048 == len(set(r.tolist())) and (r[:256] == np.arange(256)).all() and (r[-256:] == np.arange(16128, 16384)).all()
    assert (R.sample_rows(4097, 4)[:5] == np.arange(5)).all() and len(R.sample_rows(2048, 1)) == 2048
    box8 = np.array([64, 0, 0, 0, 128, 0, 0, 0, 256], np.int64)
    assert R.grid_cells(64, 40, box8) == (1, 2, 4) and np.allclose(R.widths(box8), [8.0, 16.0, 32.0], rtol=1e-12)


def test_periodic_cell_grids_cover_every_axis_length():
    """axes of 1, 2, 3, 4 and 5 or more cells, odd and even, all occur among the periodic cell-grid cases of
    test_gpu_nlist_exact.py (their ids say which)"""
    from test_gpu_nlist_exact import PERIODIC
    seen = set()
    for p in PERIODIC:
        if p.values[7] == "knn_cells_query":
            seen |= {min(int(c), 5) for c in p.id.split("-cells")[1].split("x")}
    assert seen == {1, 2, 3, 4, 5}, seen
