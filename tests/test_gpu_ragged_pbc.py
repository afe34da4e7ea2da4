"""Periodic boxes on ragged batches (structures_to_batch(boxes=): ng_knn_graph_ragged_pbc, ng_cutoff_count_ragged_pbc /
ng_cutoff_fill_rows_ragged_pbc, ng_positions_grad(_csr)_ragged_pbc, ng_box_grad(_csr)_ragged): every structure with a boundary
kind of its own, its rows bit for bit what the uniform builders give for it alone with its own box (or without one), the
gradients per structure, the model and autograd on a boxed ragged batch, eval-struct --separate --boxes."""
import csv
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import make_hp

ROOT = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = [1, 2, None, None, 63, 64, 65, 255, 256, 257, 300, 1100, 4096, 4097]      # None: K and K + 1
KS = [5, 16, 40, 64]
STYLES = ["grid", "float"]
OPEN, ORTHO, TRIC = -1, 0, 1


def _np(t):
    return t.detach().cpu().numpy()


def _sizes(K, top=4097):
    s = [K if v is None and i == 2 else K + 1 if v is None else v for i, v in enumerate(SIZES)]
    s = [v for v in s if v <= top]
    rng = np.random.default_rng(K)
    return [s[i] for i in rng.permutation(len(s))]


def _kinds(sizes, off):
    """open / orthorhombic / triclinic cycling over the structures in order of SIZE (ties by position), starting at ``off``:
    the sizes of one kernel route (<= 256 thread per query, 257 .. 4096 wave per query, above thread per query) are neighbours
    in that order, so a route with three sizes or more sees every kind, and the lone 4097 sees every kind over the offsets"""
    order = np.argsort(np.asarray(sizes), kind="stable")
    kinds = np.empty(len(sizes), np.int64)
    kinds[order] = (np.arange(len(sizes)) + off) % 3 - 1
    return kinds.tolist()


def _dims_of(v):
    v = np.asarray(v, np.float64)
    L = np.linalg.norm(v, axis=1)
    ang = lambda x, y: np.degrees(np.arccos(np.dot(x, y) / np.linalg.norm(x) / np.linalg.norm(y)))
    return np.array([L[0], L[1], L[2], ang(v[1], v[2]), ang(v[0], v[2]), ang(v[0], v[1])])


def _box_for(kind, n, g, integer, min_len=0.0, min_width=0.0, density=0.1):
    """(a, b, c, alpha, beta, gamma) of a box of about n / density A^3, or None for an open structure.  Orthorhombic: a cube
    (an integer edge when ``integer``, so that image distances of grid points tie exactly) of at least ``min_len``.  Triclinic:
    b_x = a_x / 4, c_x = -a_x / 5, c_y = 0.3 b_y (even g) or the rhombic dodecahedron (odd g).  ``min_width``: the smallest
    perpendicular width is at least that (cutoff lists need more than twice the cutoff)."""
    from nmrgnn_amd.pbc import triclinic_vectors, widths
    if kind == OPEN:
        return None
    L = max((n / density) ** (1.0 / 3.0), min_len, 1.0)
    if integer:
        L = float(np.ceil(L))
    if kind == ORTHO:
        dims = np.array([L, L, L, 90.0, 90.0, 90.0])
    elif g % 2 == 0:
        dims = _dims_of(np.array([[L, 0, 0], [L / 4, L, 0], [-L / 5, 0.3 * L, L]]))
    else:
        d = L * 2.0 ** (1.0 / 6.0)                      # volume d^3 / sqrt(2) = L^3
        dims = np.array([d, d, d, 60.0, 60.0, 90.0])
    w = widths(triclinic_vectors(dims)).min()
    if w < min_width:
        dims[:3] *= 1.02 * min_width / w
        if integer and kind == ORTHO:
            dims[:3] = np.ceil(dims[:3])
    return dims


def _structures(sizes, kinds, style, seed, C=10, min_width=0.0):
    """atoms, positions and boxes of the structures: integer-grid points (exact distance ties) or uniform floats, and for the
    periodic ones about half the atoms moved by whole lattice vectors, up to three boxes out: molecules cross faces, nothing
    is wrapped"""
    from nmrgnn_amd.pbc import triclinic_vectors
    rng = np.random.default_rng(seed)
    atoms, pos, boxes = [], [], []
    for g, (n, kind) in enumerate(zip(sizes, kinds)):
        if style == "grid":
            side = int(np.ceil((2.0 * n) ** (1.0 / 3.0))) + 1
            pick = rng.choice(side ** 3, n, replace=False)
            p = np.stack([pick // (side * side), (pick // side) % side, pick % side], axis=1).astype(np.float64)
            dims = _box_for(kind, n, g, True, min_len=side, min_width=min_width)    # no two grid points are images of each other
        else:
            dims = _box_for(kind, n, g, False, min_width=min_width)
            L = (n / 0.1) ** (1.0 / 3.0)
            p = rng.uniform(0, L, (n, 3))
        if dims is not None:
            v = triclinic_vectors(dims)
            shift = rng.integers(-3, 4, (n, 3)) * (rng.random((n, 1)) < 0.5)
            p = p + shift @ v
        pos.append(p.astype(np.float32))
        atoms.append(np.eye(C, dtype=np.float32)[rng.integers(0, C, n)])
        boxes.append(None if dims is None else tuple(float(x) for x in dims))
    return atoms, pos, boxes


def _block_kinds(sizes, kinds):
    """the number of different kinds among the rows of each 256-row workgroup"""
    row_kind = np.repeat(np.asarray(kinds), np.asarray(sizes))
    return [len(set(row_kind[r:r + 256].tolist())) for r in range(0, len(row_kind), 256)]


def _assert_knn_rows(b, g, gp, n, K, u):
    nl, ed, inv = b
    rows = slice(gp[g], gp[g + 1])
    real = np.arange(K)[None, :] < min(K, n - 1)
    want = np.where(real, _np(u.nlist) + gp[g], 0)
    np.testing.assert_array_equal(nl[rows], want, err_msg=f"structure {g} (n={n})")
    assert np.array_equal(ed[rows].view(np.uint32), _np(u.edges).view(np.uint32)), f"structure {g} (n={n})"
    assert np.array_equal(inv[rows].view(np.uint32), _np(u.inv_degree).view(np.uint32)), f"structure {g} (n={n})"
    assert not ed[rows][~np.broadcast_to(real, ed[rows].shape)].any()


# ------------------------------------------------------------------------------------------------ 1. kNN lists
@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("K", KS)
def test_boxed_ragged_knn_equals_per_structure_bitwise(gpu_device, K, style):
    from nmrgnn_amd.graph import frames_to_batch, structures_to_batch
    sizes = _sizes(K)
    kinds = _kinds(sizes, KS.index(K) + STYLES.index(style))
    assert max(_block_kinds(sizes, kinds)) >= 2                  # a workgroup's rows span structures of different kinds
    atoms, pos, boxes = _structures(sizes, kinds, style, seed=K)
    b = structures_to_batch(atoms, pos, K, device=gpu_device, boxes=boxes)
    gp = np.concatenate([[0], np.cumsum(sizes)])
    assert b.G == len(sizes) and b.N == gp[-1] and b.K == K and not b.is_csr
    assert _np(b.box_kind).tolist() == kinds and tuple(b.box.shape) == (len(sizes), 9)
    got = (_np(b.nlist), _np(b.edges), _np(b.inv_degree))
    differs = 0
    for g, n in enumerate(sizes):
        u = frames_to_batch(atoms[g], pos[g], K, device=gpu_device, box=boxes[g])
        _assert_knn_rows(got, g, gp, n, K, u)
        if boxes[g] is not None and n > 2:
            o = frames_to_batch(atoms[g], pos[g], K, device=gpu_device)
            differs += int(not np.array_equal(_np(o.nlist), _np(u.nlist)))
    assert differs >= 1                                          # the boxes were not ignored


@pytest.mark.parametrize("top, K", [(300, 16), (1100, 16), (1100, 40)], ids=["steps16", "steps32", "steps32_K40"])
def test_boxed_ragged_knn_shorter_wave_kernels(gpu_device, top, K):
    """the wave-per-query kernel is sized by the largest structure of at most 4096 atoms: batches that stop at 300 and at 1100
    atoms run its 16- and 32-step forms, every kind in each"""
    from nmrgnn_amd.graph import frames_to_batch, structures_to_batch
    sizes = _sizes(K, top=top) + [top - 3, top - 20, 257 + K]
    gp = np.concatenate([[0], np.cumsum(sizes)])
    kinds = _kinds(sizes, 1)
    assert {k for n, k in zip(sizes, kinds) if n > 256} == {OPEN, ORTHO, TRIC}
    atoms, pos, boxes = _structures(sizes, kinds, "grid", seed=top + K)
    b = structures_to_batch(atoms, pos, K, device=gpu_device, boxes=boxes)
    got = (_np(b.nlist), _np(b.edges), _np(b.inv_degree))
    for g, n in enumerate(sizes):
        _assert_knn_rows(got, g, gp, n, K, frames_to_batch(atoms[g], pos[g], K, device=gpu_device, box=boxes[g]))


# ------------------------------------------------------------------------------------------------ 2. the cell-grid route
def test_boxed_ragged_knn_cell_grid(gpu_device):
    """structures of >= 16384 atoms take the cell grid with their own box and kind; the orthorhombic one is not first, so its
    frame-local indices are shifted by the offset launch"""
    from nmrgnn_amd.graph import frames_to_batch, structures_to_batch
    K = 16
    sizes = [40, 16500, 300, 16500, 7]
    kinds = [TRIC, ORTHO, OPEN, TRIC, ORTHO]
    atoms, pos, boxes = _structures(sizes, kinds, "float", seed=165)
    b = structures_to_batch(atoms, pos, K, device=gpu_device, boxes=boxes)
    gp = np.concatenate([[0], np.cumsum(sizes)])
    got = (_np(b.nlist), _np(b.edges), _np(b.inv_degree))
    for g, n in enumerate(sizes):
        u = frames_to_batch(atoms[g], pos[g], K, device=gpu_device, box=boxes[g])
        _assert_knn_rows(got, g, gp, n, K, u)
        if n == 16500:
            o = frames_to_batch(atoms[g], pos[g], K, device=gpu_device)
            assert not np.array_equal(_np(o.nlist), _np(u.nlist))


# ------------------------------------------------------------------------------------------------ 3. cutoff lists
def _assert_cutoff_rows(b, g, gp, u):
    rp, col, dist, inv, row_of = b
    e0, e1 = rp[gp[g]], rp[gp[g + 1]]
    np.testing.assert_array_equal(rp[gp[g]:gp[g + 1] + 1] - e0, _np(u.row_ptr), err_msg=f"structure {g}")
    np.testing.assert_array_equal(col[e0:e1], _np(u.nlist) + gp[g], err_msg=f"structure {g}")
    assert np.array_equal(dist[e0:e1].view(np.uint32), _np(u.edges).view(np.uint32)), f"structure {g}"
    assert np.array_equal(inv[gp[g]:gp[g + 1]].view(np.uint32), _np(u.inv_degree).view(np.uint32)), f"structure {g}"
    np.testing.assert_array_equal(row_of[e0:e1], _np(u.row_of) + gp[g], err_msg=f"structure {g}")


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("cutoff", [3.0, 4.0])
def test_boxed_ragged_cutoff_equals_per_structure_bitwise(gpu_device, cutoff, style):
    from nmrgnn_amd.graph import frames_to_batch_cutoff, structures_to_batch
    sizes = _sizes(16)
    kinds = _kinds(sizes, int(cutoff) + STYLES.index(style))
    assert max(_block_kinds(sizes, kinds)) >= 2
    # one image per neighbour: every periodic structure more than twice the cutoff wide (the small ones grow for it)
    atoms, pos, boxes = _structures(sizes, kinds, style, seed=int(cutoff * 10), min_width=2.0 * cutoff + 0.5)
    b = structures_to_batch(atoms, pos, cutoff=cutoff, device=gpu_device, boxes=boxes)
    assert b.is_csr and b.G == len(sizes) and _np(b.box_kind).tolist() == kinds
    got = (_np(b.row_ptr), _np(b.nlist), _np(b.edges), _np(b.inv_degree), _np(b.row_of))
    gp = b.graph_ptr_host
    assert got[0][0] == 0 and got[0][-1] == len(got[1]) == b.nnz
    differs = 0
    for g, n in enumerate(sizes):
        u = frames_to_batch_cutoff(atoms[g], pos[g], cutoff, device=gpu_device, box=boxes[g])
        _assert_cutoff_rows(got, g, gp, u)
        if boxes[g] is not None and n > 2:
            o = frames_to_batch_cutoff(atoms[g], pos[g], cutoff, device=gpu_device)
            differs += int(not np.array_equal(_np(o.row_ptr), _np(u.row_ptr)))
    assert differs >= 1


# ------------------------------------------------------------------------------------------------ 4. only open structures
def test_all_none_boxes_equal_no_boxes(gpu_device):
    from nmrgnn_amd.graph import structures_to_batch
    sizes = _sizes(16)
    atoms, pos, _ = _structures(sizes, [OPEN] * len(sizes), "grid", seed=4)
    for kw in (dict(neighbor_number=16), dict(cutoff=3.0)):
        a = structures_to_batch(atoms, pos, device=gpu_device, **kw)
        b = structures_to_batch(atoms, pos, device=gpu_device, boxes=[None] * len(sizes), **kw)
        assert b.box is None and b.box_kind is None
        for name in ("nlist", "edges", "inv_degree") + (("row_ptr", "row_of") if a.is_csr else ()):
            assert np.array_equal(_np(getattr(a, name)).view(np.uint32), _np(getattr(b, name)).view(np.uint32)), name


# ------------------------------------------------------------------------------------------------ 5 / 6. gradient kernels
@functools.lru_cache(maxsize=None)
def _grad_case(form):
    """one boxed ragged batch, the per-structure batches of its structures and a seeded dedges, shared by the gradient tests"""
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff, structures_to_batch
    sizes = _sizes(16)
    kinds = _kinds(sizes, 2)
    atoms, pos, boxes = _structures(sizes, kinds, "float", seed=56, min_width=8.5 if form == "csr" else 0.0)
    if form == "padded":
        b = structures_to_batch(atoms, pos, 16, device=DEV, boxes=boxes)
        per = [frames_to_batch(atoms[g], pos[g], 16, device=DEV, box=boxes[g]) for g in range(len(sizes))]
    else:
        b = structures_to_batch(atoms, pos, cutoff=4.0, device=DEV, boxes=boxes)
        per = [frames_to_batch_cutoff(atoms[g], pos[g], 4.0, device=DEV, box=boxes[g]) for g in range(len(sizes))]
    gen = torch.Generator().manual_seed(7)
    dedges = torch.randn(tuple(b.edges.shape), generator=gen).to(DEV)
    gp = b.graph_ptr_host
    if form == "padded":
        spans = [(int(gp[g]), int(gp[g + 1])) for g in range(len(sizes))]          # rows of dedges
    else:
        rp = _np(b.row_ptr)
        spans = [(int(rp[gp[g]]), int(rp[gp[g + 1]])) for g in range(len(sizes))]  # entries of dedges
    return sizes, kinds, b, per, dedges, spans


def _positions_grad64(pos, src, dst, g, scale, vecs):
    """float64 NumPy restatement of ng_positions_grad for one structure: every live edge (src -> dst) with weight g pulls on
    both ends along its minimum-image vector (the fractional reduction, then every translation of [-2, 2]^3, over the
    float32 lattice vectors [3, 3] the device holds)"""
    p = pos.astype(np.float64)
    u = p[dst] - p[src]
    if vecs is not None:
        v = vecs.astype(np.float64)
        u0 = u - np.rint(u @ np.linalg.inv(v)) @ v
        best, u = np.full(len(u0), np.inf), u0.copy()
        for t in np.array(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij")).reshape(3, -1).T:
            c = u0 + t @ v
            c2 = (c * c).sum(-1)
            take = c2 < best
            best[take], u[take] = c2[take], c[take]
    w = (g.astype(np.float64) * scale / np.sqrt((u * u).sum(-1)))[:, None] * -u       # f * (r_i - r_j)
    out = np.zeros_like(p)
    np.add.at(out, src, w)
    np.subtract.at(out, dst, w)
    return out


@pytest.mark.parametrize("form", ["padded", "csr"])
def test_boxed_ragged_positions_grad_per_structure(gpu_device, form):
    """Rows of structure g against a float64 restatement of the kernel on that structure's own edges and box, at the bound
    tests/test_gpu_pbc.py holds the uniform periodic gradient to (1e-4 of the largest entry).

    Not bitwise against the per-structure batch's positions_grad, although the incoming edges keep their order and both
    kernels run the same row code: that code takes an edge's length as sqrtf(vx*vx + vy*vy + vz*vz) under the compiler's
    floating-point contraction, and the compiler fuses the three products differently from one instantiation to the next
    (the uniform triclinic kernel: fma(z, z, fma(y, y, x*x)), reusing a product of its image search; the open, orthorhombic
    and per-structure kernels: fma(z, z, fma(x, x, y*y))).  Open and orthorhombic structures come out bit for bit, which is
    asserted below as well; triclinic ones are a few ulp apart, and pinning the order would change the bits of the existing
    kernels."""
    sizes, kinds, b, per, dedges, spans = _grad_case(form)
    got = _np(b.positions_grad(dedges))
    assert got.shape == (b.N, 3)
    gp = b.graph_ptr_host
    pos, dd = _np(b.positions), _np(dedges)
    worst = 0.0
    for g, (u, (s0, s1)) in enumerate(zip(per, spans)):
        rows = slice(gp[g], gp[g + 1])
        n = sizes[g]
        if form == "padded":
            live = (_np(u.edges) > 0).reshape(-1)
            src = np.repeat(np.arange(n), 16)[live]
            dst = _np(u.nlist).reshape(-1).astype(np.int64)[live]
            w = dd[rows].reshape(-1)[live]
        else:
            src, dst, w = _np(u.row_of).astype(np.int64), _np(u.nlist).astype(np.int64), dd[s0:s1]
        if len(src) == 0:                                  # a structure without an edge (one atom): nothing pulls on it
            assert not got[rows].any()
            continue
        want = _positions_grad64(pos[rows], src, dst, w, b.scale, None if kinds[g] == OPEN else _np(u.box).reshape(3, 3))
        err = np.abs(got[rows] - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err <= 1e-4, f"structure {g} (n={n}, kind {kinds[g]}): {err:.2e}"
        if kinds[g] != TRIC:                               # open and orthorhombic structures: the per-structure kernel's bits
            alone = _np(u.positions_grad(dedges[s0:s1])).reshape(-1, 3)
            assert np.array_equal(got[rows].view(np.uint32), alone.view(np.uint32)), f"structure {g} (n={n}, kind {kinds[g]})"
    print(f"positions_grad ragged {form}: worst error relative to the largest entry {worst:.2e}")


@pytest.mark.parametrize("form", ["padded", "csr"])
def test_boxed_ragged_box_grad_per_structure(gpu_device, form):
    """float64 sums of equal float32 terms, chunked differently in a batch and in a structure alone: 1e-12 of the largest
    entry (the bound of tests/test_gpu_restraint.py for such sums)"""
    sizes, kinds, b, per, dedges, spans = _grad_case(form)
    strain, dvec = b.box_grad(dedges)
    strain2, dvec2 = b.box_grad(dedges)
    assert strain.dtype == dvec.dtype == torch.float64 and tuple(strain.shape) == tuple(dvec.shape) == (b.G, 3, 3)
    assert torch.equal(strain, strain2) and torch.equal(dvec, dvec2)             # the same call twice: the same bits
    strain, dvec = _np(strain), _np(dvec)
    worst = 0.0
    for g, (u, (s0, s1)) in enumerate(zip(per, spans)):
        if s1 == s0:                                   # a structure without an edge (one atom): empty sums
            assert not strain[g].any() and not dvec[g].any()
            continue
        us, ud = u.box_grad(dedges[s0:s1])
        us, ud = _np(us)[0], _np(ud)[0]
        for name, got, want in (("strain", strain[g], us), ("dvec", dvec[g], ud)):
            scale = np.abs(want).max()
            err = np.abs(got - want).max()
            worst = max(worst, err / scale if scale > 0 else 0.0)
            assert err <= 1e-12 * scale, f"{name} of structure {g} (n={sizes[g]}, kind {kinds[g]}): {err} of {scale}"
        if kinds[g] == OPEN:
            assert not dvec[g].any() and not ud.any()
        elif sizes[g] > 64:
            assert dvec[g].any()                                                  # atoms sit several boxes out: images count
    print(f"box_grad ragged {form}: worst relative difference {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 7. the model and autograd
MODEL_SIZES = [24, 9, 120, 17, 61, 300, 12]


def _model(C, seed=3):
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    m = GNNModel(make_hp(atom_feature_size=64), load_standards(), device=DEV, seed=seed)
    m.build(C)
    m.engine.edge_table = False
    return m


def _molecules(sizes, kinds, seed=5, min_width=0.0):
    """float structures with element one-hots the model knows"""
    from nmrgnn_amd.structure import atoms_onehot
    _, pos, boxes = _structures(sizes, kinds, "float", seed=seed, min_width=min_width)
    rng = np.random.default_rng(seed + 1)
    atoms = [atoms_onehot(rng.choice(["H", "C", "N", "O"], n, p=[0.5, 0.3, 0.1, 0.1])) for n in sizes]
    return atoms, pos, boxes


@pytest.mark.parametrize("form", ["padded", "csr"])
def test_model_on_boxed_ragged_batch_equals_per_structure(gpu_device, form):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff, structures_to_batch
    kinds = [ORTHO, TRIC, OPEN, TRIC, ORTHO, TRIC, OPEN]
    atoms, pos, boxes = _molecules(MODEL_SIZES, kinds, min_width=8.5 if form == "csr" else 0.0)
    model = _model(atoms[0].shape[1])
    if form == "padded":
        b = structures_to_batch(atoms, pos, 16, device=gpu_device, boxes=boxes)
    else:
        b = structures_to_batch(atoms, pos, cutoff=4.0, device=gpu_device, boxes=boxes)
    got = _np(model(b))
    want = []
    for a, p, bx in zip(atoms, pos, boxes):
        u = frames_to_batch(a, p, 16, device=gpu_device, box=bx) if form == "padded" else \
            frames_to_batch_cutoff(a, p, 4.0, device=gpu_device, box=bx)
        want.append(_np(model(u)))
    want = np.concatenate(want)
    assert got.shape == want.shape == (b.graph_ptr_host[-1],)
    assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want))


def test_forces_through_boxed_ragged_batch(gpu_device):
    from nmrgnn_amd.graph import structures_to_batch
    from nmrgnn_amd.library import shift_restraint
    sizes = MODEL_SIZES
    kinds = [ORTHO, TRIC, OPEN, TRIC, ORTHO, TRIC, OPEN]
    atoms, pos, boxes = _molecules(sizes, kinds, seed=9)
    model = _model(atoms[0].shape[1], seed=4)
    rng = np.random.default_rng(2)
    y = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    w = [rng.random(n).astype(np.float32) for n in sizes]
    P = torch.tensor(np.concatenate(pos), device=gpu_device, requires_grad=True)
    b = structures_to_batch(np.concatenate(atoms), P, 16, sizes=sizes, device=gpu_device, boxes=boxes)
    assert b.edges.requires_grad and b.box_kind is not None
    yt, wt = torch.from_numpy(np.concatenate(y)).to(gpu_device), torch.from_numpy(np.concatenate(w)).to(gpu_device)
    energy = ((model(b) - yt) ** 2 * wt).sum()
    energy.backward()
    grad = _np(P.grad)
    gp = b.graph_ptr_host
    for g in range(len(sizes)):
        e_g, f_g = shift_restraint(model, atoms[g], pos[g], y[g], w[g], neighbor_number=16, box=boxes[g])
        f = _np(f_g).astype(np.float64)
        got = -grad[gp[g]:gp[g + 1]].astype(np.float64)
        assert np.max(np.abs(got - f)) <= 1e-4 * np.max(np.abs(f)), g
    # the batch's own positions kernel gives the same gradient as autograd
    dedges = torch.autograd.grad(((model(b) - yt) ** 2 * wt).sum(), b.edges)[0]
    assert torch.equal(b.positions_grad(dedges), P.grad)


def test_boxes_grad_through_boxed_ragged_batch(gpu_device):
    """a [G, 6] boxes tensor that requires grad: box_grad chained through the box conversion, per structure what
    frames_to_batch gives for that structure's box alone"""
    from nmrgnn_amd.graph import frames_to_batch, structures_to_batch
    sizes = MODEL_SIZES
    kinds = [ORTHO, TRIC, TRIC, ORTHO, TRIC, ORTHO, TRIC]
    atoms, pos, boxes = _molecules(sizes, kinds, seed=11)
    model = _model(atoms[0].shape[1], seed=4)
    rng = np.random.default_rng(3)
    y = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(gpu_device) for n in sizes]
    B = torch.tensor(np.asarray(boxes, np.float64), requires_grad=True)
    b = structures_to_batch(atoms, pos, 16, device=gpu_device, boxes=B)
    assert b.edges.requires_grad and _np(b.box_kind).tolist() == kinds
    ((model(b) - torch.cat(y)) ** 2).sum().backward()
    got = B.grad.numpy()
    assert got.shape == (len(sizes), 6)
    for g in range(len(sizes)):
        Bg = torch.tensor(np.asarray(boxes[g], np.float64), requires_grad=True)
        u = frames_to_batch(atoms[g], pos[g], 16, device=gpu_device, box=Bg)
        ((model(u) - y[g]) ** 2).sum().backward()
        want = Bg.grad.numpy()
        assert np.abs(want).max() > 0
        assert np.max(np.abs(got[g] - want)) <= 1e-4 * np.max(np.abs(want)), g


# ------------------------------------------------------------------------------------------------ 8. eval-struct --separate --boxes
def _write_pdb(path, names, resnames, resids, elements, frame, dims):
    lines = []
    if dims is not None:
        lines.append("CRYST1%9.3f%9.3f%9.3f%7.2f%7.2f%7.2f P 1           1\n" % tuple(dims))
    lines.append("MODEL        1\n")
    for k in range(len(names)):
        nm = names[k] if len(names[k]) == 4 else " " + names[k]
        lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s\n"
                     % (k + 1, nm, resnames[k], resids[k], frame[k, 0], frame[k, 1], frame[k, 2], elements[k]))
    lines.append("ENDMDL\n")
    path.write_text("".join(lines))


def test_eval_struct_separate_boxes(gpu_device, tmp_path):
    from nmrgnn_amd.main import eval_structure
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(os.path.join(ROOT, "data", "108M.pdb"))
    t = read_pdb(os.path.join(ROOT, "data", "7lgi.pdb.gz"))
    files, periodic = [], []
    for name, u, sel, dims in (("ortho.pdb", s, np.arange(0, 400), "ortho"), ("tric.pdb", t, np.arange(t.n_atoms), "tric"),
                               ("open.pdb", s, np.arange(900, 1500), None)):
        p = np.asarray(u.frames[0], np.float64)[sel]
        if dims is not None:
            ext = p.max(0) - p.min(0) + 10.0
            L = float(ext.max())
            dims = np.array([ext[0], ext[1], ext[2], 90.0, 90.0, 90.0]) if dims == "ortho" else \
                np.round(_dims_of(np.array([[L, 0, 0], [L / 4, L, 0], [-L / 5, 0.3 * L, L]])), 2)
            dims = np.round(dims, 3)
            # wrap into the box along x: the molecule is cut by a face (CRYST1 keeps 3 decimals of a length)
            q = p - p.min(0) + np.array([0.45 * dims[0], 1.0, 1.0])
            q[:, 0] -= np.floor(q[:, 0] / dims[0]) * dims[0]
            p = q
        f = tmp_path / name
        _write_pdb(f, u.names[sel], u.resnames[sel], u.resids[sel], u.elements[sel], np.round(p, 3), dims)
        files.append(str(f))
        periodic.append(dims is not None)
    quiet = dict(keep_going=True, echo=lambda *a: None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        eval_structure(files, str(tmp_path / "sep.csv"), separate=True, boxes=True, **quiet)
        singles = []
        for k, f in enumerate(files):
            eval_structure([f], str(tmp_path / f"one{k}.csv"), pbc=periodic[k], **quiet)
            singles.append(list(csv.reader(open(tmp_path / f"one{k}.csv"))))
    sep = list(csv.reader(open(tmp_path / "sep.csv")))
    assert sep[0] == ['file'] + singles[0][0]
    body = sep[1:]
    want = [[f] + r for f, one in zip(files, singles) for r in one[1:]]
    assert len(body) == len(want) == 400 + t.n_atoms + 600
    assert [r[:5] + r[7:] for r in body] == [r[:5] + r[7:] for r in want]
    got = np.array([float(r[5]) for r in body])
    ref = np.array([float(r[5]) for r in want])
    assert np.max(np.abs(got - ref)) <= 0.011                  # the batch and a file alone: 1e-5 relative, then 2 decimals
    # and the boxes were used: without them the cut molecules give other shifts
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        eval_structure(files, str(tmp_path / "nobox.csv"), separate=True, **quiet)
    nobox = np.array([float(r[5]) for r in list(csv.reader(open(tmp_path / "nobox.csv")))[1:]])
    assert np.max(np.abs(nobox[:400] - got[:400])) > 0.011
