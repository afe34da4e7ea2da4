"""Periodic boxes on the GPU (csrc/pbc.cuh): minimum-image kNN and cutoff lists against float64 searches written here
(translations over [-2, 2]^3 after a float64 fractional reduction — not the product's 27-image code), the periodic cell
grid against brute force bit for bit, a molecule wrapped into its box against the same molecule unwrapped without one,
position gradients, shift_restraint and eval-struct --pbc."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import hp_to_oracle, make_hp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OCT = float(np.degrees(np.arccos(1.0 / 3.0)))


def _dev():
    return torch.device("cuda", 0)


def _dims_of(v):
    v = np.asarray(v, np.float64)
    L = np.linalg.norm(v, axis=1)
    ang = lambda x, y: np.degrees(np.arccos(np.dot(x, y) / np.linalg.norm(x) / np.linalg.norm(y)))
    return np.array([L[0], L[1], L[2], ang(v[1], v[2]), ang(v[0], v[2]), ang(v[0], v[1])])


def _box(kind, volume):
    """(dims [6], vectors [3, 3] float64 as the device sees them: float32-rounded)"""
    if kind == "cube":
        L = volume ** (1 / 3)
        dims = np.array([L, L, L, 90, 90, 90])
    elif kind == "flat":
        s = (volume / (6.0 * 5.0 * 1.0)) ** (1 / 3)
        dims = np.array([6.0 * s, 5.0 * s, 1.0 * s, 90, 90, 90])
    elif kind == "dodecahedron":
        d = (volume * np.sqrt(2.0)) ** (1 / 3)
        dims = np.array([d, d, d, 60, 60, 90])
    elif kind == "octahedron":
        d = (volume / (4.0 / 9.0 * np.sqrt(3.0))) ** (1 / 3)
        dims = np.array([d, d, d, OCT, 180 - OCT, OCT])
    else:                                              # the reduced-box extreme: every bound met
        v = np.array([[20.0, 0, 0], [10.0, 18.0, 0], [-10.0, 9.0, 16.0]])
        v *= (volume / abs(np.linalg.det(v))) ** (1 / 3)
        dims = _dims_of(v)
    from nmrgnn_amd.pbc import triclinic_vectors
    return dims, triclinic_vectors(dims).astype(np.float32).astype(np.float64)


def _atoms_in(vecs, n, rng, moved=0.3, far=3):
    """n uniform atoms in the box, a fraction moved by up to +-far box vectors"""
    f = rng.random((n, 3))
    shift = rng.integers(-far, far + 1, (n, 3)) * (rng.random((n, 1)) < moved)
    return ((f + shift) @ vecs).astype(np.float32)


def _mic64(pos, vecs):
    """[n, n] float64 minimum-image distances: fractional reduction, then every translation of [-2, 2]^3"""
    p = pos.astype(np.float64)
    inv = np.linalg.inv(vecs)
    d = p[None, :, :] - p[:, None, :]                 # r_j - r_i
    d -= np.rint(d @ inv) @ vecs
    best = np.full(d.shape[:2], np.inf)
    for t in np.array(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij")).reshape(3, -1).T:
        best = np.minimum(best, np.sqrt(((d + t @ vecs) ** 2).sum(-1)))
    return best


def _knn(frames, K, box, tric, scale=0.1):
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    G, n, _ = frames.shape
    dev = _dev()
    tp = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).to(dev)
    nl = torch.full((G * n, K), -7, dtype=torch.int32, device=dev)
    ed = torch.full((G * n, K), -7.0, device=dev)
    inv = torch.full((G * n,), -7.0, device=dev)
    ctx = _lib.get_context(0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if box is None:
        ctx.check(ctx.lib.ng_knn_graph(ctx.handle, st, G, n, K, scale, ptr(tp), ptr(nl), ptr(ed), ptr(inv)), "knn")
    else:
        bx = torch.from_numpy(np.ascontiguousarray(np.asarray(box).reshape(G, 9), np.float32)).to(dev)
        ctx.check(ctx.lib.ng_knn_graph_pbc(ctx.handle, st, G, n, K, scale, ptr(tp), ptr(bx), int(tric), ptr(nl), ptr(ed),
                                           ptr(inv)), "knn_pbc")
    torch.cuda.synchronize()
    return nl.cpu().numpy(), ed.cpu().numpy(), inv.cpu().numpy()


def _inv_expected(nl_local, valid):
    c = ((nl_local > 0) & valid).sum(1)
    return np.where(c > 0, 1.0 / np.maximum(c, 1), 0.0).astype(np.float32)


def _check_knn_rows(nl, ed, inv, d64, g, n, K, pos_scale):
    """frame g's rows against float64: each slot's neighbour at the float64 distance of that slot (near-ties may swap)"""
    rows = slice(g * n, (g + 1) * n)
    loc = nl[rows] - g * n
    assert (loc >= 0).all() and (loc < n).all()
    dd = d64.copy()
    np.fill_diagonal(dd, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(n), dd.shape), dd), axis=1)[:, :K]
    ref_d = np.take_along_axis(dd, order, 1)
    got_d = np.take_along_axis(dd, loc, 1)
    assert (loc != np.arange(n)[:, None]).all()                          # never the atom itself
    assert all(len(set(r)) == K for r in loc)                            # each atom at most once
    quantum = 2.0 * float(np.spacing(np.float32(pos_scale)))             # the raw positions' own float32 quantum
    np.testing.assert_allclose(got_d, ref_d, rtol=1e-6, atol=quantum)
    same = (loc == order).mean()
    assert same > 0.999, same
    np.testing.assert_allclose(ed[rows], 0.1 * got_d, rtol=1e-6, atol=0.1 * quantum)
    np.testing.assert_array_equal(inv[rows], _inv_expected(loc, np.ones_like(loc, bool)))


@pytest.mark.parametrize("kinds", [("cube",) * 3, ("flat",) * 3, ("dodecahedron",) * 3, ("octahedron",) * 3,
                                   ("skew",) * 3, ("cube", "dodecahedron", "skew")],
                         ids=["cube", "flat", "dodecahedron", "octahedron", "skew", "mixed"])
def test_knn_against_float64(kinds):
    rng = np.random.default_rng(len("".join(kinds)))
    n, K, G = 600, 16, 3
    boxes = [_box(k, n / 0.1 * s) for k, s in zip(kinds, (0.9, 1.0, 1.15))]
    frames = np.stack([_atoms_in(v, n, rng) for _, v in boxes])
    vec9 = np.stack([v.reshape(9) for _, v in boxes])
    tric = any(k not in ("cube", "flat") for k in kinds)
    nl, ed, inv = _knn(frames, K, vec9, tric)
    for g in range(G):
        _check_knn_rows(nl, ed, inv, _mic64(frames[g], boxes[g][1]), g, n, K, np.abs(frames[g]).max())


def _both(monkeypatch, frames, K, vec9, tric):
    monkeypatch.setenv("NG_KNN", "brute")
    ref = _knn(frames, K, vec9, tric)
    monkeypatch.setenv("NG_KNN", "cells")
    got = _knn(frames, K, vec9, tric)
    for a, b, name in zip(got, ref, ("nlist", "edges", "inv_degree")):
        np.testing.assert_array_equal(a, b, err_msg=name)
    return ref


@pytest.mark.parametrize("kind,n,K,G", [("cube", 40000, 16, 1), ("skew", 20000, 16, 1), ("octahedron", 6000, 16, 3),
                                        ("thin2", 3000, 16, 1), ("thin1", 3000, 16, 2), ("cube", 4000, 40, 2),
                                        ("tiny", 70, 16, 1)])
def test_periodic_cell_grid_equals_brute_force(monkeypatch, kind, n, K, G):
    rng = np.random.default_rng(n + K + G)
    boxes = []
    for g in range(G):
        if kind.startswith("thin"):                    # one axis of 2 cells (thin2) or 1 cell (thin1)
            h = 6.1 if kind == "thin2" else 3.0
            L = np.sqrt(n / 0.1 / h)
            from nmrgnn_amd.pbc import triclinic_vectors
            dims = np.array([L, L * 0.9, h, 90, 90, 90])
            boxes.append((dims, triclinic_vectors(dims).astype(np.float32).astype(np.float64)))
        else:
            boxes.append(_box("cube" if kind == "tiny" else kind, n / 0.1 * (1.0 + 0.1 * g)))
    frames = np.stack([_atoms_in(v, n, rng) for _, v in boxes])
    vec9 = np.stack([v.reshape(9) for _, v in boxes])
    tric = kind in ("skew", "octahedron")
    nl, ed, inv = _both(monkeypatch, frames, K, vec9, tric)
    # and right: a sample of rows against float64
    for g in range(G):
        p = frames[g].astype(np.float64)
        inv_v = np.linalg.inv(boxes[g][1])
        for i in rng.integers(0, n, 10):
            d = p - p[i]
            d -= np.rint(d @ inv_v) @ boxes[g][1]
            best = np.full(n, np.inf)
            for t in np.array(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij")).reshape(3, -1).T:
                best = np.minimum(best, np.sqrt(((d + t @ boxes[g][1]) ** 2).sum(-1)))
            best[i] = np.inf
            ref = np.sort(best)[:min(K, n - 1)]
            quantum = 2.0 * float(np.spacing(np.float32(np.abs(frames[g]).max())))
            np.testing.assert_allclose(ed[g * n + i, :len(ref)], 0.1 * ref, rtol=2e-6, atol=0.1 * quantum)


def test_default_path_is_the_periodic_cell_grid_from_16384_atoms(monkeypatch):
    from nmrgnn_amd import _lib
    monkeypatch.delenv("NG_KNN", raising=False)
    rng = np.random.default_rng(3)
    ctx = _lib.get_context(0)
    for n, cells in ((16383, False), (16384, True)):
        dims, v = _box("cube", n / 0.1)
        frames = _atoms_in(v, n, rng)[None]
        ctx.prof_enable(True)
        ctx.prof_reset()
        _knn(frames, 16, v.reshape(1, 9), False)
        names = ctx.prof_read()
        ctx.prof_enable(False)
        assert ("knn_cells_query" in names) == cells, names


def _cutoff(frames, cutoff, box, tric, scale=0.1):
    from nmrgnn_amd.graph import frames_to_batch_cutoff
    n = frames.shape[1]
    atoms = np.eye(4, dtype=np.float32)[np.arange(n) % 4]
    return frames_to_batch_cutoff(atoms, frames, cutoff=cutoff, scale=scale, box=box)


@pytest.mark.parametrize("kind", ["cube", "flat", "octahedron", "skew"])
def test_cutoff_against_float64(kind):
    rng = np.random.default_rng(11)
    n, G = 600, 2
    boxes = [_box(kind, n / 0.1 * s) for s in (1.0, 1.2)]
    from nmrgnn_amd.pbc import widths
    cutoff = min(4.5, 0.45 * min(widths(v).min() for _, v in boxes))     # below half the thinnest width
    frames = np.stack([_atoms_in(v, n, rng) for _, v in boxes])
    b = _cutoff(frames, cutoff, np.stack([d for d, _ in boxes]), kind not in ("cube", "flat"))
    assert b.box is not None and b.box_triclinic == (kind not in ("cube", "flat"))
    rp = b.row_ptr.cpu().numpy()
    col = b.nlist.cpu().numpy()
    dist = b.edges.detach().cpu().numpy()
    inv = b.inv_degree.cpu().numpy()
    for g in range(G):
        d64 = _mic64(frames[g], boxes[g][1])
        for i in range(n):
            r = g * n + i
            c = col[rp[r]:rp[r + 1]] - g * n
            assert (np.diff(c) > 0).all()                                  # ascending, each atom once
            ref = np.flatnonzero(d64[i] < cutoff)
            ref = ref[ref != i]
            near = np.abs(d64[i] - cutoff) <= 1e-6 * cutoff
            assert set(c) - set(ref) <= set(np.flatnonzero(near)) and set(ref) - set(c) <= set(np.flatnonzero(near))
            np.testing.assert_allclose(dist[rp[r]:rp[r + 1]], 0.1 * d64[i, c], rtol=1e-6,
                                       atol=0.2 * float(np.spacing(np.float32(np.abs(frames[g]).max()))))
            cp = int((c > 0).sum())
            assert inv[r] == (np.float32(1.0) / np.float32(cp) if cp else 0.0)


# ------------------------------------------------------------------------------------------------ a wrapped molecule
def _protein():
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(os.path.join(HERE, "data", "7lgi.pdb.gz"))
    return atoms_onehot(s.elements), np.asarray(s.frames[0], np.float32)


def _wrapped(p, shift):
    """7lgi frame 0 in an orthorhombic box of its extent + 12 A, moved by `shift` past a corner of the cell and wrapped"""
    ext = p.max(0) - p.min(0) + 12.0
    dims = np.array([ext[0], ext[1], ext[2], 90, 90, 90], np.float64)
    L = ext.astype(np.float32)
    q = (p - p.mean(0) + shift).astype(np.float32)       # the centre of mass near the corner (0, 0, 0)
    w = (q - np.floor(q / L) * L).astype(np.float32)
    return dims, q, w


def _dist64(p):
    p = p.astype(np.float64)
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    return d


def _no_near_tie_at_kth(p, K, rtol=1e-5):
    """float64: every atom's K-th and (K+1)-th nearest distances are more than rtol apart (the sets are then exact)"""
    s = np.sort(_dist64(p), 1)[:, K - 1:K + 1]
    return bool((s[:, 1] - s[:, 0] > rtol * s[:, 1]).all())


def _same_lists(got, ref, p, rtol=1e-5):
    """equal neighbour sets per row; where the order differs, only inside float64 near-ties"""
    d = _dist64(p)
    np.testing.assert_array_equal(np.sort(got, 1), np.sort(ref, 1))
    rows = np.arange(len(got))[:, None]
    np.testing.assert_allclose(d[rows, got], d[rows, ref], rtol=rtol, atol=0)


def _model(seed=3):
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    return GNNModel(make_hp(atom_feature_size=64), load_standards(), device=_dev(), seed=seed)


@pytest.mark.parametrize("shift", [(0.4, -0.7, 0.3), (13.37, -41.2, 77.7)], ids=["corner", "translated"])
def test_wrapped_molecule_equals_unwrapped(shift):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    atoms, p = _protein()
    dims, q, w = _wrapped(p, np.array(shift))
    L = dims[:3]
    assert all(((w[:, a] < 0.25 * L[a]).any() and (w[:, a] > 0.75 * L[a]).any()) for a in range(3))   # cut three ways
    K = 16
    assert _no_near_tie_at_kth(q, K)
    ref = frames_to_batch(atoms, q)
    got = frames_to_batch(atoms, w, box=dims)
    _same_lists(got.nlist.cpu().numpy(), ref.nlist.cpu().numpy(), q)
    np.testing.assert_array_equal(got.inv_degree.cpu().numpy(), ref.inv_degree.cpu().numpy())
    np.testing.assert_allclose(np.sort(got.edges.cpu().numpy(), 1), np.sort(ref.edges.cpu().numpy(), 1), rtol=1e-5, atol=2e-6)
    cut = 3.9                                          # no pair within 1e-5 of it in float64
    assert not (np.abs(_dist64(q) - cut) < 1e-5 * cut).any()
    rc = frames_to_batch_cutoff(atoms, q, cutoff=cut)
    gc = frames_to_batch_cutoff(atoms, w, cutoff=cut, box=dims)
    np.testing.assert_array_equal(gc.row_ptr.cpu().numpy(), rc.row_ptr.cpu().numpy())
    np.testing.assert_array_equal(gc.nlist.cpu().numpy(), rc.nlist.cpu().numpy())
    np.testing.assert_array_equal(gc.inv_degree.cpu().numpy(), rc.inv_degree.cpu().numpy())
    np.testing.assert_allclose(gc.edges.cpu().numpy(), rc.edges.cpu().numpy(), rtol=1e-5, atol=2e-6)
    model = _model()
    model.build(atoms.shape[1])
    pr = model(ref).cpu().numpy()
    pg = model(got).cpu().numpy()
    assert np.abs(pg - pr).max() <= 1e-5 * np.abs(pr).max()


# ------------------------------------------------------------------------------------------------ gradients
def _ref_positions_grad_mic(model, atoms, batch, frames, vecs, targets, w):
    """float64 torch: minimum-image edge vectors over the batch's own lists, torch_ref.forward, autograd"""
    from oracle import torch_ref
    G, n, _ = frames.shape
    N = G * n
    pos = torch.tensor(frames.reshape(N, 3).astype(np.float64), requires_grad=True)
    if batch.is_csr:
        rp = batch.row_ptr.cpu().numpy().astype(np.int64)
        col = batch.nlist.cpu().numpy().astype(np.int64)
        deg = np.diff(rp)
        K = int(deg.max())
        rows = np.repeat(np.arange(N), deg)
        slot = np.arange(len(col)) - rp[rows]
        nlist = np.zeros((N, K), np.int64)
        live = np.zeros((N, K), bool)
        nlist[rows, slot] = col
        live[rows, slot] = True
    else:
        nlist = batch.nlist.cpu().numpy().astype(np.int64)
        live = batch.edges.detach().cpu().numpy() > 0
    # the image of every edge, fixed (no gradient through the choice): the float64 minimum image
    V = torch.from_numpy(np.repeat(vecs, n, axis=0))                   # [N, 3, 3]
    Vinv = torch.linalg.inv(V)
    src = torch.arange(N)[:, None].expand_as(torch.from_numpy(nlist))
    d = (pos[torch.from_numpy(nlist)] - pos[src]).detach()
    f = torch.einsum("nkc,ncd->nkd", d, Vinv)
    d0 = d - torch.einsum("nkc,ncd->nkd", torch.round(f), V)
    best, shift = None, None
    for t in np.array(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij")).reshape(3, -1).T:
        tt = torch.einsum("c,ncd->nd", torch.from_numpy(t.astype(np.float64)), V)[:, None]
        cand = ((d0 + tt) ** 2).sum(-1)
        if best is None:
            best, shift = cand, (d0 + tt) - d
        else:
            better = cand < best
            best = torch.where(better, cand, best)
            shift = torch.where(better[..., None], (d0 + tt) - d, shift)
    v = pos[torch.from_numpy(nlist)] - pos[src] + shift
    dist = torch.sqrt((v * v).sum(-1).clamp_min(1e-300)) * batch.scale
    dd = torch.where(torch.from_numpy(live), dist, torch.zeros_like(dist))
    p = torch_ref.to_torch_params(model.get_weights())
    C_ = atoms.shape[1]
    peaks = torch_ref.forward((np.tile(atoms, (G, 1)), nlist, dd, batch.inv_degree.cpu().numpy()), p, hp_to_oracle(model.hypers),
                              peak_std=model.peak_std[:C_], peak_avg=model.peak_avg[:C_])
    ((peaks - torch.from_numpy(targets.astype(np.float64))) ** 2 * torch.from_numpy(w.astype(np.float64))).sum().backward()
    return pos.grad.numpy().reshape(G, n, 3)


@pytest.mark.parametrize("cutoff", [None, 4.0], ids=["knn", "cutoff"])
def test_positions_grad_against_float64(cutoff):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    atoms, p = _protein()
    rng = np.random.default_rng(5)
    d0, _, w0 = _wrapped(p, np.array([0.4, -0.7, 0.3]))
    d1 = d0.copy()
    d1[:3] += 5.0                                      # a second, larger box
    _, _, w1 = _wrapped(p + 0.05 * rng.standard_normal(p.shape).astype(np.float32), np.array([3.1, 2.2, -0.9]) + 5.0)
    w1 = (w1 - np.floor(w1 / d1[:3].astype(np.float32)) * d1[:3].astype(np.float32)).astype(np.float32)
    frames = np.stack([w0, w1])
    dims = np.stack([d0, d1])
    from nmrgnn_amd.pbc import triclinic_vectors
    vecs = np.stack([triclinic_vectors(d).astype(np.float32).astype(np.float64) for d in dims])
    G, n = 2, p.shape[0]
    model = _model()
    model.build(atoms.shape[1])
    targets = rng.standard_normal(G * n).astype(np.float32) * 2.0
    wt = (rng.random(G * n) < 0.8).astype(np.float32)
    pos = torch.tensor(frames, device=_dev(), requires_grad=True)
    batch = frames_to_batch(atoms, pos, box=dims) if cutoff is None else frames_to_batch_cutoff(atoms, pos, cutoff=cutoff, box=dims)
    assert batch.edges.grad_fn is not None and batch.box is not None
    peaks = model(batch)
    ((peaks - torch.from_numpy(targets).to(_dev())) ** 2 * torch.from_numpy(wt).to(_dev())).sum().backward()
    got = pos.grad.cpu().numpy()
    ref = _ref_positions_grad_mic(model, atoms, batch, frames, vecs, targets, wt)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"pbc positions grad cutoff={cutoff}: max rel err {err:.2e}")
    assert err <= 1e-4, err
    for g in range(G):                                 # net force ~ 0 (no torque check: it does not hold in a box)
        f = got[g].astype(np.float64)
        assert np.abs(f.sum(0)).max() / np.abs(f).sum() < 1e-5


def test_shift_restraint_with_box_equals_autograd_bitwise():
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.library import shift_restraint
    atoms, p = _protein()
    dims, _, w = _wrapped(p, np.array([0.4, -0.7, 0.3]))
    n = p.shape[0]
    rng = np.random.default_rng(8)
    model = _model()
    model.build(atoms.shape[1])
    targets = rng.standard_normal(n).astype(np.float32)
    wt = rng.random(n).astype(np.float32)
    energy, forces = shift_restraint(model, atoms, w, targets, wt, box=dims)
    pos = torch.tensor(w, device=_dev(), requires_grad=True)
    peaks = model(frames_to_batch(atoms, pos, box=dims))
    loss = ((peaks - torch.from_numpy(targets).to(_dev())) ** 2 * torch.from_numpy(wt).to(_dev())).sum()
    loss.backward()
    assert torch.equal(pos.grad, -forces)
    assert abs(float(energy) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))


# ------------------------------------------------------------------------------------------------ eval-struct --pbc
def _write_pdb(path, names, resnames, resids, elements, frames, dims):
    lines = []
    for m, (fr, d) in enumerate(zip(frames, dims)):
        if d is not None:
            lines.append("CRYST1%9.3f%9.3f%9.3f%7.2f%7.2f%7.2f P 1           1\n" % tuple(d))
        lines.append(f"MODEL     {m + 1:4d}\n")
        for k in range(len(names)):
            nm = names[k] if len(names[k]) == 4 else " " + names[k]
            lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s\n"
                         % (k + 1, nm, resnames[k], resids[k], fr[k, 0], fr[k, 1], fr[k, 2], elements[k]))
        lines.append("ENDMDL\n")
    path.write_text("".join(lines))


def test_eval_struct_pbc(tmp_path):
    import csv
    from nmrgnn_amd.main import eval_structure
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(os.path.join(HERE, "data", "7lgi.pdb.gz"))
    p = np.round(np.asarray(s.frames[0], np.float64), 3)
    qs, ws, ds = [], [], []
    for shift in ((0.4, -0.7, 0.3), (21.3, 5.5, -13.1)):
        dims, q, w = _wrapped(p.astype(np.float32), np.array(shift))
        dims = np.round(dims, 3)
        L = dims[:3]
        q = np.round(q.astype(np.float64), 3)
        qs.append(q)
        ws.append(np.round(q - np.floor(q / L) * L, 3))
        ds.append(dims)
    args = (s.names, s.resnames, s.resids, s.elements)
    _write_pdb(tmp_path / "wrapped.pdb", *args, ws, ds)
    _write_pdb(tmp_path / "whole.pdb", *args, qs, [None, None])
    assert all(_no_near_tie_at_kth(q, 16) for q in qs)
    eval_structure([str(tmp_path / "wrapped.pdb")], str(tmp_path / "pbc.csv"), pbc=True, keep_going=True, echo=lambda *a: None)
    eval_structure([str(tmp_path / "whole.pdb")], str(tmp_path / "open.csv"), keep_going=True, echo=lambda *a: None)
    a = list(csv.reader(open(tmp_path / "pbc.csv")))
    b = list(csv.reader(open(tmp_path / "open.csv")))
    assert a[0] == b[0] and len(a) == len(b) == 1 + 2 * len(s.names)
    pa = np.array([float(r[4]) for r in a[1:]])
    pb = np.array([float(r[4]) for r in b[1:]])
    assert np.abs(pa - pb).max() <= 0.01 + 1e-9
    assert [r[:4] + r[6:] for r in a[1:]] == [r[:4] + r[6:] for r in b[1:]]
    with pytest.raises(ValueError, match="no box"):
        eval_structure([str(tmp_path / "whole.pdb")], str(tmp_path / "x.csv"), pbc=True, echo=lambda *a: None)
