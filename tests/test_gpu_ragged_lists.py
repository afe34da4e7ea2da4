"""Neighbour lists of ragged batches (structures_to_batch: ng_knn_graph_ragged, ng_cutoff_count_ragged /
ng_cutoff_fill_rows_ragged): each structure's rows bit for bit what the uniform builders give for it alone, more structures
than the uniform path's 65535 frames, the model and the position gradient on ragged batches, eval-struct --separate."""
import csv
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = [1, 2, None, None, 63, 64, 65, 1000, 4096, 4097, 16500]      # None: K and K + 1; 16500 takes the cell grid


def _sizes(K):
    s = [K if v is None and i == 2 else K + 1 if v is None else v for i, v in enumerate(SIZES)]
    rng = np.random.default_rng(K)
    return [s[i] for i in rng.permutation(len(s))]


def _grid_structures(sizes, seed=0, C=10):
    """distinct points of an integer grid: exact distance ties everywhere"""
    rng = np.random.default_rng(seed)
    atoms, pos = [], []
    for n in sizes:
        side = int(np.ceil((2.0 * n) ** (1.0 / 3.0))) + 1
        pick = rng.choice(side ** 3, n, replace=False)
        p = np.stack([pick // (side * side), (pick // side) % side, pick % side], axis=1).astype(np.float32)
        pos.append(p)
        atoms.append(np.eye(C, dtype=np.float32)[rng.integers(0, C, n)])
    return atoms, pos


def _float_structures(sizes, seed=0, C=10, density=0.1):
    rng = np.random.default_rng(seed)
    atoms, pos = [], []
    for n in sizes:
        L = (n / density) ** (1.0 / 3.0)
        pos.append(rng.uniform(0, L, (n, 3)).astype(np.float32))
        atoms.append(np.eye(C, dtype=np.float32)[rng.integers(0, C, n)])
    return atoms, pos


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. kNN lists
@pytest.mark.parametrize("K", [5, 16, 40, 64])
def test_ragged_knn_equals_per_structure_bitwise(gpu_device, K):
    from nmrgnn_amd.graph import frames_to_batch, structures_to_batch
    sizes = _sizes(K)
    atoms, pos = _grid_structures(sizes, seed=K)
    b = structures_to_batch(atoms, pos, K, device=gpu_device)
    gp = np.concatenate([[0], np.cumsum(sizes)])
    assert b.G == len(sizes) and b.N == gp[-1] and b.K == K and not b.is_csr
    assert b.graph_ptr_host.tolist() == gp.tolist()
    nl, ed, inv = _np(b.nlist), _np(b.edges), _np(b.inv_degree)
    np.testing.assert_array_equal(_np(b.atoms), np.concatenate(atoms))
    for g, n in enumerate(sizes):
        u = frames_to_batch(atoms[g], pos[g], K, device=gpu_device)
        rows = slice(gp[g], gp[g + 1])
        real = np.arange(K)[None, :] < min(K, n - 1)
        want = np.where(real, _np(u.nlist) + gp[g], 0)
        np.testing.assert_array_equal(nl[rows], want, err_msg=f"structure {g} (n={n})")
        assert np.array_equal(ed[rows].view(np.uint32), _np(u.edges).view(np.uint32)), f"structure {g} (n={n})"
        assert np.array_equal(inv[rows].view(np.uint32), _np(u.inv_degree).view(np.uint32)), f"structure {g} (n={n})"
        assert not ed[rows][~np.broadcast_to(real, ed[rows].shape)].any()


@pytest.mark.parametrize("K", [5, 16, 40])
def test_ragged_knn_matches_host_builder(gpu_device, K):
    """against the host cKDTree builder, in the style of test_library.test_gpu_knn_matches_host_builder"""
    from nmrgnn_amd.graph import structures_to_batch
    from nmrgnn_amd.structure import inv_degree_of, knn_graph
    sizes = [7, 1, 300, 2, 45, 1200, 17]
    atoms, pos = _float_structures(sizes, seed=K)
    b = structures_to_batch(atoms, pos, K, device=gpu_device)
    nl, ed, inv = _np(b.nlist), _np(b.edges), _np(b.inv_degree)
    gp = b.graph_ptr_host
    for g in range(len(sizes)):
        hn, he = knn_graph(pos[g], K)
        sl = slice(gp[g], gp[g + 1])
        np.testing.assert_allclose(ed[sl], he, rtol=2e-6, atol=1e-7)
        real = he > 0
        local = np.where(real, nl[sl] - gp[g], 0)
        same = local == hn
        tied = np.isclose(he, np.roll(he, 1, axis=1), rtol=1e-6) | np.isclose(he, np.roll(he, -1, axis=1), rtol=1e-6)
        assert np.all(same | tied)
        assert same.mean() > 0.999
        assert np.all(nl[sl][~real] == 0)
        np.testing.assert_allclose(inv[sl], inv_degree_of(local), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ 2. cutoff lists
@pytest.mark.parametrize("cutoff", [1.5, 2.0, 3.2])
def test_ragged_cutoff_equals_per_structure_bitwise(gpu_device, cutoff):
    from nmrgnn_amd.graph import frames_to_batch_cutoff, structures_to_batch
    sizes = _sizes(16)
    atoms, pos = _grid_structures(sizes, seed=int(cutoff * 10))
    b = structures_to_batch(atoms, pos, cutoff=cutoff, device=gpu_device)
    assert b.is_csr and b.G == len(sizes)
    rp, col, dist, inv, row_of = _np(b.row_ptr), _np(b.nlist), _np(b.edges), _np(b.inv_degree), _np(b.row_of)
    gp = b.graph_ptr_host
    assert rp[0] == 0 and rp[-1] == len(col) == b.nnz
    for g, n in enumerate(sizes):
        u = frames_to_batch_cutoff(atoms[g], pos[g], cutoff, device=gpu_device)
        urp = _np(u.row_ptr)
        e0, e1 = rp[gp[g]], rp[gp[g + 1]]
        np.testing.assert_array_equal(rp[gp[g]:gp[g + 1] + 1] - e0, urp, err_msg=f"structure {g} (n={n})")
        np.testing.assert_array_equal(col[e0:e1], _np(u.nlist) + gp[g])
        assert np.array_equal(dist[e0:e1].view(np.uint32), _np(u.edges).view(np.uint32))
        assert np.array_equal(inv[gp[g]:gp[g + 1]].view(np.uint32), _np(u.inv_degree).view(np.uint32))
        np.testing.assert_array_equal(row_of[e0:e1], _np(u.row_of) + gp[g])


# ------------------------------------------------------------------------------------------------ 3. many structures
def test_ragged_more_structures_than_uniform_frames(gpu_device):
    """70 000 structures of 2-6 atoms (the uniform builders stop at 65535 frames) against a host search.  Coordinates are
    multiples of 1/8 A, so every squared distance is exact in float32 and the host orders by the kernels' (d2, index)."""
    from nmrgnn_amd.graph import structures_to_batch
    rng = np.random.default_rng(70)
    G, K, cutoff = 70000, 16, 2.5
    sizes = rng.integers(2, 7, G)
    N = int(sizes.sum())
    ipos = rng.integers(0, 32, (N, 3))
    pos = (ipos / 8.0).astype(np.float32)
    atoms = np.eye(10, dtype=np.float32)[rng.integers(0, 10, N)]
    b = structures_to_batch(atoms, pos, K, sizes=sizes, device=gpu_device)
    c = structures_to_batch(atoms, pos, cutoff=cutoff, sizes=sizes, device=gpu_device)
    assert b.G == c.G == G and b.N == c.N == N
    nl, ed, inv = _np(b.nlist), _np(b.edges), _np(b.inv_degree)
    rp, col, dist = _np(c.row_ptr), _np(c.nlist), _np(c.edges)
    gp = b.graph_ptr_host.astype(np.int64)
    for s in range(2, 7):
        sel = np.nonzero(sizes == s)[0]
        base = gp[sel]                                                        # [M]
        rows = base[:, None] + np.arange(s)[None, :]                          # [M, s]
        P = ipos[rows]
        d2 = ((P[:, :, None, :] - P[:, None, :, :]) ** 2).sum(-1)            # [M, s, s] in (1/8 A)^2, exact
        d2[:, np.arange(s), np.arange(s)] = 1 << 40
        order = np.argsort(d2, axis=2, kind="stable")[:, :, :s - 1]          # ties -> lower index; self last
        want_nl = np.zeros((len(sel), s, K), np.int64)
        want_nl[:, :, :s - 1] = order + base[:, None, None]
        want_ed = np.zeros((len(sel), s, K))
        want_ed[:, :, :s - 1] = np.sqrt(np.take_along_axis(d2, order, axis=2)) / 8.0 * 0.1
        np.testing.assert_array_equal(nl[rows], want_nl)
        np.testing.assert_allclose(ed[rows], want_ed, rtol=2e-6, atol=1e-7)
        cnt = (order > 0).sum(axis=2)
        np.testing.assert_allclose(inv[rows], np.where(cnt > 0, 1.0 / np.maximum(cnt, 1), 0.0), rtol=1e-6)
        # cutoff: neighbours closer than the cutoff, ascending index
        hit = d2 < int(cutoff * cutoff * 64)
        np.testing.assert_array_equal(rp[rows + 1] - rp[rows], hit.sum(axis=2))
        r, i, j = np.nonzero(hit)
        starts = rp[rows][r, i] + (np.cumsum(hit, axis=2)[r, i, j] - 1)
        np.testing.assert_array_equal(col[starts], base[r] + j)
        np.testing.assert_allclose(dist[starts], np.sqrt(d2[r, i, j]) / 8.0 * 0.1, rtol=2e-6)


# ------------------------------------------------------------------------------------------------ 4. the model
def _model(C, seed=3):
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    m = GNNModel(make_hp(atom_feature_size=64), load_standards(), device=torch.device("cuda", 0), seed=seed)
    m.build(C)
    m.engine.edge_table = False
    return m


def _molecules(sizes, seed=5):
    from nmrgnn_amd.structure import atoms_onehot
    rng = np.random.default_rng(seed)
    atoms, pos = [], []
    for n in sizes:
        atoms.append(atoms_onehot(rng.choice(["H", "C", "N", "O"], n, p=[0.5, 0.3, 0.1, 0.1])))
        L = (n / 0.1) ** (1.0 / 3.0)
        pos.append(rng.uniform(0, L, (n, 3)).astype(np.float32))
    return atoms, pos


@pytest.mark.parametrize("form", ["padded", "csr"])
def test_model_on_ragged_batch_equals_per_structure(gpu_device, form):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff, structures_to_batch
    sizes = [24, 9, 120, 17, 61, 300, 12]
    atoms, pos = _molecules(sizes)
    model = _model(atoms[0].shape[1])
    if form == "padded":
        b = structures_to_batch(atoms, pos, 16, device=gpu_device)
    else:
        b = structures_to_batch(atoms, pos, cutoff=4.0, device=gpu_device)
    got = _np(model(b))
    gp = b.graph_ptr_host
    want = []
    for a, p in zip(atoms, pos):
        u = frames_to_batch(a, p, 16, device=gpu_device) if form == "padded" else \
            frames_to_batch_cutoff(a, p, 4.0, device=gpu_device)
        want.append(_np(model(u)))
    want = np.concatenate(want)
    assert got.shape == want.shape == (gp[-1],)
    assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want))


# ------------------------------------------------------------------------------------------------ 5. forces
def test_forces_through_ragged_batch(gpu_device):
    from nmrgnn_amd.graph import structures_to_batch
    from nmrgnn_amd.library import shift_restraint
    sizes = [30, 18, 150, 45]
    atoms, pos = _molecules(sizes, seed=9)
    model = _model(atoms[0].shape[1], seed=4)
    rng = np.random.default_rng(2)
    y = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    w = [rng.random(n).astype(np.float32) for n in sizes]
    P = torch.tensor(np.concatenate(pos), device=gpu_device, requires_grad=True)
    b = structures_to_batch(np.concatenate(atoms), P, 16, sizes=sizes, device=gpu_device)
    assert b.edges.requires_grad
    peaks = model(b)
    yt, wt = torch.from_numpy(np.concatenate(y)).to(gpu_device), torch.from_numpy(np.concatenate(w)).to(gpu_device)
    energy = ((peaks - yt) ** 2 * wt).sum()
    energy.backward()
    grad = _np(P.grad)
    gp = b.graph_ptr_host
    for g in range(len(sizes)):
        e_g, f_g = shift_restraint(model, atoms[g], pos[g], y[g], w[g], neighbor_number=16)
        f = _np(f_g).astype(np.float64)
        got = -grad[gp[g]:gp[g + 1]].astype(np.float64)
        assert np.max(np.abs(got - f)) <= 1e-4 * np.max(np.abs(f)), g
        assert np.linalg.norm(got.sum(0)) <= 1e-4 * np.abs(got).sum(), g         # no net force on a structure
    # the batch's own positions kernel gives the same gradient as autograd
    dedges = torch.autograd.grad(((model(b) - yt) ** 2 * wt).sum(), b.edges)[0]
    assert torch.equal(b.positions_grad(dedges), P.grad)


# ------------------------------------------------------------------------------------------------ 6. eval-struct --separate
def _write_pdb(path, names, resnames, resids, elements, frames):
    lines = []
    for m, fr in enumerate(frames):
        lines.append(f"MODEL     {m + 1:4d}\n")
        for k in range(len(names)):
            nm = names[k] if len(names[k]) == 4 else " " + names[k]
            lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s\n"
                         % (k + 1, nm, resnames[k], resids[k], fr[k, 0], fr[k, 1], fr[k, 2], elements[k]))
        lines.append("ENDMDL\n")
    path.write_text("".join(lines))


def test_eval_struct_separate(gpu_device, tmp_path):
    from nmrgnn_amd.main import eval_structure
    from nmrgnn_amd.structure import read_pdb
    a = read_pdb(os.path.join(ROOT, "tests", "data", "108M.pdb"))
    b = read_pdb(os.path.join(ROOT, "tests", "data", "7lgi.pdb.gz"))
    files = []
    for name, s, sel in (("a.pdb", a, np.arange(0, 400)), ("b.pdb", b, np.arange(b.n_atoms)),
                         ("c.pdb", a, np.arange(900, 2100))):
        f = tmp_path / name
        _write_pdb(f, s.names[sel], s.resnames[sel], s.resids[sel], s.elements[sel], [s.frames[0][sel]])
        files.append(str(f))
    quiet = dict(keep_going=True, echo=lambda *a: None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        eval_structure(files, str(tmp_path / "sep.csv"), separate=True, frames_per_batch=2, **quiet)
        singles = []
        for k, f in enumerate(files):
            eval_structure([f], str(tmp_path / f"one{k}.csv"), **quiet)
            singles.append(list(csv.reader(open(tmp_path / f"one{k}.csv"))))
    sep = list(csv.reader(open(tmp_path / "sep.csv")))
    assert sep[0] == ['file'] + singles[0][0]
    body = sep[1:]
    want = [[f] + r for f, one in zip(files, singles) for r in one[1:]]
    assert len(body) == len(want) == 400 + b.n_atoms + 1200
    assert [r[0] for r in body] == [r[0] for r in want]
    assert [r[1:5] + r[7:] for r in body] == [r[1:5] + r[7:] for r in want]
    got = np.array([float(r[5]) for r in body])
    ref = np.array([float(r[5]) for r in want])
    assert np.max(np.abs(got - ref)) <= 0.011
