"""Box gradients on the GPU (ng_box_grad / ng_box_grad_csr, GraphBatch.box_grad, box.grad through frames_to_batch,
shift_restraint(virial=True)): the kernel against NumPy float64 sums over the same lists with images from a float64
minimum-image search written here, determinism, the identity S = sum r (x) dE/dr + h^T B, the strain derivative and
box.grad end to end against float64 torch autograd through oracle/torch_ref, and the invariances."""
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


def _edges_of(batch, dd):
    """(rows, cols, dd) of the slots the kernels count: padded slots with edges > 0, every CSR entry; dd != 0"""
    dd = dd.reshape(-1)
    if batch.is_csr:
        rp = batch.row_ptr.cpu().numpy().astype(np.int64)
        rows = np.repeat(np.arange(batch.N), np.diff(rp))
        cols = batch.nlist.cpu().numpy().astype(np.int64)
        live = np.ones(len(cols), bool)
    else:
        rows = np.repeat(np.arange(batch.N), batch.K)
        cols = batch.nlist.cpu().numpy().astype(np.int64).reshape(-1)
        live = batch.edges.detach().cpu().numpy().reshape(-1) > 0
    live &= dd != 0
    return rows[live], cols[live], dd[live].astype(np.float64), live


def _mic_images(d, vecs):
    """integer image triples n with u = d + n h the float64 minimum image: a fractional reduction, then [-2, 2]^3"""
    n0 = -np.rint(d @ np.linalg.inv(vecs))
    best = np.full(len(d), np.inf)
    img = np.zeros_like(d)
    for t in np.array(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij")).reshape(3, -1).T:
        m = n0 + t
        e = ((d + m @ vecs) ** 2).sum(-1)
        better = e < best
        best = np.where(better, e, best)
        img[better] = m[better]
    return img


def _ref_sb(batch, pos, gp, vecs, dd, scale):
    """NumPy float64 per-frame (S, B, sum |u||p|, sum |n||p|) over the batch's own lists"""
    rows, cols, g, _ = _edges_of(batch, dd)
    p64 = pos.reshape(-1, 3).astype(np.float64)
    frame = np.searchsorted(gp, rows, side="right") - 1
    d = p64[cols] - p64[rows]
    n = np.zeros_like(d)
    if vecs is not None:
        for f in range(len(gp) - 1):
            m = frame == f
            n[m] = _mic_images(d[m], vecs[f])
        u = d + np.einsum("ec,ecd->ed", n, vecs[frame])
    else:
        u = d
    ln = np.sqrt((u * u).sum(-1))
    p = (g * scale / ln)[:, None] * u
    G = len(gp) - 1
    S, B, su, sn = np.zeros((G, 3, 3)), np.zeros((G, 3, 3)), np.zeros(G), np.zeros(G)
    np.add.at(S, frame, u[:, :, None] * p[:, None, :])
    np.add.at(B, frame, n[:, :, None] * p[:, None, :])
    np.add.at(su, frame, ln * np.sqrt((p * p).sum(-1)))
    np.add.at(sn, frame, np.sqrt((n * n).sum(-1)) * np.sqrt((p * p).sum(-1)))
    return S, B, su, sn


def _random_dd(batch, rng):
    dd = rng.standard_normal(tuple(batch.edges.shape)).astype(np.float32)
    dd[rng.random(dd.shape) < 0.1] = 0.0
    return dd


def _check_kernel(batch, pos, gp, vecs, rng):
    dd = _random_dd(batch, rng)
    ddt = torch.from_numpy(dd).to(_dev())
    S, B = batch.box_grad(ddt)
    assert S.dtype == B.dtype == torch.float64 and tuple(S.shape) == tuple(B.shape) == (len(gp) - 1, 3, 3)
    S2, B2 = batch.box_grad(ddt)
    assert torch.equal(S, S2) and torch.equal(B, B2)                  # bitwise deterministic
    S, B = S.cpu().numpy(), B.cpu().numpy()
    rS, rB, su, sn = _ref_sb(batch, pos, gp, vecs, dd, batch.scale)
    for f in range(len(gp) - 1):
        assert np.abs(S[f] - rS[f]).max() <= 1e-5 * su[f], (f, np.abs(S[f] - rS[f]).max(), su[f])
        assert np.abs(B[f] - rB[f]).max() <= 1e-5 * sn[f], (f, np.abs(B[f] - rB[f]).max(), sn[f])
        np.testing.assert_array_equal(S[f], S[f].T)
    if vecs is None:
        assert (B == 0).all()
    return S, B, dd


KINDS = {"open": None, "cube": ("cube",) * 3, "flat": ("flat",) * 3, "dodecahedron": ("dodecahedron",) * 3,
         "octahedron": ("octahedron",) * 3, "skew": ("skew",) * 3, "mixed": ("cube", "dodecahedron", "skew")}


def _frames(kind, n, rng):
    if KINDS[kind] is None:
        frames = (rng.random((3, n, 3)) * (n / 0.1) ** (1 / 3)).astype(np.float32)
        return frames, None, None
    boxes = [_box(k, n / 0.1 * s) for k, s in zip(KINDS[kind], (0.9, 1.0, 1.15))]
    frames = np.stack([_atoms_in(v, n, rng) for _, v in boxes])
    return frames, np.stack([d for d, _ in boxes]), np.stack([v for _, v in boxes])


# ------------------------------------------------------------------------------------------------ 1, 2: the kernel
@pytest.mark.parametrize("form", ["knn", "knn_padded", "cutoff"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_against_float64(kind, form):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    from nmrgnn_amd.pbc import widths
    rng = np.random.default_rng(len(kind) * 7 + len(form))
    n = 10 if form == "knn_padded" else 400
    frames, dims, vecs = _frames(kind, n, rng)
    atoms = np.eye(4, dtype=np.float32)[np.arange(n) % 4]
    if form == "cutoff":
        cut = 4.0 if vecs is None else 0.45 * min(widths(v).min() for v in vecs)
        batch = frames_to_batch_cutoff(atoms, frames, cutoff=cut, box=dims)
    else:
        batch = frames_to_batch(atoms, frames, box=dims)
    if form == "knn_padded":
        assert (batch.edges.cpu().numpy() == 0).any()                # dead slots
    gp = batch.graph_ptr_host.astype(np.int64)
    _check_kernel(batch, frames, gp, vecs, rng)


@pytest.mark.parametrize("cutoff", [None, 3.5], ids=["knn", "cutoff"])
def test_kernel_ragged_against_float64(cutoff):
    from nmrgnn_amd.graph import structures_to_batch
    rng = np.random.default_rng(11)
    sizes = [1, 7, 300, 1, 50, 257, 3, 600, 2, 40]              # frames inside one chunk, across chunks, 1-atom ones
    pos = [(rng.random((s, 3)) * (max(s, 2) / 0.1) ** (1 / 3)).astype(np.float32) for s in sizes]
    atoms = [np.eye(4, dtype=np.float32)[np.arange(s) % 4] for s in sizes]
    batch = structures_to_batch(atoms, pos, cutoff=cutoff)
    gp = batch.graph_ptr_host.astype(np.int64)
    S, B, _ = _check_kernel(batch, np.concatenate(pos), gp, None, rng)
    for f, s in enumerate(sizes):
        if s == 1:
            assert (S[f] == 0).all()


def test_kernel_one_large_frame():
    """more chunks than the 64 lanes of the frame pass"""
    from nmrgnn_amd.graph import frames_to_batch
    rng = np.random.default_rng(12)
    dims, vecs = _box("dodecahedron", 20000 / 0.1)
    frames = _atoms_in(vecs, 20000, rng)[None]
    batch = frames_to_batch(np.eye(4, dtype=np.float32)[np.arange(20000) % 4], frames, box=dims)
    _check_kernel(batch, frames, batch.graph_ptr_host.astype(np.int64), vecs[None], rng)


# ------------------------------------------------------------------------------------------------ 3: the identity
@pytest.mark.parametrize("form", ["knn", "cutoff"])
@pytest.mark.parametrize("kind", ["cube", "mixed"])
def test_identity_strain_positions_box(kind, form):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    from nmrgnn_amd.pbc import widths
    rng = np.random.default_rng(21)
    n = 400
    frames, dims, vecs = _frames(kind, n, rng)
    atoms = np.eye(4, dtype=np.float32)[np.arange(n) % 4]
    if form == "cutoff":
        batch = frames_to_batch_cutoff(atoms, frames, cutoff=0.45 * min(widths(v).min() for v in vecs), box=dims)
    else:
        batch = frames_to_batch(atoms, frames, box=dims)
    ddt = torch.from_numpy(_random_dd(batch, rng)).to(_dev())
    S, B = (x.cpu().numpy() for x in batch.box_grad(ddt))
    dpos = batch.positions_grad(ddt).cpu().numpy().astype(np.float64)
    r = frames.astype(np.float64)
    rhs = np.einsum("gia,gib->gab", r, dpos) + np.einsum("gka,gkb->gab", vecs, B)
    total = np.einsum("gia,gib->gab", np.abs(r), np.abs(dpos)) + np.einsum("gka,gkb->gab", np.abs(vecs), np.abs(B))
    for g in range(3):
        assert np.abs(S[g] - rhs[g]).max() <= 1e-5 * total[g].max(), (g, np.abs(S[g] - rhs[g]).max(), total[g].max())


# ------------------------------------------------------------------------------------------------ 4, 5: end to end
def _protein():
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(os.path.join(HERE, "data", "7lgi.pdb.gz"))
    return atoms_onehot(s.elements), np.asarray(s.frames[0], np.float32)


def _model(seed=3):
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    m = GNNModel(make_hp(atom_feature_size=64), load_standards(), device=_dev(), seed=seed)
    return m


def _wrapped_frames(p, kind, rng, shared=False):
    """two 7lgi frames (the second jittered) wrapped into boxes of their extent + 12 A (or more): [2, n, 3], dims [2, 6].
    ``shared``: both frames in the second frame's box"""
    from nmrgnn_amd.pbc import triclinic_vectors, widths
    ext = float((p.max(0) - p.min(0)).max()) + 13.0
    boxes = []
    for g in range(2):
        if kind == "ortho":
            e = p.max(0) - p.min(0) + 13.0 + 5.0 * g
            boxes.append(np.array([e[0], e[1], e[2], 90, 90, 90], np.float64))
        else:
            d = np.array([1.0, 1.0, 1.0, 60, 60, 90]) if g == 0 else np.array([1.0, 1.0, 1.0, OCT, 180 - OCT, OCT])
            d[:3] *= ext / widths(triclinic_vectors(d)).min() * (1.0 + 0.1 * g)
            boxes.append(d)
    if shared:
        boxes[0] = boxes[1]
    out, dims = [], []
    for g, shift in enumerate(([0.4, -0.7, 0.3], [3.1, 2.2, -0.9])):
        q = p + (0.05 * g) * rng.standard_normal(p.shape).astype(np.float32)
        d = boxes[g]
        v = triclinic_vectors(d).astype(np.float32).astype(np.float64)
        c = (q - q.mean(0) + np.array(shift)).astype(np.float64)
        f = c @ np.linalg.inv(v)
        out.append(((f - np.floor(f)) @ v).astype(np.float32))
        dims.append(d)
    return np.stack(out), np.stack(dims)


def _padded(batch):
    """(nlist [N, K] int64, live [N, K] bool) of the batch's lists, CSR rows padded"""
    if batch.is_csr:
        rp = batch.row_ptr.cpu().numpy().astype(np.int64)
        col = batch.nlist.cpu().numpy().astype(np.int64)
        deg = np.diff(rp)
        rows = np.repeat(np.arange(batch.N), deg)
        slot = np.arange(len(col)) - rp[rows]
        nlist = np.zeros((batch.N, int(deg.max())), np.int64)
        live = np.zeros_like(nlist, dtype=bool)
        nlist[rows, slot] = col
        live[rows, slot] = True
        return nlist, live
    return batch.nlist.cpu().numpy().astype(np.int64), batch.edges.detach().cpu().numpy() > 0


class _RefEnergy:
    """float64 torch E(pos [N, 3], h [G, 3, 3]) of the restraint over the batch's own lists and the float64 minimum images
    of the starting positions, both held fixed"""

    def __init__(self, model, atoms, batch, frames, vecs, targets, w):
        from oracle import torch_ref
        self.G, self.n = frames.shape[:2]
        N = self.G * self.n
        self.nlist, self.live = _padded(batch)
        self.src = np.broadcast_to(np.arange(N)[:, None], self.nlist.shape)
        self.frame = torch.from_numpy(np.arange(N) // self.n)
        p = frames.reshape(N, 3).astype(np.float64)
        d = p[self.nlist] - p[self.src]
        img = np.zeros_like(d)
        for g in range(self.G):
            rows = slice(g * self.n, (g + 1) * self.n)
            img[rows] = _mic_images(d[rows].reshape(-1, 3), vecs[g]).reshape(d[rows].shape)
        self.img = torch.from_numpy(img)
        self.params = torch_ref.to_torch_params(model.get_weights())
        self.hp = hp_to_oracle(model.hypers)
        C_ = atoms.shape[1]
        self.std, self.avg = model.peak_std[:C_], model.peak_avg[:C_]
        self.atoms = np.tile(atoms, (self.G, 1))
        self.inv = batch.inv_degree.cpu().numpy()
        self.scale = batch.scale
        self.targets = torch.from_numpy(targets.astype(np.float64))
        self.w = torch.from_numpy(w.astype(np.float64))
        self.fwd = torch_ref.forward

    def __call__(self, pos, h):
        nl, src = torch.from_numpy(self.nlist), torch.from_numpy(np.ascontiguousarray(self.src))
        u = pos[nl] - pos[src] + torch.einsum("nkc,ncd->nkd", self.img, h[self.frame])
        dist = torch.sqrt((u * u).sum(-1).clamp_min(1e-300)) * self.scale
        dd = torch.where(torch.from_numpy(self.live), dist, torch.zeros_like(dist))
        peaks = self.fwd((self.atoms, self.nlist, dd, self.inv), self.params, self.hp, peak_std=self.std, peak_avg=self.avg)
        return ((peaks - self.targets) ** 2 * self.w).sum()

    def strain(self, frames, vecs):
        """dE/d(eps_g) of r -> r (I + eps_g), h_g -> h_g (I + eps_g) at eps = 0, per frame [G, 3, 3]"""
        eps = torch.zeros(self.G, 3, 3, dtype=torch.float64, requires_grad=True)
        T = torch.eye(3, dtype=torch.float64) + eps
        pos = torch.from_numpy(frames.reshape(-1, 3).astype(np.float64))
        self(torch.einsum("nc,ncd->nd", pos, T[self.frame]), torch.einsum("gkc,gcd->gkd", torch.from_numpy(vecs), T)).backward()
        return eps.grad.numpy()


def _restraint_dedges(model, batch, targets, w):
    edges = batch.edges.requires_grad_(True)
    peaks = model(batch)
    ((peaks - torch.from_numpy(targets).to(_dev())) ** 2 * torch.from_numpy(w).to(_dev())).sum().backward()
    return edges.grad


@pytest.mark.parametrize("cutoff", [None, 4.0], ids=["knn", "cutoff"])
@pytest.mark.parametrize("kind", ["ortho", "tric"])
def test_strain_derivative_against_float64(kind, cutoff):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    from nmrgnn_amd.pbc import triclinic_vectors
    atoms, p = _protein()
    rng = np.random.default_rng(5)
    frames, dims = _wrapped_frames(p, kind, rng)
    vecs = np.stack([triclinic_vectors(d).astype(np.float32).astype(np.float64) for d in dims])
    G, n = frames.shape[:2]
    model = _model()
    model.build(atoms.shape[1])
    targets = rng.standard_normal(G * n).astype(np.float32) * 2.0
    wt = (rng.random(G * n) < 0.8).astype(np.float32)
    batch = frames_to_batch(atoms, frames, box=dims) if cutoff is None else \
        frames_to_batch_cutoff(atoms, frames, cutoff=cutoff, box=dims)
    assert batch.box_triclinic == (kind == "tric")
    S = batch.box_grad(_restraint_dedges(model, batch, targets, wt))[0].cpu().numpy()
    ref = _RefEnergy(model, atoms, batch, frames, vecs, targets, wt).strain(frames, vecs)
    err = float(np.abs(S - ref).max() / np.abs(ref).max())
    print(f"strain {kind} cutoff={cutoff}: max rel err {err:.2e}")
    assert err <= 1e-4, err


@pytest.mark.parametrize("shared", [True, False], ids=["shared6", "perframe"])
@pytest.mark.parametrize("kind", ["ortho", "tric"])
def test_box_grad_autograd_against_float64(kind, shared):
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.pbc import triclinic_vectors_torch
    atoms, p = _protein()
    rng = np.random.default_rng(6)
    frames, dims = _wrapped_frames(p, kind, rng, shared)
    if shared:
        dims = dims[1]
    G, n = frames.shape[:2]
    model = _model()
    model.build(atoms.shape[1])
    targets = rng.standard_normal(G * n).astype(np.float32) * 2.0
    wt = (rng.random(G * n) < 0.8).astype(np.float32)

    def loss_of(batch):
        peaks = model(batch)
        return ((peaks - torch.from_numpy(targets).to(_dev())) ** 2 * torch.from_numpy(wt).to(_dev())).sum()

    pos = torch.tensor(frames, device=_dev(), requires_grad=True)
    box_t = torch.tensor(dims, dtype=torch.float64, requires_grad=True)
    batch = frames_to_batch(atoms, pos, box=box_t)
    ref_batch = frames_to_batch(atoms, frames, box=box_t.detach().cpu().numpy())
    for name in ("nlist", "edges", "inv_degree"):
        assert torch.equal(getattr(batch, name).detach(), getattr(ref_batch, name)), name
    loss_of(batch).backward()
    got = box_t.grad
    assert got is not None and got.dtype == torch.float64 and got.shape == box_t.shape
    pos2 = torch.tensor(frames, device=_dev(), requires_grad=True)           # pos.grad does not depend on the box's grad
    loss_of(frames_to_batch(atoms, pos2, box=dims)).backward()
    assert torch.equal(pos.grad, pos2.grad)
    # float64: h from the restated conversion, lists and images fixed
    vecs = triclinic_vectors_torch(torch.tensor(dims)).expand(G, 3, 3).numpy() if shared else \
        triclinic_vectors_torch(torch.tensor(dims)).numpy()
    E = _RefEnergy(model, atoms, batch, frames, vecs, targets, wt)
    d64 = torch.tensor(dims, dtype=torch.float64, requires_grad=True)
    h = triclinic_vectors_torch(d64)
    E(torch.from_numpy(frames.reshape(-1, 3).astype(np.float64)), h.expand(G, 3, 3) if shared else h).backward()
    ref = d64.grad.numpy()
    err = float(np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max())
    print(f"box.grad {kind} shared={shared}: max rel err {err:.2e}")
    assert err <= 1e-4, err


def test_box_grad_without_grad_box_is_the_old_batch():
    """a box tensor that does not require grad: no grad_fn on a batch from plain frames"""
    from nmrgnn_amd.graph import frames_to_batch
    rng = np.random.default_rng(9)
    dims, vecs = _box("cube", 3000.0)
    frames = _atoms_in(vecs, 300, rng)[None]
    atoms = np.eye(4, dtype=np.float32)[np.arange(300) % 4]
    b = frames_to_batch(atoms, frames, box=torch.tensor(dims))
    assert b.edges.grad_fn is None
    ref = frames_to_batch(atoms, frames, box=dims)
    assert torch.equal(b.edges, ref.edges) and torch.equal(b.nlist, ref.nlist)


# ------------------------------------------------------------------------------------------------ 6: invariances
@pytest.mark.parametrize("form", ["knn", "cutoff"])
@pytest.mark.parametrize("kind", ["cube", "octahedron", "skew"])
def test_invariances(kind, form):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    from nmrgnn_amd.pbc import widths
    rng = np.random.default_rng(31)
    n = 400
    dims, vecs = _box(kind, n / 0.1)
    frames = _atoms_in(vecs, n, rng, moved=0.0)[None]
    atoms = np.eye(4, dtype=np.float32)[np.arange(n) % 4]
    batch = frames_to_batch_cutoff(atoms, frames, cutoff=0.45 * widths(vecs).min(), box=dims) if form == "cutoff" else \
        frames_to_batch(atoms, frames, box=dims)
    dd = _random_dd(batch, rng)
    ddt = torch.from_numpy(dd).to(_dev())
    S0, B0 = (x.cpu().numpy()[0] for x in batch.box_grad(ddt))
    _, _, su, _ = _ref_sb(batch, frames, batch.graph_ptr_host.astype(np.int64), vecs[None], dd, batch.scale)
    rows, _, g, _ = _edges_of(batch, dd)
    sp = float(np.abs(g).sum()) * batch.scale                 # sum |p|
    pos0 = batch.positions

    def at(moved):
        batch.positions = torch.from_numpy(np.ascontiguousarray(moved, np.float32)).to(_dev())   # same lists, moved atoms
        try:
            return [x.cpu().numpy()[0] for x in batch.box_grad(ddt)]
        finally:
            batch.positions = pos0

    # single atoms by whole lattice vectors: S unchanged (B changes with the images)
    sel = rng.random(n) < 0.3
    moved = frames.copy()
    moved[0, sel] = (frames[0, sel].astype(np.float64) + rng.integers(-3, 4, (int(sel.sum()), 3)) @ vecs).astype(np.float32)
    q = float(np.spacing(np.float32(np.abs(moved).max())))
    S1, _ = at(moved)
    assert np.abs(S1 - S0).max() <= 1e-6 * su[0] + 4.0 * q * sp, np.abs(S1 - S0).max()
    # a rigid translation: S and B unchanged
    moved = (frames.astype(np.float64) + np.array([3.7, -11.2, 5.3])).astype(np.float32)
    q = float(np.spacing(np.float32(np.abs(moved).max())))
    S2, B2 = at(moved)
    assert np.abs(S2 - S0).max() <= 1e-6 * su[0] + 4.0 * q * sp, np.abs(S2 - S0).max()
    assert np.abs(B2 - B0).max() <= 1e-6 * np.abs(B0).max() + 4.0 * q * sp, np.abs(B2 - B0).max()


# ------------------------------------------------------------------------------------------------ 7: shift_restraint
@pytest.mark.parametrize("boxed", [False, True], ids=["open", "box"])
def test_shift_restraint_virial(boxed):
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.library import shift_restraint
    from nmrgnn_amd.pbc import triclinic_vectors
    atoms, p = _protein()
    rng = np.random.default_rng(8)
    frames, dims = _wrapped_frames(p, "ortho", rng)
    w = frames[0]
    d = dims[0] if boxed else None
    n = p.shape[0]
    model = _model()
    model.build(atoms.shape[1])
    targets = rng.standard_normal(n).astype(np.float32)
    wt = rng.random(n).astype(np.float32)
    e0, f0 = shift_restraint(model, atoms, w, targets, wt, box=d)
    e1, f1, vir = shift_restraint(model, atoms, w, targets, wt, box=d, virial=True)
    assert torch.equal(e0, e1) and torch.equal(f0, f1)
    assert vir.dtype == torch.float64 and tuple(vir.shape) == (3, 3)
    # the same dedges as shift_restraint computes them
    eng = model.engine
    batch = frames_to_batch(atoms, w, device=eng.device, box=d)
    y = torch.from_numpy(targets).to(_dev())
    wd = torch.from_numpy(wt).to(_dev())
    peaks = eng.forward(batch, training=False, keep_tape=True)
    dedges = torch.empty(batch.edges.shape, dtype=torch.float32, device=_dev())
    eng.backward(wd * (2.0 * (peaks - y)), edge_grad=dedges)
    assert torch.equal(vir, -batch.box_grad(dedges)[0][0])
    vecs = (triclinic_vectors(d) if boxed else np.eye(3) * 1e4).astype(np.float32).astype(np.float64)[None]
    ref = -_RefEnergy(model, atoms, batch, w[None], vecs, targets, wt).strain(w[None], vecs)[0]
    err = float(np.abs(vir.cpu().numpy() - ref).max() / np.abs(ref).max())
    print(f"virial box={boxed}: max rel err {err:.2e}")
    assert err <= 1e-4, err
