"""Replica-averaged shift restraint on the GPU: ng_restraint_loss against NumPy, the weight-gradient-free backward
(Engine.backward(param_grad=False)) against the full one bit for bit on every edge path and list form, ShiftRestraint with
R = 1 against shift_restraint, R = 4 against float64 torch autograd through oracle/torch_ref, replay against the eager
chain, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import hp_to_oracle, make_hp, randomize_biases, small_batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OCT = float(np.degrees(np.arccos(1.0 / 3.0)))


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ------------------------------------------------------------------------------------------------ 1: ng_restraint_loss
def _loss(ctx, R, n, peaks, y, w):
    from nmrgnn_amd._lib import ptr
    e = torch.full((1,), np.nan, dtype=torch.float64, device=_dev())
    dp = torch.full((R * n,), np.nan, dtype=torch.float32, device=_dev())
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    ctx.check(ctx.lib.ng_restraint_loss(ctx.handle, st, R, n, ptr(peaks), ptr(y), ptr(w), ptr(e), ptr(dp)), "ng_restraint_loss")
    torch.cuda.synchronize()
    return e, dp


@pytest.mark.parametrize("n", [1, 2770, 100000])
@pytest.mark.parametrize("R", [1, 2, 8])
def test_restraint_loss_kernel_against_numpy(R, n):
    from nmrgnn_amd import _lib
    ctx = _lib.get_context(0)
    rng = np.random.default_rng(R * 1000 + n)
    peaks = (rng.standard_normal(R * n) * 30.0 + 50.0).astype(np.float32)
    y = (rng.standard_normal(n) * 30.0 + 50.0).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    w[rng.random(n) < 0.3] = 0.0
    dev = lambda a: torch.from_numpy(a).to(_dev())
    e, dp = _loss(ctx, R, n, dev(peaks), dev(y), dev(w))
    # the float32 expressions, in the kernel's order
    s = peaks.reshape(R, n)[0].copy()
    for r in range(1, R):
        s = (s + peaks.reshape(R, n)[r]).astype(np.float32)
    mean = (s / np.float32(R)).astype(np.float32)
    diff = (mean - y).astype(np.float32)
    g = ((w * (np.float32(2.0) * diff)).astype(np.float32) / np.float32(R)).astype(np.float32)
    assert np.array_equal(dp.cpu().numpy().view(np.int32), np.tile(g, R).view(np.int32))
    if R == 1:       # the bits of shift_restraint's w * (2.0 * diff) through torch
        pt, yt, wt = dev(peaks), dev(y), dev(w)
        assert torch.equal(_bits(dp), _bits(wt * (2.0 * (pt - yt))))
    terms = ((diff * diff).astype(np.float32) * w).astype(np.float32).astype(np.float64)
    ref = float(np.sum(terms))
    assert abs(float(e[0]) - ref) <= 1e-12 * abs(ref), (float(e[0]), ref)
    e2, dp2 = _loss(ctx, R, n, dev(peaks), dev(y), dev(w))
    assert torch.equal(_bits(e), _bits(e2)) and torch.equal(_bits(dp), _bits(dp2))


# ------------------------------------------------------------------------------------------------ 2: backward, no weight grads
def _engine(F, seed=5, **kw):
    from nmrgnn_amd.engine import Engine
    hp = make_hp(atom_feature_size=F, **kw)
    eng = Engine(hp, 10, device=_dev(), seed=seed)
    randomize_biases(eng, seed=seed)
    return hp, eng


# (edge path or list form, kernel-path switches): the F = 64 window / fused FC / fast head kernels by default; "layered" the
# generic MPLayer, the layered FC block and the generic head; "fp32" the fp32-input bodies of the fused kernels
BWD_CASES = [("slots", ""), ("live", ""), ("table", ""), ("table_host", ""), ("csr", ""), ("live", "layered"),
             ("live", "fp32"), ("csr", "layered")]


@pytest.mark.parametrize("F", [64, 256])
@pytest.mark.parametrize("case,switch", BWD_CASES, ids=[f"{c}-{s or 'default'}" for c, s in BWD_CASES])
def test_backward_without_weight_gradients_is_bitwise(F, case, switch, monkeypatch):
    from nmrgnn_amd.graph import GraphBatch
    if switch == "layered":
        monkeypatch.setenv("NG_MP_PATH", "layered")
        monkeypatch.setenv("NG_FC_PATH", "layered")
        monkeypatch.setenv("NG_HEAD_PATH", "generic")
    elif switch == "fp32":
        monkeypatch.setenv("NG_GEMM_MATH", "fp32")
    kw = dict(edge_hidden_size=64) if case == "table_host" else {}
    hp, eng = _engine(F, **kw)
    b = small_batch(3, 60, 16, 10, seed=3, p_pad=0.15)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=_dev())
    eng.edge_table = case in ("table", "table_host")
    eng.use_live_edges = case != "slots"
    if eng.edge_table:
        eng.edge_table_min_edges = 0
    if case == "csr":
        gb = gb.to_csr()
    N = gb.N
    rng = np.random.default_rng(11)
    dpeaks = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(_dev())

    def run(param_grad):
        peaks = eng.forward(gb, training=False, keep_tape=True)
        path = eng.tape.edge_path
        out = torch.full(gb.edges.shape, 7.0, device=_dev())
        eng.backward(dpeaks, edge_grad=out, param_grad=param_grad)
        torch.cuda.synchronize()
        return peaks.clone(), out, path

    eng.params.grad.zero_()
    p1, e1, path1 = run(True)
    g1 = eng.params.grad.clone()
    assert torch.isfinite(g1).all()
    eng.params.grad.fill_(float("nan"))
    poisoned = _bits(eng.params.grad).clone()
    p0, e0, path0 = run(False)
    if case != "csr":
        assert path0 == path1 == case, (path0, path1)
    assert torch.equal(p0, p1)
    assert torch.equal(_bits(e0), _bits(e1))                       # dL/d(edges): the same bits
    assert torch.equal(_bits(eng.params.grad), poisoned)           # params.grad untouched
    assert eng.tape is None
    # and the full backward after it is the same as before (nothing left queued or half-reduced)
    eng.params.grad.zero_()
    p2, e2, _ = run(True)
    assert torch.equal(_bits(e2), _bits(e1)) and torch.equal(eng.params.grad, g1)


def test_backward_param_grad_false_refusals():
    from nmrgnn_amd.graph import GraphBatch
    hp, eng = _engine(64)
    b = small_batch(2, 40, 16, 10, seed=4)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=_dev())
    eng.forward(gb, training=False, keep_tape=True)
    dp = torch.ones(gb.N, device=_dev())
    with pytest.raises(ValueError):
        eng.backward(dp, param_grad=False)
    with pytest.raises(ValueError):
        eng.backward(dp, edge_grad=torch.empty_like(gb.edges), param_grad=False, on_node_grads=lambda: None)
    assert eng.tape is not None           # refused before any work: the tape is still there
    eng.backward(dp, edge_grad=torch.empty_like(gb.edges), param_grad=False)


# ------------------------------------------------------------------------------------------------ structures and models
def _structure(name):
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(os.path.join(HERE, "data", name))
    return atoms_onehot(s.elements), np.asarray(s.frames[0], np.float32)


def _model(seed=3, **kw):
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    kw.setdefault("atom_feature_size", 64)
    return GNNModel(make_hp(**kw), load_standards(), device=_dev(), seed=seed)


def _box_dims(p, kind, grow=0.0):
    """a box around the structure p (extent + 13 A): None, orthorhombic, or the rhombic dodecahedron of §7.3"""
    from nmrgnn_amd.pbc import triclinic_vectors, widths
    if kind == "none":
        return None
    e = p.max(0) - p.min(0) + 13.0 + grow
    if kind == "ortho":
        return np.array([e[0], e[1], e[2], 90, 90, 90], np.float64)
    d = np.array([1.0, 1.0, 1.0, 60, 60, 90])
    d[:3] *= (float(e.max())) / widths(triclinic_vectors(d)).min()
    return d


def _frames(p, R, rng, sigma=0.05):
    return np.stack([p + (sigma * r) * rng.standard_normal(p.shape).astype(np.float32) for r in range(R)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 3: R = 1 vs shift_restraint
@pytest.mark.parametrize("name,kind", [("108M.pdb", "none"), ("7lgi.pdb.gz", "none"), ("7lgi.pdb.gz", "ortho"),
                                       ("108M.pdb", "tric")])
def test_one_replica_equals_shift_restraint(name, kind):
    from nmrgnn_amd.library import ShiftRestraint, shift_restraint
    atoms, p = _structure(name)
    n = p.shape[0]
    rng = np.random.default_rng(2)
    targets = (rng.standard_normal(n) * 3.0).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    w[rng.random(n) < 0.2] = 0.0
    box = _box_dims(p, kind)
    model = _model()
    model.build(atoms.shape[1])
    e_ref, f_ref, v_ref = shift_restraint(model, atoms, p, targets, w, box=box, virial=True)
    for replay in (True, False):
        r = ShiftRestraint(model, atoms, targets, w, box=box, virial=True, replay=replay)
        e, f, v = r(p, box=box)
        torch.cuda.synchronize()
        assert f.shape == (n, 3) and v.shape == (1, 3, 3) and e.dtype == torch.float32 and e.dim() == 0
        assert torch.equal(_bits(f), _bits(f_ref)), replay
        assert torch.equal(_bits(v[0]), _bits(v_ref)), replay
        assert abs(float(e) - float(e_ref)) <= 1e-6 * abs(float(e_ref)), (float(e), float(e_ref))
        e2, f2 = ShiftRestraint(model, atoms, targets, w, box=box, replay=replay)(p, box=box)
        assert torch.equal(_bits(f2), _bits(f_ref))


# ------------------------------------------------------------------------------------------------ 4: R = 4 vs float64 autograd
def _mic_images(d, vecs):
    """integer image triples m with u = d + m h the float64 minimum image: a fractional reduction, then [-2, 2]^3"""
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


class _RefEnergy:
    """float64 torch E(pos [R*n, 3], h [R, 3, 3]) of the replica-averaged restraint over the restraint's own lists (read
    back from its batch) and the float64 minimum images of the starting positions, both held fixed"""

    def __init__(self, model, atoms, batch, frames, vecs, targets, w):
        from oracle import torch_ref
        self.R, self.n = frames.shape[:2]
        N = self.R * self.n
        self.nlist = batch.nlist.cpu().numpy().astype(np.int64)
        self.live = batch.edges.detach().cpu().numpy() > 0
        self.src = np.broadcast_to(np.arange(N)[:, None], self.nlist.shape)
        self.frame = torch.from_numpy(np.arange(N) // self.n)
        p = frames.reshape(N, 3).astype(np.float64)
        d = p[self.nlist] - p[self.src]
        img = np.zeros_like(d)
        if vecs is not None:
            for g in range(self.R):
                rows = slice(g * self.n, (g + 1) * self.n)
                img[rows] = _mic_images(d[rows].reshape(-1, 3), vecs[g]).reshape(d[rows].shape)
        self.vecs = np.zeros((self.R, 3, 3)) if vecs is None else vecs
        self.img = torch.from_numpy(img)
        self.params = torch_ref.to_torch_params(model.get_weights())
        self.hp = hp_to_oracle(model.hypers)
        C_ = atoms.shape[1]
        self.std, self.avg = model.peak_std[:C_], model.peak_avg[:C_]
        self.atoms = np.tile(atoms, (self.R, 1))
        self.inv = batch.inv_degree.cpu().numpy()
        self.targets = torch.from_numpy(targets.astype(np.float64))
        self.w = torch.from_numpy(w.astype(np.float64))
        self.fwd = torch_ref.forward

    def __call__(self, pos, h):
        nl, src = torch.from_numpy(self.nlist), torch.from_numpy(np.ascontiguousarray(self.src))
        u = pos[nl] - pos[src] + torch.einsum("nkc,ncd->nkd", self.img, h[self.frame])
        dist = torch.sqrt((u * u).sum(-1).clamp_min(1e-300)) * 0.1
        dd = torch.where(torch.from_numpy(self.live), dist, torch.zeros_like(dist))
        peaks = self.fwd((self.atoms, self.nlist, dd, self.inv), self.params, self.hp, peak_std=self.std, peak_avg=self.avg)
        mean = peaks.reshape(self.R, self.n).mean(0)
        return ((mean - self.targets) ** 2 * self.w).sum()

    def all(self, frames):
        """(E, dE/dpos [R, n, 3], strain dE/d(eps_r) [R, 3, 3]) at the starting positions"""
        eps = torch.zeros(self.R, 3, 3, dtype=torch.float64, requires_grad=True)
        T = torch.eye(3, dtype=torch.float64) + eps
        pos = torch.from_numpy(frames.reshape(-1, 3).astype(np.float64)).requires_grad_(True)
        E = self(torch.einsum("nc,ncd->nd", pos, T[self.frame]), torch.einsum("gkc,gcd->gkd", torch.from_numpy(self.vecs), T))
        E.backward()
        return float(E.detach()), pos.grad.numpy().reshape(frames.shape), eps.grad.numpy()


@pytest.mark.parametrize("kind", ["none", "ortho", "tric"])
def test_four_replicas_against_float64_autograd(kind):
    from nmrgnn_amd.library import ShiftRestraint
    from nmrgnn_amd.pbc import triclinic_vectors
    atoms, p = _structure("108M.pdb")
    n = p.shape[0]
    R = 4
    rng = np.random.default_rng(4)
    frames = _frames(p, R, rng, sigma=0.1)
    targets = (rng.standard_normal(n) * 3.0).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    w[rng.random(n) < 0.2] = 0.0
    box = _box_dims(p, kind)
    boxes = None if box is None else np.stack([box * np.array([1 + 0.02 * r] * 3 + [1] * 3) for r in range(R)])
    if boxes is not None:       # every replica wrapped into its box with the protein across the faces: edges through images
        for k in range(R):
            v = triclinic_vectors(boxes[k]).astype(np.float32).astype(np.float64)
            c = frames[k] - frames[k].mean(0) + np.array([0.4, -0.7, 0.3])
            f = c @ np.linalg.inv(v)
            frames[k] = ((f - np.floor(f)) @ v).astype(np.float32)
    model = _model()
    model.build(atoms.shape[1])
    r = ShiftRestraint(model, atoms, targets, w, replicas=R, box=boxes, virial=True)
    e, f, v = r(frames, box=boxes)
    torch.cuda.synchronize()
    vecs = None if boxes is None else np.stack([triclinic_vectors(b).astype(np.float32).astype(np.float64) for b in boxes])
    ref = _RefEnergy(model, atoms, r._batch, frames, vecs, targets, w)
    if vecs is not None:
        assert np.abs(ref.img.numpy()).sum() > 0          # some lists edges do go through images
    E, dpos, strain = ref.all(frames)
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())
    errs = (abs(float(e) - E) / abs(E), rel(f.cpu().numpy(), -dpos), rel(v.cpu().numpy(), -strain))
    print(f"R=4 {kind}: energy {errs[0]:.2e} forces {errs[1]:.2e} virial {errs[2]:.2e}")
    assert max(errs) <= 1e-4, errs


# ------------------------------------------------------------------------------------------------ 5: replay vs eager
REPLAY_CASES = [("108M.pdb", 2, "ortho", {}), ("108M.pdb", 3, "tric", {}), ("7lgi.pdb.gz", 8, "none", {}),
                ("7lgi.pdb.gz", 8, "none", dict(edge_hidden_size=64))]


@pytest.mark.parametrize("name,R,kind,kw", REPLAY_CASES, ids=["108M-R2-ortho", "108M-R3-tric", "7lgi-R8", "7lgi-R8-H64"])
def test_replay_equals_eager_over_calls(name, R, kind, kw):
    from nmrgnn_amd.library import ShiftRestraint
    atoms, p = _structure(name)
    n = p.shape[0]
    rng = np.random.default_rng(6)
    targets = (rng.standard_normal(n) * 3.0).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    model = _model(**kw)
    model.build(atoms.shape[1])
    box0 = _box_dims(p, kind)
    virial = box0 is not None
    ra = ShiftRestraint(model, atoms, targets, w, replicas=R, box=box0, virial=virial)
    rb = ShiftRestraint(model, atoms, targets, w, replicas=R, box=box0, virial=virial, replay=False)
    if R * n * 16 >= model.engine.edge_table_min_edges:
        assert ra._batch.n_edges >= 262144
    for call in range(5):
        frames = _frames(p, R, rng, sigma=0.05 + 0.02 * call)
        box = None if box0 is None else _box_dims(p, kind, grow=0.5 * call)
        outa = [t.clone() for t in ra(frames, box=box)]
        outb = [t.clone() for t in rb(frames, box=box)]
        torch.cuda.synchronize()
        for x, y in zip(outa, outb):
            assert torch.equal(_bits(x), _bits(y)), call
        assert torch.isfinite(outa[1]).all() and float(outa[0]) > 0


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals():
    from nmrgnn_amd.library import ShiftRestraint
    from nmrgnn_amd.train import Trainer
    atoms, p = _structure("108M.pdb")
    n = p.shape[0]
    targets = np.zeros(n, np.float32)
    model = _model()
    model.build(atoms.shape[1])
    box = _box_dims(p, "ortho")
    r2 = ShiftRestraint(model, atoms, targets, replicas=2)
    fr = np.stack([p, p])
    with pytest.raises(ValueError):
        r2(p)                                  # [n, 3] for R = 2
    with pytest.raises(ValueError):
        r2(np.stack([p, p, p]))                # R mismatch
    with pytest.raises(ValueError):
        r2(fr[:, :-1])                         # atom count
    with pytest.raises(ValueError):
        r2(fr, box=box)                        # a box where none was given
    rb = ShiftRestraint(model, atoms, targets, box=box)
    with pytest.raises(ValueError):
        rb(p)                                  # none where one was
    with pytest.raises(ValueError):
        rb(p, box=_box_dims(p, "tric"))        # the other kind
    with pytest.raises(ValueError):
        rb(p, box=np.stack([box, box]))        # [R', 6] for R = 1
    with pytest.raises(ValueError):
        rb(p, box=np.array([30.0, 30.0, 30.0, 90.0, 90.0, 40.0]))     # not a reduced box: pbc.prepare refuses
    e, f = rb(p, box=box)
    assert torch.isfinite(f).all()
    # a training step changes the weights: the captured chain would read stale ones
    from nmrgnn_amd.graph import frames_to_batch
    tr = Trainer(model.engine, lr=1e-3)
    gb = frames_to_batch(atoms, p)
    tr.step(gb, torch.zeros(n, device=_dev()), torch.ones(n, device=_dev()))
    with pytest.raises(ValueError):
        r2(fr)
    with pytest.raises(ValueError):
        rb(p, box=box)
    tr.close()
    r3 = ShiftRestraint(model, atoms, targets, replicas=2)     # a new restraint sees the new weights
    e3, f3 = r3(fr)
    assert torch.isfinite(f3).all()
