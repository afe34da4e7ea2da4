"""Gradients with respect to the inputs: ng_edge_mlp_dinput (d e / d distance), Engine.backward(edge_grad=...),
ng_positions_grad(_csr), the autograd surface (edges / positions requiring grad) and library.shift_restraint — each
against float64 torch autograd of the same function."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import hp_to_oracle, make_hp, randomize_biases, small_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = {"none": 0, "softplus": 1, "relu": 2, "tanh": 3}


def _dev():
    return torch.device("cuda", 0)


def _lib_ctx():
    from nmrgnn_amd import _lib
    return _lib.get_context(0)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


# ---------------------------------------------------------------------------------------------------------------- kernel 1
def _act64(name):
    return {"none": lambda x: x, "softplus": torch.nn.functional.softplus, "relu": torch.relu, "tanh": torch.tanh}[name]


def _edge_fn64(d, d_src, centers, gap, W, B, act):
    """the edge function e(d) in float64 torch (nmrgnn/model.py:251-261, nmrgnn/layers.py:137-140)"""
    mask = (d_src > 0).to(torch.float64)[:, None]
    x = torch.exp(-(d[:, None] - centers[None, :]) ** 2 / gap) * mask
    f = _act64(act)
    for t in range(len(W) - 1):
        x = f(x @ W[t] + B[t])
    return (x @ W[-1] + B[-1]) * mask


def _edge_case(n, H, E, Le, act, seed, dead=0.1, zero_preact=False):
    from nmrgnn_amd.engine import rbf_grid
    rng = np.random.default_rng(seed)
    centers, gap = rbf_grid(0.005, 0.20, H)
    d_src = rng.uniform(0.01, 0.21, n).astype(np.float32)
    d_src[rng.random(n) < dead] = 0.0
    d_eff = (d_src + 0.01 * rng.standard_normal(n)).astype(np.float32)
    W, B = [], []
    for t in range(Le):
        kout = H if t < Le - 1 else E
        W.append((rng.standard_normal((H, kout)) * np.sqrt(2.0 / (H + kout))).astype(np.float32))
        B.append((0.1 * rng.standard_normal(kout)).astype(np.float32))
    if zero_preact:            # pre-activations exactly 0 in column 0 of every hidden layer: relu'(0) = 0
        for t in range(Le - 1):
            W[t][:, 0] = 0.0
            B[t][0] = 0.0
    de = rng.standard_normal((n, E)).astype(np.float32)
    return dict(centers=centers, gap=gap, d_src=d_src, d_eff=d_eff, W=W, B=B, de=de)


def _dinput(c, H, E, Le, act, compact=False, with_J=True):
    from nmrgnn_amd._lib import ptr, ptr_array
    ctx = _lib_ctx()
    dev = _dev()
    n = c["d_src"].shape[0]
    d_src = torch.from_numpy(c["d_src"]).to(dev)
    d_eff = torch.from_numpy(c["d_eff"]).to(dev)
    perm = n_live = None
    if compact:
        live = np.nonzero(c["d_src"] > 0)[0]
        perm_np = np.concatenate([live, np.nonzero(~(c["d_src"] > 0))[0]]).astype(np.int32)
        perm = torch.from_numpy(perm_np).to(dev)
        n_live = torch.tensor([len(live)], dtype=torch.int32, device=dev)
        garbage = np.full(n, np.nan, np.float32)          # rows past n_live are never read
        dsc, dec = garbage.copy(), garbage.copy()
        dsc[:len(live)] = c["d_src"][live]
        dec[:len(live)] = c["d_eff"][live]
        d_src, d_eff = torch.from_numpy(dsc).to(dev), torch.from_numpy(dec).to(dev)
    W = [torch.from_numpy(w).to(dev) for w in c["W"]]
    B = [torch.from_numpy(b).to(dev) for b in c["B"]]
    de = torch.from_numpy(c["de"]).to(dev)
    J = torch.full((n, E), 7.0, device=dev) if with_J else None
    dd = torch.full((n,), 7.0, device=dev)
    centers = torch.from_numpy(c["centers"]).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ctx.check(ctx.lib.ng_edge_mlp_dinput(ctx.handle, st, n, H, E, Le, ACTS[act], ptr(d_src), ptr(d_eff), ptr(perm),
                                         ptr(n_live), ptr(centers), float(c["gap"]), ptr_array(W), ptr_array(B), ptr(de),
                                         ptr(J), ptr(dd)), "ng_edge_mlp_dinput")
    torch.cuda.synchronize()
    return (J.cpu() if with_J else None), dd.cpu()


def _dinput_ref(c, act):
    d = torch.from_numpy(c["d_eff"].astype(np.float64))
    d_src = torch.from_numpy(c["d_src"].astype(np.float64))
    centers = torch.from_numpy(c["centers"].astype(np.float64))
    W = [torch.from_numpy(w.astype(np.float64)) for w in c["W"]]
    B = [torch.from_numpy(b.astype(np.float64)) for b in c["B"]]
    _, J = torch.func.jvp(lambda x: _edge_fn64(x, d_src, centers, float(c["gap"]), W, B, act), (d,), (torch.ones_like(d),))
    dd = (J * torch.from_numpy(c["de"].astype(np.float64))).sum(1)
    return J.numpy(), dd.numpy()


KERNEL_CASES = [
    # (n, H, E, Le, act)
    (3000, 128, 3, 4, "softplus"),      # the default shape
    (3000, 128, 1, 4, "softplus"),
    (3000, 128, 8, 4, "softplus"),
    (2000, 128, 64, 4, "softplus"),
    (3000, 16, 3, 4, "softplus"),
    (3000, 64, 3, 4, "softplus"),
    (2000, 256, 3, 4, "softplus"),
    (1000, 512, 3, 3, "softplus"),
    (3000, 128, 3, 2, "softplus"),
    (3000, 128, 3, 6, "softplus"),
    (3000, 128, 3, 4, "tanh"),
    (3000, 48, 3, 4, "none"),
    (500, 16, 256, 2, "tanh"),
    (1, 128, 3, 4, "softplus"),
    (100003, 16, 2, 3, "softplus"),     # more rows than one grid-stride trip covers (1024 tiles of 32)
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,E,Le,act", KERNEL_CASES, ids=[f"n{c[0]}-H{c[1]}-E{c[2]}-Le{c[3]}-{c[4]}" for c in KERNEL_CASES])
def test_edge_dinput_kernel_against_float64(n, H, E, Le, act):
    c = _edge_case(n, H, E, Le, act, seed=H * 7 + E + Le, dead=0.0 if n == 1 else 0.1)
    J, dd = _dinput(c, H, E, Le, act)
    Jr, ddr = _dinput_ref(c, act)
    assert _rel(J, Jr) <= 1e-5, _rel(J, Jr)
    assert _rel(dd, ddr) <= 1e-5, _rel(dd, ddr)
    dead = c["d_src"] <= 0
    assert np.all(J.numpy()[dead] == 0) and np.all(dd.numpy()[dead] == 0)


@pytest.mark.gpu
def test_edge_dinput_relu_with_zero_preactivations():
    c = _edge_case(3000, 128, 3, 4, "relu", seed=11, zero_preact=True)
    J, dd = _dinput(c, 128, 3, 4, "relu")
    Jr, ddr = _dinput_ref(c, "relu")
    assert _rel(J, Jr) <= 1e-5 and _rel(dd, ddr) <= 1e-5, (_rel(J, Jr), _rel(dd, ddr))


@pytest.mark.gpu
@pytest.mark.parametrize("H,E", [(128, 3), (256, 8), (16, 1)])
def test_edge_dinput_live_view_equals_every_slot_form(H, E):
    c = _edge_case(5000, H, E, 4, "softplus", seed=5, dead=0.3)
    J0, dd0 = _dinput(c, H, E, 4, "softplus")
    J1, dd1 = _dinput(c, H, E, 4, "softplus", compact=True)
    assert torch.equal(J0, J1) and torch.equal(dd0, dd1)
    _, dd2 = _dinput(c, H, E, 4, "softplus", with_J=False)
    assert torch.equal(dd0, dd2)


@pytest.mark.gpu
def test_edge_dinput_refuses_shapes_outside_its_range():
    from nmrgnn_amd import _lib
    c = _edge_case(64, 128, 3, 4, "softplus", seed=1)
    with pytest.raises(_lib.NGError):
        _dinput(c, 120, 3, 4, "softplus")
    c7 = _edge_case(64, 16, 3, 7, "softplus", seed=1)
    with pytest.raises(_lib.NGError):
        _dinput(c7, 16, 3, 7, "softplus")


# ---------------------------------------------------------------------------------------------------------------- engine
def _engine(seed=5, **kw):
    from nmrgnn_amd.engine import Engine
    hp = make_hp(atom_feature_size=64, **kw)
    eng = Engine(hp, 10, device=_dev(), seed=seed)
    randomize_biases(eng, seed=seed)
    return hp, eng


def _ref_edge_grad(b, sd, hp, dpeaks, training=False, xi=None, mask=None):
    """dL/d(edges) of L = sum(dpeaks * peaks) by float64 torch autograd of oracle.torch_ref.forward"""
    from oracle import torch_ref
    p = torch_ref.to_torch_params(sd)
    d = torch.tensor(np.asarray(b["edges"], np.float64), requires_grad=True)
    peaks = torch_ref.forward((b["atoms"], b["nlist"], d, b["inv_degree"]), p, hp_to_oracle(hp), training=training,
                              noise=xi, dropout_mask=mask)
    (peaks * torch.from_numpy(np.asarray(dpeaks, np.float64))).sum().backward()
    return d.grad.numpy()


def _run(eng, gb, dpeaks, training=False, xi=None, mask=None, edge_grad=True):
    peaks = eng.forward(gb, training=training, noise=xi, dropout_mask=mask, keep_tape=True)
    out = torch.full(gb.edges.shape, 7.0, device=_dev()) if edge_grad else None
    tape_path = eng.tape.edge_path
    eng.backward(dpeaks, edge_grad=out)
    torch.cuda.synchronize()
    return peaks.clone(), eng.params.grad.clone(), out, tape_path


ENGINE_CASES = ["slots", "live", "table", "table_host", "csr", "training"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ENGINE_CASES)
def test_engine_edge_grad_against_float64(case):
    from nmrgnn_amd.graph import GraphBatch
    kw = dict(edge_hidden_size=64) if case == "table_host" else {}
    hp, eng = _engine(**kw)
    b = small_batch(3, 60, 16, 10, seed=3, p_pad=0.15)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=_dev())
    eng.edge_table = case in ("table", "table_host")
    eng.use_live_edges = case != "slots"
    if eng.edge_table:
        eng.edge_table_min_edges = 0
    if case == "csr":
        gb = gb.to_csr()
    N, K = b["edges"].shape
    rng = np.random.default_rng(9)
    dpeaks = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(_dev())
    training = case == "training"
    xi = mask = None
    if training:
        xi = eng.randn(N * K, seed=1).reshape(N, K)
        mask = eng.dropout_mask(N * 32, seed=2).reshape(N, 32)
    p0, g0, _, path0 = _run(eng, gb, dpeaks, training, xi, mask, edge_grad=False)
    p1, g1, eg, path1 = _run(eng, gb, dpeaks, training, xi, mask)
    expect = {"slots": "slots", "live": "live", "table": "table", "table_host": "table_host"}.get(case)
    if expect:
        assert path1 == expect, path1
    assert path0 == path1
    assert torch.equal(p0, p1) and torch.equal(g0, g1)       # the parameter gradient does not see edge_grad
    ref = _ref_edge_grad(b, eng.params.state_dict(), hp, dpeaks.cpu().numpy(), training,
                         None if xi is None else xi.cpu().numpy(), None if mask is None else (mask.cpu().numpy() > 0))
    got = eg.cpu().numpy()
    if case == "csr":
        ref = ref[b["edges"] > 0]
    err = _rel(got, ref)
    print(f"edge_grad {case}: max rel err {err:.2e}")
    assert err <= 1e-4, err
    if case != "csr":
        assert np.all(got[b["edges"] <= 0] == 0)


# ---------------------------------------------------------------------------------------------------------------- positions
def _structure():
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(os.path.join(ROOT, "tests", "data", "108M.pdb"))
    return atoms_onehot(s.elements), np.asarray(s.frames[0], np.float32)


def _model(seed=3):
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    m = GNNModel(make_hp(atom_feature_size=64), load_standards(), device=_dev(), seed=seed)
    return m


def _ref_positions_grad(model, atoms, batch, frames, targets, w):
    """d/d positions of sum w (peaks - targets)^2 in float64: distances rebuilt from the positions over the batch's
    own lists (padded; a CSR batch is padded to its largest degree), torch_ref.forward, autograd"""
    from oracle import torch_ref
    G, n, _ = frames.shape
    pos = torch.tensor(frames.reshape(G * n, 3).astype(np.float64), requires_grad=True)
    N = G * n
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
    src = torch.arange(N)[:, None].expand_as(torch.from_numpy(nlist))
    v = pos[src] - pos[torch.from_numpy(nlist)]
    dist = torch.sqrt((v * v).sum(-1).clamp_min(1e-300)) * batch.scale
    d = torch.where(torch.from_numpy(live), dist, torch.zeros_like(dist))
    atoms_b = np.tile(atoms, (G, 1))
    p = torch_ref.to_torch_params(model.get_weights())
    C_ = atoms.shape[1]
    peaks = torch_ref.forward((atoms_b, nlist, d, batch.inv_degree.cpu().numpy()), p, hp_to_oracle(model.hypers),
                              peak_std=model.peak_std[:C_], peak_avg=model.peak_avg[:C_])
    y = torch.from_numpy(targets.astype(np.float64))
    ww = torch.from_numpy(w.astype(np.float64))
    ((peaks - y) ** 2 * ww).sum().backward()
    return pos.grad.numpy().reshape(G, n, 3)


def _check_invariance(frames, grad):
    """translation and rotation: per frame, sum of forces and of torques ~ 0 relative to their magnitudes"""
    for g in range(frames.shape[0]):
        f = grad[g].astype(np.float64)
        r = frames[g].astype(np.float64)
        r = r - r.mean(0)
        fsum = np.abs(f.sum(0)).max() / np.abs(f).sum()
        tq = np.cross(r, f)
        tsum = np.abs(tq.sum(0)).max() / np.abs(tq).sum()
        assert fsum < 1e-5 and tsum < 1e-4, (fsum, tsum)


@pytest.mark.gpu
@pytest.mark.parametrize("G,cutoff", [(1, None), (3, None), (2, 4.0)], ids=["knn-G1", "knn-G3", "cutoff-G2"])
def test_positions_grad_through_autograd_against_float64(G, cutoff):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    atoms, pos0 = _structure()
    n = pos0.shape[0]
    rng = np.random.default_rng(4)
    frames = np.stack([pos0 + 0.05 * rng.standard_normal(pos0.shape).astype(np.float32) for _ in range(G)])
    model = _model()
    model.build(atoms.shape[1])
    targets = rng.standard_normal(G * n).astype(np.float32) * 2.0
    w = (rng.random(G * n) < 0.8).astype(np.float32)
    pos = torch.tensor(frames, device=_dev(), requires_grad=True)
    batch = frames_to_batch(atoms, pos) if cutoff is None else frames_to_batch_cutoff(atoms, pos, cutoff=cutoff)
    assert batch.edges.grad_fn is not None
    peaks = model(batch)
    y, wt = torch.from_numpy(targets).to(_dev()), torch.from_numpy(w).to(_dev())
    ((peaks - y) ** 2 * wt).sum().backward()
    got = pos.grad.cpu().numpy()
    ref = _ref_positions_grad(model, atoms, batch, frames, targets, w)
    err = _rel(got, ref)
    print(f"positions grad G={G} cutoff={cutoff}: max rel err {err:.2e}")
    assert err <= 1e-4, err
    _check_invariance(frames, got)


@pytest.mark.gpu
def test_shift_restraint_forces_equal_autograd_bitwise():
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.library import shift_restraint
    atoms, pos0 = _structure()
    n = pos0.shape[0]
    rng = np.random.default_rng(8)
    model = _model()
    model.build(atoms.shape[1])
    targets = rng.standard_normal(n).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    energy, forces = shift_restraint(model, atoms, pos0, targets, w)
    pos = torch.tensor(pos0, device=_dev(), requires_grad=True)
    peaks = model(frames_to_batch(atoms, pos))
    y, wt = torch.from_numpy(targets).to(_dev()), torch.from_numpy(w).to(_dev())
    loss = ((peaks - y) ** 2 * wt).sum()
    loss.backward()
    assert forces.shape == (n, 3) and forces.is_cuda
    assert torch.equal(pos.grad, -forces)
    assert abs(float(energy) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))
    _check_invariance(pos0[None], forces.cpu().numpy()[None])
    e2, f2 = shift_restraint(model, atoms, pos0, targets, w)         # determinism
    assert torch.equal(forces, f2) and torch.equal(energy, e2)


@pytest.mark.gpu
def test_watched_edges_tuple_and_determinism():
    """model((atoms, nlist, edges, inv)) with edges.requires_grad_(): edges.grad against float64; twice the same bits"""
    b = small_batch(1, 80, 16, 10, seed=12, p_pad=0.1)
    model = _model(seed=6)
    model.build(10)
    dpk = torch.from_numpy(np.random.default_rng(2).standard_normal(b["atoms"].shape[0]).astype(np.float32)).to(_dev())
    grads = []
    for _ in range(2):
        edges = torch.tensor(b["edges"], device=_dev(), requires_grad=True)
        peaks = model((torch.from_numpy(b["atoms"]).to(_dev()), torch.from_numpy(b["nlist"]).to(_dev()), edges,
                       torch.from_numpy(b["inv_degree"]).to(_dev())))
        (peaks * dpk).sum().backward()
        grads.append(edges.grad.clone())
    assert torch.equal(grads[0], grads[1])
    from oracle import torch_ref
    d = torch.tensor(np.asarray(b["edges"], np.float64), requires_grad=True)
    C_ = 10
    ref = torch_ref.forward((b["atoms"], b["nlist"], d, b["inv_degree"]), torch_ref.to_torch_params(model.get_weights()),
                            hp_to_oracle(model.hypers), peak_std=model.peak_std[:C_], peak_avg=model.peak_avg[:C_])
    (ref * dpk.cpu().double()).sum().backward()
    assert _rel(grads[0].cpu().numpy(), d.grad.numpy()) <= 1e-4


@pytest.mark.gpu
def test_no_input_grad_takes_the_parameter_path_unchanged():
    """nothing but the parameters requires grad: GNNModelFunction as before; with edges requiring grad too the peaks and
    the parameter gradient are the same bits"""
    from nmrgnn_amd.autograd import GNNModelFunction
    from nmrgnn_amd.graph import GraphBatch
    b = small_batch(2, 70, 16, 10, seed=21, p_pad=0.1)
    model = _model(seed=9)
    model.build(10)
    (leaf,) = model.parameters()
    dpk = torch.from_numpy(np.random.default_rng(3).standard_normal(b["atoms"].shape[0]).astype(np.float32)).to(_dev())
    out = []
    for watch in (False, True):
        gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=_dev())
        if watch:
            gb.edges.requires_grad_()
        leaf.grad = None
        peaks = model(gb)
        if not watch:
            assert type(peaks.grad_fn).__name__ == GNNModelFunction.__name__ + "Backward"
        (peaks * dpk).sum().backward()
        out.append((peaks.detach().clone(), leaf.grad.clone()))
        if watch:
            assert gb.edges.grad is not None
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    with torch.no_grad():
        gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=_dev())
        gb.edges.requires_grad_()
        assert model(gb).grad_fn is None
