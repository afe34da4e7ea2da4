"""Shift uncertainties on the GPU: the head with the closed-form dropout variance (ng_head_fwd_var), the moments over replicas
(ng_ensemble_moments), Engine.forward_moments, GraphBatch.replicate, GNNModel.predict_uncertainty,
library.shift_uncertainty(position_sigma=) and the eval-struct options, against tests/uncertainty_ref.py (float64) and the float64
oracle.

    var_i = (1 - keep) / keep sum_f (g_if u_if)^2        |var - ref| <= gamma V-bar,  gamma = 2 (Fh + C + 4) 2^-24
    (V-bar: the same sum with |.| inside u; gamma counts C roundings in u, doubled by the square, the product and the square
    roundings and Fh additions)

peaks of ng_head_fwd_var are the bits of ng_head_fwd(drop_mask = NULL).  Every output is pre-filled with NaN, so an entry left
unwritten fails.  Shifts are compared with the oracle at unit standardisation (tests/test_gpu_parity.py: PEAK_ATOL = 1e-4)."""
import csv
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import uncertainty_ref as U
from helpers import hp_to_oracle, make_hp, oracle_batch_forward_backward, randomize_biases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PDB1 = os.path.join(HERE, "data", "108M.pdb")
PATHS = [("default", {}), ("generic", {"NG_HEAD_PATH": "generic"})]


def use(monkeypatch, env):
    if "NG_HEAD_PATH" in env:
        monkeypatch.setenv("NG_HEAD_PATH", env["NG_HEAD_PATH"])
    else:
        monkeypatch.delenv("NG_HEAD_PATH", raising=False)


class Gpu:
    def __init__(self, dev):
        import torch
        from nmrgnn_amd import _lib
        self.torch, self.dev = torch, dev
        self.ctx = _lib.get_context(dev.index)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.cu = int(torch.cuda.get_device_properties(dev).multi_processor_count)

    def up(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)

    def nan(self, *shape):
        return self.torch.full(shape, float("nan"), device=self.dev)

    def head_var(self, N, Fh, Cn, keep, d, peaks="new", var="new"):
        """rc, peaks, var of ng_head_fwd_var on device data d = (g, W, b, atoms, std, avg)"""
        from nmrgnn_amd._lib import ptr
        pk = self.nan(max(N, 1)) if isinstance(peaks, str) else peaks
        vr = self.nan(max(N, 1)) if isinstance(var, str) else var
        g, W, b, atoms, std, avg = d
        rc = self.lib.ng_head_fwd_var(self.h, self.st, N, Fh, Cn, ptr(g), keep, ptr(W), ptr(b), ptr(atoms), ptr(std), ptr(avg),
                                      ptr(pk), ptr(vr))
        return rc, pk, vr

    def head(self, N, Fh, Cn, d):
        from nmrgnn_amd._lib import ptr
        pk = self.nan(max(N, 1))
        g, W, b, atoms, std, avg = d
        self.ctx.check(self.lib.ng_head_fwd(self.h, self.st, N, Fh, Cn, ptr(g), None, ptr(W), ptr(b), ptr(atoms), ptr(std),
                                            ptr(avg), ptr(pk)), "ng_head_fwd")
        return pk

    def moments(self, S, N, mu, v, mean="new", var_in="new", var_model="new"):
        from nmrgnn_amd._lib import ptr
        mean = self.nan(max(N, 1)) if isinstance(mean, str) else mean
        var_in = self.nan(max(N, 1)) if isinstance(var_in, str) else var_in
        var_model = self.nan(max(N, 1)) if isinstance(var_model, str) else var_model
        rc = self.lib.ng_ensemble_moments(self.h, self.st, S, N, ptr(mu), ptr(v), ptr(mean), ptr(var_in), ptr(var_model))
        return rc, mean, var_in, var_model


# ------------------------------------------------------------------------------------------------- 1. ng_head_fwd_var
def _head_rows(Fh, cu):
    """row counts on the launch geometry: R = 256 / (Fh / 4) rows per workgroup of the fast form, one row past the block of
    the one-thread-per-row form, and for the fast shapes one row past the grid cap (num_cu * 8 workgroups): a second
    grid-stride pass"""
    R = 256 // (Fh // 4)
    rows = [1, R - 1, R, R + 1, 257]
    if Fh in (32, 64, 128):
        rows.append(cu * 8 * R + 1)
    return rows


@pytest.mark.parametrize("Fh", [16, 32, 64, 128])
@pytest.mark.parametrize("path,env", PATHS, ids=[p[0] for p in PATHS])
def test_head_fwd_var(gpu_device, monkeypatch, path, env, Fh):
    import torch
    use(monkeypatch, env)
    G = Gpu(gpu_device)
    worst = 0.0
    for Cn in (1, 5, 16, 17, 32):
        for N in _head_rows(Fh, G.cu):
            for onehot in (True, False):
                rng = np.random.default_rng([Fh, Cn, N, int(onehot)])
                host = U.head_data(rng, N, Fh, Cn, onehot=onehot, zero_row=None if onehot else min(3, N - 1))
                d = tuple(G.up(x) for x in host)
                pk0 = G.head(N, Fh, Cn, d)
                _, base, vbar1 = U.head_var_ref(host[0], 0.5, *host[1:])          # keep = 1/2: the bare sums, (1 - keep) / keep = 1
                for keep in (0.8, 0.5, 1.0):
                    rc, pk, vr = G.head_var(N, Fh, Cn, keep, d)
                    G.ctx.check(rc, "ng_head_fwd_var")
                    assert torch.equal(pk, pk0), (Cn, N, onehot, keep)
                    k32 = float(np.float32(keep))
                    ref, vbar = (1.0 - k32) / k32 * base, (1.0 - k32) / k32 * vbar1
                    got = vr.cpu().numpy().astype(np.float64)
                    if keep == 1.0:
                        assert (got == 0).all(), (Cn, N, onehot)
                        continue
                    bound = U.gamma(Fh, Cn) * vbar
                    err = np.abs(got - ref)
                    assert (err <= bound).all(), (Cn, N, onehot, keep, float((err / np.maximum(bound, 1e-300)).max()))
                    if (vbar > 0).any():
                        worst = max(worst, float((err[vbar > 0] / bound[vbar > 0]).max()))
                    if not onehot:
                        assert got[min(3, N - 1)] == 0.0              # an all-zero atoms row
                    if keep == 0.8 and N == 257:                      # the same bits on a second call
                        rc, pk2, vr2 = G.head_var(N, Fh, Cn, keep, d)
                        assert rc == 0 and torch.equal(pk2, pk) and torch.equal(vr2, vr)
    print(f"{path} Fh={Fh}: largest |var - ref| / (gamma V-bar) = {worst:.3f}")


@pytest.mark.parametrize("path,env", PATHS, ids=[p[0] for p in PATHS])
def test_head_fwd_var_refusals(gpu_device, monkeypatch, path, env):
    import torch
    use(monkeypatch, env)
    G = Gpu(gpu_device)
    N, Fh = 9, 32
    host = U.head_data(np.random.default_rng(1), N, Fh, 32)
    d = tuple(G.up(x) for x in host)
    for Cn, keep in ((0, 0.8), (33, 0.8), (10, 0.0), (10, -0.5), (10, 1.5), (10, float("nan"))):
        rc, pk, vr = G.head_var(N, Fh, Cn, keep, d)
        assert rc != 0 and bool(torch.isnan(pk).all()) and bool(torch.isnan(vr).all()), (Cn, keep)
    rc, _, vr = G.head_var(N, Fh, 10, 0.8, d, peaks=None)
    assert rc != 0 and bool(torch.isnan(vr).all())
    rc, pk, _ = G.head_var(N, Fh, 10, 0.8, d, var=None)
    assert rc != 0 and bool(torch.isnan(pk).all())
    rc, pk, vr = G.head_var(0, Fh, 10, 0.8, d)                        # no rows: nothing is written
    assert rc == 0 and bool(torch.isnan(pk).all()) and bool(torch.isnan(vr).all())


# ------------------------------------------------------------------------------------------------- 2. ng_ensemble_moments
@pytest.mark.parametrize("kind", ["normal", "nitrogen", "constant"])
def test_ensemble_moments(gpu_device, kind):
    import torch
    G = Gpu(gpu_device)
    for S in (1, 2, 3, 32, 257):
        for N in (1, 255, 256, 257, 70001):
            mu_h, v_h = U.moments_data(np.random.default_rng([S, N, len(kind)]), kind, S, N)
            mu, v = G.up(mu_h), G.up(v_h)
            rc, mean, vi, vm = G.moments(S, N, mu, v)
            G.ctx.check(rc, "ng_ensemble_moments")
            rmean, rvar, rvm = U.ensemble_moments_ref(mu_h, v_h)
            mean_h, vi_h, vm_h = (t.cpu().numpy().astype(np.float64) for t in (mean, vi, vm))
            assert (np.abs(mean_h - rmean) <= U.ulp32(rmean)).all(), (S, N)
            assert (np.abs(vi_h - rvar) <= 2.0 ** -22 * rvar).all(), (S, N)
            assert (np.abs(vm_h - rvm) <= 2.0 ** -22 * rvm).all(), (S, N)
            if kind == "constant" or S == 1:
                assert (vi_h == 0).all() and np.array_equal(mean.cpu().numpy(), mu_h[0]), (S, N)
            # the form without variances: the same mean and var_input, var_model untouched
            rc, mean2, vi2, vm2 = G.moments(S, N, mu, None, var_model=None)
            assert rc == 0 and vm2 is None and torch.equal(mean2, mean) and torch.equal(vi2, vi), (S, N)
            if (S, N) == (32, 257):                                   # the same bits on a second call
                rc, mean3, vi3, vm3 = G.moments(S, N, mu, v)
                assert rc == 0 and torch.equal(mean3, mean) and torch.equal(vi3, vi) and torch.equal(vm3, vm)


def test_ensemble_moments_refusals(gpu_device):
    import torch
    G = Gpu(gpu_device)
    S, N = 3, 9
    mu, v = (G.up(x) for x in U.moments_data(np.random.default_rng(2), "normal", S, N))
    untouched = lambda *ts: all(t is None or bool(torch.isnan(t).all()) for t in ts)
    rc, mean, vi, vm = G.moments(0, N, mu, v)
    assert rc != 0 and untouched(mean, vi, vm)
    rc, mean, vi, vm = G.moments(S, N, None, v)
    assert rc != 0 and untouched(mean, vi, vm)
    rc, mean, vi, vm = G.moments(S, N, mu, v, mean=None)
    assert rc != 0 and untouched(vi, vm)
    rc, mean, vi, vm = G.moments(S, N, mu, v, var_in=None)
    assert rc != 0 and untouched(mean, vm)
    rc, mean, vi, vm = G.moments(S, N, mu, v, var_model=None)         # v without var_model
    assert rc != 0 and untouched(mean, vi)
    rc, mean, vi, vm = G.moments(S, N, mu, None)                      # var_model without v
    assert rc != 0 and untouched(mean, vi, vm)


# ------------------------------------------------------------------------------------------------- 3. Engine.forward_moments
CFG = {"F64": dict(atom_feature_size=64, edge_feature_size=3, edge_hidden_size=128),
       "F32": dict(atom_feature_size=32, edge_feature_size=2, edge_hidden_size=32, mp_layers=2, fc_layers=3, edge_fc_layers=3)}


def _var_check(eng, gb_atoms, g, var, std, avg):
    sd = eng.params.state_dict()
    Fh, Cn = sd["out/kernel"].shape
    keep = 0.8 if eng.use_dropout else 1.0
    _, ref, vbar = U.head_var_ref(g.cpu().numpy(), keep, sd["out/kernel"], sd["out/bias"], gb_atoms, std, avg)
    err = np.abs(var.cpu().numpy().astype(np.float64) - ref)
    assert (err <= U.gamma(Fh, Cn) * vbar).all(), float((err / np.maximum(U.gamma(Fh, Cn) * vbar, 1e-300)).max())
    assert (ref > 0).any()


@pytest.mark.parametrize("table", ["1", "0"], ids=["edge-default", "edge-table-off"])
@pytest.mark.parametrize("name", list(CFG))
def test_forward_moments(gpu_device, monkeypatch, name, table):
    import torch
    import test_gpu_parity as TP
    if table == "0":
        monkeypatch.setenv("NG_EDGE_TABLE", "0")
    else:
        monkeypatch.delenv("NG_EDGE_TABLE", raising=False)
    hp, b, eng, sd, gb, std, avg = TP._setup(gpu_device, CFG[name])
    assert eng.use_dropout and eng.sigma > 0
    N, ne, Fh = gb.N, gb.n_edges, hp.get('atom_feature_size') // 2
    ones = torch.ones(N * Fh, device=gpu_device)
    seed = 5
    xi = eng.randn(ne, seed, 0)
    ref = eng.forward(gb, training=True, noise=xi, dropout_mask=ones).clone()
    tape = eng.tape
    g = tape.g.clone()
    mu, var = eng.forward_moments(gb, seed=seed)
    assert eng.tape is tape and torch.equal(tape.g, g)                # the tape is left as it was
    assert torch.equal(mu, ref)
    _var_check(eng, b["atoms"], g, var, std, avg)
    # an explicit noise tensor is the same call
    mu_x, var_x = eng.forward_moments(gb, seed=seed + 1, noise=xi)
    assert torch.equal(mu_x, mu) and torch.equal(var_x, var)
    # without noise: the call with xi = 0
    ref0 = eng.forward(gb, training=True, noise=torch.zeros_like(xi), dropout_mask=ones).clone()
    g0 = eng.tape.g.clone()
    held = eng.tape
    mu0, var0 = eng.forward_moments(gb, seed=seed, noise=False)
    assert eng.tape is held and torch.equal(mu0, ref0) and not torch.equal(mu0, mu)
    _var_check(eng, b["atoms"], g0, var0, std, avg)
    # a model without dropout: the variance is exactly 0, the shifts those of its training-mode call
    hp2, b2, eng2, sd2, gb2, std2, avg2 = TP._setup(gpu_device, dict(CFG[name], dropout=False))
    assert not eng2.use_dropout
    want = eng2.forward(gb2, training=True, noise=xi).clone()
    mu2, var2 = eng2.forward_moments(gb2, seed=seed)
    assert torch.equal(mu2, want) and bool((var2 == 0).all())


def test_forward_moments_and_ensemble_moments_under_capture(gpu_device):
    """the whole chain — noise draw, trunk, ng_head_fwd_var, ng_ensemble_moments — recorded once as a HIP graph: a replay
    writes the bits of the eager calls (the seed is frozen into the recorded nodes)"""
    import torch
    import test_gpu_parity as TP
    hp, b, eng, sd, gb, std, avg = TP._setup(gpu_device, CFG["F64"])
    S, N = 3, gb.N
    rep = gb.replicate(S)

    def chain():
        mu, var = eng.forward_moments(rep, seed=9)
        return (mu, var) + eng.ensemble_moments(mu.view(S, N), var.view(S, N))
    eager = [t.clone() for t in chain()]
    cur = torch.cuda.current_stream(gpu_device)
    side, graph = torch.cuda.Stream(device=gpu_device), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        chain()
        torch.cuda.synchronize(gpu_device)
        with torch.cuda.graph(graph, stream=side):
            outs = chain()
    cur.wait_stream(side)
    for t in outs:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize(gpu_device)
    assert all(torch.equal(x, y) for x, y in zip(outs, eager))


# ------------------------------------------------------------------------------------------------- 4. GraphBatch.replicate
@pytest.mark.parametrize("name", list(CFG))
def test_replicate(gpu_device, name):
    import torch
    import test_gpu_parity as TP
    from oracle import nmrgnn_oracle as O
    hp, b, eng, sd, gb, std, avg = TP._setup(gpu_device, CFG[name])
    N, S = gb.N, 3
    r = U.replicate_ref(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], b["graph_ptr"], S)
    rep = gb.replicate(S)
    assert (rep.N, rep.K, rep.G, rep.is_csr) == (S * N, gb.K, S * gb.G, False)
    assert np.array_equal(rep.nlist.cpu().numpy(), r["nlist"]) and np.array_equal(rep.edges.cpu().numpy(), r["edges"])
    assert np.array_equal(rep.atoms.cpu().numpy(), r["atoms"]) and np.array_equal(rep.inv_degree.cpu().numpy(), r["inv"])
    assert np.array_equal(rep.graph_ptr_host, r["graph_ptr"]) and np.array_equal(rep.graph_ptr.cpu().numpy(), r["graph_ptr"])
    # the compute-side lists: a padded slot points at its own atom, inside its replica
    own = np.arange(S * N)[:, None]
    assert np.array_equal(rep.nlist_c.cpu().numpy(), np.where(r["edges"] > 0, r["nlist"], own))
    # CSR form
    csr = gb.to_csr()
    rc = U.replicate_ref(b["atoms"], csr.nlist.cpu().numpy(), csr.edges.cpu().numpy(), b["inv_degree"], b["graph_ptr"], S,
                         row_ptr=csr.row_ptr.cpu().numpy())
    crep = csr.replicate(S)
    assert crep.is_csr and crep.N == S * N and crep.nnz == S * csr.nnz
    assert np.array_equal(crep.row_ptr.cpu().numpy(), rc["row_ptr"]) and np.array_equal(crep.nlist.cpu().numpy(), rc["nlist"])
    assert np.array_equal(crep.edges.cpu().numpy(), rc["edges"]) and np.array_equal(crep.graph_ptr_host, rc["graph_ptr"])
    assert np.array_equal(crep.row_of.cpu().numpy(), np.repeat(np.arange(S * N), np.diff(rc["row_ptr"])))
    # one replica is the batch
    peaks = eng.forward(gb)
    assert torch.equal(eng.forward(gb.replicate(1)), peaks)
    assert torch.equal(eng.forward(csr.replicate(1)), eng.forward(csr))
    # every replica's shifts against the float64 oracle of the single batch
    ref = O.gnn_forward((b["atoms"], b["nlist"], b["edges"], b["inv_degree"]), sd, hp_to_oracle(hp), std, avg)
    for form in (rep, crep):
        got = eng.forward(form).cpu().numpy().reshape(S, N)
        assert np.max(np.abs(got - ref[None])) < TP.PEAK_ATOL
    with pytest.raises(ValueError):
        gb.replicate(0)


# ------------------------------------------------------------------------------------------------- 5. predict_uncertainty
def _model_108m(gpu_device, **hp_kw):
    """a GNNModel at unit standardisation (no peak standards: std 1, avg 0) on the 108M structure"""
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(PDB1)
    atoms = atoms_onehot(s.elements)
    model = GNNModel(make_hp(atom_feature_size=64, **hp_kw), {}, device=gpu_device, seed=5)
    model.build(atoms.shape[1])
    sd = randomize_biases(model.engine)
    batch = frames_to_batch(atoms, s.frames[0], 16, device=gpu_device)
    return model, sd, atoms, s, batch


def test_predict_uncertainty(gpu_device):
    import torch
    import test_gpu_parity as TP
    model, sd, atoms, s, batch = _model_108m(gpu_device)
    eng = model.engine
    N, K, S, seed = batch.N, batch.K, 8, 11
    mean, std_model, std_input = model.predict_uncertainty(batch, samples=S, seed=seed)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == (N,) for t in (mean, std_model, std_input))
    rep = batch.replicate(S)
    mu, var = eng.forward_moments(rep, seed=seed)
    m, vi, vm = eng.ensemble_moments(mu.view(S, N), var.view(S, N))
    assert torch.equal(mean, m) and torch.equal(std_model, torch.sqrt(vm)) and torch.equal(std_input, torch.sqrt(vi))
    assert bool((std_model > 0).all()) and bool((std_input > 0).any())
    # every replica against the float64 oracle fed its slice of the noise.  The oracle scales a kept unit by 1 / keep, the
    # engine's mask holds that factor itself: the engine's all-ones mask is the oracle's mask of `keep`
    xi = eng.randn(S * N * K, seed, 0).cpu().numpy().reshape(S * N, K)
    r = U.replicate_ref(atoms, batch.nlist.cpu().numpy(), batch.edges.cpu().numpy(), batch.inv_degree.cpu().numpy(), [0, N], S)
    b = dict(atoms=r["atoms"], nlist=r["nlist"], edges=r["edges"], inv_degree=r["inv"], graph_ptr=r["graph_ptr"])
    Fh = model.hypers.get('atom_feature_size') // 2
    ref, _ = oracle_batch_forward_backward(b, sd, hp_to_oracle(model.hypers), np.zeros(S * N, np.float32),
                                           np.ones(atoms.shape[1]), np.zeros(atoms.shape[1]), xi=xi,
                                           mask=np.full((S * N, Fh), 1.0 - 0.2))
    assert np.max(np.abs(mu.cpu().numpy() - ref)) < TP.PEAK_ATOL
    # chunked: 1 chunk and 3 chunks (3 + 3 + 2 replicas) of the same draw
    one = model.predict_uncertainty(batch, samples=S, seed=seed, chunk_atoms=S * N)
    three = model.predict_uncertainty(batch, samples=S, seed=seed, chunk_atoms=3 * N + 5)
    assert all(torch.equal(a, c) for a, c in zip(one, (mean, std_model, std_input)))
    for a, c in zip(one, three):
        assert float((a - c).abs().max()) <= 2 * TP.PEAK_ATOL
    # host inputs give NumPy
    host = model.predict_uncertainty((atoms, batch.nlist.cpu().numpy(), batch.edges.cpu().numpy(),
                                      batch.inv_degree.cpu().numpy()), samples=2, seed=seed)
    assert all(isinstance(t, np.ndarray) and t.shape == (N,) for t in host)
    # seed=None draws like a training-mode call: the call counter moves
    calls = model._train_calls
    model.predict_uncertainty(batch, samples=2)
    assert model._train_calls == calls + 1


def test_predict_uncertainty_special_cases(gpu_device):
    import torch
    model, sd, atoms, s, batch = _model_108m(gpu_device, noise=0.0)
    mean, std_model, std_input = model.predict_uncertainty(batch, samples=8, seed=3)
    assert bool((std_input == 0).all()) and bool((std_model > 0).all())
    assert torch.equal(mean, model.engine.forward_moments(batch, seed=3)[0])        # one replica
    model, sd, atoms, s, batch = _model_108m(gpu_device, dropout=False)
    mean, std_model, std_input = model.predict_uncertainty(batch, samples=4, seed=3)
    assert bool((std_model == 0).all()) and bool((std_input > 0).any())


# ------------------------------------------------------------------------------------------------- 6. shift_uncertainty
def test_shift_uncertainty_position_sigma(gpu_device):
    import torch
    from nmrgnn_amd.library import shift_uncertainty
    model, sd, atoms, s, batch = _model_108m(gpu_device)
    pos, n = s.frames[0], atoms.shape[0]
    mean, std_model, std_input = shift_uncertainty(model, atoms, pos, samples=4, position_sigma=0.0, seed=2)
    one = shift_uncertainty(model, atoms, pos, samples=1, position_sigma=0.0, seed=2)
    assert bool((std_input == 0).all()) and torch.equal(mean, one[0]) and bool((one[2] == 0).all())
    sigma = np.where(np.arange(n) % 2 == 0, 0.0, 0.3)
    out = shift_uncertainty(model, atoms, pos, samples=4, position_sigma=sigma, seed=2)
    for t in out:
        assert tuple(t.shape) == (n,) and bool(torch.isfinite(t).all())
    assert bool((out[1] >= 0).all()) and bool((out[2] >= 0).all()) and bool((out[2] > 0).any())
    # without position_sigma: predict_uncertainty on the structure's batch
    a = shift_uncertainty(model, atoms, pos, samples=4, seed=2)
    c = model.predict_uncertainty(batch, samples=4, seed=2)
    assert all(torch.equal(x, y) for x, y in zip(a, c))


# ------------------------------------------------------------------------------------------------- 7. eval-struct
def _write_pdb(path, s, frame):
    lines = ["MODEL        1\n"]
    for k in range(s.n_atoms):
        nm = s.names[k] if len(s.names[k]) == 4 else " " + s.names[k]
        lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s\n"
                     % (k + 1, nm, s.resnames[k], s.resids[k], frame[k, 0], frame[k, 1], frame[k, 2], s.elements[k]))
    lines.append("ENDMDL\n")
    path.write_text("".join(lines))


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_eval_struct_uncertainty_and_average(gpu_device, tmp_path):
    import io
    import nmrgnn_amd
    from click.testing import CliRunner
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.library import check_peaks
    from nmrgnn_amd.main import eval_structure, main
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    quiet = dict(keep_going=True, echo=lambda *a: None)
    s = read_pdb(PDB1)
    n = s.n_atoms
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        # the default CSV: through the function, through the command line, and rebuilt here as it was always written
        eval_structure((PDB1,), str(tmp_path / "plain.csv"), **quiet)
        res = CliRunner().invoke(main, ["eval-struct", "--keep-going", PDB1, str(tmp_path / "cli.csv")])
        assert res.exit_code == 0, res.output
        model = nmrgnn_amd.load_model()
        atoms = atoms_onehot(s.elements)
        model.build(atoms.shape[1])
        peaks = model(frames_to_batch(atoms, s.frames[0][None], 16, device=model.engine.device)).cpu().numpy()
        try:
            conf = check_peaks(atoms, peaks)
        except Warning:
            conf = np.zeros(n, dtype=bool)
        pk = np.round(peaks.astype(np.float64), 2)
        buf = io.StringIO(newline="")
        wr = csv.writer(buf)
        wr.writerow(['index', 'residues', 'resids', 'names', 'peaks', 'confident', 'time', 'frame'])
        wr.writerows([(i, s.resnames[i], int(s.resids[i]), s.names[i], pk[i], bool(conf[i]), 0.0, 0) for i in range(n)])
        plain = (tmp_path / "plain.csv").read_bytes()
        assert plain == (tmp_path / "cli.csv").read_bytes() == buf.getvalue().encode()
        # --uncertainty 4: exactly two more columns, the others as before
        res = CliRunner().invoke(main, ["eval-struct", "--keep-going", "--uncertainty", "4", PDB1, str(tmp_path / "unc.csv")])
        assert res.exit_code == 0, res.output
        base, unc = _rows(tmp_path / "plain.csv"), _rows(tmp_path / "unc.csv")
        assert unc[0] == base[0] + ['std_model', 'std_input'] and len(unc) == len(base) == n + 1
        assert [r[:8] for r in unc] == [r for r in base]
        vals = np.array([[float(r[8]), float(r[9])] for r in unc[1:]])
        assert np.isfinite(vals).all() and (vals >= 0).all() and (vals[:, 0] > 0).any() and (vals[:, 1] > 0).any()
        eval_structure((PDB1,), str(tmp_path / "sig.csv"), uncertainty=4, position_sigma=0.2, **quiet)
        sig = _rows(tmp_path / "sig.csv")
        assert sig[0] == unc[0] and [r[:8] for r in sig] == base
        # --average over two frames (the structure and a displaced copy, read as one trajectory)
        rng = np.random.default_rng(4)
        second = tmp_path / "second.pdb"
        _write_pdb(second, s, np.round(s.frames[0] + 0.2 * rng.standard_normal((n, 3)), 3))
        files = (PDB1, str(second))
        eval_structure(files, str(tmp_path / "frames.csv"), **quiet)
        eval_structure(files, str(tmp_path / "avg.csv"), average=True, **quiet)
    fr, avg = _rows(tmp_path / "frames.csv"), _rows(tmp_path / "avg.csv")
    assert avg[0] == ['index', 'residues', 'resids', 'names', 'peaks', 'peaks_std', 'confident', 'frames']
    assert len(fr) == 2 * n + 1 and len(avg) == n + 1
    assert [r[:4] for r in avg[1:]] == [r[:4] for r in fr[1:n + 1]] and all(r[7] == '2' for r in avg[1:])
    per = np.array([float(r[4]) for r in fr[1:]]).reshape(2, n)
    got_mean, got_std = np.array([float(r[4]) for r in avg[1:]]), np.array([float(r[5]) for r in avg[1:]])
    # the per-frame CSV holds shifts rounded to 0.01: each is within 0.005 of the shift the moments were taken of, so their
    # float64 mean is within 0.005 and their sample standard deviation |a - b| / sqrt(2) within 0.01 / sqrt(2) of the
    # unrounded ones; the averaged CSV rounds once more (0.005), and float32 adds 1e-4 at most
    assert np.max(np.abs(got_mean - per.mean(axis=0))) <= 0.005 + 0.005 + 1e-4
    assert np.max(np.abs(got_std - per.std(axis=0, ddof=1))) <= 0.01 / np.sqrt(2.0) + 0.005 + 1e-4
    assert got_std.max() > 0.05
