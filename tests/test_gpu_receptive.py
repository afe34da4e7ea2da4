"""Receptive-field pruning on the GPU (csrc/prune.hip, GraphBatch.restrict, GNNModel.predict_selected,
shift_restraint(prune=True), eval-struct --atom-names): bit for bit against the integer reference tests/receptive_ref.py,
and the model and the restraint on the pruned batch against float64 on the WHOLE graph."""
import csv
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import receptive_ref as R
from helpers import hp_to_oracle, make_hp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PDB = os.path.join(ROOT, "tests", "data", "108M.pdb")
PEAK_ATOL = 1e-4          # the constant of tests/test_gpu_parity.py


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


@functools.lru_cache(maxsize=None)
def _lists(N, K, seed=3):
    """one synthetic graph of N atoms (nmrgnn_amd.synth) at p_pad = 0.15"""
    from nmrgnn_amd import synth
    atoms, nl, d = synth.make_graph(N, K, 10, 0.15, np.random.default_rng(seed + 7 * N + K))
    return atoms, nl.astype(np.int32), d, synth.inv_degree(nl)


def _batch(atoms, nlist, edges, inv, graph_ptr=None):
    from nmrgnn_amd.graph import GraphBatch
    return GraphBatch(atoms, nlist, edges, inv, graph_ptr=graph_ptr, device=_dev())


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(t, ref):
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if ref.dtype.kind == "f":
        return np.array_equal(a.astype(np.float32).view(np.int32), ref.astype(np.float32).view(np.int32))
    return np.array_equal(a.astype(np.int64), ref.astype(np.int64))


def _check_padded(p, ref):
    for name in ("keep", "hop", "nlist", "edges", "atoms", "inv_degree"):
        assert _same(getattr(p, name), ref[name]), name
    assert np.array_equal(p.graph_ptr_host, ref["graph_ptr"]) and _same(p.graph_ptr, ref["graph_ptr"])
    assert np.array_equal(p.graph_index, ref["graph_index"])
    assert _same(p._prune[1], ref["hop_full"])


def _check_csr(p, ref):
    assert p.is_csr
    for name in ("keep", "hop", "row_ptr", "nlist", "edges", "row_of", "atoms", "inv_degree"):
        assert _same(getattr(p, name), ref[name]), name
    assert np.array_equal(p.graph_ptr_host, ref["graph_ptr"]) and np.array_equal(p.graph_index, ref["graph_index"])


def _seeds(N, kind):
    s = np.zeros(N, np.int32)
    if kind == "one":
        s[N // 2] = 1
    elif kind == "5pct":
        s[np.random.default_rng(N).choice(N, max(1, N // 20), replace=False)] = 1
    else:
        s[:] = 1
    return s


# ------------------------------------------------------------------------------------------------------- 1. pruned lists
@pytest.mark.parametrize("K", [1, 16, 17, 64])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_pruned_lists_bitwise(N, K):
    atoms, nlist, edges, inv = _lists(N, K)
    gb = _batch(atoms, nlist, edges, inv)
    for kind in ("one", "5pct", "all"):
        seed = _seeds(N, kind)
        for hops in (0, 1, 4, 64):
            ref = R.prune_padded(atoms, nlist, edges, inv, [0, N], seed, hops)
            p = gb.restrict(seed.astype(bool), hops)
            _check_padded(p, ref)
            assert _same(p.selected, ref["idx"][np.nonzero(seed)[0]])
            if kind == "all" and hops > 0:
                # nothing to prune: the parent's own tensors bit for bit.  This leans on two facts of these inputs: synth pads
                # with (0, 0.0), which is also the dead slot of a one-graph batch, and every slot with a distance has a target
                # inside [0, N).  (hops == 0 keeps the atoms and kills every slot.)
                assert _same(p.edges, gb.edges) and _same(p.nlist, gb.nlist) and _same(p.atoms, gb.atoms)
                assert _same(p.inv_degree, gb.inv_degree) and _same(p.keep, np.arange(N))


def test_two_calls_give_identical_bits_and_index_select():
    atoms, nlist, edges, inv = _lists(257, 16)
    gb = _batch(atoms, nlist, edges, inv)
    seed = _seeds(257, "5pct")
    a = gb.restrict(seed.astype(bool), 1)
    b = gb.restrict(torch.from_numpy(np.nonzero(seed)[0][::-1].copy()).to(_dev()), 1)     # indices, unsorted, on the device
    c = gb.restrict(torch.from_numpy(seed.astype(bool)).to(_dev()), 1)                    # a device mask
    for q in (b, c):
        for name in ("keep", "hop", "nlist", "edges", "atoms", "inv_degree", "nlist_c", "selected"):
            assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(q, name))), name
    assert a.positions is None and a.parent is gb


def test_hand_cases():
    for make, seed_at, hops, want in ((R.path_case, 0, 3, [0, 1, 2, 3] + [-1] * 8),
                                      (R.asymmetric_case, 0, 4, [0, 1, -1, -1, -1, -1, -1, -1]),
                                      (R.asymmetric_case, 5, 4, [1, 2, -1, -1, -1, 0, -1, -1]),
                                      (R.padded_row_case, 4, 4, [-1, -1, -1, 1, 0, -1])):
        nlist, edges = make()
        N = nlist.shape[0]
        atoms, inv = R.hand_batch(nlist, edges)
        seed = np.zeros(N, np.int32)
        seed[seed_at] = 1
        gb = _batch(atoms, nlist, edges, inv)
        p = gb.restrict([seed_at], hops)
        assert p._prune[1].cpu().tolist() == want
        _check_padded(p, R.prune_padded(atoms, nlist, edges, inv, [0, N], seed, hops))
        rp, col, dist, _ = R.to_csr(nlist, edges)
        _check_csr(gb.to_csr().restrict([seed_at], hops), R.prune_csr(atoms, rp, col, dist, inv, [0, N], seed, hops))


def test_ragged_graphs_seeds_in_the_last_graph_only():
    from nmrgnn_amd import synth
    rng = np.random.default_rng(12)
    parts = [synth.make_graph(n, 16, 10, 0.15, rng) for n in (1, 17, 64)]
    gp = np.array([0, 1, 18, 82])
    atoms = np.concatenate([p[0] for p in parts])
    nlist = np.concatenate([p[1] + o for p, o in zip(parts, gp[:3])]).astype(np.int32)
    edges = np.concatenate([p[2] for p in parts])
    inv = np.concatenate([synth.inv_degree(p[1]) for p in parts])
    seed = np.zeros(82, np.int32)
    seed[[20, 77]] = 1
    gb = _batch(atoms, nlist, edges, inv, gp)
    for hops in (0, 1, 4):
        p = gb.restrict(seed.astype(bool), hops)
        _check_padded(p, R.prune_padded(atoms, nlist, edges, inv, gp, seed, hops))
        assert p.G == 1 and p.graph_index.tolist() == [2]
        rp, col, dist, _ = R.to_csr(nlist, edges)
        _check_csr(gb.to_csr().restrict(seed.astype(bool), hops), R.prune_csr(atoms, rp, col, dist, inv, gp, seed, hops))


@pytest.mark.parametrize("N,K", [(1, 16), (65, 16), (257, 17), (300, 4), (4097, 16), (4097, 1)])
def test_csr_form_bitwise(N, K):
    atoms, nlist, edges, inv = _lists(N, K)
    rp, col, dist, _ = R.to_csr(nlist, edges)
    gc = _batch(atoms, nlist, edges, inv).to_csr()
    for kind in ("one", "5pct", "all"):
        seed = _seeds(N, kind)
        for hops in (0, 1, 4, 64):
            p = gc.restrict(seed.astype(bool), hops)
            _check_csr(p, R.prune_csr(atoms, rp, col, dist, inv, [0, N], seed, hops))
            if kind == "all" and hops > 0:
                assert _same(p.nlist, col) and _same(p.edges, dist) and _same(p.row_ptr, rp)


def test_python_refusals_come_before_device_work():
    atoms, nlist, edges, inv = _lists(64, 16)
    gb = _batch(atoms, nlist, edges, inv)
    for bad, hops in (([64], 1), ([-1], 1), ([3, 3], 1), (np.zeros(64, bool), 1), (np.ones(63, bool), 1), ([1], -1), ([1], 65),
                      (np.ones((2, 32), bool), 1),
                      (np.ones(64, np.int64), 1)):          # an integer array is a list of indices, here one index 64 times
        with pytest.raises(ValueError):
            gb.restrict(bad, hops)
    with pytest.raises(ValueError):
        gb.restrict(torch.zeros(64, dtype=torch.bool, device=_dev()), 1)      # a device mask: seen in the host synchronisation
    with pytest.raises(ValueError):
        gb.expand(np.zeros(3))


def test_c_refusals_leave_outputs_untouched():
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    ctx = _lib.get_context(0)
    lib, h = ctx.lib, ctx.handle
    N, K = 8, 2
    dev = _dev()
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=dev)
    f32 = lambda n, v: torch.full((n,), v, dtype=torch.float32, device=dev)
    nl, ed, seed, hop, idx = i32(N * K, 1), f32(N * K, 0.1), i32(N, 1), i32(N, 77), i32(N + 1, 0)
    rp, ro = torch.arange(0, N * K + 1, K, dtype=torch.int32, device=dev), i32(N * K, 0)
    outs_i = [i32(N * K, 77) for _ in range(4)]
    outs_f = [f32(N * K, 77.0) for _ in range(4)]
    st = None
    BIG = 1 << 26

    def hops_call(ctx_h=h, N_=N, K_=K, ne=N * K, nlist=nl, hops=1):
        return lib.ng_receptive_hops(ctx_h, st, N_, K_, ne, ptr(rp), ptr(ro), ptr(nlist) if nlist is not None else None, ptr(ed),
                                     ptr(seed), hops, ptr(hop))

    def lists_call(ctx_h=h, N_=N, K_=K, hops=1, nlist=nl):
        return lib.ng_prune_lists(ctx_h, st, N_, K_, 4, 1, hops, ptr(rp), ptr(nlist) if nlist is not None else None, ptr(ed),
                                  ptr(outs_f[3]), ptr(ed), ptr(hop), ptr(idx), ptr(outs_i[0]), ptr(outs_i[1]), ptr(outs_f[0]),
                                  ptr(outs_f[1]), ptr(outs_i[2]), ptr(outs_f[2]))

    def csr_call(ctx_h=h, ne=N * K, hops=1, col=nl):
        return lib.ng_prune_lists_csr(ctx_h, st, N, ne, 4, hops, ptr(rp), ptr(ro), ptr(col) if col is not None else None, ptr(ed),
                                      ptr(outs_f[3]), ptr(ed), ptr(hop), ptr(idx), ptr(rp), ptr(outs_i[0]), ptr(outs_i[1]),
                                      ptr(outs_f[0]), ptr(outs_f[1]), ptr(outs_i[3]), ptr(outs_i[2]), ptr(outs_f[2]), ptr(outs_i[2]))

    def de_call(ctx_h=h, N_=N, K_=K, ne=N * K, hops=1, nlist=nl):
        return lib.ng_prune_expand_edge_grad(ctx_h, st, N_, K_, ne, hops, ptr(rp), ptr(ro), ptr(nlist) if nlist is not None else None,
                                             ptr(ed), ptr(hop), ptr(idx), ptr(rp), ptr(ed), ptr(outs_f[2]))

    cases = [(hops_call, dict(hops=-1), "hops in [0, 64]"), (hops_call, dict(hops=65), "hops in [0, 64]"),
             (hops_call, dict(K_=65, ne=N * 65), "K in [0, 64]"), (hops_call, dict(N_=BIG, K_=32, ne=BIG * 32), "2^31"),
             (hops_call, dict(nlist=None), "nlist required"),
             (lists_call, dict(hops=65), "hops in [0, 64]"), (lists_call, dict(K_=65), "K in [0, 64]"),
             (lists_call, dict(N_=BIG, K_=32), "2^31"), (lists_call, dict(nlist=None), "inputs"),
             (csr_call, dict(hops=-1), "hops in [0, 64]"), (csr_call, dict(ne=1 << 31), "2^31"), (csr_call, dict(col=None), "lists"),
             (de_call, dict(hops=65), "hops in [0, 64]"), (de_call, dict(K_=65, ne=N * 65), "K in [0, 64]"),
             (de_call, dict(N_=BIG, K_=32, ne=BIG * 32), "2^31"), (de_call, dict(nlist=None), "arguments")]
    for fn, kw, text in cases:
        rc = fn(**kw)
        msg = lib.ng_last_error(h).decode()
        assert rc == -1 and text in msg, (fn.__name__, kw, rc, msg)
    for fn in (hops_call, lists_call, csr_call, de_call):
        assert fn(ctx_h=None) == -1                  # NULL context: NG_ERR_INVALID, no message to leave
    assert lib.ng_prune_expand_rows(None, st, N, N, ptr(hop), ptr(ed), 0.0, ptr(outs_f[0])) == -1
    assert lib.ng_prune_expand_rows(h, st, N, N + 1, ptr(hop), ptr(ed), 0.0, ptr(outs_f[0])) == -1
    torch.cuda.synchronize()
    assert (hop == 77).all() and all((t == 77).all() for t in outs_i) and all((t == 77.0).all() for t in outs_f)
    # N == 0 and "no seed" are legal
    assert hops_call(N_=0, ne=0) == 0
    seed.zero_()
    assert hops_call() == 0 and (hop == -1).all()


# ----------------------------------------------------------------------------------------------- 2. expanded edge gradient
@pytest.mark.parametrize("N,K,hops", [(65, 16, 1), (257, 17, 1), (300, 4, 4), (4097, 16, 1)])
def test_expanded_edge_gradient_bitwise(N, K, hops):
    atoms, nlist, edges, inv = _lists(N, K)
    gb = _batch(atoms, nlist, edges, inv)
    seed = _seeds(N, "5pct")
    rng = np.random.default_rng(N)
    p = gb.restrict(seed.astype(bool), hops)
    ref = R.prune_padded(atoms, nlist, edges, inv, [0, N], seed, hops)
    de_p = rng.standard_normal(ref["edges"].shape).astype(np.float32)
    de_p[0, 0] = -0.0
    got = p.expand_edge_grad(torch.from_numpy(de_p).to(_dev()))
    want = R.expand_edge_grad_padded(ref, nlist, edges, de_p)
    assert got.shape == gb.edges.shape and _same(got, want)
    dropped = np.ones((N, K), bool)
    dropped[ref["keep"][ref["hop"] < hops]] = ~R.live_mask(nlist, edges, N)[ref["keep"][ref["hop"] < hops]]
    assert (_bits(got)[dropped] == 0).all()                          # +0.0, not -0.0, where nothing was kept
    rp, col, dist, _ = R.to_csr(nlist, edges)
    pc = gb.to_csr().restrict(seed.astype(bool), hops)
    refc = R.prune_csr(atoms, rp, col, dist, inv, [0, N], seed, hops)
    de_c = rng.standard_normal(len(refc["edges"])).astype(np.float32)
    gotc = pc.expand_edge_grad(torch.from_numpy(de_c).to(_dev()))
    assert gotc.shape == (len(col),) and _same(gotc, R.expand_edge_grad_csr(refc, rp, col, dist, de_c))
    v = rng.standard_normal(len(ref["keep"])).astype(np.float32)
    full = p.expand(v, fill=-1.5).cpu().numpy()
    want = np.full(N, -1.5, np.float32)
    want[ref["keep"]] = v
    assert np.array_equal(full, want)
    sel = np.nonzero(seed)[0]
    part = p.expand(v[ref["idx"][sel]], selected=True).cpu().numpy()
    with pytest.raises(ValueError):
        p.expand(v[:-1] if len(v) > 1 else np.zeros(2))
    assert np.array_equal(part[sel], v[ref["idx"][sel]]) and np.isnan(np.delete(part, sel)).all()


# ------------------------------------------------------------------------------------------------------------- 3. model
@functools.lru_cache(maxsize=None)
def _structure():
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(PDB)
    return atoms_onehot(s.elements), np.asarray(s.frames[0], np.float32)


@functools.lru_cache(maxsize=None)
def _model(F, unit_scale=False, noise=None):
    """``unit_scale``: the per-element output scaling of tests/test_gpu_parity.py (std in [0.5, 2], avg in [-1, 1], the same
    draws), the setting its absolute PEAK_ATOL belongs to — shifts of order 1.  With the shipped standards the shifts of
    this structure reach 211 ppm, where one float32 step is 1.5e-5 and the engine's own rounding on the WHOLE batch is
    1.4e-4 (F = 64) to 4.2e-4 (F = 256), measured; the relative tolerances of the restraint tests use those standards."""
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    kw = {} if F is None else dict(atom_feature_size=F)
    if noise is not None:
        kw["noise"] = noise
    standards = load_standards()
    if unit_scale:
        rng = np.random.default_rng(5)
        std, avg = rng.uniform(0.5, 2.0, 10).astype(np.float32), rng.uniform(-1.0, 1.0, 10).astype(np.float32)
        standards = {k: ("X", float(avg[k]), float(std[k])) for k in range(10)}
    m = GNNModel(make_hp(**kw), standards, device=_dev(), seed=3)
    m.build(_structure()[0].shape[1])
    return m


def _padded_lists(batch):
    if not batch.is_csr:
        return batch.nlist.cpu().numpy().astype(np.int64), batch.edges.detach().cpu().numpy().astype(np.float64)
    nl, ed, _, _ = R.csr_to_padded(batch.row_ptr.cpu().numpy(), batch.nlist.cpu().numpy(),
                                   batch.edges.detach().cpu().numpy().astype(np.float64))
    return nl, ed


_REF = {}


def _ref_peaks(F, form, batch, unit_scale=True):
    """float64 shifts of the WHOLE graph, once per (width, list form, output scale)"""
    if (F, form, unit_scale) not in _REF:
        from oracle import torch_ref
        model = _model(F, unit_scale)
        atoms = _structure()[0]
        nl, ed = _padded_lists(batch)
        p = torch_ref.to_torch_params(model.get_weights())
        C_ = atoms.shape[1]
        with torch.no_grad():
            _REF[(F, form, unit_scale)] = torch_ref.forward((atoms, nl, ed, batch.inv_degree.cpu().numpy()), p, hp_to_oracle(model.hypers),
                                                peak_std=model.peak_std[:C_], peak_avg=model.peak_avg[:C_], order="alg").numpy()
    return _REF[(F, form, unit_scale)]


def _selection(n, how):
    """5 % of the atoms: at random, or the first 5 % of the chain (compact in space)"""
    if how == "random":
        return np.sort(np.random.default_rng(5).choice(n, n // 20, replace=False))
    return np.arange(n // 20)


@pytest.mark.parametrize("how", ["random", "block"])
@pytest.mark.parametrize("path", ["table", "edge", "cutoff_csr"])
@pytest.mark.parametrize("F", [64, None], ids=["F64", "F256"])
def test_predict_selected_against_float64_of_the_whole_graph(F, path, how):
    """5 % of the atoms of 108M.pdb.  Chosen at random they are everywhere in the protein, and four steps over 16 nearest
    neighbours reach all 2482 atoms from them (M == N, measured; only the entries of the outermost rows go) — so that
    the forward ran on FEWER atoms is asserted for the compact selection, the accuracy for both."""
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    atoms, pos = _structure()
    n = atoms.shape[0]
    model = _model(F, True)
    eng = model.engine
    sel = _selection(n, how)
    batch = frames_to_batch_cutoff(atoms, pos, cutoff=3.0, device=_dev()) if path == "cutoff_csr" else \
        frames_to_batch(atoms, pos, device=_dev())
    ref = _ref_peaks(F, "csr" if path == "cutoff_csr" else "knn", batch)
    saved = eng.edge_table, eng.edge_table_min_edges
    seen = []
    forward = eng.forward
    eng.forward = lambda b, *a, **k: (seen.append((b.N, b.n_edges)), forward(b, *a, **k))[1]
    try:
        eng.edge_table, eng.edge_table_min_edges = path == "table", 0
        got = model.predict_selected(batch, sel)
        mask = np.zeros(n, bool)
        mask[sel] = True
        again = model.predict_selected(batch, mask)                  # the mask form, on the same edge path
    finally:
        del eng.forward
        eng.edge_table, eng.edge_table_min_edges = saved
    assert got.shape == (len(sel),) and got.is_cuda
    err = float(np.max(np.abs(got.cpu().numpy() - ref[sel])))
    whole = model(batch).cpu().numpy()
    print(f"predict_selected F={F} {path} {how}: ran on {seen[0][0]} of {n} atoms, {seen[0][1]} of {batch.n_edges} entries, "
          f"max |err| {err:.2e} (whole batch at the same atoms {np.max(np.abs(whole[sel] - ref[sel])):.2e}, everywhere "
          f"{np.max(np.abs(whole - ref)):.2e})")
    assert len(seen) == 2                                          # the engine's forward saw the pruned batches only
    if how == "block":
        assert seen[0][0] < n and seen[0][1] < batch.n_edges
    else:                     # the fact of this structure stated above: nothing to drop but entries of the outermost rows
        assert seen[0][0] == n and seen[0][1] <= batch.n_edges
    assert err < PEAK_ATOL, err
    assert torch.equal(got, again)                                   # mask and index forms, and determinism
    assert model.receptive_hops == 4


@pytest.mark.parametrize("path", ["table", "edge", "cutoff_csr"])
@pytest.mark.parametrize("F", [64, None], ids=["F64", "F256"])
def test_predict_selected_with_the_shipped_standards(F, path):
    """the same comparison at the scale users see (shifts up to 211 ppm): PEAK_ATOL carried over per atom.  A shift is
    ``full * std_e + avg_e``; PEAK_ATOL bounds the error where std_e <= 2 (tests/test_gpu_parity.py), i.e. PEAK_ATOL / 2 on
    ``full``, so the bound of an atom of element e is PEAK_ATOL * std_e / 2 plus half a float32 step of the shift itself
    (the final ``+ avg_e`` rounds once more).  Elements without a standard (std = avg = 0) must give exactly 0."""
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    atoms, pos = _structure()
    n = atoms.shape[0]
    model = _model(F)
    eng = model.engine
    sel = _selection(n, "block")
    batch = frames_to_batch_cutoff(atoms, pos, cutoff=3.0, device=_dev()) if path == "cutoff_csr" else \
        frames_to_batch(atoms, pos, device=_dev())
    ref = _ref_peaks(F, "csr" if path == "cutoff_csr" else "knn", batch, unit_scale=False)
    saved = eng.edge_table, eng.edge_table_min_edges
    try:
        eng.edge_table, eng.edge_table_min_edges = path == "table", 0
        got = model.predict_selected(batch, sel).cpu().numpy()
    finally:
        eng.edge_table, eng.edge_table_min_edges = saved
    std = model.peak_std[:atoms.shape[1]][np.argmax(atoms[sel], axis=1)].astype(np.float64)
    bound = PEAK_ATOL * std / 2.0 + 2.0 ** -24 * np.abs(ref[sel])
    err = np.abs(got - ref[sel])
    print(f"predict_selected shipped standards F={F} {path}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
          f"max |err| {err.max():.2e}, max |shift| {np.abs(ref[sel]).max():.1f}")
    assert (err <= bound).all(), float(np.max(err / np.maximum(bound, 1e-300)))


# --------------------------------------------------------------------------------------------------------- 4. restraint
def _ref_restraint(model, atoms, batch, pos, targets, w, box_h=None):
    """(energy, d energy / d positions) of sum w (peaks - targets)^2 in float64: distances rebuilt from the positions over
    the batch's own lists (minimum image through the box's lattice vectors ``box_h`` [3, 3]), torch_ref.forward, autograd —
    as tests/test_gpu_input_grad.py's _ref_positions_grad"""
    from oracle import torch_ref
    N = pos.shape[0]
    x = torch.tensor(pos.astype(np.float64), requires_grad=True)
    nlist = batch.nlist.cpu().numpy().astype(np.int64)
    live = torch.from_numpy(batch.edges.detach().cpu().numpy() > 0)
    nl = torch.from_numpy(nlist)
    v = x[nl] - x[torch.arange(N)[:, None].expand_as(nl)]
    if box_h is not None:
        h = torch.from_numpy(np.asarray(box_h, np.float64))
        with torch.no_grad():                                        # the image the builder chose: nearest in fractional space
            shift = torch.round(v @ torch.linalg.inv(h))
        v = v - shift @ h
    dist = torch.sqrt((v * v).sum(-1).clamp_min(1e-300)) * batch.scale
    with torch.no_grad():                                            # the images must be the builder's
        assert float((torch.where(live, dist, torch.zeros_like(dist)) - batch.edges.detach().cpu().double()).abs().max()) < 1e-5
    d = torch.where(live, dist, torch.zeros_like(dist))
    p = torch_ref.to_torch_params(model.get_weights())
    C_ = atoms.shape[1]
    peaks = torch_ref.forward((atoms, nlist, d, batch.inv_degree.cpu().numpy()), p, hp_to_oracle(model.hypers),
                              peak_std=model.peak_std[:C_], peak_avg=model.peak_avg[:C_], order="alg")
    e = ((peaks - torch.from_numpy(targets.astype(np.float64))) ** 2 * torch.from_numpy(w.astype(np.float64))).sum()
    e.backward()
    return float(e), x.grad.numpy()


def _restraint_problem(n, seed=8):
    rng = np.random.default_rng(seed)
    targets = rng.standard_normal(n).astype(np.float32)
    w = np.zeros(n, np.float32)
    at = np.arange(n // 20)                    # the first 5 % of the chain: compact, so that atoms outside the field exist
    w[at] = rng.uniform(0.5, 1.5, len(at)).astype(np.float32)
    return targets, w


@pytest.mark.parametrize("kind", ["open", "ortho", "triclinic"])
def test_shift_restraint_pruned_against_float64(kind):
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.library import shift_restraint
    from nmrgnn_amd.pbc import prepare
    atoms, pos = _structure()
    n = atoms.shape[0]
    model = _model(64)
    targets, w = _restraint_problem(n)
    span = float((pos.max(0) - pos.min(0)).max())
    box = {"open": None, "ortho": (span + 3.0, span + 4.0, span + 5.0, 90.0, 90.0, 90.0),
           "triclinic": (span + 3.0, span + 4.0, span + 5.0, 80.0, 95.0, 100.0)}[kind]
    if box is not None:       # the structure's centre on a corner of the cell, wrapped: neighbours sit across every face
        h = prepare(np.asarray(box), 1)[0].reshape(3, 3).astype(np.float64)
        frac = (pos - pos.mean(0)).astype(np.float64) @ np.linalg.inv(h)
        pos = ((frac - np.floor(frac)) @ h).astype(np.float32)
    e0, f0, v0 = shift_restraint(model, atoms, pos, targets, w, box=box, virial=True)
    e0b, f0b, v0b = shift_restraint(model, atoms, pos, targets, w, box=box, virial=True, prune=False)
    assert torch.equal(e0, e0b) and torch.equal(f0, f0b) and torch.equal(v0, v0b)       # prune=False is today's call
    e1, f1, v1 = shift_restraint(model, atoms, pos, targets, w, box=box, virial=True, prune=True)
    e2, f2 = shift_restraint(model, atoms, pos, targets, w, box=box, prune=True)
    assert torch.equal(e1, e2) and torch.equal(f1, f2) and f1.shape == (n, 3) and v1.shape == (3, 3)
    batch = frames_to_batch(atoms, pos, device=_dev(), box=box)
    h = None if box is None else prepare(np.asarray(box), 1)[0].reshape(3, 3)
    e_ref, g_ref = _ref_restraint(model, atoms, batch, pos, targets, w, h)
    err_f, err_e = _rel(-f1.cpu().numpy(), g_ref), abs(float(e1) - e_ref) / abs(e_ref)
    print(f"restraint prune {kind}: forces rel err {err_f:.2e} (unpruned {_rel(-f0.cpu().numpy(), g_ref):.2e}), energy {err_e:.2e}")
    assert err_f <= 1e-4 and err_e <= 1e-5, (err_f, err_e)
    hop = batch.restrict(w != 0, model.receptive_hops)._prune[1].cpu().numpy()
    outside = hop == -1
    assert outside.any() and (f1.cpu().numpy()[outside] == 0).all()
    assert _rel(v1.cpu().numpy(), v0.cpu().numpy()) <= 1e-4         # the virial of the same edge gradient


def _ref_ragged_grad(model, atoms, batch, pos, sel, y):
    """d/d positions of sum_sel (peaks - y)^2 in float64 on a ragged batch whose structures have boxes of their own (or
    none): distances rebuilt from the positions over the batch's lists, every row with the minimum image of ITS structure's
    lattice vectors (``batch.box`` [G, 9], ``batch.box_kind_host`` < 0: open), torch_ref.forward, autograd — _ref_restraint
    per structure"""
    from oracle import torch_ref
    N = pos.shape[0]
    gp = batch.graph_ptr_host.astype(np.int64)
    G = len(gp) - 1
    H = batch.box.cpu().double().reshape(G, 3, 3)
    Hinv = torch.zeros_like(H)
    for g in range(G):
        if batch.box_kind_host[g] >= 0:
            Hinv[g] = torch.linalg.inv(H[g])
        else:
            H[g] = 0.0
    gid = torch.from_numpy(np.repeat(np.arange(G), np.diff(gp)))
    x = torch.tensor(pos.astype(np.float64), requires_grad=True)
    nlist = batch.nlist.cpu().numpy().astype(np.int64)
    live = torch.from_numpy(batch.edges.detach().cpu().numpy() > 0)
    nl = torch.from_numpy(nlist)
    v = x[nl] - x[torch.arange(N)[:, None].expand_as(nl)]
    with torch.no_grad():
        shift = torch.round(torch.einsum("nkc,ncd->nkd", v, Hinv[gid]))
    v = v - torch.einsum("nkd,ndc->nkc", shift, H[gid])
    dist = torch.sqrt((v * v).sum(-1).clamp_min(1e-300)) * batch.scale
    with torch.no_grad():                                            # the images must be the builder's
        assert float((torch.where(live, dist, torch.zeros_like(dist)) - batch.edges.detach().cpu().double()).abs().max()) < 1e-5
    d = torch.where(live, dist, torch.zeros_like(dist))
    p = torch_ref.to_torch_params(model.get_weights())
    C_ = atoms.shape[1]
    peaks = torch_ref.forward((atoms, nlist, d, batch.inv_degree.cpu().numpy()), p, hp_to_oracle(model.hypers),
                              peak_std=model.peak_std[:C_], peak_avg=model.peak_avg[:C_], order="alg")
    ((peaks[torch.from_numpy(sel)] - torch.from_numpy(y.astype(np.float64))) ** 2).sum().backward()
    return x.grad.numpy()


def test_pruned_autograd_on_a_ragged_boxed_batch():
    """loss(model(pruned)[pruned.selected]).backward() reaches pos.grad through the parent, on three structures (an
    orthorhombic box, none, a triclinic box; the boxed ones wrapped about a corner of their cell): against the float64
    positions gradient of the whole batch at relative 1e-4 of its maximum, the bound of tests/test_gpu_input_grad.py;
    exactly 0.0 on every atom outside the field"""
    from nmrgnn_amd.graph import structures_to_batch
    from nmrgnn_amd.pbc import prepare
    atoms, pos = _structure()
    model = _model(64)
    rng = np.random.default_rng(3)
    at = [atoms[:300], atoms[300:301], atoms[400:900]]
    span = 60.0
    boxes = [(span, span + 2, span + 4, 90.0, 90.0, 90.0), None, (span, span + 2, span + 4, 85.0, 95.0, 100.0)]
    parts = [pos[:300], pos[300:301], pos[400:900]]
    for g, b in enumerate(boxes):
        if b is not None:
            h = prepare(np.asarray(b), 1)[0].reshape(3, 3).astype(np.float64)
            frac = (parts[g] - parts[g].mean(0)).astype(np.float64) @ np.linalg.inv(h)
            parts[g] = ((frac - np.floor(frac)) @ h).astype(np.float32)
    N = 801
    sel = np.arange(301, 326)                                                  # in the last structure only, and compact
    y = rng.standard_normal(len(sel)).astype(np.float32)
    yd = torch.from_numpy(y).to(_dev())
    grads = {}
    for prune in (False, True):
        xs = [torch.tensor(q, device=_dev(), requires_grad=True) for q in parts]
        batch = structures_to_batch(at, xs, boxes=boxes, device=_dev())
        assert batch.edges.grad_fn is not None and batch.N == N
        if prune:
            pr = batch.restrict(sel, model.receptive_hops)
            assert pr.edges.grad_fn is not None and pr.G == 1 and pr.graph_index.tolist() == [2] and pr.N < 500
            peaks = model(pr)[pr.selected]
            hop = pr._prune[1].cpu().numpy()
        else:
            peaks = model(batch)[torch.from_numpy(sel).to(_dev())]
        ((peaks - yd) ** 2).sum().backward()
        grads[prune] = np.concatenate([x.grad.cpu().numpy() for x in xs])
    ref = _ref_ragged_grad(model, np.concatenate(at), batch, np.concatenate(parts), sel, y)
    err, err_whole = _rel(grads[True], ref), _rel(grads[False], ref)
    print(f"ragged boxed autograd against float64: pruned rel {err:.2e} (whole batch {err_whole:.2e}), kept {pr.N} of {N}")
    assert err <= 1e-4, err
    outside = hop == -1
    assert outside[:301].all() and outside[301:].any() and (grads[True][outside] == 0).all()
    assert (ref[outside] == 0).all() and np.abs(grads[True][~outside]).max() > 0


def test_shift_uncertainty_select():
    """``select=`` gives [n] outputs, NaN outside the selection.  Tight where the two calls compute the same thing: a model
    without distance noise runs one replica (mean and std_model are deterministic, std_input exactly 0), and with
    ``position_sigma`` both calls perturb the same replicas — there the pruned and the whole call differ by float32
    rounding of different tiles only, bounded like the energies of this file (relative 1e-5 of the largest value) and, for
    the shifts, by twice PEAK_ATOL carried to their scale as in test_predict_selected_with_the_shipped_standards.  With the
    model's own noise the draws run over the restricted lists: the same distribution, other numbers — shape and
    finiteness only."""
    from nmrgnn_amd.library import shift_uncertainty
    atoms, pos = _structure()
    n = atoms.shape[0]
    sel = np.sort(np.random.default_rng(5).choice(n, 40, replace=False))
    rest = np.delete(np.arange(n), sel)

    def both(model, **kw):
        full = [t.cpu().numpy() for t in shift_uncertainty(model, atoms, pos, samples=4, seed=2, **kw)]
        part = [t.cpu().numpy() for t in shift_uncertainty(model, atoms, pos, samples=4, seed=2, select=sel, **kw)]
        for b in part:
            assert b.shape == (n,) and np.isnan(b[rest]).all() and np.isfinite(b[sel]).all()
        return full, part

    quiet = _model(64, noise=0.0)
    std = quiet.peak_std[:atoms.shape[1]][np.argmax(atoms[sel], axis=1)].astype(np.float64)
    full, part = both(quiet)
    assert (part[2][sel] == 0).all() and (full[2] == 0).all()
    assert (np.abs(part[0][sel] - full[0][sel]) <= PEAK_ATOL * std + 2.0 ** -23 * np.abs(full[0][sel])).all()
    assert _rel(part[1][sel], full[1][sel]) <= 1e-5 and full[1][sel].max() > 0
    full, part = both(quiet, position_sigma=0.1)
    assert (np.abs(part[0][sel] - full[0][sel]) <= PEAK_ATOL * std + 2.0 ** -23 * np.abs(full[0][sel])).all()
    for k in (1, 2):
        assert _rel(part[k][sel], full[k][sel]) <= 1e-5 and full[k][sel].max() > 0, (k, _rel(part[k][sel], full[k][sel]))
    full, part = both(_model(64))
    assert part[2][sel].max() > 0 and part[1][sel].max() > 0


# --------------------------------------------------------------------------------------------------------------- 5. CLI
def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_eval_struct_atom_names(tmp_path):
    from click.testing import CliRunner
    from nmrgnn_amd.main import main
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(PDB)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        res = CliRunner().invoke(main, ["eval-struct", "--keep-going", PDB, str(tmp_path / "all.csv")])
        assert res.exit_code == 0, res.output
        res = CliRunner().invoke(main, ["eval-struct", "--keep-going", "--atom-names", "H,N,CA", PDB, str(tmp_path / "sel.csv")])
        assert res.exit_code == 0, res.output
        bad = CliRunner().invoke(main, ["eval-struct", "--keep-going", "--atom-names", "QQ,ZZ9", PDB, str(tmp_path / "bad.csv")])
    every, sel = _rows(tmp_path / "all.csv"), _rows(tmp_path / "sel.csv")
    want = [i for i in range(s.n_atoms) if s.names[i] in ("H", "N", "CA")]
    assert 0 < len(want) < s.n_atoms and sel[0] == every[0]
    assert [int(r[0]) for r in sel[1:]] == want
    by_index = {int(r[0]): r for r in every[1:]}
    for r in sel[1:]:
        full = by_index[int(r[0])]
        assert r[1:4] == full[1:4] and r[6:] == full[6:]
        assert abs(float(r[4]) - float(full[4])) <= 0.01 + 1e-3, (r, full)
    assert bad.exit_code != 0 and "no atom" in bad.output and "Traceback" not in bad.output
    assert not (tmp_path / "bad.csv").exists()


def test_eval_structure_atom_names_with_the_other_options(tmp_path):
    """--atom-names beside --average, --uncertainty, --pbc and --separate --boxes: the rows are the matching atoms, with
    their original indices, in every mode"""
    from nmrgnn_amd.main import AtomNamesError, eval_structure
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(PDB)
    names = ["N", "CA"]
    want = [i for i in range(s.n_atoms) if s.names[i] in names]
    quiet = dict(keep_going=True, echo=lambda *a: None, atom_names=names)
    has_box = s.dimensions[0] is not None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        eval_structure((PDB,), str(tmp_path / "plain.csv"), **quiet)
        eval_structure((PDB,), str(tmp_path / "avg.csv"), average=True, **quiet)
        eval_structure((PDB,), str(tmp_path / "unc.csv"), uncertainty=2, **quiet)
        eval_structure((PDB, PDB), str(tmp_path / "sep.csv"), separate=True, **quiet)
        eval_structure((PDB, PDB), str(tmp_path / "sepbox.csv"), separate=True, boxes=True, **quiet)
        if has_box:
            eval_structure((PDB,), str(tmp_path / "pbc.csv"), pbc=True, **quiet)
        with pytest.raises(AtomNamesError):
            eval_structure((PDB, PDB), str(tmp_path / "none.csv"), separate=True, keep_going=True, echo=lambda *a: None,
                           atom_names=["QQ"])
    plain, avg, unc, sep = (_rows(tmp_path / f) for f in ("plain.csv", "avg.csv", "unc.csv", "sep.csv"))
    assert [int(r[0]) for r in plain[1:]] == [int(r[0]) for r in avg[1:]] == [int(r[0]) for r in unc[1:]] == want
    near = lambda a, b: max(abs(float(x) - float(y)) for x, y in zip(a, b)) <= 0.01 + 1e-3      # one rounding step of the CSV
    assert near([r[4] for r in avg[1:]], [r[4] for r in plain[1:]]) and all(float(r[5]) == 0 for r in avg[1:])
    assert unc[0][-2:] == ["std_model", "std_input"] and all(np.isfinite(float(r[8])) and np.isfinite(float(r[9])) for r in unc[1:])
    assert [r[:4] + r[5:8] for r in unc[1:]] == [r[:4] + r[5:8] for r in plain[1:]] and near([r[4] for r in unc[1:]], [r[4] for r in plain[1:]])
    assert [int(r[1]) for r in sep[1:]] == want + want and near([r[5] for r in sep[1:len(want) + 1]], [r[4] for r in plain[1:]])
    assert [int(r[1]) for r in _rows(tmp_path / "sepbox.csv")[1:]] == want + want
    if has_box:
        assert [int(r[0]) for r in _rows(tmp_path / "pbc.csv")[1:]] == want
