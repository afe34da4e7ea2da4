"""Engine.backward(edge_grad=) through the table of the edge Jacobian (Engine.edge_grad_table): parity with
float64 autograd and with the per-edge launch, the default left bit for bit, the three ways the guard hands a call back to
the per-edge launch, the host-guarded table of an edge shape without the fused kernels, and the inputs-only tape."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import hp_to_oracle, make_hp, randomize_biases, small_batch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


def _engine(E=3, act="softplus", H=128, seed=5):
    from nmrgnn_amd.engine import Engine
    hp = make_hp(atom_feature_size=64, edge_hidden_size=H, edge_fc_layers=4, edge_feature_size=E, fc_activation=act)
    eng = Engine(hp, 10, device=_dev(), seed=seed)
    randomize_biases(eng, seed=seed)
    eng.edge_table, eng.edge_table_min_edges = True, 0
    return hp, eng


_BATCH = {}


def _batch():
    """512 atoms x K = 16, a third of the slots dead; the upstream gradient"""
    if not _BATCH:
        from nmrgnn_amd.graph import GraphBatch
        b = small_batch(2, 256, 16, 10, seed=3, p_pad=0.33)
        gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=_dev())
        dpeaks = np.random.default_rng(9).standard_normal(b["edges"].shape[0]).astype(np.float32)
        _BATCH.update(b=b, gb=gb, dpeaks=dpeaks, g_dpeaks=torch.from_numpy(dpeaks).to(_dev()))
        assert 0.25 < float((b["edges"] <= 0).mean()) < 0.45
    return _BATCH


def _run(eng, on, keep_tape=True, param_grad=True, record=None):
    """one forward + backward with the switch ``on``: (edge_grad, params.grad, the tape's edge path)"""
    B = _batch()
    eng.edge_grad_table = on
    eng.forward(B["gb"], training=False, keep_tape=keep_tape)
    tp = eng.tape
    path = tp.edge_path
    out = torch.full(B["gb"].edges.shape, 7.0, device=_dev())
    if record is not None:      # the tape and the de the backward hands to its input-gradient launch
        inner = eng._edge_dinput
        eng._edge_dinput = lambda tp_, de, o: (record.update(tp=tp_, de=de.clone()), inner(tp_, de, o))[1]
    try:
        eng.backward(B["g_dpeaks"], edge_grad=out, param_grad=param_grad)
    finally:
        if record is not None:
            del eng._edge_dinput
    torch.cuda.synchronize()
    return out, eng.params.grad.clone(), path


_REF = {}


def _ref_edge_grad(hp, eng, key):
    """dL/d(edges) of L = sum(dpeaks * peaks) by float64 torch autograd of oracle.torch_ref.forward (once per model)"""
    if key not in _REF:
        from oracle import torch_ref
        B = _batch()
        b = B["b"]
        p = torch_ref.to_torch_params(eng.params.state_dict())
        d = torch.tensor(np.asarray(b["edges"], np.float64), requires_grad=True)
        peaks = torch_ref.forward((b["atoms"], b["nlist"], d, b["inv_degree"]), p, hp_to_oracle(hp), training=False)
        (peaks * torch.from_numpy(B["dpeaks"].astype(np.float64))).sum().backward()
        _REF[key] = d.grad.numpy()
    return _REF[key]


@pytest.mark.parametrize("E", [3, 8])
def test_parity_with_float64_autograd_and_with_the_per_edge_launch(E, act="softplus"):
    hp, eng = _engine(E, act)
    on, g_on, path = _run(eng, True)
    assert path == "table"
    up, err, scale = eng.edge_grad_table_report()
    print(f"E={E} {act}: J check err / scale = {err / scale:.2e} (tol {eng.edge_grad_table_tol:.1e})")
    assert not up and err <= eng.edge_grad_table_tol * scale
    off, g_off, _ = _run(eng, False)
    with pytest.raises(RuntimeError):
        eng.edge_grad_table_report()          # the last backward took no Jacobian table
    ref = _ref_edge_grad(hp, eng, (E, act))
    dead = _batch()["b"]["edges"] <= 0
    e64, e_pe = _rel(on.cpu().numpy(), ref), _rel(on.cpu().numpy(), off.cpu().numpy())
    print(f"E={E} {act}: against float64 {e64:.2e}, against per edge {e_pe:.2e}")
    assert e64 <= 1e-4, e64
    assert e_pe <= 1e-5, e_pe
    assert np.all(on.cpu().numpy()[dead].view(np.uint32) == 0)
    assert not torch.equal(on, off)           # the table did answer
    assert torch.equal(g_on, g_off)           # params.grad does not see the switch


def test_default_is_one_per_edge_launch_bit_for_bit():
    from nmrgnn_amd._lib import ptr, ptr_array
    hp, eng = _engine()
    assert eng.edge_grad_table is False
    rec = {}
    off, _, path = _run(eng, False, record=rec)
    assert path == "table"
    tp, de = rec["tp"], rec["de"]
    perm, _, d_c, n_live = tp.live
    W = [eng.params[f"edge_fc/{t}/kernel"] for t in range(eng.Le)]
    B = [eng.params[f"edge_fc/{t}/bias"] for t in range(eng.Le)]
    direct = torch.full_like(off, 7.0)
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    eng._ck(eng.lib.ng_edge_mlp_dinput(eng.ctx.handle, st, tp.batch.n_edges, eng.H, eng.E, eng.Le, eng.fc_act, ptr(d_c),
                                       ptr(tp.d_eff), ptr(perm), ptr(n_live), ptr(eng.centers), eng.gap, ptr_array(W),
                                       ptr_array(B), ptr(de), None, ptr(direct)), "ng_edge_mlp_dinput")
    torch.cuda.synchronize()
    assert torch.equal(off, direct)


def test_environment_switch(monkeypatch):
    monkeypatch.setenv("NG_EDGE_GRAD_TABLE", "1")
    assert _engine()[1].edge_grad_table is True
    monkeypatch.setenv("NG_EDGE_GRAD_TABLE", "0")
    assert _engine()[1].edge_grad_table is False


@pytest.mark.parametrize("how", ["relu", "force_fallback", "weights_x16"])
def test_guard_up_returns_the_per_edge_bits(how):
    hp, eng = _engine(3, "relu" if how == "relu" else "softplus")
    if how == "force_fallback":
        eng.edge_table_force_fallback = True
    if how == "relu":
        # e of a relu MLP has kinks too: at the default tolerance the value guard is up and J is never consulted (a relu edge
        # MLP has no fused live kernels — ng_edge_live_supported — so its guard is read on the host and the tape then carries
        # no table at all).  The value table is let stand, so that the guard under test is the one of J.
        eng.edge_table_tol = 1.0
    if how == "weights_x16":
        sd = eng.params.state_dict()
        for k in sd:
            if k.startswith("edge_fc/") and k.endswith("kernel"):
                sd[k] = sd[k] * np.float32(16)
        eng.params.load_state_dict(sd)
    B = _batch()
    eng.forward(B["gb"], training=False, keep_tape=True)
    value_up = eng.edge_table_report()[0]
    eng.tape = None
    on, _, path = _run(eng, True)
    assert path in ("table", "table_host")
    up, err, scale = eng.edge_grad_table_report()
    print(f"{how}: value guard {value_up}, J guard {up}, J err / scale {err / max(scale, 1e-300):.2e}")
    assert up
    if how == "relu":           # the J check itself, not ``prev``: far above the tolerance, while the softplus model is below it
        assert value_up is False
        assert err > 1e3 * eng.edge_grad_table_tol * scale
        _, soft = _engine(3, "softplus")
        _run(soft, True)
        assert not soft.edge_grad_table_report()[0]
    if how == "weights_x16":    # the value guard of the call, carried into the J gate by ``prev``
        assert value_up
    off, _, _ = _run(eng, False)
    assert torch.equal(on, off)
    assert float(on.abs().max()) > 0


@pytest.mark.parametrize("E", [3, 8])
def test_tanh_edge_stage_through_the_c_interface(E):
    """The model's hyperparameter space offers softplus and relu only, and oracle/torch_ref evaluates softplus, so a tanh edge
    MLP is taken at the stage this path changes, through the C entry points the engine chains: the J table of the batch's
    distance range, its check (guard down at the engine's tolerance), ng_edge_table_dinput against the per-edge
    ng_edge_mlp_dinput (1e-5) and against the float64 Jacobian of tests/edge_table_grad_ref.py (1e-4)."""
    import edge_table_grad_ref as R
    from nmrgnn_amd._lib import ptr, ptr_array
    from nmrgnn_amd.engine import Engine, rbf_grid
    _, eng = _engine(E)
    H, Le, T, act = 128, 4, eng._table_points(), 3
    lib, h = eng.lib, eng.ctx.handle
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    rng = np.random.default_rng(E)
    W64, B64 = R.random_mlp(H, E, Le, 1.0, seed=E)
    W = [torch.from_numpy(w.astype(np.float32)).to(_dev()) for w in W64]
    Bs = [torch.from_numpy(b.astype(np.float32)).to(_dev()) for b in B64]
    edges = _batch()["gb"].edges.reshape(-1)
    n = edges.shape[0]
    de = torch.from_numpy(rng.standard_normal((n, E)).astype(np.float32)).to(_dev())
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=_dev())
    r4, d_tab, ones, J_all, dd0 = new(4), new(2 * T), new(2 * T), new(2 * T, E), new(2 * T)
    gate = torch.empty(8, dtype=torch.int32, device=_dev())
    eng._ck(lib.ng_edge_table_range(h, st, n, E, ptr(edges), ptr(edges), None, None, 0.0, ptr(r4)), "range")
    eng._ck(lib.ng_edge_table_points(h, st, T, 1, ptr(r4), ptr(d_tab), ptr(ones), None), "points")
    dinput = lambda m, d_src, d_eff, g, J, out: eng._ck(lib.ng_edge_mlp_dinput(
        h, st, m, H, E, Le, act, ptr(d_src), ptr(d_eff), None, None, ptr(eng.centers), eng.gap, ptr_array(W), ptr_array(Bs),
        ptr(g), ptr(J), ptr(out)), "ng_edge_mlp_dinput")
    dinput(2 * T, ones, d_tab, torch.zeros(2 * T, E, device=_dev()), J_all, dd0)
    eng._ck(lib.ng_edge_table_check(h, st, T, E, ptr(J_all), float(eng.edge_grad_table_tol), ptr(r4), None, None, 2 * T, None,
                                    ptr(gate)), "check")
    tab, per_edge = new(n), new(n)
    eng._ck(lib.ng_edge_table_dinput(h, st, n, E, T, ptr(edges), ptr(edges), None, ptr(r4), ptr(J_all), ptr(gate), ptr(de),
                                     ptr(tab)), "ng_edge_table_dinput")
    dinput(n, edges, edges, de, None, per_edge)
    torch.cuda.synchronize()
    g = gate.cpu().numpy()
    err, scale = g[4:6].view(np.float32)
    print(f"tanh E={E}: J check err / scale = {err / scale:.2e}")
    assert g[0] == 0
    d = edges.cpu().numpy()
    W32 = [w.astype(np.float32).astype(np.float64) for w in W64]
    B32 = [b.astype(np.float32).astype(np.float64) for b in B64]
    c64 = eng.centers.cpu().numpy().astype(np.float64)
    J = R.mlp_value_and_jacobian(d, c64, float(np.float32(eng.gap)), W32, B32, "tanh")[1]
    ref = np.where(d > 0, (J * de.cpu().numpy()).sum(1), 0.0)
    e64, e_pe = _rel(tab.cpu().numpy(), ref), _rel(tab.cpu().numpy(), per_edge.cpu().numpy())
    print(f"tanh E={E}: against float64 {e64:.2e}, against per edge {e_pe:.2e}")
    assert e64 <= 1e-4 and e_pe <= 1e-5
    assert np.all(tab.cpu().numpy()[d <= 0].view(np.uint32) == 0)


def test_host_guarded_table_of_an_edge_shape_without_the_fused_kernels():
    hp, eng = _engine(3, "softplus", H=64)
    on, _, path = _run(eng, True)
    assert path == "table_host"
    assert not eng.edge_grad_table_report()[0]
    off, _, _ = _run(eng, False)
    e64 = _rel(on.cpu().numpy(), _ref_edge_grad(hp, eng, "H64"))
    print(f"table_host: against float64 {e64:.2e}, against per edge {_rel(on.cpu().numpy(), off.cpu().numpy()):.2e}")
    assert e64 <= 1e-4
    assert not torch.equal(on, off)
    # a forced J guard (the value table stands: the forward took it): the per-edge bits
    eng.edge_grad_table = True
    B = _batch()
    eng.forward(B["gb"], training=False, keep_tape=True)
    assert eng.tape.edge_path == "table_host"
    eng.edge_table_force_fallback = True
    forced = torch.full_like(on, 7.0)
    eng.backward(B["g_dpeaks"], edge_grad=forced)
    eng.edge_table_force_fallback = False
    torch.cuda.synchronize()
    assert eng.edge_grad_table_report()[0]
    assert torch.equal(forced, off)


def test_inputs_only_tape():
    hp, eng = _engine()
    B = _batch()
    full, _, _ = _run(eng, True, keep_tape=True, param_grad=False)
    inp, _, path = _run(eng, True, keep_tape="inputs", param_grad=False)
    assert path == "table" and torch.equal(full, inp)
    off_full, _, _ = _run(eng, False, keep_tape=True, param_grad=False)
    off_inp, _, _ = _run(eng, False, keep_tape="inputs", param_grad=False)
    assert torch.equal(off_full, off_inp)
    # no parameter gradients from such a tape: refused before any launch, the tape stays
    eng.forward(B["gb"], training=False, keep_tape="inputs")
    assert eng.tape.z_save is None
    grad0 = eng.params.grad.clone()
    with pytest.raises(RuntimeError, match="inputs"):
        eng.backward(B["g_dpeaks"], edge_grad=torch.empty_like(full))
    with pytest.raises(RuntimeError, match="inputs"):
        eng.backward(B["g_dpeaks"])
    assert eng.tape is not None and torch.equal(grad0, eng.params.grad)
    with pytest.raises(ValueError):
        eng.forward(B["gb"], keep_tape="edges")
    # frozen weights: the second call reuses the table (and its Jacobian table) of the first
    eng.freeze_weights(True)
    a, _, _ = _run(eng, True, keep_tape="inputs", param_grad=False)
    cache = eng._table_cache
    assert cache is not None and "J_all" in cache
    J = cache["J_all"]
    b, _, _ = _run(eng, True, keep_tape="inputs", param_grad=False)
    assert eng._table_cache is cache and cache["J_all"] is J
    assert not eng.edge_grad_table_report()[0]
    # the kept table covers a quarter more than the call on either side: close to, not bitwise, the call's own table
    assert torch.equal(a, b) and _rel(a.cpu().numpy(), full.cpu().numpy()) <= 1e-5
    # a full tape under frozen weights builds its own table as before
    _run(eng, True, keep_tape=True)
    assert eng._table_cache is cache
    eng.freeze_weights(False)
