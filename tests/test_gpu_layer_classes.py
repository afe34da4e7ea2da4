"""The drop-in layer classes of nmrgnn_amd/layers.py (RBFExpansion, MPLayer, MPBlock, EdgeFCBlock, FCBlock, AMPLayer and the
shared _DenseStack._dense / _dense_bwd) by VALUE against the float64 oracle (oracle/nmrgnn_oracle.py: rbf_expand, mp_layer,
mp_block, edge_fc_block, fc_block, glorot_uniform_limit), fed the layers' own weights read back from the device.  The C entry
points behind them have their own files; this one is about the Python glue: padding, slicing, reshaping, residuals, dtypes.

Cases, inputs, references and bounds live in tests/layer_classes_ref.py (checked on the CPU by
tests/test_layer_classes_ref_host.py); its docstring states the three bounds.  Every case draws its inputs from a seeded numpy
generator, compares every element, asserts the result's shape and dtype and that the inputs are unchanged.  Dense biases are
overwritten with 0.1 x a normal draw before the call under test (the Keras zeros hide every bias-padding error): a block is
called once to build, gets its biases, and is called again.

Padding branches of _dense (contraction to a multiple of 8, outputs to a multiple of 4; with a residual both to the same
multiple of 8) and the case ids that reach them:
  contraction padded   EdgeFCBlock first layers with D = 2 / 20: ref-5x2-D2-H128-E3-L4-softplus, n7-D2-H16-E1-L2-relu,
                       60x5-D20-H128-E8-L6-relu, 5x2-D20-H16-E3-L2-relu, 77x3-D2-H128-E64-L2-softplus
  outputs padded       EdgeFCBlock last layers with E = 1 / 2 / 3 (H -> E): ref-5x2-..., n7-D2-H16-E1-L2-relu,
                       31x5-D16-H16-E2-L2-softplus, 5x2-D20-H16-E3-L2-relu, n255-D128-H16-E2-L6-softplus,
                       n1-D16-H128-E1-L4-relu, 33x8-D128-H128-E3-L2-relu
  both padded          FCBlock F = 6 (6 -> 6 as 8 -> 8, 6 -> 3 as 8 -> 4), F = 12 / 20 / 100 (residual layers F -> F on one
                       common multiple of 8, last layers 12 -> 6, 20 -> 10, 100 -> 50): F6-*, F12-*, F20-*, F100-*
  neither padded       FCBlock F16-*, F32-*, F64-*, F256-*; EdgeFCBlock 16x16-D128-H128-E64-L4-softplus,
                       n300-D16-H16-E8-L4-softplus; AMPLayer F = 64 (test_gpu_layers.py)
and of _dense_bwd, through AMPLayer.backward (F x F):
  contraction padded   test_amplayer_small_widths[F12-E3-softplus], [F12-E2-relu] (16 x 12); F = 20, 68, 100 of
                       test_gpu_layers.py
  both padded          test_amplayer_small_widths[F6-E2-tanh], [F6-E3-linear] (8 x 8)
  neither padded       F = 16, 64, 256 of test_gpu_layers.py::test_amplayer_backward_matches_oracle
  outputs padded only  cannot occur for a square kernel (an F that is a multiple of 8 is one of 4)

The FCBlock cases at F = 12, 20 and 100 are the ones that failed before _dense kept the residual under padding (it used to turn
the residual off when the two padded sizes differed): they showed ratios of order 1.

Measured on an MI355X (printed by every case; the largest of each):
  blocks     a32 5.6e-7 and GPU ratio 5.8e-7, both at fc F256-L4-softplus-r300 (300 rows of 256: the split-operand GEMM);
             the largest share of a bound used is 0.25 (fc F256-L6-relu-r1: 5.5e-7 against 8 x 1.5e-7 + 1e-6)
  MPLayer    max|err| / max(mag) 1.9e-7 (F128-E8-relu-nores-ragged-K2) against C_REL = 3e-5 per element
  one _dense max|err| / max(mag) 1.3e-7 (33x8-D128-H128-E3-L2-relu, layer 1)
  RBF        c between 2.5e-7 (one row) and 1.7e-6; at most 0.17 of the bound used by a result in float32's normal range;
             results in the denormal range come back as 0, which uses up to 0.999 of TINY
  with the residual turned off under unequal padding (layers.py before this file) the six FCBlock cases at F = 12, 20, 100
  gave ratios 0.61 .. 0.96 and every other case passed
"""
import zlib

import numpy as np
import pytest

import layer_classes_ref as R

pytestmark = pytest.mark.gpu


def _hp(**kw):
    from nmrgnn_amd.hypers import HyperParameters
    return HyperParameters(**kw)


def host(t):
    return t.detach().cpu().numpy()


def is_f32_on_device(t, shape):
    import torch
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)


def seeded(layer, cid):
    """the layer with the generator of its Glorot draw seeded from the case id: the weights of a case, and with them its
    figures, do not depend on how many layers the process has built before (layers.py counts them for its seeds)"""
    for i, part in enumerate([layer] + list(getattr(layer, "mp", []))):
        part._gen.manual_seed(zlib.crc32(f"{cid}/{i}".encode()))
    return layer


def block_bound(cid, got, ref, a32):
    r = R.ratio(got, ref)
    print(f"[layer-classes] {cid}: a32 {a32:.3e}  gpu {r:.3e}")
    assert np.isfinite(a32) and a32 > 0
    assert r <= R.BLOCK_FACTOR * a32 + R.BLOCK_FLOOR, (cid, r, a32)    # NaN fails
    return r


def set_biases(blk, dims, dev):
    import torch
    bs = R.stack_biases(dims)
    assert all(not host(b).any() for _, b in blk.weights), "a fresh Dense layer has a zero bias (Keras default)"
    assert [tuple(W.shape) for W, _ in blk.weights] == list(zip(dims[:-1], dims[1:]))
    blk.weights = [(W, torch.from_numpy(b).to(dev)) for (W, _), b in zip(blk.weights, bs)]
    return [host(W) for W, _ in blk.weights], bs


# ---------------------------------------------------------------------------------------------------------- RBFExpansion
def rbf_argument(kind, d, dev):
    """(what the layer is handed, a function that says whether it is unchanged)"""
    import torch
    if kind in ("f64", "f32"):
        a = np.array(d, np.float64 if kind == "f64" else np.float32)
        keep = a.copy()
        return a, lambda: np.array_equal(a, keep) and a.dtype == keep.dtype
    d32 = torch.from_numpy(R.f32(d).copy())
    if kind == "view":
        base = torch.full(tuple(d32.shape[:-1]) + (2 * d32.shape[-1],), 999.0)
        base[..., ::2] = d32
        a = base[..., ::2]
        assert not a.is_contiguous()
        keep = base.clone()
        return a, lambda: torch.equal(base, keep)
    a = d32.to(dev)
    return a, lambda: torch.equal(a.cpu(), d32)


@pytest.mark.parametrize("cid,count,shape,kind", R.RBF_CASES, ids=[c[0] for c in R.RBF_CASES])
def test_rbf_expansion(gpu_device, cid, count, shape, kind):
    """exp(-(d - mu)^2 / gap) without a mask (d = 0 and d < 0 give the plain Gaussian), any input rank and container"""
    import nmrgnn_amd
    d = R.rbf_distances(count, shape)
    ref, tol, c = R.rbf_reference(d, count)
    arg, unchanged = rbf_argument(kind, d, gpu_device)
    out = nmrgnn_amd.RBFExpansion(R.RBF_LOW, R.RBF_HIGH, count)(arg)
    assert is_f32_on_device(out, tuple(shape) + (count,))
    got = host(out).astype(np.float64)
    err = np.abs(got - ref)
    normal = ref >= R.TINY
    print(f"[layer-classes] rbf {cid}: c {c:.3e}  largest share of the bound used {float((err / tol)[normal].max()):.3f} "
          f"in the normal range, {float((err / tol).max()):.3f} anywhere")
    bad = ~(err <= tol)
    assert not bad.any(), (cid, int(bad.sum()), got[bad][:4], ref[bad][:4])
    assert unchanged()
    if d.size >= 7:        # rbf_distances: the special values in front
        flat = got.reshape(-1, count)
        assert flat[0, 1] == 1.0 and flat[1, count - 1] == 1.0 and flat[6, 0] == 1.0      # exact centres
        assert (flat[2] > 0).any() and (flat[3] > 0).any()                                  # d = 0, d < 0: no mask
        assert not flat[5].any()                                                            # d = 10: underflow to 0


def test_rbf_expansion_refuses_a_count_that_is_no_multiple_of_4(gpu_device):
    import nmrgnn_amd
    with pytest.raises(ValueError, match="multiple of 4"):
        nmrgnn_amd.RBFExpansion(R.RBF_LOW, R.RBF_HIGH, R.RBF_BAD_COUNT)(np.array([0.1, 0.2]))


# ---------------------------------------------------------------------------------------------------------- MPLayer
def graph_arguments(g, inv2d, nl_tensor):
    import torch
    nlist = torch.from_numpy(g["nlist"].astype(np.int32)) if nl_tensor else g["nlist"].copy()
    inv = g["inv"].reshape(-1, 1).copy() if inv2d else g["inv"].copy()
    args = [g["nodes"].copy(), nlist, g["edges"].copy(), inv]

    def unchanged():
        nl = args[1].numpy() if nl_tensor else args[1]
        return (np.array_equal(args[0], g["nodes"]) and np.array_equal(nl, g["nlist"]) and
                nl.dtype == (np.int32 if nl_tensor else np.int64) and np.array_equal(args[2], g["edges"]) and
                np.array_equal(args[3].reshape(-1), g["inv"]))
    return args, unchanged


@pytest.mark.parametrize("case", R.MP_CASES, ids=[c["id"] for c in R.MP_CASES])
def test_mplayer(gpu_device, case):
    """one MPLayer call, per element against the oracle's literal einsum over the layer's own Glorot weights"""
    import nmrgnn_amd
    g = R.graph_of(case)
    args, unchanged = graph_arguments(g, case["inv2d"], case["nl_tensor"])
    layer = seeded(nmrgnn_amd.MPLayer(activation=case["act"]), case["id"])
    out = layer(args, residual=case["residual"])
    F, E = case["F"], case["E"]
    assert is_f32_on_device(out, g["nodes"].shape) and is_f32_on_device(layer.w, (F, F, E))
    ref, mag = R.mp_reference(g, host(layer.w), case["act"], case["residual"])
    worst = R.check(case["id"], host(out), ref, mag)
    print(f"[layer-classes] mplayer {case['id']}: max err / max mag {worst:.3e}")
    assert unchanged()


def test_mplayer_refuses_a_contraction_that_is_no_multiple_of_8(gpu_device):
    import nmrgnn_amd
    from nmrgnn_amd import _lib
    F, E = R.MP_REFUSED
    g = R.ragged_graph(F, E, 5, seed=5)
    with pytest.raises(_lib.NGError, match=r"\(E\*F\) % 8"):
        nmrgnn_amd.MPLayer()([g["nodes"], g["nlist"], g["edges"], g["inv"]])


# ---------------------------------------------------------------------------------------------------------- MPBlock
@pytest.mark.parametrize("cid,L,F,E,act,graph,K", R.MPBLOCK_CASES, ids=[c[0] for c in R.MPBLOCK_CASES])
def test_mpblock(gpu_device, cid, L, F, E, act, graph, K):
    """mp_layers x (MPLayer + residual) against mp_block over the weights of block.mp"""
    import nmrgnn_amd
    g = R.graph_of(dict(graph=graph, F=F, E=E, K=K))
    args, unchanged = graph_arguments(g, False, False)
    blk = seeded(nmrgnn_amd.MPBlock(_hp(mp_layers=L, mp_activation=act)), cid)
    out = blk(args)
    assert is_f32_on_device(out, g["nodes"].shape) and len(blk.mp) == L
    ws = [host(layer.w) for layer in blk.mp]
    assert all(w.shape == (F, F, E) for w in ws)
    ref, a32 = R.anchor(R.mp_block_reference, g, ws, act)
    block_bound("mpblock " + cid, host(out), ref, a32)
    assert unchanged()


# ---------------------------------------------------------------------------------------------------------- EdgeFCBlock
@pytest.mark.parametrize("cid,lead,D,H,E,Le,act", R.EDGE_CASES, ids=[c[0] for c in R.EDGE_CASES])
def test_edge_fc_block(gpu_device, cid, lead, D, H, E, Le, act):
    """(Le - 1) x Dense(H, act) + Dense(E) on any leading shape; with two layers, each _dense call on its own per element"""
    import torch
    import nmrgnn_amd
    x = R.stack_input(cid, tuple(lead) + (D,))
    arg = x.copy()
    blk = seeded(nmrgnn_amd.EdgeFCBlock(_hp(edge_hidden_size=H, edge_feature_size=E, edge_fc_layers=Le, fc_activation=act)), cid)
    assert is_f32_on_device(blk(arg), tuple(lead) + (E,))                        # builds
    dims = R.edge_dims(D, H, E, Le)
    Ws, bs = set_biases(blk, dims, gpu_device)
    out = blk(arg)
    assert is_f32_on_device(out, tuple(lead) + (E,))
    ref, a32 = R.anchor(R.edge_block_reference, x, Ws, bs, act)
    block_bound("edge " + cid, host(out), ref, a32)
    assert np.array_equal(arg, x)
    if Le == 2:
        hidden = R.edge_hidden_reference(x, Ws, bs, act)
        for i, layer_act in enumerate((act, None)):
            xin = R.f32(hidden[i]).reshape(-1, dims[i])
            y = blk._dense(torch.from_numpy(xin).to(gpu_device), *blk.weights[i], layer_act, False, gpu_device)
            assert is_f32_on_device(y, (xin.shape[0], dims[i + 1]))
            r, m = R.dense_reference(xin, Ws[i], bs[i], layer_act)
            worst = R.check(f"{cid} dense {i}", host(y), r, m)
            print(f"[layer-classes] edge {cid} dense {i}: max err / max mag {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------- FCBlock
@pytest.mark.parametrize("cid,rows,F,Lf,act", R.FC_CASES, ids=[c[0] for c in R.FC_CASES])
def test_fc_block(gpu_device, cid, rows, F, Lf, act):
    """(Lf - 1) x (Dense(F, act) + residual) + Dense(F // 2, act) at every padding of F and F // 2"""
    import nmrgnn_amd
    x = R.stack_input(cid, (rows, F))
    arg = x.copy()
    blk = seeded(nmrgnn_amd.FCBlock(_hp(atom_feature_size=F, fc_layers=Lf, fc_activation=act)), cid)
    assert is_f32_on_device(blk(arg), (rows, F // 2))                           # builds
    Ws, bs = set_biases(blk, R.fc_dims(F, Lf), gpu_device)
    out = blk(arg)
    assert is_f32_on_device(out, (rows, F // 2))
    ref, a32 = R.anchor(R.fc_block_reference, x, Ws, bs, act)
    block_bound("fc " + cid, host(out), ref, a32)
    assert np.array_equal(arg, x)


def test_fc_block_refuses_another_feature_count(gpu_device):
    import nmrgnn_amd
    blk = nmrgnn_amd.FCBlock(_hp(atom_feature_size=16, fc_layers=2, fc_activation="relu"))
    with pytest.raises(ValueError, match="16"):
        blk(np.ones((5, 12), np.float32))
    blk(np.ones((5, 16), np.float32))
    with pytest.raises(ValueError, match="16"):
        blk(np.ones((5, 20), np.float32))


# ---------------------------------------------------------------------------------------------------------- AMPLayer
@pytest.mark.parametrize("F,E,act", R.AMP_BWD_CASES, ids=[f"F{c[0]}-E{c[1]}-{c[2]}" for c in R.AMP_BWD_CASES])
def test_amplayer_small_widths(gpu_device, F, E, act):
    """_dense and _dense_bwd under padding, through AMPLayer: the forward and all five gradients against the oracle, with the
    bounds test_gpu_layers.py holds the wider AMPLayer cases to"""
    import torch
    import nmrgnn_amd
    from oracle import nmrgnn_oracle as O
    g = R.ragged_graph(F, E, 16, seed=9)
    dout = R.f32(np.random.default_rng([9, F, E]).standard_normal(g["nodes"].shape))
    args, unchanged = graph_arguments(g, False, False)
    layer = seeded(nmrgnn_amd.AMPLayer(activation=act), f"amp-{F}-{E}-{act}")
    out = layer(args)
    assert is_f32_on_device(out, g["nodes"].shape)
    w = [host(t) for t in (layer.wq, layer.wk, layer.wv)]
    assert [a.shape for a in w] == [(F, E), (E, E), (F, F)]
    np.testing.assert_allclose(host(out), O.amp_layer_forward(g["nodes"], g["nlist"], g["edges"], g["inv"], *w, act),
                               rtol=2e-4, atol=2e-5)
    dn, de = layer.backward(dout.copy())
    assert is_f32_on_device(dn, g["nodes"].shape) and is_f32_on_device(de, g["edges"].shape)
    got = dict(nodes=dn, edges=de, **layer.grads)
    ref = O.amp_layer_backward(g["nodes"], g["nlist"], g["edges"], g["inv"], *w, act, dout)
    for name, r in ref.items():
        gv = host(got[name])
        assert gv.shape == r.shape, name
        scale = np.abs(r).max()
        assert np.abs(gv - r).max() <= 2e-5 * max(1.0, scale), (name, np.abs(gv - r).max(), scale)
    dn2, de2 = layer.backward(dout)
    assert torch.equal(dn, dn2) and torch.equal(de, de2)
    assert unchanged()


# ---------------------------------------------------------------------------------------------------------- _glorot
def test_glorot_weights_of_fresh_layers(gpu_device):
    """every |w| within the Keras GlorotUniform limit (float32 rounding of the limit allowed for), the range used (a uniform
    draw of n >= 1024 values stays below 0.9 of the limit with probability 0.9^1024 < 1e-46), the mean within four standard
    deviations of a uniform draw (limit / sqrt(3 n)), and no two layers with the same weights"""
    import torch
    import nmrgnn_amd
    from oracle import nmrgnn_oracle as O
    tensors = []
    for F, E in ((16, 2), (64, 3)):
        g = R.ring_graph(F, E)
        pair = [nmrgnn_amd.MPLayer(), nmrgnn_amd.MPLayer()]
        for layer in pair:
            layer([g["nodes"], g["nlist"], g["edges"], g["inv"]])
        assert not torch.equal(pair[0].w, pair[1].w)
        tensors += [layer.w for layer in pair]
    e = [nmrgnn_amd.EdgeFCBlock(_hp(edge_hidden_size=128, edge_feature_size=3, edge_fc_layers=3, fc_activation="relu"))
         for _ in range(2)]
    f = [nmrgnn_amd.FCBlock(_hp(atom_feature_size=20, fc_layers=2, fc_activation="relu")) for _ in range(2)]
    for blk in e:
        blk(np.ones((5, 2, 2), np.float32))
    for blk in f:
        blk(np.ones((5, 20), np.float32))
    for pair in (e, f):
        for (Wa, _), (Wb, _) in zip(pair[0].weights, pair[1].weights):
            assert Wa.shape == Wb.shape and not torch.equal(Wa, Wb)
        tensors += [W for blk in pair for W, _ in blk.weights]
    a = nmrgnn_amd.AMPLayer()
    g = R.ring_graph(16, 2)
    a([g["nodes"], g["nlist"], g["edges"], g["inv"]])
    tensors += [a.wq, a.wk, a.wv]
    assert {tuple(t.shape) for t in tensors} >= {(16, 16, 2), (64, 64, 3), (2, 128), (128, 128), (128, 3), (20, 20), (20, 10)}
    for t in tensors:
        w = host(t).astype(np.float64)
        lim = float(O.glorot_uniform_limit(tuple(t.shape)))
        assert t.dtype == torch.float32 and np.abs(w).max() <= lim * (1 + 2.0 ** -23), (tuple(t.shape), np.abs(w).max(), lim)
        if w.size >= 1024:
            assert np.abs(w).max() >= 0.9 * lim, (tuple(t.shape), np.abs(w).max(), lim)
        assert abs(w.mean()) <= 4 * lim / np.sqrt(3 * w.size), (tuple(t.shape), w.mean(), lim)


# ---------------------------------------------------------------------------------------------------------- determinism
def test_second_call_gives_the_same_bits(gpu_device):
    """one case of each class called twice with the same inputs"""
    import torch
    import nmrgnn_amd
    g = R.ragged_graph(64, 3, 16, seed=5)
    graph = [g["nodes"], g["nlist"], g["edges"], g["inv"]]
    d = R.rbf_distances(128, (385, 5))
    x = R.stack_input("determinism", (300, 20))
    calls = [(nmrgnn_amd.RBFExpansion(R.RBF_LOW, R.RBF_HIGH, 128), d),
             (nmrgnn_amd.MPLayer(activation="softplus"), graph),
             (nmrgnn_amd.MPBlock(_hp(mp_layers=4, mp_activation="tanh")), graph),
             (nmrgnn_amd.AMPLayer(activation="softplus"), graph),
             (nmrgnn_amd.EdgeFCBlock(_hp(edge_hidden_size=16, edge_feature_size=3, edge_fc_layers=4,
                                         fc_activation="softplus")), x),
             (nmrgnn_amd.FCBlock(_hp(atom_feature_size=20, fc_layers=4, fc_activation="softplus")), x)]
    for layer, arg in calls:
        first = layer(arg).clone()
        assert torch.equal(first, layer(arg)), type(layer).__name__
