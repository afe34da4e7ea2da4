"""tests/layer_classes_ref.py and the shape check of nmrgnn_amd/layers.py on the CPU: what test_gpu_layer_classes.py relies on
that needs no device.

  check_built_shapes   the pure function that MPLayer, AMPLayer and EdgeFCBlock call before anything touches the GPU: equal shapes
                       pass, any other raises ValueError naming both; the three classes raise it for a built layer (also one whose
                       weights were set by hand) BEFORE the device is looked up, so a mismatched call never reaches a kernel
  case builders        every value the cases are meant to cover appears; the generators are seeded; padded slots are nlist = 0,
                       edges = 0
  references           mp_reference equals the oracle's aggregate-then-GEMM order, magnitudes dominate values, the float32 anchors
                       are finite and non-zero for every block case, the RBF factor c likewise; a dropped residual, a dropped bias
                       and a bias shifted by one column all sit orders of magnitude outside the block bound"""
import numpy as np
import pytest

import layer_classes_ref as R
from oracle import nmrgnn_oracle as O


# ---------------------------------------------------------------------------------------------------------- shape check
def test_check_built_shapes():
    from nmrgnn_amd.layers import check_built_shapes
    check_built_shapes("l", [("w", (16, 16, 2))], [("w", (16, 16, 2))])
    check_built_shapes("l", [("w", [16, 16, 2])], [("w", (16, 16, 2))])                # any sequence of ints
    check_built_shapes("l", [("k", (2, 128))], [("k", (2, None))])                     # None leaves a dimension open
    amp = [("wq", (20, 5)), ("wk", (5, 5)), ("wv", (20, 20))]
    check_built_shapes("l", amp, list(amp))
    for built, wanted, words in (
            ([("w", (16, 16, 2))], [("w", (32, 32, 2))], ["(16, 16, 2)", "(32, 32, 2)"]),
            ([("w", (16, 16, 2))], [("w", (16, 16, 3))], ["(16, 16, 2)", "(16, 16, 3)"]),
            ([("w", (16, 16))], [("w", (16, 16, 1))], ["(16, 16)", "(16, 16, 1)"]),
            ([("k", (2, 128))], [("k", (16, None))], ["(2, 128)", "(16, None)"]),
            (amp, [("wq", (20, 4)), ("wk", (4, 4)), ("wv", (20, 20))], ["(20, 5)", "(20, 4)", "'wq'"]),
            (amp, [("wq", (20, 5)), ("wk", (5, 5)), ("wv", (24, 24))], ["(20, 20)", "(24, 24)", "'wv'"])):
        with pytest.raises(ValueError) as err:
            check_built_shapes("some-layer", built, wanted)
        assert all(w in str(err.value) for w in words + ["some-layer"]), str(err.value)


class _Shaped:
    """stands for a weight tensor: the check reads nothing but its shape"""

    def __init__(self, *shape):
        self.shape = shape


def _ring(F, E):
    g = R.ring_graph(F, E)
    return [g["nodes"], g["nlist"], g["edges"], g["inv"]]


def test_layers_check_shapes_before_they_look_for_a_device(monkeypatch):
    """a built layer called with inputs of another (F, E) or D raises ValueError, and the device is never asked for"""
    from nmrgnn_amd import layers

    def no_device():
        raise AssertionError("the shape check must come before the device")
    monkeypatch.setattr(layers, "_device", no_device)
    mp = layers.MPLayer()
    mp.w, mp.built = _Shaped(16, 16, 2), True                   # as after a first call, or a w set by hand
    amp = layers.AMPLayer()
    amp.wq, amp.wk, amp.wv, amp.built = _Shaped(16, 2), _Shaped(2, 2), _Shaped(16, 16), True
    for layer in (mp, amp):
        for F, E in ((32, 2), (16, 3), (20, 2)):
            with pytest.raises(ValueError, match=r"\(16, "):
                layer(_ring(F, E))
        with pytest.raises(AssertionError, match="before the device"):      # equal shapes pass the check
            layer(_ring(16, 2))
    mp.w = _Shaped(32, 32, 2)                                   # a hand-set w of another size than the inputs
    with pytest.raises(ValueError, match=r"\(32, 32, 2\).*\(16, 16, 2\)"):
        mp(_ring(16, 2))
    blk = layers.EdgeFCBlock({"edge_hidden_size": 128, "edge_feature_size": 3, "edge_fc_layers": 2, "fc_activation": "relu"})
    blk.weights, blk.built = [(_Shaped(2, 128), _Shaped(128)), (_Shaped(128, 3), _Shaped(3))], True
    for D in (16, 3, 128):
        with pytest.raises(ValueError, match=r"\(2, 128\)"):
            blk(np.ones((5, 2, D), np.float32))
    with pytest.raises(AssertionError, match="before the device"):
        blk(np.ones((5, 2, 2), np.float32))


def test_dense_refuses_a_residual_between_different_widths_before_the_device():
    from nmrgnn_amd import layers
    blk = layers.FCBlock({"atom_feature_size": 16, "fc_layers": 2, "fc_activation": "relu"})
    with pytest.raises(ValueError, match="residual"):
        blk._dense(_Shaped(5, 16), _Shaped(16, 8), _Shaped(8), "relu", True, None)


# ---------------------------------------------------------------------------------------------------------- case builders
def test_cases_cover_what_they_are_meant_to():
    assert {c[1] for c in R.RBF_CASES} == {4, 16, 128, 132} and R.RBF_BAD_COUNT % 4
    assert {len(c[2]) for c in R.RBF_CASES} == {1, 2, 3} and {c[3] for c in R.RBF_CASES} >= {"f64", "view", "device"}
    assert (1,) in {c[2] for c in R.RBF_CASES} and (385, 5) in {c[2] for c in R.RBF_CASES}
    for F, E in R.MP_SHAPES:
        mine = [c for c in R.MP_CASES if (c["F"], c["E"]) == (F, E) and c["graph"] == "ragged"]
        assert {c["act"] for c in mine} == {None, "relu", "softplus", "tanh"} and (E * F) % 8 == 0
        assert {c["residual"] for c in mine} == {False, True} and {c["K"] for c in mine} == {2, 5, 16, 24}
        assert {c["inv2d"] for c in mine} == {False, True} and {c["nl_tensor"] for c in mine} == {False, True}
    assert any(c["graph"] == "ring" for c in R.MP_CASES) and any(c["act"] == "linear" for c in R.MP_CASES)
    assert (R.MP_REFUSED[0] * R.MP_REFUSED[1]) % 8
    assert len({c["id"] for c in R.MP_CASES}) == len(R.MP_CASES)
    assert {(c[1], c[2], c[3]) for c in R.MPBLOCK_CASES} >= {(1, 16, 2), (4, 16, 2), (1, 64, 3), (4, 64, 3)}
    assert {c[4] for c in R.MPBLOCK_CASES} == {"softplus", "tanh", "relu"}
    e = R.EDGE_CASES
    assert 10 <= len(e) <= 15
    assert {c[2] for c in e} == {2, 16, 20, 128} and {c[4] for c in e} == {1, 2, 3, 8, 64} and {c[3] for c in e} == {16, 128}
    assert {c[5] for c in e} == {2, 4, 6} and {c[6] for c in e} == {"relu", "softplus"}
    assert (5, 2) in {c[1] for c in e} and {len(c[1]) for c in e} == {1, 2}
    rows = sorted(int(np.prod(c[1])) for c in e)
    assert 256 in rows and 300 in rows and sum(r < 256 for r in rows) > len(rows) // 2
    f = R.FC_CASES
    assert {c[2] for c in f} == {6, 12, 16, 20, 32, 64, 100, 256} and {c[3] for c in f} == {2, 4, 6}
    assert {c[4] for c in f} == {"relu", "softplus"} and {c[1] for c in f} == {1, 5, 255, 300}
    assert all(F % 8 in (1, 2, 3, 4) for F in R.FC_RESIDUAL_DEFECT)
    assert {c[0] for c in R.AMP_BWD_CASES} == {12, 6}
    assert {c[2] for c in R.AMP_BWD_CASES} == {"softplus", "tanh", "relu", "linear"}


def test_generators_are_seeded_and_pad_like_the_reference():
    a, b = R.ragged_graph(20, 2, 5, seed=5), R.ragged_graph(20, 2, 5, seed=5)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["nodes"].shape == (385, 20) and a["nlist"].dtype == np.int64 and a["edges"].dtype == np.float32
    dead = ~a["live"]
    assert 0.05 < dead.mean() < 0.15
    assert not a["nlist"][dead].any() and not a["edges"][dead].any() and a["edges"][a["live"]].all()
    own = np.arange(385)[:, None] // 77
    assert (a["nlist"][a["live"]] // 77 == np.broadcast_to(own, a["live"].shape)[a["live"]]).all()
    assert np.array_equal(a["inv"], R.f32(1.0 / np.maximum(a["live"].sum(1), 1)))
    r = R.ring_graph(16, 2)
    assert np.array_equal(r["nlist"], [[4, 1], [0, 2], [1, 3], [2, 4], [3, 0]]) and r["nodes"].sum() == 5
    assert np.array_equal(R.stack_input("x", (3, 4)), R.stack_input("x", (3, 4)))
    assert not np.array_equal(R.stack_input("x", (3, 4)), R.stack_input("y", (3, 4)))
    assert all(b.any() for b in R.stack_biases([6, 6, 3]))
    d = R.rbf_distances(128, (385, 5))
    assert np.array_equal(d, R.rbf_distances(128, (385, 5))) and d.dtype == np.float64
    centers, _ = O.rbf_centers(R.RBF_LOW, R.RBF_HIGH, 128)
    flat = d.reshape(-1)
    assert flat[0] == centers[1] and flat[1] == centers[-1] and flat[2] == 0.0 and flat[3] < R.RBF_LOW and flat[5] == 10.0
    assert (flat > R.RBF_HIGH).any() and (flat < 0).any()


# ---------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("cid,count,shape,kind", R.RBF_CASES, ids=[c[0] for c in R.RBF_CASES])
def test_rbf_bound(cid, count, shape, kind):
    d = R.rbf_distances(count, shape)
    ref, tol, c = R.rbf_reference(d, count)
    assert ref.shape == tuple(shape) + (count,) and np.isfinite(tol).all() and (tol >= R.TINY).all()
    assert 8 * 2.0 ** -26 < c < 8 * 2.0 ** -20, c              # float32's rounding scale, and not zero
    v32 = O.rbf_expand(R.f32(d), *O.rbf_centers(R.RBF_LOW, R.RBF_HIGH, count), dtype=np.float32)
    # the float32 evaluation sits 8x inside (1e-9: the element that sets c meets its share to the last bit)
    assert (np.abs(v32 - ref) <= (tol - R.TINY) / R.RBF_FACTOR * (1 + 1e-9) + R.TINY).all()
    if d.size >= 7:
        assert not ref.reshape(-1, count)[5].any()             # d = 10 underflows in float64 too


def test_rbf_cases_reach_the_denormal_range():
    ref, _, _ = R.rbf_reference(R.rbf_distances(128, (7, 11, 5)), 128)
    assert ((ref > 0) & (ref < R.TINY)).any() and (ref == 0).any() and (ref == 1).any()


def test_mp_reference_is_the_layer():
    g = R.ragged_graph(16, 2, 5, seed=5)
    w = np.random.default_rng(1).uniform(-0.3, 0.3, (16, 16, 2))
    for act in R.MP_ACTS:
        for residual in (False, True):
            ref, mag = R.mp_reference(g, w, act, residual)
            alg, _ = O.mp_layer_alg(R.f64(g["nodes"]), g["nlist"], R.f64(g["edges"]), R.f64(g["inv"]), R.f64(w), act)
            np.testing.assert_allclose(ref, alg + (R.f64(g["nodes"]) if residual else 0.0), rtol=1e-12, atol=1e-14)
            assert (mag >= np.abs(ref) * (1 - 1e-12) - (np.log(2) if act == "softplus" else 0)).all()
    col = R.mp_reference(dict(g, inv=g["inv"].reshape(-1, 1)), w, "tanh", True)
    assert np.array_equal(col[0], R.mp_reference(g, w, "tanh", True)[0])


def test_dense_reference():
    rng = np.random.default_rng(2)
    x, W, b = R.f32(rng.standard_normal((7, 6))), R.f32(rng.standard_normal((6, 3))), R.f32(rng.standard_normal(3))
    ref, mag = R.dense_reference(x, W, b, "relu")
    assert np.array_equal(ref, np.maximum(x.astype(np.float64) @ W.astype(np.float64) + b, 0)) and (mag >= ref).all()
    hidden = R.edge_hidden_reference(x, [W, W.T.copy()], [b, R.f32(np.zeros(6))], "relu")
    assert len(hidden) == 2 and np.array_equal(hidden[1], ref)


def _blocks():
    for cid, lead, D, H, E, Le, act in R.EDGE_CASES:
        dims = R.edge_dims(D, H, E, Le)
        yield "edge " + cid, R.edge_block_reference, R.stack_input(cid, tuple(lead) + (D,)), dims, act
    for cid, rows, F, Lf, act in R.FC_CASES:
        yield "fc " + cid, R.fc_block_reference, R.stack_input(cid, (rows, F)), R.fc_dims(F, Lf), act


def test_block_anchors_are_finite_and_non_zero():
    for name, fn, x, dims, act in _blocks():
        ref, a32 = R.anchor(fn, x, R.host_glorot(dims), R.stack_biases(dims), act)
        assert ref.shape == x.shape[:-1] + (dims[-1],) and np.isfinite(ref).all(), name
        assert 2.0 ** -27 < a32 < 2.0 ** -17, (name, a32)
    for cid, L, F, E, act, graph, K in R.MPBLOCK_CASES:
        g = R.graph_of(dict(graph=graph, F=F, E=E, K=K))
        rng = np.random.default_rng(L)
        ws = [R.f32(rng.uniform(-1, 1, (F, F, E)) * O.glorot_uniform_limit((F, F, E))) for _ in range(L)]
        ref, a32 = R.anchor(R.mp_block_reference, g, ws, act)
        assert ref.shape == g["nodes"].shape and np.isfinite(ref).all()
        assert 2.0 ** -27 < a32 < 2.0 ** -17, (cid, a32)


def test_glue_defects_sit_far_outside_the_block_bound():
    """what the block bound is for: a residual dropped, a bias left out, a bias shifted by one column"""
    for cid, rows, F, Lf, act in R.FC_CASES:
        dims = R.fc_dims(F, Lf)
        x, Ws, bs = R.stack_input(cid, (rows, F)), R.host_glorot(dims), R.stack_biases(dims)
        ref, a32 = R.anchor(R.fc_block_reference, x, Ws, bs, act)
        bound = R.BLOCK_FACTOR * a32 + R.BLOCK_FLOOR
        h = R.f64(x)
        for W, b in zip(Ws, bs):                                 # every layer without its residual
            h = O._act(act)(h @ R.f64(W) + R.f64(b))
        assert R.ratio(h, ref) > 1000 * bound, (cid, R.ratio(h, ref), bound)
        none = R.fc_block_reference(x, Ws, [np.zeros_like(b) for b in bs], act)
        rolled = R.fc_block_reference(x, Ws, [np.roll(b, 1) for b in bs], act)
        assert R.ratio(none, ref) > 1000 * bound and R.ratio(rolled, ref) > 1000 * bound, cid
