"""Cases, inputs, float64 references and bounds for tests/test_gpu_layer_classes.py (the drop-in layer classes of
nmrgnn_amd/layers.py); tests/test_layer_classes_ref_host.py checks this module on the CPU.  NumPy and the float64 oracle
(oracle/nmrgnn_oracle.py) only: nothing here needs a device, and no GPU result enters a bound.

Bounds
  single layer   |got - ref| <= C_REL * mag + 1e-7 * max(mag) per element (mp_layer_ref.check), mag the same expression on
                 absolute values plus the activation's own rounding, as tests/mp_layer_ref.py and tests/test_gpu_dense.py
                 state it (test_gpu_dense's C = 3e-5 max(1, sqrt(n / 1024)) equals C_REL for the contractions n <= 1024 used
                 here).  For one MPLayer call and for one _dense call.
  block          ratio = max|got - ref| / max|ref| over the block's output; a32 = the same ratio of the oracle function
                 evaluated in float32 (numpy, float32 weights and inputs) against float64.  A block passes when its ratio
                 is at most BLOCK_FACTOR * a32 + BLOCK_FLOOR (the margin tests/test_gpu_edge_fused.py gives a
                 split-operand path over an fp32 one).
  RBF            |got - ref| <= c (1 + a) ref + TINY, a the exponent's magnitude (d - mu)^2 / gap (a relative error eps
                 of the exponent is a relative error a eps of the value), c = RBF_FACTOR x the largest
                 |f32 - ref| / ((1 + a) ref) of the numpy float32 evaluation on the same inputs, taken over the results in
                 float32's normal range (a float32 denormal carries fewer bits, and counting its relative error would only
                 widen c); TINY = the smallest normal float32 covers the denormal range, flushed to 0 or not.
"""
import zlib

import numpy as np

from mp_layer_ref import C_REL, check  # noqa: F401  (re-exported: the per-element criterion)
from oracle import nmrgnn_oracle as O

BLOCK_FACTOR, BLOCK_FLOOR = 8.0, 1e-6
RBF_FACTOR = 8.0
TINY = float(np.finfo(np.float32).tiny)
RBF_LOW, RBF_HIGH = 0.005, 0.20


def f32(a):
    return np.asarray(a, np.float32)


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def ratio(got, ref):
    """max|got - ref| / max|ref| (NaN when got holds one)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------- RBFExpansion
# (id, count, shape of d, how the layer is handed d)
RBF_CASES = [("c4-rank1-n1-f64", 4, (1,), "f64"),
             ("c16-rank2-385x5-view", 16, (385, 5), "view"),          # a non-contiguous torch view
             ("c128-rank3-device", 128, (7, 11, 5), "device"),         # a torch tensor already on the device
             ("c132-rank2-385x5-f64", 132, (385, 5), "f64"),
             ("c128-rank1-f32", 128, (40,), "f32"),
             ("c4-rank2-385x5-device", 4, (385, 5), "device")]
RBF_BAD_COUNT = 6


def rbf_distances(count, shape, seed=11):
    """float64 distances: uniform over [-0.05, 0.6] (inside and on both sides of [low, high]; the far end reaches float32's
    denormal range and below at the narrow gaps), and in front: exact centres, 0.0, values outside [low, high], and one so
    large that every result underflows to 0"""
    rng = np.random.default_rng([seed, count] + list(shape))
    centers, _ = O.rbf_centers(RBF_LOW, RBF_HIGH, count)
    d = rng.uniform(-0.05, 0.6, size=int(np.prod(shape)))
    special = [float(centers[1]), float(centers[-1]), 0.0, -0.03, 0.3, 10.0, float(centers[0])]
    d[:min(len(special), d.size)] = special[:d.size]
    return d.reshape(shape)


def rbf_reference(d, count):
    """(ref float64, tol float64, c): d as the layer sees it, i.e. rounded to float32"""
    centers, gap = O.rbf_centers(RBF_LOW, RBF_HIGH, count)
    d32 = f32(d)
    ref = O.rbf_expand(d32, centers, gap)
    v32 = O.rbf_expand(d32, centers, gap, dtype=np.float32)
    assert ref.dtype == np.float64 and v32.dtype == np.float32
    a = (d32.astype(np.float64)[..., None] - centers.astype(np.float64)) ** 2 / float(gap)
    normal = ref >= TINY
    c = RBF_FACTOR * float((np.abs(v32.astype(np.float64) - ref)[normal] / ((1.0 + a) * ref)[normal]).max())
    return ref, c * (1.0 + a) * ref + TINY, c


# ---------------------------------------------------------------------------------------------------------- graphs
def ring_graph(F, E):
    """the 5-atom ring of the reference's layer tests: one-hot rows, both ring neighbours, edges of ones, degree 2"""
    nodes = np.eye(F, dtype=np.float32)[[2, 4, 0, 1, 3]]
    nlist = np.array([[(i - 1) % 5, (i + 1) % 5] for i in range(5)], np.int64)
    return dict(nodes=nodes, nlist=nlist, edges=np.ones((5, 2, E), np.float32), inv=np.full(5, 0.5, np.float32))


def ragged_graph(F, E, K, seed, graphs=5, atoms=77, p_dead=0.1):
    """a batch of `graphs` structures of `atoms` atoms (385 rows: no multiple of any tile), neighbours inside the own
    structure; about a tenth of the slots padded as the reference pads them: nlist = 0 and edges = 0"""
    rng = np.random.default_rng([seed, F, E, K])
    N = graphs * atoms
    base = (np.arange(N) // atoms) * atoms
    nlist = base[:, None] + rng.integers(0, atoms, (N, K))
    live = rng.random((N, K)) >= p_dead
    nlist = np.where(live, nlist, 0).astype(np.int64)
    edges = f32(rng.standard_normal((N, K, E)) * live[:, :, None])
    inv = f32(1.0 / np.maximum(live.sum(1), 1))
    return dict(nodes=f32(0.5 * rng.standard_normal((N, F))), nlist=nlist, edges=edges, inv=inv, live=live)


def graph_of(case):
    if case["graph"] == "ring":
        return ring_graph(case["F"], case["E"])
    return ragged_graph(case["F"], case["E"], case["K"], seed=case.get("seed", 5))


# ---------------------------------------------------------------------------------------------------------- MPLayer
MP_SHAPES = [(16, 2), (32, 1), (64, 3), (128, 8), (256, 3), (20, 2)]
MP_ACTS = [None, "relu", "softplus", "tanh"]
MP_KS = [2, 5, 16, 24]
MP_REFUSED = (20, 3)            # (E F) % 8 != 0


def _mp_cases():
    """every (F, E) with every activation on the ragged batch; residual, K, the form of inv_degree ((N,) / (N, 1)) and of
    nlist (int64 numpy / int32 tensor) rotate so that every (F, E) sees both values of each and all four K; then the ring"""
    cases = []
    for s, (F, E) in enumerate(MP_SHAPES):
        for a, act in enumerate(MP_ACTS):
            cases.append(dict(F=F, E=E, act=act, residual=bool((a + s) % 2), graph="ragged", K=MP_KS[(a + s) % 4],
                              inv2d=bool((a // 2 + s) % 2), nl_tensor=bool((a + s // 2) % 2)))
    for F, E, act, residual in ((16, 2, None, False), (16, 2, "softplus", True), (64, 3, "tanh", True),
                                (20, 2, "relu", False), (256, 3, "softplus", False), (32, 1, "linear", True)):
        cases.append(dict(F=F, E=E, act=act, residual=residual, graph="ring", K=2, inv2d=residual, nl_tensor=not residual))
    for c in cases:
        c["id"] = (f"F{c['F']}-E{c['E']}-{c['act']}-{'res' if c['residual'] else 'nores'}-{c['graph']}-K{c['K']}"
                   f"-inv{'2d' if c['inv2d'] else '1d'}-{'i32t' if c['nl_tensor'] else 'i64'}")
    return cases


MP_CASES = _mp_cases()


def mp_reference(g, w, act, residual):
    """(ref, mag) of one MPLayer call from the oracle's literal einsum"""
    nodes, edges, inv, w = f64(g["nodes"]), f64(g["edges"]), f64(g["inv"]).reshape(-1), f64(w)
    s, _ = O.mp_layer(nodes, g["nlist"], edges, inv, w, act)
    _, mag = O.mp_layer(np.abs(nodes), g["nlist"], np.abs(edges), np.abs(inv), np.abs(w), None)
    if act not in (None, "linear"):
        mag = mag + np.abs(s)                                   # + the activation's own rounding
    return (s + nodes, mag + np.abs(nodes)) if residual else (s, mag)


# ---------------------------------------------------------------------------------------------------------- MPBlock
# (id, mp_layers, F, E, activation, graph, K)
MPBLOCK_CASES = [("L1-F16-E2-softplus-ragged-K5", 1, 16, 2, "softplus", "ragged", 5),
                 ("L4-F16-E2-tanh-ragged-K16", 4, 16, 2, "tanh", "ragged", 16),
                 ("L1-F64-E3-tanh-ragged-K16", 1, 64, 3, "tanh", "ragged", 16),
                 ("L4-F64-E3-softplus-ragged-K24", 4, 64, 3, "softplus", "ragged", 24),
                 ("L4-F16-E2-softplus-ring", 4, 16, 2, "softplus", "ring", 2),
                 ("L4-F64-E3-tanh-ring", 4, 64, 3, "tanh", "ring", 2),
                 ("L4-F16-E2-relu-ragged-K2", 4, 16, 2, "relu", "ragged", 2)]


def mp_block_reference(g, ws, act, dtype=np.float64):
    t = (lambda a: f64(a)) if dtype == np.float64 else (lambda a: f32(a))
    p = {f"mp/{l}/w": t(w) for l, w in enumerate(ws)}
    out = O.mp_block(t(g["nodes"]), g["nlist"], t(g["edges"]), t(g["inv"]).reshape(-1), p,
                     O.hypers(mp_layers=len(ws), mp_activation=act))
    assert out.dtype == dtype
    return out


# ---------------------------------------------------------------------------------------------------------- dense stacks
# (id, leading shape, D, edge_hidden_size, edge_feature_size, edge_fc_layers, fc_activation)
EDGE_CASES = [("ref-5x2-D2-H128-E3-L4-softplus", (5, 2), 2, 128, 3, 4, "softplus"),      # the reference's own test
              ("n7-D2-H16-E1-L2-relu", (7,), 2, 16, 1, 2, "relu"),
              ("31x5-D16-H16-E2-L2-softplus", (31, 5), 16, 16, 2, 2, "softplus"),
              ("60x5-D20-H128-E8-L6-relu", (60, 5), 20, 128, 8, 6, "relu"),              # 300 rows
              ("16x16-D128-H128-E64-L4-softplus", (16, 16), 128, 128, 64, 4, "softplus"),  # exactly 256 rows
              ("5x2-D20-H16-E3-L2-relu", (5, 2), 20, 16, 3, 2, "relu"),
              ("n255-D128-H16-E2-L6-softplus", (255,), 128, 16, 2, 6, "softplus"),
              ("n1-D16-H128-E1-L4-relu", (1,), 16, 128, 1, 4, "relu"),
              ("77x3-D2-H128-E64-L2-softplus", (77, 3), 2, 128, 64, 2, "softplus"),
              ("33x8-D128-H128-E3-L2-relu", (33, 8), 128, 128, 3, 2, "relu"),            # 264 rows
              ("n300-D16-H16-E8-L4-softplus", (300,), 16, 16, 8, 4, "softplus")]

# (id, rows, atom_feature_size, fc_layers, fc_activation)
FC_CASES = [("F6-L4-softplus-r5", 5, 6, 4, "softplus"),
            ("F6-L2-relu-r300", 300, 6, 2, "relu"),
            ("F12-L2-relu-r255", 255, 12, 2, "relu"),
            ("F12-L4-softplus-r5", 5, 12, 4, "softplus"),
            ("F16-L4-softplus-r5", 5, 16, 4, "softplus"),                                # the reference's own test
            ("F20-L6-relu-r300", 300, 20, 6, "relu"),
            ("F20-L2-softplus-r1", 1, 20, 2, "softplus"),
            ("F32-L2-relu-r300", 300, 32, 2, "relu"),
            ("F64-L4-softplus-r255", 255, 64, 4, "softplus"),
            ("F100-L4-relu-r5", 5, 100, 4, "relu"),
            ("F100-L2-softplus-r300", 300, 100, 2, "softplus"),
            ("F256-L4-softplus-r300", 300, 256, 4, "softplus"),
            ("F256-L6-relu-r1", 1, 256, 6, "relu")]
FC_RESIDUAL_DEFECT = (12, 20, 100)      # F % 8 in 1..4: the widths whose residual _dense used to drop


def edge_dims(D, H, E, Le):
    return [D] + [H] * (Le - 1) + [E]


def fc_dims(F, Lf):
    return [F] * Lf + [F // 2]


def stack_input(cid, shape, seed=21):
    rng = np.random.default_rng([seed, zlib.crc32(cid.encode())] + list(shape))
    return f32(rng.standard_normal(shape))


def stack_biases(dims, seed=22):
    """non-zero biases (the Keras zeros hide every bias-padding error): 0.1 x a normal draw"""
    rng = np.random.default_rng([seed] + list(dims))
    return [f32(0.1 * rng.standard_normal(n)) for n in dims[1:]]


def host_glorot(dims, seed=23):
    """stand-ins for a built stack's kernels where no device is at hand (the host tests)"""
    rng = np.random.default_rng([seed] + list(dims))
    return [f32(rng.uniform(-1, 1, (a, b)) * O.glorot_uniform_limit((a, b))) for a, b in zip(dims[:-1], dims[1:])]


def _stack_params(prefix, Ws, bs, t):
    p = {}
    for i, (W, b) in enumerate(zip(Ws, bs)):
        p[f"{prefix}/{i}/kernel"], p[f"{prefix}/{i}/bias"] = t(W), t(b)
    return p


def _cast(dtype):
    return f64 if dtype == np.float64 else f32


def edge_block_reference(x, Ws, bs, act, dtype=np.float64):
    t = _cast(dtype)
    out, _ = O.edge_fc_block(t(x), _stack_params("edge_fc", Ws, bs, t), O.hypers(edge_fc_layers=len(Ws), fc_activation=act))
    assert out.dtype == dtype
    return out


def fc_block_reference(x, Ws, bs, act, dtype=np.float64):
    t = _cast(dtype)
    out = O.fc_block(t(x), _stack_params("fc", Ws, bs, t), O.hypers(fc_layers=len(Ws), fc_activation=act))
    assert out.dtype == dtype
    return out


def anchor(fn, *args):
    """(ref float64, a32): fn(*args, dtype=...) in both precisions"""
    ref = fn(*args, dtype=np.float64)
    return ref, ratio(fn(*args, dtype=np.float32), ref)


def dense_reference(x, W, b, act):
    """(ref, mag) of one Dense layer act(x W + b), float64"""
    x, W, b = f64(x), f64(W), f64(b)
    ref = O._act(act)(O.dense(x, W, b))
    mag = np.abs(x) @ np.abs(W) + np.abs(b) + (np.abs(ref) if act is not None else 0.0)
    return ref, mag


def edge_hidden_reference(x, Ws, bs, act):
    """float64 inputs of every layer of an edge stack (the oracle's own list of activations)"""
    _, acts = O.edge_fc_block(f64(x), _stack_params("edge_fc", Ws, bs, f64), O.hypers(edge_fc_layers=len(Ws), fc_activation=act))
    return acts


# ---------------------------------------------------------------------------------------------------------- AMPLayer
# _dense_bwd through AMPLayer.backward: (F, E, activation); F = 12 pads the contraction only (16 x 12), F = 6 both (8 x 8)
AMP_BWD_CASES = [(12, 3, "softplus"), (6, 2, "tanh"), (12, 2, "relu"), (6, 3, "linear")]
