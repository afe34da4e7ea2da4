"""tests/edge_mlp_ref.py checked on the CPU: the float64 statement that test_gpu_edge_fused.py holds the fused edge-MLP kernels to.

Forward: against oracle/nmrgnn_oracle.py's rbf_expand + edge_fc_block.  Backward: dW, db against central differences in float64 of
L = sum(de * e).  The magnitudes dominate their values.  For every normal case of the GPU file (256 compute units assumed for the
sizes that follow the device): r32 of the plain float32 evaluation, held against C_EDGE (8 * r32 <= C_EDGE), and the two anchors of
the statistic, a factor 16 apart wherever the GPU test uses them.  For every exact case: the float64 statement is made of float32
numbers which a float32 evaluation reaches in two edge orders, every sum of |terms| stays below 2^24 granules, the pre-activations
avoid the interval where softplus rounds, and every operand of a split product fits two fp16 pieces."""
import functools

import numpy as np
import pytest

import edge_mlp_ref as R
from edge_mlp_ref import C_EDGE, H, STAT_MIN, f32
from oracle import nmrgnn_oracle as O
from test_gpu_edge_fused import (EXACT_BWD, EXACT_FWD, HOST_CU, LIVE_BWD, LIVE_FWD, LIVE_N, LIVE_P, NORMAL_BWD, NORMAL_FWD,
                                 RANGE_ROWS, _overflow_case, bwd_reference, fwd_reference, rows_of)

FP16_MAX = 65504.0


def _args(c):
    return c["d_src"], c["d_eff"], c["centers"], c["gap"], c["Ws"], c["bs"]


def test_forward_equals_the_oracle_chain():
    c = R.normal_case(60, 3, seed=3)
    v, mg = R.ref_forward(*_args(c))
    m = (c["d_src"] > 0).astype(np.float64)[:, None]
    assert 0 < m.sum() < 60 and (c["d_eff"][m[:, 0] > 0] < 0).any() and (c["d_eff"] > c["centers"][-1]).any()
    p = {}
    for t in range(4):
        p[f"edge_fc/{t}/kernel"], p[f"edge_fc/{t}/bias"] = c["Ws"][t], c["bs"][t]
    out, acts = O.edge_fc_block(O.rbf_expand(c["d_eff"], c["centers"], c["gap"]) * m, p,
                                {"fc_activation": "softplus", "edge_fc_layers": 4})
    assert np.abs(v["e"] - m * out).max() <= 1e-13 * np.abs(out).max()
    for l in range(3):
        assert np.abs(v["z"][l] - acts[l + 1]).max() <= 1e-13 * np.abs(acts[l + 1]).max()
    for (k, a), (_, b) in zip(R.tensors(v), R.tensors(mg)):
        assert (b >= np.abs(a) * (1 - 1e-12)).all(), k
    assert not np.signbit(v["e"][m[:, 0] == 0]).any()


def test_backward_equals_central_differences():
    c = R.normal_case(24, 2, seed=11, p_dead=0.2)
    v, _ = R.ref_forward(*_args(c))
    zs32 = [f32(z) for z in v["z"]]
    g, mg = R.ref_backward(c["d_src"], c["d_eff"], c["centers"], c["gap"], c["Ws"], zs32, c["de"])
    for (k, a), (_, b) in zip(R.tensors(g), R.tensors(mg)):
        assert (b >= np.abs(a) * (1 - 1e-12)).all(), k

    def loss(Ws, bs):
        return float(np.sum(c["de"] * R.ref_forward(c["d_src"], c["d_eff"], c["centers"], c["gap"], Ws, bs)[0]["e"]))

    rng = np.random.default_rng(5)
    eps = 1e-6
    for l in range(4):
        for name, arrs, got in (("dW", c["Ws"], g["dW"][l]), ("db", c["bs"], g["db"][l])):
            for k in rng.choice(arrs[l].size, min(arrs[l].size, 25), replace=False):
                Ws, bs = [w.copy() for w in c["Ws"]], [b.copy() for b in c["bs"]]
                tgt = (Ws if name == "dW" else bs)[l].reshape(-1)
                tgt[k] += eps
                up = loss(Ws, bs)
                tgt[k] -= 2 * eps
                fd = (up - loss(Ws, bs)) / (2 * eps)
                # the tape is rounded to float32 (2^-24 relative); the differences are good to ~1e-9
                assert abs(got.reshape(-1)[k] - fd) <= 2e-6 * max(1.0, abs(fd)), (name, l, int(k), got.reshape(-1)[k], fd)


def test_tape_layouts_are_inverse_and_follow_the_header():
    """ng_edge_tape_layout (include/nmrgnn_hip.h): edge r, feature 32 bo + 8 q + 4 hf + j of a full group of 32 -> float
    ((bo 4 + q) 64 + hf 32 + r) 4 + j of the group's 4096; a last partial group row-major"""
    n = 77
    rows = np.arange(n * H, dtype=np.float32).reshape(n, H)
    blk = R.rows_to_tape(rows, 1)
    assert np.array_equal(R.tape_to_rows(blk, n, 1), rows) and np.array_equal(R.rows_to_tape(rows, 0), rows.reshape(-1))
    for gr, col in ((0, 0), (5, 37), (31, 127), (40, 64), (63, 3), (64, 0), (76, 127)):
        bo, q, hf, j, r = col // 32, (col // 8) % 4, (col // 4) % 2, col % 4, gr % 32
        at = (gr // 32) * 4096 + ((bo * 4 + q) * 64 + hf * 32 + r) * 4 + j if gr < 64 else gr * H + col
        assert blk[at] == rows[gr, col], (gr, col)


def _report(kind, n, E, st):
    for k, (r32, r32s, r_drop) in st.items():
        print(f"R32 {kind} n {n:6d} E {E} {k:4s} r32 {r32:.3e} r32s {r32s:.3e} r_drop {r_drop:.3e}")


def _hold_constants(st, split_keys):
    for k, (r32, r32s, r_drop) in st.items():
        assert 8.0 * r32 <= C_EDGE, (k, r32)
        if k in split_keys:
            assert r32s > 0 and r_drop >= 16.0 * r32s, (k, r32s, r_drop)


@pytest.mark.parametrize("n,E", NORMAL_FWD, ids=str)
def test_float32_scale_of_every_normal_forward_case(n, E):
    n = rows_of(n, HOST_CU)
    _, v, _, st = fwd_reference("normal", n, E)
    _report("fwd", n, E, st)
    _hold_constants(st, [k for k, a in R.tensors(v) if a.size >= STAT_MIN])


@pytest.mark.parametrize("n,E", NORMAL_BWD, ids=str)
def test_float32_scale_of_every_normal_backward_case(n, E):
    n = rows_of(n, HOST_CU)
    _, v, _, st = bwd_reference("normal", n, E)
    _report("bwd", n, E, st)
    _hold_constants(st, ["dW0", "dW1", "dW2"])


@pytest.mark.parametrize("p_dead", LIVE_P)
def test_float32_scale_of_the_live_view_cases(p_dead):
    for E in sorted({v[0] for v in LIVE_FWD.values()}):
        st = fwd_reference("normal", LIVE_N, E, p_dead)[3]
        _report("live", LIVE_N, E, st)
        _hold_constants(st, [])
    for E in sorted({v[0] for v in LIVE_BWD.values()}):
        st = bwd_reference("normal", LIVE_N, E, p_dead)[3]
        _report("live", LIVE_N, E, st)
        _hold_constants(st, [])


@pytest.mark.parametrize("E,env", RANGE_ROWS, ids=["E8", "E3"])
def test_float32_scale_of_the_range_fallback_row(E, env):
    d_src, centers, gap, Ws, bs = _overflow_case(1000, E)
    c = dict(d_src=f32(d_src), d_eff=f32(d_src), centers=f32(centers), gap=float(np.float32(gap)), Ws=[f32(w) for w in Ws],
             bs=[f32(b) for b in bs])
    v, mg = R.ref_forward(*_args(c))
    st = R.forward_stats(c, v, mg)
    _report("range", 1000, E, st)
    _hold_constants(st, [])


# ------------------------------------------------------------------------------------------------------------------ exact family
def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), b)


def _is_f32(a):
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


def _pieces_ok(x):
    return bool((np.abs(x) < FP16_MAX).all() and R.two_piece(x).all())


@functools.lru_cache(maxsize=2)
def _exact_hidden_checked(n):
    """the hidden layers of the exact forward case of n rows, checked once for every E"""
    c, v, _, _ = fwd_reference("exact", n, 1)
    a = (c["d_src"], c["d_eff"], c["centers"], c["gap"], c["Ws"], c["bs"])
    order = np.random.default_rng(n).permutation(n)
    z32, z32p = R.f32_hidden(*a), R.f32_hidden(*a, order=order)
    Rm, _, _ = R.rbf(c["d_src"], c["d_eff"], c["centers"], c["gap"])
    assert ((Rm == 0) | (Rm == 1)).all() and (Rm.sum(1) == (c["d_src"] > 0)).all()
    x = Rm
    for l in range(3):
        W, b = c["Ws"][l], c["bs"][l]
        pre = x @ W + b
        assert not ((pre > -746.0) & (pre < 40.0)).any(), l          # outside (-128, 40), and float64's softplus exact as well
        z = v["z"][l]
        assert _is_f32(z) and _same(z32[l], z) and _same(z32p[l], z), l
        top = (np.abs(x) @ np.abs(W) + np.abs(b)).max()
        gran = min(R.granule(x) * R.granule(W), R.granule(b))
        assert top / gran < 2.0 ** 24, (l, top, gran)
        assert _pieces_ok(256.0 * W) and _pieces_ok(z), l
        x = z
    assert 0 < (v["z"][2] > 0).mean() < 1
    for l in (1, 2):            # the small fp16 piece of the activations is in play (layer 2 and the output layer)
        assert (v["z"][l].astype(np.float16).astype(np.float64) != v["z"][l]).any(), l
    return z32p[2]


@pytest.mark.parametrize("n,E", EXACT_FWD, ids=str)
def test_exact_forward_family_is_exact_in_float32(n, E):
    n = rows_of(n, HOST_CU)
    z3p = _exact_hidden_checked(n)
    c, v, _, _ = fwd_reference("exact", n, E)
    Wo, bo, z3 = c["Ws"][3], c["bs"][3], v["z"][2]
    assert _is_f32(v["e"])
    assert _same(R.f32_output(c["d_src"], z3, Wo, bo), v["e"]) and _same(R.f32_output(c["d_src"], z3p, Wo, bo), v["e"])
    top = (np.abs(z3) @ np.abs(Wo) + np.abs(bo)).max()
    gran = min(R.granule(z3) * R.granule(Wo), R.granule(bo))
    assert top / gran < 2.0 ** 24, (top, gran)
    assert _pieces_ok(256.0 * Wo)
    assert not np.signbit(v["e"][c["d_src"] <= 0]).any()


@pytest.mark.parametrize("n,E", EXACT_BWD, ids=str)
def test_exact_backward_family_is_exact_in_float32(n, E):
    n = rows_of(n, HOST_CU)
    c, v, mg, _ = bwd_reference("exact", n, E)
    a = (c["d_src"], c["d_eff"], c["centers"], c["gap"], c["Ws"], c["zs32"], c["de"])
    g32, g32p = R.f32_backward(*a), R.f32_backward(*a, order=np.random.default_rng(n).permutation(n))
    Rm, _, _ = R.rbf(c["d_src"], c["d_eff"], c["centers"], c["gap"])
    xs = [Rm] + c["zs32"]
    for z in c["zs32"]:
        assert ((z == 0) | (z >= 40)).all() and _pieces_ok(z)
    S = R.grad_scale(c["Ws"], c["de"])
    for l in range(3):
        G = v["G"][l]
        assert _pieces_ok(S * G), (l, S)
        if l:       # dZ_l = G_{l+1} W_{l+1}^T on the matrix pipe: sums of |terms| in granules, and the W^T pieces
            top = (np.abs(G) @ np.abs(c["Ws"][l]).T).max()
            assert top / (R.granule(G) * R.granule(c["Ws"][l])) < 2.0 ** 24, l
            assert _pieces_ok(256.0 * c["Ws"][l]), l
    dE = c["de"] * (c["d_src"] > 0)[:, None]
    for l in range(4):
        gG = R.granule(v["G"][l] if l < 3 else dE)
        for key, term_gran in (("dW", R.granule(xs[l]) * gG), ("db", gG)):
            ref = v[key][l]
            assert _is_f32(ref) and _same(g32[key][l], ref) and _same(g32p[key][l], ref), (key, l)
            assert mg[key][l].max() / term_gran < 2.0 ** 24, (key, l, mg[key][l].max(), term_gran)
    if n >= 63:
        assert all(np.abs(v["dW"][l]).max() > 0 for l in range(4))
