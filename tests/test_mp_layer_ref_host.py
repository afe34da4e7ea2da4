"""tests/mp_layer_ref.py checked on the CPU: the float64 statement that the GPU tests of the MPLayer kernels hold them to.

Forward: against oracle/nmrgnn_oracle.py's MPLayer (the literal four-operand einsum of nmrgnn/layers.py:39-40).
Backward: dh, de, dw against central finite differences in float64 of L = sum(dH * (act(P) + h)) — the C ABI's backward always
adds the upstream gradient to dh_in (ng_mp_layer_bwd takes no residual flag), so that is the function ref_layer differentiates
for both values of `residual`.
The two emulations behind the statistical criterion: the float32 evaluation must sit at float32's rounding scale, the
dropped-cross-term evaluation well above it, and the node-side formulas (dh = dH + B Wn, dw = h^T B) must equal ref_layer's.
The exact family (mp_layer_ref.exact_inputs) at every shape test_gpu_mp_default_width.py uses it: the float64 statement is made of
float32 numbers that a float32 evaluation reaches bit for bit, every magnitude stays below 2^24 granules (so does every partial
sum in any order), and the operands of the split products fit two fp16 pieces."""
import numpy as np
import pytest

from mp_layer_ref import (ACT, GRANULE, act_fwd, act_grad_from_out, f32_layer, graph_layout, host_records, incoming, layer_stats,
                          lead_piece, padded_case, ref_layer, rstat, sigbits, sub_case)
from test_gpu_mp_default_width import CASES, EXACT_CASES, big_case, build
from oracle import nmrgnn_oracle as O

ORACLE_ACT = {"none": None, "softplus": "softplus", "relu": "relu", "tanh": "tanh"}


def _ref(c):
    return ref_layer(c["h"], c["nl"], c["e"], c["inv"], c["w"], c["dH"], c["act"], c["residual"])


@pytest.mark.parametrize("residual", [0, 1])
@pytest.mark.parametrize("act", list(ACT))
def test_forward_equals_the_oracle_layer(act, residual):
    c = padded_case(16, 3, 5, 60, 0, act, residual, seed=3)
    v, mg = _ref(c)
    out, P = O.mp_layer(c["h"], c["nl"], c["e"], c["inv"], c["w"], ORACLE_ACT[act])
    want = out + (c["h"] if residual else 0.0)
    assert np.abs(v["s"] - out).max() <= 1e-13 * max(1.0, np.abs(out).max())
    assert np.abs(v["h_out"] - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    assert np.array_equal(v["s_in"], v["s"].astype(np.float32).astype(np.float64))
    A = np.einsum("ijn,ijl->inl", c["e"], c["h"][c["nl"]])
    assert np.abs(v["A"] - A).max() <= 1e-13 * max(1.0, np.abs(A).max())
    # magnitudes dominate the values they belong to
    for k in ("A", "s", "h_out", "dh", "de", "dw"):
        assert (mg[k] >= np.abs(v[k]) * (1 - 1e-12)).all(), k


@pytest.mark.parametrize("residual", [0, 1])
@pytest.mark.parametrize("act", list(ACT))
def test_backward_equals_central_differences(act, residual):
    c = padded_case(8, 2, 4, 24, 0, act, residual, seed=11, p_dead=0.2)
    rng = np.random.default_rng(5)
    # duplicates of one source inside a list, a target nobody points at, and pre-activations away from relu's kink
    c["nl"][3, :] = 7
    c["nl"][c["nl"] == 20] = 21
    v, _ = _ref(c)
    P = c["inv"][:, None] * np.einsum("inl,lmn->im", v["A"], c["w"])
    assert np.abs(P).min() > 1e-5

    def loss(h, e, w):
        A = np.einsum("ijn,ijl->inl", e, h[c["nl"]])
        return float(np.sum(c["dH"] * (act_fwd(c["act"], c["inv"][:, None] * np.einsum("inl,lmn->im", A, w)) + h)))

    eps = 1e-6
    for name, key, arr in (("dh", 0, c["h"]), ("de", 1, c["e"]), ("dw", 2, c["w"])):
        flat = rng.choice(arr.size, min(arr.size, 60), replace=False)
        for k in flat:
            args = [c["h"].copy(), c["e"].copy(), c["w"].copy()]
            args[key].reshape(-1)[k] += eps
            up = loss(*args)
            args[key].reshape(-1)[k] -= 2 * eps
            fd = (up - loss(*args)) / (2 * eps)
            got = v[name].reshape(-1)[k]
            # the slope is taken from s_save rounded to float32 (2^-24 relative); the differences are good to ~1e-9
            assert abs(got - fd) <= 2e-6 * max(1.0, abs(fd)), (name, int(k), got, fd)


def test_node_side_formulas_equal_the_edge_side_ones():
    c = padded_case(64, 3, 8, 500, 0, "tanh", 1, seed=2)
    v, _ = _ref(c)
    N, E, F = c["N"], c["E"], c["F"]
    slope = 1.0 - v["s_in"] ** 2
    B = incoming(c["nl"], c["e"], c["dH"] * slope * c["inv"][:, None]).reshape(N, E * F)
    dh = c["dH"] + B @ c["w"].transpose(2, 1, 0).reshape(E * F, F)
    dw = (c["h"].T @ B).reshape(F, E, F).transpose(0, 2, 1)
    assert np.abs(dh - v["dh"]).max() <= 1e-12 * np.abs(v["dh"]).max()
    assert np.abs(dw - v["dw"]).max() <= 1e-12 * np.abs(v["dw"]).max()


def test_lead_piece_keeps_eleven_bits_of_the_row_maximum():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 192)) * np.exp2(rng.integers(-30, 30, (50, 1)))
    x[7] = 0.0
    p = lead_piece(x)
    assert (p[7] == 0).all()
    assert (np.abs(p - x) <= np.exp2(-11) * np.abs(x) + 1e-300).all()           # half an ulp of an 11-bit significand
    rel = np.abs(p - x)[x != 0] / np.abs(x)[x != 0]
    assert rel.max() > np.exp2(-14)                                               # and it IS a reduction


@pytest.mark.parametrize("act", ["none", "relu"])
def test_the_two_emulations_bracket_a_threshold(act):
    """r32 at float32's rounding scale, r_drop at the scale of a missing fp16 piece (2^-12 of an operand, divided by the square
    root of the contraction length): two decades apart and more, so sqrt(r32 * r_drop) separates them"""
    c = padded_case(64, 3, 16, 3000, 0, act, 1, seed=4)
    v, mg = _ref(c)
    st = layer_stats(c["h"], c["nl"], c["e"], c["inv"], c["w"], c["dH"], c["act"], c["residual"], v, mg, c["live"])
    print({k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in st.items()})
    for k, (r32, r_drop) in st.items():
        assert 0 < r32 < 1e-7, (k, r32)
        assert 1e-6 < r_drop < 1e-4, (k, r_drop)
        assert r_drop > 100 * r32, (k, r32, r_drop)
    assert rstat(v["s"], v["s"], mg["s"]) == 0.0


@pytest.mark.parametrize("name", EXACT_CASES + ["big"])
def test_exact_family_is_exact_in_float32(name):
    """per exact case of test_gpu_mp_default_width.py (256 compute units assumed for the sizes that follow the device; the
    two-tiles case on the graphs it samples): float32 evaluation == float64 bit for bit; A, dP, dA and B within 20 significant
    bits; mag / granule < 2^24 for every output the case compares"""
    if name == "big":
        c, rows = big_case("exact", 256)
        c, keys = sub_case(c, rows), ("dh", "de")
    else:
        c = build(name, "exact", 256)
        keys = ("A", "s", "h_out") + (("dh", "de", "dw") if CASES[name]["bwd"] else ())
    v, mg = _ref(c)
    slope = act_grad_from_out(c["act"], v["s_in"])
    g32 = f32_layer(c["h"], c["nl"], c["e"], c["inv"], c["w"], c["dH"], c["act"], c["residual"], slope)
    for k in keys:
        assert np.array_equal(g32[k].astype(np.float64), v[k]), k
        assert np.array_equal(v[k].astype(np.float32).astype(np.float64), v[k]), k
        top = float(mg[k].max()) + (3.0 if k == "de" else 0.0)                   # de may be added to a prior in {-3..3}
        assert top / GRANULE[k] < 2.0 ** 24, (k, top / GRANULE[k])
    assert sigbits(v["A"]) <= 20
    if "dh" in keys:
        E, Fw = c["E"], c["F"]
        dP = c["dH"] * slope * c["inv"][:, None]
        dA = dP @ c["w"].transpose(2, 0, 1).reshape(E * Fw, Fw).T
        B = incoming(c["nl"], c["e"], dP)
        bits = {"dP": sigbits(dP), "dA": sigbits(dA), "B": sigbits(B)}
        assert max(bits.values()) <= 20, bits


def test_mixed_spans_and_host_records():
    """graph_layout with a list of sizes (the last one repeats); host_records: CSC order, and a permutation that stays inside
    every target's segment"""
    gi, base, size = graph_layout(700, [100, 100, 500])
    assert list(np.unique(base)) == [0, 100, 200] and size[0] == 100 and size[250] == 500 and gi[699] == 2
    _, base, size = graph_layout(1300, [100, 500])
    assert list(np.unique(base)) == [0, 100, 600, 1100] and size[1299] == 200
    c = padded_case(16, 2, 4, 50, [7, 20], "none", 1, seed=1)
    assert c["span"] == 20 and (c["nl"] >= graph_layout(50, [7, 20])[1][:, None]).all()
    ptr, rec = host_records(c)
    src, tgt_sorted = rec[:, 0].view(np.int32), np.repeat(np.arange(50), np.diff(ptr))
    assert len(rec) == int(c["live"].sum()) and (rec[:, 3] == 0).all()
    for a, b in zip(ptr[:-1], ptr[1:]):
        assert (np.diff(src[a:b]) >= 0).all()
    hit = {(int(i), int(t)) for i, t in zip(src, tgt_sorted)}
    assert hit == {(int(i), int(c["nl"][i, j])) for i, j in zip(*np.nonzero(c["live"]))}
    _, rec_p = host_records(c, permute=3)
    assert not np.array_equal(rec_p, rec)
    for a, b in zip(ptr[:-1], ptr[1:]):
        assert sorted(map(tuple, rec_p[a:b].view(np.int32))) == sorted(map(tuple, rec[a:b].view(np.int32)))
