"""tests/fc_block_ref.py checked on the CPU: the float64 statement that test_gpu_fc_block.py holds the FC block kernels to.

Backward: dx, dW_l, db_l against central finite differences in float64 of sum(dg * g(x, W, b)) for all four activations (the
tape handed to ref_bwd is the float64 chain rounded to float32, as the kernels get it: 2^-24 relative in the slopes).
Exact family: float64, a float32 evaluation and the two dropped-piece evaluations all give the same numbers, and the CPU-side
conditions hold at N = 65 and N = 66,000, a size like the GPU test's largest (which takes its row counts from the device and
asserts the conditions again on its own data before it calls the GPU).
Statistic: the float32 evaluation sits at float32's rounding scale, the dropped-piece evaluation more than 4x above it."""
import numpy as np
import pytest

from fc_block_ref import (ACT, bwd_stats, exact_conditions, exact_data, f32, fixed_piece, fwd_stats, normal_data, plain_piece,
                          ref_bwd, ref_fwd, ref_layer_fwd, sig_bits)
from mp_layer_ref import lead_piece


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("act", list(ACT))
def test_backward_equals_central_differences(act, L):
    rng = np.random.default_rng(3)
    N, F = 12, 8
    x, Ws, bs, dg = normal_data(rng, N, F, L)
    a = ACT[act]
    xs, g, mags = ref_fwd(x, Ws, bs, a)
    assert min(np.abs(xs[l] @ Ws[l] + bs[l]).min() for l in range(L)) > 1e-4      # pre-activations away from relu's kink
    (dx, dWs, dbs), (mx, mWs, mbs) = ref_bwd([f32(v) for v in xs], f32(g), Ws, dg, a)
    assert (mx >= np.abs(dx) * (1 - 1e-12)).all()
    for l in range(L):
        assert (mWs[l] >= np.abs(dWs[l]) * (1 - 1e-12)).all() and (mbs[l] >= np.abs(dbs[l]) * (1 - 1e-12)).all()
        assert (mags[l] >= np.abs(xs[l + 1] if l < L - 1 else g) * (1 - 1e-12) - (np.log(2) if a == 1 else 0)).all()

    def loss(x_, Ws_, bs_):
        return float(np.sum(dg * ref_fwd(x_, Ws_, bs_, a)[1]))

    eps = 1e-6
    targets = [("dx", dx, lambda v: (v, Ws, bs), x)]
    for l in range(L):
        targets.append((f"dW{l}", dWs[l], lambda v, l=l: (x, Ws[:l] + [v] + Ws[l + 1:], bs), Ws[l]))
        targets.append((f"db{l}", dbs[l], lambda v, l=l: (x, Ws, bs[:l] + [v] + bs[l + 1:]), bs[l]))
    for name, got, place, arr in targets:
        for k in rng.choice(arr.size, min(arr.size, 24), replace=False):
            up, dn = arr.copy(), arr.copy()
            up.reshape(-1)[k] += eps
            dn.reshape(-1)[k] -= eps
            fd = (loss(*place(up)) - loss(*place(dn))) / (2 * eps)
            assert abs(got.reshape(-1)[k] - fd) <= 2e-6 * max(1.0, abs(fd)), (name, int(k), got.reshape(-1)[k], fd)


def test_one_layer_is_the_chain():
    rng = np.random.default_rng(4)
    x, Ws, bs, _ = normal_data(rng, 40, 16, 3)
    xs, g, mags = ref_fwd(x, Ws, bs, 1)
    v, m = ref_layer_fwd(xs[1], Ws[1], bs[1], 1, False)
    assert np.array_equal(v, xs[2]) and np.array_equal(m, mags[1])
    v, m = ref_layer_fwd(xs[2], Ws[2], bs[2], 1, True)
    assert np.array_equal(v, g) and v.shape == (40, 8)


def test_significant_bits():
    assert sig_bits(np.array([0.0, 3.0, -2048.0, 2047.0])) == 11
    assert sig_bits(np.array([2049.0])) == 12 and sig_bits(np.array([4094.0])) == 11 and sig_bits(np.zeros(3)) == 0


@pytest.mark.parametrize("N", [65, 66000])
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("L", [2, 6])
def test_the_exact_family_is_exact(act, L, N):
    """the conditions of exact_conditions hold, and float32 / dropped-piece evaluations reproduce float64 bit for bit"""
    rng = np.random.default_rng([N, L, ACT[act], 1])
    x, Ws, bs, dg = exact_data(rng, N, 64, L)
    xs, g, dx, dWs, dbs = exact_conditions(x, Ws, bs, dg, ACT[act])
    print("max|x_l|", max(np.abs(v).max() for v in xs), "max|dx|", np.abs(dx).max(), "max|dW|", max(np.abs(w).max() for w in dWs))
    for a, b in fwd_stats(xs, Ws, bs, ACT[act]):
        assert a == 0.0 and b == 0.0
    st = bwd_stats(xs, g, Ws, dg, ACT[act])
    assert st["dx"] == (0.0, 0.0) and all(v == (0.0, 0.0) for v in st["dW"])
    assert all(np.array_equal(fixed_piece(v), v) and np.array_equal(plain_piece(v), v) for v in xs)


def test_exact_conditions_refuse_data_outside_the_exact_set():
    rng = np.random.default_rng(5)
    x, Ws, bs, dg = exact_data(rng, 200, 64, 3)
    x[7, 3] = 2049.0
    with pytest.raises(AssertionError):
        exact_conditions(x, Ws, bs, dg, 0)
    x[7, 3] = 5000.0
    with pytest.raises(AssertionError):
        exact_conditions(x, Ws, bs, dg, 0)


def test_pieces_keep_eleven_bits():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 64)) * 3
    for p in (fixed_piece(x), plain_piece(x), lead_piece(x)):
        assert (np.abs(p - x) <= np.exp2(-11) * np.abs(x) + 1e-7).all()
        assert (np.abs(p - x) / np.abs(x)).max() > np.exp2(-14)


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("L", [2, 4, 5])
def test_the_two_emulations_bracket_a_threshold(act, L):
    """r_drop > 4 r32 on the statistic cases, so that sqrt(r32 * r_drop) separates the two"""
    rng = np.random.default_rng([L, ACT[act]])
    x, Ws, bs, dg = normal_data(rng, 3000, 64, L)
    xs, g, _ = ref_fwd(x, Ws, bs, ACT[act])
    tape, g32 = [f32(v) for v in xs], f32(g)
    fs = fwd_stats(tape, Ws, bs, ACT[act])
    bst = bwd_stats(tape, g32, Ws, dg, ACT[act])
    print([(f"{a:.2e}", f"{b:.2e}") for a, b in fs + [bst["dx"]] + bst["dW"]])
    for r32, r_drop in fs + [bst["dx"]] + bst["dW"]:
        assert 0 < r32 < 1e-7, r32
        assert r_drop > 4 * r32, (r32, r_drop)
