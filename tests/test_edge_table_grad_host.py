"""The float64 reference of the Jacobian table (tests/edge_table_grad_ref.py) checked on its own, without a GPU: against the
analytic Jacobian of a float64 edge MLP, and the recorded reason for the design — interpolate a table of J, do
not differentiate the interpolant of the table of e."""
import numpy as np
import pytest

import edge_table_grad_ref as R

LO, HI = 0.09, 0.5
N = 20000


def _model(act, scale=1.0, E=3):
    centers, gap = R.rbf_grid64()
    W, B = R.random_mlp(128, E, 4, scale, seed=11)
    return lambda d: R.mlp_value_and_jacobian(d, centers, gap, W, B, act)


def _tables(fn, T):
    x, xm, _ = R.table_points(LO, HI, T)
    e, J = fn(x)
    em, Jm = fn(xm)
    return e, J, em, Jm


def _distances():
    lo, hi = float(np.float32(LO)), float(np.float32(HI))
    d = np.random.default_rng(3).uniform(lo, hi, N)
    d[:2] = lo, hi
    return d


@pytest.mark.parametrize("act", ["softplus", "tanh"])
def test_interpolated_jacobian_table_matches_the_analytic_jacobian(act):
    """T = 4096 on [0.09, 0.5], unit-scale weights: within 1e-8 of max |J| (measured 5.5e-11 softplus, 1.4e-10 tanh: a loose
    sanity bound on the reference, not on any kernel).  The formula is compared at float64 stencil positions.  The float32
    position of the kernel displaces a distance by up to ~2.5e-4 of a cell (the roundings of d - lo and of 1 / h, times up to
    T cells), 2.5e-8 in d: that moves J itself by |J'| 2.5e-8 ~ 1e-6 max |J|, the same displacement the table of e has always
    had.  With the float32 position the interpolant is therefore compared with the analytic J AT the position it encodes."""
    fn = _model(act)
    T = 4096
    _, J, _, _ = _tables(fn, T)
    d = _distances()
    scale = np.abs(J).max()
    err = np.abs(R.interp(J, d, LO, HI, "float64") - fn(d)[1]).max() / scale
    print(f"{act}: J table, float64 position: {err:.2e}")
    assert err <= 1e-8, err
    i0, f = R.position(d.astype(np.float32), LO, HI, T)
    x, _, h = R.table_points(LO, HI, T)
    d_enc = x[i0 + 1] + f * h
    assert np.abs(d_enc - d.astype(np.float32)).max() <= 4e-4 * h        # the displacement itself: a fraction of a cell
    err32 = np.abs(R.interp(J, d.astype(np.float32), LO, HI) - fn(d_enc)[1]).max() / scale
    print(f"{act}: J table, float32 position, at the encoded distance: {err32:.2e}")
    assert err32 <= 1e-8, err32


def test_relu_jacobian_has_kinks_the_guard_can_see():
    """J of a relu edge MLP jumps where a hidden unit switches: at the midpoints the cubic interpolant of the J table misses it
    by more than 1e-2 of max |J| — what ng_edge_table_check compares, five orders above any tolerance in use"""
    fn = _model("relu")
    T = 4096
    _, J, _, Jm = _tables(fn, T)
    t = np.arange(1, T - 2)
    it = 0.5625 * (J[t] + J[t + 1]) - 0.0625 * (J[t - 1] + J[t + 2])
    err = np.abs(it - Jm[t]).max() / np.abs(J).max()
    print(f"relu: J check at the midpoints: {err:.2e}")
    assert err > 1e-2, err
    # and the smooth activations sit far below it at the same midpoints
    for act in ("softplus", "tanh"):
        _, J, _, Jm = _tables(_model(act), T)
        it = 0.5625 * (J[t] + J[t + 1]) - 0.0625 * (J[t - 1] + J[t + 2])
        assert np.abs(it - Jm[t]).max() / np.abs(J).max() < 1e-8


@pytest.mark.parametrize("act", ["softplus", "tanh"])
def test_differentiated_interpolant_of_a_float32_table_is_worse_than_the_jacobian_table(act):
    """the recorded reason for the design: with the tables rounded to float32 (what the device holds) the derivative of the
    interpolant of e carries the table's rounding noise divided by h; the interpolated J table carries only its own rounding"""
    fn = _model(act)
    T = 4096
    e, J, _, _ = _tables(fn, T)
    d = _distances()
    Jref = fn(d)[1]
    scale = np.abs(Jref).max()
    e32, J32 = e.astype(np.float32), J.astype(np.float32)
    err_J = np.abs(R.interp(J32, d, LO, HI, "float64") - Jref).max() / scale
    err_de = np.abs(R.dinterp(e32, d, LO, HI, "float64") - Jref).max() / scale
    print(f"{act}: float32 tables: J table {err_J:.2e}, d/dd of the e table {err_de:.2e}")
    assert err_J <= 2e-7                     # 2^-24 per entry, |weights| sum to at most 1.25, a margin for max|J| entries
    assert err_de >= 100 * err_J, (err_de, err_J)
    # in float64 both converge, the J table three orders further (the issue's table: 5.5e-11 against 2.2e-8)
    err_de64 = np.abs(R.dinterp(e, d, LO, HI, "float64") - Jref).max() / scale
    err_J64 = np.abs(R.interp(J, d, LO, HI, "float64") - Jref).max() / scale
    print(f"{act}: float64 tables: J table {err_J64:.2e}, d/dd of the e table {err_de64:.2e}")
    assert err_J64 < err_de64 <= 1e-6


def test_table_dinput_reference_on_a_hand_made_case():
    """dead slots of every kind are zero whatever their de holds; pos indexes compacted distances; a distance on a table point
    reads that row of J"""
    T, E = 16, 2
    lo, hi = np.float32(0.0625), np.float32(0.0625 + 13 * 2.0 ** -6)          # h = 2^-6, exact
    J = np.random.default_rng(0).standard_normal((T, E))
    d_src = np.array([0.0625 + 3 * 2.0 ** -6, 0.0, -0.0, -1.0, np.nan, 0.0625 + 5.5 * 2.0 ** -6], np.float32)
    de = np.array([[1, 2], [np.nan, 1e30], [1e30, 1], [np.nan, np.nan], [3, 3], [0.5, -1]], np.float32)
    dd, mag = R.table_dinput(d_src, d_src, None, lo, hi, T, J, de)
    assert np.all(dd[1:5] == 0) and np.all(mag[1:5] == 0)
    assert dd[0] == pytest.approx(J[4, 0] * 1 + J[4, 1] * 2, rel=1e-14)          # u = 3 + 1: table row 4
    w = np.array([-0.0625, 0.5625, 0.5625, -0.0625])
    assert dd[5] == pytest.approx(0.5 * (w @ J[5:9, 0]) - (w @ J[5:9, 1]), rel=1e-13)
    pos = np.array([2, -1, -1, -1, -1, 0], np.int32)
    d_c = np.array([d_src[5], np.nan, d_src[0]], np.float32)
    dd2, _ = R.table_dinput(d_src, d_c, pos, lo, hi, T, J, de)
    assert np.array_equal(dd, dd2)
