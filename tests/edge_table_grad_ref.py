"""NumPy float64 reference of the table path's input gradient (csrc/edge_table.hip: ng_edge_table_dinput) and the float64
model of the design decision behind it: a table of the edge Jacobian J = d f_W / d d, interpolated with the
four-point cubic Lagrange stencil of the table of e, against the derivative of the interpolant of e.

The stencil POSITION (u, the cell i and the fraction f) is taken in float32 exactly as et_geom / et_stencil compute it —
h = (hi - lo) / (T - 3), inv_h = 1 / h, u = (d - lo) inv_h + 1, i = clamp(floor(u), 1, T - 3), f = u - i — so that the
reference reads the same four table rows as the kernel; everything behind it (weights, sums) is float64.  ``position="float64"``
takes the position in float64 too: the interpolation formula on its own, for the comparison with an analytic Jacobian."""
import numpy as np

ACTS = ("softplus", "tanh", "relu")


# ------------------------------------------------------------------------------------------------------------ stencil
def geom32(lo, hi, T):
    """(lo, inv_h, h) in float32, as et_geom"""
    lo, hi = np.float32(lo), np.float32(hi)
    h = np.float32(np.float32(hi - lo) / np.float32(T - 3))
    return lo, np.float32(np.float32(1.0) / h), h


def position(d, lo, hi, T, position="float32"):
    """(i0, f): the first of the four table rows a distance reads and its fraction in the cell.  float32: the kernel's own
    arithmetic (the product and the sum rounded separately; on a grid whose h is a power of two both are exact up to the one
    rounding of the sum, so a contracted multiply-add gives the same u)."""
    if position == "float32":
        lo32, inv_h, _ = geom32(lo, hi, T)
        d = np.asarray(d, np.float32)
        u = (np.float32(d - lo32) * inv_h).astype(np.float32) + np.float32(1.0)
        with np.errstate(invalid="ignore"):
            i = np.clip(np.floor(u), 1, T - 3)
        i = np.where(np.isfinite(u), i, 1).astype(np.int64)
        f = (u - i.astype(np.float32)).astype(np.float32)
        return i - 1, f.astype(np.float64)
    h = (np.float64(np.float32(hi)) - np.float64(np.float32(lo))) / (T - 3)
    u = (np.asarray(d, np.float64) - np.float64(np.float32(lo))) / h + 1.0
    i = np.clip(np.floor(u), 1, T - 3).astype(np.int64)
    return i - 1, u - i


def weights(f):
    """the Lagrange weights at nodes -1, 0, 1, 2 of the fraction f, float64: [n, 4]"""
    f = np.asarray(f, np.float64)
    return np.stack([-f * (f - 1) * (f - 2) / 6, (f + 1) * (f - 1) * (f - 2) / 2, -(f + 1) * f * (f - 2) / 2,
                     (f + 1) * f * (f - 1) / 6], 1)


def dweights(f):
    """d weights / d f"""
    f = np.asarray(f, np.float64)
    return np.stack([-(3 * f * f - 6 * f + 2) / 6, (3 * f * f - 4 * f - 1) / 2, -(3 * f * f - 2 * f - 2) / 2,
                     (3 * f * f - 1) / 6], 1)


def table_points(lo, hi, T):
    """float64 positions of the T table points and of the T midpoints (x_t + h / 2), for the float32 range [lo, hi]"""
    lo64, hi64 = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    h = (hi64 - lo64) / (T - 3)
    t = np.arange(T)
    return lo64 + (t - 1.0) * h, lo64 + (t - 0.5) * h, h


def interp(tab, d, lo, hi, position_="float32"):
    """the cubic interpolant of the table tab [T, E] at the distances d: [n, E] float64"""
    T = tab.shape[0]
    i0, f = position(d, lo, hi, T, position_)
    return np.einsum("nk,nke->ne", weights(f), np.asarray(tab, np.float64)[i0[:, None] + np.arange(4)])


def dinterp(tab, d, lo, hi, position_="float32"):
    """the derivative with respect to d of the cubic interpolant of tab [T, E]: [n, E] float64"""
    T = tab.shape[0]
    i0, f = position(d, lo, hi, T, position_)
    h = table_points(lo, hi, T)[2]
    return np.einsum("nk,nke->ne", dweights(f), np.asarray(tab, np.float64)[i0[:, None] + np.arange(4)]) / h


def table_dinput(d_src, d_eff, pos, lo, hi, T, j_tab, de):
    """ng_edge_table_dinput in float64: dd[i] = m_i sum_c de[i][c] sum_k w_k(d_i) j_tab[i0 + k][c], m_i = d_src[i] > 0, slot
    i's distance d_eff[pos[i]] when pos is given.  Returns (dd [n], mag [n]): mag = sum_{k,c} |w_k J de|, the terms in float64
    from the same float32 inputs (what a rounding bound scales with).  Dead slots: 0, their de is not read."""
    d_src = np.asarray(d_src, np.float32)
    n = d_src.shape[0]
    with np.errstate(invalid="ignore"):
        live = np.nonzero(d_src > 0)[0]
    dd, mag = np.zeros(n), np.zeros(n)
    if len(live):
        d = np.asarray(d_eff, np.float32)[np.asarray(pos)[live] if pos is not None else live]
        i0, f = position(d, lo, hi, T)
        w = weights(f)
        J = np.asarray(j_tab, np.float64).reshape(T, -1)[i0[:, None] + np.arange(4)]          # [n, 4, E]
        g = np.asarray(de, np.float64).reshape(n, -1)[live]
        terms = w[:, :, None] * J * g[:, None, :]
        dd[live] = terms.sum((1, 2))
        mag[live] = np.abs(terms).sum((1, 2))
    return dd, mag


# ----------------------------------------------------------------------------------------------------- float64 edge MLP
def rbf_grid64(low=0.005, high=0.20, count=128):
    c = np.linspace(low, high, count)
    return c, float(c[1] - c[0])


def random_mlp(H=128, E=3, Le=4, scale=1.0, seed=0):
    """Glorot-scaled normal weights times ``scale`` and small biases: (W, B) float64"""
    rng = np.random.default_rng(seed)
    W, B = [], []
    for t in range(Le):
        kout = H if t < Le - 1 else E
        W.append(scale * rng.standard_normal((H, kout)) * np.sqrt(2.0 / (H + kout)))
        B.append(0.1 * rng.standard_normal(kout))
    return W, B


def _act(name, a):
    """act(a), act'(a) (relu'(0) = 0)"""
    if name == "softplus":
        return np.logaddexp(a, 0.0), 1.0 / (1.0 + np.exp(-a))
    if name == "tanh":
        y = np.tanh(a)
        return y, 1.0 - y * y
    if name == "relu":
        return np.maximum(a, 0.0), (a > 0).astype(np.float64)
    raise ValueError(name)


def mlp_value_and_jacobian(d, centers, gap, W, B, act):
    """(f_W(d), d f_W / d d), each [n, E] float64: the value and its tangent carried through the layers (forward mode)"""
    d = np.asarray(d, np.float64)
    diff = d[:, None] - centers[None, :]
    x = np.exp(-diff * diff / gap)
    t = x * (-2.0 * diff / gap)
    for l in range(len(W) - 1):
        y, g = _act(act, x @ W[l] + B[l])
        x, t = y, g * (t @ W[l])
    return x @ W[-1] + B[-1], t @ W[-1]
