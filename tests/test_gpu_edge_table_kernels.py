"""The five entry points of the edge-function table (csrc/edge_table.hip) called directly, each against a plain NumPy
float64 statement of the same operation: ng_edge_table_range (min / max of the live distances, max |de|), ng_edge_table_points,
ng_edge_table_interp (four-point cubic Lagrange), ng_edge_table_scatter (its exact adjoint, 64-bit fixed point) and
ng_edge_table_check (the guard).  The inputs are the ones where such kernels go wrong: dead slots of every kind, the stencil's
clamped end cells, degenerate ranges, one huge gradient row, non-finite gradients, and more same-sign terms on one table entry
than the fixed point of 2^38 held."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _K:
    """the library context and the current stream; ``call(name, *args)`` checks the return code.  ``t`` keeps every tensor it
    makes alive for the test (a pointer taken from a temporary would be handed to the next allocation)."""

    def __init__(self, dev):
        import torch
        from nmrgnn_amd import _lib
        self.torch, self.dev = torch, dev
        self.keep = []
        self.ctx = _lib.get_context(dev.index or 0)
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(self, name, *args):
        self.ctx.check(getattr(self.ctx.lib, name)(self.ctx.handle, self.st, *args), name)

    def t(self, a):
        x = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(x)
        return x

    def get(self, x):
        self.torch.cuda.synchronize(self.dev)
        return x.cpu().numpy()


def _p(x):
    from nmrgnn_amd._lib import ptr
    return ptr(x)


@pytest.fixture
def K(gpu_device):
    return _K(gpu_device)


def _range(K, d_src, d_eff=None, pos=None, de=None, E=1, pad=0.0, fill=-7.0):
    out = K.t(np.full(4, fill, np.float32))
    K.call("ng_edge_table_range", len(d_src), E, _p(d_src), _p(d_eff), _p(pos), _p(de), float(pad), _p(out))
    return K.get(out)


def _range_ref(d_src, d_eff, pos, pad):
    """range[0..1] of the kernel, in float32 arithmetic: min / max over d_src > 0, a degenerate range widened to
    max(1e-6, |lo| 2^-20), then pad * width on either side"""
    live = d_src > 0
    if not live.any():
        lo, hi = np.float32(0), np.float32(1)
    else:
        idx = np.nonzero(live)[0]
        d = d_eff[pos[idx]] if pos is not None else d_eff[idx]
        lo, hi = np.float32(d.min()), np.float32(d.max())
    wmin = max(np.float32(1e-6), np.float32(abs(lo)) * np.float32(2.0 ** -20))
    if not (hi - lo >= wmin):
        hi = np.float32(lo + wmin)
    w = np.float32((hi - lo) * np.float32(pad))
    return np.float32(lo - w), np.float32(hi + w)


def _ulp(x):
    return np.spacing(np.abs(np.float32(x))).astype(np.float64)


def _slots(n, seed, frac_dead=0.3):
    """distances in slot order with dead slots of every kind (0, -0.0, negative, NaN)"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.09, 0.45, n).astype(np.float32)
    dead = rng.random(n) < frac_dead
    kinds = np.array([0.0, -0.0, -0.2, np.nan], np.float32)
    d[dead] = kinds[rng.integers(0, 4, dead.sum())]
    return d


# ------------------------------------------------------------------------------------------------------------- range
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 2_500_001])
@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("use_pos", [False, True])
def test_range_min_max_and_max_abs_de(K, n, E, use_pos):
    rng = np.random.default_rng(n * 10 + E)
    d_src = _slots(n, n + E)
    if n > 1:       # the extremes in the last slots (the last grid-stride trip, the clamped tail)
        d_src[-1], d_src[n // 2] = 0.4999, 0.0501
    live = d_src > 0
    de = rng.standard_normal((n, E)).astype(np.float32)
    de[~live] = np.float32(1e30) * np.sign(rng.standard_normal((int((~live).sum()), E))).astype(np.float32)  # dead rows: ignored
    if n > 3 and live[n // 3]:
        de[n // 3, E - 1] = -55.0        # the largest |de|, negative, in the last column
    if use_pos:     # compacted distances: slot i's distance is d_eff[pos[i]]
        pos = rng.permutation(n).astype(np.int32)
        d_eff = np.full(n, np.float32(np.nan))
        d_eff[pos] = np.where(live, d_src, np.float32(-1.0))
        d_eff = d_eff.astype(np.float32)
    else:
        pos, d_eff = None, d_src
    g_src, g_eff, g_de = K.t(d_src), K.t(d_eff), K.t(de)
    g_pos = K.t(pos) if pos is not None else None
    for pad in (0.0, 0.25):
        r = _range(K, g_src, g_eff, g_pos, g_de, E, pad)
        lo, hi = _range_ref(d_src, d_eff, pos, pad)
        tol = 0 if pad == 0 else 1      # lo - w may be contracted into one fma: one rounding fewer
        assert abs(float(r[0]) - float(lo)) <= tol * _ulp(lo) and abs(float(r[1]) - float(hi)) <= tol * _ulp(hi), (pad, r, lo, hi)
        mx = np.abs(de[live]).max() if live.any() else 0.0
        assert r[2] == np.float32(mx), (r[2], mx)
        assert r[3] == np.float32(-7.0)
    # distances only: range[2] is left alone; gradients only: range[0..1] are
    r = _range(K, g_src, g_eff, g_pos, None, E)
    assert r[2] == np.float32(-7.0) and r[0] == _range_ref(d_src, d_eff, pos, 0.0)[0]
    r = _range(K, g_src, None, None, g_de, E)
    assert r[0] == r[1] == np.float32(-7.0) and r[2] == np.float32(np.abs(de[live]).max() if live.any() else 0.0)


@pytest.mark.parametrize("T", [8, 4096])
def test_range_of_degenerate_distance_sets_has_positive_width(K, T):
    """no live slot: [0, 1]; one live slot, or all live distances equal (0.3, 40, 1000): a table of positive width, so that
    h = (hi - lo) / (T - 3) > 0 in float32 and the stencil of a distance at lo is finite"""
    n = 1000
    cases = {"none": _slots(n, 1, frac_dead=1.0)}
    one = np.zeros(n, np.float32); one[417] = 0.23
    cases["one"] = one
    for v in (0.3, 40.0, 1000.0):
        d = _slots(n, 2); d[d > 0] = v
        cases[f"equal {v}"] = d
    for name, d in cases.items():
        r = _range(K, K.t(d), K.t(d))
        lo, hi = _range_ref(d, d, None, 0.0)
        assert r[0] == lo and r[1] == hi, (name, r, lo, hi)
        if name == "none":
            assert (r[0], r[1]) == (0.0, 1.0)
            continue
        assert r[0] == d[d > 0].min(), name
        h = np.float32(np.float32(r[1] - r[0]) / np.float32(T - 3))
        assert r[1] > r[0] and h > 0 and np.isfinite(np.float32(1) / h), (name, r, h)
        # the kernels themselves: the table point at lo and the interpolation there are finite (no 0 * inf)
        rng_t = K.t(np.array([r[0], r[1], 0, 0], np.float32))
        d_tab, ones = K.t(np.zeros(T, np.float32)), K.t(np.zeros(T, np.float32))
        K.call("ng_edge_table_points", T, 0, _p(rng_t), _p(d_tab), _p(ones), None)
        tab = np.linspace(1.0, 2.0, T, dtype=np.float32)
        e = K.t(np.full(n, np.nan, np.float32))
        K.call("ng_edge_table_interp", n, 1, T, _p(K.t(d)), _p(K.t(d)), None, _p(rng_t), _p(K.t(tab)), None, _p(e))
        e = K.get(e)
        assert K.get(d_tab)[1] == r[0]
        assert np.array_equal(e, np.where(d > 0, tab[1], np.float32(0))), name


def test_range_records_non_finite_gradients_of_live_slots_only(K):
    n = 3000
    d = _slots(n, 5)
    live = np.nonzero(d > 0)[0]
    dead = np.nonzero(~(d > 0))[0]
    de = np.random.default_rng(5).standard_normal((n, 2)).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        x = de.copy(); x[dead[7], 1] = bad
        assert _range(K, K.t(d), None, None, K.t(x), 2)[2] == np.abs(de[live]).max()
        x = de.copy(); x[live[11], 0] = bad
        assert _range(K, K.t(d), None, None, K.t(x), 2)[2] == np.inf, bad


# ------------------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize("T", [8, 2048, 4096])
@pytest.mark.parametrize("lo,hi", [(0.09, 0.45), (-0.3, 0.7), (40.0, 40.0004)])
def test_points_and_midpoints(K, T, lo, hi):
    for mid in (0, 1):
        rows = 2 * T if mid else T
        rng_t = K.t(np.array([lo, hi, 0, 0], np.float32))
        d_tab, ones = K.t(np.full(2 * T + 5, -9.0, np.float32)), K.t(np.full(2 * T + 5, -9.0, np.float32))
        perm = K.t(np.full(2 * T + 5, -9, np.int32))
        K.call("ng_edge_table_points", T, mid, _p(rng_t), _p(d_tab), _p(ones), _p(perm))
        d_tab, ones, perm = K.get(d_tab), K.get(ones), K.get(perm)
        lo32, hi32 = np.float32(lo), np.float32(hi)
        h = float(hi32 - lo32) / (T - 3)                      # float64 statement
        t = np.arange(rows)
        ref = np.where(t < T, lo32 + (t - 1.0) * h, lo32 + (t - T - 0.5) * h)
        # one rounding of the fma plus the float32 rounding of h itself (relative 2^-24 of |t - 1| h <= hi - lo)
        tol = _ulp(ref.astype(np.float32)) + 2.0 ** -23 * abs(float(hi32 - lo32))
        assert np.all(np.abs(d_tab[:rows] - ref) <= tol), (mid, np.abs(d_tab[:rows] - ref).max())
        assert np.all(ones[:rows] == 1.0) and np.array_equal(perm[:rows], np.arange(rows))
        assert np.all(d_tab[rows:] == -9.0) and np.all(ones[rows:] == -9.0) and np.all(perm[rows:] == -9)
        assert d_tab[1] == lo32 and np.all(np.diff(d_tab[:T]) >= 0)
    # perm may be NULL
    d_tab, ones = K.t(np.zeros(T, np.float32)), K.t(np.zeros(T, np.float32))
    K.call("ng_edge_table_points", T, 0, _p(rng_t), _p(d_tab), _p(ones), None)
    assert np.all(K.get(ones) == 1.0)


# ----------------------------------------------------------------------------------------------------------- interp
def _grid(T, lo=0.0625):
    """a range whose h is a power of two: every distance below is exact in float32, and so are (d - lo) / h and the stencil's
    fraction f — the float64 references use the same u as the kernel"""
    k = int(np.ceil(np.log2(T))) + 1
    h = 2.0 ** -k
    return np.float32(lo), np.float32(lo + (T - 3) * h), h


def _grid_distances(T, n, rng, lo, h):
    """distances lo + (j + m / 256) h: every cell, at exact table points (m = 0), at lo and hi, in the first and last cells"""
    j = rng.integers(0, T - 3, n)
    m = rng.integers(0, 256, n)
    m[rng.random(n) < 0.2] = 0
    d = (lo + (j + m / 256.0) * h).astype(np.float32)
    special = [lo, lo + (T - 3) * h, lo + h / 256, lo + 0.5 * h, lo + 0.99609375 * h, lo + (T - 4) * h,
               lo + (T - 3.5) * h, lo + (T - 3 - 1 / 256) * h, lo + h, lo + (T - 4) * h]
    d[:len(special)] = np.array(special, np.float32)
    assert np.all(np.float64(d) == lo + np.round((np.float64(d) - lo) / h * 256) / 256 * h)
    return d


def _stencil64(d, lo, h, T):
    """float64 stencil: first point i0 and the four Lagrange weights at nodes -1, 0, 1, 2 of the cell [i, i + 1] that holds
    u = (d - lo) / h + 1, the cell clamped to [1, T - 3]"""
    u = (np.asarray(d, np.float64) - np.float64(lo)) / h + 1.0
    i = np.clip(np.floor(u).astype(np.int64), 1, T - 3)
    f = u - i
    w = np.stack([-f * (f - 1) * (f - 2) / 6, (f + 1) * (f - 1) * (f - 2) / 2, -(f + 1) * f * (f - 2) / 2,
                  (f + 1) * f * (f - 1) / 6], 1)
    return i - 1, w


def _stencil32(d, lo, h, T):
    """the kernel's float32 weights (exact u, f as in _grid; the products in the kernel's order)"""
    u = (np.asarray(d, np.float64) - np.float64(lo)) / h + 1.0
    i = np.clip(np.floor(u).astype(np.int64), 1, T - 3)
    f = (u - i).astype(np.float32)
    one, two, c6, half = np.float32(1), np.float32(2), np.float32(1.0) / np.float32(6.0), np.float32(0.5)
    fm1, fm2, fp1 = f - one, f - two, f + one
    w = np.stack([(-f) * fm1 * fm2 * c6, fp1 * fm1 * fm2 * half, (-fp1) * f * fm2 * half, fp1 * f * fm1 * c6], 1)
    return i - 1, w.astype(np.float32)


def _interp(K, n, E, T, d_src, d_eff, pos, rng_t, tab, gate=None, fill=np.nan):
    e = K.t(np.full((n, E), fill, np.float32))
    K.call("ng_edge_table_interp", n, E, T, _p(d_src), _p(d_eff), _p(pos), _p(rng_t), _p(tab), _p(gate), _p(e))
    return K.get(e)


@pytest.mark.parametrize("E,T", [(1, 8), (3, 8), (2, 64), (5, 64), (8, 2048), (4, 4096), (1, 4096), (3, 4096)])
def test_interp_against_float64_lagrange(K, E, T):
    rng = np.random.default_rng(E * 100 + T)
    n = 20000
    lo, hi, h = _grid(T)
    d = _grid_distances(T, n, rng, float(lo), h)
    dead = rng.random(n) < 0.25
    dead[:10] = False
    d_src = d.copy()
    d_src[dead] = np.array([0.0, -0.0, np.nan, -1.0], np.float32)[rng.integers(0, 4, dead.sum())]
    tab = rng.standard_normal((T, E)).astype(np.float32) * np.float32(3)
    rng_t = K.t(np.array([lo, hi, 0, 0], np.float32))
    for use_pos in (False, True):
        if use_pos:
            pos = rng.permutation(n).astype(np.int32)
            d_eff = np.empty(n, np.float32); d_eff[pos] = d
            g_pos = K.t(pos)
        else:
            d_eff, g_pos = d, None
        e = _interp(K, n, E, T, K.t(d_src), K.t(d_eff), g_pos, rng_t, K.t(tab))
        i0, w = _stencil64(d, lo, h, T)
        vals = tab.astype(np.float64)[i0[:, None] + np.arange(4)]            # [n, 4, E]
        ref = np.einsum("nk,nke->ne", w, vals)
        mag = np.einsum("nk,nke->ne", np.abs(w), np.abs(vals))
        live = ~dead
        assert np.all(e[dead] == 0) and not np.signbit(e[dead]).any()       # dead slots: exactly +0, whatever e_out held
        err = np.abs(e[live] - ref[live])
        assert np.all(err <= 12 * 2.0 ** -24 * mag[live] + 1e-30), (use_pos, float((err / mag[live]).max()))
        # on a table point (f = 0) the kernel returns the table value itself
        on = live & (np.floor((np.float64(d) - lo) / h) == (np.float64(d) - lo) / h) & (np.float64(d) < float(hi))
        j = np.round((np.float64(d[on]) - lo) / h).astype(np.int64) + 1
        assert np.array_equal(e[on], tab[j]), use_pos
        # the clamped ends: d = lo reads table point 1, d = hi table point T - 2
        assert np.array_equal(e[0], tab[1]) and np.array_equal(e[1], tab[T - 2])


@pytest.mark.parametrize("E,T", [(1, 8), (3, 64), (8, 2048), (4, 4096)])
def test_interp_reproduces_a_cubic(K, E, T):
    """a table sampled from a cubic polynomial: the cubic interpolant is the cubic itself, in every cell including the clamped
    end cells (a wrong weight or a stencil off by one is off by far more than rounding)"""
    rng = np.random.default_rng(T + E)
    n = 8000
    lo, hi, h = _grid(T, lo=0.125)
    d = _grid_distances(T, n, rng, float(lo), h)
    span = float(hi - lo)
    coef = rng.uniform(-2, 2, (4, E))

    def p(x):
        s = (np.float64(x)[:, None] - float(lo)) / span * 2 - 1           # [-1, 1] over the table
        return coef[0] + coef[1] * s + coef[2] * s ** 2 + coef[3] * s ** 3

    x_t = float(lo) + (np.arange(T) - 1.0) * h
    tab = p(x_t).astype(np.float32)
    rng_t = K.t(np.array([lo, hi, 0, 0], np.float32))
    e = _interp(K, n, E, T, K.t(d), K.t(d), None, rng_t, K.t(tab))
    i0, w = _stencil64(d, lo, h, T)
    mag = np.einsum("nk,nke->ne", np.abs(w), np.abs(tab.astype(np.float64)[i0[:, None] + np.arange(4)]))
    err = np.abs(e - p(d))
    assert np.all(err <= 12 * 2.0 ** -24 * mag), float((err / mag).max())


def test_interp_gate(K):
    """gate[0] != 0: the per-edge kernels answered the call, e_out is not touched; gate[0] == 0: written"""
    T, E, n = 64, 3, 5000
    lo, hi, h = _grid(T)
    rng = np.random.default_rng(1)
    d = _grid_distances(T, n, rng, float(lo), h)
    rng_t, tab = K.t(np.array([lo, hi, 0, 0], np.float32)), K.t(rng.standard_normal((T, E)).astype(np.float32))
    up = K.t(np.array([1, 7, 0, 0, 0, 0, 0, 0], np.int32))
    down = K.t(np.array([0, -1, 2 * T, 0, 0, 0, 0, 0], np.int32))
    e = _interp(K, n, E, T, K.t(d), K.t(d), None, rng_t, tab, gate=up, fill=123.0)
    assert np.all(e == 123.0)
    e_down = _interp(K, n, E, T, K.t(d), K.t(d), None, rng_t, tab, gate=down, fill=123.0)
    assert np.array_equal(e_down, _interp(K, n, E, T, K.t(d), K.t(d), None, rng_t, tab))
    assert not np.any(e_down == 123.0)


# ---------------------------------------------------------------------------------------------------------- scatter
def _scatter(K, n, E, T, rows_out, d_src, d_eff, pos, rng_t, de, fill=np.nan):
    out = K.t(np.full((rows_out, E), fill, np.float32))
    K.call("ng_edge_table_scatter", n, E, T, rows_out, _p(d_src), _p(d_eff), _p(pos), _p(rng_t), _p(de), _p(out))
    return K.get(out)


def _quantum(maxabs, n):
    """the scatter's fixed-point quantum: q = 2^(ex - sh), maxabs < 2^ex, sh = 38 - max(0, ceil(log2 n) - 24)"""
    ex = int(np.frexp(np.float64(maxabs))[1]) if maxabs > 0 else 0
    lg = int(np.ceil(np.log2(n))) if n > 1 else 0
    return 2.0 ** (ex - (38 - max(0, lg - 24)))


def _scatter_ref(d, live, de, lo, h, T):
    """float64 sum, per table entry, of the kernel's fp32 terms fl(w_k de) (its own weights) and how many land there"""
    E = de.shape[1]
    i0, w = _stencil32(d[live], lo, h, T)
    terms = (w[:, :, None] * de[live][:, None, :]).astype(np.float64)      # fp32 products, summed in float64
    ref, cnt = np.zeros((T, E)), np.zeros(T)
    for k in range(4):
        np.add.at(ref, i0 + k, terms[:, k, :])
        np.add.at(cnt, i0 + k, 1)
    return ref, cnt


@pytest.mark.parametrize("E,T", [(1, 8), (3, 64), (5, 2048), (8, 2048), (4, 4096)])
def test_scatter_is_the_adjoint(K, E, T):
    rng = np.random.default_rng(7 * E + T)
    n = 60000
    lo, hi, h = _grid(T)
    d = _grid_distances(T, n, rng, float(lo), h)
    d_src = d.copy()
    dead = rng.random(n) < 0.2
    dead[:10] = False
    d_src[dead] = np.array([0.0, -0.0, np.nan], np.float32)[rng.integers(0, 3, dead.sum())]
    live = ~dead
    de = rng.standard_normal((n, E)).astype(np.float32)
    de[dead] = np.float32(3e30)                     # dead rows are not read into the max or the sums
    rng_t = K.t(np.array([lo, hi, 0, 0], np.float32))
    rows_out = 2 * T
    g_src, g_eff, g_de = K.t(d_src), K.t(d), K.t(de)
    out = _scatter(K, n, E, T, rows_out, g_src, g_eff, None, rng_t, g_de)
    assert np.all(out[T:] == 0) and not np.signbit(out[T:]).any()
    assert K.get(rng_t)[2] == np.abs(de[live]).max()
    ref, cnt = _scatter_ref(d, live, de, lo, h, T)
    q = _quantum(np.abs(de[live]).max(), n)
    bound = (cnt[:, None] + 1) * q + 2.0 ** -23 * np.abs(ref)
    assert np.all(np.abs(out[:T] - ref) <= bound), float((np.abs(out[:T] - ref) / bound).max())
    # the adjoint identity, both sides in float64: <interp(tab), de> = <tab, scatter(de)>
    tab = rng.standard_normal((T, E)).astype(np.float32)
    e = _interp(K, n, E, T, g_src, g_eff, None, rng_t, K.t(tab))
    lhs = np.sum(e.astype(np.float64)[live] * de[live])
    rhs = np.sum(tab.astype(np.float64) * out[:T])
    assert abs(lhs - rhs) <= 1e-6 * np.sum(np.abs(e.astype(np.float64)[live] * de[live])), (lhs, rhs)
    # the same bits from run to run, for the compacted form (pos), and for any order of the edges
    assert np.array_equal(out, _scatter(K, n, E, T, rows_out, g_src, g_eff, None, rng_t, g_de, fill=-1.0))
    pos = rng.permutation(n).astype(np.int32)
    d_c = np.empty(n, np.float32); d_c[pos] = d
    assert np.array_equal(out, _scatter(K, n, E, T, rows_out, g_src, K.t(d_c), K.t(pos), rng_t, g_de))
    perm = rng.permutation(n)
    outp = _scatter(K, n, E, T, rows_out, K.t(d_src[perm]), K.t(d[perm]), None, rng_t, K.t(de[perm]))
    assert np.array_equal(out, outp)


def test_scatter_with_one_gradient_row_a_million_times_larger(K):
    T, E, n = 64, 2, 30000
    rng = np.random.default_rng(11)
    lo, hi, h = _grid(T)
    d = _grid_distances(T, n, rng, float(lo), h)
    live = np.ones(n, bool)
    de = rng.standard_normal((n, E)).astype(np.float32)
    de[1234] *= np.float32(1e6)
    rng_t = K.t(np.array([lo, hi, 0, 0], np.float32))
    out = _scatter(K, n, E, T, T, K.t(d), K.t(d), None, rng_t, K.t(de))
    ref, cnt = _scatter_ref(d, live, de, lo, h, T)
    q = _quantum(np.abs(de).max(), n)
    assert np.all(np.abs(out - ref) <= (cnt[:, None] + 1) * q + 2.0 ** -23 * np.abs(ref))


def test_scatter_does_not_wrap_with_many_same_sign_terms_on_one_entry(K):
    """2^25 + 2^22 live edges at one distance, de = 1 - 2^-24 each: every term lands on table point 1 (degenerate range:
    w = (0, 1, 0, 0)) with the same sign and nearly the largest magnitude.  With a fixed point of 2^38 the sum over the
    workgroups passes 2^63; the shift now gives up one bit per doubling of n beyond 2^24."""
    torch = K.torch
    n, T = (1 << 25) + (1 << 22), 64
    d = torch.full((n,), 0.3, dtype=torch.float32, device=K.dev)
    de = torch.full((n, 1), 1.0 - 2.0 ** -24, dtype=torch.float32, device=K.dev)
    rng_t = K.t(np.zeros(4, np.float32))
    K.call("ng_edge_table_range", n, 1, _p(d), _p(d), None, None, 0.0, _p(rng_t))
    r = K.get(rng_t)
    assert r[0] == np.float32(0.3) and r[1] > r[0]
    out = _scatter(K, n, 1, T, T, d, d, None, rng_t, de)
    del d, de
    expect = n * (1.0 - 2.0 ** -24)
    assert abs(float(out[1, 0]) - expect) <= 1e-6 * expect, (float(out[1, 0]), expect)
    assert np.all(np.delete(out[:, 0], 1) == 0)


def test_scatter_propagates_non_finite_gradients(K):
    """a NaN or inf de in a live slot makes the table's gradient non-finite (the per-edge backward would give NaN weight
    gradients); a NaN in a dead slot changes no bit"""
    T, E, n = 64, 3, 10000
    rng = np.random.default_rng(13)
    lo, hi, h = _grid(T)
    d = _grid_distances(T, n, rng, float(lo), h)
    d_src = d.copy()
    d_src[500:600] = 0.0
    de = rng.standard_normal((n, E)).astype(np.float32)
    rng_t = K.t(np.array([lo, hi, 0, 0], np.float32))
    g_src, g_eff = K.t(d_src), K.t(d)
    clean = _scatter(K, n, E, T, 2 * T, g_src, g_eff, None, rng_t, K.t(de))
    assert np.isfinite(clean).all(), np.argwhere(~np.isfinite(clean))[:8]
    i0, _ = _stencil64(d[77:78], lo, h, T)
    j = int(i0[0])
    for bad in (np.nan, np.inf, -np.inf):
        x = de.copy(); x[77, 1] = bad
        out = _scatter(K, n, E, T, 2 * T, g_src, g_eff, None, rng_t, K.t(x))
        assert not np.isfinite(out[j:j + 4, 1]).any(), (bad, j, out[j:j + 4], K.get(rng_t))
        assert np.all(out[T:] == 0), (bad, out[T:][out[T:] != 0][:8])
        x = de.copy(); x[550, 2] = bad                  # dead slot
        o2 = _scatter(K, n, E, T, 2 * T, g_src, g_eff, None, rng_t, K.t(x))
        assert np.array_equal(clean, o2), (bad, np.argwhere(clean != o2)[:8], K.get(rng_t))


# ------------------------------------------------------------------------------------------------------------ check
def _e_all(fn, T, E, lo=0.1, hi=0.5):
    h = (hi - lo) / (T - 3)
    x = np.concatenate([lo + (np.arange(T) - 1.0) * h, lo + (np.arange(T) - 0.5) * h])
    return fn(x[:, None] * np.ones(E) + 0.01 * np.arange(E)).astype(np.float32), np.array([lo, hi, 0, 0], np.float32)


def _check_ref(e_all, T):
    """float64 err (interior midpoints, the kernel's -1/16 9/16 9/16 -1/16 stencil on the fp32 values) and scale"""
    v = e_all.astype(np.float64)
    t = np.arange(1, T - 2)
    it = 0.5625 * (v[t] + v[t + 1]) - 0.0625 * (v[t - 1] + v[t + 2])
    return float(np.abs(it - v[T + t]).max()), float(np.abs(v[:T]).max())


def _check(K, T, E, e_all, tol, rng_t, cover=None, n_live=None, rows=None, prev=None):
    gate = K.t(np.full(8, -77, np.int32))
    K.call("ng_edge_table_check", T, E, _p(e_all), float(tol), _p(rng_t), _p(cover), _p(n_live), 2 * T if rows is None else rows,
           _p(prev), _p(gate))
    g = K.get(gate)
    return g, float(g[4:6].view(np.float32)[0]), float(g[4:6].view(np.float32)[1])


@pytest.mark.parametrize("T,E", [(8, 1), (64, 3), (2048, 8), (4096, 4)])
def test_check_err_scale_and_gate(K, T, E):
    n_live = K.t(np.array([12345], np.int32))
    cubic = lambda x: 3 * x ** 3 - 2 * x ** 2 + 0.5 * x - 0.25
    h = 0.4 / (T - 3)
    k = 0.6 / h                                       # k h = 0.6: a cubic midpoint error of ~ 3e-3 of the amplitude
    sine = lambda x: 1.5 * np.sin(k * x)
    for name, fn in (("cubic", cubic), ("sine", sine)):
        e_np, r_np = _e_all(fn, T, E)
        e_all, rng_t = K.t(e_np), K.t(r_np)
        err, sc = _check_ref(e_np, T)
        g, gerr, gsc = _check(K, T, E, e_all, 1.0, rng_t, n_live=n_live)
        assert gsc == sc, (name, gsc, sc)
        assert abs(gerr - err) <= 8 * 2.0 ** -24 * sc, (name, gerr, err)
        if name == "cubic":
            assert err <= 8 * 2.0 ** -24 * sc
            continue
        ratio = err / sc
        assert ratio > 1e-4, ratio
        g, _, _ = _check(K, T, E, e_all, ratio / 2, rng_t, n_live=n_live)
        assert list(g[:4]) == [1, 12345, 0, 0], g
        g, _, _ = _check(K, T, E, e_all, ratio * 2, rng_t, n_live=n_live)
        assert list(g[:4]) == [0, -1, 2 * T, 0], g
        assert g[6] == g[7] == -77


def test_check_raises_the_guard(K):
    T, E = 64, 3
    n_live = K.t(np.array([999], np.int32))
    e_np, r_np = _e_all(lambda x: np.exp(-x), T, E)
    rng_t = K.t(r_np)
    down = [0, -1, 2 * T, 0]
    up = [1, 999, 0, 0]
    g, err, sc = _check(K, T, E, K.t(e_np), 1e-3, rng_t, n_live=n_live)
    assert list(g[:4]) == down, g
    for row in (5, T - 1, T + 1, T + 9, 2 * T - 3):     # a table value or an interior midpoint not finite
        for bad in (np.nan, np.inf):
            x = e_np.copy(); x[row, 1] = bad
            assert list(_check(K, T, E, K.t(x), 1e-3, rng_t, n_live=n_live)[0][:4]) == up, (row, bad)
    # n_live NULL: the per-edge row count is 0 when up
    x = e_np.copy(); x[3, 0] = np.nan
    assert list(_check(K, T, E, K.t(x), 1e-3, rng_t)[0][:4]) == [1, 0, 0, 0]
    # the call's distances against the table's range: inside (bounds included) down, outside up
    for cov, bad in (((0.1, 0.5), False), ((0.2, 0.3), False), ((0.0999, 0.3), True), ((0.2, 0.5001), True), ((np.nan, 0.3), True)):
        cover = K.t(np.array([cov[0], cov[1], 0, 0], np.float32))
        g = _check(K, T, E, K.t(e_np), 1e-3, rng_t, cover=cover, n_live=n_live)[0]
        assert list(g[:4]) == (up if bad else down), cov
    # a gate decided earlier: bad stays bad
    prev_up = K.t(np.array([1, 999, 0, 0, 0, 0, 0, 0], np.int32))
    assert list(_check(K, T, E, K.t(e_np), 1e-3, rng_t, n_live=n_live, prev=prev_up)[0][:4]) == up


def test_check_of_the_range_only_reports_the_tables_err_and_scale(K):
    """a table kept over calls: later calls pass e_all = NULL, their distance range as cover and the table's own gate as prev;
    their gate carries the err and scale the table was built with"""
    T, E = 64, 2
    n_live = K.t(np.array([31], np.int32))
    e_np, r_np = _e_all(lambda x: np.cos(3 * x), T, E)
    rng_t = K.t(r_np)
    prev_np, err, sc = _check(K, T, E, K.t(e_np), 1e-3, rng_t, n_live=n_live)
    assert prev_np[0] == 0 and np.isfinite([err, sc]).all() and sc > 0
    prev = K.t(prev_np)
    for cov, bad in (((0.2, 0.3), 0), ((0.05, 0.3), 1)):
        cover = K.t(np.array([cov[0], cov[1], 0, 0], np.float32))
        g, gerr, gsc = _check(K, T, E, None, 0.0, rng_t, cover=cover, n_live=n_live, prev=prev)
        assert g[0] == bad and g[1] == (31 if bad else -1) and g[2] == (0 if bad else 2 * T), g
        assert (gerr, gsc) == (err, sc), (gerr, gsc, err, sc)
    # without prev: zeros, not whatever the words held
    cover = K.t(np.array([0.2, 0.3, 0, 0], np.float32))
    g, gerr, gsc = _check(K, T, E, None, 0.0, rng_t, cover=cover, n_live=n_live)
    assert g[0] == 0 and (gerr, gsc) == (0.0, 0.0)
