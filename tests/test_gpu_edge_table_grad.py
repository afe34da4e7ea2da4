"""ng_edge_table_dinput (csrc/edge_table.hip) called directly, against the float64 statement of tests/edge_table_grad_ref.py,
and the one change to ng_edge_mlp_dinput: a negative live count skips the launch.

The rounding bound, per slot: |dd - ref| <= (4 E + 8) 2^-24 sum_{k,c} |w_k J de|, the terms in float64 from the same float32
inputs.  What the kernel does to one term w_k J_kc de_c, in units of u = 2^-24 (first order):
  the weight      f - 1, f - 2, f + 1 are rounded (1 u each, at most three of them in a weight), then two or three rounded
                  products and the float32 constant 1/6: at most 6 u;
  the stencil     r_c = fma(w_k, J_kc, r_c) over k = 0 .. 3: a term goes through at most 4 roundings: 4 u;
  the dot         s = fma(de_c, r_c, s) over c: at most E roundings: E u.
(E + 10) u in all, which (4 E + 8) u covers for every E >= 1; the bound asserted is the one the interface states.  The
distances sit on a grid whose h is a power of two, so the float32 stencil position (u, i, f) is exact and the reference
reads the kernel's own rows and fraction."""
import ctypes as C

import numpy as np
import pytest

import edge_table_grad_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(123.0)


class _K:
    """the library context and the current stream; ``call(name, *args)`` checks the return code; ``t`` keeps every tensor it
    makes alive for the test"""

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


def _grid(T, lo=0.0625):
    """a range whose h is a power of two: the distances below, (d - lo) / h and the fraction f are exact in float32"""
    k = int(np.ceil(np.log2(T))) + 1
    h = 2.0 ** -k
    return np.float32(lo), np.float32(lo + (T - 3) * h), h


def _distances(T, n, rng, lo, hi, h):
    """lo + (j + m / 256) h over every cell, a fifth on table points; then the edges: exactly lo and hi, one ulp outside
    either, and the two clamped end cells (the first and the last cell of the range)"""
    j = rng.integers(0, T - 3, n)
    m = rng.integers(0, 256, n)
    m[rng.random(n) < 0.2] = 0
    d = (lo + (j + m / 256.0) * h).astype(np.float32)
    special = np.array([lo, hi, np.nextafter(np.float32(lo), np.float32(0)), np.nextafter(np.float32(hi), np.float32(1)),
                        lo + h / 256, lo + 0.5 * h, lo + 0.99609375 * h, lo + (T - 4) * h, lo + (T - 3.5) * h,
                        lo + (T - 3 - 1 / 256) * h, lo + h], np.float32)
    k = min(n, len(special))
    d[:k] = special[:k]
    return d, k


def _dinput(K, n, E, T, d_src, d_eff, pos, rng_t, tab, de, gate=None, fill=SENTINEL):
    out = K.t(np.full(n, fill, np.float32))
    K.call("ng_edge_table_dinput", n, E, T, _p(d_src), _p(d_eff), _p(pos), _p(rng_t), _p(tab), _p(gate), _p(de), _p(out))
    return K.get(out)


def _ref_chunked(d_src, d_eff, pos, lo, hi, T, tab, de, chunk=400_000):
    n = len(d_src)
    dd, mag = np.empty(n), np.empty(n)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        if pos is None:
            dd[a:b], mag[a:b] = R.table_dinput(d_src[a:b], d_eff[a:b], None, lo, hi, T, tab, de[a:b])
        else:       # compacted distances: the whole d_eff, indexed through the chunk's pos
            dd[a:b], mag[a:b] = R.table_dinput(d_src[a:b], d_eff, pos[a:b], lo, hi, T, tab, de[a:b])
    return dd, mag


@pytest.mark.parametrize("n", [1, 255, 1023, 1024, 1025, 4099, 2_500_001])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 8])
def test_table_dinput_against_float64(K, n, E):
    T = 4096 if E <= 4 else 2048
    rng = np.random.default_rng(n * 10 + E)
    lo, hi, h = _grid(T)
    d, n_special = _distances(T, n, rng, float(lo), float(hi), h)
    dead = rng.random(n) < 0.3
    dead[:n_special] = False
    if n > 20:
        dead[17] = False                                 # the huge row below is a live one
    d_src = d.copy()
    d_src[dead] = np.array([0.0, -0.0, -0.2, np.nan], np.float32)[rng.integers(0, 4, int(dead.sum()))]
    de = rng.standard_normal((n, E)).astype(np.float32)
    de[dead] = np.array([np.nan, 1e30], np.float32)[rng.integers(0, 2, (int(dead.sum()), E))]      # never read
    if n > 20:
        de[17] = np.float32(1e20) * np.sign(de[17])      # one huge row
    tab = (rng.standard_normal((T, E)) * 3).astype(np.float32)
    rng_t, g_tab, g_de, g_src = K.t(np.array([lo, hi, 0, 0], np.float32)), K.t(tab), K.t(de), K.t(d_src)
    for use_pos in (False, True):
        if use_pos:     # compacted distances: slot i's distance is d_eff[pos[i]], dead slots have no row (pos = -1)
            pos = rng.permutation(n).astype(np.int32)
            d_eff = np.full(n, np.nan, np.float32)
            d_eff[pos] = d
            pos[dead] = -1
            g_pos = K.t(pos)
        else:
            pos, d_eff, g_pos = None, d, None
        g_eff = K.t(d_eff)
        dd = _dinput(K, n, E, T, g_src, g_eff, g_pos, rng_t, g_tab, g_de)
        ref, mag = _ref_chunked(d_src, d_eff, pos, lo, hi, T, tab, de)
        # dead slots of every kind: the bits of +0.0f, whatever their de holds and whatever dd_out held
        assert np.all(dd[dead].view(np.uint32) == 0), use_pos
        live = ~dead
        err = np.abs(dd[live].astype(np.float64) - ref[live])
        bound = (4 * E + 8) * 2.0 ** -24 * mag[live]
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        print(f"n={n} E={E} pos={use_pos}: max err / bound = {ratio:.3f}")
        assert np.all(err <= bound), (use_pos, ratio)
        assert np.all(np.isfinite(dd))
        # the same bits on a second launch
        assert np.array_equal(dd.view(np.uint32), _dinput(K, n, E, T, g_src, g_eff, g_pos, rng_t, g_tab, g_de).view(np.uint32))
    # at lo and at hi the stencil sits on table points 1 and T - 2: J of that row, no interpolation error at all
    if n >= 2:
        for slot, row in ((0, 1), (1, T - 2)):
            exact = float(np.sum(np.float64(de[slot]) * np.float64(tab[row])))
            assert abs(dd[slot] - exact) <= (E + 1) * 2.0 ** -24 * float(np.sum(np.abs(np.float64(de[slot]) * tab[row])))


@pytest.mark.parametrize("E,T", [(3, 4096), (8, 2048), (2, 64)])
def test_table_dinput_gate(K, E, T):
    """gate[0] != 0: the per-edge launch answered the call, dd_out is not touched; gate[0] == 0 and gate == NULL: written"""
    n = 5000
    rng = np.random.default_rng(E)
    lo, hi, h = _grid(T)
    d, _ = _distances(T, n, rng, float(lo), float(hi), h)
    rng_t, tab = K.t(np.array([lo, hi, 0, 0], np.float32)), K.t(rng.standard_normal((T, E)).astype(np.float32))
    de = K.t(rng.standard_normal((n, E)).astype(np.float32))
    up = K.t(np.array([1, 7, 0, 0, 0, 0, 0, 0], np.int32))
    down = K.t(np.array([0, -1, 2 * T, 0, 0, 0, 0, 0], np.int32))
    g_d = K.t(d)
    assert np.all(_dinput(K, n, E, T, g_d, g_d, None, rng_t, tab, de, gate=up) == SENTINEL)
    open_ = _dinput(K, n, E, T, g_d, g_d, None, rng_t, tab, de)
    assert np.array_equal(_dinput(K, n, E, T, g_d, g_d, None, rng_t, tab, de, gate=down), open_)
    assert not np.any(open_ == SENTINEL)


def test_table_dinput_refuses_bad_arguments(K):
    from nmrgnn_amd._lib import NGError
    x = K.t(np.ones(64, np.float32))
    for E, T in ((0, 64), (9, 64), (8, 4096), (3, 4)):
        with pytest.raises(NGError, match="edge_table_dinput"):
            K.call("ng_edge_table_dinput", 4, E, T, _p(x), _p(x), None, _p(x), _p(x), None, _p(x), _p(x))
    with pytest.raises(NGError, match="edge_table_dinput"):
        K.call("ng_edge_table_dinput", 4, 3, 8, _p(x), _p(x), None, _p(x), _p(x), None, None, _p(x))
    K.call("ng_edge_table_dinput", 0, 3, 8, None, None, None, None, None, None, None, None)      # nothing to do


# ------------------------------------------------------------------------------------------- ng_edge_mlp_dinput, n_live < 0
def _mlp_dinput(K, c, H, E, Le, d_src, d_eff, perm, n_live):
    from nmrgnn_amd._lib import ptr_array
    n = len(d_src)
    W = [K.t(w) for w in c["W"]]
    B = [K.t(b) for b in c["B"]]
    J, dd = K.t(np.full((n, E), SENTINEL, np.float32)), K.t(np.full(n, SENTINEL, np.float32))
    K.call("ng_edge_mlp_dinput", n, H, E, Le, 1, _p(K.t(d_src)), _p(K.t(d_eff)), _p(None if perm is None else K.t(perm)),
           _p(None if n_live is None else K.t(np.array([n_live], np.int32))), _p(K.t(c["centers"])), float(c["gap"]),
           ptr_array(W), ptr_array(B), _p(K.t(c["de"])), _p(J), _p(dd))
    return K.get(J), K.get(dd)


def test_edge_mlp_dinput_negative_live_count_skips_the_launch(K):
    """*n_live = -1: J_out and dd_out keep what they held; *n_live = 0 and > 0: the bits of the every-slot form on the same
    rows (rows past the count dead)"""
    from nmrgnn_amd.engine import rbf_grid
    H, E, Le, n = 128, 3, 4, 1000
    rng = np.random.default_rng(5)
    centers, gap = rbf_grid(0.005, 0.20, H)
    c = dict(centers=centers, gap=gap, W=[], B=[], de=rng.standard_normal((n, E)).astype(np.float32))
    for t in range(Le):
        kout = H if t < Le - 1 else E
        c["W"].append((rng.standard_normal((H, kout)) * np.sqrt(2.0 / (H + kout))).astype(np.float32))
        c["B"].append((0.1 * rng.standard_normal(kout)).astype(np.float32))
    d_slot = rng.uniform(0.01, 0.21, n).astype(np.float32)
    d_slot[rng.random(n) < 0.2] = 0.0
    live = np.nonzero(d_slot > 0)[0]
    perm = np.concatenate([live, np.nonzero(~(d_slot > 0))[0]]).astype(np.int32)
    d_c = np.full(n, np.nan, np.float32)          # rows past the live ones are never read
    d_c[:len(live)] = d_slot[live]
    J, dd = _mlp_dinput(K, c, H, E, Le, d_c, d_c, perm, -1)
    assert np.all(J == SENTINEL) and np.all(dd == SENTINEL)
    for k in (0, 37, len(live)):
        J, dd = _mlp_dinput(K, c, H, E, Le, d_c, d_c, perm, k)
        d_k = np.zeros(n, np.float32)
        d_k[perm[:k]] = d_slot[perm[:k]]
        Js, dds = _mlp_dinput(K, c, H, E, Le, d_k, d_k, None, None)
        assert np.array_equal(J.view(np.uint32), Js.view(np.uint32)), k
        assert np.array_equal(dd.view(np.uint32), dds.view(np.uint32)), k
        assert (k == 0) == (not np.any(dd != 0))
