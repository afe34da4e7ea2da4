"""The neighbour-list builders against the exact integer reference of tests/nlist_ref.py, bit for bit: every kernel of knn.hip,
knn_cells.hip, cutoff.hip, ragged.hip and ng_exclusive_scan_i32, at the sizes where the dispatch changes.

Positions are multiples of 1/8 (box lengths powers of two), where the kernels' float32 distance expression is exact however it
is rounded (nlist_ref.check_exact_domain, asserted on every case's own data), so every output is compared with
assert_array_equal: every slot of every row, ties included, the distances sqrtf(d2) * scale, inv_degree, CSR rows in order.
Frames of up to 4097 atoms are compared row by row; larger ones row by row on 2048 rows (the first 256, the last 256, 1536
seeded) and by the row-wise invariants on every row.  Outputs are pre-filled with a sentinel, so an unwritten entry fails.
Case ids name the branch taken; where NG_KNN does not force it, the profile scope names say which family ran."""
import ctypes as C
import functools

import numpy as np
import pytest

import nlist_ref as R

pytestmark = pytest.mark.gpu
SCALE = 0.1
FAMS = ("ties", "spread")


# ------------------------------------------------------------------------------------------------ data and references, shared
@functools.lru_cache(maxsize=None)
def _open_frame(fam, n, seed):
    return R.family(fam, n, seed), None


@functools.lru_cache(maxsize=None)
def _box_frame(n, seed, diag, off, kind):
    return R.periodic_family(n, seed, diag, off, kind=kind)


@functools.lru_cache(maxsize=None)
def _top(key):
    """(rows, top_j, top_d2) of a frame for K up to 64: every row up to 4097 atoms, the 2048 sampled rows above"""
    q8, box8 = _frame_of(key)
    n = len(q8)
    rows = np.arange(n) if n <= 4097 else R.sample_rows(n, 17)
    j, d2 = R.knn_top(q8, 64, box8, rows)
    return rows, j, d2


def _frame_of(key):
    return _open_frame(*key[1:]) if key[0] == "open" else _box_frame(*key[1:])


def _okey(fam, n, seed=0):
    return ("open", fam, n, seed)


def _bkey(n, seed, diag, off=(0, 0, 0), kind="spread"):
    return ("box", n, seed, tuple(diag), tuple(off), kind)


def _three(make, G):
    """G frames: three different ones in turn, so that the frame offsets take part and the reference is computed three times"""
    return [make(g % 3) for g in range(G)]


# ------------------------------------------------------------------------------------------------ the C entry points
def _ctx():
    from nmrgnn_amd import _lib
    return _lib.get_context(0)


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev_pos(dev, keys):
    import torch
    return torch.from_numpy(np.stack([R.positions_f32(_frame_of(k)[0]) for k in keys])).to(dev)


def _dev_box(dev, keys):
    import torch
    return torch.from_numpy(np.stack([R.box_f32(_frame_of(k)[1]) for k in keys])).to(dev)


def _is_tric(keys):
    return any(_frame_of(k)[1][[3, 6, 7]].any() for k in keys)


def _scopes(fn):
    ctx = _ctx()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        names = set(ctx.prof_read())
    finally:
        ctx.prof_enable(False)
    return out, names


def _knn_gpu(dev, keys, K):
    import torch
    from nmrgnn_amd._lib import ptr
    G, n = len(keys), len(_frame_of(keys[0])[0])
    pos = _dev_pos(dev, keys)
    nl = torch.full((G * n, K), -7, dtype=torch.int32, device=dev)
    ed = torch.full((G * n, K), float("nan"), device=dev)
    inv = torch.full((G * n,), float("nan"), device=dev)
    ctx = _ctx()
    if keys[0][0] == "open":
        ctx.check(ctx.lib.ng_knn_graph(ctx.handle, _stream(dev), G, n, K, SCALE, ptr(pos), ptr(nl), ptr(ed), ptr(inv)), "knn")
    else:
        box = _dev_box(dev, keys)
        ctx.check(ctx.lib.ng_knn_graph_pbc(ctx.handle, _stream(dev), G, n, K, SCALE, ptr(pos), ptr(box), int(_is_tric(keys)),
                                           ptr(nl), ptr(ed), ptr(inv)), "knn_pbc")
    torch.cuda.synchronize()
    return nl.cpu().numpy(), ed.cpu().numpy(), inv.cpu().numpy()


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("NG_KNN", raising=False)
    else:
        monkeypatch.setenv("NG_KNN", mode)


def _assert_knn(got, keys, K):
    nl, ed, inv = got
    n = len(_frame_of(keys[0])[0])
    assert nl.shape == (len(keys) * n, K)
    for g, key in enumerate(keys):
        q8, box8 = _frame_of(key)
        rows, tj, td = _top(key)
        kk = min(K, n - 1)
        R.check_exact_domain(q8, box8, kth_d2=td[:, kk - 1] if kk else None)
        want = R.knn_format(tj, td, K, base=g * n, scale=SCALE)
        sl = g * n + rows
        np.testing.assert_array_equal(nl[sl], want[0], err_msg=f"nlist, frame {g}")
        np.testing.assert_array_equal(ed[sl], want[1], err_msg=f"edges, frame {g}")
        np.testing.assert_array_equal(inv[sl], want[2], err_msg=f"inv_degree, frame {g}")
        if len(rows) < n:                                  # a large frame: every row by the invariants
            fr = slice(g * n, (g + 1) * n)
            d2 = R.check_knn_rows(q8, K, nl[fr], ed[fr], inv[fr], box8, base=g * n, scale=SCALE)
            assert d2.max() < R.EXACT


def _run_knn_case(gpu_device, monkeypatch, mode, keys, K, scope=None):
    _set_mode(monkeypatch, mode)
    got, names = _scopes(lambda: _knn_gpu(gpu_device, keys, K))
    scope = scope or "knn_graph"                          # NG_KNN=serial / lanes: a brute-force kernel, never the cell grid
    assert scope in names and ({"knn_graph", "knn_cells_query"} - {scope}).isdisjoint(names), names
    _assert_knn(got, keys, K)


def _case(name, mode, n, G, K, scope="knn_graph", fams=FAMS):
    return [pytest.param(mode, fam, n, G, K, scope, id=f"{name}-n{n}-G{G}-K{K}-{fam}") for fam in fams]


# ------------------------------------------------------------------------------------------------ kNN, open boundaries
OPEN = []
for _n in (1024, 1025, 2048, 2049, 3072, 3073, 4096):                       # the template switch of the wave kernel
    OPEN += _case(f"wave_steps{16 * -(-_n // 1024)}", None, _n, 1, 16)
for _K in (1, 17, 64):
    OPEN += _case("wave_steps64", None, 4096, 1, _K)
OPEN += _case("wave_16384_rows", None, 1024, 16, 16) + _case("wave_16384_rows", None, 4096, 4, 16)
for _n in (1, 2, 17, 64, 65, 66):                                            # fewer than K occupied lanes, n - 1 < K
    for _K in (16, 64):
        OPEN += _case("wave_few_minima", None, _n, 1, _K)
for _n in (4097, 5000):
    OPEN += _case("lanes16_default", None, _n, 1, 16)
for _n in (15, 16, 17, 1023, 1024, 1025, 2049):
    OPEN += _case("lanes16_forced", "lanes", _n, 1, 16, None)
for _n, _G in ((1025, 16), (4096, 5), (5462, 3)):
    for _K in (1, 5, 16):
        OPEN += _case("lanes8_default", None, _n, _G, _K)
for _K in (1, 16, 17, 32, 33, 64):
    for _n in (255, 256, 257, 1024, 1025, 2049):
        OPEN += _case(f"serial_kmax{16 if _K <= 16 else 32 if _K <= 32 else 64}", "serial", _n, 1, _K, None)
for _K in (17, 40, 64):
    OPEN += _case("serial_default", None, 4097, 1, _K) + _case("serial_default", None, 1025, 16, _K)
for _K in (16, 32, 64):
    OPEN += _case("serial_n_le_K", "serial", _K, 1, _K, None) + _case("serial_n_le_K", "serial", _K - 3, 3, _K, None)
for _K in (16, 17, 33, 64):
    OPEN += _case("cells_gate_refuses", "cells", 63, 1, _K)
    for _n in (64, 65, 300, 4097):
        OPEN += _case(f"cells_kmax{16 if _K <= 16 else 32 if _K <= 32 else 64}", "cells", _n, 1, _K, "knn_cells_query")
for _fam in ("plane", "line", "point", "blobs", "offset"):
    for _K in (16, 64):
        OPEN += _case("cells_shape", "cells", 4096, 1, _K, "knn_cells_query", fams=(_fam,))
OPEN += _case("cells_frames", "cells", 300, 3, 16, "knn_cells_query") + _case("cells_frames", "cells", 1500, 3, 40, "knn_cells_query")
OPEN += _case("brute_below_16384", None, 16383, 1, 16) + _case("cells_from_16384", None, 16384, 1, 16, "knn_cells_query")


@pytest.mark.parametrize("mode,fam,n,G,K,scope", OPEN)
def test_knn_open(gpu_device, monkeypatch, mode, fam, n, G, K, scope):
    keys = _three(lambda s: _okey(fam, n, s), G)
    _run_knn_case(gpu_device, monkeypatch, mode, keys, K, scope)


# ------------------------------------------------------------------------------------------------ kNN, periodic boxes
ORTHO, TRIC = (0, 0, 0), None
TRIC_OFF = {(16, 16, 16): (32, -40, 24), (32, 16, 16): (-128, 64, 24), (32, 32, 16): (64, -96, 56), (32, 32, 32): (64, -128, 48),
            (32, 32, 8): (64, -40, 24), (8, 16, 32): (-24, 32, 64), (16, 16, 8): (64, -64, 64), (8, 8, 8): (16, -24, 8),
            (16, 8, 8): (-64, 40, 32), (32, 16, 8): (128, -96, 64)}


def _pcase(name, mode, n, G, K, diag, tric, scope="knn_graph", kind="spread"):
    off = TRIC_OFF[diag] if tric else ORTHO
    tag = "tric" if tric else "ortho"
    cid = f"{name}-{tag}-n{n}-G{G}-K{K}-box{diag[0]}x{diag[1]}x{diag[2]}-{kind}"
    if scope == "knn_cells_query":
        box8 = np.array([diag[0] * 8, 0, 0, off[0], diag[1] * 8, 0, off[1], off[2], diag[2] * 8])
        cid += "-cells%dx%dx%d" % R.grid_cells(n, K, box8)
    return pytest.param(mode, n, G, K, diag, off, kind, scope, id=cid)


PERIODIC = []
for _t in (False, True):
    for _n, _d in ((700, (16, 16, 16)), (1100, (32, 16, 16)), (2100, (32, 32, 16)), (3100, (32, 32, 32))):
        PERIODIC.append(_pcase(f"wave_steps{16 * -(-_n // 1024)}", None, _n, 1, 16, _d, _t))
    PERIODIC.append(_pcase("wave_steps16", None, 700, 1, 64, (16, 16, 16), _t, kind="ties"))
    PERIODIC.append(_pcase("lanes16_forced", "lanes", 1025, 1, 16, (32, 16, 16), _t))
    PERIODIC.append(_pcase("lanes8_default", None, 1025, 17, 16, (32, 16, 16), _t))
    PERIODIC.append(_pcase("serial_kmax16", "serial", 700, 1, 16, (16, 16, 16), _t))
    PERIODIC.append(_pcase("serial_kmax32", "serial", 700, 1, 17, (16, 16, 16), _t))
    PERIODIC.append(_pcase("serial_kmax64", "serial", 700, 3, 64, (16, 16, 16), _t))
    PERIODIC.append(_pcase("cells_kmax32", "cells", 64, 1, 17, (8, 16, 32), _t, "knn_cells_query"))
    for _K in (16, 40):
        PERIODIC.append(_pcase("cells", "cells", 64, 1, _K, (8, 16, 32), _t, "knn_cells_query"))
        PERIODIC.append(_pcase("cells", "cells", 64, 1, _K, (8, 8, 8), _t, "knn_cells_query", kind="ties"))
        PERIODIC.append(_pcase("cells", "cells", 300, 1, _K, (16, 16, 8), _t, "knn_cells_query"))
        PERIODIC.append(_pcase("cells", "cells", 300, 3, _K, (32, 16, 8), _t, "knn_cells_query"))
        PERIODIC.append(_pcase("cells", "cells", 4097, 1, _K, (32, 32, 32), _t, "knn_cells_query"))
# the 27-image search for most pairs (a box thin along c: images two cells up and down win), and for none
PERIODIC.append(_pcase("wave_steps32_search_always", None, 1100, 1, 16, (32, 32, 8), True))
PERIODIC.append(_pcase("serial_kmax16_search_always", "serial", 1100, 1, 16, (32, 32, 8), True))
PERIODIC.append(_pcase("cells_search_always", "cells", 1100, 1, 16, (32, 32, 8), True, "knn_cells_query"))
PERIODIC.append(_pcase("wave_steps16_search_never", None, 700, 1, 16, (32, 32, 32), True, kind="cluster"))


@pytest.mark.parametrize("mode,n,G,K,diag,off,kind,scope", PERIODIC)
def test_knn_periodic(gpu_device, monkeypatch, mode, n, G, K, diag, off, kind, scope):
    keys = _three(lambda s: _bkey(n, s, diag, off, kind), G)
    _run_knn_case(gpu_device, monkeypatch, mode, keys, K, scope)


# ------------------------------------------------------------------------------------------------ cutoff graphs
def _cutoff_gpu(dev, keys, cutoff):
    """count, scan, fill with row_of, through the C entry points -> dict of host arrays and the scope names"""
    import torch
    from nmrgnn_amd._lib import ptr
    G, n = len(keys), len(_frame_of(keys[0])[0])
    N = G * n
    pos = _dev_pos(dev, keys)
    ctx, st = _ctx(), _stream(dev)
    boxed = keys[0][0] == "box"
    box, tric = (_dev_box(dev, keys), int(_is_tric(keys))) if boxed else (None, 0)
    deg = torch.full((N,), -7, dtype=torch.int32, device=dev)
    if boxed:
        ctx.check(ctx.lib.ng_cutoff_count_pbc(ctx.handle, st, G, n, cutoff, ptr(pos), ptr(box), tric, ptr(deg)), "count_pbc")
    else:
        ctx.check(ctx.lib.ng_cutoff_count(ctx.handle, st, G, n, cutoff, ptr(pos), ptr(deg)), "count")
    row_ptr = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.ng_exclusive_scan_i32(ctx.handle, st, N, ptr(deg), ptr(row_ptr)), "scan")
    nnz = int(row_ptr[-1])
    assert 0 <= nnz == int(deg.sum(dtype=torch.int64))
    col = torch.full((nnz + 8,), -7, dtype=torch.int32, device=dev)          # 8 slots of slack: nothing is written past nnz
    dist = torch.full((nnz + 8,), float("nan"), device=dev)
    row_of = torch.full((nnz + 8,), -7, dtype=torch.int32, device=dev)
    inv = torch.full((N,), float("nan"), device=dev)
    if boxed:
        ctx.check(ctx.lib.ng_cutoff_fill_rows_pbc(ctx.handle, st, G, n, cutoff, SCALE, ptr(pos), ptr(box), tric, ptr(row_ptr),
                                                  ptr(col), ptr(dist), ptr(inv), ptr(row_of)), "fill_pbc")
    else:
        ctx.check(ctx.lib.ng_cutoff_fill_rows(ctx.handle, st, G, n, cutoff, SCALE, ptr(pos), ptr(row_ptr), ptr(col), ptr(dist),
                                              ptr(inv), ptr(row_of)), "fill")
    torch.cuda.synchronize()
    assert (col[nnz:] == -7).all() and (row_of[nnz:] == -7).all() and torch.isnan(dist[nnz:]).all()
    return dict(deg=deg.cpu().numpy(), row_ptr=row_ptr.cpu().numpy(), col=col[:nnz].cpu().numpy(), dist=dist[:nnz].cpu().numpy(),
                inv_degree=inv.cpu().numpy(), row_of=row_of[:nnz].cpu().numpy())


@functools.lru_cache(maxsize=None)
def _cutoff_ref(key, cutoff):
    q8, box8 = _frame_of(key)
    R.check_exact_domain(q8, box8, cutoff=cutoff)
    return R.cutoff(q8, cutoff, box8, 0, SCALE)


def _assert_cutoff(got, keys, cutoff):
    n = len(_frame_of(keys[0])[0])
    parts = [_cutoff_ref(k, cutoff) for k in keys]
    deg = np.concatenate([p[0] for p in parts])
    want = dict(deg=deg, row_ptr=R.scan(deg), col=np.concatenate([p[1] + g * n for g, p in enumerate(parts)]),
                dist=np.concatenate([p[2] for p in parts]), inv_degree=np.concatenate([p[3] for p in parts]),
                row_of=np.repeat(np.arange(len(deg), dtype=np.int32), deg))
    for name in ("deg", "row_ptr", "col", "dist", "inv_degree", "row_of"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    return want


# (family, cutoff): 3.0 on the whole-Angstrom grids, where many pairs sit exactly at the cutoff and stay out; 2.5; 3.2, whose
# float32 square is rounded; 0.9 on distinct whole-Angstrom sites: below the smallest spacing, every row empty
CUTS = (("ties", 3.0), ("spread", 2.5), ("spread", 3.2), ("distinct", 0.9))
CUTOFF = []


def _ccase(name, mode, n, G, cuts=CUTS):
    return [pytest.param(mode, fam, c, n, G, id=f"{name}-n{n}-G{G}-{fam}-cut{c}") for fam, c in cuts]


for _n in (1, 2, 63, 64, 65, 1024, 1025, 4096):
    CUTOFF += _ccase("wave", None, _n, 1)
CUTOFF += _ccase("wave_16384_rows", None, 4096, 4, CUTS[1:])
for _n in (15, 16, 17, 63, 64, 65, 1023, 1024, 1025):
    CUTOFF += _ccase("lanes16_forced", "lanes", _n, 1)
CUTOFF += _ccase("lanes16_default", None, 4097, 1) + _ccase("lanes16_default", None, 1025, 16, CUTS[1:])
for _n in (255, 256, 257, 1024, 1025, 2049):
    CUTOFF += _ccase("serial", "serial", _n, 1)
for _name, _mode in (("wave", None), ("lanes16_forced", "lanes"), ("serial", "serial")):      # the j > 0 rule of inv_degree
    CUTOFF += _ccase(_name + "_atom0", _mode, 130, 1, (("atom0", 3.2), ("atom0far", 3.2)))
    CUTOFF += _ccase(_name + "_atom0", _mode, 130, 3, (("atom0", 3.2),))


@pytest.mark.parametrize("mode,fam,cutoff,n,G", CUTOFF)
def test_cutoff_open(gpu_device, monkeypatch, mode, fam, cutoff, n, G):
    keys = _three(lambda s: _okey(fam, n, s), G)
    _set_mode(monkeypatch, mode)
    got, names = _scopes(lambda: _cutoff_gpu(gpu_device, keys, cutoff))
    assert {"cutoff_count", "exclusive_scan", "cutoff_fill"} <= names, names
    want = _assert_cutoff(got, keys, cutoff)
    if fam == "distinct":
        assert not want["deg"].any() and not want["inv_degree"].any()
    if fam == "ties" and n >= 63:                          # pairs exactly at the cutoff exist and are excluded
        q8 = _frame_of(keys[0])[0]
        assert (R.d2_rows(q8, np.arange(min(n, 64))) == 9 * 64).any()
    if fam == "atom0":                                     # atom 0 is a neighbour of most rows, and never counts
        listed0 = (got["col"] % n == 0).sum()
        assert listed0 > 0.5 * (n - 1) * G
        uncounted = got["inv_degree"] != R.inv_degree_value(got["deg"])
        assert uncounted.sum() == listed0
    if fam == "atom0far":
        assert got["deg"][0] == 0 and got["inv_degree"][0] == 0 and not (got["col"] == 0).any()


CUTOFF_P = []
for _name, _mode, _n, _G in (("wave", None, 700, 1), ("lanes16_forced", "lanes", 700, 3), ("serial", "serial", 700, 1),
                             ("lanes16_default", None, 1025, 17)):
    CUTOFF_P.append(pytest.param(_mode, _n, _G, (16, 16, 16), ORTHO, "ties", 3.0, id=f"{_name}-ortho-n{_n}-G{_G}-ties-cut3.0"))
    CUTOFF_P.append(pytest.param(_mode, _n, _G, (16, 16, 16), TRIC_OFF[(16, 16, 16)], "spread", 3.2,
                                 id=f"{_name}-tric-n{_n}-G{_G}-spread-cut3.2"))
    CUTOFF_P.append(pytest.param(_mode, _n, _G, (32, 32, 8), TRIC_OFF[(32, 32, 8)], "spread", 2.5,
                                 id=f"{_name}-tric_thin-n{_n}-G{_G}-spread-cut2.5"))


@pytest.mark.parametrize("mode,n,G,diag,off,kind,cutoff", CUTOFF_P)
def test_cutoff_periodic(gpu_device, monkeypatch, mode, n, G, diag, off, kind, cutoff):
    keys = _three(lambda s: _bkey(n, s, diag, off, kind), G)
    for k in keys:
        assert cutoff < 0.5 * R.widths(_frame_of(k)[1]).min() * (1 - 1e-9)      # as the entry point requires
    _set_mode(monkeypatch, mode)
    got, names = _scopes(lambda: _cutoff_gpu(gpu_device, keys, cutoff))
    assert {"cutoff_count", "exclusive_scan", "cutoff_fill"} <= names, names
    _assert_cutoff(got, keys, cutoff)


# ------------------------------------------------------------------------------------------------ ragged batches
RAGGED_TOP = {16: (1024,), 32: (1024, 1025), 48: (1024, 1025, 2100), 64: (1024, 1025, 4096)}


def _ragged_keys(K, steps=64, boxed=True):
    """structures of 1, 2, K, K + 1, 255, 256, 257, 1024, 1025 and 4096 atoms, boundaries cycling open / orthorhombic /
    triclinic, each in a box of its own size (``boxed`` = False: all open).  The largest structure sizes the wave kernel's
    template: ``steps`` = 16, 32 and 48 end the list at 1024, 1025 and 2100 atoms instead"""
    keys = []
    for g, n in enumerate((1, 2, K, K + 1, 255, 256, 257) + RAGGED_TOP[steps]):
        diag = (8, 8, 8) if n <= 64 else (16, 16, 8) if n <= 257 else (32, 16, 16) if n <= 1025 else (32, 32, 32)
        kinds = ("ties", "spread")
        if g % 3 == 0 or not boxed:
            keys.append(_okey(kinds[g % 2], n, g))
        else:
            keys.append(_bkey(n, g, diag, ORTHO if g % 3 == 1 else TRIC_OFF[diag], kinds[g % 2]))
    return keys


def _ragged_inputs(dev, keys):
    import torch
    sizes = [len(_frame_of(k)[0]) for k in keys]
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pos = torch.from_numpy(np.concatenate([R.positions_f32(_frame_of(k)[0]) for k in keys])).to(dev)
    kind = np.array([-1 if k[0] == "open" else int(_frame_of(k)[1][[3, 6, 7]].any()) for k in keys], np.int32)
    box = np.stack([np.zeros(9, np.float32) if k[0] == "open" else R.box_f32(_frame_of(k)[1]) for k in keys])
    return sizes, gp, pos, kind, torch.from_numpy(box).to(dev), torch.from_numpy(kind).to(dev), torch.from_numpy(gp).to(dev)


def _run_ragged_knn(dev, K, steps, boxed):
    """the structures of _ragged_keys through ng_knn_graph_ragged_pbc (``boxed``) or ng_knn_graph_ragged, every structure
    against the reference directly"""
    import torch
    from nmrgnn_amd._lib import ptr
    keys = _ragged_keys(K, steps, boxed)
    sizes, gp, pos, kind_host, box, kind, gp_dev = _ragged_inputs(dev, keys)
    assert 64 * (steps // 16 - 1) * 16 < max(sizes) <= 64 * steps
    N = int(gp[-1])
    nl = torch.full((N, K), -7, dtype=torch.int32, device=dev)
    ed = torch.full((N, K), float("nan"), device=dev)
    inv = torch.full((N,), float("nan"), device=dev)
    ctx = _ctx()

    def call():
        if boxed:
            ctx.check(ctx.lib.ng_knn_graph_ragged_pbc(ctx.handle, _stream(dev), len(keys), N, K, SCALE, ptr(pos), ptr(gp_dev),
                                                      C.c_void_p(gp.ctypes.data), max(sizes), ptr(box), ptr(kind),
                                                      C.c_void_p(kind_host.ctypes.data), ptr(nl), ptr(ed), ptr(inv)),
                      "knn_ragged_pbc")
        else:
            assert (kind_host == -1).all()
            ctx.check(ctx.lib.ng_knn_graph_ragged(ctx.handle, _stream(dev), len(keys), N, K, SCALE, ptr(pos), ptr(gp_dev),
                                                  C.c_void_p(gp.ctypes.data), max(sizes), ptr(nl), ptr(ed), ptr(inv)),
                      "knn_ragged")
        torch.cuda.synchronize()

    # the scope says which displacement policy the kernels were built with: DispPer behind _pbc, DispOpen behind the open entry
    _, names = _scopes(call)
    scope, other = ("knn_graph_ragged_pbc", "knn_graph_ragged") if boxed else ("knn_graph_ragged", "knn_graph_ragged_pbc")
    assert scope in names and other not in names and "knn_cells_query" not in names, names
    nl, ed, inv = nl.cpu().numpy(), ed.cpu().numpy(), inv.cpu().numpy()
    for g, key in enumerate(keys):
        q8, box8 = _frame_of(key)
        rows, tj, td = _top(key)
        kk = min(K, sizes[g] - 1)
        R.check_exact_domain(q8, box8, kth_d2=td[:, kk - 1] if kk else None)
        want = R.knn_format(tj, td, K, base=int(gp[g]), scale=SCALE)
        sl = slice(gp[g], gp[g + 1])
        np.testing.assert_array_equal(nl[sl], want[0], err_msg=f"nlist, structure {g} (n={sizes[g]})")
        np.testing.assert_array_equal(ed[sl], want[1], err_msg=f"edges, structure {g} (n={sizes[g]})")
        np.testing.assert_array_equal(inv[sl], want[2], err_msg=f"inv_degree, structure {g} (n={sizes[g]})")


@pytest.mark.parametrize("steps", [16, 32, 48, 64], ids=lambda v: f"wave_per_row_steps{v}")
@pytest.mark.parametrize("K", [16, 40], ids=["thread_per_row_kmax16-K16", "thread_per_row_kmax64-K40"])
def test_ragged_knn(gpu_device, monkeypatch, K, steps):
    """knn_ragged_kernel (structures up to 256 atoms) and knn_ragged_wave_kernel (257 .. 4096, its template sized by the largest
    structure) through ng_knn_graph_ragged_pbc"""
    monkeypatch.delenv("NG_KNN", raising=False)
    _run_ragged_knn(gpu_device, K, steps, True)


@pytest.mark.parametrize("boxed", [True, False], ids=["pbc_entry", "open_entry"])
def test_ragged_knn_kmax32(gpu_device, monkeypatch, boxed):
    """K = 17: the 32-slot lists of knn_ragged_kernel for both displacement policies; the open entry point with a largest
    structure of 2100 atoms also runs the open knn_ragged_wave_kernel of 48 steps"""
    monkeypatch.delenv("NG_KNN", raising=False)
    _run_ragged_knn(gpu_device, 17, 48, boxed)


def test_ragged_cutoff(gpu_device, monkeypatch):
    """cutoff_ragged_kernel, count and fill, through the _pbc entry points: every structure against the reference directly"""
    import torch
    from nmrgnn_amd._lib import ptr
    monkeypatch.delenv("NG_KNN", raising=False)
    dev, cutoff = gpu_device, 3.0
    keys = _ragged_keys(16)
    sizes, gp, pos, kind_host, box, kind, gp_dev = _ragged_inputs(dev, keys)
    N, G = int(gp[-1]), len(keys)
    ctx, st, kh = _ctx(), _stream(dev), C.c_void_p(kind_host.ctypes.data)
    deg = torch.full((N,), -7, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.ng_cutoff_count_ragged_pbc(ctx.handle, st, G, N, cutoff, ptr(pos), ptr(gp_dev), max(sizes), ptr(box),
                                                 ptr(kind), kh, ptr(deg)), "count_ragged_pbc")
    row_ptr = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.ng_exclusive_scan_i32(ctx.handle, st, N, ptr(deg), ptr(row_ptr)), "scan")
    nnz = int(row_ptr[-1])
    col = torch.full((nnz + 8,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((nnz + 8,), float("nan"), device=dev)
    row_of = torch.full((nnz + 8,), -7, dtype=torch.int32, device=dev)
    inv = torch.full((N,), float("nan"), device=dev)
    ctx.check(ctx.lib.ng_cutoff_fill_rows_ragged_pbc(ctx.handle, st, G, N, cutoff, SCALE, ptr(pos), ptr(gp_dev), max(sizes),
                                                     ptr(box), ptr(kind), kh, ptr(row_ptr), ptr(col), ptr(dist), ptr(inv),
                                                     ptr(row_of)), "fill_ragged_pbc")
    torch.cuda.synchronize()
    assert (col[nnz:] == -7).all() and (row_of[nnz:] == -7).all()
    parts = []
    for g, key in enumerate(keys):
        q8, box8 = _frame_of(key)
        if box8 is not None:
            assert cutoff < 0.5 * R.widths(box8).min()
        p = _cutoff_ref(key, cutoff)
        parts.append((p[0], p[1] + gp[g], p[2], p[3]))
    wdeg = np.concatenate([p[0] for p in parts])
    np.testing.assert_array_equal(deg.cpu().numpy(), wdeg, err_msg="deg")
    np.testing.assert_array_equal(row_ptr.cpu().numpy(), R.scan(wdeg), err_msg="row_ptr")
    np.testing.assert_array_equal(col[:nnz].cpu().numpy(), np.concatenate([p[1] for p in parts]), err_msg="col")
    np.testing.assert_array_equal(dist[:nnz].cpu().numpy(), np.concatenate([p[2] for p in parts]), err_msg="dist")
    np.testing.assert_array_equal(inv.cpu().numpy(), np.concatenate([p[3] for p in parts]), err_msg="inv_degree")
    np.testing.assert_array_equal(row_of[:nnz].cpu().numpy(), np.repeat(np.arange(N, dtype=np.int32), wdeg), err_msg="row_of")


# ------------------------------------------------------------------------------------------------ ng_exclusive_scan_i32
def _scan_values(kind, n):
    rng = np.random.default_rng(n + 1)
    if kind == "random":
        return rng.integers(0, 41, n).astype(np.int32)
    v = np.zeros(n, np.int32)
    if kind == "last_one" and n:
        v[-1] = 1
    if kind == "total_2^31-1" and n:
        v[:] = (2 ** 31 - 1) // n
        v[rng.integers(0, n)] += (2 ** 31 - 1) % n
        assert int(v.astype(np.int64).sum()) == 2 ** 31 - 1
    return v


SCAN_N = (0, 1, 1023, 1024, 1025, 32767, 32768, 32769, 262143, 262144, 262145, 1050000)
SCAN = [(n, k) for n in SCAN_N for k in ("random", "zeros", "last_one")] + [(n, "total_2^31-1") for n in (1, 1025, 32769, 262145)]


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("n,kind", SCAN, ids=[f"n{n}-{k}" for n, k in SCAN])
def test_exclusive_scan(gpu_device, n, kind, in_place):
    """out of place: one launch up to 32768 values, three launches above; in place (in == out): three launches at every size.
    Sizes on both sides of that switch, of the 1024-value tiles of n + 1 and of the 256 block totals one pass of the totals
    kernel takes (262144 + 1 values are 257 tiles)"""
    import torch
    from nmrgnn_amd._lib import ptr
    dev = gpu_device
    v = _scan_values(kind, n)
    out = torch.full((n + 1 + 8,), -7, dtype=torch.int32, device=dev)
    if in_place:
        out[:n] = torch.from_numpy(v).to(dev)
        src = out
    else:
        src = torch.from_numpy(v).to(dev) if n else torch.zeros(1, dtype=torch.int32, device=dev)
    ctx = _ctx()
    _, names = _scopes(lambda: ctx.check(ctx.lib.ng_exclusive_scan_i32(ctx.handle, _stream(dev), n, ptr(src), ptr(out)), "scan"))
    torch.cuda.synchronize()
    assert "exclusive_scan" in names
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:n + 1], R.scan(v))
    assert (got[n + 1:] == -7).all()                       # nothing past out[n]
    if not in_place and n:
        np.testing.assert_array_equal(src.cpu().numpy(), v)
