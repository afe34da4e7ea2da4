"""The choice of a library entry point for the list builders and the geometry gradients (nmrgnn_amd/geometry.py), checked on the
host against ``_lib.SIGNATURES``: every cell of (operation, list form or layout, boundary case) gives the symbol of the table
below with arguments that convert under its declared ctypes types, and the pointers whose identity matters are those of the
intended tensors.  N = 6 atoms in G = 2 graphs (ragged: 5 + 1), K = 2, CSR with 3 entries; all tensors on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from nmrgnn_amd import _lib, geometry as GEO
from nmrgnn_amd.geometry import OPEN, PER_STRUCTURE, UNIFORM, Boundary, Geometry, Layout, ListView

N, G, K, NNZ = 6, 2, 2, 3
SCALE, CUTOFF = 0.1, 3.5


def _t(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def _boundary(case):
    if case == OPEN:
        return GEO.OPEN_BOUNDARY
    if case == UNIFORM:
        return Boundary(UNIFORM, _t((G, 9)), True)
    return Boundary.from_host((np.zeros((G, 9), np.float32), np.array([1, -1], np.int32), None), "cpu")


def _layout(ragged):
    if not ragged:
        return Layout.frames(G, N // G)
    gp = np.array([0, 5, 6], np.int32)                  # a 1-atom structure
    return Layout.ragged(gp, torch.from_numpy(gp.copy()))


def _geometry(csr, case, ragged):
    gp = torch.tensor([0, 5, 6] if ragged else [0, 3, 6], dtype=torch.int32)
    pos = _t((N, 3)) if ragged else _t((G, N // G, 3))
    if csr:
        view = ListView(True, N, 0, _t(NNZ, torch.int32), _t(NNZ), _t(N + 1, torch.int32), _t(NNZ, torch.int32))
    else:
        view = ListView(False, N, K, _t((N, K), torch.int32), _t((N, K)))
    return Geometry(None, torch.device("cpu"), pos, SCALE, _boundary(case), view, G, gp, _t(N + 1, torch.int32),
                    _t(max(NNZ, N * K), torch.int32))


def _value(a):
    return a.value if isinstance(a, C.c_void_p) else a


def _check(name, args, want_name, want):
    """``want``: {argument index after ctx and stream: expected value}"""
    assert name == want_name
    argtypes = _lib.SIGNATURES[name][1]
    full = (C.c_void_p(1), C.c_void_p(2), *args)
    assert len(full) == len(argtypes), (name, len(full), len(argtypes))
    for a, t in zip(full, argtypes):
        if t is C.c_void_p:
            assert a is None or isinstance(a, C.c_void_p), (name, a)
        elif t is C.c_float:
            assert type(a) is float, (name, a)
        else:
            assert t in (C.c_int, C.c_int64) and type(a) is int, (name, a)
        t.from_param(a)
    for i, v in want.items():
        assert _value(args[i]) == v, (name, i, _value(args[i]), v)
    return name


def _bd_want(bd, at):
    """the boundary's arguments, expected from index ``at``"""
    if bd.case == UNIFORM:
        return {at: bd.box.data_ptr(), at + 1: 1}
    if bd.case == PER_STRUCTURE:
        return {at: bd.box.data_ptr(), at + 1: bd.kind.data_ptr(), at + 2: bd.kind_host.ctypes.data}
    return {}


BUILD_CELLS = [(False, OPEN, ""), (False, UNIFORM, "_pbc"), (True, OPEN, "_ragged"), (True, PER_STRUCTURE, "_ragged_pbc")]


def _knn_build(ragged, case, suffix):
    lay, bd = _layout(ragged), _boundary(case)
    pos, nlist, edges, inv = _t((N, 3)), _t((N, K), torch.int32), _t((N, K)), _t(N)
    name, args = GEO.knn_call(lay, bd, K, SCALE, pos, nlist, edges, inv)
    want = {0: G, 1: N if ragged else N // G, 2: K, 3: SCALE, 4: pos.data_ptr()}
    at = 5
    if ragged:
        want.update({5: lay.graph_ptr.data_ptr(), 6: lay.graph_ptr_host.ctypes.data, 7: 5})
        at = 8
    want.update(_bd_want(bd, at))
    n = len(args)
    want.update({n - 3: nlist.data_ptr(), n - 2: edges.data_ptr(), n - 1: inv.data_ptr()})
    return {_check(name, args, "ng_knn_graph" + suffix, want)}


def _cutoff_build(ragged, case, suffix):
    lay, bd = _layout(ragged), _boundary(case)
    pos, deg, row_ptr = _t((N, 3)), _t(N, torch.int32), _t(N + 1, torch.int32)
    col, dist, inv, row_of = _t(NNZ, torch.int32), _t(NNZ), _t(N), _t(NNZ, torch.int32)
    counts = {0: G, 1: N if ragged else N // G, 2: CUTOFF}
    name, args = GEO.cutoff_count_call(lay, bd, CUTOFF, pos, deg)
    want = {**counts, 3: pos.data_ptr(), len(args) - 1: deg.data_ptr()}
    if ragged:
        want.update({4: lay.graph_ptr.data_ptr(), 5: 5})
    want.update(_bd_want(bd, 6 if ragged else 4))
    count = _check(name, args, "ng_cutoff_count" + suffix, want)
    name, args = GEO.cutoff_fill_call(lay, bd, CUTOFF, SCALE, pos, row_ptr, col, dist, inv, row_of)
    n = len(args)
    want = {**counts, 3: SCALE, 4: pos.data_ptr(), n - 5: row_ptr.data_ptr(), n - 4: col.data_ptr(), n - 3: dist.data_ptr(),
            n - 2: inv.data_ptr(), n - 1: row_of.data_ptr()}
    if ragged:
        want.update({5: lay.graph_ptr.data_ptr(), 6: 5})
    want.update(_bd_want(bd, 7 if ragged else 5))
    return {count, _check(name, args, "ng_cutoff_fill_rows" + suffix, want)}


# (boundary case, ragged positions, symbol suffix of positions_grad after the optional _csr, the same of box_grad)
GRAD_CELLS = [(OPEN, False, "", ""), (OPEN, True, "", ""), (UNIFORM, False, "_pbc", ""),
              (PER_STRUCTURE, True, "_ragged_pbc", "_ragged")]


def _positions_grad(csr, case, ragged, suffix, _):
    g = _geometry(csr, case, ragged)
    v, bd = g.lists, g.boundary
    dd, dpos = torch.zeros_like(v.edges), torch.zeros_like(g.positions)
    name, args = GEO.positions_grad_call(g, dd, dpos)
    if csr:
        want = {0: N, 1: NNZ, 2: g.positions.data_ptr(), 3: v.row_ptr.data_ptr(), 4: v.nlist.data_ptr(), 5: v.row_of.data_ptr(),
                6: dd.data_ptr(), 7: SCALE, 8: g.csc_ptr.data_ptr(), 9: g.csc_edge.data_ptr()}
    else:
        want = {0: N, 1: K, 2: g.positions.data_ptr(), 3: v.nlist.data_ptr(), 4: v.edges.data_ptr(), 5: dd.data_ptr(), 6: SCALE,
                7: g.csc_ptr.data_ptr(), 8: g.csc_edge.data_ptr()}
    at = 10 if csr else 9
    if case == UNIFORM:
        want.update({at: N // G, **_bd_want(bd, at + 1)})           # n = positions.shape[-2]
    elif case == PER_STRUCTURE:
        want.update({at: G, at + 1: g.graph_ptr.data_ptr(), **_bd_want(bd, at + 2)})
    want[len(args) - 1] = dpos.data_ptr()
    return {_check(name, args, "ng_positions_grad" + ("_csr" if csr else "") + suffix, want)}


def _box_grad(csr, case, ragged, _, suffix):
    g = _geometry(csr, case, ragged)
    v, bd = g.lists, g.boundary
    dd, strain, dvec = torch.zeros_like(v.edges), _t((G, 3, 3), torch.float64), _t((G, 3, 3), torch.float64)
    name, args = GEO.box_grad_call(g, dd, strain, dvec)
    if csr:
        want = {0: N, 1: NNZ, 2: g.positions.data_ptr(), 3: v.row_ptr.data_ptr(), 4: v.nlist.data_ptr(), 5: dd.data_ptr()}
    else:
        want = {0: N, 1: K, 2: g.positions.data_ptr(), 3: v.nlist.data_ptr(), 4: v.edges.data_ptr(), 5: dd.data_ptr()}
    want.update({6: SCALE, 7: G, 8: g.graph_ptr.data_ptr()})
    if case == OPEN:
        want.update({9: None, 10: -1})                              # open boundaries: no box, tric == -1
    else:
        want.update(_bd_want(bd, 9))
    want.update({len(args) - 2: strain.data_ptr(), len(args) - 1: dvec.data_ptr()})
    # without dvec: NULL in its place
    assert GEO.box_grad_call(g, dd, strain, None)[1][-1] is None
    return {_check(name, args, "ng_box_grad" + ("_csr" if csr else "") + suffix, want)}


@pytest.mark.parametrize("cell", BUILD_CELLS, ids=lambda c: c[2] or "open")
@pytest.mark.parametrize("run", [_knn_build, _cutoff_build], ids=["knn", "cutoff"])
def test_list_builders(run, cell):
    run(*cell)


@pytest.mark.parametrize("csr", [False, True], ids=["padded", "csr"])
@pytest.mark.parametrize("cell", GRAD_CELLS, ids=["open", "ragged-open", "uniform", "per-structure"])
@pytest.mark.parametrize("run", [_positions_grad, _box_grad], ids=["positions_grad", "box_grad"])
def test_gradients(run, cell, csr):
    run(csr, *cell)


def test_every_entry_point_is_produced():
    """the 22 symbols of the five operations: each is in the dispatch tables, and some cell above produces it"""
    forms = ("", "_pbc", "_ragged", "_ragged_pbc")
    want = {op + f for op in ("ng_knn_graph", "ng_cutoff_count", "ng_cutoff_fill_rows") for f in forms}
    want |= {"ng_positions_grad" + c + f for c in ("", "_csr") for f in ("", "_pbc", "_ragged_pbc")}
    want |= {"ng_box_grad" + c + f for c in ("", "_csr") for f in ("", "_ragged")}
    assert len(want) == 22 and want <= set(_lib.SIGNATURES)
    tabled = [n for names in GEO._BUILDERS.values() for n in names] + [*GEO._POSITIONS_GRAD.values(), *GEO._BOX_GRAD.values()]
    assert sorted(tabled) == sorted(want)                           # each once
    seen = set()
    for cell in BUILD_CELLS:
        seen |= _knn_build(*cell) | _cutoff_build(*cell)
    for cell in GRAD_CELLS:
        for csr in (False, True):
            seen |= _positions_grad(csr, *cell) | _box_grad(csr, *cell)
    assert seen == want, sorted(want ^ seen)


@pytest.mark.parametrize("ragged,case", [(False, PER_STRUCTURE), (True, UNIFORM)])
def test_layout_and_boundary_that_have_no_entry_point(ragged, case):
    with pytest.raises(ValueError, match="no list builder"):
        GEO.knn_call(_layout(ragged), _boundary(case), K, SCALE, _t((N, 3)), _t((N, K), torch.int32), _t((N, K)), _t(N))
    with pytest.raises(ValueError, match="no list builder"):
        GEO.cutoff_count_call(_layout(ragged), _boundary(case), CUTOFF, _t((N, 3)), _t(N, torch.int32))


def test_boundary_refuses_inconsistent_input():
    box, kind, kh = _t((G, 9)), _t(G, torch.int32), np.zeros(G, np.int32)
    for bad in (dict(case=PER_STRUCTURE, kind=kind, kind_host=kh),                     # kinds without a box
                dict(case=OPEN, box=box),
                dict(case=UNIFORM),
                dict(case=UNIFORM, box=_t((G, 6))),
                dict(case=UNIFORM, box=_t((G, 9), torch.float64)),
                dict(case=UNIFORM, box=box, kind=kind, kind_host=kh),
                dict(case=PER_STRUCTURE, box=box, kind=kind),
                dict(case=PER_STRUCTURE, box=box, kind=_t(G + 1, torch.int32), kind_host=kh),
                dict(case=PER_STRUCTURE, box=box, kind=kind, kind_host=np.zeros(G, np.int64)),
                dict(case="periodic", box=box)):
        with pytest.raises(ValueError, match="Boundary"):
            Boundary(**bad)
    # a [G, 9] box with another G than the layout
    with pytest.raises(ValueError, match="boxes"):
        GEO.knn_call(_layout(False), Boundary(UNIFORM, _t((G + 1, 9)), False), K, SCALE, _t((N, 3)), _t((N, K), torch.int32),
                     _t((N, K)), _t(N))
    with pytest.raises(Exception):
        _boundary(UNIFORM).box = None                                                  # immutable


def test_boundary_cases_and_flags():
    assert GEO.OPEN_BOUNDARY.case == OPEN and GEO.OPEN_BOUNDARY.box is None and GEO.OPEN_BOUNDARY.args() == ()
    assert Boundary.from_host(None, "cpu") is GEO.OPEN_BOUNDARY
    u = Boundary.from_host((np.ones((G, 9), np.float32), False, None), "cpu")
    assert u.case == UNIFORM and u.triclinic is False and u.args()[1] == 0 and _boundary(UNIFORM).args()[1] == 1
    p = _boundary(PER_STRUCTURE)
    assert p.case == PER_STRUCTURE and p.kind.tolist() == p.kind_host.tolist() == [1, -1]


def test_batch_without_geometry_reports_none():
    from nmrgnn_amd.graph import GraphBatch
    atoms = np.eye(3, dtype=np.float32)
    nlist = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    edges = np.full((3, 2), 0.1, np.float32)
    for gb in (GraphBatch(atoms, nlist, edges, np.full(3, 0.5, np.float32), device="cpu"),
               GraphBatch.from_csr(atoms, [0, 2, 4, 6], nlist.reshape(-1), edges.reshape(-1), device="cpu")):
        assert gb.positions is None and gb.scale is None and gb.box is None and gb.box_triclinic is False
        assert gb.box_kind is None and gb.box_kind_host is None
        with pytest.raises(ValueError, match="positions"):
            gb.positions_grad(torch.zeros(gb.edges.shape))
        with pytest.raises(ValueError, match="positions"):
            gb.box_grad(torch.zeros(gb.edges.shape), want_dvec=False)
        gb.set_geometry(torch.zeros(1, 3, 3), 0.1, _boundary(OPEN))
        assert gb.positions is not None and gb.scale == 0.1 and gb.box is None
