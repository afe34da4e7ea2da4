"""Geometry of a batch: its boundary conditions (``Boundary``), how a build divides the atoms (``Layout``), what the position
and box gradients read (``Geometry``), and the ONE place that chooses a library entry point for the list builders and these
gradients and lays out its arguments: ``knn_call`` .. ``box_grad_call``, pure functions (list form or layout, boundary case)
-> (symbol, arguments after ctx and stream), checked against ``_lib.SIGNATURES`` without a device
(tests/test_geometry_dispatch_host.py).  ``library_calls`` is the executor of every library call of the graph layer."""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import ptr

OPEN, UNIFORM, PER_STRUCTURE = "open", "uniform", "per structure"


@contextlib.contextmanager
def library_calls(ctx, device):
    """``call(symbol, args)`` on ``device``'s current stream, under its device guard, the return code checked.  ``ctx``
    None: the device's shared context, looked up now."""
    ctx = ctx or _lib.get_context(device.index)
    with torch.cuda.device(device):
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        lib, handle = ctx.lib, ctx.handle
        yield lambda name, args: ctx.check(getattr(lib, name)(handle, st, *args), name)


def edge_grad_input(dedges, device, n, what):
    """an edge gradient as the library reads it: detached float32, contiguous, ``n`` entries"""
    dd = dedges.detach().to(device=device, dtype=torch.float32).contiguous()
    if dd.numel() != n:
        raise ValueError(f"{what}: dedges has {dd.numel()} entries for {n} edges")
    return dd


@dataclass(frozen=True, eq=False)
class Boundary:
    """Immutable; built from fields that are already on the device (a static buffer that later calls refill), or by
    ``from_host``.  open: nothing.  uniform: ``box`` [G, 9] float32 lattice vectors on the device (nmrgnn_amd.pbc) and the
    triclinic flag of the whole batch.  per structure: ``box`` [G, 9] (zeros for open structures), ``kind`` [G] int32 on the
    device (-1 open, 0 orthorhombic, 1 reduced triclinic) and the same kinds on the host."""
    case: str = OPEN
    box: torch.Tensor = None
    triclinic: bool = False
    kind: torch.Tensor = None
    kind_host: np.ndarray = None

    def __post_init__(self):
        box, k, kh = self.box, self.kind, self.kind_host
        boxed = isinstance(box, torch.Tensor) and box.dim() == 2 and box.shape[1] == 9 and box.dtype == torch.float32
        kinds = boxed and isinstance(k, torch.Tensor) and k.dtype == torch.int32 and k.device == box.device \
            and isinstance(kh, np.ndarray) and kh.dtype == np.int32 and kh.flags.c_contiguous \
            and tuple(k.shape) == kh.shape == (box.shape[0],)
        ok = {OPEN: box is None and self.triclinic is False, UNIFORM: boxed and isinstance(self.triclinic, bool),
              PER_STRUCTURE: kinds and self.triclinic is False}.get(self.case, False)
        if not ok or (self.case != PER_STRUCTURE and (k is not None or kh is not None)):
            raise ValueError(f"Boundary: inconsistent fields for the case {self.case!r}")

    @classmethod
    def from_host(cls, prepared, device):
        """from None (open), pbc.prepare's (vectors, triclinic flag, widths) or pbc.prepare_ragged's (vectors, kinds,
        widths): the vectors, and the kinds, go to the device here"""
        if prepared is None:
            return OPEN_BOUNDARY
        box = torch.from_numpy(prepared[0]).to(device)
        if not isinstance(prepared[1], np.ndarray):
            return cls(UNIFORM, box, bool(prepared[1]))
        kind_host = np.ascontiguousarray(prepared[1], dtype=np.int32)
        return cls(PER_STRUCTURE, box, False, torch.from_numpy(kind_host).to(device), kind_host)

    def args(self):
        """what the ``_pbc`` entry points take for the boundary: box and flag, or box, kinds and host kinds"""
        if self.case == UNIFORM:
            return ptr(self.box), int(self.triclinic)
        return (ptr(self.box), ptr(self.kind), C.c_void_p(self.kind_host.ctypes.data)) if self.case == PER_STRUCTURE else ()


OPEN_BOUNDARY = Boundary()


@dataclass(frozen=True, eq=False)
class Layout:
    """G frames of n atoms (``graph_ptr`` None), or G structures of their own sizes, ragged: ``graph_ptr`` [G+1] int32 on
    the device, with the same array on the host (what the ragged kNN entry points read there)"""
    G: int
    N: int
    min_n: int
    max_n: int
    graph_ptr_host: np.ndarray
    graph_ptr: torch.Tensor = None

    @classmethod
    def frames(cls, G, n):
        return cls(int(G), int(G) * int(n), int(n), int(n), np.arange(int(G) + 1, dtype=np.int64) * int(n))

    @classmethod
    def ragged(cls, graph_ptr_host, graph_ptr):
        gp = np.ascontiguousarray(graph_ptr_host, dtype=np.int32)
        sizes = np.diff(gp)
        if len(sizes) < 1 or gp[0] != 0 or (sizes <= 0).any() or tuple(graph_ptr.shape) != gp.shape:
            raise ValueError("Layout: graph_ptr must be [G+1], start at 0 and increase, on the host and on the device")
        return cls(len(sizes), int(gp[-1]), int(sizes.min()), int(sizes.max()), gp, graph_ptr)


@dataclass(frozen=True, eq=False)
class ListView:
    """the lists of a batch as the library takes them: padded [N, K], or CSR (``K`` 0, ``row_ptr`` [N+1], ``row_of`` [nnz]);
    ``edges`` detached"""
    is_csr: bool
    N: int
    K: int
    nlist: torch.Tensor
    edges: torch.Tensor
    row_ptr: torch.Tensor = None
    row_of: torch.Tensor = None


# ------------------------------------------------------------------------------------------------ the entry points
# the kNN build, the cutoff count and the cutoff fill by (ragged layout, boundary case); a combination not here has none
KNN, COUNT, FILL = range(3)
_BUILDERS = {(False, OPEN): ("ng_knn_graph", "ng_cutoff_count", "ng_cutoff_fill_rows"),
             (False, UNIFORM): ("ng_knn_graph_pbc", "ng_cutoff_count_pbc", "ng_cutoff_fill_rows_pbc"),
             (True, OPEN): ("ng_knn_graph_ragged", "ng_cutoff_count_ragged", "ng_cutoff_fill_rows_ragged"),
             (True, PER_STRUCTURE): ("ng_knn_graph_ragged_pbc", "ng_cutoff_count_ragged_pbc", "ng_cutoff_fill_rows_ragged_pbc")}
# gradients by (CSR lists, boundary case)
_POSITIONS_GRAD = {(False, OPEN): "ng_positions_grad", (True, OPEN): "ng_positions_grad_csr",
                   (False, UNIFORM): "ng_positions_grad_pbc", (True, UNIFORM): "ng_positions_grad_csr_pbc",
                   (False, PER_STRUCTURE): "ng_positions_grad_ragged_pbc",
                   (True, PER_STRUCTURE): "ng_positions_grad_csr_ragged_pbc"}
# by (CSR lists, a kind per structure)
_BOX_GRAD = {(False, False): "ng_box_grad", (True, False): "ng_box_grad_csr",
             (False, True): "ng_box_grad_ragged", (True, True): "ng_box_grad_csr_ragged"}


def _builder(op, layout, boundary, host_ptr=False):
    """(symbol, the counts in front: G and n, or G and N, what a ragged entry point takes after ``pos`` + the boundary's)"""
    ragged = layout.graph_ptr is not None
    names = _BUILDERS.get((ragged, boundary.case))
    if names is None:
        raise ValueError(f"no list builder for a {'ragged' if ragged else 'uniform'} layout with a {boundary.case} boundary")
    if boundary.box is not None and boundary.box.shape[0] != layout.G:
        raise ValueError(f"the boundary holds {boundary.box.shape[0]} boxes, the layout {layout.G} graphs")
    if not ragged:
        return names[op], (layout.G, layout.max_n), boundary.args()
    host = (C.c_void_p(layout.graph_ptr_host.ctypes.data),) if host_ptr else ()      # the kNN search reads the sizes there
    return names[op], (layout.G, layout.N), (ptr(layout.graph_ptr), *host, layout.max_n, *boundary.args())


def knn_call(layout, boundary, K, scale, pos, nlist, edges, inv):
    name, counts, where = _builder(KNN, layout, boundary, host_ptr=True)
    return name, (*counts, int(K), float(scale), ptr(pos), *where, ptr(nlist), ptr(edges), ptr(inv))


def cutoff_count_call(layout, boundary, cutoff, pos, deg):
    name, counts, where = _builder(COUNT, layout, boundary)
    return name, (*counts, float(cutoff), ptr(pos), *where, ptr(deg))


def cutoff_fill_call(layout, boundary, cutoff, scale, pos, row_ptr, col, dist, inv, row_of):
    name, counts, where = _builder(FILL, layout, boundary)
    return name, (*counts, float(cutoff), float(scale), ptr(pos), *where, ptr(row_ptr), ptr(col), ptr(dist), ptr(inv),
                  ptr(row_of))


def _grad_head(geom, dd, row_of):
    """N, K or nnz, positions, the lists (CSR: with ``row_of`` where the entry point takes it), dedges, scale"""
    v = geom.lists
    if v.is_csr:
        lists = (v.edges.numel(), ptr(geom.positions), ptr(v.row_ptr), ptr(v.nlist), *((ptr(v.row_of),) if row_of else ()))
    else:
        lists = (v.K, ptr(geom.positions), ptr(v.nlist), ptr(v.edges))
    return (v.N, *lists, ptr(dd), geom.scale)


def positions_grad_call(geom, dd, dpos):
    bd = geom.boundary
    # what finds an edge's box (csrc/pbc.cuh): n atoms per frame, or the structures (DispPer: each by its own boundary kind)
    where = {OPEN: (), UNIFORM: (int(geom.positions.shape[-2]),), PER_STRUCTURE: (geom.G, ptr(geom.graph_ptr))}[bd.case]
    return _POSITIONS_GRAD[geom.lists.is_csr, bd.case], (*_grad_head(geom, dd, True), ptr(geom.csc_ptr), ptr(geom.csc_edge),
                                                         *where, *bd.args(), ptr(dpos))


def box_grad_call(geom, dd, strain, dvec):
    bd = geom.boundary
    # open and uniform boundaries share an entry point: its flag is -1 open (no box, dvec = 0), 0 orthorhombic, 1 triclinic
    where = bd.args() if bd.case == PER_STRUCTURE else (ptr(bd.box), int(bd.triclinic) if bd.case == UNIFORM else -1)
    return _BOX_GRAD[geom.lists.is_csr, bd.case == PER_STRUCTURE], (*_grad_head(geom, dd, False), geom.G, ptr(geom.graph_ptr),
                                                                    *where, ptr(strain), ptr(dvec))


@dataclass(frozen=True, eq=False)
class Geometry:
    """what ``positions_grad`` and ``box_grad`` read, taken from a batch when the call or the autograd node is made.
    ``ctx`` None: the device's shared context, resolved at the call.  ``csc_ptr`` / ``csc_edge`` (the incoming-edge lists)
    are needed by ``positions_grad`` alone."""
    ctx: object
    device: torch.device
    positions: torch.Tensor
    scale: float
    boundary: Boundary
    lists: ListView
    G: int
    graph_ptr: torch.Tensor
    csc_ptr: torch.Tensor = None
    csc_edge: torch.Tensor = None

    def positions_grad(self, dedges):
        dd = edge_grad_input(dedges, self.device, self.lists.edges.numel(), "positions_grad")
        dpos = torch.empty_like(self.positions)
        with library_calls(self.ctx, self.device) as call:
            call(*positions_grad_call(self, dd, dpos))
        return dpos

    def box_grad(self, dedges, want_dvec=True):
        dd = edge_grad_input(dedges, self.device, self.lists.edges.numel(), "box_grad")
        strain = torch.empty(self.G, 3, 3, dtype=torch.float64, device=self.device)
        dvec = torch.empty(self.G, 3, 3, dtype=torch.float64, device=self.device) if want_dvec else None
        with library_calls(self.ctx, self.device) as call:
            call(*box_grad_call(self, dd, strain, dvec))
        return strain, dvec
