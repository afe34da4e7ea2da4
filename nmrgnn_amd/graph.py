"""Graph batches in device memory.

The reference feeds ONE graph per model call as the 4-tuple
``(atoms[N,C] one-hot f32, nlist[N,K] int, edges[N,K] f32 distances, inv_degree[N] f32)``
(nmrgnn/library.py:106-117, nmrgnn/model.py:249).  The model is per-atom with indices local to a
graph, so any number of graphs can be concatenated along N with offset neighbour indices
(SURVEY App. C KAT-6); that is how the engine batches molecules.

Besides the reference's padded [N,K] lists a batch can hold the CSR form of SURVEY §8(b)
(``GraphBatch.from_csr`` / ``to_csr`` / ``frames_to_batch_cutoff``): ``row_ptr`` [N+1], ``nlist`` = col [nnz],
``edges`` = dist [nnz] — the padded lists with their ``edges == 0`` slots dropped, or a variable-degree
(distance-cutoff) graph.  ``is_csr`` tells the engine which entry points to call.

A GraphBatch additionally carries
  * ``graph_ptr`` [G+1]: atom ranges of the member graphs (loss is per graph, losses.py:37-39);
  * the transposed incoming-edge lists ``csc_ptr`` [N+1] / ``csc_edge`` [nnz] used by the
    deterministic backward scatter (edge id = i*K + j, grouped by target nlist[i,j]); slots with
    ``edges == 0`` are dropped — they carry e == 0 exactly because of the edge mask (model.py:261);
  * where it was built from positions, those, the distance scale and the boundary conditions (``set_geometry``).  The
    records behind ``positions_grad`` / ``box_grad`` and the choice of a library entry point live in geometry.py.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from .geometry import OPEN_BOUNDARY, Boundary, Geometry, Layout, ListView, cutoff_count_call, cutoff_fill_call, edge_grad_input, \
    knn_call, library_calls
from .pbc import prepare, prepare_ragged, triclinic_vectors_torch


def _norm_device(device):
    """torch.device with an explicit index for cuda ('cuda' / torch.device('cuda') name the current device): the
    library's per-device context is looked up by index"""
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


_GRAPH_PTR_CACHE = {}


def _graph_ptr_dev(host, device):
    """device copy of a graph_ptr array.  Small partitions repeat from batch to batch (one graph per call: [0, n]; fixed-size
    graphs) and a pageable host-to-device copy blocks the host until the stream has drained — per call that stall was a tenth of
    a one-graph training step — so the copies are kept (at most 64 of at most 4096 entries)."""
    if host.size > 4096 or device.type != "cuda":
        return torch.as_tensor(host, device=device)
    # keyed by the allocating stream as well: a copy made under the prefetcher's side stream is never handed to a batch
    # built on another stream (the caching allocator recycles a block on the stream that allocated it)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, host.tobytes())
    t = _GRAPH_PTR_CACHE.get(key)
    if t is None:
        if len(_GRAPH_PTR_CACHE) >= 64:
            _GRAPH_PTR_CACHE.clear()
        t = torch.as_tensor(host, device=device)
        _GRAPH_PTR_CACHE[key] = t
    return t


def _to_dev(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    # tf eager tensors and friends expose __array__
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x)), device=device).to(dtype).contiguous()


class GraphBatch:
    is_csr = False
    row_ptr = None
    positions = None   # [G, n, 3] (ragged: [N, 3]) Angstrom, the distance scale and the boundary conditions the lists were
    scale = None       # built with: set_geometry, called by the builders from positions
    boundary = OPEN_BOUNDARY

    def set_geometry(self, positions, scale, boundary):
        """the one place that attaches the geometry the lists were built from (geometry.Boundary)"""
        self.positions, self.scale, self.boundary = positions, float(scale), boundary

    # the boundary, field by field (geometry.Boundary): None / False without periodic boxes, the kinds None unless the
    # structures have kinds of their own (structures_to_batch(boxes=))
    box = property(lambda self: self.boundary.box)
    box_triclinic = property(lambda self: self.boundary.triclinic)
    box_kind = property(lambda self: self.boundary.kind)
    box_kind_host = property(lambda self: self.boundary.kind_host)

    _ctx = None        # library context for the list builders; None = the device's shared one (BatchPrefetcher sets its own)

    def __init__(self, atoms, nlist, edges, inv_degree, graph_ptr=None, device=None,
                 validate=True, nlist_c=None, ctx=None, graph_ptr_dev=None):
        self.device = _norm_device(device)
        self._ctx = ctx
        self.atoms = _to_dev(atoms, torch.float32, self.device)
        self.nlist = _to_dev(nlist, torch.int32, self.device)
        self.edges = _to_dev(edges, torch.float32, self.device)
        inv = _to_dev(inv_degree, torch.float32, self.device)
        self.inv_degree = inv.reshape(-1)
        if self.atoms.dim() != 2 or self.nlist.dim() != 2 or self.edges.dim() != 2:
            raise ValueError("atoms must be [N,C], nlist and edges [N,K]")
        self.N, self.C = self.atoms.shape
        self.K = self.nlist.shape[1]
        if self.nlist.shape[0] != self.N or tuple(self.edges.shape) != (self.N, self.K) \
                or self.inv_degree.shape[0] != self.N:
            raise ValueError("inconsistent leading dimensions in graph tuple")
        if validate and self.N > 0:
            lo, hi = int(self.nlist.min()), int(self.nlist.max())
            if lo < 0 or hi >= self.N:
                raise ValueError(f"nlist entries must lie in [0,{self.N}); got [{lo},{hi}]")
        if graph_ptr is None:
            graph_ptr = [0, self.N]
        self.graph_ptr_host = np.asarray(graph_ptr, dtype=np.int32)
        # graph_ptr_dev: the caller already holds this partition on the device (dataset.ShiftDataset.batch sends it with the
        # record ids in one copy)
        self.graph_ptr = graph_ptr_dev if graph_ptr_dev is not None else _graph_ptr_dev(self.graph_ptr_host, self.device)
        self.G = len(self.graph_ptr_host) - 1
        self._csc = None
        self._live = None
        # compute-side copy of the lists: padded slots (edges == 0, weight exactly 0 after the edge mask)
        # point at the atom itself instead of row 0, so that the row range a tile of atoms references
        # stays local and the window-resident MP kernels (csrc/mp_win.hip) can keep it in LDS
        if nlist_c is not None:            # the caller knows the lists carry no padded slot (e.g. kNN with n > K)
            self.nlist_c = nlist_c
        else:
            # one library call builds the compute-side list AND the incoming-edge lists (ng_build_incoming_lists)
            self.nlist_c = torch.empty_like(self.nlist)
            self._build_lists(self.nlist_c)

    # ------------------------------------------------------------------ CSR form
    @classmethod
    def from_csr(cls, atoms, row_ptr, col, dist, inv_degree=None, graph_ptr=None, device=None, validate=True, row_of=None):
        """Variable-degree graph(s): row i owns the entries [row_ptr[i], row_ptr[i+1]) of ``col`` (neighbour
        atom, batch-global) and ``dist`` (distance > 0).  ``inv_degree`` defaults to the reference's rule
        1 / #(graph-local neighbour index > 0), 0 when that count is 0 (nmrgnn/library.py:115-116)."""
        self = cls.__new__(cls)
        self.device = _norm_device(device)
        self.is_csr = True
        self.atoms = _to_dev(atoms, torch.float32, self.device)
        if self.atoms.dim() != 2:
            raise ValueError("atoms must be [N,C]")
        self.N, self.C = self.atoms.shape
        self.row_ptr = _to_dev(row_ptr, torch.int32, self.device).reshape(-1)
        self.nlist = _to_dev(col, torch.int32, self.device).reshape(-1)
        self.edges = _to_dev(dist, torch.float32, self.device).reshape(-1)
        self.nnz = int(self.nlist.shape[0])
        self.K = 0
        if self.row_ptr.shape[0] != self.N + 1 or self.edges.shape[0] != self.nnz:
            raise ValueError("row_ptr must be [N+1]; col and dist must have the same length")
        if graph_ptr is None:
            graph_ptr = [0, self.N]
        self.graph_ptr_host = np.asarray(graph_ptr, dtype=np.int32)
        self.graph_ptr = _graph_ptr_dev(self.graph_ptr_host, self.device)
        self.G = len(self.graph_ptr_host) - 1
        if validate:
            rp = self.row_ptr.to(torch.int64)
            if int(rp[0]) != 0 or int(rp[-1]) != self.nnz or bool((rp[1:] < rp[:-1]).any()):
                raise ValueError("row_ptr must start at 0, end at nnz and be non-decreasing")
            if self.nnz:
                lo, hi = int(self.nlist.min()), int(self.nlist.max())
                if lo < 0 or hi >= self.N:
                    raise ValueError(f"col entries must lie in [0,{self.N}); got [{lo},{hi}]")
                if bool((self.edges <= 0).any()):
                    raise ValueError("CSR distances must be > 0 (zero-distance slots are the padded form's mask)")
        if row_of is not None:             # the builder already knows the row of every entry
            self.row_of = _to_dev(row_of, torch.int32, self.device).reshape(-1)
        else:
            deg = (self.row_ptr[1:] - self.row_ptr[:-1]).to(torch.int64)
            self.row_of = torch.repeat_interleave(torch.arange(self.N, device=self.device, dtype=torch.int32),
                                                  deg).contiguous()
        if inv_degree is None:
            gp = torch.as_tensor(self.graph_ptr_host.astype(np.int64), device=self.device)
            rows = self.row_of.to(torch.int64)
            gid = torch.bucketize(rows, gp[1:], right=True)
            local = self.nlist.to(torch.int64) - gp[gid]
            cnt = torch.zeros(self.N, dtype=torch.float32, device=self.device)
            cnt.index_add_(0, rows, (local > 0).to(torch.float32))
            inv_degree = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0), torch.zeros_like(cnt))
        self.inv_degree = _to_dev(inv_degree, torch.float32, self.device).reshape(-1)
        if self.inv_degree.shape[0] != self.N:
            raise ValueError("inv_degree must be [N]")
        self.nlist_c = self.nlist
        self._csc = None
        self._live = None
        return self

    def to_csr(self):
        """the same graph(s) with the ``edges == 0`` slots dropped (entry order inside a row is kept)"""
        if self.is_csr:
            return self
        keep = self.edges > 0
        deg = keep.sum(dim=1)
        row_ptr = torch.zeros(self.N + 1, dtype=torch.int64, device=self.device)
        row_ptr[1:] = torch.cumsum(deg, 0)
        return GraphBatch.from_csr(self.atoms, row_ptr.to(torch.int32), self.nlist[keep], self.edges[keep],
                                   self.inv_degree, graph_ptr=self.graph_ptr_host, device=self.device, validate=False)

    def replicate(self, S):
        """This batch ``S`` times in ONE batch of S * N atoms (replica s owns the atoms [s * N, (s + 1) * N)): the input of
        a replica ensemble (``Engine.forward_moments``, ``GNNModel.predict_uncertainty``).  ``atoms``, ``edges`` and
        ``inv_degree`` are tiled; ``nlist`` / ``col`` get ``+ s * N`` in EVERY slot, so a padded slot of replica s points
        into replica s; ``row_ptr`` is offset by ``s * nnz`` and ``graph_ptr`` by ``s * N``.  Torch ops on the device, no
        host read.  The replicas keep no positions or box (their lists are fixed: ``positions_grad`` is not for them)."""
        S = int(S)
        if S < 1:
            raise ValueError(f"replicate: at least one replica, got {S}")
        N = self.N
        if S * max(N, 1) >= 2 ** 31 or S * self.n_edges >= 2 ** 31:
            raise ValueError("replicate: more than 2^31 - 1 atoms or list entries in one batch")
        gp = self.graph_ptr_host.astype(np.int64)
        graph_ptr = np.concatenate([gp[:1]] + [gp[1:] + s * N for s in range(S)])
        off = torch.arange(S, dtype=torch.int32, device=self.device) * N
        atoms = self.atoms.repeat(S, 1)
        inv = self.inv_degree.repeat(S)
        if self.is_csr:
            nnz = self.nnz
            col = (self.nlist[None, :] + off[:, None]).reshape(-1)
            row_of = (self.row_of[None, :] + off[:, None]).reshape(-1)
            roff = torch.arange(S, dtype=torch.int32, device=self.device) * nnz
            row_ptr = torch.cat([(self.row_ptr[None, :-1] + roff[:, None]).reshape(-1),
                                 torch.full((1,), S * nnz, dtype=torch.int32, device=self.device)])
            return GraphBatch.from_csr(atoms, row_ptr, col, self.edges.detach().repeat(S), inv, graph_ptr=graph_ptr,
                                       device=self.device, validate=False, row_of=row_of)
        nlist = (self.nlist[None] + off[:, None, None]).reshape(S * N, self.K)
        # lists without a padded slot stay their own compute-side lists
        return GraphBatch(atoms, nlist, self.edges.detach().repeat(S, 1), inv, graph_ptr=graph_ptr, device=self.device,
                          validate=False, nlist_c=nlist if self.nlist_c is self.nlist else None, ctx=self._ctx)

    @property
    def max_graph_atoms(self):
        """atoms of the largest member graph (a hint for the engine: ng_ctx_set_graph_span)"""
        gp = self.graph_ptr_host
        return int(np.max(np.diff(gp))) if len(gp) > 1 else int(self.N)

    @property
    def n_edges(self):
        return self.nnz if self.is_csr else self.N * self.K

    def _build_lists(self, nlist_c=None):
        """csc_ptr [N+1] / csc_edge [n_entries capacity; csc_ptr[N] live entries] by the library's counting sort — a
        stable sort of the live entries by target, no host synchronisation, no torch kernels (include/nmrgnn_hip.h:
        ng_build_incoming_lists; the reference sees a new graph every step, nmrgnn/library.py:88-89)."""
        if self.device.type != "cuda":
            return self._build_lists_host(nlist_c)
        n_entries = self.n_edges
        csc_ptr = torch.empty(self.N + 1, dtype=torch.int32, device=self.device)
        csc_edge = torch.empty(max(n_entries, 1), dtype=torch.int32, device=self.device)
        with library_calls(self._ctx, self.device) as call:
            if nlist_c is not None and not self.is_csr and self._live is None \
                    and _lib.load().ng_graph_lists_one_launch(self.N, self.K):
                # molecule-sized call: the live-edge view in the same launch (ng_build_graph_lists)
                live = self._live_buffers()
                call("ng_build_graph_lists", (self.N, self.K, ptr(self.nlist), ptr(self.edges), ptr(nlist_c), ptr(csc_ptr),
                                              ptr(csc_edge), *map(ptr, live)))
                self._live = live
            else:
                call("ng_build_incoming_lists", (self.N, 0 if self.is_csr else self.K, n_entries, ptr(self.nlist),
                                                 None if self.is_csr else ptr(self.edges), ptr(nlist_c), ptr(csc_ptr),
                                                 ptr(csc_edge)))
        self._csc = (csc_ptr, csc_edge)

    def _live_buffers(self):
        """(perm, pos, d_c, n_live), to be written"""
        new = partial(torch.empty, dtype=torch.int32, device=self.device)
        return new(self.n_edges), new(self.n_edges), new(self.n_edges, dtype=torch.float32), new(1)

    def _build_lists_host(self, nlist_c=None):
        """the same lists with torch ops, for batches held in HOST memory (shard bookkeeping in the multi-process CPU
        tests); a device batch never comes here"""
        if nlist_c is not None:
            own = torch.arange(self.N, dtype=torch.int32)[:, None]
            nlist_c.copy_(torch.where(self.edges > 0, self.nlist, own))
        flat = self.nlist.reshape(-1)
        eid = torch.arange(flat.shape[0]) if self.is_csr else torch.nonzero((self.edges > 0).reshape(-1)).reshape(-1)
        tgt = flat[eid].to(torch.int64)
        order = torch.argsort(tgt, stable=True)
        cptr = torch.zeros(self.N + 1, dtype=torch.int64)
        cptr[1:] = torch.cumsum(torch.bincount(tgt, minlength=self.N), 0)
        self._csc = (cptr.to(torch.int32).contiguous(), eid[order].to(torch.int32).contiguous())

    def live_edges(self, force=False):
        """(perm, pos, d_c, n_live) of the padded lists (include/nmrgnn_hip.h: ng_build_live_edges) — the row order of
        the compacted edge kernels; built once per batch on the device, no host synchronisation.  None for a CSR batch
        (every entry is live) and for lists known to carry no padded slot — unless ``force``: the edge-function table's
        guard runs the per-edge kernels over a device-side row count, which only the live view offers (the view of a list
        without dead entries is the identity)."""
        if self.device.type != "cuda" or self.n_edges == 0:
            return None
        if not force and (self.is_csr or self.nlist_c is self.nlist):
            return None
        if self._live is None:
            live = self._live_buffers()
            with library_calls(self._ctx, self.device) as call:
                call("ng_build_live_edges", (self.n_edges, ptr(self.edges), *map(ptr, live)))
            self._live = live
        return self._live

    def csc(self):
        """incoming-edge lists for the backward scatter; built once per batch.  ``csc_edge`` is allocated for every
        entry; its first ``csc_ptr[N]`` elements are the live ones (the kernels walk it through ``csc_ptr``)."""
        if self._csc is None:
            self._build_lists(None)
        return self._csc

    def positions_grad(self, dedges):
        """dL/d(positions) [G, n, 3] from dL/d(edges) ``dedges`` (shaped like ``edges``), at fixed neighbour lists: the
        chain rule through edges = |r_i - r_j| * scale (include/nmrgnn_hip.h: ng_positions_grad).  Needs the positions the
        lists were built from (frames_to_batch / frames_to_batch_cutoff).  An edge between coincident atoms (a cutoff list
        holds them) contributes nothing whatever its ``dedges``, here and in ``box_grad``."""
        if self.positions is None:
            raise ValueError("positions_grad: this batch was not built from positions (frames_to_batch / frames_to_batch_cutoff)")
        return self.geometry(incoming=True).positions_grad(dedges)

    def box_grad(self, dedges, want_dvec=True):
        """``(strain, dvec)``, both [G, 3, 3] float64 on the device, from dL/d(edges) ``dedges`` in one library call
        (include/nmrgnn_hip.h: ng_box_grad), at fixed lists and images.  Per frame, over its live edges u (the displacement
        that built the edge), p = dL/du and n the image triple with u = r_j - r_i + n h:
        ``strain`` = sum u (x) p, the derivative with respect to a homogeneous strain of positions and box together (the
        virial is ``-strain``); ``dvec`` = sum n (x) p = dL/d(lattice vectors) [rows a, b, c] at fixed positions, zero without
        a box; ``want_dvec=False`` skips it (``dvec`` is None).  Works on batches built from positions (frames_to_batch,
        frames_to_batch_cutoff, structures_to_batch)."""
        if self.positions is None:
            raise ValueError("box_grad: this batch was not built from positions (frames_to_batch / frames_to_batch_cutoff / "
                             "structures_to_batch)")
        return self.geometry().box_grad(dedges, want_dvec)

    def _list_view(self):
        return ListView(self.is_csr, self.N, self.K, self.nlist, self.edges.detach(), self.row_ptr, getattr(self, "row_of", None))

    def geometry(self, incoming=False):
        """what positions_grad and box_grad read as of now, without the batch itself (an autograd node keeps this, not the
        batch whose edges are its output: no reference cycle).  ``incoming``: with the incoming-edge lists, which
        positions_grad alone needs."""
        csc_ptr, csc_edge = self.csc() if incoming else (None, None)
        return Geometry(self._ctx, self.device, self.positions, float(self.scale), self.boundary, self._list_view(), self.G,
                        self.graph_ptr, csc_ptr, csc_edge)

    def as_tuple(self):
        if self.is_csr:
            raise ValueError("a CSR batch has no (atoms, nlist, edges, inv_degree) tuple; see row_ptr / nlist / edges")
        return self.atoms, self.nlist, self.edges, self.inv_degree

    # ------------------------------------------------------------------ receptive-field pruning (csrc/prune.hip)
    parent = None        # set on the result of restrict(): the batch it was cut from
    keep = None          # [M] int32: parent index of every row
    hop = None           # [M] int32: list steps from the nearest selected atom (0 = selected)
    graph_index = None   # [G'] host int32: parent graph of every graph (graphs without a kept atom are dropped)
    _Cut = namedtuple("_Cut", "hops hop idx row_ptr_p")
    _prune = None        # _Cut(hops, hop [N], idx [N+1], row_ptr_p) of the parent's shape, for the expansions
    _selected = None

    def restrict(self, select, hops):
        """This batch cut down to the receptive field of the ``select``-ed atoms: every atom within ``hops`` steps
        i -> nlist[i, k] along live entries, and the live entries of the rows closer than ``hops``.  With
        ``hops = mp_layers`` the model's output at the selected atoms, and every gradient of a loss that reads only them, is
        that of the whole batch.

        ``select``: a mask [N] (bool, or floating point holding only 0.0 and 1.0) or an integer index array, on the host or
        the device; the dtype decides, so every integer array is read as INDICES (``selection_mask``).  A wrong length,
        indices out of range or twice, nothing selected, or ``hops`` outside [0, 64] raise ValueError.  Host inputs are
        checked before any device work.  A device bool mask is not read back: when it selects nothing, that shows only in
        the call's one host synchronisation, after the pruning launches.  A device index array is copied to the host to be
        checked, a host synchronisation of its own: pass a mask, or host indices, where that matters.

        Returns a GraphBatch of M <= N atoms in the parent's order and list form, with ``parent``, ``keep`` [M], ``hop`` [M],
        ``selected`` [S] (its rows that hold the selected atoms, ascending parent index), ``graph_ptr`` without the graphs
        that lost every atom, ``graph_index`` [G'], ``expand`` and ``expand_edge_grad``.  It keeps no positions: geometry
        gradients go through the parent, ``parent.positions_grad(pruned.expand_edge_grad(de))``.  Where the parent's
        ``edges`` require grad the pruned ``edges`` carry a grad_fn back to them.  Values at rows with ``hop > 0`` are NOT
        the model's values of those atoms."""
        hops = int(hops)
        if not 0 <= hops <= 64:
            raise ValueError(f"restrict: hops must be in [0, 64], got {hops}")
        if self.device.type != "cuda":
            raise ValueError("restrict: a device batch is needed")
        seed, sel_host = _select_seed(select, self.N, self.device)
        N, K, dev = self.N, self.K, self.device
        if not self.is_csr and N * K >= 2 ** 31:
            raise ValueError("restrict: N * K exceeds 2^31 - 1 slots")
        csr, ne, view = self.is_csr, self.n_edges, self._list_view()
        edges, row_ptr, row_of = view.edges, view.row_ptr, view.row_of
        new = partial(torch.empty, dtype=torch.int32, device=dev)
        hop, flag, idx = new(N), new(N), new(N + 1)
        gp_long = torch.as_tensor(self.graph_ptr_host.astype(np.int64), device=dev)
        with library_calls(self._ctx, dev) as call:
            call("ng_receptive_hops", (N, K, ne, ptr(row_ptr), ptr(row_of), ptr(self.nlist), ptr(edges), ptr(seed), hops,
                                       ptr(hop)))
            call("ng_prune_keep_flags", (N, ptr(hop), ptr(flag)))
            call("ng_exclusive_scan_i32", (N, ptr(flag), ptr(idx)))
            sizes = [idx[gp_long]]
            if csr:
                rp_full = new(N + 1)
                call("ng_prune_degrees_csr", (N, hops, ptr(row_ptr), ptr(hop), ptr(flag)))
                call("ng_exclusive_scan_i32", (N, ptr(flag), ptr(rp_full)))
                sizes.append(rp_full[N:])
            # the one host synchronisation: kept atoms in front of every graph (the last is M) and, for CSR, the kept entries
            sizes = torch.cat(sizes).cpu().numpy().astype(np.int64)
            before, M = sizes[:self.G + 1], int(sizes[self.G])
            if M == 0:
                raise ValueError("restrict: nothing selected")
            counts = np.diff(before)
            graph_index = np.nonzero(counts > 0)[0].astype(np.int32)
            gp_p = np.concatenate([[0], np.cumsum(counts[graph_index])]).astype(np.int32)
            keep, hop_p = new(M), new(M)
            atoms_p, inv_p = new(M, self.C, dtype=torch.float32), new(M, dtype=torch.float32)
            if csr:
                nnz_p = int(sizes[self.G + 1])
                row_ptr_p, col_p, row_of_p = new(M + 1), new(nnz_p), new(nnz_p)
                dist_p = new(nnz_p, dtype=torch.float32)
                call("ng_prune_lists_csr", (N, ne, self.C, hops, ptr(row_ptr), ptr(row_of), ptr(self.nlist), ptr(edges),
                                            ptr(self.atoms), ptr(self.inv_degree), ptr(hop), ptr(idx), ptr(rp_full), ptr(keep),
                                            ptr(hop_p), ptr(atoms_p), ptr(inv_p), ptr(row_ptr_p), ptr(col_p) if nnz_p else None,
                                            ptr(dist_p) if nnz_p else None, ptr(row_of_p) if nnz_p else None))
                b = GraphBatch.from_csr(atoms_p, row_ptr_p, col_p, dist_p, inv_p, graph_ptr=gp_p, device=dev, validate=False,
                                        row_of=row_of_p)
                b._ctx = self._ctx
            else:
                row_ptr_p = None
                nlist_p, edges_p = new(M, K), new(M, K, dtype=torch.float32)
                call("ng_prune_lists", (N, K, self.C, self.G, hops, ptr(self.graph_ptr), ptr(self.nlist), ptr(edges),
                                        ptr(self.atoms), ptr(self.inv_degree), ptr(hop), ptr(idx), ptr(keep), ptr(hop_p),
                                        ptr(atoms_p), ptr(inv_p), ptr(nlist_p), ptr(edges_p)))
                b = GraphBatch(atoms_p, nlist_p, edges_p, inv_p, graph_ptr=gp_p, device=dev, validate=False, nlist_c=None,
                               ctx=self._ctx)
        b.parent, b.keep, b.hop, b.graph_index = self, keep, hop_p, graph_index
        b._prune = self._Cut(hops, hop, idx, row_ptr_p)
        if sel_host is not None:           # indices known on the host: their rows without a data-dependent torch op
            b._selected = idx[torch.as_tensor(sel_host, device=dev)].to(torch.int64)
        if self.edges.requires_grad and torch.is_grad_enabled():
            b.edges = _PrunedEdges.apply(self.edges, b._expansion(), {"edges": b.edges})
        return b

    @property
    def selected(self):
        """[S] int64: the rows of a restricted batch that hold the selected atoms, in ascending parent index"""
        if self._selected is None and self.hop is not None:
            self._selected = torch.nonzero(self.hop == 0).reshape(-1)
        return self._selected

    def _expansion(self):
        """what expand_edge_grad reads, without the pruned batch itself (an autograd node keeps this)"""
        p = self.parent
        return _Expansion(p._ctx, p.device, p._list_view(), n_pruned=self.n_edges, **self._prune._asdict())

    def expand_edge_grad(self, dedges):
        """dL/d(edges) of a restricted batch in the PARENT's shape: its value where the entry was kept, +0.0 elsewhere
        (ng_prune_expand_edge_grad); the input of ``parent.positions_grad`` / ``parent.box_grad``"""
        if self.parent is None:
            raise ValueError("expand_edge_grad: not a restricted batch (GraphBatch.restrict)")
        return self._expansion().edge_grad(dedges)

    def expand(self, values, fill=float("nan"), selected=False):
        """per-atom values of a restricted batch in the PARENT's shape [N], ``fill`` on the other atoms
        (ng_prune_expand_rows).  ``values`` is [M], one per row of this batch; with ``selected=True`` it is [S], one per
        selected atom (the order of ``self.selected``), and every atom that is not selected gets ``fill``."""
        if self.parent is None:
            raise ValueError("expand: not a restricted batch (GraphBatch.restrict)")
        p = self.parent
        v = torch.as_tensor(values).detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        keep = self.keep[self.selected].contiguous() if selected else self.keep
        if v.shape[0] != keep.shape[0]:
            raise ValueError(f"expand: values has {v.shape[0]} entries for {keep.shape[0]} "
                             f"{'selected atoms' if selected else 'rows'}")
        out = torch.empty(p.N, dtype=torch.float32, device=self.device)
        with library_calls(p._ctx, self.device) as call:
            call("ng_prune_expand_rows", (p.N, v.shape[0], ptr(keep), ptr(v), float(fill), ptr(out)))
        return out


@dataclass(frozen=True, eq=False)
class _Expansion:
    """what leads from a restricted batch back to its parent: the parent's lists, and ``hops``, ``hop`` [N], ``idx`` [N+1]
    and the pruned ``row_ptr`` (CSR) of the cut; ``n_pruned`` entries in the pruned lists"""
    ctx: object
    device: torch.device
    lists: ListView
    hops: int
    hop: torch.Tensor
    idx: torch.Tensor
    row_ptr_p: torch.Tensor
    n_pruned: int

    def edge_grad(self, dedges):
        v, dd = self.lists, edge_grad_input(dedges, self.device, self.n_pruned, "expand_edge_grad")
        de = torch.empty(v.edges.shape, dtype=torch.float32, device=self.device)
        with library_calls(self.ctx, self.device) as call:
            call("ng_prune_expand_edge_grad", (v.N, v.K, v.edges.numel(), self.hops, ptr(v.row_ptr), ptr(v.row_of), ptr(v.nlist),
                                               ptr(v.edges), ptr(self.hop), ptr(self.idx), ptr(self.row_ptr_p), ptr(dd), ptr(de)))
        return de


def concat_graphs(graphs, device=None):
    """Concatenate per-graph tuples into one batch, offsetting neighbour indices.
    NB padded slots (nlist == 0, edges == 0) get the offset too; they stay harmless because the
    edge mask zeroes their features and only ``edges > 0`` slots enter the backward lists."""
    atoms, nlist, edges, inv, ptr = [], [], [], [], [0]
    off = 0
    for g in graphs:
        a, nl, e, v = [np.asarray(x) for x in g]
        atoms.append(a.astype(np.float32))
        nlist.append(nl.astype(np.int64) + off)
        edges.append(e.astype(np.float32))
        inv.append(np.asarray(v, np.float32).reshape(-1))
        off += a.shape[0]
        ptr.append(off)
    return GraphBatch(np.concatenate(atoms), np.concatenate(nlist).astype(np.int32),
                      np.concatenate(edges), np.concatenate(inv), graph_ptr=ptr, device=device)


class BatchPrefetcher:
    """Iterate over graph tuples as device-resident GraphBatches, building batch t+1 while the caller's step t runs.

    The reference sees a new graph tuple every step (nmrgnn/library.py:88-89; keras ``model.fit`` pulls them from a
    ``tf.data`` pipeline with prefetch, nmrgnn/main.py:79-80).  Here the per-batch preprocessing is device work — the copy
    of the tuple, the compute-side lists, the incoming-edge lists and the live-edge view (ng_build_incoming_lists,
    ng_build_live_edges) — a chain of small launches, 0.16 ms for 512 graphs, that the step's kernels would otherwise
    wait behind.  The prefetcher issues that chain on its own HIP stream with its OWN library context (the list builders
    use context scratch; the step's kernels use the shared context's), one batch ahead; the consumer's stream waits on the
    batch's event when it takes the batch.  Results are the same bits as from ``GraphBatch(*tuple)`` on the compute stream.

    ``source`` yields ``(atoms, nlist, edges, inv_degree)`` or ``((atoms, nlist, edges, inv_degree), graph_ptr)``; extra
    keyword arguments go to GraphBatch.  On a CPU device it degenerates to building each batch when it is asked for."""

    def __init__(self, source, device=None, **batch_kw):
        self.source = source
        self.device = _norm_device(device)
        self.batch_kw = batch_kw
        self._stream = None
        self._ctx = None

    def _construct(self, item, ctx):
        """the batch of one source item (a subclass may return a tuple whose first element is the batch)"""
        if len(item) == 2 and not hasattr(item[0], "shape"):
            raw, graph_ptr = item
        else:
            raw, graph_ptr = item, None
        return GraphBatch(*raw, graph_ptr=graph_ptr, device=self.device, ctx=ctx, **self.batch_kw)

    def _device_inputs(self, item):
        """does the item hold device tensors that the consumer's stream may still be writing?"""
        raw = item[0] if len(item) == 2 and not hasattr(item[0], "shape") else item
        return any(isinstance(x, torch.Tensor) and x.is_cuda for x in raw)

    def _build(self, item):
        if self.device.type != "cuda":
            return self._construct(item, None), None
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.device)
            self._ctx = _lib.Context(self.device.index)
        if self._device_inputs(item):
            # device inputs may have been produced on the consumer's stream: wait for what is enqueued there (at most the
            # previous step).  Host arrays need no such wait — and must not have one: a pageable copy holds the host until it
            # has run, and behind that wait it would run only after the previous step, with the next step not yet enqueued
            self._stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._stream):
            out = self._construct(item, self._ctx)
            gb = out[0] if isinstance(out, tuple) else out
            gb.csc()
            gb.live_edges()
            ready = torch.cuda.Event()
            ready.record(self._stream)
        return out, ready

    def _hand_over(self, gb, ready):
        if ready is None:
            return gb
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_event(ready)
        # the tensors were allocated under the side stream: tell the caching allocator who uses them from here on
        # (graph_ptr included: the loss kernels read it on the consumer's stream, and a cached or evicted copy that was
        # allocated under the side stream could otherwise be handed back to the side stream while a step is still queued)
        held = [gb.atoms, gb.nlist, gb.edges, gb.inv_degree, gb.nlist_c, gb.graph_ptr, gb.row_ptr,
                getattr(gb, "row_of", None), *(gb._csc or ()), *(gb._live or ())]
        for t in held:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(consumer)
        gb._ctx = None          # nothing lazy is left to build; later calls on this batch use the shared context
        return gb

    def __iter__(self):
        it = iter(self.source)
        try:
            nxt = self._build(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur = nxt
            try:
                nxt = self._build(next(it))       # issued before the consumer enqueues its step on batch `cur`
            except StopIteration:
                nxt = None
            yield self._hand_over(*cur)


def selection_mask(select, N, device):
    """The int32 0/1 mask [N] on ``device`` of a selection as ``GraphBatch.restrict`` reads it (validated the same way):
    for callers that repeat or combine selections before restricting, e.g. one selection in every replica."""
    return _select_seed(select, N, device)[0]


def _select_seed(select, N, device):
    """(seed [N] int32 on the device, sorted host indices or None) of a selection.  The dtype decides the reading, never the
    values: bool [N], or floating point [N] holding only 0.0 and 1.0, is a mask; every integer array is a list of INDICES
    (so an integer 0-1 array is not a mask: convert it with ``.astype(bool)``).  Host inputs are validated on the host;
    a device bool mask is only shape-checked (no read-back); any other device tensor is copied to the host first."""
    if isinstance(select, torch.Tensor) and select.is_cuda:
        if select.dtype == torch.bool:
            if select.dim() != 1 or select.shape[0] != N:
                raise ValueError(f"restrict: a mask needs {N} entries, got {tuple(select.shape)}")
            return select.to(device=device, dtype=torch.int32).contiguous(), None
        select = select.cpu()              # index arrays are checked on the host: a host synchronisation of its own
    s = select.numpy() if isinstance(select, torch.Tensor) else np.asarray(select)
    if s.ndim != 1:
        raise ValueError(f"restrict: select must be a mask [N] or an index array, got shape {s.shape}")
    if s.dtype == np.bool_:
        if s.shape[0] != N:
            raise ValueError(f"restrict: a mask needs {N} entries, got {s.shape[0]}")
        idx = np.nonzero(s)[0]
    elif np.issubdtype(s.dtype, np.integer):
        idx = s.astype(np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= N):
            raise ValueError(f"restrict: indices must lie in [0, {N})")
        idx = np.sort(idx)
        if (np.diff(idx) == 0).any():
            raise ValueError("restrict: an index is given twice")
    elif np.issubdtype(s.dtype, np.floating) and s.shape[0] == N and np.isin(s, (0.0, 1.0)).all():
        idx = np.nonzero(s)[0]
    else:
        raise ValueError("restrict: select must be a bool / 0-1 mask [N] or an integer index array")
    if len(idx) == 0:
        raise ValueError("restrict: nothing selected")
    seed = np.zeros(N, dtype=np.int32)
    seed[idx] = 1
    return torch.from_numpy(seed).to(device), idx.astype(np.int64)


class _PrunedEdges(torch.autograd.Function):
    """the edges of a restricted batch as a function of the parent's (the pruned batch's own tensor, not a copy); the
    backward is ng_prune_expand_edge_grad"""

    @staticmethod
    def forward(ctx, parent_edges, expansion, holder):
        ctx.expansion = expansion
        return holder.pop("edges")

    @staticmethod
    def backward(ctx, dedges):
        return ctx.expansion.edge_grad(dedges), None, None


def _box_dims_grad(dims, dvec):
    """d(loss)/d(a, b, c, alpha, beta, gamma) from dvec = d(loss)/d(lattice vectors) [G, 3, 3]: the chain rule through the
    float64 restatement of the conversion (pbc.triclinic_vectors_torch); a shared [6] box sums over the frames"""
    with torch.enable_grad():
        d = dims.detach().to(dtype=torch.float64).requires_grad_(True)
        h = triclinic_vectors_torch(d.expand(dvec.shape[0], 6) if d.dim() == 1 else d)
        (g,) = torch.autograd.grad(h, d, dvec.to(device=d.device))
    return g.to(dtype=dims.dtype)


class _EdgesOfPositions(torch.autograd.Function):
    """edges = |r_i - r_j| * scale of a batch built from ``frames`` (the batch's own edges tensor, not a copy); the
    backward is ng_positions_grad at fixed neighbour lists, and, for a ``box`` tensor that requires grad, ng_box_grad
    chained through the box conversion"""

    @staticmethod
    def forward(ctx, frames, box, build, holder):
        # a copy of the positions: an in-place update of ``frames`` before the backward must not move the lists' atoms
        batch = holder["batch"] = build(frames.detach().clone() if isinstance(frames, torch.Tensor) else frames)
        ctx.geometry = batch.geometry(incoming=ctx.needs_input_grad[0])
        ctx.box_dims = box.detach().clone() if ctx.needs_input_grad[1] else None
        if ctx.needs_input_grad[0]:
            ctx.frames_shape, ctx.frames_device = frames.shape, frames.device
        return batch.edges

    @staticmethod
    def backward(ctx, dedges):
        dpos = dbox = None
        if ctx.needs_input_grad[0]:
            dpos = ctx.geometry.positions_grad(dedges).reshape(ctx.frames_shape).to(ctx.frames_device)
        if ctx.needs_input_grad[1]:
            dbox = _box_dims_grad(ctx.box_dims, ctx.geometry.box_grad(dedges)[1])
        return dpos, dbox, None, None


def _positions_batch(frames, build, box=None):
    """``build(frames)`` with edges that carry a grad_fn back to ``frames`` and to a ``box`` tensor when they require
    grad"""
    box_grad = isinstance(box, torch.Tensor) and box.requires_grad
    if not ((isinstance(frames, torch.Tensor) and frames.requires_grad or box_grad) and torch.is_grad_enabled()):
        return build(frames)
    holder = {}
    edges = _EdgesOfPositions.apply(frames, box if box_grad else None, build, holder)
    batch = holder.pop("batch")
    batch.edges = edges         # the same storage the kernels read, now with a grad_fn
    return batch


def batch_from_positions(atoms, pos, layout, scale, boundary, K=None, cutoff=None, out=None):
    """The one list-build path: the batch of device ``atoms`` [N, C] and device positions ``pos`` under ``layout`` and
    ``boundary``, with its geometry attached.  ``cutoff`` None: padded kNN lists with ``K`` neighbours, one library call
    and no host synchronisation; ``out``: (nlist [N, K], edges [N, K], inv_degree [N]) allocated by the caller (a captured
    chain writes into static buffers).  Else the CSR lists of the cutoff: count, scan, size the buffers, fill."""
    N, dev = layout.N, pos.device
    new = partial(torch.empty, dtype=torch.int32, device=dev)
    with library_calls(None, dev) as call:
        if cutoff is None:
            nlist, edges, inv = out or (new(N, K), new(N, K, dtype=torch.float32), new(N, dtype=torch.float32))
            call(*knn_call(layout, boundary, K, scale, pos, nlist, edges, inv))
            # every graph larger than K: every atom has K real neighbours, no padded slot -> the compute-side list IS the list
            b = GraphBatch(atoms, nlist, edges, inv, graph_ptr=layout.graph_ptr_host, device=dev, validate=False,
                           nlist_c=nlist if layout.min_n > K else None)
        else:
            deg, row_ptr = new(N), new(N + 1)
            call(*cutoff_count_call(layout, boundary, cutoff, pos, deg))
            call("ng_exclusive_scan_i32", (N, ptr(deg), ptr(row_ptr)))
            # the one host synchronisation: the list length sizes the buffers.  Summed in int64 — the device scan is int32
            # and a total of 2^32 or more would wrap back to a plausible positive number
            nnz = int(deg.sum(dtype=torch.int64))
            if nnz >= 2 ** 31:
                raise ValueError("cutoff graph: more than 2^31 edges in one batch")
            col, dist, row_of, inv = new(nnz), new(nnz, dtype=torch.float32), new(nnz), new(N, dtype=torch.float32)
            call(*cutoff_fill_call(layout, boundary, cutoff, scale, pos, row_ptr, col, dist, inv, row_of))
            b = GraphBatch.from_csr(atoms, row_ptr, col, dist, inv, graph_ptr=layout.graph_ptr_host, device=dev,
                                    validate=False, row_of=row_of)
    b.set_geometry(pos, scale, boundary)
    return b


def _host_box(box, frames):
    """None, or (vectors [G, 9] float32, triclinic flag, smallest perpendicular widths [G]): validated on the host.  A torch
    ``box`` gives what its detached host copy gives."""
    if box is None:
        return None
    if isinstance(box, torch.Tensor):
        box = box.detach().cpu().numpy()
    shape = tuple(frames.shape) if hasattr(frames, "shape") else np.shape(frames)
    return prepare(box, 1 if len(shape) == 2 else int(shape[0]))


def frames_to_batch(atoms, frames, neighbor_number=16, scale=0.1, device=None, box=None):
    """Build the graphs of ``G`` trajectory frames on the GPU (ng_knn_graph) and return them as one
    device-resident GraphBatch: ``atoms`` [n,C] one-hot (shared by all frames), ``frames`` [G,n,3]
    positions in Angstrom.  Same conventions as :func:`nmrgnn_amd.structure.knn_graph`.
    The batch keeps the positions and ``scale`` (``GraphBatch.positions_grad``); with ``frames.requires_grad`` (and
    grad mode on) its ``edges`` carry a grad_fn back to ``frames``, so a loss of ``model(batch)`` differentiates to
    ``frames.grad`` — at fixed neighbour lists, as TensorFlow's tape does through the reference's graph.

    ``box``: periodic boxes under the minimum-image convention (csrc/pbc.cuh), ``(a, b, c, alpha, beta, gamma)`` in
    Angstrom and degrees, [6] for every frame or [G, 6] one per frame (nmrgnn_amd.pbc: orthorhombic and reduced triclinic
    boxes).  Positions may lie anywhere; nothing is wrapped.  The batch keeps the box (``GraphBatch.box``) and its
    gradient uses the minimum-image vector of each edge.  None: open boundaries, as before.  A torch ``box`` that requires
    grad (and grad mode on) gets ``box.grad`` from a loss of ``model(batch)``: ``GraphBatch.box_grad`` chained through the
    box conversion (nmrgnn_amd.pbc.triclinic_vectors_torch), at fixed lists and images, summed over the frames of a
    shared [6] box; the lists are those of ``box.detach().cpu().numpy()``."""
    pbc = _host_box(box, frames)
    return _positions_batch(frames, lambda f: _frames_batch(atoms, f, scale, device, pbc, K=int(neighbor_number)), box)


def _frames_batch(atoms, frames, scale, device, pbc, K=None, cutoff=None):
    """the positions and atoms of G frames on the device, then the one list-build path"""
    device = _norm_device(device)
    pos = _to_dev(np.asarray(frames, dtype=np.float32) if not isinstance(frames, torch.Tensor) else frames,
                  torch.float32, device)
    if pos.dim() == 2:
        pos = pos[None]
    G, n, _ = pos.shape
    at = _to_dev(atoms, torch.float32, device)
    if at.shape[0] != n:
        raise ValueError(f"atoms has {at.shape[0]} rows but frames have {n} atoms")
    return batch_from_positions(at.repeat(G, 1) if G > 1 else at, pos, Layout.frames(G, n), scale,
                                Boundary.from_host(pbc, device), K, cutoff)


def frames_to_batch_cutoff(atoms, frames, cutoff=4.0, scale=0.1, device=None, box=None):
    """Distance-cutoff graphs of ``G`` trajectory frames, built on the GPU (ng_cutoff_count / ng_cutoff_fill) and
    returned as one device-resident CSR GraphBatch: every other atom of the same frame closer than ``cutoff``
    (Angstrom) is a neighbour, rows in ascending neighbour index, distances x ``scale`` (nm), inv_degree by the
    reference's rule (library.py:115-116).  Variable degree: BASELINE configs[4].
    Positions, gradients and ``box`` as in :func:`frames_to_batch`; with a box, ``cutoff`` must stay below half the
    smallest perpendicular width of every frame's box (one image per neighbour)."""
    pbc = _host_box(box, frames)
    if pbc is not None and len(pbc[2]) and not float(cutoff) < 0.5 * float(pbc[2].min()):
        raise ValueError(f"cutoff {cutoff} must be below half the smallest box width ({0.5 * float(pbc[2].min()):.6g})")
    return _positions_batch(frames, lambda f: _frames_batch(atoms, f, scale, device, pbc, cutoff=cutoff), box)


def _cat_rows(parts, device):
    """one [N, ...] array from per-structure parts: a torch tensor (on ``device``, grad kept) when any part is one"""
    if any(isinstance(p, torch.Tensor) for p in parts):
        return torch.cat([torch.as_tensor(p).to(device=device, dtype=torch.float32) for p in parts])
    return np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])


def _ragged_inputs(atoms, positions, sizes, graph_ptr, device):
    """(atoms [N, C], positions [N, 3], graph_ptr [G+1] int64 on the host), validated before any device work"""
    if isinstance(atoms, (list, tuple)) or isinstance(positions, (list, tuple)):
        if not (isinstance(atoms, (list, tuple)) and isinstance(positions, (list, tuple))):
            raise ValueError("structures_to_batch: atoms and positions must both be lists, or both concatenated arrays")
        if sizes is not None or graph_ptr is not None:
            raise ValueError("structures_to_batch: sizes= / graph_ptr= go with concatenated arrays, not with lists")
        if len(atoms) != len(positions):
            raise ValueError(f"structures_to_batch: {len(atoms)} atom arrays but {len(positions)} position arrays")
        n = []
        for g, (a, p) in enumerate(zip(atoms, positions)):
            sa, sp = tuple(np.shape(a)), tuple(np.shape(p))
            if len(sa) != 2 or len(sp) != 2 or sp[1] != 3:
                raise ValueError(f"structures_to_batch: structure {g}: atoms must be [n, C] and positions [n, 3]")
            if sa[0] != sp[0]:
                raise ValueError(f"structures_to_batch: structure {g}: {sa[0]} atom rows but {sp[0]} positions")
            n.append(sa[0])
        sizes = np.asarray(n, dtype=np.int64)
        if len(sizes) == 0:
            raise ValueError("structures_to_batch: no structures")
        if (sizes == 0).any():
            raise ValueError(f"structures_to_batch: structure {int(np.argmax(sizes == 0))} has no atoms")
        atoms, positions = _cat_rows(atoms, device), _cat_rows(positions, device)
    else:
        sa, sp = tuple(np.shape(atoms)), tuple(np.shape(positions))
        if len(sa) != 2 or len(sp) != 2 or sp[1] != 3:
            raise ValueError("structures_to_batch: atoms must be [N, C] and positions [N, 3]")
        if sa[0] != sp[0]:
            raise ValueError(f"structures_to_batch: {sa[0]} atom rows but {sp[0]} positions")
        if (sizes is None) == (graph_ptr is None):
            raise ValueError("structures_to_batch: concatenated arrays need exactly one of sizes= or graph_ptr=")
        if sizes is not None:
            sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
        else:
            gp = np.asarray(graph_ptr, dtype=np.int64).reshape(-1)
            if len(gp) < 1 or gp[0] != 0:
                raise ValueError("structures_to_batch: graph_ptr must start at 0")
            sizes = np.diff(gp)
        if len(sizes) == 0:
            raise ValueError("structures_to_batch: no structures")
        if (sizes <= 0).any():
            raise ValueError(f"structures_to_batch: structure {int(np.argmax(sizes <= 0))} has no atoms")
        if int(sizes.sum()) != sa[0]:
            raise ValueError(f"structures_to_batch: the structures hold {int(sizes.sum())} atoms, the arrays {sa[0]}")
    gp = np.zeros(len(sizes) + 1, dtype=np.int64)
    gp[1:] = np.cumsum(sizes)
    if gp[-1] >= 2 ** 31:
        raise ValueError("structures_to_batch: more than 2^31 - 1 atoms in one batch")
    return atoms, positions, gp


def _ragged_count(atoms, sizes, graph_ptr):
    """the number of structures as the caller states it, or None where _ragged_inputs will refuse the call anyway"""
    if isinstance(atoms, (list, tuple)):
        return len(atoms)
    if sizes is not None:
        return int(np.size(sizes))
    if graph_ptr is not None:
        return int(np.size(graph_ptr)) - 1
    return None


def _host_boxes(boxes, G, cutoff):
    """None (every structure open), or pbc.prepare_ragged's (vectors, kinds, widths) for G structures, validated on the host"""
    if boxes is None:
        return None
    pr = prepare_ragged(boxes, G)
    if not (pr[1] >= 0).any():
        return None
    if cutoff is not None:
        for g in np.nonzero(pr[1] >= 0)[0]:
            if not float(cutoff) < 0.5 * float(pr[2][g]):
                raise ValueError(f"structures_to_batch: structure {int(g)}: cutoff {cutoff} must be below half the smallest box "
                                 f"width ({0.5 * float(pr[2][g]):.6g})")
    return pr


def structures_to_batch(atoms, positions, neighbor_number=16, cutoff=None, scale=0.1, device=None, sizes=None,
                        graph_ptr=None, box=None, boxes=None):
    """Build the graphs of G DIFFERENT structures on the GPU in one launch per pass and return them as one device-resident
    GraphBatch with ``graph_ptr`` set: a library of small molecules, several proteins, a training set given as coordinates.

    ``atoms`` / ``positions``: lists of per-structure ``[n_g, C]`` one-hot and ``[n_g, 3]`` Angstrom arrays, or the
    concatenated ``[N, C]`` / ``[N, 3]`` with ``sizes=`` [G] or ``graph_ptr=`` [G+1].  Only atoms of the same structure are
    neighbours.  ``cutoff=None``: the padded kNN lists of :func:`frames_to_batch` (ng_knn_graph_ragged) with
    ``neighbor_number`` neighbours; a cutoff in Angstrom: the CSR lists of :func:`frames_to_batch_cutoff`
    (ng_cutoff_count_ragged / ng_cutoff_fill_rows_ragged).  Each structure's rows are bit for bit that builder's lists for
    the structure alone, with indices shifted to the batch; a one-atom structure has only padded slots and inv_degree 0.

    The batch keeps the concatenated positions [N, 3] and ``scale``; with a ``positions`` tensor (or list of tensors) that
    requires grad its ``edges`` carry a grad_fn back to them, as in :func:`frames_to_batch`.

    ``boxes``: one periodic box, or none, per structure (csrc/pbc.cuh: DispPer): a sequence of G entries, each ``None`` (open
    boundaries) or ``(a, b, c, alpha, beta, gamma)`` as in :func:`frames_to_batch`, or a ``[G, 6]`` array or tensor (every
    structure periodic).  Every structure keeps a boundary kind of its own (open, orthorhombic or reduced triclinic): its rows
    are bit for bit what :func:`frames_to_batch` / :func:`frames_to_batch_cutoff` give for it alone with its own box, or
    without one.  Positions may lie anywhere; nothing is wrapped.  ``cutoff`` must stay below half the smallest perpendicular
    width of every periodic structure.  The batch keeps ``box`` [G, 9] (zeros for open structures) and ``box_kind`` [G];
    ``positions_grad`` and ``box_grad`` use each structure's own minimum-image vectors.  A ``[G, 6]`` tensor that requires grad
    gets ``boxes.grad`` as ``box`` does in :func:`frames_to_batch`; entries of the list form are not differentiated.
    ``boxes=None``, or only ``None`` entries: open boundaries, the same calls as without the argument.  The singular ``box=``
    of the uniform builders raises ValueError here."""
    if box is not None:
        raise ValueError("structures_to_batch: periodic boxes are not supported through box= on ragged batches; give one box "
                         "(or None) per structure with boxes=, or use frames_to_batch")
    K = int(neighbor_number)
    if not 1 <= K <= 64:
        raise ValueError(f"structures_to_batch: neighbor_number must be in [1, 64], got {neighbor_number}")
    if cutoff is not None and not float(cutoff) > 0:
        raise ValueError(f"structures_to_batch: cutoff must be > 0, got {cutoff}")
    device = _norm_device(device)
    # the boxes are validated before any device work, against the count the caller states; where the caller states none
    # (_ragged_inputs refuses such a call), or states one that the arrays contradict, against the count _ragged_inputs finds
    G = _ragged_count(atoms, sizes, graph_ptr)
    pr = _host_boxes(boxes, G, cutoff) if G is not None else None
    atoms, pos, gp = _ragged_inputs(atoms, positions, sizes, graph_ptr, device)
    if G != len(gp) - 1:
        pr = _host_boxes(boxes, len(gp) - 1, cutoff)
    if cutoff is None and int(gp[-1]) * K >= 2 ** 31:
        raise ValueError("structures_to_batch: N * neighbor_number exceeds 2^31 - 1 slots")
    return _positions_batch(pos, lambda f: _structures_batch(atoms, f, gp, K, cutoff, scale, device, pr),
                            boxes if pr is not None and isinstance(boxes, torch.Tensor) else None)


def _structures_batch(atoms, positions, gp, K, cutoff, scale, device, pr=None):
    """the concatenated positions and atoms and the partition on the device, then the one list-build path"""
    pos = _to_dev(positions, torch.float32, device).reshape(-1, 3)
    at = _to_dev(atoms, torch.float32, device)
    gp_host = gp.astype(np.int32)
    return batch_from_positions(at, pos, Layout.ragged(gp_host, _graph_ptr_dev(gp_host, device)), scale,
                                Boundary.from_host(pr, device), K, cutoff)
