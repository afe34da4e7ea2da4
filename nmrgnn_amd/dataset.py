"""``ShiftDataset`` — a ragged record store in device memory, and mini-batches from it in one launch.

A record is what the reference's ``nmrdata.dataset(..., label_info=True)`` yields (nmrgnn/library.py:50-89):
``x = (atoms[n, C], nlist[n, K], edges[n, K], inv_degree[n])``, ``y[n, 3]`` = [shift, name id, mask], ``w[n]``.  ``nlist`` is
record-local; padded slots hold ``nlist == 0`` and ``edges == 0``.  The store keeps R records back to back:

    atoms [Ntot, C] f32 (rows as given)     nlist [Ntot, K] i32 (record-local)     edges [Ntot, K] f32
    inv_degree [Ntot] f32 (as given)        y [Ntot, 3] f32                        w [Ntot] f32
    rec_ptr [R + 1] int64 (device and host)  file_ptr [S + 1] int64 (host: the records of source s)

A whole training set fits on the device (100 000 records of up to 256 atoms at K = 16 are about 5 GB), so a mini-batch is
``ng_collate_batch`` (csrc/collate.hip) away: the host knows every record's size, forms ``graph_ptr`` by a NumPy cumsum,
sends it with the record ids in ONE small copy, and one launch writes the batch — the arrays of ``graph.concat_graphs``
over the same records in the same order, bit for bit.  Everything is validated once, when the store is built; a batch
checks nothing and never reads the device.

On a CPU device ``batch`` does the same with torch indexing (host tests, shard bookkeeping).

Ensemble groups: ``group_ptr`` [S + 1] (host int64 over the view's records) makes consecutive records of
one structure — its frames, with equal sizes and labels — one group; training and evaluation then take the loss on the mean
prediction of a group.  A grouped store splits, permutes and cuts by groups and yields the batch's ``group_ptr`` beside each
batch; an ungrouped one (every record its own group) behaves as it always did.

``from_structures`` fills a store from structures and shift tables, the lists built on the GPU and written into the store by
``ng_store_from_batch`` (csrc/records.hip); ``standards()`` gives the per-element label statistics of a view
(``ng_label_moments``) for ``build_GNNModel(peak_standards=)``."""
from __future__ import annotations

import numpy as np
import torch

from .graph import BatchPrefetcher, GraphBatch, _norm_device

FORMAT_VERSION = 1
_ARRAYS = ("atoms", "nlist", "edges", "inv_degree", "y", "w")
_DTYPES = {"atoms": np.float32, "nlist": np.int32, "edges": np.float32, "inv_degree": np.float32, "y": np.float32,
           "w": np.float32}
_TORCH_DTYPES = {k: (torch.int32 if v is np.int32 else torch.float32) for k, v in _DTYPES.items()}
_MAX_BATCH_ATOMS = 2 ** 31 - 256          # ng_collate_batch's limit on N


def _check_record(r, rec, C, K):
    """one ``(x, y, w)`` tuple -> its six host arrays, or ValueError naming record ``r``"""
    try:
        x, y, w = rec
        atoms, nlist, edges, inv = x
    except (TypeError, ValueError):
        raise ValueError(f"record {r}: expected ((atoms, nlist, edges, inv_degree), y, w)") from None
    atoms, nlist_raw, edges = np.asarray(atoms), np.asarray(nlist), np.asarray(edges)
    inv, y, w = np.asarray(inv).reshape(-1), np.asarray(y), np.asarray(w).reshape(-1)
    if atoms.ndim != 2 or nlist_raw.ndim != 2 or edges.ndim != 2 or y.ndim != 2 or y.shape[1] != 3:
        raise ValueError(f"record {r}: atoms must be [n, C], nlist and edges [n, K], y [n, 3]")
    n = atoms.shape[0]
    if n == 0:
        raise ValueError(f"record {r}: no atoms")
    if atoms.shape[1] < 1 or nlist_raw.shape[1] < 1:
        raise ValueError(f"record {r}: C and K must be at least 1")
    if C is not None and (atoms.shape[1] != C or nlist_raw.shape[1] != K):
        raise ValueError(f"record {r}: C = {atoms.shape[1]}, K = {nlist_raw.shape[1]}, but the records before it have "
                         f"C = {C}, K = {K}")
    if nlist_raw.shape[0] != n or tuple(edges.shape) != tuple(nlist_raw.shape) or inv.shape[0] != n or y.shape[0] != n \
            or w.shape[0] != n:
        raise ValueError(f"record {r}: {n} atom rows, but nlist {nlist_raw.shape}, edges {edges.shape}, inv_degree "
                         f"{inv.shape}, y {y.shape}, w {w.shape}")
    nl = nlist_raw.astype(np.int64)
    if not np.array_equal(nl, nlist_raw):
        raise ValueError(f"record {r}: nlist holds values that are no integers")
    if nl.min() < 0 or nl.max() >= n:
        raise ValueError(f"record {r}: nlist entries must lie in [0, {n}); got [{nl.min()}, {nl.max()}]")
    edges = edges.astype(np.float32)
    if not np.isfinite(edges).all() or (edges < 0).any():
        raise ValueError(f"record {r}: edges must be finite and >= 0")
    return (atoms.astype(np.float32), nl.astype(np.int32), edges, inv.astype(np.float32), y.astype(np.float32),
            w.astype(np.float32))


def label_moments_host(atoms, y):
    """float64 [C, 3]: (count, sum y0, sum y0^2) per element over the rows with ``y[:, 2] > 0``; the element of a row is its
    first non-zero atom column, a row without one is skipped (what ``ng_label_moments`` sums on the device)"""
    atoms, y = np.asarray(atoms), np.asarray(y)
    C = atoms.shape[1]
    nz = atoms != 0
    use = (y[:, 2] > 0) & nz.any(axis=1)
    el = np.argmax(nz, axis=1)[use]
    y0 = y[use, 0].astype(np.float64)
    out = np.zeros((C, 3), np.float64)
    out[:, 0] = np.bincount(el, minlength=C)
    out[:, 1] = np.bincount(el, weights=y0, minlength=C)
    out[:, 2] = np.bincount(el, weights=y0 * y0, minlength=C)
    return out


class _StorePrefetcher(BatchPrefetcher):
    """BatchPrefetcher over lists of record ids: batch t + 1 is collated on the side stream, with the side context, while
    step t runs; the label tensors are handed over like the batch's own"""

    def __init__(self, dataset, id_lists):
        super().__init__(id_lists, device=dataset.device)
        self.dataset = dataset
        self._first = True
        if self.device.type == "cuda":
            # one side stream and library context per store, shared by its views and kept across epochs
            side = dataset._side
            if not side:
                from . import _lib
                side["stream"] = torch.cuda.Stream(device=self.device)
                side["ctx"] = _lib.Context(self.device.index)
            self._stream, self._ctx = side["stream"], side["ctx"]

    def _construct(self, ids, ctx):
        return self.dataset._collate(ids, False, ctx)[:4]

    def _device_inputs(self, ids):
        # the store was written long before; only the first batch waits for whatever built it on the consumer's stream
        first, self._first = self._first, False
        return first

    def _hand_over(self, out, ready):
        gb = super()._hand_over(out[0], ready)
        if ready is not None:
            consumer = torch.cuda.current_stream(self.device)
            for t in out[1:]:
                t.record_stream(consumer)
        return (gb,) + tuple(out[1:])


class ShiftDataset:
    """A record store, or a view of one by a list of record ids (``split``); see the module docstring.  ``len()`` is the
    number of records of the view, and every record id a method takes counts within the view."""

    name_table = None      # {'RES-NAME': id} of a store built by from_structures
    join_report = None     # its label-join counts (structure.JOIN_COUNTS, 'rows', 'labelled', 'structures')

    def __init__(self, arrays, rec_ptr, file_ptr, device=None, _ids=None, _parent=None, group_ptr=None):
        if _parent is not None:                       # a view: shares every array
            self.__dict__.update(_parent.__dict__)
            self.record_ids = np.asarray(_ids, np.int64)
            self.group_ptr = self._view_groups(self.record_ids)
            return
        self.device = _norm_device(device)
        self.rec_ptr_host = np.ascontiguousarray(rec_ptr, dtype=np.int64)
        self.file_ptr = np.ascontiguousarray(file_ptr, dtype=np.int64)
        self.R = len(self.rec_ptr_host) - 1
        self.Ntot = int(self.rec_ptr_host[-1])
        for k in _ARRAYS:
            a = arrays[k]
            if isinstance(a, torch.Tensor):           # built on the device (from_structures): taken as it is
                if a.device != self.device or a.dtype != _TORCH_DTYPES[k] or not a.is_contiguous():
                    raise ValueError(f"{k}: a contiguous {_TORCH_DTYPES[k]} tensor on {self.device} expected")
            else:
                a = np.ascontiguousarray(a, dtype=_DTYPES[k])
            if a.shape[0] != self.Ntot:
                raise ValueError(f"{k} has {a.shape[0]} rows, rec_ptr ends at {self.Ntot}")
            setattr(self, k, a if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(self.device))
        self.C, self.K = int(self.atoms.shape[1]), int(self.nlist.shape[1])
        self.rec_ptr = torch.from_numpy(self.rec_ptr_host).to(self.device)
        self._sizes = np.diff(self.rec_ptr_host)
        self._side = {}                               # the prefetcher's stream and context (made at the first epoch)
        self.record_ids = np.arange(self.R, dtype=np.int64)
        # ensemble groups.  Per STORE record: the first record and the size of its group; per view:
        # group_ptr [S + 1] over the view's records.  Ungrouped: every record a group of its own.
        self.grouped = False
        self._group_first = np.arange(self.R, dtype=np.int64)
        self._group_size = np.ones(self.R, np.int64)
        self.group_ptr = np.arange(self.R + 1, dtype=np.int64)
        if group_ptr is not None:
            self._set_groups(group_ptr)

    # ------------------------------------------------------------------ ensemble groups
    def _set_groups(self, group_ptr):
        """make the view's records the groups ``group_ptr`` [S + 1]; ``ValueError`` naming the group whose members are not
        consecutive store records of one size"""
        gp = np.asarray(group_ptr)
        n = len(self.record_ids)
        if gp.ndim != 1 or len(gp) < 1 or not np.issubdtype(gp.dtype, np.integer):
            raise ValueError("group_ptr must be a 1-D integer array")
        gp = gp.astype(np.int64)
        if gp[0] != 0 or gp[-1] != n or (np.diff(gp) < 1).any():
            raise ValueError(f"group_ptr must rise strictly from 0 to the {n} records")
        if self.grouped:
            raise ValueError("the store is grouped already")
        counts = np.diff(gp)
        ids = self.record_ids
        first = np.repeat(ids[gp[:-1]], counts)
        offs = np.arange(n) - np.repeat(gp[:-1], counts)
        group_of = np.repeat(np.arange(len(counts)), counts)
        bad = np.flatnonzero(ids != first + offs)
        if len(bad):
            raise ValueError(f"group {int(group_of[bad[0]])}: its members are not consecutive records of the store")
        bad = np.flatnonzero(self._sizes[ids] != self._sizes[first])
        if len(bad):
            raise ValueError(f"group {int(group_of[bad[0]])}: record {int(bad[0])} has {int(self._sizes[ids[bad[0]]])} atoms, "
                             f"the group's first member {int(self._sizes[first[bad[0]]])}")
        self._group_first, self._group_size = self._group_first.copy(), self._group_size.copy()
        self._group_first[ids] = first
        self._group_size[ids] = np.repeat(counts, counts)
        self.group_ptr = gp
        self.grouped = True

    def _view_groups(self, ids):
        """group_ptr of a view of the records ``ids`` (store ids); ``ValueError`` when the view breaks a group: every group
        it touches must be there whole, its members in their order"""
        n = len(ids)
        if not self.grouped:
            return np.arange(n + 1, dtype=np.int64)
        first = self._group_first[ids]
        head = np.flatnonzero(ids == first)                     # view positions that hold a group's first member
        gp = np.concatenate([head, [n]]).astype(np.int64)
        counts = np.diff(gp)
        ok = n == 0 or (len(head) > 0 and head[0] == 0 and np.array_equal(counts, self._group_size[ids[head]]) and
                        np.array_equal(ids, np.repeat(ids[head], counts) + np.arange(n) - np.repeat(head, counts)))
        if not ok:
            raise ValueError("the records of a view of a grouped store must be whole groups, their members in order")
        return gp

    def _label_mismatch(self, gp):
        """index of the first group of ``gp`` (over the view's records) whose members differ from its first member in a ``y``,
        ``w`` or ``atoms`` row, or -1: one comparison on the store's device, one read"""
        counts = np.diff(gp)
        multi = np.flatnonzero(counts > 1)
        if len(multi) == 0:
            return -1
        ids = self.record_ids
        a_parts, b_parts, g_parts = [], [], []
        for q in multi:                                         # rows of the members r >= 1 against the first member's
            r0 = int(self.rec_ptr_host[ids[gp[q]]])
            n = int(self._sizes[ids[gp[q]]])
            extra = (int(counts[q]) - 1) * n
            a_parts.append(r0 + n + np.arange(extra))
            b_parts.append(r0 + np.arange(extra) % n)
            g_parts.append(np.full(extra, q, np.int64))
        a = torch.from_numpy(np.concatenate(a_parts)).to(self.device)
        b = torch.from_numpy(np.concatenate(b_parts)).to(self.device)
        bits = lambda t: t.view(torch.int32)                    # bit patterns: equal labels, NaN included
        neq = (bits(self.y)[a] != bits(self.y)[b]).any(dim=1) | (bits(self.w)[a] != bits(self.w)[b]) \
            | (bits(self.atoms)[a] != bits(self.atoms)[b]).any(dim=1)
        hit, where = (int(v) for v in torch.stack([neq.any().to(torch.int64), torch.argmax(neq.to(torch.int8))]).cpu())
        return int(np.concatenate(g_parts)[where]) if hit else -1

    def with_groups(self, group_ptr):
        """A grouped store over the same arrays: the view's records ``[group_ptr[q], group_ptr[q+1])`` are the frames of one
        structure (``group_ptr`` host integers [S + 1], from 0 to ``len(self)``, strictly increasing).  Checked here, once:
        the members of a group are consecutive records of the store with equal sizes (host) and equal ``y``, ``w`` and
        ``atoms`` rows (one device comparison, one host read); ``ValueError`` naming the group otherwise.  No data is
        copied."""
        new = ShiftDataset(None, None, None, _ids=self.record_ids, _parent=self)
        new._set_groups(group_ptr)
        q = new._label_mismatch(new.group_ptr)
        if q >= 0:
            raise ValueError(f"group {q}: its members differ in their y, w or atoms rows; the frames of one structure carry "
                             "the same labels")
        return new

    def group_sizes(self):
        """members of every group of the view (host)"""
        return np.diff(self.group_ptr)

    def _batch_groups(self, ids):
        """int32 group_ptr [Q + 1] of the batch of the view's records ``ids``; ``ValueError`` when they are not whole groups"""
        ids = np.asarray(ids, np.int64).reshape(-1)
        if len(ids) == 0 or ids.min() < 0 or ids.max() >= len(self.record_ids):
            raise ValueError(f"batch: record ids must lie in [0, {len(self.record_ids)})")
        return self._view_groups(self.record_ids[ids]).astype(np.int32)

    def _group_lists(self, order, batch_graphs):
        """record-id lists of batches of ``batch_graphs`` GROUPS in the group order ``order``"""
        gp = self.group_ptr
        return [np.concatenate([np.arange(gp[q], gp[q + 1]) for q in order[i:i + batch_graphs]]).astype(np.int64)
                for i in range(0, len(order), batch_graphs)]

    # ------------------------------------------------------------------ building, files
    @classmethod
    def from_records(cls, records, device=None):
        """The store of an iterable of the reference's ``(x, y, w)`` tuples (anything with ``__array__``: a user with
        TensorFlow and nmrdata converts once).  Validated here, once: ``ValueError`` naming the record for C or K that
        differ between records, ``nlist`` outside [0, n), negative or non-finite ``edges``, a row-count mismatch, n == 0."""
        parts, C, K = [], None, None
        for r, rec in enumerate(records):
            arrs = _check_record(r, rec, C, K)
            C, K = arrs[0].shape[1], arrs[1].shape[1]
            parts.append(arrs)
        if not parts:
            raise ValueError("from_records: no records")
        arrays = {k: np.concatenate([p[i] for p in parts]) for i, k in enumerate(_ARRAYS)}
        rec_ptr = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])])
        return cls(arrays, rec_ptr, [0, len(parts)], device=device)

    @classmethod
    def from_structures(cls, structures, shifts, neighbor_number=16, frames='first', names=None, boxes=False, strict=True,
                        chunk_atoms=1 << 20, device=None, ensembles=False):
        """The store of structures with assigned shifts: one record per structure (``frames='first'``) or
        per frame of it (``frames='all'``, every frame with the structure's labels), kNN lists of ``neighbor_number``
        neighbours, one source (``file_ptr = [0, R]``).  ``ensembles=True`` (with ``frames='all'``): the frames of every
        structure are one ensemble group (``group_ptr``), so that training fits their MEAN to the labels.

        ``structures``: ``structure.Structure`` objects or PDB paths.  ``shifts``: per structure a table (the dict of
        ``structure.read_shift_table``), a path to one, or ``None`` (no labels).  Labels are joined on the host by ``(resid,
        atom name)`` (``structure.join_shifts``): with ``strict`` a table row that matches no atom, two atoms, another
        residue name or an atom already labelled raises ``ValueError`` naming the structure and the row; otherwise such rows
        are dropped and counted in ``join_report`` on the returned store.  ``names``: a ``{'RES-NAME': id}`` table (default
        ``structure.name_table(structures)``; kept as ``name_table``); an atom whose key it lacks gets id 0.  A labelled atom
        has ``y = (shift, id, 1)`` and ``w = 1``, every other ``y = (0, id, 0)`` and ``w = 0``.

        On the GPU the structures go through ``graph.structures_to_batch`` in chunks of at most ``chunk_atoms`` atoms (a
        larger structure is a chunk of its own), each chunk written by one ``ng_store_from_batch`` launch into store arrays
        allocated once at their final size; the launch's two counters are read once, at the end.  ``boxes=True``: every
        frame's ``Structure.dimensions`` goes to ``structures_to_batch(boxes=)``.  On a CPU device the same arrays come
        from ``structure.knn_graph`` per record and NumPy (host tests; no periodic boxes).  A slot whose distance is not
        > 0 (padding, coincident atoms) holds ``nlist = 0, edges = 0``; ``inv_degree`` is ``structure.inv_degree_of`` of the
        stored list."""
        import os
        from .structure import (Structure, atoms_onehot, inv_degree_of, join_shifts, knn_graph, name_ids, name_keys,
                                name_table, read_pdb, read_shift_table)
        if frames not in ('first', 'all'):
            raise ValueError(f"from_structures: frames is 'first' or 'all', got {frames!r}")
        if ensembles and frames != 'all':
            raise ValueError("from_structures: ensembles=True groups the frames of a structure and needs frames='all'")
        structures = list(structures)
        shifts = list(shifts) if shifts is not None else [None] * len(structures)
        if not structures:
            raise ValueError("from_structures: no structures")
        if len(shifts) != len(structures):
            raise ValueError(f"from_structures: {len(structures)} structures but {len(shifts)} shift tables")
        K, chunk_atoms = int(neighbor_number), int(chunk_atoms)
        if not 1 <= K <= 64:
            raise ValueError(f"from_structures: neighbor_number must be in [1, 64], got {neighbor_number}")
        if chunk_atoms < 1:
            raise ValueError(f"from_structures: chunk_atoms must be >= 1, got {chunk_atoms}")
        device = _norm_device(device)
        labels = [str(s) if isinstance(s, (str, os.PathLike)) else f"structure {k}" for k, s in enumerate(structures)]
        structs = [read_pdb(s) if isinstance(s, (str, os.PathLike)) else s for s in structures]
        for k, s in enumerate(structs):
            if not isinstance(s, Structure) or s.n_atoms == 0 or len(s) == 0:
                raise ValueError(f"from_structures: {labels[k]}: a Structure with atoms and at least one frame expected")
        keys = [name_keys(s) for s in structs]
        table = dict(names) if names is not None else name_table(structs, keys)
        report = {"structures": len(structs), "rows": 0}
        per = []                                      # per structure: (atoms one-hot, shift or NaN, name id)
        for k, (s, t) in enumerate(zip(structs, shifts)):
            if isinstance(t, (str, os.PathLike)):
                t = read_shift_table(t)
            sh, rep = join_shifts(s, t, strict=strict, label=labels[k])
            report["rows"] += 0 if t is None else len(t["shift"])
            for key, v in rep.items():
                report[key] = report.get(key, 0) + v
            per.append((atoms_onehot(s.elements), sh, name_ids(s, table, keys[k])))
        items = [(k, fr) for k, s in enumerate(structs) for fr in (range(len(s)) if frames == 'all' else (0,))]
        sizes = np.asarray([structs[k].n_atoms for k, _ in items], np.int64)
        rec_ptr = np.zeros(len(items) + 1, np.int64)
        np.cumsum(sizes, out=rec_ptr[1:])
        Ntot, C = int(rec_ptr[-1]), per[0][0].shape[1]
        if device.type != "cuda":
            if boxes:
                raise ValueError("from_structures: periodic boxes need the GPU list builder")
            parts = {k: [] for k in _ARRAYS}
            for k, fr in items:
                atoms, sh, ids = per[k]
                nlist, edges = knn_graph(structs[k].frames[fr], K)
                live = edges > 0
                nlist, edges = np.where(live, nlist, 0).astype(np.int32), np.where(live, edges, 0).astype(np.float32)
                has = np.isfinite(sh)
                mask = has.astype(np.float32)
                parts["atoms"].append(atoms)
                parts["nlist"].append(nlist)
                parts["edges"].append(edges)
                parts["inv_degree"].append(inv_degree_of(nlist))
                parts["y"].append(np.stack([np.where(has, sh, 0).astype(np.float32), ids.astype(np.float32), mask], axis=1))
                parts["w"].append(mask)
            ds = cls({k: np.concatenate(v) for k, v in parts.items()}, rec_ptr, [0, len(items)], device=device)
            report["labelled"] = int(ds.w.sum().item())
        else:
            import ctypes as C_
            from . import _lib
            from ._lib import ptr
            from .graph import structures_to_batch
            ctx = _lib.get_context(device.index)
            shape = {"atoms": (Ntot, C), "nlist": (Ntot, K), "edges": (Ntot, K), "inv_degree": (Ntot,), "y": (Ntot, 3),
                     "w": (Ntot,)}
            arrays = {k: torch.empty(shape[k], dtype=_TORCH_DTYPES[k], device=device) for k in _ARRAYS}
            counters = torch.zeros(2, dtype=torch.int32, device=device)
            a = 0
            while a < len(items):                     # items [a, b): as many as fit chunk_atoms, at least one
                b, n = a + 1, int(sizes[a])
                while b < len(items) and n + int(sizes[b]) <= chunk_atoms:
                    n += int(sizes[b])
                    b += 1
                if n >= _MAX_BATCH_ATOMS:
                    raise ValueError(f"from_structures: {n} atoms in one chunk")
                chunk = items[a:b]
                gb = structures_to_batch([per[k][0] for k, _ in chunk], [structs[k].frames[fr] for k, fr in chunk], K,
                                         device=device,
                                         boxes=[structs[k].dimensions[fr] for k, fr in chunk] if boxes else None)
                # labels and name ids of the chunk in ONE copy: the shifts' bits ride as int32
                meta = torch.from_numpy(np.concatenate([np.concatenate([per[k][1] for k, _ in chunk]).view(np.int32),
                                                        np.concatenate([per[k][2] for k, _ in chunk])])).to(device)
                with torch.cuda.device(device):
                    st = C_.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                    ctx.check(ctx.lib.ng_store_from_batch(
                        ctx.handle, st, n, K, C, len(chunk), ptr(gb.graph_ptr), ptr(gb.atoms), ptr(gb.nlist), ptr(gb.edges),
                        ptr(meta[:n]), ptr(meta[n:]), int(rec_ptr[a]), Ntot, ptr(arrays["atoms"]), ptr(arrays["nlist"]),
                        ptr(arrays["edges"]), ptr(arrays["inv_degree"]), ptr(arrays["y"]), ptr(arrays["w"]), ptr(counters)),
                        "ng_store_from_batch")
                a = b
            bad, labelled = (int(v) for v in counters.cpu())      # the one read of the device
            if bad:
                raise ValueError(f"from_structures: {bad} neighbour-list slot(s) point outside their structure")
            ds = cls(arrays, rec_ptr, [0, len(items)], device=device)
            report["labelled"] = labelled
        if ensembles:                                 # same atoms and labels by construction: no comparison needed
            ds._set_groups(np.concatenate([[0], np.cumsum([len(s) for s in structs])]).astype(np.int64))
        ds.name_table = table
        ds.join_report = report
        return ds

    def standards(self):
        """``{element index: (symbol, avg, std)}`` of this view's labelled rows, in the shape of
        ``standards.load_standards()``: take it from the TRAIN view and hand it to ``build_GNNModel(peak_standards=)``.  The
        element of a row is its first non-zero atom column; a row counts when ``y[:, 2] > 0``.  ``avg = sum(y) / n``, ``std =
        sqrt(max(sum(y^2) / n - avg^2, 0))`` in float64: the POPULATION form (this package's convention; nmrdata's is not
        pinned).  An element with fewer than 2 labels gets ``(symbol, 0.0, 0.0)``.  ``ng_label_moments`` on the GPU (one
        read of 3 C doubles), NumPy on a CPU device."""
        from .standards import ELEMENTS
        ids = self.record_ids
        if self.device.type == "cuda":
            import ctypes as C_
            from . import _lib
            from ._lib import ptr
            ctx = _lib.get_context(self.device.index)
            ids_dev = torch.from_numpy(ids.astype(np.int32)).to(self.device)
            out = torch.empty(self.C, 3, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                st = C_.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
                ctx.check(ctx.lib.ng_label_moments(ctx.handle, st, self.R, self.Ntot, self.C, ptr(self.atoms), ptr(self.y),
                                                   ptr(self.rec_ptr), ptr(ids_dev), len(ids), ptr(out)), "ng_label_moments")
            mom = out.cpu().numpy()
        else:
            arrays, _ = self._host_arrays()
            mom = label_moments_host(arrays["atoms"], arrays["y"])
        res = {}
        for c in range(self.C):
            sym = ELEMENTS[c] if c < len(ELEMENTS) else 'X'
            n, s1, s2 = (float(v) for v in mom[c])
            if n < 2:
                res[c] = (sym, 0.0, 0.0)
            else:
                avg = s1 / n
                res[c] = (sym, avg, float(np.sqrt(max(s2 / n - avg * avg, 0.0))))
        return res

    def _host_arrays(self):
        """(arrays, rec_ptr) of this view's records in view order, on the host"""
        ids = self.record_ids
        sizes = self._sizes[ids]
        gp = np.concatenate([[0], np.cumsum(sizes)])
        rows = torch.from_numpy(np.repeat(self.rec_ptr_host[ids] - gp[:-1], sizes) + np.arange(gp[-1]))
        return {k: getattr(self, k).cpu()[rows].numpy() for k in _ARRAYS}, gp

    def save(self, path):
        """one ``.npz``: the six arrays, ``rec_ptr``, ``file_ptr`` and ``format_version``.  A view saves its own records,
        in its order, as one source.  A grouped store adds ``group_ptr`` (same format version: a reader that does not know
        the array sees an ungrouped store)."""
        whole = len(self.record_ids) == self.R and np.array_equal(self.record_ids, np.arange(self.R))
        arrays, rec_ptr = self._host_arrays()
        file_ptr = self.file_ptr if whole else np.asarray([0, len(self.record_ids)], np.int64)
        if self.grouped:
            arrays["group_ptr"] = self.group_ptr.astype(np.int64)
        with open(path, "wb") as f:
            np.savez(f, rec_ptr=rec_ptr.astype(np.int64), file_ptr=file_ptr, format_version=np.asarray(FORMAT_VERSION, np.int64),
                     **arrays)

    @classmethod
    def load(cls, paths, device=None):
        """the store of one file or of several, concatenated in the order given; ``file_ptr`` keeps the sources apart
        (``split`` takes its validation share from every source).  The arrays were validated when they were built; here
        only their shapes and the version are checked."""
        if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
            paths = [paths]
        parts, rec_ptrs, file_ptrs, base_r, base_n = [], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], 0, 0
        group_ptrs, grouped = [np.zeros(1, np.int64)], False
        for p in paths:
            with np.load(p) as z:
                if "format_version" not in z.files or int(z["format_version"]) != FORMAT_VERSION:
                    raise ValueError(f"{p}: not a ShiftDataset file of format version {FORMAT_VERSION}")
                arrs = {k: z[k] for k in _ARRAYS}
                rp, fp = z["rec_ptr"].astype(np.int64), z["file_ptr"].astype(np.int64)
                gq = z["group_ptr"].astype(np.int64) if "group_ptr" in z.files else None
            if gq is None:                            # a file without groups: every record a group of its own
                gq = np.arange(len(rp), dtype=np.int64)
            else:
                grouped = True
                if gq.ndim != 1 or len(gq) < 1 or gq[0] != 0 or gq[-1] != len(rp) - 1 or (np.diff(gq) < 1).any():
                    raise ValueError(f"{p}: inconsistent group_ptr")
            group_ptrs.append(gq[1:] + base_r)
            if parts and (arrs["atoms"].shape[1] != parts[0]["atoms"].shape[1]
                          or arrs["nlist"].shape[1] != parts[0]["nlist"].shape[1]):
                raise ValueError(f"{p}: C or K differ from those of {paths[0]}")
            if rp[0] != 0 or (np.diff(rp) < 1).any() or fp[0] != 0 or fp[-1] != len(rp) - 1 or (np.diff(fp) < 0).any():
                raise ValueError(f"{p}: inconsistent rec_ptr / file_ptr")
            parts.append(arrs)
            rec_ptrs.append(rp[1:] + base_n)
            file_ptrs.append(fp[1:] + base_r)
            base_r += len(rp) - 1
            base_n += int(rp[-1])
        if not parts:
            raise ValueError("load: no files")
        arrays = {k: np.concatenate([a[k] for a in parts]) for k in _ARRAYS}
        return cls(arrays, np.concatenate(rec_ptrs), np.concatenate(file_ptrs), device=device,
                   group_ptr=np.concatenate(group_ptrs) if grouped else None)

    def __len__(self):
        return len(self.record_ids)

    def record_sizes(self):
        """atoms of every record of the view (host)"""
        return self._sizes[self.record_ids]

    def _view(self, ids):
        return ShiftDataset(None, None, None, _ids=ids, _parent=self)

    def split(self, validation):
        """``(train, val)`` views: of every source's records (within this view, in its order) the first
        ``int(validation * count)`` go to validation, the rest to train (nmrgnn/library.py:60-70 takes the same share of
        every file).  No data is copied.  A grouped store splits by GROUPS: of every source's groups (a group belongs to the
        source of its first member) the first ``int(validation * groups)`` go to validation, whole."""
        validation = float(validation)
        if not 0.0 <= validation <= 1.0:
            raise ValueError(f"split: validation must lie in [0, 1], got {validation}")
        if self.grouped:
            gp = self.group_ptr
            gsrc = np.searchsorted(self.file_ptr, self.record_ids[gp[:-1]], side="right") - 1
            train, val = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
            for s in range(len(self.file_ptr) - 1):
                mine = np.flatnonzero(gsrc == s)
                k = int(validation * len(mine))
                val += [self.record_ids[gp[q]:gp[q + 1]] for q in mine[:k]]
                train += [self.record_ids[gp[q]:gp[q + 1]] for q in mine[k:]]
            return self._view(np.concatenate(train)), self._view(np.concatenate(val))
        src = np.searchsorted(self.file_ptr, self.record_ids, side="right") - 1
        train, val = [], []
        for s in range(len(self.file_ptr) - 1):
            mine = self.record_ids[src == s]
            k = int(validation * len(mine))
            val.append(mine[:k])
            train.append(mine[k:])
        return self._view(np.concatenate(train)), self._view(np.concatenate(val))

    # ------------------------------------------------------------------ batches
    def _collate(self, ids, want_y_true, ctx=None):
        """(GraphBatch, y, w, names, y_true or None) of the view's records ``ids``"""
        ids = np.asarray(ids, np.int64).reshape(-1)
        if len(ids) == 0:
            raise ValueError("batch: no record ids")
        if ids.min() < 0 or ids.max() >= len(self.record_ids):
            raise ValueError(f"batch: record ids must lie in [0, {len(self.record_ids)})")
        store_ids = self.record_ids[ids]
        sizes = self._sizes[store_ids]
        G = len(store_ids)
        gp = np.zeros(G + 1, np.int64)
        np.cumsum(sizes, out=gp[1:])
        N = int(gp[-1])
        if N >= _MAX_BATCH_ATOMS:
            raise ValueError(f"batch: {N} atoms in one batch")
        dev = self.device
        if dev.type != "cuda":
            rows = torch.from_numpy(np.repeat(self.rec_ptr_host[store_ids] - gp[:-1], sizes) + np.arange(N))
            off = torch.from_numpy(np.repeat(gp[:-1], sizes).astype(np.int32))
            yt = self.y[rows]
            gb = GraphBatch(self.atoms[rows], self.nlist[rows] + off[:, None], self.edges[rows], self.inv_degree[rows],
                            graph_ptr=gp, device=dev, validate=False)
            return gb, yt[:, 0].contiguous(), self.w[rows], yt[:, 1].to(torch.int32), (yt if want_y_true else None)
        import ctypes as C
        from . import _lib
        from ._lib import ptr
        lib_ctx = ctx or _lib.get_context(dev.index)
        # graph_ptr first, so that the batch's graph_ptr starts its allocation; the ids behind it: one copy
        meta = torch.from_numpy(np.concatenate([gp, store_ids]).astype(np.int32)).to(dev)
        gp_dev, ids_dev = meta[:G + 1], meta[G + 1:]
        atoms = torch.empty(N, self.C, dtype=torch.float32, device=dev)
        nlist = torch.empty(N, self.K, dtype=torch.int32, device=dev)
        edges = torch.empty(N, self.K, dtype=torch.float32, device=dev)
        inv = torch.empty(N, dtype=torch.float32, device=dev)
        y0 = torch.empty(N, dtype=torch.float32, device=dev)
        w = torch.empty(N, dtype=torch.float32, device=dev)
        names = torch.empty(N, dtype=torch.int32, device=dev)
        y_true = torch.empty(N, 3, dtype=torch.float32, device=dev) if want_y_true else None
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            lib_ctx.check(lib_ctx.lib.ng_collate_batch(
                lib_ctx.handle, st, self.R, self.Ntot, ptr(self.atoms), ptr(self.nlist), ptr(self.edges), ptr(self.inv_degree),
                ptr(self.y), ptr(self.w), ptr(self.rec_ptr), ptr(ids_dev), ptr(gp_dev), N, self.K, self.C, G, ptr(atoms),
                ptr(nlist), ptr(edges), ptr(inv), ptr(y0), ptr(w), ptr(names), ptr(y_true)), "ng_collate_batch")
        gb = GraphBatch(atoms, nlist, edges, inv, graph_ptr=gp, device=dev, validate=False, ctx=ctx, graph_ptr_dev=gp_dev)
        return gb, y0, w, names, y_true

    def batch(self, ids):
        """``(GraphBatch, y[N], w[N], names[N] int32)`` of the records ``ids`` (any order, repeats allowed): the arrays of
        ``concat_graphs`` over these records in this order, padded slots offset like the rest; ``y`` is the shift column,
        ``names`` the int32 truncation of the name column (``metrics._split_y_true``).  No host synchronisation."""
        return self._collate(ids, False)[:4]

    def _epoch_order(self, shuffle, seed, epoch):
        n = len(self.group_ptr) - 1 if self.grouped else len(self.record_ids)
        if not shuffle:
            return np.arange(n, dtype=np.int64)
        return np.random.default_rng([int(seed), int(epoch)]).permutation(n).astype(np.int64)

    def epoch_ids(self, batch_graphs, shuffle=True, seed=0, epoch=0, drop_remainder=False):
        """the id lists of an epoch's batches (what ``batches`` collates).  On a grouped store the permutation runs over the
        GROUPS and ``batch_graphs`` counts groups: a list holds the records of whole groups, members in order."""
        batch_graphs = int(batch_graphs)
        if batch_graphs < 1:
            raise ValueError(f"batch_graphs must be >= 1, got {batch_graphs}")
        order = self._epoch_order(shuffle, seed, epoch)
        if self.grouped:
            if drop_remainder:
                order = order[:len(order) - len(order) % batch_graphs]
            return self._group_lists(order, batch_graphs)
        out = [order[i:i + batch_graphs] for i in range(0, len(order), batch_graphs)]
        if drop_remainder and out and len(out[-1]) < batch_graphs:
            out.pop()
        return out

    def batches(self, batch_graphs, shuffle=True, seed=0, epoch=0, drop_remainder=False):
        """Iterate over one epoch: ``(GraphBatch, y, w, names)`` per batch of ``batch_graphs`` records.  The order is
        ``np.random.default_rng([seed, epoch]).permutation(len(self))`` — a FULL permutation, where the reference shuffles
        through a 500-record buffer (nmrgnn/library.py:73); store order with ``shuffle=False``.  The last, shorter batch is
        kept unless ``drop_remainder``.  On the GPU batch t + 1 is collated on a side stream with its own library context
        while the caller's step t runs (``graph.BatchPrefetcher``); the bits are those of ``batch(ids)``.  A grouped store
        yields ``(GraphBatch, y, w, names, group_ptr)``: batches of ``batch_graphs`` groups and the batch's ``group_ptr``
        (int32 host array [Q + 1] over its graphs, what ``Trainer.step(groups=)`` takes)."""
        lists = self.epoch_ids(batch_graphs, shuffle, seed, epoch, drop_remainder)
        if self.grouped:
            gps = [self._batch_groups(ids) for ids in lists]
            return (out + (gp,) for out, gp in zip(_StorePrefetcher(self, lists), gps))
        return iter(_StorePrefetcher(self, lists))

    def eval_batches(self, batch_graphs):
        """``(GraphBatch, y_true[N, 3])`` in store order: what ``GNNModel.evaluate`` takes.  A grouped store yields
        ``(GraphBatch, y_true, group_ptr)``, batches of ``batch_graphs`` groups."""
        for ids in self.epoch_ids(batch_graphs, shuffle=False):
            out = self._collate(ids, True)
            if self.grouped:
                yield out[0], out[4], self._batch_groups(ids)
            else:
                yield out[0], out[4]
