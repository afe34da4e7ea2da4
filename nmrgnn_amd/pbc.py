"""Periodic boxes on the host: validation and conversion for the minimum-image builders (csrc/pbc.cuh).

A box is given per frame as ``(a, b, c, alpha, beta, gamma)`` in Angstrom and degrees — the form of a PDB ``CRYST1`` record
and of MDAnalysis ``u.dimensions`` — and converted to lower-triangular lattice vectors, a along x and b in the xy plane
(the GROMACS / MDAnalysis ``triclinic_vectors`` convention).  Accepted are orthorhombic boxes and reduced triclinic boxes,
``|b_x| <= a_x/2``, ``|c_x| <= a_x/2``, ``|c_y| <= b_y/2`` up to a small relative tolerance for the rounding of the angle
conversion (the GROMACS rhombic dodecahedron and truncated octahedron qualify; the octahedron sits on the ``c_y`` bound).
Everything else raises ``ValueError`` here, before any device work.

``triclinic_vectors_torch`` restates the conversion in float64 torch for the Jacobian of the box gradient
(``GraphBatch.box_grad``); the kernels keep reading what :func:`prepare` gives.
"""
from __future__ import annotations

import numpy as np

REDUCED_RTOL = 1e-5


def _cos_sin(deg):
    if deg == 90.0:                 # exact zero off-diagonals for right angles (an orthorhombic box stays orthorhombic)
        return 0.0, 1.0
    r = np.radians(deg)
    return float(np.cos(r)), float(np.sin(r))


def triclinic_vectors(dims):
    """``(a, b, c, alpha, beta, gamma)`` -> [3, 3] float64 lattice vectors (rows a, b, c), lower triangular"""
    d = np.asarray(dims, dtype=np.float64).reshape(-1)
    if d.shape[0] != 6:
        raise ValueError(f"box: (a, b, c, alpha, beta, gamma) expected, got {d.shape[0]} values")
    if not np.isfinite(d).all():
        raise ValueError(f"box: non-finite values {d.tolist()}")
    a, b, c, al, be, ga = (float(x) for x in d)
    if min(a, b, c) <= 0.0:
        raise ValueError(f"box: lengths must be > 0, got {a}, {b}, {c}")
    if not all(0.0 < x < 180.0 for x in (al, be, ga)):
        raise ValueError(f"box: angles must lie in (0, 180) degrees, got {al}, {be}, {ga}")
    ca, _ = _cos_sin(al)
    cb, _ = _cos_sin(be)
    cg, sg = _cos_sin(ga)
    cx = c * cb
    cy = c * (ca - cb * cg) / sg
    cz2 = c * c - cx * cx - cy * cy
    if not cz2 > 1e-12 * c * c:
        raise ValueError(f"box: angles {al}, {be}, {ga} give no cell")
    return np.array([[a, 0.0, 0.0], [b * cg, b * sg, 0.0], [cx, cy, np.sqrt(cz2)]])


def triclinic_vectors_torch(dims):
    """float64 torch restatement of :func:`triclinic_vectors`: ``[..., 6]`` -> ``[..., 3, 3]`` (rows a, b, c), differentiable
    everywhere, at 90 degrees too (cos(pi/2) is then ~6e-17 instead of the exact zero of ``_cos_sin``).  It serves the
    Jacobian d(vectors)/d(a, b, c, alpha, beta, gamma); the values the kernels see stay those of :func:`prepare`."""
    import torch
    d = dims.to(torch.float64)
    a, b, c = d[..., 0], d[..., 1], d[..., 2]
    al, be, ga = torch.deg2rad(d[..., 3]), torch.deg2rad(d[..., 4]), torch.deg2rad(d[..., 5])
    ca, cb, cg, sg = torch.cos(al), torch.cos(be), torch.cos(ga), torch.sin(ga)
    cx = c * cb
    cy = c * (ca - cb * cg) / sg
    cz = torch.sqrt(c * c - cx * cx - cy * cy)
    z = torch.zeros_like(a)
    return torch.stack([torch.stack([a, z, z], -1), torch.stack([b * cg, b * sg, z], -1), torch.stack([cx, cy, cz], -1)], -2)


def widths(vecs):
    """perpendicular widths of the box along a, b, c (distances between opposite faces)"""
    v = np.asarray(vecs, dtype=np.float64).reshape(3, 3)
    if v[1, 0] == v[2, 0] == v[2, 1] == 0.0:         # orthorhombic: the edge lengths, exactly
        return np.diag(v).copy()
    vol = abs(np.linalg.det(v))
    return np.array([vol / np.linalg.norm(np.cross(v[1], v[2])), vol / np.linalg.norm(np.cross(v[2], v[0])),
                     vol / np.linalg.norm(np.cross(v[0], v[1]))])


def check_reduced(vecs):
    """True for a reduced triclinic box, False for an orthorhombic one; ValueError for anything else"""
    v = np.asarray(vecs, dtype=np.float64).reshape(3, 3)
    bx, cx, cy = v[1, 0], v[2, 0], v[2, 1]
    tol = 1.0 + REDUCED_RTOL
    if abs(bx) > 0.5 * v[0, 0] * tol or abs(cx) > 0.5 * v[0, 0] * tol or abs(cy) > 0.5 * v[1, 1] * tol:
        raise ValueError("box: only orthorhombic and reduced triclinic boxes (|b_x| <= a_x/2, |c_x| <= a_x/2, "
                         f"|c_y| <= b_y/2) are supported, got vectors {v.tolist()}")
    return bool(bx != 0.0 or cx != 0.0 or cy != 0.0)


def prepare(box, G):
    """host side of a periodic build: ``box`` [6] (every frame) or [G, 6] -> (vectors [G, 9] float32, triclinic flag,
    smallest perpendicular width of every frame [G])"""
    d = np.asarray(box, dtype=np.float64)
    if d.ndim == 1:
        d = np.broadcast_to(d, (G, d.shape[0]))
    if d.ndim != 2 or d.shape != (G, 6):
        raise ValueError(f"box: [6] or [G, 6] = [{G}, 6] expected, got shape {tuple(np.shape(box))}")
    vecs = np.stack([triclinic_vectors(x) for x in d]) if G else np.zeros((0, 3, 3))
    tric = any([check_reduced(v) for v in vecs])
    w_min = np.array([widths(v).min() for v in vecs])
    return np.ascontiguousarray(vecs.reshape(G, 9), dtype=np.float32), tric, w_min


def prepare_ragged(boxes, G):
    """host side of a periodic build on a ragged batch, where every structure has a boundary kind of its own: ``boxes`` is a
    sequence of G entries, each ``None`` (open boundaries) or ``(a, b, c, alpha, beta, gamma)``, or a ``[G, 6]`` array (every
    structure periodic) -> (vectors [G, 9] float32, kinds [G] int32, smallest perpendicular width [G]).  Kinds: -1 open,
    0 orthorhombic, 1 reduced triclinic, decided per structure (:func:`prepare` decides once for a whole uniform batch).  An
    open structure has zero vectors and an infinite width.  A periodic entry's vectors are those :func:`prepare` gives for
    that box alone; the refusals are the same, with the structure index in front."""
    if hasattr(boxes, "detach"):                        # a torch tensor: its detached host copy
        boxes = boxes.detach().cpu().numpy()
    if isinstance(boxes, np.ndarray):
        if boxes.ndim != 2 or boxes.shape[1:] != (6,):
            raise ValueError(f"boxes: a sequence of G entries or a [G, 6] array expected, got shape {boxes.shape}")
    elif not isinstance(boxes, (list, tuple)):
        raise ValueError("boxes: a sequence of G entries (None or (a, b, c, alpha, beta, gamma)) or a [G, 6] array expected")
    if len(boxes) != G:
        raise ValueError(f"boxes: {len(boxes)} entries for {G} structures")
    vecs = np.zeros((G, 9), dtype=np.float32)
    kinds = np.full(G, -1, dtype=np.int32)
    w_min = np.full(G, np.inf)
    for g, entry in enumerate(boxes):
        if entry is None:
            continue
        if hasattr(entry, "detach"):
            entry = entry.detach().cpu().numpy()
        try:
            v = triclinic_vectors(entry)
            kinds[g] = 1 if check_reduced(v) else 0
            w_min[g] = widths(v).min()
        except ValueError as e:
            raise ValueError(f"structure {g}: {e}") from None
        vecs[g] = v.reshape(9)
    return vecs, kinds, w_min
