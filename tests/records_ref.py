"""NumPy statements of ``ng_store_from_batch``, ``ng_label_moments`` (csrc/records.hip) and of the label join of
``ShiftDataset.from_structures``.

``store_from_batch_ref(graph_ptr, b_atoms, b_nlist, b_edges, shift, name_id)`` returns the store rows of one ragged batch:
slot k of batch row i of structure g is live iff ``b_edges[i, k] > 0`` (false for -0.0 and NaN); a live slot keeps its edge
and gets the record-local index ``b_nlist[i, k] - graph_ptr[g]``, unless that index lies outside ``[0, n_g)``: then it is
counted in ``counters[0]`` and written as every other slot, ``(0, +0.0)``.  ``inv_degree`` is ``1 / #(local nlist > 0)`` (0 for
a count of 0), ``y = (finite shift or 0, float(name_id), mask)``, ``w = mask``, ``counters[1]`` the number of finite shifts."""
import numpy as np


def store_from_batch_ref(graph_ptr, b_atoms, b_nlist, b_edges, shift, name_id):
    gp = np.asarray(graph_ptr, np.int64)
    N, K = b_nlist.shape
    g = np.searchsorted(gp, np.arange(N), side="right") - 1
    off, n = gp[g], gp[g + 1] - gp[g]
    with np.errstate(invalid="ignore"):
        live = b_edges > 0
    loc = b_nlist.astype(np.int64) - off[:, None]
    inside = (loc >= 0) & (loc < n[:, None])
    keep = live & inside
    nlist = np.where(keep, loc, 0).astype(np.int32)
    edges = np.where(keep, b_edges, np.float32(0.0)).astype(np.float32)
    deg = (nlist > 0).sum(axis=1).astype(np.float32)
    inv = np.zeros(N, np.float32)
    np.divide(np.float32(1.0), deg, out=inv, where=deg > 0)
    has = np.isfinite(shift)
    mask = has.astype(np.float32)
    y = np.stack([np.where(has, shift, np.float32(0.0)).astype(np.float32), name_id.astype(np.float32), mask], axis=1)
    return dict(atoms=np.ascontiguousarray(b_atoms, np.float32), nlist=nlist, edges=edges, inv_degree=inv,
                y=np.ascontiguousarray(y, np.float32), w=mask, counters=np.asarray([(live & ~inside).sum(), has.sum()], np.int64))


def label_moments_ref(atoms, y, rec_ptr, ids):
    """float64 [C, 3] = (count, sum y0, sum y0^2) per element over the rows of the records ``ids`` (ids outside [0, R) are
    skipped, repeats count again) with ``y[:, 2] > 0``; the element is the first non-zero atom column, rows without one are
    skipped.  y0 is converted to float64 before it is squared."""
    C = atoms.shape[1]
    R = len(rec_ptr) - 1
    out = np.zeros((C, 3), np.float64)
    for i in ids:
        if not 0 <= i < R:
            continue
        a, b = int(rec_ptr[i]), int(rec_ptr[i + 1])
        nz = atoms[a:b] != 0
        use = (y[a:b, 2] > 0) & nz.any(axis=1)
        el = np.argmax(nz, axis=1)[use]
        y0 = y[a:b, 0][use].astype(np.float64)
        out[:, 0] += np.bincount(el, minlength=C)
        out[:, 1] += np.bincount(el, weights=y0, minlength=C)
        out[:, 2] += np.bincount(el, weights=y0 * y0, minlength=C)
    return out


def join_ref(resids, names, table_rows):
    """float32 [n], NaN where no label: ``table_rows`` = [(resid, name, shift)] laid on the atoms by (resid, name); every row
    must match exactly one atom"""
    out = np.full(len(names), np.nan, np.float32)
    for rid, nm, sh in table_rows:
        hit = [i for i in range(len(names)) if int(resids[i]) == int(rid) and str(names[i]).strip() == nm]
        assert len(hit) == 1, (rid, nm, hit)
        out[hit[0]] = sh
    return out


def synthetic_labels(structure, seed, share=0.4):
    """[(resid, name, shift)] for a random ``share`` of the atoms whose (resid, name) is unique in the structure; shifts are
    multiples of 1/64 so that their decimal text is exact"""
    rng = np.random.default_rng(seed)
    keys = [(int(r), str(n).strip()) for r, n in zip(structure.resids, structure.names)]
    count = {}
    for k in keys:
        count[k] = count.get(k, 0) + 1
    rows = []
    for i, k in enumerate(keys):
        if count[k] == 1 and rng.random() < share:
            rows.append((k[0], k[1], float(rng.integers(-64 * 20, 64 * 200)) / 64.0))
    return rows


def write_table(path, rows, structure=None):
    """the CSV ``read_shift_table`` reads; with ``structure`` a ``resname`` column as well"""
    res = {}
    if structure is not None:
        res = {(int(r), str(n).strip()): str(rn).strip() for r, n, rn in zip(structure.resids, structure.names, structure.resnames)}
    with open(path, "w") as f:
        f.write("resid,name,shift,resname\n" if structure is not None else "resid,name,shift\n")
        for rid, nm, sh in rows:
            f.write(f"{rid},{nm},{sh!r}" + (f",{res[(rid, nm)]}" if structure is not None else "") + "\n")
    return path
