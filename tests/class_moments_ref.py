"""Host references for the evaluation report (no GPU, no package code): a float64 statement of ``ng_class_moments`` and a
statement of the table that nmrgnn/main.py:93-189 (``eval-tfrecords``) writes, both written from their descriptions."""
import math

import numpy as np

SUMS = 7


def atom_terms(y, p):
    """the seven terms one counted atom adds: y and p go to float64 BEFORE any product"""
    yd, pd = float(np.float64(np.float32(y))), float(np.float64(np.float32(p)))
    d = yd - pd
    return (1.0, d * d, yd, pd, yd * yd, pd * pd, yd * pd)


def class_moments_ref(y, w, names, pred, class_of, K, start=None):
    """``(moments [K][7], abs_sums [K][7], counts [K])``: a loop over atoms and groupings, ``math.fsum`` per sum.
    ``class_of`` is [M][n_ids]; an atom counts when ``w > 0`` (false for 0, -0.0, negatives, NaN) and its id lies in
    [0, n_ids), with weight 1; a table value outside [0, K) is no class.  ``abs_sums`` are the sums of |term|, the scale of
    the rounding bound; ``start`` [K][7] is added at the end (``accumulate = 1``)."""
    class_of = np.asarray(class_of, np.int64).reshape(len(class_of), -1)
    M, n_ids = class_of.shape
    terms = [[[] for _ in range(SUMS)] for _ in range(K)]
    for i in range(len(y)):
        if not (float(w[i]) > 0):
            continue
        nm = int(names[i])
        if nm < 0 or nm >= n_ids:
            continue
        t = None
        for m in range(M):
            c = int(class_of[m, nm])
            if 0 <= c < K:
                t = atom_terms(y[i], pred[i]) if t is None else t
                for j in range(SUMS):
                    terms[c][j].append(t[j])
    moments = np.array([[math.fsum(terms[c][j]) for j in range(SUMS)] for c in range(K)], np.float64).reshape(K, SUMS)
    abs_sums = np.array([[math.fsum(map(abs, terms[c][j])) for j in range(SUMS)] for c in range(K)], np.float64).reshape(K, SUMS)
    counts = np.array([len(terms[c][0]) for c in range(K)], np.int64)
    if start is not None:
        moments = moments + np.asarray(start, np.float64)
    return moments, abs_sums, counts


def float_bound(abs_sums, counts):
    """|S - S_ref| <= n_c * 2^-52 * sum |term|: a float64 summation of n_c terms in any order (at most (n_c - 1) u sum |term|
    with u = 2^-53) plus the rounding of each term (one or two more u per term)"""
    return np.asarray(counts, np.float64)[:, None] * 2.0 ** -52 * np.asarray(abs_sums, np.float64)


def pearson_two_pass(x, y):
    """Pearson r from centred data; NaN below two points, 0 where one side is constant"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if len(x) < 2:
        return math.nan
    dx, dy = x - math.fsum(x) / len(x), y - math.fsum(y) / len(y)
    den = math.sqrt(math.fsum(dx * dx) * math.fsum(dy * dy))
    return math.fsum(dx * dy) / den if den != 0 else 0.0


def report_table_ref(keys, y, yhat, w, data_name):
    """The rows of the reference's table, in its order, as ``{row key: [N, value]}``.  ``keys``: the 'RES-NAME' key of every
    atom.  Atoms with ``w > 0`` are kept; the atom name is the part behind the first '-', the element its first character.
    Rows: ``{data_name}-{e}-r`` per element (sorted), ``{data_name}-{n}-r`` per atom name (sorted), then both again with
    ``-rmsd``, whose value is the MEAN SQUARED error (no root).  A key written twice keeps its first place and its last
    value, as a dict does."""
    keep = [i for i in range(len(keys)) if float(w[i]) > 0]
    name = [keys[i].split('-')[1] for i in keep]
    elem = [n[0] for n in name]
    ys = np.array([float(np.float32(y[i])) for i in keep], np.float64)
    ps = np.array([float(np.float32(yhat[i])) for i in keep], np.float64)
    out = {}
    for stat in ('r', 'rmsd'):
        for col in (elem, name):
            col = np.array(col, dtype=object)
            for v in sorted(set(col.tolist())):
                sel = np.nonzero(col == v)[0]
                a, b = ys[sel], ps[sel]
                val = pearson_two_pass(a, b) if stat == 'r' else math.fsum((b - a) ** 2) / len(sel)
                out[f'{data_name}-{v}-{stat}'] = [len(sel), val]
    return out
