"""Evaluation report over a record set (nmrgnn/main.py:93-189, ``eval-tfrecords``): count, Pearson r and squared error per atom
name, per residue and per element, from ONE device pass per batch (``ng_class_moments``) instead of every prediction copied to
the host and grouped in pandas.

``class_maps(name_table)`` turns the ``{'RES-NAME': id}`` table of a record set into the three groupings of main.py:130-135
(``name`` = ``key.split('-')[1]``, ``class`` = ``key.split('-')[0]``, ``element`` = the first character of ``name``), laid out in
one row space.  ``ClassMoments`` accumulates the seven float64 sums per row on the device (the sums of ``metrics.NameMetrics``:
count, sum (y - p)^2, sum y, sum p, sum y^2, sum p^2, sum y p; an atom counts when its weight is > 0, and then once).
``EvalReport`` forms the statistics on the host and writes the reference's CSV and markdown table.

Deviations from the reference, all deliberate:

* the rows keyed ``-rmsd`` hold the MEAN SQUARED ERROR by default, as the reference's do (main.py:165-171 takes no root), so that
  a table merges with one the reference wrote; ``square_root=True`` gives the root.  ``EvalReport.groups`` has both.
* r is ``metrics._corr`` on the float64 moments: NaN for fewer than two atoms, 0 where a variance is zero after rounding (pandas
  gives NaN there).
* a labelled atom whose key has no ``'-'`` (id 0, ``'X'``), or whose id the table lacks, is in no class: the reference stops
  with an IndexError on it; here ``EvalReport.unnamed`` counts such atoms, and their rows carry empty text columns.

There is no CPU path: the sums run on the GPU through libnmrgnn_hip.so."""
from __future__ import annotations

import csv
import math
import os
import re
from collections import namedtuple

import numpy as np

from .metrics import _MOMENTS, _corr

MAX_CLASSES = 1024            # ng_class_moments: rows of one call
MAX_NAME_ID = 1 << 24         # ng_class_moments: size of the class table
GROUPINGS = ('name', 'class', 'element')

ClassLabels = namedtuple('ClassLabels', 'text ranges')
ClassLabels.__doc__ = """``text[row]``: the label of every class row; ``ranges[grouping] = (first row, end row)``"""
ClassStats = namedtuple('ClassStats', 'count r mse rmsd bias')


def _split_key(key):
    """(name, class, element) of a 'RES-NAME' key as main.py:130-135 splits it; None for a key in no class"""
    parts = str(key).split('-')
    if len(parts) < 2 or parts[1] == '':
        return None
    return parts[1], parts[0], parts[1][0]


def class_maps(name_table):
    """``(class_of int32 [3][n_ids], ClassLabels)`` of a ``{'RES-NAME': id}`` table: row ``class_of[g][id]`` of name id ``id``
    under grouping ``GROUPINGS[g]``, -1 for an id in no class (a key without ``'-'`` such as ``'X'``, an id the table skips).
    Rows: the names in sorted order, then the residue classes, then the elements.  ``n_ids`` is the largest id + 1.  Where two
    keys share an id the later key of the table wins (the reference's ``rev_names``).  ``ValueError``: an id that is no integer
    in [0, 2^24), or more than 1024 classes in total."""
    by_id = {}
    for key, v in dict(name_table).items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"class_maps: the id of {key!r} is {v!r}, not an integer")
        if not 0 <= int(v) < MAX_NAME_ID:
            raise ValueError(f"class_maps: the id {int(v)} of {key!r} lies outside [0, 2^24)")
        by_id[int(v)] = _split_key(key)
    n_ids = max(by_id) + 1 if by_id else 0
    text, ranges = [], {}
    row_of = []
    for g, grouping in enumerate(GROUPINGS):
        values = sorted({s[g] for s in by_id.values() if s is not None})
        ranges[grouping] = (len(text), len(text) + len(values))
        row_of.append({v: ranges[grouping][0] + i for i, v in enumerate(values)})
        text.extend(values)
    if len(text) > MAX_CLASSES:
        raise ValueError(f"class_maps: {len(text)} classes in total ({', '.join(f'{ranges[g][1] - ranges[g][0]} {g}' for g in GROUPINGS)}"
                         f"), one report holds at most {MAX_CLASSES}")
    class_of = np.full((len(GROUPINGS), n_ids), -1, np.int32)
    for i, s in by_id.items():
        if s is not None:
            for g in range(len(GROUPINGS)):
                class_of[g, i] = row_of[g][s[g]]
    return class_of, ClassLabels(text, ranges)


class ClassMoments:
    """Device accumulator of ``[K][7]`` float64 moments over any number of ``update`` calls (``ng_class_moments`` with
    ``accumulate = 1`` on the current stream and the device's library context, as ``NameMetrics.update``).  ``class_of``: int32
    ``[M][n_ids]`` with 1 <= M <= 4 and rows in [-1, K).  ``update`` queues two launches and never waits; ``moments()`` is the
    one device read."""

    def __init__(self, class_of, K, device):
        import torch
        from . import _lib
        class_of = np.ascontiguousarray(class_of, dtype=np.int32)
        if class_of.ndim != 2 or not 1 <= class_of.shape[0] <= 4:
            raise ValueError(f"ClassMoments: class_of must be [M][n_ids] with 1 <= M <= 4, got shape {class_of.shape}")
        if not 1 <= int(K) <= MAX_CLASSES:
            raise ValueError(f"ClassMoments: K must lie in [1, {MAX_CLASSES}], got {K}")
        if class_of.shape[1] > MAX_NAME_ID:
            raise ValueError(f"ClassMoments: {class_of.shape[1]} name ids, at most 2^24")
        device = torch.device(device)
        if device.type != 'cuda':
            raise ValueError("ClassMoments runs on the GPU: pass a cuda device")
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        self.M, self.n_ids, self.K = int(class_of.shape[0]), int(class_of.shape[1]), int(K)
        self.ctx = _lib.get_context(device.index)
        self.class_of = torch.from_numpy(class_of).to(device)
        self.moments_dev = torch.zeros(self.K, _MOMENTS, dtype=torch.float64, device=device)
        self.updates = 0

    def update(self, peaks, y, w, names):
        """Queue one update: ``peaks``, ``y``, ``w`` float32 [N] and ``names`` int32 [N], contiguous, on the device."""
        import torch
        from . import _lib
        from ._lib import ptr
        N = peaks.numel() if isinstance(peaks, torch.Tensor) else -1
        for t, dt, what in ((peaks, torch.float32, 'peaks'), (y, torch.float32, 'y'), (w, torch.float32, 'w'),
                            (names, torch.int32, 'names')):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device:
                raise ValueError(f"ClassMoments.update: {what} must be a {dt} tensor on {self.device}")
            if t.numel() != N or not t.is_contiguous():
                raise ValueError(f"ClassMoments.update: {what} must be contiguous with {N} elements")
        st = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx.check(self.ctx.lib.ng_class_moments(self.ctx.handle, _lib._vp(st), N, ptr(y), ptr(w), ptr(names), ptr(peaks),
                                                     self.n_ids, self.M, ptr(self.class_of), self.K, 1, ptr(self.moments_dev)),
                       "ng_class_moments")
        self.updates += 1

    def reset(self):
        self.moments_dev.zero_()
        self.updates = 0

    def moments(self):
        """the ``[K][7]`` float64 sums as a NumPy array: ONE device-to-host copy"""
        return self.moments_dev.cpu().numpy()


def class_stats(s):
    """``ClassStats`` of one row of moments: count, r (``metrics._corr``; NaN below two atoms), mse, rmsd = sqrt(mse) and
    bias = mean(p - y); an empty class has count 0 and NaN everywhere else"""
    n = float(s[0])
    if n == 0:
        return ClassStats(0, math.nan, math.nan, math.nan, math.nan)
    mse = float(s[1]) / n
    return ClassStats(int(round(n)), _corr(s) if n >= 2 else math.nan, mse, math.sqrt(mse), (float(s[3]) - float(s[2])) / n)


def _fmt(v):
    """a table cell as pandas ``to_markdown`` prints it (tabulate's ``g`` format)"""
    if isinstance(v, str):
        return v
    if v is None:
        return 'nan'
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    return f"{float(v):g}"


_DASHES = re.compile(r':?-+:?$')


def read_markdown_table(path):
    """``(columns, rows)`` of a pipe table: first column the key, a header row, a dash row — what ``to_markdown`` below writes
    and what pandas ``DataFrame.to_markdown()`` writes.  ``columns``: the header cells behind the key column; ``rows``: a list
    of ``(key, [cell text per column])``.  ``ValueError`` naming the line for anything else."""
    def cells(line, no):
        parts = line.strip().split('|')
        if len(parts) < 4 or parts[0] != '' or parts[-1] != '':
            raise ValueError(f"{path}, line {no}: not a row of a pipe table with a key column: {line.rstrip()!r}")
        return [p.strip() for p in parts[1:-1]]

    with open(path) as f:
        lines = [(no, ln) for no, ln in enumerate(f.read().splitlines(), 1)]
    while lines and not lines[-1][1].strip():
        lines.pop()
    if len(lines) < 2:
        raise ValueError(f"{path}, line {len(lines) + 1}: a pipe table has a header row and a dash row")
    header = cells(lines[0][1], lines[0][0])
    dashes = cells(lines[1][1], lines[1][0])
    if len(dashes) != len(header) or not all(_DASHES.match(d) for d in dashes):
        raise ValueError(f"{path}, line {lines[1][0]}: the dash row of a pipe table expected, got {lines[1][1].rstrip()!r}")
    columns = header[1:]
    if len(set(columns)) != len(columns) or '' in columns:
        raise ValueError(f"{path}, line {lines[0][0]}: column names must be distinct and not empty, got {columns}")
    rows = []
    for no, ln in lines[2:]:
        c = cells(ln, no)
        if len(c) != len(header):
            raise ValueError(f"{path}, line {no}: {len(c)} cells, the header has {len(header)}")
        for v in c[1:]:
            try:
                float(v) if v else None
            except ValueError:
                raise ValueError(f"{path}, line {no}: {v!r} is not a number") from None
        rows.append((c[0], c[1:]))
    return columns, rows


class EvalReport:
    """Statistics per class of each grouping, from ``moments [K][7]`` and the ``ClassLabels`` of ``class_maps``.

    ``groups[grouping][label]`` is a ``ClassStats(count, r, mse, rmsd, bias)`` for every class of the table, empty ones
    included; ``labelled`` the number of atoms with a label, ``unnamed`` those of them in no class.  ``rows`` (``rows=True``):
    a dict of arrays over the labelled atoms in store order — ``record`` (index in the data evaluated), ``atom`` (index within
    the record), ``id`` (name id), ``y``, ``yhat`` — from which ``row_tuples()`` and ``to_csv`` take the text columns."""

    def __init__(self, moments, labels, class_of=None, data_name='', rows=None, labelled=None):
        self.moments = np.asarray(moments, np.float64).reshape(-1, _MOMENTS)
        self.labels = labels
        self.class_of = None if class_of is None else np.asarray(class_of, np.int32)
        self.data_name = data_name
        self.rows = rows
        if len(labels.text) != self.moments.shape[0]:
            raise ValueError(f"EvalReport: {self.moments.shape[0]} rows of moments for {len(labels.text)} labels")
        self.groups = {g: {labels.text[k]: class_stats(self.moments[k]) for k in range(*labels.ranges[g])} for g in labels.ranges}
        named = sum(s.count for s in self.groups['element'].values()) if 'element' in self.groups else 0
        self.labelled = named if labelled is None else int(labelled)
        self.unnamed = self.labelled - named

    # ------------------------------------------------------------------ the table
    def table(self, model_name, square_root=False):
        """``(columns, rows)``: ``columns = ['N', model_name]`` and ``rows`` a dict ``key -> [N, statistic]`` in the reference's
        order (main.py:155-171): ``{data_name}-{e}-r`` for every element with atoms, sorted, ``{data_name}-{n}-r`` for every
        atom name with atoms, sorted, then the same keys with ``-rmsd``.  As in the reference, a name that is also an element
        (``H``, ``N``, ``C``) shares the element's key: the row keeps the element's place and holds the NAME's numbers.

        The ``-rmsd`` rows hold the MEAN SQUARED ERROR, as the reference's do (``np.mean((yhat - y)**2)``, no root), so that the
        table merges with one the reference made; ``square_root=True`` writes the real RMSD under the same keys."""
        rows = {}
        for stat in ('r', 'rmsd'):
            for g in ('element', 'name'):
                for label in sorted(self.groups[g]):
                    s = self.groups[g][label]
                    if s.count:
                        rows[f'{self.data_name}-{label}-{stat}'] = [s.count, s.r if stat == 'r' else (s.rmsd if square_root else s.mse)]
        return ['N', model_name], rows

    def to_markdown(self, path, model_name, merge=None, square_root=False):
        """Write the table as a pipe table (the layout of pandas ``to_markdown``).  ``merge``: an existing pipe table (this
        method's or pandas's) whose rows are appended after this report's, as ``pd.concat([results, other])`` does: a column
        only one of the two has is filled with ``nan`` in the other's rows.  A ``merge`` path that does not exist is ignored, as
        in the reference; one that does not parse gives a ``ValueError`` naming the line."""
        columns, rows = self.table(model_name, square_root=square_root)
        body = [(k, [_fmt(v) for v in vals]) for k, vals in rows.items()]
        if merge is not None and os.path.exists(merge):
            ocols, orows = read_markdown_table(merge)
            allc = columns + [c for c in ocols if c not in columns]
            body = [(k, vals + ['nan'] * (len(allc) - len(columns))) for k, vals in body]
            for k, vals in orows:
                have = dict(zip(ocols, vals))
                body.append((k, [have.get(c) or 'nan' for c in allc]))
            columns = allc
        width = [max([len(k) for k, _ in body] + [1])] + [max([len(c)] + [len(v[j]) for _, v in body]) for j, c in enumerate(columns)]
        with open(path, 'w') as f:
            f.write('| ' + ' | '.join([' ' * width[0]] + [c.rjust(w) for c, w in zip(columns, width[1:])]) + ' |\n')
            f.write('|:' + '-' * (width[0] + 1) + '|' + '|'.join('-' * (w + 1) + ':' for w in width[1:]) + '|\n')
            for k, vals in body:
                f.write('| ' + ' | '.join([k.ljust(width[0])] + [v.rjust(w) for v, w in zip(vals, width[1:])]) + ' |\n')

    # ------------------------------------------------------------------ the atoms
    def _row_text(self, g):
        if self.rows is None:
            raise ValueError("this report was made with rows=False: it holds no atoms")
        ids = np.asarray(self.rows['id'], np.int64)
        text = np.array(self.labels.text + [''], dtype=object)
        n_ids = self.class_of.shape[1]
        inside = (ids >= 0) & (ids < n_ids)
        row = np.full(len(ids), -1, np.int64)
        row[inside] = self.class_of[g][ids[inside]]
        return text[row]          # -1 picks the trailing ''

    def row_tuples(self):
        """the labelled atoms in store order: ``(record, atom index, element, y, yhat, class, name)``"""
        name, cls, elem = (self._row_text(g) for g in range(3))
        r = self.rows
        return [(int(r['record'][i]), int(r['atom'][i]), elem[i], float(r['y'][i]), float(r['yhat'][i]), cls[i], name[i])
                for i in range(len(name))]

    def to_csv(self, path):
        """the reference's CSV (main.py:145-152): ``element,y,yhat,class,name``, one row per labelled atom"""
        with open(path, 'w', newline='') as f:
            wr = csv.writer(f)
            wr.writerow(['element', 'y', 'yhat', 'class', 'name'])
            wr.writerows((e, repr(y), repr(p), c, n) for _, _, e, y, p, c, n in self.row_tuples())
