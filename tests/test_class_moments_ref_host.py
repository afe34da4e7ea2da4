"""Host side of the evaluation report (nmrgnn_amd/report.py) against tests/class_moments_ref.py: the class maps, the table
and its order, the markdown round trip and merge, every ValueError, and r from float64 moments against the two-pass r.
No GPU: the moments here come from the host reference."""
import math

import numpy as np
import pytest

import class_moments_ref as R

TABLE = {'X': 0, 'ALA-H': 1, 'ALA-CA': 2, 'GLY-H': 3, 'GLY-CA': 4, 'GLY-HA2': 5, 'DFT-H': 6, 'ALA-N': 7, 'LYS-HZ1': 9,
         'GLY-C': 10}


def _atoms(rng, table=TABLE, n=400):
    """hand-made labelled atoms over every key of ``table`` but 'X': (keys, ids, y, yhat, w)"""
    keyed = [k for k in table if '-' in k]
    keys = [keyed[i % len(keyed)] for i in range(n)]
    ids = np.array([table[k] for k in keys], np.int32)
    centre = np.array([{'H': 8.0, 'C': 60.0, 'N': 120.0}[k.split('-')[1][0]] for k in keys])
    y = (centre + 3.0 * rng.standard_normal(n)).astype(np.float32)
    yhat = (y + 0.5 * rng.standard_normal(n) + 0.1).astype(np.float32)
    w = np.where(rng.random(n) < 0.25, 0.0, 1.0).astype(np.float32)
    return keys, ids, y, yhat, w


def _report(rng, data_name='d', **kw):
    from nmrgnn_amd.report import EvalReport, class_maps
    keys, ids, y, yhat, w = _atoms(rng, **kw)
    class_of, labels = class_maps(TABLE)
    moments, _, _ = R.class_moments_ref(y, w, ids, yhat, class_of, len(labels.text))
    return EvalReport(moments, labels, class_of=class_of, data_name=data_name), (keys, ids, y, yhat, w)


def test_class_maps_hand_written():
    from nmrgnn_amd.report import class_maps
    class_of, labels = class_maps(TABLE)
    assert class_of.dtype == np.int32 and class_of.shape == (3, 11)          # n_ids = largest id + 1
    names = ['C', 'CA', 'H', 'HA2', 'HZ1', 'N']
    classes = ['ALA', 'DFT', 'GLY', 'LYS']
    elements = ['C', 'H', 'N']
    assert labels.text == names + classes + elements
    assert labels.ranges == {'name': (0, 6), 'class': (6, 10), 'element': (10, 13)}
    want = {0: None, 8: None,                                                # 'X' has no '-'; id 8 is not in the table
            1: ('H', 'ALA', 'H'), 2: ('CA', 'ALA', 'C'), 3: ('H', 'GLY', 'H'), 4: ('CA', 'GLY', 'C'), 5: ('HA2', 'GLY', 'H'),
            6: ('H', 'DFT', 'H'), 7: ('N', 'ALA', 'N'), 9: ('HZ1', 'LYS', 'H'), 10: ('C', 'GLY', 'C')}
    for i, trio in want.items():
        got = class_of[:, i]
        if trio is None:
            assert (got == -1).all(), i
        else:
            assert [labels.text[r] for r in got] == list(trio), i
            for g, grouping in enumerate(('name', 'class', 'element')):
                assert labels.ranges[grouping][0] <= got[g] < labels.ranges[grouping][1]
    assert class_of[0, 1] == class_of[0, 3] == class_of[0, 6]                # two residues (and DFT) share the name H
    empty_of, empty = class_maps({'X': 0})
    assert empty_of.shape == (3, 1) and (empty_of == -1).all() and empty.text == []


def test_table_holds_to_the_reference():
    rep, (keys, ids, y, yhat, w) = _report(np.random.default_rng(0))
    for square_root in (False, True):
        columns, rows = rep.table('model-a', square_root=square_root)
        assert columns == ['N', 'model-a']
        want = R.report_table_ref(keys, y, yhat, w, 'd')
        assert list(rows) == list(want)                                      # the keys, in the reference's order
        assert list(rows)[:4] == ['d-C-r', 'd-H-r', 'd-N-r', 'd-CA-r']       # elements first; the names C, H, N share their keys
        for k in want:
            n, v = want[k]
            if square_root and k.endswith('-rmsd'):
                v = math.sqrt(v)
            assert rows[k][0] == n and isinstance(rows[k][0], int), k
            assert rows[k][1] == pytest.approx(v, rel=1e-12, abs=1e-9), k
    # the shared key holds the NAME's numbers: the name H (ALA, GLY, DFT) has fewer atoms than the element H (HA2, HZ1 too)
    assert rep.table('m')[1]['d-H-r'][0] == rep.groups['name']['H'].count < rep.groups['element']['H'].count
    s = rep.groups['element']['N']
    sel = [i for i, k in enumerate(keys) if k.endswith('-N') and w[i] > 0]
    assert s.count == len(sel)
    assert s.bias == pytest.approx(float(np.mean(yhat[sel].astype(np.float64) - y[sel].astype(np.float64))), abs=1e-12)
    assert s.rmsd == pytest.approx(math.sqrt(s.mse), rel=1e-15)
    assert rep.labelled == int((w > 0).sum()) and rep.unnamed == 0


def test_empty_and_single_atom_classes():
    from nmrgnn_amd.report import EvalReport, class_maps
    class_of, labels = class_maps(TABLE)
    y = np.array([8.0, 120.0, 121.0], np.float32)
    p = np.array([8.5, 119.0, 121.0], np.float32)
    ids = np.array([TABLE['LYS-HZ1'], TABLE['ALA-N'], TABLE['ALA-N']], np.int32)
    moments, _, _ = R.class_moments_ref(y, np.ones(3, np.float32), ids, p, class_of, len(labels.text))
    rep = EvalReport(moments, labels, class_of=class_of, labelled=4)
    one = rep.groups['name']['HZ1']
    assert one.count == 1 and math.isnan(one.r) and one.mse == 0.25 and one.bias == 0.5
    none = rep.groups['name']['CA']
    assert none.count == 0 and all(math.isnan(v) for v in none[1:])
    _, rows = rep.table('m')
    assert list(rows) == ['-H-r', '-N-r', '-HZ1-r', '-H-rmsd', '-N-rmsd', '-HZ1-rmsd']   # classes without atoms give no row
    assert rows['-N-rmsd'] == [2, 0.5]                                       # the MEAN SQUARED error under the -rmsd key
    assert rep.table('m', square_root=True)[1]['-N-rmsd'] == [2, math.sqrt(0.5)]
    assert rep.unnamed == 1                                                  # a labelled atom in no class


def test_markdown_round_trip_and_merge(tmp_path):
    from nmrgnn_amd.report import read_markdown_table
    rep, _ = _report(np.random.default_rng(1))
    path = str(tmp_path / 'a.md')
    rep.to_markdown(path, 'model-a')
    columns, rows = read_markdown_table(path)
    _, want = rep.table('model-a')
    assert columns == ['N', 'model-a'] and [k for k, _ in rows] == list(want)
    for k, cells in rows:
        assert int(cells[0]) == want[k][0] and float(cells[1]) == pytest.approx(want[k][1], rel=1e-5)
    # merge with itself: its own rows, then the file's
    rep.to_markdown(path, 'model-a', merge=path)
    columns2, rows2 = read_markdown_table(path)
    assert columns2 == columns and rows2 == rows + rows
    # another model's table: the columns of both, nan where a table lacks one (pd.concat)
    other = str(tmp_path / 'b.md')
    rep.to_markdown(other, 'model-b', merge=path, square_root=True)
    columns3, rows3 = read_markdown_table(other)
    assert columns3 == ['N', 'model-b', 'model-a'] and len(rows3) == 3 * len(rows)
    assert all(c[2] == 'nan' for _, c in rows3[:len(rows)]) and all(c[1] == 'nan' for _, c in rows3[len(rows):])
    # a merge path that does not exist yet is where the table goes, as in the reference
    fresh = str(tmp_path / 'c.md')
    rep.to_markdown(fresh, 'model-a', merge=fresh)
    assert read_markdown_table(fresh) == (columns, rows)


def test_pandas_tables_merge_and_own_file_parses_in_pandas(tmp_path):
    pd = pytest.importorskip('pandas')
    pytest.importorskip('tabulate')
    from nmrgnn_amd.report import read_markdown_table
    rep, _ = _report(np.random.default_rng(2))
    theirs = str(tmp_path / 'pandas.md')
    frame = pd.DataFrame({'d-H-r': [12, 0.75], 'd-H-rmsd': [12, 0.125]}, index=['N', 'ref-model']).transpose()
    with open(theirs, 'w') as f:
        f.write(frame.to_markdown())
        f.write('\n')
    columns, rows = read_markdown_table(theirs)
    assert columns == ['N', 'ref-model'] and [k for k, _ in rows] == ['d-H-r', 'd-H-rmsd']
    assert [float(v) for v in rows[1][1]] == [12.0, 0.125]
    rep.to_markdown(theirs, 'model-a', merge=theirs)
    columns, rows = read_markdown_table(theirs)
    assert columns == ['N', 'model-a', 'ref-model'] and [k for k, _ in rows[-2:]] == ['d-H-r', 'd-H-rmsd']
    # the package's own file through the reference's reader (main.py:181-184)
    mine = str(tmp_path / 'mine.md')
    rep.to_markdown(mine, 'model-a')
    other = pd.read_table(mine, sep="|", header=0, index_col=1, skipinitialspace=True).dropna(axis=1, how='all').iloc[1:]
    other.columns = other.columns.str.replace(' ', '')
    _, want = rep.table('model-a')
    assert list(other.columns) == ['N', 'model-a']
    assert [str(k).strip() for k in other.index] == list(want)
    got = other.astype(float).to_numpy()
    np.testing.assert_allclose(got[:, 0], [v[0] for v in want.values()])
    np.testing.assert_allclose(got[:, 1], [v[1] for v in want.values()], rtol=1e-5)


def test_every_value_error(tmp_path):
    from nmrgnn_amd.report import ClassMoments, EvalReport, class_maps, read_markdown_table
    many = {f'R{i}-A{i}': i + 1 for i in range(600)}                         # 600 names + 600 residues + 1 element
    with pytest.raises(ValueError, match='1201 classes'):
        class_maps(many)
    assert len(class_maps({f'R{i}-A{i}': i + 1 for i in range(511)})[1].text) == 1023      # 511 + 511 + 1 fit
    with pytest.raises(ValueError, match='16777216'):
        class_maps({'ALA-H': 1 << 24})
    with pytest.raises(ValueError, match='-1'):
        class_maps({'ALA-H': -1})
    with pytest.raises(ValueError, match='not an integer'):
        class_maps({'ALA-H': 1.5})
    class_of, labels = class_maps(TABLE)
    with pytest.raises(ValueError, match='rows of moments'):
        EvalReport(np.zeros((3, 7)), labels)
    rep = EvalReport(np.zeros((len(labels.text), 7)), labels, class_of=class_of)
    with pytest.raises(ValueError, match='rows=False'):
        rep.to_csv(str(tmp_path / 'x.csv'))
    with pytest.raises(ValueError, match='1 <= M <= 4'):
        ClassMoments(np.zeros((5, 3), np.int32), 4, 'cuda:0')
    with pytest.raises(ValueError, match='1 <= M <= 4'):
        ClassMoments(np.zeros(3, np.int32), 4, 'cuda:0')
    for K in (0, 1025):
        with pytest.raises(ValueError, match=r'\[1, 1024\]'):
            ClassMoments(np.zeros((1, 3), np.int32), K, 'cuda:0')
    with pytest.raises(ValueError, match='GPU'):
        ClassMoments(np.zeros((1, 3), np.int32), 4, 'cpu')
    good = ['|      |   N |   m |', '|:-----|----:|----:|', '| -H-r |   3 | 0.5 |']
    bad = {
        1: ['key      N     m'] + good[1:],                                   # a header without pipes
        2: [good[0], '| -H-r |   3 | 0.5 |', good[2]],                       # no dash row
        3: good[:2] + ['| -H-r |   3 |'],                                    # a short row
        4: good + ['| -N-r |   3 | abc |'],                                  # a cell that is no number
        5: good + ['| -N-r |   3 | 0.5 |', 'not a row'],
    }
    for line, text in bad.items():
        path = str(tmp_path / f'bad{line}.md')
        with open(path, 'w') as f:
            f.write('\n'.join(text) + '\n')
        with pytest.raises(ValueError, match=f'line {line}'):
            read_markdown_table(path)
        with pytest.raises(ValueError, match=f'line {line}'):
            rep.to_markdown(str(tmp_path / 'out.md'), 'm', merge=path)
    empty = str(tmp_path / 'empty.md')
    open(empty, 'w').close()
    with pytest.raises(ValueError, match='line 1'):
        read_markdown_table(empty)
    dup = str(tmp_path / 'dup.md')
    with open(dup, 'w') as f:
        f.write('|   | N | N |\n|:--|--:|--:|\n')
    with pytest.raises(ValueError, match='line 1'):
        read_markdown_table(dup)


def test_r_from_moments_against_two_pass():
    """A class near 120 ppm with a spread of 5: the moments form loses log10(120^2 / 25) ~ 3 digits to cancellation.  In
    NumPy float64 it stays within 1e-11 of the two-pass r, so the 1e-9 asked of the report has a margin of 100 that comes from
    the CPU alone."""
    from nmrgnn_amd.metrics import _corr
    rng = np.random.default_rng(3)
    worst_plain, worst_report = 0.0, 0.0
    for n in (300, 500):
        y = (120.0 + 5.0 * rng.standard_normal(n)).astype(np.float32)
        p = (y + 1.5 * rng.standard_normal(n)).astype(np.float32)
        want = R.pearson_two_pass(y, p)
        assert 0.9 < want < 0.99
        x, q = y.astype(np.float64), p.astype(np.float64)
        # the moments form, plain NumPy float64
        sx, sq, sxx, sqq, sxq = x.sum(), q.sum(), (x * x).sum(), (q * q).sum(), (x * q).sum()
        plain = (sxq - sx * sq / n) / math.sqrt((sxx - sx * sx / n) * (sqq - sq * sq / n))
        worst_plain = max(worst_plain, abs(plain - want))
        # the report's r on the moments of the host reference
        moments, _, _ = R.class_moments_ref(y, np.ones(n), np.zeros(n, np.int32), p, [[0]], 1)
        worst_report = max(worst_report, abs(_corr(moments[0]) - want))
    assert worst_plain <= 1e-11, worst_plain
    assert worst_report <= 1e-9, worst_report
