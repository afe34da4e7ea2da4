"""GNNModel.evaluate_report and the eval-records command (nmrgnn_amd/report.py, model.py, main.py) on a store of 6 synthetic
records of 8-40 atoms (K = 16 neighbours, F = 64): the device moments against tests/class_moments_ref.py applied to the
predictions of plain model(...) calls, the rows, the agreement with GNNModel.evaluate, and the files the command writes."""
import functools
import json
import math
import os

import numpy as np
import pytest

import class_moments_ref as R

pytestmark = pytest.mark.gpu

TABLE = {'X': 0, 'ALA-H': 1, 'ALA-HA': 2, 'ALA-N': 3, 'ALA-CA': 4, 'ALA-CB': 5, 'GLY-H': 6, 'GLY-N': 7, 'GLY-C': 8, 'DFT-H': 9,
         'MB-H': 10}
CENTRE = {'H': (8.0, 1.0), 'C': (60.0, 5.0), 'N': (120.0, 5.0)}


@functools.lru_cache(maxsize=None)
def _records():
    from nmrgnn_amd import synth
    rng = np.random.default_rng(77)
    keys = {v: k for k, v in TABLE.items()}
    recs = []
    for n in (8, 40, 17, 33, 25, 12):
        atoms, nl, d = synth.make_graph(n, 16, 10, 0.1, rng)
        ids = rng.integers(0, len(TABLE), size=n)
        mask = (rng.random(n) < 0.7).astype(np.float32)
        mask[0] = 1.0
        mu_sd = [CENTRE[keys[i].split('-')[1][0]] if i else (0.0, 1.0) for i in ids]
        shift = np.array([m + s * rng.standard_normal() for m, s in mu_sd])
        y = np.stack([shift, ids, mask], axis=1).astype(np.float32)
        recs.append(((atoms, nl.astype(np.int32), d, synth.inv_degree(nl)), y, mask.copy()))
    return recs


@functools.lru_cache(maxsize=None)
def _data(dev):
    from nmrgnn_amd.dataset import ShiftDataset
    return ShiftDataset.from_records(_records(), device=dev)


@functools.lru_cache(maxsize=None)
def _model(dev, seed=1234):
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    from nmrgnn_amd.metrics import reference_metrics
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    model = GNNModel(declare_gnn_space(HyperParameters(atom_feature_size=64)), load_standards(), device=dev, seed=seed)
    model.metrics = reference_metrics({'name': TABLE})
    model.build(10)
    return model


@functools.lru_cache(maxsize=None)
def _per_record_predictions(dev):
    """plain model(...) calls, one per record, on host inputs: the shifts of every atom in store order"""
    model = _model(dev)
    return np.concatenate([np.asarray(model(rec[0])).reshape(-1) for rec in _records()]).astype(np.float32)


def _reference(yhat_all):
    """(moments, bound) of the host reference over all atoms of the store, in store order"""
    from nmrgnn_amd.report import class_maps
    class_of, labels = class_maps(TABLE)
    y_true = np.concatenate([rec[1] for rec in _records()])
    want, abs_sums, counts = R.class_moments_ref(y_true[:, 0], y_true[:, 2], y_true[:, 1].astype(np.int32), yhat_all, class_of,
                                                 len(labels.text))
    return want, R.float_bound(abs_sums, counts), counts


@functools.lru_cache(maxsize=None)
def _report(dev, batch_graphs):
    return _model(dev).evaluate_report(_data(dev), TABLE, data_name='syn', batch_graphs=batch_graphs)


def test_moments_against_host_reference(gpu_device):
    rep = _report(gpu_device, 1)
    yhat = _per_record_predictions(gpu_device)
    want, bound, counts = _reference(yhat)
    err = np.abs(rep.moments - want)
    print("max err / bound:", float(np.max(err / np.maximum(bound, 1e-300))), "counts:", counts.tolist())
    assert (rep.moments[:, 0] == counts).all()
    assert (err <= bound).all()
    y_true = np.concatenate([rec[1] for rec in _records()])
    assert rep.labelled == int((y_true[:, 2] > 0).sum())
    assert rep.unnamed == int(((y_true[:, 2] > 0) & (y_true[:, 1] == 0)).sum()) > 0


def test_batching_changes_at_most_the_last_bits(gpu_device):
    """batch_graphs = 4: the class terms are added in another order (tiles hold several records), so the float bound, not the
    bits, is what holds; the reference takes the predictions of that very run"""
    rep = _report(gpu_device, 4)
    y_true = np.concatenate([rec[1] for rec in _records()])
    yhat = np.zeros(len(y_true), np.float32)
    yhat[y_true[:, 2] > 0] = rep.rows['yhat']
    want, bound, counts = _reference(yhat)
    assert (rep.moments[:, 0] == counts).all()
    assert (np.abs(rep.moments - want) <= bound).all()
    np.testing.assert_allclose(rep.rows['yhat'], _report(gpu_device, 1).rows['yhat'], rtol=1e-4, atol=1e-4)


def test_rows_are_the_labelled_atoms_in_store_order(gpu_device):
    yhat = _per_record_predictions(gpu_device)
    for bg in (1, 4):
        rep = _report(gpu_device, bg)
        record, atom, ids, y = [], [], [], []
        for r, rec in enumerate(_records()):
            on = np.nonzero(rec[1][:, 2] > 0)[0]
            record += [r] * len(on)
            atom += on.tolist()
            ids += rec[1][on, 1].astype(np.int32).tolist()
            y += rec[1][on, 0].tolist()
        np.testing.assert_array_equal(rep.rows['record'], record)
        np.testing.assert_array_equal(rep.rows['atom'], atom)
        np.testing.assert_array_equal(rep.rows['id'], ids)
        np.testing.assert_array_equal(rep.rows['y'], np.array(y, np.float32))
    rep = _report(gpu_device, 1)
    on = np.concatenate([rec[1][:, 2] for rec in _records()]) > 0
    np.testing.assert_array_equal(rep.rows['yhat'], yhat[on])               # the same forward on the same arrays
    keys = {v: k for k, v in TABLE.items()}
    tuples = rep.row_tuples()
    assert len(tuples) == int(on.sum())
    for (rec_i, atom_i, element, yv, pv, cls, name), i in zip(tuples, rep.rows['id']):
        want = ('', '', '') if i == 0 else (keys[i].split('-')[1][0], keys[i].split('-')[0], keys[i].split('-')[1])
        assert (element, cls, name) == want


def test_agrees_with_evaluate_and_leaves_it_alone(gpu_device):
    model, data = _model(gpu_device), _data(gpu_device)
    before = model.evaluate(data.eval_batches(4))
    rep = model.evaluate_report(data, TABLE, batch_graphs=4, rows=False)
    after = model.evaluate(data.eval_batches(4))
    assert list(before) == list(after)                                        # evaluate's own result is unchanged
    np.testing.assert_array_equal(list(before.values()), list(after.values()))
    assert rep.rows is None
    for element, key in (('H', 'h_rmsd'), ('N', 'n_rmsd'), ('C', 'c_rmsd')):
        assert rep.groups['element'][element].rmsd == pytest.approx(before[key], rel=1e-6), key
    np.testing.assert_array_equal(rep.moments, _report(gpu_device, 4).moments)    # rows or not, the same sums


def test_eval_records_writes_both_files_and_merges(gpu_device, tmp_path, monkeypatch):
    import csv
    from click.testing import CliRunner
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.main import eval_records, main
    from nmrgnn_amd.report import read_markdown_table
    recs = str(tmp_path / 'recs.npz')
    ShiftDataset.from_records(_records(), device='cpu').save(recs)
    emb = str(tmp_path / 'emb.json')
    with open(emb, 'w') as f:
        json.dump({'name': TABLE}, f)
    dirs = {}
    for name, model in (('model-a', _model(gpu_device)), ('model-b', _model(gpu_device, 99))):
        dirs[name] = str(tmp_path / name)
        model.save(dirs[name])
    rep = eval_records([recs], model_file=dirs['model-a'], embeddings=emb, data_name='syn', batch_graphs=4, device=gpu_device,
                       out_dir=str(tmp_path), echo=lambda *a: None)
    md_a, csv_a = str(tmp_path / 'model-a.md'), str(tmp_path / 'model-a.csv')
    columns, rows = read_markdown_table(md_a)
    _, want = rep.table('model-a')
    assert columns == ['N', 'model-a'] and [k for k, _ in rows] == list(want) and 'syn-H-rmsd' in want
    assert float(dict(rows)['syn-N-rmsd'][1]) == pytest.approx(rep.groups['name']['N'].mse, rel=1e-5)   # the mean SQUARED error
    with open(csv_a, newline='') as f:
        lines = list(csv.reader(f))
    assert lines[0] == ['element', 'y', 'yhat', 'class', 'name'] and len(lines) == 1 + rep.labelled
    assert [float(r[2]) for r in lines[1:]] == [float(v) for v in rep.rows['yhat']]
    np.testing.assert_array_equal(rep.moments, _report(gpu_device, 4).moments)     # the saved and reloaded model-a is the model
    # the second model through the command line, merged into the first table
    monkeypatch.chdir(tmp_path)
    res = CliRunner().invoke(main, ['eval-records', recs, '--model-file', dirs['model-b'], '--embeddings', emb, '--data-name',
                                    'syn', '--batch-graphs', '4', '--device', str(gpu_device), '--merge', md_a, '--sqrt'])
    assert res.exit_code == 0, res.output + repr(res.exception)
    assert os.path.exists(str(tmp_path / 'model-b.csv')) and not os.path.exists(str(tmp_path / 'model-b.md'))
    columns2, rows2 = read_markdown_table(md_a)
    assert columns2 == ['N', 'model-b', 'model-a'] and len(rows2) == 2 * len(rows)
    assert [k for k, _ in rows2] == 2 * [k for k, _ in rows]
    assert [c[2] for _, c in rows2[len(rows):]] == [c[1] for _, c in rows]           # model-a's block, as it was
    b = dict(rows2[:len(rows)])
    assert int(b['syn-N-rmsd'][0]) == want['syn-N-rmsd'][0] and not math.isnan(float(b['syn-N-rmsd'][1]))
    # --validation: only that share is evaluated; --no-csv writes no CSV
    os.remove(str(tmp_path / 'model-b.csv'))
    res = CliRunner().invoke(main, ['eval-records', recs, '--model-file', dirs['model-b'], '--embeddings', emb, '--validation',
                                    '0.5', '--device', str(gpu_device), '--no-csv'])
    assert res.exit_code == 0, res.output + repr(res.exception)
    assert not os.path.exists(str(tmp_path / 'model-b.csv'))
    _, rows3 = read_markdown_table(str(tmp_path / 'model-b.md'))
    n_atoms = sum(int(((rec[1][:, 2] > 0) & np.isin(rec[1][:, 1], [TABLE['ALA-N'], TABLE['GLY-N']])).sum()) for rec in _records()[:3])
    assert int(dict(rows3)['-N-r'][0]) == n_atoms > 0                         # the first three records only
    res = CliRunner().invoke(main, ['eval-records', '--embeddings', emb])          # no record files
    assert res.exit_code != 0
