"""Ensemble-averaged training end to end: the grouped ShiftDataset, Trainer.step(groups=), GNNModel.fit,
evaluate and evaluate_report on a store of 6 synthetic structures x 3 frames of 8-40 atoms (nmrgnn_amd/synth.py:
make_ensemble_records; K = 16, F = 64)."""
import functools

import numpy as np
import pytest

import class_moments_ref as CM
import group_loss_ref as R

pytestmark = pytest.mark.gpu

SIZES, FRAMES = (8, 40, 17, 33, 25, 12), 3
GROUP_PTR = np.arange(0, len(SIZES) * FRAMES + 1, FRAMES)
TABLE = {'X': 0, 'ALA-H': 1, 'ALA-HA': 2, 'ALA-N': 3, 'ALA-CA': 4, 'ALA-CB': 5, 'GLY-H': 6, 'GLY-N': 7, 'GLY-C': 8, 'DFT-H': 9,
         'MB-H': 10}


@functools.lru_cache(maxsize=None)
def _records():
    from nmrgnn_amd import synth
    rng = np.random.default_rng(808)
    recs = []
    for n in SIZES:
        recs += synth.make_ensemble_records(n, FRAMES, rng=rng, n_names=len(TABLE))
    return recs


@functools.lru_cache(maxsize=None)
def _plain(dev):
    from nmrgnn_amd.dataset import ShiftDataset
    return ShiftDataset.from_records(_records(), device=dev)


@functools.lru_cache(maxsize=None)
def _store(dev):
    return _plain(dev).with_groups(GROUP_PTR)


def _model(dev):
    from nmrgnn_amd.hypers import HyperParameters
    from nmrgnn_amd.model import build_GNNModel
    model = build_GNNModel(HyperParameters(atom_feature_size=64), embeddings={'name': TABLE}, device=dev)
    model.optimizer["learning_rate"] = 1e-3
    return model


def _state(eng):
    return eng.params.flat.detach().clone(), eng.adam_m.clone(), eng.adam_v.clone(), int(eng.adam_t)


def _same_state(a, b):
    import torch
    return a[3] == b[3] and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:3], b[:3]))


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------- the store
def test_from_structures_groups_the_frames(gpu_device):
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.structure import Structure
    rng = np.random.default_rng(5)
    structs, tables = [], []
    for n, frames in ((9, 3), (14, 2), (6, 1)):
        names = [f"{'HCNO'[i % 4]}{i}" for i in range(n)]
        structs.append(Structure(names, ["ALA"] * n, [i // 5 for i in range(n)], ["HCNO"[i % 4] for i in range(n)],
                                 [rng.uniform(0, 6, (n, 3)) for _ in range(frames)]))
        lab = np.arange(0, n, 2)
        tables.append({"resid": np.array([i // 5 for i in lab], np.int64), "name": np.array([names[i] for i in lab]),
                       "shift": rng.normal(8, 1, len(lab)).astype(np.float32), "resname": None})
    ds = ShiftDataset.from_structures(structs, tables, frames='all', ensembles=True, device=gpu_device)
    assert ds.grouped and ds.R == 6 and ds.group_ptr.tolist() == [0, 3, 5, 6] and ds.group_ptr.dtype == np.int64
    assert ds.group_sizes().tolist() == [3, 2, 1]
    assert ds._label_mismatch(ds.group_ptr) == -1                       # the frames of a structure do carry equal labels
    flat = ShiftDataset.from_structures(structs, tables, frames='all', device=gpu_device)
    assert not flat.grouped and flat.group_ptr.tolist() == list(range(7))
    assert flat.with_groups([0, 3, 5, 6]).group_ptr.tolist() == [0, 3, 5, 6]
    with pytest.raises(ValueError, match="frames='all'"):
        ShiftDataset.from_structures(structs, tables, frames='first', ensembles=True, device=gpu_device)


def test_with_groups_checks_sizes_and_labels(gpu_device):
    from nmrgnn_amd.dataset import ShiftDataset
    plain = _plain(gpu_device)
    g = _store(gpu_device)
    assert g.grouped and not plain.grouped and g.atoms is plain.atoms and g.group_ptr.tolist() == GROUP_PTR.tolist()
    with pytest.raises(ValueError, match="group 1: record 3 has 40 atoms"):
        plain.with_groups([0, 2, 18])
    with pytest.raises(ValueError, match="group_ptr"):
        plain.with_groups([0, 3, 6, 9, 12, 15, 17])
    with pytest.raises(ValueError, match="grouped already"):
        g.with_groups(GROUP_PTR)
    recs = list(_records())
    for what in ("y", "w", "atoms"):
        x, y, w = recs[7]
        x, y, w = list(x), y.copy(), w.copy()
        if what == "y":
            y[2, 0] += 1.0
        elif what == "w":
            w[0] = 0.25
        else:
            x[0] = np.roll(x[0], 1, axis=1)
        bad = recs[:7] + [(tuple(x), y, w)] + recs[8:]
        with pytest.raises(ValueError, match="group 2: its members differ"):
            ShiftDataset.from_records(bad, device=gpu_device).with_groups(GROUP_PTR)
    with pytest.raises(ValueError, match="whole groups"):                 # a view that breaks a group
        g._view(np.array([0, 1, 3, 4, 5]))
    with pytest.raises(ValueError, match="whole groups"):
        g._batch_groups([3, 4])


def test_save_load_round_trip(gpu_device, tmp_path):
    from nmrgnn_amd.dataset import FORMAT_VERSION, ShiftDataset
    g, plain = _store(gpu_device), _plain(gpu_device)
    a, b = str(tmp_path / "g.npz"), str(tmp_path / "p.npz")
    g.save(a)
    plain.save(b)
    with np.load(a) as z, np.load(b) as zp:
        assert "group_ptr" in z.files and "group_ptr" not in zp.files and int(z["format_version"]) == FORMAT_VERSION == 1
    back = ShiftDataset.load(a, device=gpu_device)
    assert back.grouped and back.group_ptr.tolist() == GROUP_PTR.tolist()
    assert not ShiftDataset.load(b, device=gpu_device).grouped
    both = ShiftDataset.load([b, a], device=gpu_device)                  # an ungrouped file in front: singletons, then offsets
    assert both.grouped and both.group_ptr.tolist() == list(range(18)) + (GROUP_PTR + 18).tolist()
    val = g.split(0.34)[1]
    val.save(a)                                                           # a view saves its own groups
    assert ShiftDataset.load(a, device=gpu_device).group_ptr.tolist() == [0, 3, 6]


def test_split_and_epochs_go_by_groups(gpu_device):
    g = _store(gpu_device)
    train, val = g.split(0.34)
    assert val.record_ids.tolist() == list(range(6)) and train.record_ids.tolist() == list(range(6, 18))
    assert val.group_ptr.tolist() == [0, 3, 6] and train.group_ptr.tolist() == [0, 3, 6, 9, 12] and train.grouped
    lists = train.epoch_ids(3, shuffle=True, seed=2, epoch=1)
    order = np.random.default_rng([2, 1]).permutation(4)
    assert [l.tolist() for l in lists] == [sum([[3 * q, 3 * q + 1, 3 * q + 2] for q in order[:3]], []),
                                           [3 * order[3], 3 * order[3] + 1, 3 * order[3] + 2]]
    assert len(train.epoch_ids(3, drop_remainder=True)) == 1
    got = list(train.batches(3, shuffle=True, seed=2, epoch=1))
    assert [len(o) for o in got] == [5, 5]
    assert got[0][4].dtype == np.int32 and got[0][4].tolist() == [0, 3, 6, 9] and got[1][4].tolist() == [0, 3]
    assert got[0][0].G == 9 and got[1][0].G == 3
    rb, ry, rw, rn = train.batch(lists[0])
    import torch
    assert torch.equal(_bits(got[0][0].atoms), _bits(rb.atoms)) and torch.equal(_bits(got[0][1]), _bits(ry))
    ev = list(val.eval_batches(1))
    assert [len(o) for o in ev] == [3, 3] and ev[0][2].tolist() == [0, 3] and ev[0][0].G == 3


def test_ungrouped_store_is_as_before(gpu_device):
    import torch
    plain = _plain(gpu_device)
    lists = plain.epoch_ids(4, shuffle=True, seed=3, epoch=1)
    assert [l.tolist() for l in lists] == [np.random.default_rng([3, 1]).permutation(18)[i:i + 4].tolist() for i in range(0, 18, 4)]
    got = list(plain.batches(4, shuffle=True, seed=3, epoch=1))
    assert len(got) == 5
    for ids, out in zip(lists, got):
        assert len(out) == 4
        rb, ry, rw, rn = plain.batch(ids)
        for k in ("atoms", "nlist", "edges", "inv_degree", "graph_ptr"):
            assert torch.equal(_bits(getattr(out[0], k)), _bits(getattr(rb, k))), k
        assert torch.equal(_bits(out[1]), _bits(ry)) and torch.equal(_bits(out[2]), _bits(rw)) and torch.equal(out[3], rn)
    assert all(len(o) == 2 for o in plain.eval_batches(4))
    train, val = plain.split(0.34)
    assert len(val) == 6 and len(train) == 12 and not train.grouped


# ------------------------------------------------------------------------------------------------- training
def test_fit_follows_the_hand_loop(gpu_device):
    import torch
    from nmrgnn_amd.train import Trainer
    train, val = _store(gpu_device).split(0.34)
    model = _model(gpu_device)
    hist = model.fit(train, epochs=2, validation_data=val, batch_graphs=3, seed=5, verbose=0)
    hand = _model(gpu_device)
    hand.build(10)
    tr = Trainer(hand.engine, lr=hand.optimizer["learning_rate"], loss_balance=hand.loss.s, metrics=hand.metrics)
    losses = []
    for epoch in range(2):
        total, steps = torch.zeros((), dtype=torch.float64, device=gpu_device), 0
        for batch, y, w, names, gp in train.batches(3, shuffle=True, seed=5, epoch=epoch):
            total += tr.step(batch, y, w, names=names, groups=gp).reshape(()).to(torch.float64)
            steps += 1
        losses.append(float(total.item()) / steps)
    assert steps == 2 and hand.engine.adam_t == 4
    assert _same_state(_state(model.engine), _state(hand.engine))
    assert hist.history['loss'] == losses and losses[0] != losses[1]
    tm = tr.metric_results()
    for k, v in tm.items():
        assert hist.history[k][-1] == v or (np.isnan(v) and np.isnan(hist.history[k][-1])), k
    ev = hand.evaluate(val.eval_batches(3))
    assert hist.history['val_loss'][-1] == ev['loss']
    tr.close()


def test_step_is_its_pieces_and_repeats(gpu_device):
    import torch
    from nmrgnn_amd.train import Trainer
    train, _ = _store(gpu_device).split(0.34)
    batch, y, w, names, gp = next(iter(train.batches(3, shuffle=False)))
    seed = 1234567
    states, first = [], None
    for run in range(2):
        model = _model(gpu_device)
        model.build(10)
        tr = Trainer(model.engine, lr=1e-3, loss_balance=0.5)
        loss = tr.step(batch, y, w, seed=seed, groups=gp)
        states.append((_state(model.engine), loss.clone()))
        tr.close()
    assert _same_state(states[0][0], states[1][0]) and torch.equal(_bits(states[0][1]), _bits(states[1][1]))
    model = _model(gpu_device)
    model.build(10)
    eng = model.engine
    tr = Trainer(eng, lr=1e-3, loss_balance=0.5)              # attached for its weight-image contract only; the pieces by hand
    peaks = eng.forward(batch, training=True, seed=seed)
    loss, dpred, means, _ = eng.loss_groups(batch, y, w, peaks, gp, s=0.5)
    eng.backward(dpred)
    eng.adam_step(lr=1e-3)
    assert _same_state(_state(eng), states[0][0]) and torch.equal(_bits(loss), _bits(states[0][1]))
    tr.close()
    with pytest.raises(ValueError, match="member_weights go with groups"):
        tr.step(batch, y, w, member_weights=np.ones(batch.G, np.float32))


def test_replay_refuses_groups(gpu_device):
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.train import Trainer
    model = _model(gpu_device)
    model.build(10)
    tr = Trainer(model.engine, lr=1e-3)
    rec = _records()[0]
    with pytest.raises(ValueError, match="ensemble groups"):
        TrainStepReplay(tr, rec[0], rec[1][:, 0], rec[2], groups=[0, 1])
    tr.close()


def test_straddling_members_are_pulled_together_not_apart(gpu_device):
    """The point of the feature.  Two frames of one structure whose predictions lie on either side of the label: the
    ensemble loss pulls both members the same way, by the sign of (mean - y); the per-frame loss pulls them in opposite
    directions.  Asserted on dpred."""
    import torch
    g = _store(gpu_device)
    gb, y, w, names = g.batch([3, 4])                          # two frames of the 40-atom structure
    model = _model(gpu_device)
    model.build(10)
    eng = model.engine
    peaks = eng.forward(gb, training=True, seed=99).reshape(-1)
    p0, p1 = peaks[:40], peaks[40:]
    assert bool((p0 != p1).all())
    y_one = 0.5 * (p0 + p1) + 0.25 * (p1 - p0)                 # between the two, nearer to p1: the mean lies on p0's side
    y2 = torch.cat([y_one, y_one]).contiguous()
    w2 = torch.ones_like(y2)
    loss, dpred, means, _ = eng.loss_groups(gb, y2, w2, peaks, [0, 2])
    d0, d1 = dpred[:40], dpred[40:]
    assert torch.equal(_bits(d0), _bits(d1))
    assert bool((torch.sign(d0) == torch.sign(means - y_one)).all()) and bool((d0 != 0).all())
    _, plain = eng.loss_l2(gb, y2, w2, peaks)
    assert bool((torch.sign(plain[:40]) == -torch.sign(plain[40:])).all()) and bool((plain != 0).all())
    assert bool((torch.sign(plain[:40]) == torch.sign(p0 - y_one)).all())


# ------------------------------------------------------------------------------------------------- evaluation
def _val_reference(dev, model, val, bg):
    """per batch of the grouped view: the peaks of a plain inference forward, the batch's labels and partitions (host)"""
    out = []
    for gb, y_true, gp in val.eval_batches(bg):
        peaks = model.engine.forward(gb, training=False).reshape(-1).cpu().numpy()
        out.append((gb.graph_ptr_host.copy(), np.asarray(gp), peaks, y_true.cpu().numpy()))
    return out


def test_evaluate_on_the_means(gpu_device):
    """loss: the float64 ensemble loss (s = 1) of every batch, weighted by its groups; tolerance of tests/test_gpu_metrics.py:
    test_evaluate (rel 1e-6).  The metrics agree with the report's element groups as in tests/test_gpu_eval_report.py."""
    _, val = _store(gpu_device).split(0.34)
    model = _model(gpu_device)
    model.build(10)
    got = model.evaluate(val.eval_batches(1))
    ref = _val_reference(gpu_device, model, val, 1)
    losses = [R.ensemble_loss_f64(gp, qp, p, yt[:, 0], yt[:, 2], s=1.0)[0] for gp, qp, p, yt in ref]
    print("evaluate loss", got['loss'], "float64", float(np.mean(losses)), "rel", abs(got['loss'] / float(np.mean(losses)) - 1))
    assert got['loss'] == pytest.approx(float(np.mean(losses)), rel=1e-6)
    # both groups in one batch: still the mean over groups (the forward of another batch shape moves the last digits of the
    # shifts, tests/test_gpu_eval_report.py: rtol 1e-4)
    two = model.evaluate(val.eval_batches(2))
    assert two['loss'] == pytest.approx(got['loss'], rel=1e-3)
    rep = model.evaluate_report(val, TABLE, batch_graphs=1, rows=False)
    for element, key in (('H', 'h_rmsd'), ('N', 'n_rmsd'), ('C', 'c_rmsd')):
        assert rep.groups['element'][element].count > 0
        assert rep.groups['element'][element].rmsd == pytest.approx(got[key], rel=1e-6), key
    # the ungrouped records of the same view: another number (every frame judged on its own)
    flat = model.evaluate(_plain(gpu_device).split(0.34)[1].eval_batches(3))
    assert flat['loss'] != got['loss']


def test_report_takes_one_row_per_atom_of_a_structure(gpu_device):
    """ng_class_moments is fed the group means (float32, the bits of group_loss_ref.group_mean_f32 on the peaks of a plain
    inference forward) and the groups' labels: float64 moments within class_moments_ref.float_bound, as
    tests/test_gpu_eval_report.py"""
    from nmrgnn_amd.report import class_maps
    _, val = _store(gpu_device).split(0.34)
    model = _model(gpu_device)
    model.build(10)
    rep = model.evaluate_report(val, TABLE, batch_graphs=1)
    ref = _val_reference(gpu_device, model, val, 1)
    means, ys, ws, ns = [], [], [], []
    for gp, qp, p, yt in ref:
        m, yo, wo, no = R.group_mean_f32(gp, qp, p, yt[:, 0], yt[:, 2], names=yt[:, 1].astype(np.int32))
        means.append(m); ys.append(yo); ws.append(wo); ns.append(no)
    means, ys, ws, ns = (np.concatenate(v) for v in (means, ys, ws, ns))
    assert len(means) == 8 + 40                                # one row per atom of a structure, not per frame
    class_of, labels = class_maps(TABLE)
    want, abs_sums, counts = CM.class_moments_ref(ys, ws, ns, means, class_of, len(labels.text))
    assert (rep.moments[:, 0] == counts).all() and (np.abs(rep.moments - want) <= CM.float_bound(abs_sums, counts)).all()
    on = ws > 0
    assert rep.labelled == int(on.sum())
    np.testing.assert_array_equal(rep.rows['yhat'], means[on])
    np.testing.assert_array_equal(rep.rows['y'], ys[on])
    np.testing.assert_array_equal(rep.rows['record'], np.repeat([0, 3], [8, 40])[on])      # the group's first record
    np.testing.assert_array_equal(rep.rows['atom'], np.concatenate([np.arange(8), np.arange(40)])[on])
