"""GNNModel.fit over a ShiftDataset (nmrgnn_amd/model.py, dataset.py, callbacks.py, main.py: train) against a hand loop of
Trainer.step over GraphBatches built by graph.concat_graphs from the same records in the same order: the parameters and Adam
moments bit for bit after every epoch, the history, the prefetching iterator, checkpoint and resume, and the command line.

F = 64, 24 synthetic records of 8-40 atoms, validation 0.25 (6 records), 3 epochs, 4 records or 1 record per step; noise
and dropout are left on."""
import functools
import json
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_REC, VALIDATION, EPOCHS = 24, 0.25, 3


@functools.lru_cache(maxsize=None)
def _records():
    from nmrgnn_amd import synth
    rng = np.random.default_rng(2024)
    recs = []
    for n in rng.integers(8, 41, size=N_REC):
        atoms, nl, d = synth.make_graph(int(n), 16, 10, 0.1, rng)
        mask = (rng.random(int(n)) < 0.8).astype(np.float32)
        mask[0] = 1.0
        y = np.stack([rng.standard_normal(int(n)), rng.integers(0, 8, size=int(n)), mask], axis=1).astype(np.float32)
        w = (mask * rng.choice([1.0, 0.5], size=int(n))).astype(np.float32)
        recs.append(((atoms, nl.astype(np.int32), d, synth.inv_degree(nl)), y, w))
    return recs


def _model(dev, lr=None, metrics=True):
    from nmrgnn_amd.hypers import HyperParameters
    from nmrgnn_amd.metrics import NameCorr, NameCount, NameRMSD
    from nmrgnn_amd.model import build_GNNModel
    model = build_GNNModel(HyperParameters(atom_feature_size=64), device=dev)
    if metrics:
        model.metrics = [NameRMSD([0, 1, 2, 3], name='lo_rmsd'), NameCorr([0, 1, 2, 3, 4, 5, 6, 7], name='all_r'),
                         NameCount([4, 5], name='mid_count')]
    if lr is not None:
        model.optimizer["learning_rate"] = lr
    return model


def _state(model):
    eng = model.engine
    return eng.params.flat.detach().clone(), eng.adam_m.clone(), eng.adam_v.clone(), int(eng.adam_t)


def _same_state(a, b):
    import torch
    return a[3] == b[3] and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:3], b[:3]))


class _Snap:
    def __init__(self):
        self.states, self.logs = [], []

    def on_epoch_end(self, epoch, logs, model, trainer):
        self.states.append(_state(model))
        self.logs.append(dict(logs))


def _hand_batch(recs, ids, dev):
    import torch
    from nmrgnn_amd.graph import concat_graphs
    gb = concat_graphs([recs[i][0] for i in ids], device=dev)
    y_true = torch.from_numpy(np.concatenate([recs[i][1] for i in ids])).to(dev)
    w = torch.from_numpy(np.concatenate([recs[i][2] for i in ids])).to(dev)
    return gb, y_true, w


def _hand_loop(dev, bg, shuffle, seed, epochs, lr=None):
    """the same training with the parent's own pieces: per epoch (state, loss, training metrics, evaluate() results)"""
    import torch
    from nmrgnn_amd.train import Trainer
    recs = _records()
    n_val = int(VALIDATION * N_REC)
    val_ids, train_ids = list(range(n_val)), list(range(n_val, N_REC))
    model = _model(dev, lr)
    model.build(10)
    tr = Trainer(model.engine, lr=model.optimizer["learning_rate"], loss_balance=model.loss.s, metrics=model.metrics)
    out = []
    for epoch in range(epochs):
        order = np.random.default_rng([seed, epoch]).permutation(len(train_ids)) if shuffle else np.arange(len(train_ids))
        total, steps = torch.zeros((), dtype=torch.float64, device=dev), 0
        for c in range(0, len(order), bg):
            ids = [train_ids[j] for j in order[c:c + bg]]
            gb, y_true, w = _hand_batch(recs, ids, dev)
            loss = tr.step(gb, y_true[:, 0].contiguous(), w, names=y_true[:, 1].to(torch.int32))
            total += loss.reshape(()).to(torch.float64)
            steps += 1
        val = model.evaluate([_hand_batch(recs, val_ids[c:c + bg], dev)[:2] for c in range(0, n_val, bg)])
        out.append((_state(model), float(total.item()) / steps, tr.metric_results(), val))
    tr.close()
    return out


@functools.lru_cache(maxsize=None)
def _datasets(dev):
    from nmrgnn_amd.dataset import ShiftDataset
    return ShiftDataset.from_records(_records(), device=dev).split(VALIDATION)


@pytest.mark.parametrize("bg", [4, 1])
@pytest.mark.parametrize("shuffle", [False, True])
def test_fit_follows_the_hand_loop(gpu_device, bg, shuffle):
    train, val = _datasets(gpu_device)
    assert len(train) == 18 and len(val) == 6
    model, snap = _model(gpu_device), _Snap()
    hist = model.fit(train, epochs=EPOCHS, validation_data=val, batch_graphs=bg, callbacks=[snap], shuffle=shuffle, seed=5,
                     verbose=0)
    want = _hand_loop(gpu_device, bg, shuffle, 5, EPOCHS)
    h = hist.history
    assert set(h) == {'loss', 'lo_rmsd', 'all_r', 'mid_count', 'val_loss', 'val_lo_rmsd', 'val_all_r', 'val_mid_count', 'lr'}
    assert all(len(v) == EPOCHS and all(isinstance(x, float) for x in v) for v in h.values()) and hist.epoch == [0, 1, 2]
    for e, (state, loss, tm, ev) in enumerate(want):
        assert _same_state(snap.states[e], state), f"parameters / Adam moments differ after epoch {e}"
        assert state[3] == (e + 1) * -(-18 // bg)
        assert h['loss'][e] == loss                                   # the same float64 sum of the same step losses
        for k, v in tm.items():
            assert h[k][e] == v or (np.isnan(v) and np.isnan(h[k][e])), k
        assert h['val_loss'][e] == ev['loss']
        for k, v in ev.items():
            if k != 'loss':
                assert h['val_' + k][e] == v or (np.isnan(v) and np.isnan(h['val_' + k][e])), k
        assert h['lr'][e] == model.optimizer["learning_rate"]
        assert set(snap.logs[e]) == set(h) and snap.logs[e]['loss'] == h['loss'][e]
    assert h['loss'][0] != h['loss'][1] and h['val_loss'][0] != h['val_loss'][2]          # it trains
    assert model.engine.cache_images is False                        # the trainer is closed: a later call packs as before


def test_plateau_callback_sets_the_rate(gpu_device):
    import torch
    from nmrgnn_amd.callbacks import EarlyStopping, ReduceLROnPlateau
    train, val = _datasets(gpu_device)
    # a learning rate of 0: the weights never move, the validation loss is flat, and a rate of 0 stays 0
    model = _model(gpu_device, lr=0.0, metrics=False)
    model.build(10)
    before = model.engine.params.flat.detach().clone()
    hist = model.fit(train, epochs=3, validation_data=val, batch_graphs=4, verbose=0,
                     callbacks=[ReduceLROnPlateau(monitor='val_loss', factor=0.5, patience=1, min_lr=0.0)])
    assert torch.equal(model.engine.params.flat, before)
    assert hist.history['lr'] == [0.0, 0.0, 0.0]
    v = hist.history['val_loss']
    assert v[0] == v[1] == v[2] and set(hist.history) == {'loss', 'val_loss', 'lr'}
    # a rate far below the weights' resolution: the loss is flat within min_delta, so with patience 1 the rate halves
    # behind epochs 1 and 2; 'lr' is the rate each epoch ran with
    r = 2.0 ** -100
    model = _model(gpu_device, lr=r, metrics=False)
    seen = []

    class Watch:
        def on_epoch_end(self, epoch, logs, model, trainer):
            seen.append(trainer.lr)
    hist = model.fit(train, epochs=3, validation_data=val, batch_graphs=4, verbose=0,
                     callbacks=[ReduceLROnPlateau(monitor='val_loss', factor=0.5, patience=1, min_lr=0.0), Watch()])
    v = hist.history['val_loss']
    assert max(v) - min(v) < 1e-4
    assert hist.history['lr'] == [r, r, r / 2] and seen == [r, r / 2, r / 4]
    # the floor holds, and early stopping ends the loop: flat loss, patience 2 -> epochs 0, 1, 2 run
    model = _model(gpu_device, lr=r, metrics=False)
    hist = model.fit(train, epochs=6, validation_data=val, batch_graphs=4, verbose=0,
                     callbacks=[ReduceLROnPlateau(monitor='val_loss', factor=0.5, patience=1, min_lr=r * 0.75),
                                EarlyStopping(monitor='val_loss', patience=2, min_delta=1e-4)])
    assert hist.history['lr'] == [r, r, r * 0.75] and hist.epoch == [0, 1, 2]
    with pytest.raises(KeyError):           # val_loss without validation data
        _model(gpu_device, lr=r, metrics=False).fit(train, epochs=1, batch_graphs=4, verbose=0, callbacks=[ReduceLROnPlateau()])
    with pytest.raises(TypeError):
        _model(gpu_device).fit(_records(), epochs=1)


def test_prefetched_batches_are_the_bits_of_batch(gpu_device):
    import torch
    train, _ = _datasets(gpu_device)
    id_lists = train.epoch_ids(4, shuffle=True, seed=3, epoch=1)
    busy = torch.randn(512, 512, device=gpu_device)
    got = []
    for out in train.batches(4, shuffle=True, seed=3, epoch=1):
        busy = busy @ busy * 1e-3              # work on the consumer's stream while the next batch is collated beside it
        got.append(out)
    assert len(got) == len(id_lists) == 5
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for ids, (gb, y, w, names) in zip(id_lists, got):
        rb, ry, rw, rn = train.batch(ids)
        assert gb._ctx is None and gb.G == rb.G and gb.N == rb.N and np.array_equal(gb.graph_ptr_host, rb.graph_ptr_host)
        for k in ("atoms", "nlist", "edges", "inv_degree", "nlist_c", "graph_ptr"):
            assert torch.equal(bits(getattr(gb, k)), bits(getattr(rb, k))), k
        n_in = int(rb.csc()[0][-1])
        assert torch.equal(gb.csc()[0], rb.csc()[0]) and torch.equal(gb.csc()[1][:n_in], rb.csc()[1][:n_in])
        lv, lr = gb.live_edges(), rb.live_edges()
        n_live = int(lr[3])
        assert int(lv[3]) == n_live and torch.equal(lv[0][:n_live], lr[0][:n_live]) and torch.equal(lv[1], lr[1])
        assert torch.equal(bits(lv[2][:n_live]), bits(lr[2][:n_live]))
        assert torch.equal(bits(y), bits(ry)) and torch.equal(bits(w), bits(rw)) and torch.equal(names, rn)


def test_checkpoint_and_resume(gpu_device, tmp_path):
    from nmrgnn_amd.callbacks import ModelCheckpoint
    train, val = _datasets(gpu_device)
    whole = _model(gpu_device)
    h2 = whole.fit(train, epochs=2, validation_data=val, batch_graphs=4, seed=9, verbose=0)
    ckpt = str(tmp_path / "ckpt")
    first = _model(gpu_device)
    h_a = first.fit(train, epochs=1, validation_data=val, batch_graphs=4, seed=9, verbose=0, callbacks=[ModelCheckpoint(ckpt)])
    assert os.path.exists(os.path.join(ckpt, "weights.npz"))
    resumed = _model(gpu_device)
    resumed.load_weights(ckpt)
    h_b = resumed.fit(train, epochs=1, validation_data=val, batch_graphs=4, seed=9, initial_epoch=1, verbose=0)
    assert h_b.epoch == [1]
    assert _same_state(_state(resumed), _state(whole))
    for k in h2.history:
        got = h_a.history[k] + h_b.history[k]
        assert got == h2.history[k] or any(np.isnan(x) for x in got), k


def test_train_command(gpu_device, tmp_path):
    from click.testing import CliRunner
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.library import load_model
    from nmrgnn_amd.main import main
    recs = _records()
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    ShiftDataset.from_records(recs[:12], device="cpu").save(a)
    ShiftDataset.from_records(recs[12:], device="cpu").save(b)
    emb = str(tmp_path / "emb.json")
    with open(emb, "w") as f:
        json.dump({"name": {"ALA-H": 1, "ALA-N": 2, "ALA-C": 3, "ALA-HA": 4, "DFT-H": 5, "MB-H": 6}}, f)
    name, ckpt = str(tmp_path / "model"), str(tmp_path / "ckpt")
    common = [a, b, name, "1", "--validation", "0.25", "--batch-graphs", "4", "--checkpoint-path", ckpt, "--device", str(gpu_device)]
    res = CliRunner().invoke(main, ["train"] + common + ["--embeddings", emb])
    assert res.exit_code == 0, res.output + repr(res.exception)
    m1 = load_model(name, device=gpu_device)
    p1 = m1.get_weights()
    assert m1.engine.adam_t == 5                    # 2 x 9 training records, 4 per step: 3 + 2 steps
    hist = pickle.load(open(name + "-history-0.pb", "rb"))
    metric_names = ['h_rmsd', 'n_rmsd', 'c_rmsd', 'hn_rmsd', 'ha_rmsd', 'h_r', 'n_r', 'c_r', 'hn_r', 'ha_r', 'avg_ha_count', 'mb_r',
                    'avg_mb_count', 'dft_r', 'avg_dft_count']
    assert set(hist) == {'loss', 'val_loss', 'lr'} | set(metric_names) | {'val_' + k for k in metric_names}
    assert all(len(v) == 1 for v in hist.values()) and hist['lr'] == [pytest.approx(1e-4)]
    assert os.path.exists(os.path.join(ckpt, "weights.npz"))
    # --load: starts from the checkpoint (5 optimiser steps in), so it ends somewhere else than a fresh run
    res = CliRunner().invoke(main, ["train"] + common + ["--load"])
    assert res.exit_code == 0, res.output + repr(res.exception)
    m2 = load_model(name, device=gpu_device)
    assert m2.engine.adam_t == 10
    p2 = m2.get_weights()
    assert any(not np.array_equal(p1[k], p2[k]) for k in p1)
    hist2 = pickle.load(open(name + "-history-1.pb", "rb"))
    assert set(hist2) == {'loss', 'val_loss', 'lr'}
    res = CliRunner().invoke(main, ["train", name, "1"])          # no record files
    assert res.exit_code != 0
