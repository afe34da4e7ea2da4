"""nmrgnn_amd/callbacks.py on hand-written loss sequences: keras's plateau counting, early stopping, and the numbering of
the history files."""
import pytest


class _Trainer:
    def __init__(self, lr):
        self.lr = lr


class _Model:
    stop_training = False


def _run(cb, losses, lr, monitor="val_loss"):
    """the rate every epoch ran with, and the rate after the last one"""
    tr, model = _Trainer(lr), _Model()
    cb.on_train_begin(model, tr)
    ran = []
    for e, v in enumerate(losses):
        ran.append(tr.lr)
        cb.on_epoch_end(e, {monitor: v}, model, tr)
    return ran, tr.lr


def test_plateau_small_improvement_does_not_reset_the_wait():
    from nmrgnn_amd.callbacks import ReduceLROnPlateau
    # min_delta 0.1: 1.0 -> 0.95 is no improvement (needs < 0.9), so epochs 1 and 2 both count and the rate drops behind epoch 2
    ran, last = _run(ReduceLROnPlateau(factor=0.5, patience=2, min_lr=0.0, min_delta=0.1), [1.0, 0.95, 0.92, 0.92], 1.0)
    assert ran == [1.0, 1.0, 1.0, 0.5] and last == 0.5
    # a real improvement at epoch 1 resets the wait: epochs 2 and 3 count, the drop lands behind epoch 3
    ran, last = _run(ReduceLROnPlateau(factor=0.5, patience=2, min_lr=0.0, min_delta=0.1), [1.0, 0.85, 0.8, 0.8, 0.8], 1.0)
    assert ran == [1.0, 1.0, 1.0, 1.0, 0.5] and last == 0.5
    # the best value is not moved by the small step either: 0.95, then 0.88 (< 1.0 - 0.1) improves
    cb = ReduceLROnPlateau(factor=0.5, patience=3, min_lr=0.0, min_delta=0.1)
    _run(cb, [1.0, 0.95, 0.88], 1.0)
    assert cb.best == 0.88 and cb.wait == 0


def test_plateau_reduces_on_the_patience_th_epoch_and_repeats():
    from nmrgnn_amd.callbacks import ReduceLROnPlateau
    cb = ReduceLROnPlateau(factor=0.1, patience=3, min_lr=0.0)
    ran, last = _run(cb, [2.0] * 8, 1.0)
    # epoch 0 improves on infinity; epochs 1-3 do not: reduced behind epoch 3, then again behind epoch 6
    assert ran == pytest.approx([1.0, 1.0, 1.0, 1.0, 0.1, 0.1, 0.1, 0.01], rel=1e-12) and last == pytest.approx(0.01)
    ran, last = _run(ReduceLROnPlateau(factor=0.5, patience=1, min_lr=0.0), [3.0, 3.0, 3.0], 0.25)
    assert ran == [0.25, 0.25, 0.125] and last == 0.0625
    with pytest.raises(ValueError):
        ReduceLROnPlateau(factor=1.0)
    with pytest.raises(KeyError):
        _run(ReduceLROnPlateau(), [1.0], 1.0, monitor="loss")


def test_plateau_floor():
    from nmrgnn_amd.callbacks import ReduceLROnPlateau
    ran, last = _run(ReduceLROnPlateau(factor=0.5, patience=1, min_lr=0.3), [1.0] * 6, 1.0)
    assert ran == [1.0, 1.0, 0.5, 0.3, 0.3, 0.3] and last == 0.3
    # the reference's settings: rate 1e-4 with floor 1e-4 never moves, whatever the losses do
    ran, last = _run(ReduceLROnPlateau(monitor="val_loss", factor=0.99, patience=4, min_lr=1e-4), [1.0] * 20 + [2.0] * 20, 1e-4)
    assert set(ran) == {1e-4} and last == 1e-4
    # one fit after another starts counting afresh
    cb = ReduceLROnPlateau(factor=0.5, patience=2, min_lr=0.0)
    _run(cb, [1.0, 1.0], 1.0)
    assert cb.wait == 1
    ran, _ = _run(cb, [1.0, 1.0, 1.0], 1.0)
    assert ran == [1.0, 1.0, 1.0]


def test_early_stopping():
    from nmrgnn_amd.callbacks import EarlyStopping
    cb, model, tr = EarlyStopping(monitor="val_loss", patience=2), _Model(), _Trainer(1.0)
    cb.on_train_begin(model, tr)
    stopped = None
    for e, v in enumerate([1.0, 0.9, 0.95, 0.85, 0.86, 0.87, 0.5]):
        cb.on_epoch_end(e, {"val_loss": v}, model, tr)
        if model.stop_training:
            stopped = e
            break
    # best 0.85 at epoch 3; epochs 4 and 5 do not improve: the wait reaches 2 at epoch 5
    assert stopped == 5 and cb.stopped_epoch == 5 and cb.best == 0.85


def test_history_numbering(tmp_path):
    from nmrgnn_amd.callbacks import history_path
    name = str(tmp_path / "model")
    assert history_path(name) == name + "-history-0.pb"
    open(name + "-history-0.pb", "wb").close()
    open(name + "-history-1.pb", "wb").close()
    open(name + "-history-3.pb", "wb").close()
    assert history_path(name) == name + "-history-2.pb"
