"""Callbacks of ``GNNModel.fit``: the three the reference's training command uses or a user reaches for first
(nmrgnn/main.py:52-68).  Plain objects: ``fit`` calls ``on_train_begin(model, trainer)`` once where a callback has it,
and ``on_epoch_end(epoch, logs, model, trainer)`` after every epoch, with ``logs`` the epoch's history entries
(``loss``, the metric names, ``val_*``, ``lr``)."""
from __future__ import annotations

import os


class Callback:
    def on_train_begin(self, model, trainer):
        pass

    def on_epoch_end(self, epoch, logs, model, trainer):
        pass


def _monitored(logs, monitor, who):
    if monitor not in logs:
        raise KeyError(f"{who}: '{monitor}' is not among the epoch's results ({', '.join(sorted(logs))}); "
                       "val_* entries need validation_data")
    return float(logs[monitor])


class ReduceLROnPlateau(Callback):
    """keras's counting (mode 'min', no cooldown): an epoch improves only if the monitored value is below
    ``best - min_delta``; then the wait restarts at 0.  Otherwise the wait grows by one, and when it reaches ``patience``
    the trainer's rate becomes ``max(lr * factor, min_lr)`` (only if it is above ``min_lr``) and the wait restarts.
    The reference's settings (factor 0.99, patience 4, min_lr 1e-4) with its learning rate of 1e-4 never move the rate."""

    def __init__(self, monitor='val_loss', factor=0.1, patience=10, min_lr=0.0, min_delta=1e-4, verbose=0):
        if not factor < 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0")
        self.monitor, self.factor, self.patience = monitor, float(factor), int(patience)
        self.min_lr, self.min_delta, self.verbose = float(min_lr), float(min_delta), verbose
        self.on_train_begin(None, None)

    def on_train_begin(self, model, trainer):
        self.best = float("inf")
        self.wait = 0

    def on_epoch_end(self, epoch, logs, model, trainer):
        current = _monitored(logs, self.monitor, "ReduceLROnPlateau")
        if current < self.best - self.min_delta:
            self.best = current
            self.wait = 0
            return
        self.wait += 1
        if self.wait >= self.patience:
            old = float(trainer.lr)
            if old > self.min_lr:
                trainer.lr = max(old * self.factor, self.min_lr)
                if self.verbose:
                    print(f"Epoch {epoch + 1}: ReduceLROnPlateau reducing learning rate to {trainer.lr}.")
            self.wait = 0


class ModelCheckpoint(Callback):
    """``model.save(filepath)`` at the end of every epoch (weights, Adam state and the draw counter: what
    ``load_weights`` + ``fit(initial_epoch=...)`` resume from)"""

    def __init__(self, filepath):
        self.filepath = os.fspath(filepath)

    def on_epoch_end(self, epoch, logs, model, trainer):
        model.save(self.filepath)


class EarlyStopping(Callback):
    """stops ``fit`` after ``patience`` epochs in a row without the monitored value falling below ``best - min_delta``
    (keras's counting: the epoch at which the wait reaches ``patience`` is the last one; ``stopped_epoch`` holds it)"""

    def __init__(self, monitor='val_loss', patience=0, min_delta=0.0):
        self.monitor, self.patience, self.min_delta = monitor, int(patience), float(min_delta)
        self.on_train_begin(None, None)

    def on_train_begin(self, model, trainer):
        self.best = float("inf")
        self.wait = 0
        self.stopped_epoch = None

    def on_epoch_end(self, epoch, logs, model, trainer):
        current = _monitored(logs, self.monitor, "EarlyStopping")
        if current < self.best - self.min_delta:
            self.best = current
            self.wait = 0
            return
        self.wait += 1
        if self.wait >= self.patience:
            self.stopped_epoch = epoch
            model.stop_training = True


def history_path(name):
    """the first free ``<name>-history-<i>.pb``, i = 0, 1, ... (the reference's numbering, nmrgnn/main.py:84-88)"""
    i = 0
    while os.path.exists(f"{name}-history-{i}.pb"):
        i += 1
    return f"{name}-history-{i}.pb"
