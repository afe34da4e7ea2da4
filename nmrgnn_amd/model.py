"""``GNNModel`` / ``build_GNNModel`` — the reference's model object (nmrgnn/model.py:12-105, 205-274)
on top of the HIP engine.  ``model((atoms, nlist, edges, inv_degree), training=False)`` returns one
chemical shift per atom, exactly like the Keras model's ``call``.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .engine import Engine
from .graph import GraphBatch
from .hypers import HyperParameters, declare_gnn_space
from .standards import load_standards

LOTS_OF_ELEMENTS = 100   # nmrgnn/model.py:222


class Peaks(np.ndarray):
    """numpy array that also answers ``.numpy()`` like the TF eager tensor the reference returns."""

    def numpy(self):
        return np.asarray(self)


class History:
    """what ``GNNModel.fit`` returns: ``history`` {name: one value per epoch} and ``epoch``, the epoch numbers"""

    def __init__(self):
        self.history = {}
        self.epoch = []


class GNNModel:
    def __init__(self, hypers, peak_standards, name='gnn-model', device=None, seed=1234, **kwargs):
        self.hypers = hypers
        self.name = name
        self.peak_standards = dict(peak_standards)
        # nmrgnn/model.py:220-228: large std/avg tables, cut to num_elem at build time
        self.peak_std = np.ones(LOTS_OF_ELEMENTS, dtype=np.float32)
        self.peak_avg = np.zeros(LOTS_OF_ELEMENTS, dtype=np.float32)
        for k, v in self.peak_standards.items():
            self.peak_std[k] = v[2]
            self.peak_avg[k] = v[1]
        self.embed_dim = hypers.get('atom_feature_size')
        self._device = device
        self._seed = seed
        self.engine = None
        self._pending_state = None
        self._train_calls = 0         # training-mode calls so far: every one draws fresh noise / dropout
        self._flat_leaf = None        # torch.nn.Parameter over the flat weight buffer, created by parameters()
        self.metrics = []             # Name* metrics (build_GNNModel with embeddings); reported by evaluate()

    # -- keras-like build: the number of elements comes from the first input (model.py:236-243)
    def build(self, num_elem):
        if self.engine is not None:
            if self.engine.C != num_elem:
                raise ValueError(f"model was built for {self.engine.C} elements, got {num_elem}")
            return
        self.engine = Engine(self.hypers, num_elem, self.peak_std[:num_elem], self.peak_avg[:num_elem],
                             device=self._device, seed=self._seed)
        if self._pending_state is not None:
            self.engine.params.load_state_dict(self._pending_state)
            self._pending_state = None
        self._restore_adam()

    def _restore_adam(self):
        pend = getattr(self, "_pending_adam", None)
        if pend is None or self.engine is None:
            return
        self._pending_adam = None
        if pend == "reset":            # a checkpoint without optimiser state: moments of OTHER weights must not survive
            self.engine.adam_m.zero_()
            self.engine.adam_v.zero_()
            self.engine.adam_t = 0
            return
        m, v, t = pend
        if m.shape[0] != self.engine.adam_m.shape[0]:
            raise ValueError(f"checkpoint Adam state has {m.shape[0]} entries, the model's flat parameter buffer "
                             f"{self.engine.adam_m.shape[0]}: it belongs to a different architecture")
        self.engine.adam_m.copy_(torch.from_numpy(m))
        self.engine.adam_v.copy_(torch.from_numpy(v))
        self.engine.adam_t = t

    def _as_batch(self, inputs):
        if isinstance(inputs, GraphBatch):
            return inputs, True
        atoms, nlist, edges, inv_degree = inputs
        on_device = all(isinstance(x, torch.Tensor) and x.is_cuda for x in (atoms, nlist, edges))
        num_elem = int(atoms.shape[-1])
        self.build(num_elem)
        return GraphBatch(atoms, nlist, edges, inv_degree, device=self.engine.device), on_device

    def __call__(self, inputs, training=False, seed=None):
        """``training=True`` applies GaussianNoise and Dropout with a FRESH draw per call, as Keras does
        (model.py:253,266-267): the Philox key is derived from the model seed and a per-model call counter;
        pass ``seed=`` to fix it."""
        batch, on_device = self._as_batch(inputs)
        if self.engine is None:
            self.build(batch.C)
        if training and seed is None:
            seed = self._train_seed()
        leaf = self._flat_leaf
        if torch.is_grad_enabled() and batch.edges.requires_grad:
            # gradients with respect to the inputs (a watched ``edges``, or positions through frames_to_batch): the edges
            # are an input of the autograd node too, whether or not the parameters require grad
            from .autograd import model_forward_inputs
            flat = leaf if leaf is not None else self.engine.params.flat
            return model_forward_inputs(self.engine, flat, batch, training=training, seed=seed or 0)
        if leaf is not None and leaf.requires_grad and torch.is_grad_enabled():
            # differentiable call (nmrgnn/main.py:74-80 trains by autodiff through model(x)): the result is a device
            # tensor with a grad_fn whatever the input container was — a numpy array could not carry one
            from .autograd import model_forward
            return model_forward(self.engine, leaf, batch, training=training, seed=seed or 0)
        peaks = self.engine.forward(batch, training=training, seed=seed or 0)
        if on_device:
            return peaks
        return peaks.cpu().numpy().view(Peaks)

    call = __call__
    predict = __call__

    @property
    def receptive_hops(self):
        """list steps a predicted shift can see: one per message-passing layer (the FC and head layers are per atom, the
        model has no global term) — the ``hops`` of ``GraphBatch.restrict`` that leave the selected shifts exact"""
        return int(self.hypers.get('mp_layers'))

    def predict_selected(self, inputs, select):
        """the [S] shifts of the ``select``-ed atoms (a mask [N] or an index array; ascending atom index), from an inference
        forward on their receptive field alone (``GraphBatch.restrict(select, receptive_hops)``): the
        values ``self(inputs)[select]`` holds, at the cost of the atoms and edges that can reach them.  ``inputs`` as
        ``__call__``; device inputs give a device tensor, host inputs NumPy."""
        batch, on_device = self._as_batch(inputs)
        if self.engine is None:
            self.build(batch.C)
        pruned = batch.restrict(select, self.receptive_hops)
        with torch.no_grad():
            peaks = self.engine.forward(pruned, training=False)[pruned.selected]
        if on_device:
            return peaks
        return peaks.cpu().numpy().view(Peaks)

    def _train_seed(self):
        """the Philox key of the next training-mode call (``__call__(training=True)`` without ``seed=``)"""
        seed = ((int(self._seed) * 0x9E3779B97F4A7C15) ^ (self._train_calls * 1000003 + 0x632BE5AB)) & ((1 << 63) - 1)
        self._train_calls += 1
        return seed

    def predict_uncertainty(self, inputs, samples=32, seed=None, chunk_atoms=1 << 20):
        """``(mean, std_model, std_input)``, each [N] in ppm: an error bar for every predicted shift from the model's own two
        random layers (nmrgnn/model.py:253,266-267), which the reference reaches only through ``model(x, training=True)``.

        ``std_model``: the Dropout in front of the output layer, in CLOSED FORM — Var = (1 - keep) / keep * sum_f (g_f u_f)^2
        per replica (``ng_head_fwd_var``), averaged over the replicas; no mask is drawn.  ``std_input``: the GaussianNoise on
        the distances, SAMPLED — the spread of the dropout-mean shift over ``samples`` noisy replicas of the input, which run
        as one batch (``GraphBatch.replicate``) in chunks of at most ``chunk_atoms`` atoms (always at least one replica per
        chunk).  ``mean`` is the mean over the replicas.  By the law of total variance the two parts add:
        ``total_std = sqrt(std_model**2 + std_input**2)``.

        A model with ``noise == 0`` runs one replica and returns ``std_input`` exactly 0; a model without dropout returns
        ``std_model`` exactly 0.  ``seed=None`` derives the seed as ``__call__(training=True)`` does (a fresh draw per call).
        The noise of all replicas is ONE draw, ``ng_randn(seed, offset 0)`` over [samples, edges] — what the unchunked call
        draws inside its launch; a chunk takes its slice of it, so the result does not depend on ``chunk_atoms`` beyond
        float32 rounding (a seed per chunk would make it depend on the chunking).  Device inputs give device tensors, host inputs NumPy, as ``__call__``."""
        samples = int(samples)
        if samples < 1:
            raise ValueError(f"predict_uncertainty: samples must be >= 1, got {samples}")
        if int(chunk_atoms) < 1:
            raise ValueError(f"predict_uncertainty: chunk_atoms must be >= 1, got {chunk_atoms}")
        batch, on_device = self._as_batch(inputs)
        if self.engine is None:
            self.build(batch.C)
        eng = self.engine
        if seed is None:
            seed = self._train_seed()
        S = samples if eng.sigma > 0 else 1
        N = batch.N
        per = max(1, min(S, int(chunk_atoms) // max(N, 1)))
        mu = torch.empty(S, N, dtype=torch.float32, device=eng.device)
        var = torch.empty(S, N, dtype=torch.float32, device=eng.device)
        ne = batch.n_edges
        for s0 in range(0, S, per):
            n = min(per, S - s0)
            noise = True            # one chunk: the draw inside the launch, as forward(training=True, seed=seed)
            if per < S and eng.sigma > 0:
                # the chunk's slice of that same draw: elements [s0 * ne, (s0 + n) * ne) of ng_randn(seed, offset 0)
                # (a Philox counter holds four elements; a slice that starts inside one is copied to an aligned buffer)
                lead = (s0 * ne) % 4
                noise = eng.randn(lead + n * ne, int(seed), (s0 * ne) // 4)
                if lead:
                    noise = noise[lead:].clone()
            m, v = eng.forward_moments(batch.replicate(n), seed=int(seed), noise=noise)
            mu[s0:s0 + n] = m.view(n, N)
            var[s0:s0 + n] = v.view(n, N)
        mean, var_in, var_model = eng.ensemble_moments(mu, var)
        out = (mean, torch.sqrt(var_model), torch.sqrt(var_in))
        if on_device:
            return out
        return tuple(t.cpu().numpy().view(Peaks) for t in out)

    def evaluate(self, data, metrics=None):
        """Validation pass (keras ``evaluate`` / the ``validation_data`` of nmrgnn/main.py:79-80).  ``data`` yields
        ``(inputs, y_true[N, 3])`` or ``(inputs, y_true, graph_ptr)``; ``inputs`` is the model's input tuple.
        Inference-mode forwards; the loss and the metric sums stay on the device until the end (no host read per batch).
        Returns ``{'loss': mean over ALL graphs of the per-graph L2 NameLoss, <metric name>: value}`` for ``metrics``
        (default ``self.metrics``).  The metrics are ACCUMULATED over the whole set (``NameMetrics(accumulate=True)``):
        the reference's metrics keep only the last batch (``assign``), which says nothing about a validation set.
        With one graph per batch the loss equals keras's mean over batches.

        Ensemble groups: an item ``(GraphBatch, y_true, group_ptr)`` — what a grouped store's
        ``eval_batches`` yields; a GraphBatch carries its own ``graph_ptr``, so the third element is the batch's ensemble
        ``group_ptr`` — is judged on the MEAN prediction of every group against the group's labels: the loss is the mean
        over all GROUPS, and the metrics take one row per atom of a group."""
        from .losses import NameLoss
        from .metrics import NameMetrics, _split_y_true
        metrics = getattr(self, 'metrics', []) if metrics is None else metrics
        nm = metrics if isinstance(metrics, NameMetrics) else (NameMetrics(metrics, accumulate=True) if metrics else None)
        if nm is not None:
            if not nm.accumulate:
                raise ValueError("evaluate: a NameMetrics passed in must accumulate")
            nm.reset_states()
        loss_fn = getattr(self, 'loss', None)
        label_idx = loss_fn.label_idx if isinstance(loss_fn, NameLoss) else None
        loss_sum, graphs = None, 0
        for item in data:
            inputs, y_true = item[0], item[1]
            graph_ptr = item[2] if len(item) > 2 else None
            groups = None
            if isinstance(inputs, GraphBatch):
                batch, groups = inputs, graph_ptr
            else:
                atoms, nlist, edges, inv_degree = inputs
                self.build(int(atoms.shape[-1]))
                batch = GraphBatch(atoms, nlist, edges, inv_degree, graph_ptr=graph_ptr, device=self.engine.device)
            if self.engine is None:
                self.build(batch.C)
            eng = self.engine
            peaks = eng.forward(batch, training=False)
            y, w, names = _split_y_true(y_true, eng.device)
            if y.shape[0] != batch.N:
                raise ValueError(f"evaluate: y_true has {y.shape[0]} rows for {batch.N} atoms")
            if groups is not None:      # the groups' means and labels stand for the batch from here on
                batch = eng.group_means(batch, y, w, peaks, groups, names=names)
                peaks, y, w, names = batch.means, batch.y, batch.w, batch.names
            lw = w
            if label_idx is not None:
                ln = torch.as_tensor(np.atleast_1d(np.asarray(label_idx, np.int32)), device=eng.device)
                lw = w * torch.isin(names, ln).to(torch.float32)
            loss, _ = eng.loss_l2(batch, y, lw, peaks)
            part = loss.to(torch.float64) * batch.G          # ng_loss_l2 is the mean over the batch's graphs
            loss_sum = part if loss_sum is None else loss_sum + part
            graphs += batch.G
            if nm is not None:
                nm.update(peaks, y, w, names)
        out = {'loss': float(loss_sum.item()) / graphs if graphs else 0.0}
        if nm is not None:
            out.update(nm.results())
        return out

    def evaluate_report(self, data, name_table, data_name='', batch_graphs=64, rows=True):
        """The table of nmrgnn/main.py:93-189 (``eval-tfrecords``) over ``data``, a ``dataset.ShiftDataset`` or a view of one:
        count, Pearson r, squared error and bias per atom name, per residue and per element of ``name_table`` (the
        ``{'RES-NAME': id}`` table the records' name ids come from: ``ShiftDataset.name_table`` or ``embeddings['name']``).
        Inference forwards over ``data.eval_batches(batch_graphs)``; after each, ONE ``ng_class_moments`` call adds the batch's
        sums to the device accumulator (``report.ClassMoments``), weighting by the mask column of ``y_true`` exactly as
        ``evaluate`` does.  The device is read once at the end; with ``rows=True`` the labelled atoms' predictions are read too
        and the ``report.EvalReport`` returned holds them in store order.  A class's terms are added in the order the batches lay
        the atoms out, so the last bits of the float64 moments depend on ``batch_graphs``.  On a grouped
        store the moments take the MEAN prediction of every ensemble group against the group's labels: one
        row per labelled atom of a structure, not one per frame, ``record`` being the group's first record."""
        from .dataset import ShiftDataset
        from .metrics import _split_y_true
        from .report import ClassMoments, EvalReport, class_maps
        if not isinstance(data, ShiftDataset):
            raise TypeError("evaluate_report: data is a dataset.ShiftDataset or a view of one")
        class_of, labels = class_maps(name_table)
        if len(labels.text) == 0:
            raise ValueError("evaluate_report: the name table has no 'RES-NAME' key, so there is no class to report")
        self.build(data.C)
        eng = self.engine
        if data.device != eng.device:
            raise ValueError(f"evaluate_report: the data lives on {data.device}, the model on {eng.device}")
        cm = ClassMoments(class_of, len(labels.text), eng.device)
        labelled = torch.zeros((), dtype=torch.float64, device=eng.device)
        kept, record0 = [], 0
        for item in (data.eval_batches(batch_graphs) if len(data) else ()):
            batch, y_true = item[0], item[1]
            peaks = eng.forward(batch, training=False).reshape(-1)
            y, w, names = _split_y_true(y_true, eng.device)
            first = None
            if data.grouped:            # one row per atom of a GROUP: its mean prediction against its labels
                first = record0 + np.asarray(item[2][:-1], np.int64)
                means = eng.group_means(batch, y, w, peaks, item[2], names=names)
                peaks, y, w, names = means.means, means.y, means.w, means.names
            cm.update(peaks, y, w, names)
            on = w > 0
            labelled += on.sum()
            if rows:
                gp = (batch if first is None else means).graph_ptr_host.astype(np.int64)
                # (the record of a row: its graph's, or the FIRST member's of its group)
                kept.append((record0 + np.arange(batch.G) if first is None else first, gp, on, y, names, peaks))
            record0 += batch.G
        out = torch.cat([cm.moments_dev.reshape(-1), labelled.reshape(1)]).cpu().numpy()     # the one read of the sums
        moments, n_labelled = out[:-1].reshape(-1, 7), int(out[-1])
        row_arrays = None
        if rows:
            if kept:
                on = torch.cat([k[2] for k in kept])
                vals = torch.stack([torch.cat([k[3] for k in kept])[on], torch.cat([k[5] for k in kept])[on]]).cpu().numpy()
                ids = torch.cat([k[4] for k in kept])[on].cpu().numpy()
                on = on.cpu().numpy()
                record = np.concatenate([np.repeat(rec, np.diff(gp)) for rec, gp, *_ in kept])[on]
                atom = np.concatenate([np.arange(gp[-1]) - np.repeat(gp[:-1], np.diff(gp)) for _, gp, *_ in kept])[on]
            else:
                vals, ids = np.zeros((2, 0), np.float32), np.zeros(0, np.int32)
                record = atom = np.zeros(0, np.int64)
            row_arrays = {'record': record, 'atom': atom, 'id': ids, 'y': vals[0], 'yhat': vals[1]}
        return EvalReport(moments, labels, class_of=class_of, data_name=data_name, rows=row_arrays, labelled=n_labelled)

    def fit(self, train, epochs=1, validation_data=None, batch_graphs=1, callbacks=(), shuffle=True, seed=0,
            initial_epoch=0, verbose=1, trainable=None, lr_scale=None, clipnorm=None):
        """Train on a ``dataset.ShiftDataset`` (keras ``model.fit`` as nmrgnn/main.py:79-80 calls it).  Runs ``epochs``
        epochs, numbered ``initial_epoch, initial_epoch + 1, ...`` (the number seeds the shuffle and is what callbacks see;
        unlike keras, ``epochs`` counts the epochs RUN, so ``fit(epochs=1, initial_epoch=1)`` after ``load_weights`` is the
        second epoch of ``fit(epochs=2)``).  Returns an object whose ``.history`` is a ``dict[str, list[float]]`` with the
        keys ``loss``, the metric names, ``val_loss`` / ``val_<metric>`` (with ``validation_data``) and ``lr``.

        ``batch_graphs=1`` is the reference's one record per step.  Larger values are this package's batched step and CHANGE
        THE OPTIMISATION: the loss is a mean over the batch's graphs, so G records make one step on their mean gradient
        instead of G steps.  Single process: a ``torch.distributed`` world larger than 1 is refused (``Trainer`` with
        ``parallel.GradBuckets`` is the data-parallel path).

        Per epoch: ``Trainer.step`` over ``train.batches(batch_graphs, shuffle, seed, epoch)`` (a full permutation keyed on
        ``[seed, epoch]``; batches collated on the device one ahead of the step).  The trainer is built once per ``fit`` from
        ``self.loss.s``, ``self.optimizer['learning_rate']`` and ``self.metrics`` and closed at the end; the step's weight
        column is the records' ``w``, times the membership of ``self.loss.label_idx`` where that is set (as ``evaluate``).
        ``loss`` is the mean of the step losses (summed on the device in float64, read once per epoch), as keras reports it;
        the training metrics are those of the epoch's LAST step (the reference's overwrite semantics,
        ``Trainer.metric_results``).  ``val_*`` come from ``self.evaluate(validation_data.eval_batches(...))``: metrics
        accumulated over the whole set, and ``val_loss`` the L2 loss whatever ``loss_balance`` is.  ``lr`` is the rate the
        epoch ran with (callbacks change it afterwards).  Noise and dropout draws are keyed on the optimiser step, which
        checkpoints carry, so a resumed run continues the sequence.

        Ensemble-averaged training: on a grouped ``train`` store (``from_structures(ensembles=True)``,
        ``with_groups``) ``batch_graphs`` counts GROUPS and every step is ``Trainer.step(groups=)`` — the loss of the mean
        prediction over a structure's frames; a grouped ``validation_data`` is judged on the means as well.

        Fine-tuning: ``trainable`` (patterns as ``trainable_names``), ``lr_scale`` ({pattern: scale}, first match wins) and
        ``clipnorm`` go to the ``Trainer``: only the selected tensors are updated, the others keep their bits, and the
        backward stops at the lowest stage a trainable tensor needs."""
        from .dataset import ShiftDataset
        from .losses import NameLoss
        from .train import Trainer
        if not isinstance(train, ShiftDataset) or not (validation_data is None or isinstance(validation_data, ShiftDataset)):
            raise TypeError("fit: train and validation_data are dataset.ShiftDataset objects (ShiftDataset.from_records)")
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise RuntimeError("fit is single process; in a torch.distributed world larger than 1 drive Trainer.step yourself")
        if len(train) == 0:
            raise ValueError("fit: the training set holds no record")
        epochs, batch_graphs, initial_epoch = int(epochs), int(batch_graphs), int(initial_epoch)
        self.build(train.C)
        eng = self.engine
        if train.device != eng.device:
            raise ValueError(f"fit: the data lives on {train.device}, the model on {eng.device}")
        loss_fn = getattr(self, 'loss', None)
        label_idx = loss_fn.label_idx if isinstance(loss_fn, NameLoss) else None
        ln = None if label_idx is None else torch.as_tensor(np.atleast_1d(np.asarray(label_idx, np.int32)), device=eng.device)
        opt = getattr(self, 'optimizer', None) or {}
        metrics = getattr(self, 'metrics', None) or None
        trainer = Trainer(eng, lr=float(opt.get('learning_rate', self.hypers.get('learning_rate'))),
                          loss_balance=float(getattr(loss_fn, 's', 1.0)), metrics=metrics,
                          trainable=None if trainable is None else self.trainable_names(trainable), lr_scale=lr_scale,
                          clipnorm=clipnorm)
        history = History()
        self.stop_training = False
        try:
            for cb in callbacks:
                if hasattr(cb, 'on_train_begin'):
                    cb.on_train_begin(self, trainer)
            for epoch in range(initial_epoch, initial_epoch + epochs):
                total = torch.zeros((), dtype=torch.float64, device=eng.device)
                steps = 0
                for batch, y, w, names, *groups in train.batches(batch_graphs, shuffle=shuffle, seed=seed, epoch=epoch):
                    lw = w if ln is None else w * torch.isin(names, ln).to(torch.float32)
                    # a grouped store yields the batch's ensemble group_ptr too: the step then fits the groups' means
                    loss = trainer.step(batch, y, lw, names=names if metrics else None, groups=groups[0] if groups else None)
                    total += loss.reshape(()).to(torch.float64)
                    steps += 1
                logs = {'loss': float(total.item()) / steps}
                if metrics:
                    logs.update(trainer.metric_results())
                if validation_data is not None and len(validation_data):
                    val = self.evaluate(validation_data.eval_batches(batch_graphs))
                    logs.update({f'val_{k}': v for k, v in val.items()})
                logs['lr'] = float(trainer.lr)
                for k, v in logs.items():
                    history.history.setdefault(k, []).append(float(v))
                history.epoch.append(epoch)
                if verbose:
                    print(f"Epoch {epoch + 1}: " + " - ".join(f"{k}: {v:.6g}" for k, v in logs.items()))
                for cb in callbacks:
                    cb.on_epoch_end(epoch, logs, self, trainer)
                if self.stop_training:
                    break
        finally:
            trainer.close()
        return history

    # -- torch.autograd surface (the outer autograd shell)
    def parameters(self):
        """The trainable state as ONE leaf tensor: the engine's flat fp32 parameter buffer, shared, not copied.
        After this call ``model(g)`` under ``torch.enable_grad()`` returns a tensor with a grad_fn, and
        ``loss.backward()`` accumulates into ``parameters()[0].grad`` (autograd.GNNModelFunction).
        ``torch.optim.Adam(model.parameters(), lr, eps=1e-7)`` is the reference's optimiser (model.py:44-45)."""
        self._need_engine()
        if self._flat_leaf is None:
            self._flat_leaf = torch.nn.Parameter(self.engine.params.flat, requires_grad=True)
        return [self._flat_leaf]

    def named_parameter_views(self):
        """{keras-style name: (weight view, gradient view or None)} into the flat leaf and its ``.grad``"""
        leaf = self.parameters()[0]
        P = self.engine.params
        out = {}
        for name, shape in P.shapes.items():
            o, n = P.offsets[name], int(np.prod(shape))
            g = None if leaf.grad is None else leaf.grad[o:o + n].view(*shape)
            out[name] = (leaf.data[o:o + n].view(*shape), g)
        return out

    def requires_grad_(self, on=True):
        self.parameters()[0].requires_grad_(bool(on))
        return self

    def freeze(self, on=True):
        """declare ALL weights constant (inference): packed weight images are cached across calls.  Training part of the
        model while the rest keeps its values is ``fit(trainable=...)`` / ``trainable_names``, not this."""
        self._need_engine()
        self.engine.freeze_weights(on)
        return self

    def parameter_names(self):
        """the parameter tensors in buffer order (they depend on the hyper-parameters alone: no engine needed)"""
        from .params import param_shapes
        return [n for n, _ in param_shapes(self.hypers, 1)]

    def trainable_names(self, patterns):
        """The parameter tensors ``patterns`` select, for ``fit(trainable=...)`` / ``Trainer(trainable=...)``: tensor names
        ("fc/0/bias"), group names ("mp/2", "fc", "edge_fc", "out", "embed") or fnmatch patterns ("mp/*"), as a list or one
        comma-separated string; a pattern that matches nothing raises ValueError.  (``freeze()`` is something else: all
        weights constant, for inference.)"""
        from .finetune import resolve
        return resolve(patterns, self.parameter_names())

    # -- weights
    def get_weights(self):
        self._need_engine()
        return self.engine.params.state_dict()

    def set_weights(self, state):
        if self.engine is None:
            self._pending_state = state
        else:
            self.engine.params.load_state_dict(state)

    def count_params(self):
        self._need_engine()
        return self.engine.params.count()

    def _need_engine(self):
        if self.engine is None:
            raise RuntimeError("model is not built yet: call it once (or model.build(num_elem))")

    def get_config(self):
        return {'hypers': self.hypers.as_dict(), 'peak_standards': self.peak_standards}

    def save(self, path):
        """own flat format: <path>/weights.npz + <path>/config.json (names follow the Keras variable tree).
        weights.npz also carries the Adam state (``__adam_m`` / ``__adam_v`` flat buffers, ``__adam_t``) once a
        step has been taken, so training resumes where it stopped (the reference's checkpoints hold the Adam
        slots too, main.py:63-68).  The TensorFlow bundle written beside it holds the WEIGHT tensors under the
        reference's variable keys — it is what ``load_model`` reads back and what a TF-side reader can pick tensors
        from by key; it is not a complete Keras SavedModel (no object graph, no saved_model.pb)."""
        self._need_engine()
        os.makedirs(path, exist_ok=True)
        arrays = {k.replace("/", "."): v for k, v in self.engine.params.state_dict().items()}
        if self.engine.adam_t > 0:
            arrays["__adam_m"] = self.engine.adam_m.cpu().numpy()
            arrays["__adam_v"] = self.engine.adam_v.cpu().numpy()
            arrays["__adam_t"] = np.asarray(self.engine.adam_t, np.int64)
        arrays["__train_calls"] = np.asarray(self._train_calls, np.int64)   # seeds the next noise / dropout draw
        np.savez(os.path.join(path, "weights.npz"), **arrays)
        cfg = {"hypers": self.hypers.as_dict(), "num_elem": self.engine.C,
               "peak_standards": {str(k): list(v) for k, v in self.peak_standards.items()}}
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(cfg, f, indent=1)
        # the same weights as a TensorFlow checkpoint bundle under the reference's variable names
        from .tfbundle import save_gnn_bundle
        save_gnn_bundle(os.path.join(path, "variables", "variables"), self.engine.params.state_dict(),
                        self.hypers)

    def load_weights(self, path):
        """weights.npz (own format) or a TensorFlow checkpoint bundle / SavedModel directory."""
        from .library import _bundle_prefix
        if not path.endswith(".npz") and not os.path.exists(os.path.join(path, "weights.npz")):
            prefix = _bundle_prefix(path)
            if prefix is None:
                raise ValueError(f"{path}: no weights.npz and no checkpoint bundle")
            from .tfbundle import load_gnn_bundle
            self.set_weights(load_gnn_bundle(prefix)[0])
            self._pending_adam = "reset"       # our bundle reader takes the weight tensors only
            self._restore_adam()
            return
        f = path if path.endswith(".npz") else os.path.join(path, "weights.npz")
        z = np.load(f)
        self.set_weights({k.replace(".", "/"): z[k] for k in z.files if not k.startswith("__")})
        if "__adam_t" in z.files:
            self._pending_adam = (z["__adam_m"], z["__adam_v"], int(z["__adam_t"]))
        else:
            self._pending_adam = "reset"
        if "__train_calls" in z.files:
            self._train_calls = int(z["__train_calls"])
        self._restore_adam()


def build_GNNModel(hp=None, metrics=True, loss_balance=1.0, device=None, embeddings=None, peak_standards=None):
    """nmrgnn/model.py:12-105.  Declares the hyper-parameter space on ``hp`` (same names/defaults),
    loads the peak standards and returns a GNNModel with ``optimizer`` / ``loss`` attributes set
    (Adam at hp['learning_rate'], NameLoss(s=loss_balance)).
    ``metrics=True`` with an ``embeddings`` dict that has ``'name'`` (nmrdata.load_embeddings(), not shipped here: the
    package has no residue-name table) sets ``model.metrics`` to the reference's 15 metrics (model.py:56-103,
    ``metrics.reference_metrics``; ``ValueError`` when a regular expression matches no name); otherwise
    ``model.metrics = []``.  ``Trainer(..., metrics=model.metrics)`` and ``model.evaluate`` report them.
    ``peak_standards``: ``{element index: (symbol, avg, std)}`` of the training data (``ShiftDataset.standards()`` of the
    train view) in place of the bundled ``standards.load_standards()``; ``save`` / ``load_model`` carry them."""
    from .losses import NameLoss
    from .metrics import reference_metrics
    hp = HyperParameters() if hp is None else hp
    declare_gnn_space(hp)
    model = GNNModel(hp, load_standards() if peak_standards is None else peak_standards, device=device)
    model.metrics = reference_metrics(embeddings) if (metrics and embeddings is not None and 'name' in embeddings) else []
    model.loss = NameLoss(label_idx=None, s=loss_balance)
    model.optimizer = {"name": "Adam", "learning_rate": hp.get('learning_rate'),
                       "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7}
    return model
