"""Training step for the hot path: forward (noise + dropout) -> NameLoss(s=1) -> backward ->
gradient all-reduce -> Adam.  Mirrors what keras ``model.fit`` does per record in the reference
(nmrgnn/main.py:79-80 with nmrgnn/model.py:44-52), batched over many graphs."""
from __future__ import annotations

import torch

from . import finetune
from .engine import Engine
from .graph import GraphBatch
from .parallel import GradBuckets, shard_grad_weight


class Trainer:
    """Owns the weight update of ``engine``.

    Contract on the packed weight images (``cache_images``, default True): while a Trainer is attached, the engine
    keeps the fp16-piece images of its weights across calls instead of packing them per call; ``Engine.adam_step``
    (``ng_adam_step`` inside an ``ng_weights_frozen`` window) and ``load_state_dict`` rebuild them.  Anything ELSE that
    writes into ``engine.params.flat`` in place between steps (weight surgery, finite-difference probes, a manual
    broadcast, clipping) must call ``engine.weights_changed()`` afterwards, or the next forward multiplies with the
    old images.  ``Trainer(..., cache_images=False)`` keeps per-call packing (always correct, one repack launch per
    call slower); ``close()`` restores the engine's previous setting.

    ``metrics``: a list of ``NameRMSD`` / ``NameCorr`` / ``NameCount`` (``model.metrics``) or a ``NameMetrics``.  A step
    given ``names`` (int32 name ids [N], the int32 of y_true[:, 1]) queues ONE ``ng_name_metrics`` launch on the step's
    training-mode peaks (what keras reports its training metrics on), with ``w`` as the weight column;
    ``metric_results()`` reads them.  A step without ``names`` launches nothing more.

    Fine-tuning.  ``trainable``: the tensors that train — names of ``engine.params.shapes``, group names
    ("mp/2", "fc", "edge_fc") or fnmatch patterns ("mp/*"), see ``finetune.resolve``; everything else keeps its bits,
    moments included, and the backward stops at the lowest stage a trainable tensor needs.  ``lr_scale``: {pattern: scale} on
    the rate of the tensors a pattern selects, the first match winning.  ``clipnorm``: the gradient of the trained tensors is
    clipped to that norm (``last_grad_norm()``).  All three None: the plain step.  In a data-parallel run EVERY RANK MUST BE
    GIVEN THE SAME SET: the all-reduce still moves the whole gradient buffer, whose frozen ranges carry undefined values
    that nothing reads."""

    def __init__(self, engine: Engine, lr=None, loss_balance=1.0, cache_images=True, metrics=None, trainable=None,
                 lr_scale=None, clipnorm=None):
        from .metrics import NameMetrics
        self.engine = engine
        self.metrics = None if not metrics else (metrics if isinstance(metrics, NameMetrics) else NameMetrics(metrics))
        # the trainer owns the weight update: packed weight images are kept and refreshed in one launch behind Adam
        self._prev_cache_images = engine.cache_images
        engine.cache_images = bool(cache_images)
        self.lr = lr
        self.loss_balance = float(loss_balance)      # NameLoss s (build_GNNModel's loss_balance)
        P = engine.params
        # edge-MLP parameters sit first in the flat buffer (params.param_shapes)
        first_node = next(k for k in P.offsets if not k.startswith("edge_fc/"))
        self.buckets = GradBuckets(P.grad, P.offsets[first_node])
        self.step_count = 0
        # fine-tuning: the trainable tensors (None: all, the plain backward) and {tensor: rate scale} (None: the plain Adam)
        names = list(P.shapes)
        self.trainable = None if trainable is None else frozenset(finetune.resolve(trainable, names))
        self.clipnorm = None if clipnorm is None else float(clipnorm)
        self.groups = None
        if trainable is not None or lr_scale or clipnorm is not None:
            self.groups = finetune.scales(names, self.trainable, lr_scale)
        # measure_comm = True: two events per step around the wait for the gradient all-reduces on the compute stream
        # (the time the collectives are EXPOSED, i.e. not hidden under the edge-MLP backward); comm_exposed_ms() reads them
        self.measure_comm = False
        self._comm_events = []

    def step(self, batch: GraphBatch, y: torch.Tensor, w: torch.Tensor, seed=None, total_graphs=None, names=None, groups=None,
             member_weights=None):
        """One optimiser step.  ``total_graphs``: number of graphs over ALL ranks this step (every rank can
        compute it from ``parallel.shard_range``); needed only when the shards are uneven — the loss is a mean
        over graphs, so a rank holding G_local of G_total graphs must weigh its gradient G_local/G_total, not
        1/world.  Default: equal shards.

        ``groups``: the batch's ensemble ``group_ptr`` (host integers [Q + 1] over its graphs, the fifth
        element of a grouped store's ``batches``).  The loss is then the NameLoss of every group's MEAN prediction
        (``Engine.loss_groups`` with ``loss_balance`` as ``s``; ``member_weights`` [G]: the members' weights in the mean,
        normalised per group), ``total_graphs`` counts groups, and the name metrics are taken on the means with the groups'
        labels.  ``groups=None`` is the plain step."""
        eng = self.engine
        if groups is None and member_weights is not None:
            raise ValueError("Trainer.step: member_weights go with groups")
        if groups is not None and (eng.capture_warmup or torch.cuda.is_current_stream_capturing()):
            raise ValueError("Trainer.step(groups=): ensemble steps are not replayed (replay.TrainStepReplay captures the plain "
                             "step only)")
        world, rank = self.buckets.world(), self.buckets.rank()
        if seed is None:
            # different noise / dropout draws on every rank and every step
            # keyed on the optimiser step, which checkpoints carry (Engine.adam_t): a resumed run continues the
            # sequence of draws instead of replaying it
            seed = 0x9E3779B97F4A7C15 ^ (eng.adam_t * 1000003) ^ (rank * 0x5851F42D4C957F2D)
        seed &= (1 << 63) - 1
        wgt = shard_grad_weight(batch.G if groups is None else len(groups) - 1, world, total_graphs)
        if groups is not None:
            # ensemble groups: the loss of the groups' mean predictions (the spread launch applies wgt), the metrics on the means
            peaks = eng.forward(batch, training=True, seed=seed)
            loss, dpred, means, labels = eng.loss_groups(batch, y, w, peaks, groups, s=self.loss_balance,
                                                         member_weights=member_weights, grad_weight=wgt,
                                                         names=names if self.metrics is not None else None)
            if len(labels) == 3:
                self.metrics.update(means, *labels)
        elif self.loss_balance == 1.0:
            # the L2 loss is taken inside the forward: head, loss and the head's backward are one launch where the shape allows
            eng.forward(batch, training=True, seed=seed, loss=(y, w, wgt))
            loss, dpred = eng.tape.loss, None
        else:
            peaks = eng.forward(batch, training=True, seed=seed)
            loss, dpred = eng.loss_name(batch, y, w, peaks, self.loss_balance)
            if wgt != 1.0:
                dpred.mul_(wgt)
        if groups is None and names is not None and self.metrics is not None:
            self.metrics.update(eng.tape.peaks, y, w, names)
        eng.backward(dpred, on_node_grads=self.buckets.launch_node, trainable=self.trainable)
        self.buckets.launch_edge()
        if self.measure_comm:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.buckets.wait()
            e1.record()
            self._comm_events.append((e0, e1))
        else:
            self.buckets.wait()
        eng.adam_step(lr=self.lr, grad_scale=self.buckets.grad_scale(), groups=self.groups, clipnorm=self.clipnorm)
        self.step_count += 1
        return loss

    def last_grad_norm(self):
        """the gradient norm of the last step, over the trained tensors (needs ``clipnorm``; one device-to-host read)"""
        if self.clipnorm is None:
            raise ValueError("Trainer was built without clipnorm: no norm is measured")
        return self.engine.last_grad_norm()

    def trainable_count(self):
        """number of parameters the steps update"""
        P = self.engine.params
        names = P.shapes if self.groups is None else [n for n, sc in self.groups.items() if sc > 0]
        return sum(int(torch.Size(P.shapes[n]).numel()) for n in names)

    def metric_results(self):
        """{metric name: value} of the last step that was given ``names`` (one device-to-host copy)"""
        if self.metrics is None:
            raise ValueError("Trainer was built without metrics")
        return self.metrics.results()

    def comm_exposed_ms(self):
        """mean stall of the compute stream at the all-reduce wait over the steps measured so far (resets)"""
        if not self._comm_events:
            return 0.0
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self._comm_events]
        self._comm_events = []
        return sum(ms) / len(ms)

    def close(self):
        """Detach from the engine: restore its previous ``cache_images`` setting (a bare Engine packs per call)."""
        self.engine.cache_images = self._prev_cache_images
        if not self.engine.cache_images:
            self.engine.weights_changed()
