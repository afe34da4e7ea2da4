"""The hot-path engine: forward and hand-derived backward of GNNModel.call
(nmrgnn/model.py:245-274) as a sequence of C-ABI calls into libnmrgnn_hip.so.

torch is used for device memory and streams only; every arithmetic step is a HIP kernel.
There is no CPU fallback — constructing an Engine without the library / a GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib, finetune
from ._lib import ptr, ptr_array
from .graph import GraphBatch
from .params import ParamStore

ACT = {None: 0, "linear": 0, "softplus": 1, "relu": 2, "tanh": 3}
DROPOUT_RATE = 0.2   # nmrgnn/model.py:217
# batches up to this many atoms take the fused FC-block + head launch in inference (above it the per-layer GEMMs have
# enough rows to fill the chip and the launch chain no longer sets the pace)
FUSED_TAIL_MAX_ATOMS = 16384


def rbf_grid(low, high, count):
    """nmrgnn/layers.py:126-129 — float32 linspace as tf.linspace computes it, gap = c[1]-c[0]."""
    lo, hi = np.float32(low), np.float32(high)
    delta = (hi - lo) / np.float32(count - 1)
    c = (lo + delta * np.arange(count, dtype=np.float32)).astype(np.float32)
    c[-1] = hi
    return c, float(np.float32(c[1] - c[0]))


def edge_path(edge_table, use_live_edges, live_kernels, E, n_edges, min_edges, is_csr, capturing):
    """How the edge stage computes e for one call:
    "table"      the edge-function table, its guard read on the device (fused live-edge kernels only);
    "table_host" the same table, its guard read on the host (edge shapes without the fused kernels);
    "live"       the per-edge MLP over the compacted live slots;
    "slots"      the per-edge MLP over every slot.
    ``live_kernels``: ng_edge_live_supported of the edge shape; ``capturing``: a stream capture is in progress,
    or the eager warm-up of one (``Engine.capture_warmup``).
    The caller still falls back to "slots" where the batch has no live view ("table", "live") or the host-read guard
    is up ("table_host")."""
    # the live kernels and the table index e with 32 bits (check_live in edge_fwd_h2.hip)
    fits = n_edges * E * 4 < (1 << 31)
    sized = edge_table and E <= 8 and n_edges >= min_edges and fits
    if live_kernels and fits:
        return "table" if sized else ("live" if use_live_edges else "slots")
    # is_csr and capturing gate only the host-guarded table: the device-guarded one also runs on CSR batches (through a
    # forced live view) and under capture.  A host read cannot be captured, so a captured call goes per edge here even
    # where its eager warm-up took the table (first finding).
    if sized and not is_csr and not capturing:
        return "table_host"
    return "slots"


class Tape:
    """activations kept between forward(training=True) and backward()"""
    __slots__ = ("batch", "d_eff", "z_save", "z_layout", "e", "h", "A", "S", "fx", "g", "drop_mask",
                 "peaks", "edge_path", "live", "table", "loss", "dpeaks", "dg", "head_partial", "inputs_only")


class GroupMeans:
    """what ``Engine.group_means`` returns: the member means of a batch's ensemble groups with the groups' labels, shaped
    like a batch of Q graphs for the loss calls (``N`` = M means, ``G`` = Q, ``graph_ptr`` = mean_ptr on the device)"""
    __slots__ = ("N", "G", "graph_ptr", "graph_ptr_host", "group_ptr", "member_weights", "means", "y", "w", "names")


class Engine:
    _ids = 0

    def __init__(self, hp, num_elem, peak_std=None, peak_avg=None, device=None, seed=1234):
        if not torch.cuda.is_available():
            raise _lib.NGError("nmrgnn_amd needs an AMD GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.ctx = _lib.get_context(self.device.index)
        self.lib = self.ctx.lib
        self.hp = hp
        self.C = int(num_elem)
        self.F = hp.get('atom_feature_size')
        self.E = hp.get('edge_feature_size')
        self.H = hp.get('edge_hidden_size')
        self.L = hp.get('mp_layers')
        self.Le = hp.get('edge_fc_layers')
        self.Lf = hp.get('fc_layers')
        self.sigma = float(hp.get('noise'))
        self.use_dropout = bool(hp.get('dropout'))
        if hp.get('fc_activation') not in ACT or hp.get('mp_activation') not in ACT:
            raise ValueError(f"unsupported activation {hp.get('fc_activation')!r} / {hp.get('mp_activation')!r}")
        self.fc_act = ACT[hp.get('fc_activation')]
        self.mp_act = ACT[hp.get('mp_activation')]
        self.params = ParamStore(hp, self.C, self.device, seed=seed)
        self.params.on_change = self._on_params_changed
        c, gap = rbf_grid(hp.get('rbf_low'), hp.get('rbf_high'), self.H)
        self.centers = torch.from_numpy(c).to(self.device)
        self.gap = gap
        std = np.ones(self.C, np.float32) if peak_std is None else np.asarray(peak_std, np.float32)[:self.C]
        avg = np.zeros(self.C, np.float32) if peak_avg is None else np.asarray(peak_avg, np.float32)[:self.C]
        self.peak_std = torch.from_numpy(np.ascontiguousarray(std)).to(self.device)
        self.peak_avg = torch.from_numpy(np.ascontiguousarray(avg)).to(self.device)
        # Adam state (keras defaults, nmrgnn/model.py:44-45)
        self.adam_m = torch.zeros_like(self.params.flat)
        self.adam_v = torch.zeros_like(self.params.flat)
        self.adam_t = 0
        # fine-tuning: the launch plan of a backward that trains everything; the segment tables of
        # adam_step(groups=) by their key; the device words (factor, norm) of the last adam_step(clipnorm=)
        self._full_plan = finetune.full_plan(self.L)
        self._seg_tables = {}
        self._clip = None
        self.tape = None
        self._rng_calls = 0
        self._frozen = False
        # training with refreshed images (round 4): the library keeps every packed weight image of this engine and
        # ng_adam_step rebuilds them all in ONE launch right behind the update, instead of one small launch in front of
        # every consumer of the next step.  Weights then have to change through adam_step / params.load_state_dict (or be
        # followed by weights_changed()) — the Trainer, which owns the update, switches it on; a bare Engine keeps packing
        # per call, so code that writes into parameter views directly stays correct.
        self.cache_images = False
        self.defer_reductions = True      # backward(): queue the weight-gradient sums, one launch (ng_defer_reductions)
        # forward(loss=...): head + L2 loss + head backward as one launch where the shape allows (ng_head_loss_bwd)
        self.fuse_head_loss = os.environ.get("NG_HEAD_LOSS", "1") != "0"
        # padded slots (edges == 0) are skipped by the fused edge kernels (include/nmrgnn_hip.h: ng_edge_mlp_fwd_live);
        # NG_EDGE_LIVE=0 runs every slot as rounds 1-3 did (A/B measurements, tests)
        self.use_live_edges = os.environ.get("NG_EDGE_LIVE", "1") != "0"
        # DEFAULT since round 6 (round 5: opt-in; csrc/edge_table.hip): the edge MLP is a function of one scalar per edge —
        # evaluate it on _table_points() equidistant distances and interpolate every edge (cubic); the backward scatters de
        # onto the table (exact adjoint) and runs the MLP backward on the table.  The guard: the same launch evaluates the
        # function at the midpoints too, ng_edge_table_check compares, and where the interpolation error there exceeds
        # ``edge_table_tol`` x max |e| of the table (an absolute bound: a small component of e has no relative one) the SAME
        # call is answered per edge.  With the fused live-edge kernels the guard is read on the device (the per-edge kernels
        # run over a row count that is zero unless it is up); edge shapes without them read it on the host, one
        # synchronisation per call (see edge_path).  NG_EDGE_TABLE=0 / edge_table = False: the per-edge kernels always —
        # what the reference does and what bench.py's `value` is measured on.
        self.edge_table = os.environ.get("NG_EDGE_TABLE", "1") != "0"
        self.edge_table_tol = 3.0e-6          # bound on |interpolant - function| at the midpoints, relative to max |e| of the table
        self.edge_table_min_edges = 262144    # below, the table's extra launches (range, check, gated per-edge launch, interpolation:
                                              # ~60 us) cost more than the per-edge MLP itself (7lgi, one 44 K-edge frame per call: 0.161 against 0.154 ms)
        self.edge_table_force_fallback = False   # tests: raise the guard whatever the check finds (tol = -1)
        # OPT-IN (NG_EDGE_GRAD_TABLE=1): backward(edge_grad=) on a tape of the table path interpolates a table of the edge
        # Jacobian J = d f_W / d d (ng_edge_mlp_dinput's J_out on the table's 2T rows, ng_edge_table_dinput per edge) instead of
        # re-evaluating the MLP in forward mode on every edge.  Guarded like the table of e: where the cubic interpolant of J
        # misses the midpoints by more than ``edge_grad_table_tol`` x max |J| (a relu edge MLP: J has kinks), or the value guard
        # of the call was up, the SAME call is answered per edge.  Off: one ng_edge_mlp_dinput launch on every path.
        self.edge_grad_table = os.environ.get("NG_EDGE_GRAD_TABLE", "0") == "1"
        self.edge_grad_table_tol = 6.7e-6     # bound on |interpolant - J| at the midpoints, relative to max |J| of the table: four times the
                                              # largest floor of the forward-mode fp32 J measured (1.67e-6: DESIGN 7.11)
        self._jgate = None                    # the gate words of the last backward's J check (edge_grad_table_report)
        self._wgen = 0                        # bumped whenever the weights change: a table kept over calls (frozen weights)
        self._table_cache = None
        # set by replay.py around the eager warm-up calls of a chain that is about to be captured: they must take the path
        # the captured call will take (edge_path: capturing), or they size the scratch of another one
        self.capture_warmup = False
        self.last_edge_path = None
        # announced weight changes (load_state_dict, weights_changed()): they leave every packed image invalid, and a captured
        # chain — recorded while the images were valid — holds no pack launch.  ``_images_gen`` is the value of ``_announced``
        # at the last adam_step that rebuilt the images (cache_images): replay.py refuses a chain in between
        self._announced = 0
        self._images_gen = 0
        # the row count of the table's own MLP launches (2T: the table and its midpoints), a device word the live kernels read
        self._rows_2t = torch.full((1,), 2 * self._table_points(), dtype=torch.int32, device=self.device)
        Engine._ids += 1
        self._id = Engine._ids          # owner tag of the frozen-weight cache

    # ------------------------------------------------------------------ frozen weights (inference)
    def freeze_weights(self, on=True):
        """Inference with constant weights: the library keeps its packed weight images across calls instead of
        re-packing them on every call (several launches per call at molecule size).  Weight changes through
        ``params.load_state_dict`` / ``adam_step`` are noticed; after writing into a parameter view directly call
        ``weights_changed()``.  The library's cache is keyed by weight addresses and shared by everything on the
        device, so it is switched on only for the duration of THIS engine's forward calls, under this engine's id."""
        self._frozen = bool(on)
        if not on:
            self._ck(self.lib.ng_weights_frozen(self.ctx.handle, 0), "ng_weights_frozen")

    def _own_images(self):
        """ng_weights_frozen under this engine's id.  The context object counts how often the cache changed hands BETWEEN
        ENGINES (the library then drops every registered rebuild job: an engine coming back re-registers only what its next
        calls use); replay.py reads the count.  Only engines are counted: a caller that passes an owner id of its own to
        ng_weights_frozen at the C ABI drops the jobs too, without the count moving — such a caller must not share a context
        with a TrainStepReplay in use."""
        ctx = self.ctx
        if ctx.image_owner != self._id:
            ctx.image_owner = self._id
            ctx.owner_switches += 1
        self._ck(self.lib.ng_weights_frozen(ctx.handle, self._id), "ng_weights_frozen")

    def weights_changed(self):
        self._wgen += 1
        self._announced += 1
        self._ck(self.lib.ng_weights_changed(self.ctx.handle), "ng_weights_changed")

    def _on_params_changed(self):
        self._wgen += 1
        self._announced += 1
        self.lib.ng_weights_changed(self.ctx.handle)

    # ------------------------------------------------------------------ helpers
    def _st(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _new(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def _ck(self, rc, what):
        self.ctx.check(rc, what)

    def randn(self, n, seed, offset=0):
        out = self._new(n)
        self._ck(self.lib.ng_randn(self.ctx.handle, self._st(), seed, offset, ptr(out), n), "ng_randn")
        return out

    def dropout_mask(self, n, seed, offset=0, keep=1.0 - DROPOUT_RATE):
        out = self._new(n)
        self._ck(self.lib.ng_dropout_mask(self.ctx.handle, self._st(), seed, offset, keep, ptr(out), n),
                 "ng_dropout_mask")
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, batch: GraphBatch, training=False, noise=None, dropout_mask=None, seed=0, keep_tape=None, loss=None):
        """peaks[N].  training=True keeps the tape for backward(); ``keep_tape=True`` keeps it for an inference-mode
        forward too (no noise, no dropout — what autograd through ``model(g, training=False)`` differentiates).
        ``keep_tape="inputs"``: a tape for ``backward(param_grad=False)`` only — the edge MLP keeps no activations (its
        input gradient recomputes them, or reads the Jacobian table), so with frozen weights the edge-function table of an
        earlier call is reused; ``backward(param_grad=True)`` on such a tape raises.
        ``noise`` (xi[N,K], standard normal) / ``dropout_mask`` ([N,F/2], values 0 or 1/keep) may be
        supplied explicitly (parity tests); otherwise they are drawn on the GPU from ``seed``.
        ``loss = (y, w, grad_weight)``: the L2 NameLoss (``loss_l2``) of the peaks is taken inside the forward —
        ``tape.loss`` holds it ONCE ``backward(None)`` HAS RUN (which continues from its gradient); where the shape
        allows, the head, the loss and the head's backward are ONE launch whose second stage rides with the backward's
        other reductions (``ng_head_loss_bwd``; ``fuse_head_loss = False`` / NG_HEAD_LOSS=0: three calls)."""
        if loss is not None and not (training if keep_tape is None else keep_tape):
            raise ValueError("forward(loss=...) needs a tape (training=True)")
        if isinstance(keep_tape, str):
            if keep_tape != "inputs":
                raise ValueError(f"forward: keep_tape is True, False, None or \"inputs\", got {keep_tape!r}")
            if loss is not None:
                raise ValueError("forward(loss=...) forms parameter gradients; keep_tape=\"inputs\" keeps no tape for them")
        if not (self._frozen or self.cache_images):
            return self._forward(batch, training, noise, dropout_mask, seed, keep_tape, loss)
        self._own_images()
        try:
            return self._forward(batch, training, noise, dropout_mask, seed, keep_tape, loss)
        finally:
            self.lib.ng_weights_frozen(self.ctx.handle, 0)

    def forward_moments(self, batch: GraphBatch, seed=0, noise=True):
        """(mu[N], var_drop[N]): the mean and the variance, over the Dropout in front of the output layer, of the shifts of a
        training-mode forward — in closed form (``ng_head_fwd_var``), no mask is drawn and no tape is kept (``self.tape`` is
        left as it is).  ``noise=True`` draws the GaussianNoise on the distances exactly as ``forward(training=True,
        seed=seed)`` does (counter offset 0) — ``mu`` then carries the bits of that call with an all-ones dropout mask;
        ``noise=False`` feeds the distances as they are; a tensor ``noise`` (xi, standard normal, one entry per list slot) is
        added as ``forward(training=True, noise=xi)`` adds it.  The edge-path choice and every launch up to the FC block are
        those of the training-mode forward; the fused FC + head tail is never taken (it produces no g).  A model without
        dropout has keep = 1 and ``var_drop`` exactly 0.  ``var_drop`` is in ppm^2; no gradient of it is formed."""
        xi = noise if isinstance(noise, torch.Tensor) else None
        draw = xi is not None or bool(noise)
        if not (self._frozen or self.cache_images):
            return self._forward(batch, draw, xi, None, seed, moments=True)
        self._own_images()
        try:
            return self._forward(batch, draw, xi, None, seed, moments=True)
        finally:
            self.lib.ng_weights_frozen(self.ctx.handle, 0)

    def ensemble_moments(self, mu, v=None):
        """(mean[N], var_input[N], var_model[N] or None) over the S rows of ``mu`` [S, N] — the shifts of S replicas — and of
        their dropout variances ``v`` [S, N] (``ng_ensemble_moments``: float64 sums in replica order, the unbiased variance,
        0 for S = 1).  The total variance of a shift is var_model + var_input."""
        if mu.dim() != 2 or mu.shape[0] < 1:
            raise ValueError("ensemble_moments: mu must be [S, N] with S >= 1")
        if v is not None and tuple(v.shape) != tuple(mu.shape):
            raise ValueError("ensemble_moments: v must have the shape of mu")
        S, N = int(mu.shape[0]), int(mu.shape[1])
        mu = mu.to(device=self.device, dtype=torch.float32).contiguous()
        v = None if v is None else v.to(device=self.device, dtype=torch.float32).contiguous()
        mean, var_in = self._new(N), self._new(N)
        var_model = None if v is None else self._new(N)
        self._ck(self.lib.ng_ensemble_moments(self.ctx.handle, self._st(), S, N, ptr(mu), ptr(v), ptr(mean), ptr(var_in),
                                              ptr(var_model)), "ng_ensemble_moments")
        return mean, var_in, var_model

    def _forward(self, batch, training, noise, dropout_mask, seed, keep_tape=None, loss=None, moments=False):
        # moments (forward_moments): the launches of a taped training-mode call without its tape; ``training`` says only
        # whether the distance noise is drawn, and the head is ng_head_fwd_var
        tape = False if moments else (bool(training) if keep_tape is None else bool(keep_tape))
        inputs_only = isinstance(keep_tape, str)      # "inputs": the node side keeps its tape, the edge MLP none
        edge_tape = tape and not inputs_only
        lib, h, st = self.lib, self.ctx.handle, self._st()
        P = self.params
        N, K, F, E, H = batch.N, batch.K, self.F, self.E, self.H
        if batch.C != self.C:
            raise ValueError(f"atoms has {batch.C} element columns, model was built for {self.C}")
        ne = batch.n_edges
        # locality hint for the default-width aggregation (results do not depend on it)
        self._ck(lib.ng_ctx_set_graph_span(h, batch.max_graph_atoms), "ng_ctx_set_graph_span")
        d_src = batch.edges.reshape(-1)
        d_eff = d_src
        live_kernels = bool(lib.ng_edge_live_supported(H, E, self.Le, self.fc_act))
        path = edge_path(self.edge_table, self.use_live_edges, live_kernels, E, ne, self.edge_table_min_edges, batch.is_csr,
                         self.capture_warmup or torch.cuda.is_current_stream_capturing())
        # live-edge view: the fused edge kernels walk the compacted live slots only (same e bit for bit); the device-guarded
        # table needs one even where no slot is dead
        live = batch.live_edges(force=path == "table") if path in ("table", "live") else None
        if live is None and path in ("table", "live"):
            path = "slots"
        perm = pos = rows = None
        if live is not None:
            perm, pos, d_c, rows = live
            d_src = d_eff = d_c
            if training and self.sigma > 0:
                d_eff = self._new(ne)       # compacted: the first n_live entries are used
                self._ck(lib.ng_add_noise_live(h, st, seed, 0, ne, ptr(batch.edges), ptr(None if noise is None else noise.reshape(-1)),
                                               self.sigma, ptr(pos), ptr(d_eff)), "ng_add_noise_live")
        elif training and self.sigma > 0:
            d_eff = self._new(ne)
            if noise is None:     # the draw and d + sigma * xi in one launch (the bits of randn + add_scaled)
                self._ck(lib.ng_add_noise(h, st, seed, 0, ne, ptr(d_src), self.sigma, ptr(d_eff)), "ng_add_noise")
            else:
                noise = noise.reshape(-1)
                self._ck(lib.ng_add_scaled(h, st, ne, ptr(d_src), ptr(noise), self.sigma, ptr(d_eff)),
                         "ng_add_scaled")
        # the table of the edge function and the guard's verdict — before the per-edge launch, which on the "table" path runs
        # over gate[1] rows: none unless the guard is up
        table = self._edge_table_build(batch, live, d_eff, edge_tape, training or moments) if path in ("table", "table_host") else None
        if path == "table_host" and table is None:      # the guard, read on the host, is up
            path = "slots"
        if path == "table":
            rows = table["gate"][1:]
        self.last_edge_path = path      # the path this call runs (replay.py compares its warm-up with its capture)
        e = self._new(ne, E)
        z_save, z_layout = None, 0
        if path != "table_host":
            z_save, z_layout = self._edge_mlp_fwd(ne, d_src, d_eff, e, edge_tape, perm, rows)
        if table is not None:       # every slot from the table — unless the device guard is up: then the launch returns at once
            self._ck(lib.ng_edge_table_interp(h, st, ne, E, table["T"], ptr(batch.edges), ptr(d_eff), ptr(pos),
                                              ptr(table["rng"]), ptr(table["e_all"]), ptr(table["gate"]), ptr(e)),
                     "ng_edge_table_interp")
        h0 = self._new(N, F)
        self._ck(lib.ng_embed_fwd(h, st, N, self.C, F, ptr(batch.atoms), ptr(P["embed/kernel"]),
                                  ptr(h0)), "ng_embed_fwd")
        hs, As, Ss = [h0], [], []
        # moments: the layer launches of the taped call (which kernel runs depends on whether A / S are asked for), their
        # by-products written to one scratch pair that every layer overwrites
        scratch = {}

        def taped(*shape):
            if tape:
                return self._new(*shape)
            if shape not in scratch:
                scratch[shape] = self._new(*shape)
            return scratch[shape]
        like_tape = tape or moments
        for l in range(self.L):
            hn = self._new(N, F)
            S = taped(N, F) if (like_tape and self.mp_act != 0) else None
            if batch.is_csr and not tape and not moments and N <= FUSED_TAIL_MAX_ATOMS and lib.ng_mp_layer_short_ok(N, 1, F, E):
                A = None        # molecule-sized inference over CSR lists: one launch per layer
                self._ck(lib.ng_mp_layer_fwd_short_csr(h, st, N, F, E, self.mp_act, 1, ptr(hs[-1]), ptr(batch.row_ptr),
                                                       ptr(batch.nlist), ptr(e), ptr(batch.inv_degree), ptr(P[f"mp/{l}/w"]),
                                                       ptr(hn)), "ng_mp_layer_fwd_short_csr")
            elif batch.is_csr:        # variable-degree lists: row_ptr / col instead of [N,K]
                A = taped(N, E, F) if like_tape else None
                self._ck(lib.ng_mp_layer_fwd_csr(h, st, N, ne, F, E, self.mp_act, 1, ptr(hs[-1]),
                                                 ptr(batch.row_ptr), ptr(batch.nlist), ptr(e),
                                                 ptr(batch.inv_degree), ptr(P[f"mp/{l}/w"]), ptr(hn), ptr(A),
                                                 ptr(S)), "ng_mp_layer_fwd_csr")
            elif not tape and not moments and N <= FUSED_TAIL_MAX_ATOMS and lib.ng_mp_layer_short_ok(N, K, F, E):
                # molecule-sized inference: aggregate + update of the layer in ONE launch (csrc/frame_fused.hip)
                A = None
                self._ck(lib.ng_mp_layer_fwd_short(h, st, N, K, F, E, self.mp_act, 1, ptr(hs[-1]), ptr(batch.nlist_c), ptr(e),
                                                   ptr(batch.inv_degree), ptr(P[f"mp/{l}/w"]), ptr(hn)), "ng_mp_layer_fwd_short")
            else:
                A = taped(N, E, F) if (like_tape and lib.ng_mp_layer_wants_aggregate(F, E, K)) else None
                self._ck(lib.ng_mp_layer_fwd(h, st, N, K, F, E, self.mp_act, 1, ptr(hs[-1]),
                                             ptr(batch.nlist_c), ptr(e), ptr(batch.inv_degree),
                                             ptr(P[f"mp/{l}/w"]), ptr(hn), ptr(A), ptr(S)),
                         "ng_mp_layer_fwd")
            hs.append(hn)
            As.append(A)
            Ss.append(S)
        Wfc = [P[f"fc/{t}/kernel"] for t in range(self.Lf)]
        Bfc = [P[f"fc/{t}/bias"] for t in range(self.Lf)]
        # molecule-sized inference: FC block + head in ONE launch (csrc/frame_fused.hip)
        # (not for a training-mode forward without a tape: the fused tail has no dropout, the layered path applies it)
        if not tape and not moments and not (training and self.use_dropout) and N <= FUSED_TAIL_MAX_ATOMS \
                and lib.ng_fc_head_ok(N, F, self.Lf, self.C, self.fc_act):
            peaks = self._new(N)
            self._ck(lib.ng_fc_head_fwd(h, st, N, F, self.Lf, self.C, self.fc_act, ptr(hs[-1]), ptr_array(Wfc), ptr_array(Bfc),
                                        ptr(P["out/kernel"]), ptr(P["out/bias"]), ptr(batch.atoms), ptr(self.peak_std),
                                        ptr(self.peak_avg), ptr(peaks)), "ng_fc_head_fwd")
            return peaks
        # FC block: every layer in one call; the tape keeps the layer inputs only (nmrgnn/model.py:191-196)
        fx = [hs[-1]]
        for t in range(self.Lf - 1):
            fx.append(self._new(N, F))
        Fh = F // 2
        g = self._new(N, Fh)
        self._ck(lib.ng_fc_block_fwd(h, st, N, F, self.Lf, self.fc_act, ptr(fx[0]), ptr_array(Wfc),
                                     ptr_array(Bfc), ptr_array(fx[1:]), ptr(g)), "ng_fc_block_fwd")
        mask = None
        peaks = self._new(N)
        if moments:
            var = self._new(N)
            keep = (1.0 - DROPOUT_RATE) if self.use_dropout else 1.0
            self._ck(lib.ng_head_fwd_var(h, st, N, Fh, self.C, ptr(g), keep, ptr(P["out/kernel"]), ptr(P["out/bias"]),
                                         ptr(batch.atoms), ptr(self.peak_std), ptr(self.peak_avg), ptr(peaks), ptr(var)),
                     "ng_head_fwd_var")
            return peaks, var
        loss_t = dpeaks = dg = head_partial = None
        nb = 0
        if loss is not None and self.fuse_head_loss and dropout_mask is None:
            nb = int(lib.ng_head_loss_blocks(h, batch.G, Fh, self.C, batch.max_graph_atoms))
        if nb > 0:
            y, w, gw = loss
            keep = (1.0 - DROPOUT_RATE) if (training and self.use_dropout) else 1.0
            loss_t, dg = self._new(1), self._new(N, Fh)
            head_partial = self._new(nb, Fh * self.C + self.C + 1)
            self._ck(lib.ng_head_loss_bwd(h, st, N, batch.G, Fh, self.C, batch.max_graph_atoms, ptr(g), seed, 1 << 40, keep,
                                          None, ptr(P["out/kernel"]), ptr(P["out/bias"]), ptr(batch.atoms),
                                          ptr(self.peak_std), ptr(self.peak_avg), ptr(batch.graph_ptr), ptr(y), ptr(w),
                                          float(gw), ptr(peaks), ptr(dg), ptr(head_partial)),
                     "ng_head_loss_bwd")
        elif training and self.use_dropout and dropout_mask is None:
            # the keep-mask is drawn inside the head launch and kept for the backward (the values of ng_dropout_mask)
            mask = self._new(N, Fh)
            self._ck(lib.ng_head_fwd_dropout(h, st, N, Fh, self.C, ptr(g), seed, 1 << 40, 1.0 - DROPOUT_RATE, ptr(mask),
                                             ptr(P["out/kernel"]), ptr(P["out/bias"]), ptr(batch.atoms),
                                             ptr(self.peak_std), ptr(self.peak_avg), ptr(peaks)), "ng_head_fwd_dropout")
        else:
            if training and self.use_dropout:
                mask = dropout_mask.reshape(N, Fh).contiguous()
            self._ck(lib.ng_head_fwd(h, st, N, Fh, self.C, ptr(g), ptr(mask), ptr(P["out/kernel"]),
                                     ptr(P["out/bias"]), ptr(batch.atoms), ptr(self.peak_std),
                                     ptr(self.peak_avg), ptr(peaks)), "ng_head_fwd")
        if loss is not None and nb == 0:
            y, w, gw = loss
            loss_t, dpeaks = self.loss_l2(batch, y, w, peaks)
            if gw != 1.0:
                dpeaks.mul_(gw)
        if tape:
            tp = Tape()
            tp.loss, tp.dpeaks, tp.dg, tp.head_partial = loss_t, dpeaks, dg, head_partial
            tp.batch, tp.d_eff, tp.z_save, tp.e = batch, d_eff, z_save, e
            tp.z_layout = z_layout
            tp.edge_path, tp.live, tp.table = path, live, table
            tp.inputs_only = inputs_only
            tp.h, tp.A, tp.S, tp.fx, tp.g, tp.drop_mask, tp.peaks = hs, As, Ss, fx, g, mask, peaks
            self.tape = tp
        return peaks

    # ------------------------------------------------------------------ edge MLP and edge function table
    EDGE_TABLE_POINTS = 4096      # E <= 4; 2048 for E = 5 .. 8 (the scatter's 64-bit table and the guard's staged copy share the LDS)

    def _table_points(self):
        return self.EDGE_TABLE_POINTS if self.E <= 4 else self.EDGE_TABLE_POINTS // 2

    def _edge_weights(self):
        P = self.params
        return [P[f"edge_fc/{t}/kernel"] for t in range(self.Le)], [P[f"edge_fc/{t}/bias"] for t in range(self.Le)]

    def _edge_grads(self, view=None):
        """(dW, dB) of the edge MLP: views of params.grad, or ``view(name)`` of a buffer laid out like it"""
        view = view or self.params.g
        return [view(f"edge_fc/{t}/kernel") for t in range(self.Le)], [view(f"edge_fc/{t}/bias") for t in range(self.Le)]

    def _edge_mlp_fwd(self, n, d_src, d_eff, e, tape, perm=None, rows=None):
        """the per-edge MLP over n rows into e: with ``perm`` the live kernels over the rows it lists, as many as the device
        word ``rows`` says; without (``rows`` unused), the every-slot kernels.  Returns the tape (z, its layout) when
        ``tape``, else (None, 0)."""
        lib, h, st = self.lib, self.ctx.handle, self._st()
        z, z_layout = None, 0
        if tape:
            z = self._new(self.Le - 1, n, self.H)
            # element order of the tape the launch is about to write (it depends on the NG_EDGE_* switches in force NOW; the
            # backward is told, so a switch flipped in between cannot make it misread the tape)
            z_layout = int(lib.ng_edge_tape_layout(self.H, self.E, self.Le, self.fc_act, n))
        W, B = self._edge_weights()
        if perm is None:
            self._ck(lib.ng_edge_mlp_fwd(h, st, n, self.H, self.E, self.Le, self.fc_act, ptr(d_src), ptr(d_eff), ptr(self.centers),
                                         self.gap, ptr_array(W), ptr_array(B), ptr(e), ptr(z)), "ng_edge_mlp_fwd")
        else:
            self._ck(lib.ng_edge_mlp_fwd_live(h, st, n, self.H, self.E, self.Le, self.fc_act, ptr(d_src), ptr(d_eff), ptr(perm),
                                              ptr(rows), ptr(self.centers), self.gap, ptr_array(W), ptr_array(B), ptr(e), ptr(z)),
                     "ng_edge_mlp_fwd_live")
        return z, z_layout

    def _edge_mlp_bwd(self, n, d_src, d_eff, z, z_layout, de, grads, perm=None, rows=None):
        """the backward of _edge_mlp_fwd over the same rows: the weight gradients into ``grads`` = (dW, dB)"""
        lib, h, st = self.lib, self.ctx.handle, self._st()
        W, _ = self._edge_weights()
        dW, dB = grads
        if perm is None:
            self._ck(lib.ng_edge_mlp_bwd_tape(h, st, n, self.H, self.E, self.Le, self.fc_act, ptr(d_src), ptr(d_eff),
                                              ptr(self.centers), self.gap, ptr_array(W), ptr(z), ptr(de), ptr_array(dW),
                                              ptr_array(dB), z_layout), "ng_edge_mlp_bwd")
        else:
            self._ck(lib.ng_edge_mlp_bwd_live(h, st, n, self.H, self.E, self.Le, self.fc_act, ptr(d_src), ptr(d_eff), ptr(perm),
                                              ptr(rows), ptr(self.centers), self.gap, ptr_array(W), ptr(z), ptr(de),
                                              ptr_array(dW), ptr_array(dB), z_layout), "ng_edge_mlp_bwd_live")

    def _edge_table_build(self, batch, live, d_eff, tape, training):
        """The table of the edge function for this call (csrc/edge_table.hip) and the guard's gate words: the distance range,
        the T points and their T midpoints, the per-edge MLP on those 2T rows, the check.  ``d_eff``: the distances fed to the
        RBF (noise already added when training), in the compacted row order of the live view ``live``.
        ``live`` None: the host-guarded table of an edge shape without the fused kernels — the every-slot MLP on the 2T rows,
        and the guard's verdict read on the host; None when the guard is up.
        With a live view, frozen weights and no edge tape (``tape``: that of the edge MLP — none for keep_tape="inputs") the
        table of an earlier call is reused while the weights stay the same: then only the call's distance range is checked
        against the table's."""
        lib, h, st = self.lib, self.ctx.handle, self._st()
        pos, n_live = (None, None) if live is None else (live[1], live[3])
        ne, E, T = batch.n_edges, self.E, self._table_points()
        d_src = batch.edges.reshape(-1)
        tol = -1.0 if self.edge_table_force_fallback else float(self.edge_table_tol)
        reuse = live is not None and self._frozen and not tape and not training and not self.edge_table_force_fallback
        gate = torch.empty(8, dtype=torch.int32, device=self.device)
        kept = reuse and self._table_cache is not None and self._table_cache["key"] == (self._wgen, T, E)
        # the call's distance range; a table kept over calls covers a quarter more on either side than the call that builds it
        rng = self._new(4)
        self._ck(lib.ng_edge_table_range(h, st, ne, E, ptr(d_src), ptr(d_eff), ptr(pos), None, 0.25 if reuse and not kept else 0.0,
                                         ptr(rng)), "ng_edge_table_range")
        if kept:        # the check's range-only form: the call's range against the kept table's, whose err and scale it copies
            c = self._table_cache
            self._ck(lib.ng_edge_table_check(h, st, T, E, None, 0.0, ptr(c["rng"]), ptr(rng), ptr(n_live), 2 * T,
                                             ptr(c["gate"]), ptr(gate)), "ng_edge_table_check")
            return {"e_all": c["e_all"], "rng": c["rng"], "gate": gate, "T": T, "kept": c, "cover": rng}
        d_tab, ones = self._new(2 * T), self._new(2 * T)
        perm_tab = None if live is None else torch.empty(2 * T, dtype=torch.int32, device=self.device)
        self._ck(lib.ng_edge_table_points(h, st, T, 1, ptr(rng), ptr(d_tab), ptr(ones), ptr(perm_tab)), "ng_edge_table_points")
        e_all = self._new(2 * T, E)
        # rows 0 .. T-1: the table; rows T .. 2T-1: the midpoints the guard compares at (same launch: the 32 tiles run side by side)
        z_tab, z_layout = self._edge_mlp_fwd(2 * T, ones, d_tab, e_all, tape, perm_tab, self._rows_2t)
        self._ck(lib.ng_edge_table_check(h, st, T, E, ptr(e_all), tol, ptr(rng), None, ptr(n_live), 2 * T, None, ptr(gate)),
                 "ng_edge_table_check")
        if live is None and int(gate[0].item()) != 0:      # the host read of the guard: the one synchronisation of "table_host"
            return None
        kept = None
        if reuse:
            kept = self._table_cache = {"key": (self._wgen, T, E), "e_all": e_all, "rng": rng, "gate": gate}
        # "kept": the entry of _table_cache this call's table is (its Jacobian table is kept beside it); "cover": the call's range
        return {"e_all": e_all, "rng": rng, "gate": gate, "T": T, "d_tab": d_tab, "ones": ones, "perm_tab": perm_tab,
                "z_tab": z_tab, "z_layout": z_layout, "kept": kept, "cover": rng}

    def _edge_table_backward(self, tp, de, grads):
        """the table's share of the edge-weight gradients, into ``grads``: de scattered onto the table's points (the exact
        adjoint of the interpolation), then the MLP backward on its 2T rows — with the device guard over gate[2] rows, zero
        when the guard was up"""
        tb, b = tp.table, tp.batch
        T = tb["T"]
        pos = None if tp.live is None else tp.live[1]
        de_tab = self._new(2 * T, self.E)
        self._ck(self.lib.ng_edge_table_scatter(self.ctx.handle, self._st(), b.n_edges, self.E, T, 2 * T, ptr(b.edges), ptr(tp.d_eff),
                                                ptr(pos), ptr(tb["rng"]), ptr(de), ptr(de_tab)), "ng_edge_table_scatter")
        self._edge_mlp_bwd(2 * T, tb["ones"], tb["d_tab"], tb["z_tab"], tb["z_layout"], de_tab, grads, tb["perm_tab"], tb["gate"][2:])

    def edge_table_report(self, table=None):
        """(guard up?, interpolation error at the midpoints, largest |e| of the table) of the last taped call's table (or of
        ``table``; a call that reused the table of frozen weights reports the error and scale measured when it was built).
        Reads device words: synchronises; for tests and diagnostics.  Raises RuntimeError when there is no table to report on."""
        tb = table if table is not None else (self.tape.table if self.tape is not None else None)
        if tb is None:
            raise RuntimeError("edge_table_report: no edge-function table (no taped call, or the call went per edge)")
        g = tb["gate"].cpu().numpy()
        return bool(g[0]), float(g[4:6].view(np.float32)[0]), float(g[4:6].view(np.float32)[1])

    # ------------------------------------------------------------------ backward
    def backward(self, dpeaks, on_node_grads=None, edge_grad=None, param_grad=True, trainable=None):
        """fills params.grad (overwrite) from the upstream gradient dpeaks[N] (None: the gradient of the loss
        taken inside ``forward(loss=...)``).
        ``on_node_grads`` is called once every non-edge gradient has been enqueued (the data-parallel
        trainer launches the node-side all-reduce there, overlapping the edge-MLP backward).
        ``edge_grad``: a float32 device tensor shaped like ``batch.edges``, OVERWRITTEN with dL/d(edges) — one
        ng_edge_mlp_dinput launch behind the rest, from the tape's distances, de and the current weights; exact on every
        edge path (the table's included: the derivative is of the edge function itself).  With ``edge_grad_table`` on, a tape
        of the table path interpolates the guarded table of the Jacobian instead (``_edge_dinput``).  In training mode it is the
        gradient with respect to the un-noised input (d d_eff / d edges = 1).  params.grad is the same bits either way.
        ``param_grad=False`` (needs ``edge_grad``): input gradients only — the head, FC-block and MPLayer backward get NULL
        weight-gradient outputs (include/nmrgnn_hip.h: no weight-gradient products, partials or queued sums are formed), and
        nothing whose only output is a parameter gradient is launched (no edge-MLP / table backward, no ng_embed_bwd, no
        reduction flush).  ``params.grad`` is left untouched; ``edge_grad`` is bit for bit that of ``param_grad=True``.
        ``trainable`` (fine-tuning; None: everything, today's launches exactly): a set of parameter tensor names
        (``params.shapes``).  The backward stops at the lowest stage a trainable tensor needs (``finetune.launch_plan``): the
        walk is out -> fc -> mp[L-1..0] -> embed, then the edge MLP from the summed de.  A group (out, fc, mp/l, embed,
        edge_fc) is computed when any of its tensors is trainable; frozen groups the walk passes through get NULL
        weight-gradient outputs.  AFTER SUCH A CALL ``params.grad`` IS DEFINED ONLY ON THE COMPUTED GROUPS
        (``finetune.computed_groups``) — there bit for bit what the full backward writes — and holds stale or unwritten values
        elsewhere: hand it to ``adam_step(groups=...)`` with the same tensors, never to the plain ``adam_step()``.
        ``param_grad=False`` with ``trainable`` is refused, and so is ``edge_grad`` when the walk stops above MP layer 0: the
        input gradient needs the full de.  Not to be confused with ``freeze_weights`` (constant weights, inference)."""
        plan = None
        if trainable is not None:
            if not param_grad:
                raise ValueError("backward(trainable=...) forms parameter gradients; param_grad=False forms none")
            names = finetune.check_names(trainable, self.params.shapes)
            plan = finetune.launch_plan(self.L, finetune.group_names(n for n in self.params.shapes if n in names))
            if edge_grad is not None and plan.mp_stop > 0:
                raise ValueError("backward(edge_grad=...) needs the full de, summed over every MP layer; this trainable set "
                                 f"stops the backward above MP layer {plan.mp_stop - 1} (train embed, edge_fc or mp/0, or "
                                 "drop trainable=)")
        if not param_grad:
            if edge_grad is None:
                raise ValueError("backward(param_grad=False) needs edge_grad: without parameter gradients it is the only output")
            if on_node_grads is not None:
                raise ValueError("backward(param_grad=False): on_node_grads hands on parameter gradients, and none are formed")
            if dpeaks is None:
                raise ValueError("backward(param_grad=False) needs dpeaks: the fused head + loss launch already formed the "
                                 "head's weight-gradient partials")
        if edge_grad is not None:
            b = self.tape.batch if self.tape is not None else None
            if b is not None and (edge_grad.dtype != torch.float32 or edge_grad.device != self.device
                                  or not edge_grad.is_contiguous() or tuple(edge_grad.shape) != tuple(b.edges.shape)):
                raise ValueError("backward: edge_grad must be a contiguous float32 tensor on the engine's device, "
                                 "shaped like batch.edges")
        tp = self.tape
        if tp is None:
            raise RuntimeError("backward() without forward(training=True)")
        if tp.inputs_only and param_grad:
            raise RuntimeError("backward(param_grad=True) on a tape of forward(keep_tape=\"inputs\"): the edge MLP kept no "
                               "activations; call backward(param_grad=False, edge_grad=...)")
        lib, h, st = self.lib, self.ctx.handle, self._st()
        # the seven second-stage sums of the node-side weight gradients (head, FC block, MPLayers, embedding) are queued
        # and run as ONE launch before the node gradients are handed on (ng_defer_reductions: same bits, ~45 us less)
        self._ck(lib.ng_defer_reductions(h, st, 1 if self.defer_reductions and param_grad else 0), "ng_defer_reductions")
        if self.cache_images:
            self._own_images()
        try:
            self._backward(tp, dpeaks, on_node_grads, lib, h, st, edge_grad, bool(param_grad), plan)
        finally:
            if self.cache_images:
                lib.ng_weights_frozen(h, 0)
            self._ck(lib.ng_defer_reductions(h, st, 0), "ng_defer_reductions")

    def _backward(self, tp, dpeaks, on_node_grads, lib, h, st, edge_grad=None, param_grad=True, plan=None):
        P = self.params
        # the weight-gradient outputs: views of params.grad, or NULL (param_grad=False)
        wg = P.g if param_grad else (lambda name: None)
        warr = ptr_array if param_grad else (lambda ts: None)
        # plan (backward(trainable=)): where the walk stops and which stages on the way keep their weight-gradient outputs
        if plan is None:
            plan = self._full_plan
        null = lambda name: None
        wg_fc, warr_fc = (wg, warr) if plan.fc_dw else (null, null)
        b = tp.batch
        N, K, F, E = b.N, b.K, self.F, self.E
        Fh = F // 2
        ne = b.n_edges
        self._ck(lib.ng_ctx_set_graph_span(h, b.max_graph_atoms), "ng_ctx_set_graph_span")
        if dpeaks is None and tp.dg is not None:
            # head + loss + head backward ran as one launch in the forward: only its weight-gradient partials are left
            dg = tp.dg
            self._ck(lib.ng_head_loss_reduce(h, st, ptr(tp.head_partial), tp.head_partial.shape[0], Fh, self.C,
                                             ptr(P.g("out/kernel")), ptr(P.g("out/bias")), ptr(tp.loss)),
                     "ng_head_loss_reduce")
        else:
            if tp.dg is not None:
                raise RuntimeError("backward(dpeaks) after forward(loss=...): the head's backward already ran with the "
                                   "loss gradient; call backward(None)")
            if dpeaks is None:
                dpeaks = tp.dpeaks
            if dpeaks is None:
                raise RuntimeError("backward(None) without forward(loss=...)")
            dpeaks = dpeaks.contiguous()
            dg = self._new(N, Fh)
            self._ck(lib.ng_head_bwd(h, st, N, Fh, self.C, ptr(tp.g), ptr(tp.drop_mask),
                                     ptr(P["out/kernel"]), ptr(b.atoms), ptr(self.peak_std),
                                     ptr(dpeaks), ptr(dg), ptr(wg("out/kernel")), ptr(wg("out/bias"))),
                     "ng_head_bwd")
        dx = None
        if plan.fc_run:
            dx = self._new(N, F)
            Wfc = [P[f"fc/{t}/kernel"] for t in range(self.Lf)]
            ns = int(lib.ng_fc_block_scratch_floats(N, F, self.Lf))
            scratch = self._new(ns) if ns else None
            self._ck(lib.ng_fc_block_bwd(h, st, N, F, self.Lf, self.fc_act, ptr_array(tp.fx), ptr(tp.g),
                                         ptr_array(Wfc), ptr(dg), ptr(dx),
                                         warr_fc([wg_fc(f"fc/{t}/kernel") for t in range(self.Lf)]),
                                         warr_fc([wg_fc(f"fc/{t}/bias") for t in range(self.Lf)]),
                                         ptr(scratch)), "ng_fc_block_bwd")
        csc_ptr = csc_edge = de = rec = None
        if plan.mp_stop < self.L:
            csc_ptr, csc_edge = b.csc()
            de = self._new(ne, E)
            # incoming-edge records (source atom + edge features in CSC order): shared by all MP layers
            if E <= 3 and not b.is_csr:
                rec = self._new(ne, 4)
                self._ck(lib.ng_mp_edge_records(h, st, N, K, E, ptr(csc_ptr), ptr(csc_edge), ptr(tp.e), ptr(rec)),
                         "ng_mp_edge_records")
        dh = dx
        for l in reversed(range(plan.mp_stop, self.L)):
            dhn = self._new(N, F)
            wg_mp = wg if plan.mp_dw[l] else null
            if b.is_csr:
                self._ck(lib.ng_mp_layer_bwd_csr(h, st, N, ne, F, E, self.mp_act, ptr(tp.h[l]), ptr(b.row_ptr),
                                                 ptr(b.nlist), ptr(b.row_of), ptr(tp.e), ptr(b.inv_degree),
                                                 ptr(P[f"mp/{l}/w"]), ptr(tp.A[l]), ptr(tp.S[l]), ptr(csc_ptr),
                                                 ptr(csc_edge), ptr(dh), ptr(dhn), ptr(de),
                                                 0 if l == self.L - 1 else 1, ptr(wg_mp(f"mp/{l}/w"))),
                         "ng_mp_layer_bwd_csr")
                dh = dhn
                continue
            self._ck(lib.ng_mp_layer_bwd_rec(h, st, N, K, F, E, self.mp_act, ptr(tp.h[l]), ptr(b.nlist_c),
                                         ptr(tp.e), ptr(b.inv_degree), ptr(P[f"mp/{l}/w"]),
                                         ptr(tp.A[l]), ptr(tp.S[l]), ptr(csc_ptr), ptr(csc_edge),
                                         ptr(dh), ptr(dhn), ptr(de), 0 if l == self.L - 1 else 1,
                                         ptr(wg_mp(f"mp/{l}/w")), ptr(rec)), "ng_mp_layer_bwd")
            dh = dhn
        if not param_grad:      # the embedding, the reductions and the edge MLP's weights: parameter gradients only
            self._edge_dinput(tp, de, edge_grad)
            self.tape = None
            return
        if plan.embed:
            self._ck(lib.ng_embed_bwd(h, st, N, self.C, F, ptr(b.atoms), ptr(dh),
                                      ptr(P.g("embed/kernel"))), "ng_embed_bwd")
        self._ck(lib.ng_flush_reductions(h, st), "ng_flush_reductions")
        if on_node_grads is not None:
            on_node_grads()
        if not plan.edge_fc:        # the edge MLP is frozen: its gradient is not formed
            pass
        elif tp.edge_path == "slots":
            self._edge_mlp_bwd(ne, b.edges, tp.d_eff, tp.z_save, tp.z_layout, de, self._edge_grads())
        elif tp.edge_path == "live":
            perm, _, d_c, n_live = tp.live
            self._edge_mlp_bwd(ne, d_c, tp.d_eff, tp.z_save, tp.z_layout, de, self._edge_grads(), perm, n_live)
        elif tp.edge_path == "table_host":
            self._edge_table_backward(tp, de, self._edge_grads())
        else:
            # "table": the per-edge backward over gate[1] rows (none unless the guard was up) into temporaries, the table's
            # over gate[2] rows (none when it was) into the gradients, and the sum of the two — one of which is exactly zero
            names = [f"edge_fc/{t}/{k}" for t in range(self.Le) for k in ("kernel", "bias")]
            o0 = min(P.offsets[n] for n in names)
            o1 = max(P.offsets[n] + int(np.prod(P.shapes[n])) for n in names)
            tmp = self._new(o1 - o0)
            tv = lambda n: tmp[P.offsets[n] - o0:P.offsets[n] - o0 + int(np.prod(P.shapes[n]))]
            perm, _, d_c, _ = tp.live
            self._edge_mlp_bwd(ne, d_c, tp.d_eff, tp.z_save, tp.z_layout, de, self._edge_grads(tv), perm, tp.table["gate"][1:])
            self._edge_table_backward(tp, de, self._edge_grads())
            blk = P.grad[o0:o1]
            self._ck(lib.ng_add_scaled(h, st, o1 - o0, ptr(blk), ptr(tmp), 1.0, ptr(blk)), "ng_add_scaled")
        if edge_grad is not None:
            self._edge_dinput(tp, de, edge_grad)
        self.tape = None

    def _edge_dinput(self, tp, de, out):
        """dL/d(edges) into ``out`` (slot layout): de . de/dd per edge (ng_edge_mlp_dinput), over the live view where the
        forward had one (the per-edge "live" path and the device-guarded table), over every slot otherwise"""
        b = tp.batch
        if tp.live is not None:
            perm, _, d_src, n_live = tp.live
        else:
            perm = n_live = None
            d_src = b.edges.reshape(-1)
        if not (self.edge_grad_table and tp.table is not None and tp.edge_path in ("table", "table_host")):
            self._jgate = None
            self._edge_mlp_dinput(b.n_edges, d_src, tp.d_eff, perm, n_live, de, None, out)
            return
        # the table path: the Jacobian table and its gate; then the per-edge launch over jgate[1] rows (skipped unless the guard
        # is up) and the interpolation (skipped when it is) — one of the two writes ``out``
        J_all, rng, jgate = self._edge_jacobian_table(tp)
        self._jgate = jgate
        lib, h, st = self.lib, self.ctx.handle, self._st()
        if tp.edge_path == "table":
            self._edge_mlp_dinput(b.n_edges, d_src, tp.d_eff, perm, jgate[1:], de, None, out)
        elif int(jgate[0].item()) != 0:      # "table_host": the guard is read on the host, one of the two launches is issued
            self._edge_mlp_dinput(b.n_edges, d_src, tp.d_eff, None, None, de, None, out)
            return
        self._ck(lib.ng_edge_table_dinput(h, st, b.n_edges, self.E, tp.table["T"], ptr(b.edges), ptr(tp.d_eff),
                                          ptr(None if tp.live is None else tp.live[1]), ptr(rng), ptr(J_all), ptr(jgate), ptr(de),
                                          ptr(out)), "ng_edge_table_dinput")

    def _edge_mlp_dinput(self, n, d_src, d_eff, perm, n_live, de, J_out, out):
        W, B = self._edge_weights()
        self._ck(self.lib.ng_edge_mlp_dinput(self.ctx.handle, self._st(), n, self.H, self.E, self.Le, self.fc_act,
                                             ptr(d_src), ptr(d_eff), ptr(perm), ptr(n_live), ptr(self.centers), self.gap,
                                             ptr_array(W), ptr_array(B), ptr(de), ptr(J_out), ptr(out)), "ng_edge_mlp_dinput")

    def _edge_jacobian_table(self, tp):
        """(J_all [2T, E], the table's range, jgate) for the backward of a call that took the edge-function table: J = d f_W / d d
        at the table's points and midpoints (ng_edge_mlp_dinput's J_out, exact: forward mode on the same rows as e_all) and the
        gate of its check, chained to the value gate of the call — up when the value guard was up, the call's distances left
        the table, J fails at the midpoints or is not finite.  A table kept over calls keeps J_all and its own gate (chained
        to the kept value gate) beside e_all; later calls run the range-only form of the check."""
        lib, h, st = self.lib, self.ctx.handle, self._st()
        tb, E, T = tp.table, self.E, tp.table["T"]
        n_live = None if tp.live is None else tp.live[3]
        # (a forced fallback is this call's alone: its gate is not kept beside a table that later calls read)
        c = None if self.edge_table_force_fallback else tb["kept"]
        jgate = torch.empty(8, dtype=torch.int32, device=self.device)
        if c is None or "J_all" not in c:
            tol = -1.0 if self.edge_table_force_fallback else float(self.edge_grad_table_tol)
            if "d_tab" in tb:
                d_tab, ones, perm_tab = tb["d_tab"], tb["ones"], tb["perm_tab"]
            else:       # a kept table: its points again, from its range
                d_tab, ones = self._new(2 * T), self._new(2 * T)
                perm_tab = None if tp.live is None else torch.empty(2 * T, dtype=torch.int32, device=self.device)
                self._ck(lib.ng_edge_table_points(h, st, T, 1, ptr(tb["rng"]), ptr(d_tab), ptr(ones), ptr(perm_tab)),
                         "ng_edge_table_points")
            J_all, de0, dd0 = self._new(2 * T, E), torch.zeros(2 * T, E, dtype=torch.float32, device=self.device), self._new(2 * T)
            self._edge_mlp_dinput(2 * T, ones, d_tab, perm_tab, None if perm_tab is None else self._rows_2t, de0, J_all, dd0)
            own = jgate if c is None else torch.empty(8, dtype=torch.int32, device=self.device)
            self._ck(lib.ng_edge_table_check(h, st, T, E, ptr(J_all), tol, ptr(tb["rng"]), None, ptr(n_live), 2 * T,
                                             ptr(tb["gate"] if c is None else c["gate"]), ptr(own)), "ng_edge_table_check")
            if c is None:
                return J_all, tb["rng"], jgate
            c["J_all"], c["jgate"] = J_all, own
        self._ck(lib.ng_edge_table_check(h, st, T, E, None, 0.0, ptr(c["rng"]), ptr(tb["cover"]), ptr(n_live), 2 * T,
                                         ptr(c["jgate"]), ptr(jgate)), "ng_edge_table_check")
        return c["J_all"], c["rng"], jgate

    def edge_grad_table_report(self):
        """(guard up?, interpolation error of J at the midpoints, largest |J| of the table) of the J check of the last backward
        (a call on a kept table reports the error and scale measured when its Jacobian table was built).  Reads device words:
        synchronises; for tests and diagnostics.  Raises RuntimeError when the last backward took no Jacobian table."""
        if self._jgate is None:
            raise RuntimeError("edge_grad_table_report: the last backward took no Jacobian table (edge_grad_table off, no "
                               "edge_grad, or a per-edge tape)")
        g = self._jgate.cpu().numpy()
        return bool(g[0]), float(g[4:6].view(np.float32)[0]), float(g[4:6].view(np.float32)[1])

    # ------------------------------------------------------------------ loss / optimiser
    def loss_l2(self, batch, y, w, peaks):
        """NameLoss with s = 1 (nmrgnn/losses.py:30-39), mean over the batch's graphs.
        Returns (loss[1] device tensor, dloss/dpeaks[N])."""
        loss = self._new(1)
        dpred = self._new(batch.N)
        self._ck(self.lib.ng_loss_l2(self.ctx.handle, self._st(), batch.N, batch.G,
                                     ptr(batch.graph_ptr), ptr(y), ptr(w), ptr(peaks), ptr(loss),
                                     ptr(dpred)), "ng_loss_l2")
        return loss, dpred

    def loss_name(self, batch, y, w, peaks, s=1.0):
        """NameLoss with balance ``s`` (nmrgnn/losses.py:30-39): mean over graphs of
        s*l2 + (1-s)*(1-r).  ``w`` is already the label-filtered weight column.
        Returns (loss[1] device tensor, dloss/dpeaks[N])."""
        if not 0.0 <= float(s) <= 1.0:
            raise ValueError("NameLoss balance s must lie in [0, 1]")
        loss = self._new(1)
        dpred = self._new(batch.N)
        self._ck(self.lib.ng_loss_name(self.ctx.handle, self._st(), batch.N, batch.G,
                                       ptr(batch.graph_ptr), ptr(y), ptr(w), ptr(peaks), float(s),
                                       ptr(loss), ptr(dpred)), "ng_loss_name")
        return loss, dpred

    @staticmethod
    def group_layout(graph_ptr, group_ptr, member_weights=None):
        """``(group_ptr int32 [Q+1], mean_ptr int32 [Q+1])`` of the ensemble groups ``group_ptr`` over the graphs of
        ``graph_ptr`` (host arrays), checked: ``group_ptr`` runs from 0 to G strictly increasing, the members of a group have
        the same atom count, ``member_weights`` (if given) has one entry per graph.  ``ValueError`` otherwise."""
        gp = np.asarray(graph_ptr, dtype=np.int64).reshape(-1)
        G = len(gp) - 1
        raw = np.asarray(group_ptr)
        if raw.ndim != 1 or len(raw) < 2 or not np.issubdtype(raw.dtype, np.integer):
            raise ValueError("loss_groups: group_ptr must be a 1-D integer array of at least two entries")
        qp = raw.astype(np.int64)
        if qp[0] != 0 or qp[-1] != G or (np.diff(qp) < 1).any():
            raise ValueError(f"loss_groups: group_ptr must rise strictly from 0 to the batch's {G} graphs")
        sizes = np.diff(gp)
        first = sizes[qp[:-1]]
        bad = np.flatnonzero(sizes != np.repeat(first, np.diff(qp)))
        if len(bad):
            q = int(np.searchsorted(qp, bad[0], side="right") - 1)
            raise ValueError(f"loss_groups: group {q}: graph {int(bad[0])} has {int(sizes[bad[0]])} atoms, the group's first "
                             f"member {int(first[q])}")
        if member_weights is not None and int(np.prod(member_weights.shape)) != G:
            raise ValueError(f"loss_groups: member_weights has {int(np.prod(member_weights.shape))} entries, the batch {G} "
                             "graphs")
        mp = np.zeros(len(qp), np.int64)
        np.cumsum(first, out=mp[1:])
        return qp.astype(np.int32), mp.astype(np.int32)

    def group_means(self, batch, y, w, peaks, group_ptr, member_weights=None, names=None):
        """The member means of the ensemble groups ``group_ptr`` (host integers [Q+1] over the batch's graphs) and the groups'
        labels, by one ``ng_group_mean`` launch: a ``GroupMeans`` with ``means``, ``y``, ``w`` [M] (``names`` [M] int32 when
        given) that stands for a batch of Q graphs of the means in ``loss_l2`` / ``loss_name`` (``N`` = M, ``G`` = Q,
        ``graph_ptr`` = ``mean_ptr``).  ``ValueError`` before the launch as ``loss_groups``."""
        c = None
        if member_weights is not None:
            c = member_weights if isinstance(member_weights, torch.Tensor) else torch.as_tensor(np.asarray(member_weights))
        qp, mp = self.group_layout(batch.graph_ptr_host, group_ptr, c)
        if c is not None:
            c = c.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        Q, M = len(qp) - 1, int(mp[-1])
        meta = torch.from_numpy(np.concatenate([qp, mp])).to(self.device)      # one small copy
        gm = GroupMeans()
        gm.G, gm.N, gm.group_ptr, gm.graph_ptr, gm.graph_ptr_host, gm.member_weights = Q, M, meta[:Q + 1], meta[Q + 1:], mp, c
        gm.means, gm.y, gm.w = self._new(M), self._new(M), self._new(M)
        gm.names = None if names is None else torch.empty(M, dtype=torch.int32, device=self.device)
        self._ck(self.lib.ng_group_mean(self.ctx.handle, self._st(), batch.N, batch.G, Q, ptr(batch.graph_ptr),
                                        ptr(gm.group_ptr), ptr(gm.graph_ptr), ptr(peaks), ptr(c), ptr(y), ptr(w), ptr(names),
                                        ptr(gm.means), ptr(gm.y), ptr(gm.w), ptr(gm.names)), "ng_group_mean")
        return gm

    def loss_groups(self, batch, y, w, peaks, group_ptr, s=1.0, member_weights=None, grad_weight=1.0, names=None):
        """Ensemble-averaged NameLoss: the graphs ``[group_ptr[q], group_ptr[q+1])`` of the batch are the
        frames of one structure, and the loss is the mean over GROUPS of the NameLoss of the group's mean prediction against
        the labels of its first member.  ``group_ptr``: host integers [Q+1].  ``member_weights`` [G] (optional, device or
        host): the weight of every member in its group's mean, normalised per group by the caller (the ``p`` of a
        ``ShiftReweighter``); None: the plain mean.  ``grad_weight`` scales ``dpred`` (``parallel.shard_grad_weight``).
        Three launches: ``ng_group_mean``, ``ng_loss_l2`` (s == 1) or ``ng_loss_name`` on the means, ``ng_group_spread``.
        Returns ``(loss[1], dpred[N], means[M], (y_g[M], w_g[M]))``; with ``names`` (int32 [N]) the last is
        ``(y_g, w_g, names_g)``.  ``ValueError`` before any launch for members of different sizes, a malformed ``group_ptr``
        or ``member_weights`` of the wrong length."""
        if not 0.0 <= float(s) <= 1.0:
            raise ValueError("NameLoss balance s must lie in [0, 1]")
        gm = self.group_means(batch, y, w, peaks, group_ptr, member_weights, names)
        if float(s) == 1.0:
            loss, dmean = self.loss_l2(gm, gm.y, gm.w, gm.means)
        else:
            loss, dmean = self.loss_name(gm, gm.y, gm.w, gm.means, s)
        dpred = self._new(batch.N)
        self._ck(self.lib.ng_group_spread(self.ctx.handle, self._st(), batch.N, batch.G, gm.G, ptr(batch.graph_ptr),
                                          ptr(gm.group_ptr), ptr(gm.graph_ptr), ptr(dmean), ptr(gm.member_weights),
                                          float(grad_weight), ptr(dpred)), "ng_group_spread")
        return loss, dpred, gm.means, ((gm.y, gm.w) if names is None else (gm.y, gm.w, gm.names))

    def _segment_table(self, groups):
        """(n_seg, begin, end, scale) host arrays of ng_adam_step_groups for ``groups`` = {tensor: scale}
        (``finetune.segments``); kept per distinct ``groups``"""
        key = tuple(sorted((str(k), float(v)) for k, v in groups.items()))
        tab = self._seg_tables.get(key)
        if tab is None:
            P = self.params
            segs = finetune.segments(dict(key), {n: int(np.prod(s)) for n, s in P.shapes.items()}, P.offsets)
            n = len(segs)
            tab = (n, (C.c_int64 * max(n, 1))(*[s[0] for s in segs]), (C.c_int64 * max(n, 1))(*[s[1] for s in segs]),
                   (C.c_float * max(n, 1))(*[s[2] for s in segs]))
            self._seg_tables[key] = tab
        return tab

    def last_grad_norm(self):
        """the gradient norm the last ``adam_step(clipnorm=)`` measured, over the trained tensors and after ``grad_scale``
        (one device-to-host read; None before the first such step)"""
        return None if self._clip is None else float(self._clip[1].item())

    def adam_step(self, lr=None, grad_scale=1.0, beta1=0.9, beta2=0.999, eps=1e-7, groups=None, clipnorm=None):
        """One Adam update of the flat buffer from ``params.grad``.  Fine-tuning: ``groups`` = {tensor name:
        rate scale} updates the listed tensors only, each at ``lr * scale`` — a tensor not listed, or of scale 0, keeps the
        bits of its weights and moments and its gradient is not read (what a ``backward(trainable=)`` leaves undefined).
        ``clipnorm``: the gradient of the updated tensors is scaled to that norm where it exceeds it, by one
        ``ng_grad_clip_factor`` launch in front (``last_grad_norm()`` reads the norm); without ``groups`` it clips over
        everything.  Neither given: ``ng_adam_step`` as ever."""
        if lr is None:
            lr = float(self.hp.get('learning_rate'))
        if clipnorm is not None and not (0.0 < float(clipnorm) < float("inf")):
            raise ValueError(f"adam_step: clipnorm must be positive and finite, got {clipnorm}")
        if groups is None and clipnorm is not None:
            groups = {n: 1.0 for n in self.params.shapes}
        tab = None if groups is None else self._segment_table(groups)
        if clipnorm is not None and self._clip is None:
            self._clip = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.adam_t += 1
        self._wgen += 1
        P = self.params
        if self.cache_images:       # the update is followed by ONE launch that rebuilds this engine's packed weight images
            self._own_images()
        try:
            if tab is None:
                self._ck(self.lib.ng_adam_step(self.ctx.handle, self._st(), P.numel, ptr(P.flat), ptr(P.grad),
                                               ptr(self.adam_m), ptr(self.adam_v), lr, beta1, beta2, eps,
                                               self.adam_t, grad_scale), "ng_adam_step")
            else:
                clip = None
                if clipnorm is not None:
                    clip = ptr(self._clip)
                    self._ck(self.lib.ng_grad_clip_factor(self.ctx.handle, self._st(), P.numel, ptr(P.grad), grad_scale, *tab,
                                                          float(clipnorm), clip), "ng_grad_clip_factor")
                self._ck(self.lib.ng_adam_step_groups(self.ctx.handle, self._st(), P.numel, ptr(P.flat), ptr(P.grad),
                                                      ptr(self.adam_m), ptr(self.adam_v), lr, beta1, beta2, eps,
                                                      self.adam_t, grad_scale, *tab, clip), "ng_adam_step_groups")
            if self.cache_images:   # every registered image of this engine is that of the new weights
                self._images_gen = self._announced
        finally:
            if self.cache_images:
                self.lib.ng_weights_frozen(self.ctx.handle, 0)
