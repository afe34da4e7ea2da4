"""Per-name shift metrics (nmrgnn/metrics.py): ``type_mask``, ``NameRMSD``, ``NameCorr``, ``NameCount``, and
``NameMetrics``, which evaluates up to 32 of them in ONE device pass (``ng_name_metrics``).

The inputs are the reference's ``y_true[N, 3]`` = [shift, name id (float), weight] and ``y_pred[N]``.  For a metric with
``label_idx`` = ln the mask is ``m_i = y_true[i, 2] * any(int32(y_true[i, 1]) == ln)`` (metrics.py:38-39), the weight used
as given.  The device reduces, per metric, the seven float64 sums {S0 = sum m, sum m (y - p)^2, sum m y, sum m p,
sum m y^2, sum m p^2, sum m y p}; ``result()`` / ``results()`` read them (the one device-to-host copy) and form

* NameRMSD  ``sqrt(divide_no_nan(sum m (y - p)^2, sum m))``               (metrics.py:36-43)
* NameCount ``sum m``                                                    (metrics.py:64-70)
* NameCorr  ``cov / (m sqrt((xm2 - xm^2) (ym2 - ym^2)))``, divide_no_nan   (metrics.py:91-116; no clip, unlike the loss)

Edge cases:

* an empty class (sum m == 0): RMSD 0 and count 0, as in the reference; r is NaN, as in the reference (its xm = 0/0).
* a variance that is zero after rounding (constant labels or predictions): a variance below 1e-12 of the mean square (a
  spread under 1e-6 of the values, a few fp32 ulps) counts as zero, so r is 0.  Deliberate deviation: the reference's
  exact-arithmetic answer is 0 as well, its fp32 rounding can give NaN or noise instead.
* name ids outside the membership table, and negative ids, belong to no class (as in the reference, whose label ids are
  table entries).

``update_state`` OVERWRITES the state, as the reference's ``assign`` does.  ``NameMetrics(..., accumulate=True)`` sums
instead until ``reset_states()`` — the statistic of a validation set (``GNNModel.evaluate``).  There is no CPU path: the
sums run on the GPU through libnmrgnn_hip.so."""
from __future__ import annotations

import math
import re

import numpy as np
import torch

from . import _lib
from ._lib import ptr

MAX_CLASSES = 32          # one bit per metric in the uint32 membership table
MAX_NAME_ID = 1 << 24     # largest label id a membership table is built for
VAR_RTOL = 1e-12          # a variance below VAR_RTOL x mean square is zero (module docstring)
_MOMENTS = 7


def type_mask(label_name, embeddings, regex=False):
    """nmrgnn/metrics.py:5-19: the name ids of ``embeddings['name']`` that ``label_name`` selects.
    ``regex=True``: every id whose key ``re.match``-es ``label_name`` — a PREFIX match (``'GLU'`` matches ``'GLU-H'``);
    ``ValueError`` when nothing matches.  Otherwise ``[embeddings['name'][label_name]]``."""
    if regex:
        m = re.compile(label_name)
        ln = [v for k, v in embeddings['name'].items() if m.match(k)]
        if len(ln) == 0:
            raise ValueError('Regular expression did not match any embeddings')
        return ln
    return [embeddings['name'][label_name]]


def _rmsd(s):
    with np.errstate(invalid='ignore'):
        return float(np.sqrt(s[1] / s[0])) if s[0] != 0 else 0.0


def _count(s):
    return float(s[0])


def _corr(s):
    S0, _, Sx, Sy, Sxx, Syy, Sxy = (float(v) for v in s)
    if S0 == 0:
        return math.nan
    xm, ym = Sx / S0, Sy / S0
    xm2, ym2 = Sxx / S0, Syy / S0
    vx, vy = xm2 - xm * xm, ym2 - ym * ym
    vx = 0.0 if vx <= VAR_RTOL * abs(xm2) else vx
    vy = 0.0 if vy <= VAR_RTOL * abs(ym2) else vy
    cov = Sxy - xm * Sy                   # = sum m (x - xm)(y - ym)
    den = S0 * math.sqrt(vx * vy)
    return cov / den if den != 0 else 0.0


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return None


def _split_y_true(y_true, device):
    """y_true[N, 3] -> (shift, weight, int32 name id) contiguous device tensors; int32() truncates like tf.cast"""
    yt = y_true if isinstance(y_true, torch.Tensor) else torch.as_tensor(np.asarray(y_true))
    yt = yt.to(device=device, dtype=torch.float32)
    if yt.dim() != 2 or yt.shape[1] < 3:
        raise ValueError(f"y_true must be [N, 3] (shift, name id, weight); got {tuple(yt.shape)}")
    return yt[:, 0].contiguous(), yt[:, -1].contiguous(), yt[:, 1].to(torch.int32)


class NameMetrics:
    """Up to 32 ``NameRMSD`` / ``NameCorr`` / ``NameCount`` metrics evaluated by ONE ``ng_name_metrics`` launch per update.

    ``member`` (uint32 per name id, bit k set for ``metrics[k]``'s label ids) is built once per device.  ``update`` takes
    device tensors and converts nothing; it queues the launch on the current stream and never waits for the device.
    ``moments`` is the ``[K, 7]`` float64 device tensor of sums (a data-parallel caller may all-reduce it).
    ``accumulate=False``: every update overwrites (the reference); ``True``: updates add up until ``reset_states()``."""

    def __init__(self, metrics, accumulate=False):
        metrics = list(metrics)
        if not 1 <= len(metrics) <= MAX_CLASSES:
            raise ValueError(f"NameMetrics takes 1 to {MAX_CLASSES} metrics, got {len(metrics)}")
        for m in metrics:
            if not isinstance(m, _NameMetric):
                raise TypeError(f"NameMetrics takes NameRMSD / NameCorr / NameCount, got {type(m).__name__}")
        self.metrics = metrics
        self.accumulate = bool(accumulate)
        ids = [np.atleast_1d(m.ln).astype(np.int64) for m in metrics]
        top = max([int(i.max()) for i in ids if i.size] + [-1])
        if top >= MAX_NAME_ID:
            raise ValueError(f"label id {top} is too large for a membership table (limit {MAX_NAME_ID - 1})")
        table = np.zeros(max(top + 1, 1), np.uint32)
        for k, i in enumerate(ids):
            i = i[i >= 0]                 # a negative name id belongs to no class
            table[i] |= np.uint32(1 << k)
        self._table = table
        self.n_names = top + 1
        self.device = None
        self.member = None
        self.moments = None
        self.updates = 0                  # updates since construction / reset_states()

    @property
    def K(self):
        return len(self.metrics)

    def _bind(self, device):
        if self.device == device:
            return
        if device.type != 'cuda':
            raise ValueError("NameMetrics runs on the GPU: pass device tensors to update()")
        self.ctx = _lib.get_context(device.index)
        self.member = torch.from_numpy(self._table.view(np.int32)).to(device)
        self.moments = torch.zeros(self.K, _MOMENTS, dtype=torch.float64, device=device)
        self.device = device
        self.updates = 0

    def update(self, pred, y, w, names):
        """Queue one update: ``pred``, ``y``, ``w`` float32 [N] and ``names`` int32 [N], contiguous, on one GPU."""
        if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
            raise ValueError("NameMetrics.update: pred must be a float32 tensor on the GPU")
        dev, N = pred.device, pred.numel()
        for t, dt, what in ((pred, torch.float32, 'pred'), (y, torch.float32, 'y'), (w, torch.float32, 'w'),
                            (names, torch.int32, 'names')):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or t.device != dev:
                raise ValueError(f"NameMetrics.update: {what} must be a {dt} tensor on {dev}")
            if t.numel() != N or not t.is_contiguous():
                raise ValueError(f"NameMetrics.update: {what} must be contiguous with {N} elements")
        self._bind(dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        self.ctx.check(self.ctx.lib.ng_name_metrics(self.ctx.handle, _lib._vp(st), N, ptr(y), ptr(w), ptr(names), ptr(pred),
                                                    self.n_names, ptr(self.member), self.K, 1 if self.accumulate else 0,
                                                    ptr(self.moments)), "ng_name_metrics")
        self.updates += 1

    def update_state(self, y_true, y_pred, sample_weight=None):
        """``update`` from the reference's ``(y_true[N, 3], y_pred[N])`` (NumPy or torch, host or device).
        ``sample_weight`` is accepted and ignored, as in the reference."""
        dev = _device_of(y_pred, y_true) or self.device or torch.device('cuda', torch.cuda.current_device())
        y, w, names = _split_y_true(y_true, dev)
        p = y_pred if isinstance(y_pred, torch.Tensor) else torch.as_tensor(np.asarray(y_pred))
        p = p.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        self.update(p, y, w, names)

    def reset_states(self):
        if self.moments is not None:
            self.moments.zero_()
        self.updates = 0

    def results(self):
        """{metric.name: float}: ONE device-to-host copy of ``moments``.  Before any update (or right after a reset)
        every value is 0.0, the reference's initial state."""
        if self.updates == 0:
            return {m.name: 0.0 for m in self.metrics}
        s = self.moments.cpu().numpy()
        return {m.name: m._from_moments(s[k]) for k, m in enumerate(self.metrics)}


class _NameMetric:
    """The reference's keras metric surface: ``(label_idx, name=..., **kwargs)``, ``update_state``, ``result``,
    ``reset_states``, ``get_config``.  One metric is a ``NameMetrics`` of K = 1."""
    default_name = None

    def __init__(self, label_idx, name=None, **kwargs):
        self.name = self.default_name if name is None else name
        self.dtype = kwargs.pop('dtype', 'float32')
        self.label_idx = label_idx
        self.ln = np.array(label_idx, dtype=np.int32)
        self._nm = None

    def get_config(self):
        return {'name': self.name, 'dtype': self.dtype, 'label_idx': self.label_idx}

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def _single(self):
        if self._nm is None:
            self._nm = NameMetrics([self])
        return self._nm

    def update_state(self, y_true, y_pred, sample_weight=None):
        self._single().update_state(y_true, y_pred, sample_weight)

    def result(self):
        return self._single().results()[self.name]

    def reset_states(self):
        self._single().reset_states()

    def __repr__(self):
        return f"{type(self).__name__}(label_idx={self.label_idx!r}, name={self.name!r})"


class NameRMSD(_NameMetric):
    """Weighted RMSD of the atoms whose name id is in ``label_idx`` (nmrgnn/metrics.py:22-47).  An empty class gives 0."""
    default_name = 'name-specific-loss'

    @staticmethod
    def _from_moments(s):
        return _rmsd(s)


class NameCount(_NameMetric):
    """Sum of the weights of the atoms whose name id is in ``label_idx`` (nmrgnn/metrics.py:49-73)."""
    default_name = 'avg-name-count'

    @staticmethod
    def _from_moments(s):
        return _count(s)


class NameCorr(_NameMetric):
    """Weighted Pearson r between shifts and predictions of the atoms whose name id is in ``label_idx``
    (nmrgnn/metrics.py:76-116).  An empty class gives NaN; a (numerically) constant side gives 0 (module docstring)."""
    default_name = 'name-specific-r'

    @staticmethod
    def _from_moments(s):
        return _corr(s)

    @staticmethod
    def corr_coeff(x, y, w=None):
        """nmrgnn/metrics.py:105-116 on host arrays (float64), with this module's edge cases."""
        x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
        w = np.ones_like(x) if w is None else np.asarray(w, np.float64).reshape(-1)
        return _corr([w.sum(), 0.0, (w * x).sum(), (w * y).sum(), (w * x * x).sum(), (w * y * y).sum(),
                      (w * x * y).sum()])


def reference_metrics(embeddings):
    """The 15 metrics ``build_GNNModel(metrics=True)`` compiles into the model (nmrgnn/model.py:56-103), in the
    reference's order and with its regular expressions verbatim.  ``ValueError`` when one matches no name."""
    tm = lambda rx: type_mask(rx, embeddings, regex=True)
    ha = tm(r'.*\-HA.*')
    dft, mb = tm(r'DFT.*'), tm(r'MB.*')
    return [
        NameRMSD(tm(r'.*\-H.*'), name='h_rmsd'),
        NameRMSD(tm(r'.*\-N.*'), name='n_rmsd'),
        NameRMSD(tm(r'.*\-C.*'), name='c_rmsd'),
        NameRMSD(tm(r'.*\-H$'), name='hn_rmsd'),
        NameRMSD(tm(r'.*\-HA*'), name='ha_rmsd'),
        NameCorr(tm(r'.*\-H.*'), name='h_r'),
        NameCorr(tm(r'.*\-N.*'), name='n_r'),
        NameCorr(tm(r'.*\-C.*'), name='c_r'),
        NameCorr(tm(r'.*\-H$'), name='hn_r'),
        NameCorr(ha, name='ha_r'),
        NameCount(ha, name='avg_ha_count'),
        NameCorr(mb, name='mb_r'),
        NameCount(mb, name='avg_mb_count'),
        NameCorr(dft, name='dft_r'),
        NameCount(dft, name='avg_dft_count'),
    ]
