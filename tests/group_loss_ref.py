"""Host restatements of the ensemble-averaged loss (csrc/group_loss.hip, Engine.loss_groups).

A batch of G graphs (``graph_ptr`` [G+1]) is partitioned into Q groups by ``group_ptr`` [Q+1]; the R_q members of group q have
the same n_q atoms, member r's atom i at row ``graph_ptr[group_ptr[q]] + r n_q + i``; ``mean_ptr`` is the prefix sum of n_q.

``group_mean_f32`` / ``group_spread_f32``: what ng_group_mean / ng_group_spread write, in float32 with every product and sum
rounded on its own, in member order — the device's bits.
``ensemble_loss_f64``: the whole loss (mean over groups of NameLoss(group mean, group labels), nmrgnn/losses.py:4-15,30-39)
and its gradient with respect to every member prediction, in float64.
``ensemble_loss_f32``: the same chain through the float32 mean and spread, the loss arithmetic in ``loss_dtype`` — the
rounding a device result may show against ``ensemble_loss_f64`` (the float64 test takes its bound from it)."""
import numpy as np

f32 = np.float32


def mean_ptr_of(graph_ptr, group_ptr):
    gp, qp = np.asarray(graph_ptr, np.int64), np.asarray(group_ptr, np.int64)
    sizes = np.diff(gp)
    for q in range(len(qp) - 1):
        assert (sizes[qp[q]:qp[q + 1]] == sizes[qp[q]]).all(), f"group {q}: members of different sizes"
    return np.concatenate([[0], np.cumsum(sizes[qp[:-1]])]).astype(np.int64)


def group_mean_f32(graph_ptr, group_ptr, pred, y, w, c=None, names=None):
    """(mean [M], y_out [M], w_out [M], names_out [M] or None) as ng_group_mean writes them"""
    gp, qp = np.asarray(graph_ptr, np.int64), np.asarray(group_ptr, np.int64)
    mp = mean_ptr_of(gp, qp)
    pred, y, w = np.asarray(pred, f32), np.asarray(y, f32), np.asarray(w, f32)
    M = int(mp[-1])
    mean, yo, wo = np.empty(M, f32), np.empty(M, f32), np.empty(M, f32)
    no = None if names is None else np.empty(M, np.int32)
    for q in range(len(qp) - 1):
        g0, R = int(qp[q]), int(qp[q + 1] - qp[q])
        n, a = int(mp[q + 1] - mp[q]), int(gp[g0])
        rows = pred[a:a + R * n].reshape(R, n)
        if c is None:
            acc = rows[0].copy()
            for r in range(1, R):
                acc = (acc + rows[r]).astype(f32)
            m = (acc / f32(R)).astype(f32)
        else:
            cg = np.asarray(c, f32)[g0:g0 + R]
            m = (cg[0] * rows[0]).astype(f32)
            for r in range(1, R):
                m = (m + (cg[r] * rows[r]).astype(f32)).astype(f32)
        mean[mp[q]:mp[q + 1]] = m
        yo[mp[q]:mp[q + 1]] = y[a:a + n]
        wo[mp[q]:mp[q + 1]] = w[a:a + n]
        if names is not None:
            no[mp[q]:mp[q + 1]] = np.asarray(names, np.int32)[a:a + n]
    return mean, yo, wo, no


def group_spread_f32(graph_ptr, group_ptr, dmean, c=None, scale=1.0):
    """dpred [N] as ng_group_spread writes it"""
    gp, qp = np.asarray(graph_ptr, np.int64), np.asarray(group_ptr, np.int64)
    mp = mean_ptr_of(gp, qp)
    dmean, scale = np.asarray(dmean, f32), f32(scale)
    out = np.full(int(gp[-1]), np.nan, f32)
    for q in range(len(qp) - 1):
        g0, R = int(qp[q]), int(qp[q + 1] - qp[q])
        n, a = int(mp[q + 1] - mp[q]), int(gp[g0])
        d = dmean[mp[q]:mp[q + 1]]
        for r in range(R):
            if c is None:
                v = ((d / f32(R)).astype(f32) * scale).astype(f32)
            else:
                v = ((d * np.asarray(c, f32)[g0 + r]).astype(f32) * scale).astype(f32)
            out[a + r * n:a + (r + 1) * n] = v
    return out


def _no_nan(a, b):
    return a / b if b != 0 else 0.0 * a


def name_loss(y, w, x, s, dtype=np.float64):
    """(loss, dloss/dx) of one graph: s * l2 + (1 - s) * (1 - r), every step in ``dtype`` (divide_no_nan throughout; r and
    its gradient in the moment form of losses.py:4-15, the clip passing its gradient inside [0, 1e32])"""
    t = dtype
    y, w, x, s = np.asarray(y, t), np.asarray(w, t), np.asarray(x, t), t(s)
    m = w.sum(dtype=t)
    d = y - x
    l2 = _no_nan((w * d * d).sum(dtype=t), m)
    dl2 = _no_nan(t(-2) * w * d, m)
    if s == 1:
        return l2, dl2
    xm, ym = _no_nan((w * x).sum(dtype=t), m), _no_nan((w * y).sum(dtype=t), m)
    vx = _no_nan((w * x * x).sum(dtype=t), m) - xm * xm
    vy = _no_nan((w * y * y).sum(dtype=t), m) - ym * ym
    cov = (w * (x - xm) * (y - ym)).sum(dtype=t)
    syc = (w * (y - ym)).sum(dtype=t)
    prod = vx * vy
    inside = 0 <= prod <= 1e32
    root = np.sqrt(min(max(prod, t(0)), t(1e32)))
    den = m * root
    r = cov / den if den != 0 else t(0)
    c1 = 1 / den if den != 0 else t(0)
    c2 = cov / (den * den) * vy / root if (den != 0 and inside and root != 0) else t(0)
    dr = w * ((y - ym) - _no_nan(syc, m)) * c1 - c2 * w * (x - xm)
    return s * l2 + (1 - s) * (1 - r), s * dl2 - (1 - s) * dr


def ensemble_loss_f64(graph_ptr, group_ptr, pred, y, w, s=1.0, c=None, scale=1.0):
    """(loss, dpred [N], means [M]) in float64: loss = mean over groups of name_loss(group mean, the first member's labels),
    group mean = sum_r c_r pred_r (c_r = 1 / R_q by default), dpred = scale * dloss / dpred"""
    gp, qp = np.asarray(graph_ptr, np.int64), np.asarray(group_ptr, np.int64)
    mp = mean_ptr_of(gp, qp)
    pred, y, w = np.asarray(pred, np.float64), np.asarray(y, np.float64), np.asarray(w, np.float64)
    Q = len(qp) - 1
    loss, dpred, means = 0.0, np.zeros(int(gp[-1])), np.zeros(int(mp[-1]))
    for q in range(Q):
        g0, R = int(qp[q]), int(qp[q + 1] - qp[q])
        n, a = int(mp[q + 1] - mp[q]), int(gp[g0])
        cg = np.full(R, 1.0 / R) if c is None else np.asarray(c, np.float64)[g0:g0 + R]
        rows = pred[a:a + R * n].reshape(R, n)
        m = (cg[:, None] * rows).sum(axis=0)
        lq, dm = name_loss(y[a:a + n], w[a:a + n], m, s)
        loss += lq / Q
        dpred[a:a + R * n] = (cg[:, None] * dm[None, :] * (scale / Q)).reshape(-1)
        means[mp[q]:mp[q + 1]] = m
    return loss, dpred, means


def ensemble_loss_f32(graph_ptr, group_ptr, pred, y, w, s=1.0, c=None, scale=1.0, loss_dtype=np.float32):
    """(loss, dpred [N]) through the float32 mean and spread; the per-group losses in ``loss_dtype``, dmean rounded to float32
    (the device's ng_loss_l2 works in float32, ng_loss_name keeps its sums in float64)"""
    gp, qp = np.asarray(graph_ptr, np.int64), np.asarray(group_ptr, np.int64)
    mp = mean_ptr_of(gp, qp)
    mean, yo, wo, _ = group_mean_f32(gp, qp, pred, y, w, c)
    Q = len(qp) - 1
    t = loss_dtype
    per, dmean = [], np.empty(int(mp[-1]), f32)
    for q in range(Q):
        sl = slice(int(mp[q]), int(mp[q + 1]))
        lq, dm = name_loss(yo[sl], wo[sl], mean[sl], s, dtype=t)
        per.append(f32(lq))
        dmean[sl] = (np.asarray(dm, t) / t(Q)).astype(f32)
    loss = f32(np.sum(np.asarray(per, f32), dtype=f32) / f32(Q))
    return loss, group_spread_f32(gp, qp, dmean, c, scale)


# ------------------------------------------------------------------------------------------------- test data
def make_case(seed, sizes_members, zero_weight_group=None):
    """(graph_ptr, group_ptr, pred, y, w, names) of groups ``[(n_q, R_q), ...]``: carbon-like shifts 120 +- 3, the members
    of a group scattered 0.7 around the label, equal labels on every member"""
    rng = np.random.default_rng(seed)
    sizes, qp, ys, ws, ns, ps = [], [0], [], [], [], []
    for q, (n, m) in enumerate(sizes_members):
        yq = (120.0 + 3.0 * rng.standard_normal(n)).astype(np.float32)
        wq = (rng.uniform(0.5, 2.0, n) * (rng.uniform(size=n) < 0.85)).astype(np.float32)
        if q == zero_weight_group:
            wq[:] = 0.0
        nq = rng.integers(0, 40, n).astype(np.int32)
        for _ in range(m):
            sizes.append(n)
            ys.append(yq)
            ws.append(wq)
            ns.append(nq)
            ps.append((yq + 0.7 * rng.standard_normal(n)).astype(np.float32))
        qp.append(qp[-1] + m)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return (gp, np.asarray(qp, np.int32), np.concatenate(ps), np.concatenate(ys), np.concatenate(ws), np.concatenate(ns))


def member_weights(seed, group_ptr, zero=True):
    """normalised per group, float32; with ``zero`` the second member of every group of three or more weighs nothing"""
    rng = np.random.default_rng(seed)
    qp = np.asarray(group_ptr, np.int64)
    c = np.empty(int(qp[-1]), np.float32)
    for q in range(len(qp) - 1):
        v = rng.uniform(0.2, 1.0, int(qp[q + 1] - qp[q]))
        if zero and len(v) >= 3:
            v[1] = 0.0
        c[qp[q]:qp[q + 1]] = (v / v.sum()).astype(np.float32)
    return c
