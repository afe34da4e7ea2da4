"""The float64 statement of the edge MLP at H = 128 (nmrgnn/model.py:251-261 + layers.py:137-140 + model.py:132-138: RBF, three
softplus layers of 128, E linear outputs, masked by d_src > 0) and of its backward with respect to the weights and biases, shared
by test_gpu_edge_fused.py; tests/test_edge_mlp_ref_host.py checks it on the CPU.  NumPy only.

Criteria (mp_layer_ref.check / rstat):
  per element   |got - ref| <= C_EDGE * mag + 1e-7 * max(mag), mag the same expression on absolute values carried through the chain
  statistical   r = rms(got - ref) / rms(mag) per tensor, held against sqrt(r32s * r_drop): r32s the statistic of a plain float32
                NumPy evaluation of the chain, r_drop that of the float64 evaluation in which the activation-side operand of every
                matrix product (R, Z_l forward; G_l backward) is reduced to its leading fp16 piece (lead_piece)
Both come from the reference side alone; no GPU result enters a threshold.

Exact family: inputs for which the float64 statement consists of float32 numbers that every float32 evaluation order reaches
(exact_forward_case / exact_backward_case; the conditions are asserted per case by the host test)."""
import numpy as np

from mp_layer_ref import STAT_MIN, check, f32, lead_piece, rstat  # noqa: F401  (re-exported to the edge tests)
from test_gpu_edge_h2 import tape_perm  # blocked_flat[tape_perm(n)] == row-major flat of one tape layer [n][128]

H = 128
# per-element constant of `check` for the edge chain: 8 x the largest r32 = max |f32 - f64| / (mag + 1e-7 max mag) of the plain
# float32 NumPy evaluation over the normal cases of test_gpu_edge_fused.py (measured by test_edge_mlp_ref_host.py, which asserts
# 8 * r32 <= C_EDGE per case): largest r32 = 4.89e-6 (dW[2] of the backward of one edge at E = 2, where 1 - exp(-z) of a small
# z cancels; forward 1.7e-7, range-fallback row 1.2e-7)
C_EDGE = 4.0e-5


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def rbf(d_src, d_eff, centers, gap):
    """masked RBF rows and the exponent's argument"""
    m = (d_src > 0).astype(d_eff.dtype)
    arg = -(d_eff[:, None] - centers[None, :]) ** 2 / gap
    return np.exp(arg) * m[:, None], arg, m


# ------------------------------------------------------------------------------------------------------------- float64 statement
def ref_hidden(d_src, d_eff, centers, gap, Ws, bs):
    """the three hidden layers: (R, [z_1, z_2, z_3]) and the magnitudes (m_0, [m_1, m_2, m_3]).  m_0 = R (1 + |arg|) for the
    rounding of the exponent's argument; m_l = (m_{l-1} + |x_{l-1}|) |W_l| + |b_l| + |z_l| (softplus has slope <= 1)"""
    R, arg, _ = rbf(d_src, d_eff, centers, gap)
    x, mx = R, R * (1.0 + np.abs(arg))
    zs, ms = [], []
    for W, b in zip(Ws[:3], bs[:3]):
        z = softplus(x @ W + b)
        mz = (mx + np.abs(x)) @ np.abs(W) + np.abs(b) + np.abs(z)
        zs.append(z)
        ms.append(mz)
        x, mx = z, mz
    return (R, zs), (R * (1.0 + np.abs(arg)), ms)


def ref_output(d_src, z3, m3, Wo, bo):
    m = (d_src > 0)[:, None]
    e = np.where(m, z3 @ Wo + bo, 0.0)                            # a dead row is +0
    return e, np.where(m, (m3 + np.abs(z3)) @ np.abs(Wo) + np.abs(bo), 0.0) + np.abs(e)


def ref_forward(d_src, d_eff, centers, gap, Ws, bs):
    """float64 forward on inputs already rounded to float32: ({"e", "z": [3]}, the same keys' magnitudes)"""
    (_, zs), (_, ms) = ref_hidden(d_src, d_eff, centers, gap, Ws, bs)
    e, me = ref_output(d_src, zs[2], ms[2], Ws[3], bs[3])
    return {"e": e, "z": zs}, {"e": me, "z": ms}


def ref_backward(d_src, d_eff, centers, gap, Ws, zs32, de, drop=False):
    """float64 weight / bias gradients from the float32-rounded tape zs32, as the kernels read it: ({"dW": [4], "db": [4]}, the
    magnitudes = sum over edges of |x| |G| with |G| carried through |W|); the values also carry "G": [G_1, G_2, G_3], the gradients
    at the hidden pre-activations.  drop: every G_l is reduced to its leading fp16 piece before its two matrix products (the r_drop
    evaluation)"""
    R, _, m = rbf(d_src, d_eff, centers, gap)
    xs = [R] + list(zs32)
    red = lead_piece if drop else (lambda a: a)
    dE = de * m[:, None]
    v = {"dW": [None] * 4, "db": [None] * 4, "G": [None] * 3}
    mg = {"dW": [None] * 4, "db": [None] * 4, "G": [None] * 3}
    v["dW"][3], v["db"][3] = xs[3].T @ dE, dE.sum(0)
    mg["dW"][3], mg["db"][3] = np.abs(xs[3]).T @ np.abs(dE), np.abs(dE).sum(0)
    g, gm = dE @ Ws[3].T, np.abs(dE) @ np.abs(Ws[3]).T
    for l in (2, 1, 0):
        slope = -np.expm1(-xs[l + 1])
        G, Gm = red(g * slope), gm * np.abs(slope)
        v["dW"][l], v["db"][l] = xs[l].T @ G, G.sum(0)
        mg["dW"][l], mg["db"][l] = np.abs(xs[l]).T @ Gm, Gm.sum(0)
        v["G"][l], mg["G"][l] = G, Gm
        g, gm = G @ Ws[l].T, Gm @ np.abs(Ws[l]).T
    return v, mg


# ------------------------------------------------------------------------------------------------- the two emulated evaluations
def f32_hidden(d_src, d_eff, centers, gap, Ws, bs, order=None):
    """plain float32 NumPy evaluation of the hidden layers (every operand and intermediate float32); order: a permutation of the
    edges the chain is evaluated in (results returned in the caller's order)"""
    t = np.float32
    ds, dn = d_src.astype(t), d_eff.astype(t)
    if order is not None:
        ds, dn = ds[order], dn[order]
    x, _, _ = rbf(ds, dn, centers.astype(t), t(gap))
    zs = []
    for W, b in zip(Ws[:3], bs[:3]):
        x = softplus(x @ W.astype(t) + b.astype(t))
        zs.append(x)
    assert all(z.dtype == t for z in zs)
    return zs if order is None else [z[np.argsort(order)] for z in zs]


def f32_output(d_src, z3, Wo, bo):
    t = np.float32
    e = np.where((d_src > 0)[:, None], z3.astype(t) @ Wo.astype(t) + bo.astype(t), t(0))
    assert e.dtype == t
    return e


def f32_forward(d_src, d_eff, centers, gap, Ws, bs, order=None):
    zs = f32_hidden(d_src, d_eff, centers, gap, Ws, bs, order)
    return {"e": f32_output(d_src, zs[2], Ws[3], bs[3]), "z": zs}


def drop_hidden(d_src, d_eff, centers, gap, Ws, bs):
    """float64 evaluation in which the activation operand of every matrix product keeps only its leading fp16 piece"""
    x, _, _ = rbf(d_src, d_eff, centers, gap)
    zs = []
    for W, b in zip(Ws[:3], bs[:3]):
        x = softplus(lead_piece(x) @ W + b)
        zs.append(x)
    return zs


def drop_output(d_src, z3, Wo, bo):
    return np.where((d_src > 0)[:, None], lead_piece(z3) @ Wo + bo, 0.0)


def f32_backward(d_src, d_eff, centers, gap, Ws, zs32, de, order=None):
    """plain float32 NumPy evaluation of ref_backward; order: the edge order the sums run in"""
    t = np.float32
    ds, dn, dd = d_src.astype(t), d_eff.astype(t), de.astype(t)
    zs = [z.astype(t) for z in zs32]
    if order is not None:
        ds, dn, dd, zs = ds[order], dn[order], dd[order], [z[order] for z in zs]
    R, _, m = rbf(ds, dn, centers.astype(t), t(gap))
    xs = [R] + zs
    dE = dd * m[:, None]
    dW, db = [None] * 4, [None] * 4
    dW[3], db[3] = xs[3].T @ dE, dE.sum(0, dtype=t)
    g = dE @ Ws[3].astype(t).T
    for l in (2, 1, 0):
        G = g * (t(1) - np.exp(-xs[l + 1]))
        dW[l], db[l] = xs[l].T @ G, G.sum(0, dtype=t)
        g = G @ Ws[l].astype(t).T
    assert all(a.dtype == t for a in dW + db)
    return {"dW": dW, "db": db}


def r32_of(got, ref, mag):
    """max |got - ref| / (mag + 1e-7 max mag): the smallest c_rel with which `check` would pass `got`"""
    top = float(mag.max()) if mag.size else 0.0
    den = mag + 1e-7 * top
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.where(den > 0, den, 1.0)).max()) if mag.size else 0.0


def tensors(v):
    """(name, array) of a forward or backward result dictionary, in a fixed order"""
    out = []
    for k in ("e", "z", "dW", "db"):
        if k in v:
            out += [(k, v[k])] if k == "e" else [(f"{k}{l}", a) for l, a in enumerate(v[k])]
    return out


def stats_of(g32, gd, v, mg):
    """{tensor: (r32, r32s, r_drop)} of a float32 and a dropped-piece evaluation against the float64 values and magnitudes"""
    g32, gd, M = dict(tensors(g32)), dict(tensors(gd)), dict(tensors(mg))
    return {k: (r32_of(g32[k], r, M[k]), rstat(g32[k], r, M[k]), rstat(gd[k], r, M[k])) for k, r in tensors(v) if k in g32}


def forward_stats(c, v, mg):
    """stats_of the forward of case c"""
    a = (c["d_src"], c["d_eff"], c["centers"], c["gap"], c["Ws"], c["bs"])
    zd = drop_hidden(*a)
    return stats_of(f32_forward(*a), {"e": drop_output(c["d_src"], zd[2], c["Ws"][3], c["bs"][3]), "z": zd}, v, mg)


def backward_stats(c, v, mg):
    a = (c["d_src"], c["d_eff"], c["centers"], c["gap"], c["Ws"], c["zs32"], c["de"])
    return stats_of(f32_backward(*a), ref_backward(*a, drop=True)[0], v, mg)


# ----------------------------------------------------------------------------------------------------------------- tape layouts
def tape_to_rows(flat, n, layout):
    """row-major [n][128] of one tape layer stored in `layout` (1 = blocked, 0 = row-major)"""
    flat = np.asarray(flat).reshape(-1)[:n * H]
    return (flat[tape_perm(n)] if layout else flat).reshape(n, H)


def rows_to_tape(rows, layout):
    """one tape layer in `layout` from its row-major [n][128] form"""
    rows = np.asarray(rows)
    n = rows.shape[0]
    if not layout:
        return rows.reshape(-1).copy()
    out = np.empty(n * H, rows.dtype)
    out[tape_perm(n)] = rows.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------------------------------ cases
def normal_hidden(n, seed, p_dead=0.15):
    """the part of a normal case that does not depend on E: distances and the three hidden layers.  Glorot-scale weights, centres
    linspace(0, 1.2, 128), d_eff = d_src + 0.025 noise; a few live edges whose d_eff is negative and a few past the last centre"""
    rng = np.random.default_rng(seed)
    d_src = rng.uniform(0.05, 1.2, n)
    d_src[rng.random(n) < p_dead] = 0.0
    d_eff = np.where(d_src > 0, d_src + 0.025 * rng.standard_normal(n), d_src)
    live = np.flatnonzero(d_src > 0)
    if len(live):
        k = max(1, min(4, len(live) // 8))
        pick = rng.choice(live, min(len(live), 2 * k), replace=False)
        d_eff[pick[:k]] = -rng.uniform(0.001, 0.03, len(pick[:k]))
        d_eff[pick[k:]] = 1.2 + rng.uniform(0.001, 0.05, len(pick[k:]))
    centers = np.linspace(0.0, 1.2, H)
    Wh = [f32(rng.standard_normal((H, H)) * 0.15) for _ in range(3)]
    bh = [f32(rng.standard_normal(H) * 0.1) for _ in range(3)]
    c32 = f32(centers)
    return dict(n=n, family="normal", d_src=f32(d_src), d_eff=f32(d_eff), centers=c32,
                gap=float(np.float32(centers[1] - centers[0])), Wh=Wh, bh=bh)


def normal_output(hid, E, seed):
    """the case completed with the output layer, the upstream gradient de and (lazily, by the tests) the tape"""
    rng = np.random.default_rng(1000003 * E + seed)
    n = hid["n"]
    c = dict(hid, E=E, Ws=hid["Wh"] + [f32(rng.standard_normal((H, E)) * 0.2)], bs=hid["bh"] + [f32(rng.standard_normal(E) * 0.1)],
             de=f32(rng.standard_normal((n, E))))
    return c


def normal_case(n, E, seed, p_dead=0.15):
    return normal_output(normal_hidden(n, seed, p_dead), E, seed)


def _two_perms(rng, vals):
    """sum of two signed, scaled permutation matrices [128][128] with entries in +-vals"""
    W = np.zeros((H, H))
    for _ in range(2):
        W[np.arange(H), rng.permutation(H)] += rng.choice(vals, H) * rng.choice([-1.0, 1.0], H)
    return W


def _on_centres(rng, n, p_dead):
    centers = 64.0 * np.arange(H)
    idx = rng.integers(1, H, n)
    d = centers[idx]
    if n > 1:
        d[rng.random(n) < p_dead] = 0.0
    return centers, d


def exact_hidden(n, seed, p_dead=0.15):
    """exact forward family, the E-independent part.  Edges sit on a centre with index >= 1 of centers = 64 arange(128), gap 1: the
    RBF row is one-hot in float32 and float64.  Every pre-activation is >= 40 or <= -746: softplus is the identity or 0 in
    float32 (max(x, 0) + ln2 log2(1 + 2^(-|x| log2 e))) AND in float64 (exp(-746) = 0), so the float64 statement itself is made
    of float32 numbers.  Layer 0: "on" columns W in {0, 64}, b = 64; "off" columns W in {-192, 0, 64}, b = -1024 (an "on" column
    must not go below 40, and -746 is out of reach of a weight whose 2^8-fold fits an fp16 piece).  Layers 1, 2: two signed
    permutation matrices with entries +-{1, 2}; b = 4096 + {0, 1, 3} / -8192 and 32768 + {0, 1} / -65536: z_2 (3584 .. 4611) and
    z_3 (up to 51213) need more than the 11 bits of one fp16 piece, so the small piece of the activations is in play in layer 2
    and in the output layer"""
    rng = np.random.default_rng(seed)
    centers, d = _on_centres(rng, n, p_dead)
    on = [rng.random(H) < 0.5 for _ in range(3)]
    W0 = np.where(on[0][None, :], rng.choice([0.0, 64.0], (H, H)), rng.choice([-192.0, 0.0, 64.0], (H, H)))
    Wh = [W0, _two_perms(rng, [1.0, 2.0]), _two_perms(rng, [1.0, 2.0])]
    bh = [np.where(on[0], 64.0, -1024.0), np.where(on[1], 4096.0 + rng.choice([0.0, 1.0, 3.0], H), -8192.0),
          np.where(on[2], 32768.0 + rng.choice([0.0, 1.0], H), -65536.0)]
    return dict(n=n, family="exact", d_src=d, d_eff=d.copy(), centers=centers, gap=1.0, Wh=Wh, bh=bh)


def exact_output(hid, E, seed):
    """output layer W in {0, +-1/2, +-1}, b in half-integers"""
    rng = np.random.default_rng(1000003 * E + seed)
    Wo = rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], (H, E))
    bo = rng.integers(-8, 9, E) / 2.0
    return dict(hid, E=E, Ws=hid["Wh"] + [Wo], bs=hid["bh"] + [bo])


def exact_forward_case(n, E, seed, p_dead=0.15):
    return exact_output(exact_hidden(n, seed, p_dead), E, seed)


def exact_backward_case(n, E, seed, p_dead=0.15):
    """exact backward family: edges on centres (one-hot R); tape entries from {0, 40, 48, 64}, about a quarter nonzero, so that
    1 - exp(-z) is exactly 0 or 1 in float32 and float64; hidden weights two signed permutation matrices with entries
    +-{1/2, 1, 2}, output weights in {0, +-1/2, +-1}; de integers in [-2, 2], about half of them zero: every gradient is a short
    dyadic number"""
    rng = np.random.default_rng(seed + 77 * E)
    centers, d = _on_centres(rng, n, p_dead)
    zs32 = [rng.choice([40.0, 48.0, 64.0], (n, H)) * (rng.random((n, H)) < 0.25) for _ in range(3)]
    Ws = [_two_perms(rng, [0.5, 1.0, 2.0]) for _ in range(3)] + [rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], (H, E))]
    de = rng.integers(-2, 3, (n, E)).astype(np.float64) * (rng.random((n, E)) < 0.6)
    return dict(n=n, E=E, family="exact", d_src=d, d_eff=d.copy(), centers=centers, gap=1.0, Ws=Ws,
                bs=[np.zeros(H)] * 3 + [np.zeros(E)], zs32=zs32, de=de)


def grad_scale(Ws, de):
    """the power-of-two scale S of the split-operand backward (edge_bwd_h2.hip, Ranges): max|de| times the largest absolute row
    sums of Wo, W3, W2 in float32, S = 2^(15 - eb) with bound <= 2^eb"""
    t = np.float32
    m = t(np.abs(de).max()) if de.size else t(0)
    nW = [t(np.abs(W.astype(t)).sum(1, dtype=t).max()) for W in (Ws[1], Ws[2], Ws[3])]
    b3 = m * nW[2]
    b2 = b3 * nW[1]
    b1 = b2 * nW[0]
    bound = float(max(b3, b2, b1))
    if not 0 < bound < 3e38:
        return 1.0
    _, eb = np.frexp(bound)
    return float(np.exp2(np.clip(15 - int(eb), -100, 100)))


def granule(x):
    """the largest power of two that divides every element of x (1 for an all-zero x)"""
    x = np.abs(np.asarray(x, np.float64)).reshape(-1)
    x = x[x > 0]
    if not x.size:
        return 1.0
    m, ex = np.frexp(x)
    mi = np.round(m * 2.0 ** 53).astype(np.int64)
    low = np.log2((mi & -mi).astype(np.float64)) + ex - 53
    return float(np.exp2(low.min()))


def two_piece(x):
    """True where x is the sum of an fp16 number and an fp16 number (the two-piece split of the kernels reaches it exactly)"""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16).astype(np.float64)
        lo = (x - hi).astype(np.float16).astype(np.float64)
    return np.isfinite(hi) & (hi + lo == x)
