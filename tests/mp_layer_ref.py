"""The float64 statement of one MPLayer (nmrgnn/layers.py:26-46 + model.py:165-167) and of its backward, shared
by test_gpu_mp_generic.py and test_gpu_mp_window.py; tests/test_mp_layer_ref_host.py checks it on the CPU.  NumPy and SciPy only:
the device side of those tests is tests/mp_layer_gpu.py.

Two criteria come out of it.
  per element   |got - ref| <= C_REL * mag + 1e-7 * max(mag), mag the same expression on absolute values (check)
  statistical   r = rms(got - ref) / rms(mag) per output tensor (rstat), held against sqrt(r32 * r_drop) (layer_stats):
    r32     the statistic of a plain float32 numpy evaluation of the same formula: the honest error scale
    r_drop  the statistic of the float64 evaluation in which one operand of one contraction is reduced to its leading fp16
            piece under a per-row power-of-two scale, i.e. the `lo x hi` cross term of the split product is missing:
              P  (s_save, h_out)   A   in  P  = inv * (A Wp)        rows of the aggregate [N, E*F]
              dA (de)              dP  in  dA = dP Wp^T             rows of dP [N, F]
              dh (dh_in)           B   in  dh = dH + B Wn           rows of the incoming-edge aggregate of dP [N, E*F]
              dw                   B   in  dw = h^T B               the same rows
Both numbers come from the reference side alone; no GPU result enters a threshold."""
import numpy as np

C_REL = 3e-5
ACT = {"none": 0, "softplus": 1, "relu": 2, "tanh": 3}


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def act_fwd(act, P):
    if act == 1:
        return np.maximum(P, 0) + np.log1p(np.exp(-np.abs(P)))
    if act == 2:
        return np.maximum(P, 0)
    if act == 3:
        return np.tanh(P)
    return P


def act_grad_from_out(act, S):
    if act == 1:
        return -np.expm1(-S)
    if act == 2:
        return (S > 0).astype(np.float64)
    if act == 3:
        return 1.0 - S * S
    return np.ones_like(S)


def scatter_matrix(nl, dtype=np.float64):
    """[N, N*K] sparse 0/1 matrix: row t sums the slots (i, j) with nl[i, j] == t"""
    from scipy.sparse import csr_matrix
    N, K = nl.shape
    return csr_matrix((np.ones(N * K, dtype), (nl.reshape(-1).astype(np.int64), np.arange(N * K))), shape=(N, N * K))


def ref_layer(h, nl, e, inv, w, dH, act, residual):
    """float64 forward and backward of one MPLayer over padded lists, with the per-element magnitudes of every output.
    The backward is handed s_save = the float64 S rounded to float32, as the kernels are."""
    N, K = nl.shape
    E, F = e.shape[2], h.shape[1]
    Wp = w.transpose(2, 0, 1).reshape(E * F, F)                 # Wp[n F + l][m] = w[l][m][n]
    Sc = scatter_matrix(nl)
    v, mg = {}, {}
    slope = None
    for out, hh, ee, WW, dd in ((v, h, e, Wp, dH), (mg, np.abs(h), np.abs(e), np.abs(Wp), np.abs(dH))):
        hg = hh[nl]                                             # [N, K, F]
        A = np.matmul(ee.transpose(0, 2, 1), hg)                # [N, E, F]
        P = inv[:, None] * (A.reshape(N, E * F) @ WW)
        out["A"] = A
        out["s"] = act_fwd(act, P) if out is v else P + np.abs(v["s"])   # + the activation's own rounding
        out["h_out"] = out["s"] + (hh if residual else 0.0)
        if slope is None:
            v["s_in"] = f32(out["s"])
            slope = act_grad_from_out(act, v["s_in"])
        dP = dd * (slope if out is v else np.abs(slope)) * inv[:, None]
        out["dw"] = (A.reshape(N, E * F).T @ dP).reshape(E, F, F).transpose(1, 2, 0)
        dA = (dP @ WW.T).reshape(N, E, F)
        out["de"] = np.matmul(hg, dA.transpose(0, 2, 1))        # [N, K, E]
        out["dh"] = dd + Sc @ np.matmul(ee, dA).reshape(N * K, F)
    return v, mg


def check(name, got, ref, mag, sel=None, c_rel=C_REL):
    """per-element bound; returns max|err| / max(mag) for the comparison with the f32-input GEMM run"""
    got = np.asarray(got, np.float64)
    if sel is not None:
        got, ref, mag = got[sel], ref[sel], mag[sel]
    err = np.abs(got - ref)
    top = float(mag.max()) if mag.size else 0.0
    bad = ~(err <= c_rel * mag + 1e-7 * top)                   # NaN fails
    if bad.any():
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries outside the bound; first at flat {k}: "
                             f"got {got.reshape(-1)[k]!r} ref {ref.reshape(-1)[k]!r} mag {mag.reshape(-1)[k]!r}")
    return float(err.max()) / top if top > 0 else 0.0


# ---------------------------------------------------------------------------------------------------------- statistic
STAT_MIN = 4096                 # selected elements a tensor needs to carry the statistic
STAT_KEYS = ("s", "h_out", "dh", "de", "dw")


def rstat(got, ref, mag, sel=None):
    """rms(got - ref) / rms(mag) over the selected elements"""
    got = np.asarray(got, np.float64)
    if sel is not None:
        got, ref, mag = got[sel], ref[sel], mag[sel]
    den = float(np.sqrt(np.mean(np.square(mag)))) if mag.size else 0.0
    return float(np.sqrt(np.mean(np.square(got - ref)))) / den if den > 0 else 0.0


def lead_piece(x):
    """every row of x [N, M] reduced to its leading fp16 piece under the row's power-of-two scale S = 2^(14 - e), 2^e > max|row|
    (what is left of a two-piece operand whose small piece never reaches the product)"""
    m = np.abs(x).max(axis=1, keepdims=True)
    ex = np.where(m > 0, np.floor(np.log2(np.where(m > 0, m, 1.0))) + 1.0, 0.0)
    S = np.exp2(14.0 - ex)
    return (x * S).astype(np.float16).astype(np.float64) / S


def incoming(nl, e, dP, Sc=None):
    """B [N, E, F]: B[t][n] = sum over the slots (i, j) with nl[i, j] == t of e[i][j][n] * dP[i]"""
    N, K = nl.shape
    Sc = scatter_matrix(nl, dP.dtype) if Sc is None else Sc
    return np.stack([Sc @ (e[:, :, n, None] * dP[:, None, :]).reshape(N * K, -1) for n in range(e.shape[2])], axis=1)


def layer_stats(h, nl, e, inv, w, dH, act, residual, v, mg, live):
    """{key: (r32, r_drop)} for key in STAT_KEYS, against the float64 values v and magnitudes mg of ref_layer.  The backward
    of both emulations takes the slope from v["s_in"], as the kernels take it from the s_save they are handed."""
    N, K = nl.shape
    E, F = e.shape[2], h.shape[1]
    slope = act_grad_from_out(act, v["s_in"])
    Wp = w.transpose(2, 0, 1).reshape(E * F, F)
    Wn = w.transpose(2, 1, 0).reshape(E * F, F)                 # Wn[n F + m][l] = w[l][m][n]
    sel = {"de": live}
    # ---- plain float32 evaluation of the formula of ref_layer
    t = np.float32
    h_, e_, inv_, W_, dd_ = h.astype(t), e.astype(t), inv.astype(t), Wp.astype(t), dH.astype(t)
    hg = h_[nl]
    A = np.matmul(e_.transpose(0, 2, 1), hg)
    s = act_fwd(act, inv_[:, None] * (A.reshape(N, E * F) @ W_)).astype(t)
    dP = dd_ * slope.astype(t) * inv_[:, None]
    dA = (dP @ W_.T).reshape(N, E, F)
    g32 = {"s": s, "h_out": s + (h_ if residual else t(0)),
           "dw": (A.reshape(N, E * F).T @ dP).reshape(E, F, F).transpose(1, 2, 0),
           "de": np.matmul(hg, dA.transpose(0, 2, 1)),
           "dh": dd_ + scatter_matrix(nl, t) @ np.matmul(e_, dA).reshape(N * K, F)}
    assert all(a.dtype == t for a in g32.values())
    r32 = {k: rstat(g32[k], v[k], mg[k], sel.get(k)) for k in STAT_KEYS}
    del g32, hg, A, dA
    # ---- float64 with the small piece of one operand missing (module docstring)
    s = act_fwd(act, inv[:, None] * (lead_piece(v["A"].reshape(N, E * F)) @ Wp))
    dP = dH * slope * inv[:, None]
    dA = (lead_piece(dP) @ Wp.T).reshape(N, E, F)
    B = lead_piece(incoming(nl, e, dP).reshape(N, E * F))
    gd = {"s": s, "h_out": s + (h if residual else 0.0), "de": np.matmul(h[nl], dA.transpose(0, 2, 1)),
          "dh": dH + B @ Wn, "dw": (h.T @ B).reshape(F, E, F).transpose(0, 2, 1)}
    return {k: (r32[k], rstat(gd[k], v[k], mg[k], sel.get(k))) for k in STAT_KEYS}


# ---------------------------------------------------------------------------------------------------------- cases
def padded_case(F, E, K, N, span, act, residual, seed, hub=0, p_dead=0.1):
    """padded lists: graphs of `span` atoms (one graph when span == 0), neighbours inside the own graph; a `hub` > 0 sends
    that many live slots of every graph to one target"""
    rng = np.random.default_rng(seed)
    g = span if span else N
    base = (np.arange(N) // g) * g
    size = np.minimum(base + g, N) - base
    nl = (base[:, None] + (rng.random((N, K)) * size[:, None]).astype(np.int64)).astype(np.int32)
    live = rng.random((N, K)) >= p_dead
    if hub:
        t = min(300, N - 2)
        nl[(nl == t) & live] = t + 1
        slots = np.flatnonzero(live.reshape(-1))
        nl.reshape(-1)[rng.choice(slots, hub, replace=False)] = t
        assert int(((nl == t) & live).sum()) == hub
    e = f32(rng.standard_normal((N, K, E)) * np.where(live, 1.0, 0.0)[:, :, None])
    return dict(kind="padded", F=F, E=E, K=K, N=N, span=span, act=ACT[act], residual=residual, nl=nl, e=e, live=live,
                **_node_inputs(rng, N, F, E, K))


def csr_case(F, E, N, degrees, act, residual, seed, hub=0):
    """CSR lists with the given row lengths; neighbours anywhere in the batch; `hub` extra entries into one target"""
    rng = np.random.default_rng(seed)
    deg = np.asarray(degrees, np.int64)
    col = rng.integers(0, N, int(deg.sum())).astype(np.int32)
    if hub:
        t = N // 2
        col[col == t] = t + 1
        col[rng.choice(len(col), hub, replace=False)] = t
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(row_ptr[-1])
    e = f32(rng.standard_normal((nnz, E)))
    # the reference runs on the padded form with K = the longest row
    K = max(1, int(deg.max()))
    rows = np.repeat(np.arange(N), deg)
    slot = np.arange(nnz) - np.repeat(row_ptr[:-1], deg)
    nl = np.zeros((N, K), np.int32)
    nl[rows, slot] = col
    ep = np.zeros((N, K, E))
    ep[rows, slot] = e
    live = np.zeros((N, K), bool)
    live[rows, slot] = True
    return dict(kind="csr", F=F, E=E, K=K, N=N, span=0, act=ACT[act], residual=residual, nl=nl, e=ep, live=live,
                row_ptr=row_ptr, col=col, e_flat=e, rows=rows, slot=slot, **_node_inputs(rng, N, F, E, K))


def _node_inputs(rng, N, F, E, K):
    # weights scaled so that P stays O(1): activation slopes away from 0 (their float32 form is then good to a few ulp)
    return dict(h=f32(rng.standard_normal((N, F)) * 0.5), inv=f32(rng.uniform(0.05, 1.0, N)),
                w=f32(rng.standard_normal((F, F, E)) / np.sqrt(F * E * K)), dH=f32(rng.standard_normal((N, F))))


def degrees_with(rng, N, hi, must):
    d = rng.integers(0, hi + 1, N)
    d[:len(must)] = must
    return rng.permutation(d)
