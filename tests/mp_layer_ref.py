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


def f32_layer(h, nl, e, inv, w, dH, act, residual, slope):
    """plain float32 NumPy evaluation of ref_layer's formulas (every operand and every intermediate float32); the backward takes
    the slope it is handed, as the kernels take it from s_save"""
    N, K = nl.shape
    E, F = e.shape[2], h.shape[1]
    t = np.float32
    Wp = w.transpose(2, 0, 1).reshape(E * F, F)
    h_, e_, inv_, W_, dd_ = h.astype(t), e.astype(t), inv.astype(t), Wp.astype(t), dH.astype(t)
    hg = h_[nl]
    A = np.matmul(e_.transpose(0, 2, 1), hg)
    s = act_fwd(act, inv_[:, None] * (A.reshape(N, E * F) @ W_)).astype(t)
    dP = dd_ * slope.astype(t) * inv_[:, None]
    dA = (dP @ W_.T).reshape(N, E, F)
    g32 = {"A": A, "s": s, "h_out": s + (h_ if residual else t(0)),
           "dw": (A.reshape(N, E * F).T @ dP).reshape(E, F, F).transpose(1, 2, 0),
           "de": np.matmul(hg, dA.transpose(0, 2, 1)),
           "dh": dd_ + scatter_matrix(nl, t) @ np.matmul(e_, dA).reshape(N * K, F)}
    assert all(a.dtype == t for a in g32.values())
    return g32


def layer_stats(h, nl, e, inv, w, dH, act, residual, v, mg, live, keys=STAT_KEYS):
    """{key: (r32, r_drop)} for key in keys, against the float64 values v and magnitudes mg of ref_layer.  The backward
    of both emulations takes the slope from v["s_in"], as the kernels take it from the s_save they are handed."""
    N, K = nl.shape
    E, F = e.shape[2], h.shape[1]
    slope = act_grad_from_out(act, v["s_in"])
    Wp = w.transpose(2, 0, 1).reshape(E * F, F)
    Wn = w.transpose(2, 1, 0).reshape(E * F, F)                 # Wn[n F + m][l] = w[l][m][n]
    sel = {"de": live}
    # ---- plain float32 evaluation of the formula of ref_layer
    g32 = f32_layer(h, nl, e, inv, w, dH, act, residual, slope)
    r32 = {k: rstat(g32[k], v[k], mg[k], sel.get(k)) for k in keys}
    del g32
    # ---- float64 with the small piece of one operand missing (module docstring)
    s = act_fwd(act, inv[:, None] * (lead_piece(v["A"].reshape(N, E * F)) @ Wp))
    gd = {"s": s, "h_out": s + (h if residual else 0.0)}
    if set(keys) - set(gd):                                     # a backward key is asked for
        dP = dH * slope * inv[:, None]
        dA = (lead_piece(dP) @ Wp.T).reshape(N, E, F)
        B = lead_piece(incoming(nl, e, dP).reshape(N, E * F))
        gd.update(de=np.matmul(h[nl], dA.transpose(0, 2, 1)), dh=dH + B @ Wn, dw=(h.T @ B).reshape(F, E, F).transpose(0, 2, 1))
    return {k: (r32[k], rstat(gd[k], v[k], mg[k], sel.get(k))) for k in keys}


# ---------------------------------------------------------------------------------------------------------- cases
def graph_layout(N, span):
    """graph index, first row and size of every atom's graph.  span: an int (graphs of that many atoms; one graph when 0) or a
    sequence of graph sizes whose last one repeats (mixed spans in one batch)"""
    if np.ndim(span) == 0:
        g = int(span) if span else N
        gi = np.arange(N) // g
        base = gi * g
        return gi, base, np.minimum(base + g, N) - base
    sizes, starts, at = list(span), [], 0
    while at < N:
        starts.append(at)
        at += int(sizes[min(len(starts) - 1, len(sizes) - 1)])
    starts = np.array(starts + [at], np.int64)
    gi = np.searchsorted(starts, np.arange(N), side="right") - 1
    return gi, starts[gi], np.minimum(starts[gi + 1], N) - starts[gi]


def padded_case(F, E, K, N, span, act, residual, seed, hub=0, p_dead=0.1, bias=None, hub_local=False):
    """padded lists: graphs of `span` atoms (graph_layout), neighbours inside the own graph; a `hub` > 0 sends that many live
    slots (of the whole batch, or with hub_local of the target's own graph) to one target.  bias = (form, p) draws a slot's
    local index as size * u^p: "low" favours the lower-numbered atoms of every graph, "ends" the higher-numbered atoms of the
    even graphs and the lower-numbered ones of the odd graphs (targets on both sides of every second graph boundary crowd)"""
    rng = np.random.default_rng(seed)
    gi, base, size = graph_layout(N, span)
    u = rng.random((N, K))
    if bias is not None:
        u = u ** bias[1]
        if bias[0] == "ends":
            u = np.where((gi % 2 == 0)[:, None], np.nextafter(1.0, 0.0) - u, u)
    nl = (base[:, None] + (u * size[:, None]).astype(np.int64)).astype(np.int32)
    live = rng.random((N, K)) >= p_dead
    if hub:
        t = min(300, N - 2)
        nl[(nl == t) & live] = t + 1
        pool = live & (gi == gi[t])[:, None] if hub_local else live
        slots = np.flatnonzero(pool.reshape(-1))
        nl.reshape(-1)[rng.choice(slots, hub, replace=False)] = t
        assert int(((nl == t) & live).sum()) == hub
    e = f32(rng.standard_normal((N, K, E)) * np.where(live, 1.0, 0.0)[:, :, None])
    return dict(kind="padded", F=F, E=E, K=K, N=N, span=int(np.max(span)), act=ACT[act], residual=residual, nl=nl, e=e, live=live,
                **_node_inputs(rng, N, F, E, K))


def csr_case(F, E, N, degrees, act, residual, seed, hub=0, local=0):
    """CSR lists with the given row lengths; neighbours anywhere in the batch, or with `local` inside the row's own graph of that
    many atoms; `hub` extra entries into one target"""
    rng = np.random.default_rng(seed)
    deg = np.asarray(degrees, np.int64)
    if local:
        _, base, size = graph_layout(N, local)
        col = (np.repeat(base, deg) + (rng.random(int(deg.sum())) * np.repeat(size, deg)).astype(np.int64)).astype(np.int32)
    else:
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
    return dict(kind="csr", F=F, E=E, K=K, N=N, span=local, act=ACT[act], residual=residual, nl=nl, e=ep, live=live,
                row_ptr=row_ptr, col=col, e_flat=e, rows=rows, slot=slot, **_node_inputs(rng, N, F, E, K))


def _node_inputs(rng, N, F, E, K):
    # weights scaled so that P stays O(1): activation slopes away from 0 (their float32 form is then good to a few ulp)
    return dict(h=f32(rng.standard_normal((N, F)) * 0.5), inv=f32(rng.uniform(0.05, 1.0, N)),
                w=f32(rng.standard_normal((F, F, E)) / np.sqrt(F * E * K)), dH=f32(rng.standard_normal((N, F))))


def degrees_with(rng, N, hi, must):
    d = rng.integers(0, hi + 1, N)
    d[:len(must)] = must
    return rng.permutation(d)


# ---------------------------------------------------------------------------------------------------------- exact family
# Inputs on coarse binary grids: every output of the layer is then a sum of multiples of one power of two (its granule), and
# while mag / granule stays below 2^24 every partial sum in any order is a float32 number: a kernel must give the float64
# statement bit for bit.  (h, dH in {-3..3}; e in {-2..2}/2; w in {-4..4}/8; inv_degree in {1, 1/2, 1/4, 1/8}; activation none
# or relu.)  granule: A = e h -> 1/2; P = inv A w -> 1/128; dP = dH inv -> 1/8; dw = A dP -> 1/16; dA = dP w -> 1/64; de = h dA
# -> 1/64; dh = dH + e dA -> 1/128.  The operands of the split products (A, dP, dA, B) must fit two fp16 pieces: at most 20
# significant bits (test_mp_layer_ref_host.py).
GRANULE = {"A": 2.0 ** -1, "s": 2.0 ** -7, "h_out": 2.0 ** -7, "dw": 2.0 ** -4, "de": 2.0 ** -6, "dh": 2.0 ** -7}
# incoming edges one target may have in the exact family: one edge adds at most sum_n |e_n| * mag(dA) to mag(dh), mag(dA) about
# 256 * mean|dP| * mean|w| = 60 on average and a few hundred at most (inv_degree = 1, |dP| = 3): 2^24 / 128 / (3 * 300) = 145
EXACT_HUB = 128


def exact_inputs(case, seed):
    """the case with its numbers replaced by the exact family's (lists, live slots and shape kept)"""
    assert case["act"] in (ACT["none"], ACT["relu"])
    rng = np.random.default_rng(seed)
    N, K, E, F = case["N"], case["K"], case["E"], case["F"]
    c = dict(case, family="exact")
    c["h"] = rng.integers(-3, 4, (N, F)).astype(np.float64)
    c["dH"] = rng.integers(-3, 4, (N, F)).astype(np.float64)
    c["e"] = rng.integers(-2, 3, (N, K, E)) / 2.0 * case["live"][:, :, None]
    c["w"] = rng.integers(-4, 5, (F, F, E)) / 8.0
    c["inv"] = 2.0 ** -rng.integers(0, 4, N).astype(np.float64)
    if case["kind"] == "csr":
        c["e_flat"] = c["e"][case["rows"], case["slot"]]
    return c


def sigbits(x):
    """the largest number of significant bits among the non-zero elements of x"""
    x = np.abs(np.asarray(x, np.float64)).reshape(-1)
    x = x[x > 0]
    if not x.size:
        return 0
    m, _ = np.frexp(x)
    mi = np.round(m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi                                              # lowest set bit
    return int(53 - np.log2(low.min().astype(np.float64)))


def host_records(case, permute=None):
    """csc_ptr [N + 1] and the incoming-edge records [live entries, 4] = {source row (int bits), e_0, e_1, e_2} in CSC order
    (stable by target: ascending entry id, hence ascending source), as ng_mp_edge_records writes them; `permute` (a seed)
    shuffles the records inside every target's segment — a caller-built order"""
    N, K, E = case["N"], case["K"], case["E"]
    if case["kind"] == "padded":
        eid = np.flatnonzero(case["live"].reshape(-1))
        tgt, src, ev = case["nl"].reshape(-1)[eid].astype(np.int64), eid // K, case["e"].reshape(-1, E)[eid]
    else:
        tgt, src, ev = case["col"].astype(np.int64), case["rows"], case["e_flat"]
    order = np.argsort(tgt, kind="stable")
    if permute is not None:
        key = tgt[order] + np.random.default_rng(permute).random(len(order))
        order = order[np.argsort(key, kind="stable")]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=N))]).astype(np.int32)
    rec = np.zeros((len(order), 4), np.float32)
    rec[:, 0] = src[order].astype(np.int32).view(np.float32)
    rec[:, 1:1 + min(E, 3)] = ev[order][:, :3]
    return ptr, rec


def sub_case(case, rows):
    """the padded case restricted to `rows` (whole graphs: every neighbour of a kept row is kept), lists renumbered"""
    rows = np.asarray(rows)
    nl = np.searchsorted(rows, case["nl"][rows])
    assert (rows[np.minimum(nl, len(rows) - 1)] == case["nl"][rows]).all()
    c = dict(case, N=len(rows), nl=nl.astype(np.int32))
    for k in ("e", "live", "h", "inv", "dH"):
        c[k] = case[k][rows]
    return c
