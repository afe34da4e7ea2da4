"""Plain NumPy float64 statements of the shift-uncertainty pieces: the head with the closed-form dropout variance
(ng_head_fwd_var, csrc/head_ops.hip + csrc/node_ops.hip), the moments over replicas (ng_ensemble_moments, csrc/ensemble.hip) and
GraphBatch.replicate.  No GPU is needed to import or run this; tests/test_uncertainty_ref_host.py checks it on the CPU and
tests/test_gpu_uncertainty.py holds the kernels to it.

    delta_i = sum_f m_f g_if u_if + v_i,   u_if = sum_c a_ic std_c Wout[f][c],   v_i = sum_c a_ic (std_c b_c + avg_c)
    m_f = Bernoulli(keep) / keep independent:   E delta_i = peaks_i,   Var delta_i = (1 - keep) / keep sum_f (g_if u_if)^2"""
import numpy as np

U24 = 2.0 ** -24


def gamma(Fh, C):
    """the relative bound of the float32 variance on V-bar: C roundings in u, doubled by the square, the product and the
    square roundings, Fh additions"""
    return 2.0 * (Fh + C + 4) * U24


def head_var_ref(g, keep, Wout, bout, atoms, std, avg):
    """(peaks, var, vbar) [N] float64 from float32 inputs; ``keep`` is taken as the float32 the entry point receives.
    vbar: the same variance with |.| inside u (the scale the kernel's bound is stated on)."""
    g, Wout, bout, atoms, std, avg = (np.asarray(x, np.float32).astype(np.float64) for x in (g, Wout, bout, atoms, std, avg))
    keep = float(np.float32(keep))
    u = (atoms * std) @ Wout.T
    ua = np.abs(atoms * std) @ np.abs(Wout).T
    v = atoms @ (std * bout + avg)
    coef = (1.0 - keep) / keep
    peaks = np.sum(g * u, axis=1) + v
    return peaks, coef * np.sum((g * u) ** 2, axis=1), coef * np.sum((np.abs(g) * ua) ** 2, axis=1)


def ensemble_moments_ref(mu, v=None):
    """two-pass float64: (mean [N], unbiased variance over the S rows [N] (0 for S = 1), mean of v [N] or None)"""
    mu = np.asarray(mu, np.float32).astype(np.float64)
    S = mu.shape[0]
    mean = mu.mean(axis=0)
    var = ((mu - mean) ** 2).sum(axis=0) / (S - 1) if S > 1 else np.zeros(mu.shape[1])
    vm = None if v is None else np.asarray(v, np.float32).astype(np.float64).mean(axis=0)
    return mean, var, vm


def ensemble_moments_shifted(mu, v=None):
    """the kernel's own order in float64: sums of d_s = mu_s - mu_0 over the replicas in their order, each result rounded to
    float32 once (returned as float32)"""
    mu = np.asarray(mu, np.float32).astype(np.float64)
    S, N = mu.shape
    sd, sd2 = np.zeros(N), np.zeros(N)
    for s in range(1, S):
        d = mu[s] - mu[0]
        sd += d
        sd2 += d * d
    mean = mu[0] + sd / S
    var = np.maximum((sd2 - sd * sd / S) / (S - 1), 0.0) if S > 1 else np.zeros(N)
    vm = None
    if v is not None:
        v = np.asarray(v, np.float32).astype(np.float64)
        acc = v[0].copy()
        for s in range(1, S):
            acc += v[s]
        vm = (acc / S).astype(np.float32)
    return mean.astype(np.float32), var.astype(np.float32), vm


def replicate_ref(atoms, nlist, edges, inv, graph_ptr, S, row_ptr=None):
    """the lists of S replicas in one batch.  Padded form (row_ptr None): nlist / edges [N, K]; CSR form: nlist = col [nnz],
    edges = dist [nnz], row_ptr [N + 1].  Returns dict(atoms, nlist, edges, inv, graph_ptr, row_ptr)."""
    atoms, nlist, edges, inv = np.asarray(atoms), np.asarray(nlist).astype(np.int64), np.asarray(edges), np.asarray(inv)
    gp = np.asarray(graph_ptr, np.int64)
    N = atoms.shape[0]
    out = dict(atoms=np.concatenate([atoms] * S), edges=np.concatenate([edges] * S), inv=np.concatenate([inv] * S),
               nlist=np.concatenate([nlist + s * N for s in range(S)]).astype(np.int32),
               graph_ptr=np.concatenate([gp[:1]] + [gp[1:] + s * N for s in range(S)]).astype(np.int32), row_ptr=None)
    if row_ptr is not None:
        rp = np.asarray(row_ptr, np.int64)
        nnz = int(rp[-1])
        out["row_ptr"] = np.concatenate([rp[:-1] + s * nnz for s in range(S)] + [[S * nnz]]).astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------- data
MC_SHAPES = [(16, 5), (32, 10), (64, 16), (128, 32)]      # (Fh, C) of the Monte-Carlo check
MC_S, MC_N, MC_SEED = 4096, 48, 77


def head_data(rng, N, Fh, C, onehot=True, zero_row=None):
    """float32 inputs of the head: normal g, Wout ~ 1 / sqrt(Fh), std in 0.5 .. 40, avg in -3 .. 120 (the spread of the
    reference's peak standards); ``onehot`` rows or general floats; ``zero_row``: that atoms row is all zero"""
    g = rng.standard_normal((N, Fh)).astype(np.float32)
    W = (rng.standard_normal((Fh, C)) / np.sqrt(Fh)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    std = rng.uniform(0.5, 40.0, C).astype(np.float32)
    avg = rng.uniform(-3.0, 120.0, C).astype(np.float32)
    if onehot:
        atoms = np.eye(C, dtype=np.float32)[rng.integers(0, C, N)]
    else:
        atoms = rng.standard_normal((N, C)).astype(np.float32)
    if zero_row is not None and zero_row < N:
        atoms[zero_row] = 0.0
    return g, W, b, atoms, std, avg


def moments_data(rng, kind, S, N):
    """the replica data sets: standard normal; 120 + 1e-3 normal (the nitrogen case); constant columns"""
    if kind == "normal":
        mu = rng.standard_normal((S, N))
    elif kind == "nitrogen":
        mu = 120.0 + 1e-3 * rng.standard_normal((S, N))
    else:
        mu = np.repeat(rng.uniform(-3.0, 200.0, (1, N)), S, axis=0)
    v = rng.uniform(0.0, 2.0, (S, N))
    return mu.astype(np.float32), v.astype(np.float32)


def ulp32(x):
    """one float32 unit in the last place at |x| (float64 array in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
