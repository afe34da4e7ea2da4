"""Host reference for the maximum-entropy reweighting (no GPU, no package code): a float64 NumPy statement of the formulas of
DESIGN.md §7.22, an independent damped Newton solver, and the error bound the kernel tests use.

Formulas (S [T][M] and y [M] are float32 values converted to float64 first; logw0 None = uniform = -log T):

    d_tm = S_tm - y_m        a_t = logw0_t - sum_m lam_m d_tm        logZ = log sum_t exp(a_t)        p_t = exp(a_t - logZ)
    mean_m = sum_t p_t d_tm  Gamma = logZ + theta/2 sum_m sigma_m^2 lam_m^2       grad_m = -mean_m + theta sigma_m^2 lam_m

The bound.  u = 2^-53, A = max_t (|logw0_t| + sum_m |lam_m d_tm|).  d_tm is exact in float64 (two float32 values whose
exponents differ by less than 29).  A logit is a sum of M + 1 terms: in ANY order its error is at most (M + 1) u times the sum of
the absolute terms, so |delta a_t| <= (M + 1) u A, and the same for the running maximum that is subtracted: the exponent is off
by at most 2 (M + 1) u A + u A.  exp adds a relative 2 u, a sum of T positive terms in any order at most (T - 1) u, the rescaling
of the online form at most one rounding per frame, T u, and the merge a few more.  So Z = sum exp(a_t - max) is off by a relative
(2 (M + 1) + 1) u A + (2 T + 8) u, and logZ = max + log Z by that plus u (1 + A) for the last sum and the log:

    |delta logZ|   <=  C (M + T) u (1 + A),             C = 8  (the count above stays below 4 (M + T) (1 + A) u: a factor 2 spare)
    |delta mean_m| <=  C (M + T) u (1 + A) sum_t p_t |d_tm|          (numerator and denominator are sums of the same shape)
    |delta p_t|    <=  C (M + T) u (1 + A) p_t + 4 * 2^-1074         (at an exact logZ; the floor is the spacing of subnormals)

Weighted moments over T frames (e_t = mu_t - mu_0 exact): |delta sum p e| <= C T u sum p |e|, |delta sum p e^2| <= C T u sum p e^2,
and each float32 result carries one rounding, 2^-24 relative."""
import numpy as np

U = 2.0 ** -53
C_BOUND = 8.0
SUBNORMAL = 2.0 ** -1074


def _prep(S, y, logw0):
    S = np.asarray(S, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    T = S.shape[0]
    lw = np.full(T, -np.log(float(T))) if logw0 is None else np.asarray(logw0, np.float64)
    return S - y[None, :], lw


def evaluate(S, y, lam, logw0=None):
    """dict: logZ, mean [M], p [T], a [T], dot [T], and the sizes of the bound: A, absmean [M] = sum_t p_t |d_tm|.  A plain
    two-pass log-sum-exp.  Frames with logw0 = -inf have p = 0; if every frame has, logZ = -inf, mean = 0, p = 0."""
    d, lw = _prep(S, y, logw0)
    lam = np.asarray(lam, np.float64)
    dot = d @ lam
    a = lw - dot
    finite_lw = np.where(np.isfinite(lw), np.abs(lw), 0.0)
    A = float(np.max(finite_lw + np.abs(d) @ np.abs(lam)))
    mx = np.max(a)
    if mx == -np.inf:
        z = np.zeros_like(a)
        return dict(logZ=-np.inf, mean=np.zeros(d.shape[1]), p=z, a=a, dot=dot, A=A, absmean=np.zeros(d.shape[1]))
    e = np.exp(a - mx)
    Z = e.sum()
    logZ = mx + np.log(Z)
    p = np.exp(a - logZ)
    p = np.where(a == -np.inf, 0.0, p)
    return dict(logZ=float(logZ), mean=p @ d, p=p, a=a, dot=dot, A=A, absmean=p @ np.abs(d))


def _pairwise(v):
    v = np.array(v, np.float64)
    while len(v) > 1:
        if len(v) % 2:
            v = np.concatenate([v, [0.0]])
        v = v[0::2] + v[1::2]
    return float(v[0])


def evaluate_ordered(S, y, lam, logw0=None, order="reversed", logit_dtype=np.float64):
    """(logZ, mean) with every sum taken in another order: ``reversed`` (columns and frames back to front, one running sum) or
    ``pairwise`` (a binary tree).  ``logit_dtype=np.float32`` forms the logits in float32 — what the bound must exclude."""
    d, lw = _prep(S, y, logw0)
    lam = np.asarray(lam, np.float64)
    T, M = d.shape
    if logit_dtype == np.float32:
        dot = (d.astype(np.float32) @ lam.astype(np.float32)).astype(np.float64)
        a = (lw.astype(np.float32) - dot.astype(np.float32)).astype(np.float64)
    else:
        terms = d * lam[None, :]
        if order == "reversed":
            dot = np.zeros(T)
            for m in range(M - 1, -1, -1):
                dot = dot + terms[:, m]
        else:
            dot = np.array([_pairwise(terms[t]) for t in range(T)])
        a = lw - dot
    mx = np.max(a)
    e = np.exp(a - mx)
    if order == "reversed":
        Z = 0.0
        for t in range(T - 1, -1, -1):
            Z += e[t]
        num = np.zeros(M)
        for t in range(T - 1, -1, -1):
            num = num + e[t] * d[t]
    else:
        Z = _pairwise(e)
        num = np.array([_pairwise(e * d[:, m]) for m in range(M)])
    return float(mx + np.log(Z)), num / Z


def bound_factor(T, M, A):
    return C_BOUND * (M + T) * U * (1.0 + A)


def gamma_grad(S, y, sigma, theta, lam, logw0=None):
    r = evaluate(S, y, lam, logw0)
    s2 = np.asarray(sigma, np.float64) ** 2
    lam = np.asarray(lam, np.float64)
    return r["logZ"] + 0.5 * theta * float(np.sum(s2 * lam * lam)), -r["mean"] + theta * s2 * lam


def newton(S, y, sigma, theta, logw0=None, lam0=None, tol=1e-12, max_iter=50):
    """Damped Newton on Gamma: H = Cov_p(d) + theta diag(sigma^2), Armijo backtracking (full steps at the rounding floor).
    Returns (lam, iterations, converged); converged: max |grad| <= tol * min sigma."""
    d, lw = _prep(S, y, logw0)
    sigma = np.asarray(sigma, np.float64) * np.ones(d.shape[1])
    s2 = sigma ** 2
    lam = np.zeros(d.shape[1]) if lam0 is None else np.array(lam0, np.float64)
    gtol = tol * float(sigma.min())
    for it in range(max_iter + 1):
        r = evaluate(S, y, lam, logw0)
        g = -r["mean"] + theta * s2 * lam
        if np.max(np.abs(g)) <= gtol:
            return lam, it, True
        if it == max_iter:
            break
        f = r["logZ"] + 0.5 * theta * np.sum(s2 * lam * lam)
        dc = d - r["mean"][None, :]
        H = (dc * r["p"][:, None]).T @ dc + theta * np.diag(s2)
        step = -np.linalg.solve(H, g)
        t = 1.0
        # where the predicted decrease g.step falls below the rounding of Gamma itself the Armijo test cannot see it: the
        # full Newton step is taken (the quadratic model is exact to rounding there)
        while t > 1e-12 and abs(float(g @ step)) > 64 * U * (1.0 + abs(f)):
            f_new, _ = gamma_grad(S, y, sigma, theta, lam + t * step, logw0)
            if f_new <= f + 1e-4 * t * float(g @ step):
                break
            t *= 0.5
        lam = lam + t * step
    return lam, max_iter, False


def stats(p, logw0=None):
    """(phi_eff, kish) of weights p under the log prior logw0 (None: uniform)"""
    p = np.asarray(p, np.float64)
    T = len(p)
    lw = np.full(T, -np.log(float(T))) if logw0 is None else np.asarray(logw0, np.float64)
    nz = p > 0
    ent = float(np.sum(p[nz] * (np.log(p[nz]) - lw[nz])))
    return float(np.exp(-ent)), float(1.0 / (T * np.sum(p * p)))


def chi2(mean, sigma):
    return float(np.mean((np.asarray(mean, np.float64) / np.asarray(sigma, np.float64)) ** 2))


def solve(S, y, sigma, theta, logw0=None, lam0=None, tol=1e-12):
    """the whole reference answer at theta: dict(lam, p, phi_eff, kish, chi2_prior, chi2_post, iterations, converged)"""
    lam, it, ok = newton(S, y, sigma, theta, logw0, lam0, tol)
    r = evaluate(S, y, lam, logw0)
    r0 = evaluate(S, y, np.zeros_like(lam), logw0)
    phi, kish = stats(r["p"], logw0)
    return dict(lam=lam, p=r["p"], phi_eff=phi, kish=kish, chi2_prior=chi2(r0["mean"], sigma), chi2_post=chi2(r["mean"], sigma),
                iterations=it, converged=ok)


def weighted_moments(mu, p):
    """dict: mean, var (float64, before the float32 rounding) and the sizes abs1 = sum p |e|, sq = sum p e^2, s1 = sum p e"""
    mu = np.asarray(mu, np.float32).astype(np.float64)
    p = np.asarray(p, np.float64)
    e = mu - mu[0][None, :]
    s1 = p @ e
    sq = p @ (e * e)
    return dict(mean=mu[0] + s1, var=np.maximum(0.0, sq - s1 * s1), abs1=p @ np.abs(e), sq=sq, s1=s1)


# ----------------------------------------------------------------------------------------------------------------- data
END_TO_END = ((65, 5, 0.5, 11), (300, 37, 4.0, 12))      # (T, M, theta, seed) of the fits compared with the Newton solver; sigma 0.5


def synthetic(T, M, seed):
    """the synthetic sets of the end-to-end tests: S ~ column offsets + 1.5 N(0,1), y = column mean + 0.7 N(0,1)"""
    rng = np.random.default_rng(seed)
    offsets = rng.uniform(1.0, 130.0, M)
    S = (offsets[None, :] + 1.5 * rng.standard_normal((T, M))).astype(np.float32)
    y = (S.astype(np.float64).mean(axis=0) + 0.7 * rng.standard_normal(M)).astype(np.float32)
    return S, y


def wide_case(T, M, where, seed, span=1600.0):
    """(S, y, lam) whose logits span ``span`` (> 1500: exp of a double overflows at 709) under a uniform prior, the largest
    logit in frame ``where``"""
    S, y = synthetic(T, M, seed)
    rng = np.random.default_rng(seed + 1)
    lam = rng.standard_normal(M)
    a = -((S.astype(np.float64) - y.astype(np.float64)[None, :]) @ lam)
    lam = lam * (span / float(a.max() - a.min()))
    k = int(np.argmax(a))
    S[[k, where]] = S[[where, k]]
    return S, y, lam
