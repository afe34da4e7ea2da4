"""ng_reweight_eval, ng_reweight_weights and ng_weighted_moments (csrc/reweight.hip) through the C entry points, against the
float64 reference tests/reweight_ref.py.

Tolerances are those derived in the reference's docstring (C = 8, u = 2^-53, A = max_t (|logw0_t| + sum_m |lam_m d_tm|)):

    |delta logZ| <= C (M + T) u (1 + A)        |delta mean_m| <= C (M + T) u (1 + A) sum_t p_t |d_tm|
    |delta p_t|  <= C (M + T) u (1 + A) p_t + 4 * 2^-1074      (ng_reweight_weights is given the reference's logZ)
    stats: the same factor times sum_t p_t (|dot_t| + |logZ| + 1) for sum p log(p / w0), and twice it times sum p^2
    weighted moments: C T u sum p |e| (mean), C T u (sum p e^2 + 2 |sum p e| sum p |e|) (var), plus 2^-24 of the result

Every output sits between guard values and is pre-filled with NaN; every call is made twice and must give the same bits.
Shapes keep T M <= 4e6.  Dispatch constants of csrc/reweight.hip: 4 waves per workgroup, at least 8 frames per wave before a
second workgroup is used, at most 1024 workgroups (768 / 512 for 512 < M <= 1024 / 2048: the same span rule, and a full grid
there needs T M > 4e6); chunk-count instantiations at M <= 256, 512, 1024, 2048; two passes above."""
import numpy as np
import pytest
import torch

import reweight_ref as R

pytestmark = pytest.mark.gpu

NG_ERR_INVALID = -1
GUARD = -6.02e23
WAVES, MIN_SPAN, MAX_BLOCKS = 4, 8, 1024
FULL_GRID = WAVES * MIN_SPAN * MAX_BLOCKS      # 32768 frames: every wave of the full grid owns 8


class _Lib:
    def __init__(self, dev):
        from nmrgnn_amd import _lib
        self.ctx = _lib.get_context(dev.index)
        self.dev = dev

    def st(self):
        from nmrgnn_amd._lib import _vp
        return _vp(torch.cuda.current_stream(self.dev).cuda_stream)

    def eval_raw(self, T, M, S, y, logw0, lam, out, handle=True):
        from nmrgnn_amd._lib import ptr
        return self.ctx.lib.ng_reweight_eval(self.ctx.handle if handle else None, self.st(), T, M, ptr(S), ptr(y), ptr(logw0),
                                             ptr(lam), ptr(out))

    def weights_raw(self, T, M, S, y, logw0, lam, logZ, p, stats, handle=True):
        from nmrgnn_amd._lib import ptr
        return self.ctx.lib.ng_reweight_weights(self.ctx.handle if handle else None, self.st(), T, M, ptr(S), ptr(y), ptr(logw0),
                                                ptr(lam), ptr(logZ), ptr(p), ptr(stats))

    def moments_raw(self, T, N, mu, p, mean, var, handle=True):
        from nmrgnn_amd._lib import ptr
        return self.ctx.lib.ng_weighted_moments(self.ctx.handle if handle else None, self.st(), T, N, ptr(mu), ptr(p), ptr(mean),
                                                ptr(var))

    def error(self):
        return (self.ctx.lib.ng_last_error(self.ctx.handle) or b'').decode()


@pytest.fixture(scope="module")
def L(gpu_device):
    return _Lib(gpu_device)


def _up(x, dev, dt):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dt).contiguous()


def _guarded(n, dev, dtype=torch.float64):
    buf = torch.full((n + 2,), float("nan"), dtype=dtype, device=dev)
    buf[0] = buf[-1] = GUARD
    return buf


def _eval(L, S, y, lam, logw0=None):
    """{logZ, mean} of one checked call made twice: guards intact, both calls the same bits"""
    dev = L.dev
    T, M = S.shape
    args = (_up(S, dev, torch.float32), _up(y, dev, torch.float32), _up(logw0, dev, torch.float64), _up(lam, dev, torch.float64))
    outs = []
    for _ in range(2):
        buf = _guarded(1 + M, dev)
        rc = L.eval_raw(T, M, *args, buf[1:])
        assert rc == 0, L.error()
        o = buf.cpu().numpy()
        assert o[0] == GUARD and o[-1] == GUARD
        outs.append(o[1:-1])
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def _check_eval(L, S, y, lam, logw0=None, what=""):
    T, M = S.shape
    got = _eval(L, S, y, lam, logw0)
    ref = R.evaluate(S, y, lam, logw0)
    f = R.bound_factor(T, M, ref["A"])
    assert not np.isnan(got).any(), what
    e0 = abs(got[0] - ref["logZ"])
    em = np.abs(got[1:] - ref["mean"])
    tol = f * ref["absmean"]
    worst = float(np.max(em / np.maximum(tol, 1e-300))) if M else 0.0
    print(f"reweight_eval {what} T={T} M={M}: |dlogZ| {e0:.2e} (bound {f:.2e}), mean err / bound {worst:.3f}, A {ref['A']:.3g}")
    assert e0 <= f, (what, e0, f)
    assert (em <= tol).all(), (what, worst)
    return got, ref


def _weights(L, S, y, lam, logw0, logZ):
    dev = L.dev
    T, M = S.shape
    args = (_up(S, dev, torch.float32), _up(y, dev, torch.float32), _up(logw0, dev, torch.float64), _up(lam, dev, torch.float64),
            _up(np.array([logZ]), dev, torch.float64))
    outs = []
    for _ in range(2):
        p, st = _guarded(T, dev), _guarded(2, dev)
        rc = L.weights_raw(T, M, *args, p[1:], st[1:])
        assert rc == 0, L.error()
        p, st = p.cpu().numpy(), st.cpu().numpy()
        assert p[0] == GUARD and p[-1] == GUARD and st[0] == GUARD and st[-1] == GUARD
        outs.append((p[1:-1], st[1:-1]))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    return outs[0]


def _check_weights(L, S, y, lam, logw0=None, what=""):
    T, M = S.shape
    ref = R.evaluate(S, y, lam, logw0)
    p, st = _weights(L, S, y, lam, logw0, ref["logZ"])
    f = R.bound_factor(T, M, ref["A"])
    assert not np.isnan(p).any() and not np.isnan(st).any(), what
    ep = np.abs(p - ref["p"])
    assert (ep <= f * ref["p"] + 4 * R.SUBNORMAL).all(), (what, float(np.max(ep / np.maximum(ref["p"], 1e-300))), f)
    nz = ref["p"] > 0
    lw = np.full(T, -np.log(float(T))) if logw0 is None else np.asarray(logw0, np.float64)
    ent = float(np.sum(ref["p"][nz] * (ref["a"][nz] - ref["logZ"] - lw[nz])))
    ent_size = float(np.sum(ref["p"] * (np.abs(ref["dot"]) + abs(ref["logZ"]) + 1.0)))
    sq = float(np.sum(ref["p"] ** 2))
    print(f"reweight_weights {what} T={T} M={M}: max rel p err {float(np.max(ep[nz] / ref['p'][nz])) if nz.any() else 0:.2e} "
          f"(bound {f:.2e}), entropy err {abs(st[0] - ent):.2e} (bound {f * ent_size:.2e}), sum p^2 err {abs(st[1] - sq):.2e}")
    assert abs(st[0] - ent) <= f * ent_size, what
    assert abs(st[1] - sq) <= 2 * f * sq, what
    assert abs(p.sum() - 1.0) <= f + T * R.U, what
    return p, st


def _case(T, M, seed, scale=0.3):
    S, y = R.synthetic(T, M, seed)
    lam = scale * np.random.default_rng(seed + 7).standard_normal(M) / np.sqrt(M)
    return S, y, lam


# -------------------------------------------------------------------------------------------------------- ng_reweight_eval
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65,
                               MIN_SPAN - 1, MIN_SPAN, MIN_SPAN + 1,                       # around one wave's span
                               WAVES * MIN_SPAN, WAVES * MIN_SPAN + 1])                    # the second workgroup
def test_eval_frame_counts(L, T):
    S, y, lam = _case(T, 5, 100 + T)
    _check_eval(L, S, y, lam, what="frames")
    _check_weights(L, S, y, lam, what="frames")


def test_eval_one_more_frame_than_the_full_grid(L):
    """FULL_GRID frames give every wave of the 1024 workgroups its 8; one more makes the span 9 and leaves waves empty"""
    for T in (FULL_GRID, FULL_GRID + 1):
        S, y, lam = _case(T, 3, 5)
        _check_eval(L, S, y, lam, what="full grid")
    _check_weights(L, S, y, lam, what="full grid")


@pytest.mark.parametrize("M", [1, 3, 4, 63, 64, 65, 255, 256, 257, 260, 511, 512, 513, 516, 1023, 1024, 1025, 1028, 2047,
                               2048, 2049, 2052])
def test_eval_observable_counts(L, M):
    """each side of every chunk-count instantiation (256, 512, 1024, 2048 columns), of the two-pass form (2049), and M % 4 == 0
    (16-byte loads) beside M % 4 != 0 at each"""
    T = 70
    S, y, lam = _case(T, M, 200 + M)
    _check_eval(L, S, y, lam, what="columns")
    _check_weights(L, S, y, lam, what="columns")


@pytest.mark.parametrize("M", [4100, 4099])
def test_eval_two_pass_wide(L, M):
    S, y, lam = _case(130, M, 300 + M)
    _check_eval(L, S, y, lam, what="two-pass")
    _check_weights(L, S, y, lam, what="two-pass")


def test_eval_unaligned_rows(L):
    """M % 4 == 0 but S starts 4 bytes past a 16-byte boundary: the dword path, the same numbers"""
    T, M = 40, 64
    S, y, lam = _case(T, M, 9)
    dev = L.dev
    flat = torch.zeros(T * M + 1, dtype=torch.float32, device=dev)
    flat[1:] = _up(S, dev, torch.float32).reshape(-1)
    out = _guarded(1 + M, dev)
    rc = L.eval_raw(T, M, flat[1:], _up(y, dev, torch.float32), None, _up(lam, dev, torch.float64), out[1:])
    assert rc == 0, L.error()
    ref = R.evaluate(S, y, lam)
    f = R.bound_factor(T, M, ref["A"])
    got = out.cpu().numpy()[1:-1]
    assert abs(got[0] - ref["logZ"]) <= f and (np.abs(got[1:] - ref["mean"]) <= f * ref["absmean"]).all()


@pytest.mark.parametrize("prior", ["uniform", "nonuniform"])
def test_eval_lambda_zero_gives_the_prior(L, prior):
    T, M = 97, 37
    S, y, _ = _case(T, M, 21)
    logw0 = None
    if prior == "nonuniform":
        w0 = np.random.default_rng(3).uniform(0.1, 2.0, T)
        logw0 = np.log(w0 / w0.sum())
    got, ref = _check_eval(L, S, y, np.zeros(M), logw0, what=f"lambda=0 {prior}")
    assert abs(got[0]) <= R.bound_factor(T, M, ref["A"])      # logZ = log sum w0 = 0
    p, _ = _check_weights(L, S, y, np.zeros(M), logw0, what=f"lambda=0 {prior}")
    w0 = np.full(T, 1.0 / T) if logw0 is None else np.exp(logw0)
    assert np.max(np.abs(p - w0) / w0) <= R.bound_factor(T, M, ref["A"])


SPREAD_T, SPREAD_M = 4 * WAVES * MIN_SPAN + 5, 37      # 133 frames: five workgroups, the last with one live wave


@pytest.mark.parametrize("where", ["first", "last", "last_wave"])
def test_eval_logits_spanning_1600(L, where):
    """exp of a double overflows at 709: a spread of 1600 must go through the running maximum.  The largest logit sits in the
    first frame (no later rescale), in the last frame (the last step rescales everything), or in the first frame of the last
    live wave of the last workgroup (a rescale inside a wave and at both merge levels)"""
    T, M = SPREAD_T, SPREAD_M
    span = -(-T // (-(-T // (WAVES * MIN_SPAN)) * WAVES))
    last_wave_first = ((T - 1) // span) * span
    at = {"first": 0, "last": T - 1, "last_wave": last_wave_first}[where]
    S, y, lam = R.wide_case(T, M, at, 31)
    ref = R.evaluate(S, y, lam)
    assert ref["a"].max() - ref["a"].min() > 1500 and int(np.argmax(ref["a"])) == at
    _check_eval(L, S, y, lam, what=f"spread {where}")
    _check_weights(L, S, y, lam, what=f"spread {where}")


@pytest.mark.parametrize("dead", ["frame0", "wave", "workgroup", "all"])
def test_eval_frames_of_weight_zero(L, dead):
    T, M = 3 * WAVES * MIN_SPAN + 3, 21
    S, y, lam = _case(T, M, 41)
    w0 = np.random.default_rng(5).uniform(0.5, 1.5, T)
    span = -(-T // (-(-T // (WAVES * MIN_SPAN)) * WAVES))
    if dead == "frame0":
        w0[0] = 0
    elif dead == "wave":
        w0[span:2 * span] = 0
    elif dead == "workgroup":
        w0[:WAVES * span] = 0
    with np.errstate(divide="ignore"):
        logw0 = np.log(w0 / w0.sum())
    if dead == "all":
        logw0 = np.full(T, -np.inf)
        got = _eval(L, S, y, lam, logw0)
        assert got[0] == -np.inf and (got[1:] == 0).all()
        p, st = _weights(L, S, y, lam, logw0, -np.inf)
        assert (p == 0).all() and (st == 0).all()
        return
    _check_eval(L, S, y, lam, logw0, what=f"zero weight {dead}")
    p, _ = _check_weights(L, S, y, lam, logw0, what=f"zero weight {dead}")
    assert (p[w0 == 0] == 0).all() and (p[w0 > 0] > 0).all()


def test_eval_zero_weight_with_the_largest_logit(L):
    """the frame that would dominate has weight zero and comes first: the running maximum must stay -inf over it"""
    T, M = 50, 7
    S, y, lam = R.wide_case(T, M, 0, 51, span=900.0)
    w0 = np.ones(T)
    w0[0] = 0
    with np.errstate(divide="ignore"):
        logw0 = np.log(w0 / w0.sum())
    _check_eval(L, S, y, lam, logw0, what="dead maximum")


def test_eval_refusals(L):
    dev = L.dev
    T, M = 16, 8
    S, y, lam = _case(T, M, 61)
    Sd, yd, ld = _up(S, dev, torch.float32), _up(y, dev, torch.float32), _up(lam, dev, torch.float64)
    out = torch.full((1 + M,), GUARD, dtype=torch.float64, device=dev)
    p = torch.full((T,), GUARD, dtype=torch.float64, device=dev)
    st = torch.full((2,), GUARD, dtype=torch.float64, device=dev)
    z = torch.zeros(1, dtype=torch.float64, device=dev)
    bad = [((0, M, Sd, yd, None, ld, out), "frame count"), ((2 ** 31, M, Sd, yd, None, ld, out), "frame count"),
           ((-1, M, Sd, yd, None, ld, out), "frame count"), ((T, 0, Sd, yd, None, ld, out), "observables"),
           ((T, 16385, Sd, yd, None, ld, out), "observables"), ((T, M, None, yd, None, ld, out), "required"),
           ((T, M, Sd, None, None, ld, out), "required"), ((T, M, Sd, yd, None, None, out), "required"),
           ((T, M, Sd, yd, None, ld, None), "no output")]
    for args, word in bad:
        assert L.eval_raw(*args) == NG_ERR_INVALID
        assert word in L.error(), (word, L.error())
    assert L.eval_raw(T, M, Sd, yd, None, ld, out, handle=False) == NG_ERR_INVALID
    badw = [((0, M, Sd, yd, None, ld, z, p, st), "frame count"), ((T, 16385, Sd, yd, None, ld, z, p, st), "observables"),
            ((T, M, None, yd, None, ld, z, p, st), "required"), ((T, M, Sd, yd, None, ld, None, p, st), "required"),
            ((T, M, Sd, yd, None, ld, z, None, st), "required"), ((T, M, Sd, yd, None, ld, z, p, None), "required")]
    for args, word in badw:
        assert L.weights_raw(*args) == NG_ERR_INVALID
        assert word in L.error(), (word, L.error())
    assert L.weights_raw(T, M, Sd, yd, None, ld, z, p, st, handle=False) == NG_ERR_INVALID
    torch.cuda.synchronize(dev)
    assert bool((out == GUARD).all()) and bool((p == GUARD).all()) and bool((st == GUARD).all())      # nothing was launched


# ----------------------------------------------------------------------------------------------------- ng_weighted_moments
def _moments(L, mu, p):
    dev = L.dev
    T, N = mu.shape
    mud, pd = _up(mu, dev, torch.float32), _up(p, dev, torch.float64)
    outs = []
    for _ in range(2):
        mean, var = _guarded(N, dev, torch.float32), _guarded(N, dev, torch.float32)
        rc = L.moments_raw(T, N, mud, pd, mean[1:], var[1:])
        assert rc == 0, L.error()
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        g = np.float32(GUARD)
        assert mean[0] == g and mean[-1] == g and var[0] == g and var[-1] == g
        outs.append((mean[1:-1], var[1:-1]))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    return outs[0]


@pytest.mark.parametrize("T", [1, 2, 65])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_weighted_moments(L, T, N):
    rng = np.random.default_rng([T, N])
    mu = (rng.uniform(1, 130, N)[None, :] + 0.3 * rng.standard_normal((T, N))).astype(np.float32)
    if N > 1:
        mu[:, N // 2] = mu[0, N // 2]                  # a constant column
    p = rng.uniform(0.0, 1.0, T)
    if T > 2:
        p[rng.choice(T, T // 4, replace=False)] = 0.0      # weights containing zeros
    p = p / p.sum()
    mean, var = _moments(L, mu, p)
    ref = R.weighted_moments(mu, p)
    f = R.C_BOUND * T * R.U
    tol_mean = f * ref["abs1"] + 2.0 ** -24 * np.abs(ref["mean"])
    tol_var = f * (ref["sq"] + 2 * np.abs(ref["s1"]) * ref["abs1"]) + 2.0 ** -24 * ref["var"]
    assert (np.abs(mean - ref["mean"]) <= tol_mean).all()
    assert (np.abs(var - ref["var"]) <= tol_var).all()
    if N > 1:
        assert var[N // 2] == 0.0 and mean[N // 2] == mu[0, N // 2]
    if T == 1:
        assert (var == 0).all() and (mean == mu[0]).all()


def test_weighted_moments_refusals(L):
    dev = L.dev
    mu = torch.zeros(4, 3, dtype=torch.float32, device=dev)
    p = torch.full((4,), 0.25, dtype=torch.float64, device=dev)
    mean = torch.full((3,), GUARD, dtype=torch.float32, device=dev)
    var = torch.full((3,), GUARD, dtype=torch.float32, device=dev)
    for args, word in [((0, 3, mu, p, mean, var), "frame count"), ((4, -1, mu, p, mean, var), "atom count"),
                       ((4, 3, None, p, mean, var), "required"), ((4, 3, mu, None, mean, var), "required"),
                       ((4, 3, mu, p, None, var), "required"), ((4, 3, mu, p, mean, None), "required")]:
        assert L.moments_raw(*args) == NG_ERR_INVALID
        assert word in L.error(), (word, L.error())
    assert L.moments_raw(4, 3, mu, p, mean, var, handle=False) == NG_ERR_INVALID
    assert L.moments_raw(4, 0, mu, p, mean, var) == 0          # no atoms: nothing to do
    torch.cuda.synchronize(dev)
    assert bool((mean == GUARD).all()) and bool((var == GUARD).all())
