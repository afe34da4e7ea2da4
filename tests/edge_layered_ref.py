"""The float64 statement of the layered edge MLP (csrc/edge_ops.hip: rbf_kernel, one dense GEMM per hidden layer, edge_out_fwd_kernel /
edge_out_bwd_kernel for E <= 8, a plain GEMM + mask_rows_kernel for wider E) for any H, Le, E and all four activations, of its backward
with respect to weights and biases, the launch plans of its kernels, and the case builders of tests/test_gpu_edge_layered_kernels.py;
tests/test_edge_layered_ref_host.py checks all of it on the CPU.  NumPy only.

Statement (nmrgnn/model.py:251-261 + layers.py:137-140 + model.py:111-138):
  m = d_src > 0;  X0 = m exp(-(d_eff - centers)^2 / gap);  z_t = act(x_t W_t + b_t), x_0 = X0, x_{t+1} = z_t rounded to float32 (what
  the tape holds and the next launch reads);  e = m ? z_{Le-2} W_{Le-1} + b_{Le-1} : +0.
The backward reads the tape rounded to float32 and takes the activation's slope from the saved OUTPUT (softplus 1 - exp(-z), relu
z > 0, tanh 1 - z^2, none 1), as dense_dw / dense_dx do.

Criteria
  exact    the GPU result equals the float64 statement rounded to float32 BIT FOR BIT (same_bits); the conditions under which every
           float32 evaluation order reaches that value are asserted on the CPU for every exact case (exact_conditions)
  normal   |got - ref| <= C_REL * mag + 1e-7 * max(mag) per element; mag is the same expression on absolute values, as in
           tests/test_gpu_edge_layered.py (activation slopes bounded by 1, + |act| for the activation's own rounding), with the RBF
           magnitude R (1 + |arg|) of tests/edge_mlp_ref.py for the rounding of the exponent's argument
  rbf      ng_rbf_expand alone: |got - ref| <= C_RBF * 2^-24 * R * (1 + |arg|) + RBF_FLOOR, a COUNTED constant:

rbf_kernel computes __expf((d - mu) * (d - mu) * c), c = float(-1 / gap), and __expf(x) is the hardware exp2 of x * log2(e).  With
u = 2^-24 (half an ulp, the bound of one rounding to nearest) the relative error of the exponent's argument collects, to first order,
      d - mu              1 rounding, entering the square twice      2 u
      the square          1 rounding                                  1 u
      c itself            -1 / gap rounded to float32                 1 u
      the product with c  1 rounding                                  1 u
      log2(e)             the constant rounded to float32             1 u
      x * log2(e)         1 rounding                                  1 u
  = 7 u |arg| on the result's relative error (d exp(x) / exp(x) = dx), and the hardware exponential adds 1 ulp = 2 u of its own:
  |got - ref| <= (7 |arg| + 2) u R <= 7 u R (1 + |arg|).  C_RBF = 8 = 7 counted + 1 for the second-order terms ((1 + 7 u |arg|)^2
  with |arg| <= 88 wherever R is a normal number).  The fast exponential flushes results below float32's smallest normal number to
  zero, so RBF_FLOOR = 2^-126 is added: a result the statement puts below it may come out as 0, and one a rounding-error above it too.
No GPU result enters any of these numbers."""
import numpy as np

from edge_mlp_ref import granule, two_piece  # noqa: F401  (re-exported)
from mp_layer_ref import ACT, act_fwd, act_grad_from_out, f32

C_REL = 3e-5                    # tests/test_gpu_edge_layered.py's constant
C_RBF = 8.0                     # counted above
U = 2.0 ** -24
RBF_FLOOR = 2.0 ** -126         # float32's smallest normal number
FP16_MAX = 65504.0
MAX_E = 8                       # edge_ops.hip: widest edge_out_*_kernel
CHUNK = 1 << 18                 # rows per slice of the backward's sums (the 4.2 M-row case stays within a few hundred MB)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ launch plans
def plan(n):
    """(nb, rows) of edge_out_bwd: nb = clamp(ceil(n / 2048), 1, 2048) workgroups of rows = roundup64(ceil(n / nb)) rows each"""
    nb = max(1, min(cdiv(n, 2048), 2048))
    return nb, cdiv(cdiv(n, nb), 64) * 64


def block_ranges(n):
    """[(r0, r1)] per workgroup of edge_out_bwd_kernel; r1 <= r0 for a trailing block without rows (it still writes a zero partial)"""
    nb, rows = plan(n)
    return [(b * rows, min(b * rows + rows, n)) for b in range(nb)]


def trips(n):
    """row counts nr of every 64-row trip of edge_out_bwd_kernel, block after block"""
    out = []
    for r0, r1 in block_ranges(n):
        out += [min(64, r1 - rb) for rb in range(r0, r1, 64)]
    return out


def last_rows_of_trips(n):
    """the last row of every 64-row trip"""
    out = []
    for r0, r1 in block_ranges(n):
        out += [min(rb + 64, r1) - 1 for rb in range(r0, r1, 64)]
    return np.asarray(out, np.int64)


def ew_trips(items):
    """trips of the grid-stride loop of rbf_kernel / mask_rows_kernel / sum_partials2_kernel: ew_grid caps the grid at 2048
    workgroups of 256 threads"""
    if items <= 0:
        return 0
    grid = max(1, min(cdiv(items, 256), 2048))
    return cdiv(items, grid * 256)


def split_gemm(H, n):
    """the hidden layers' GEMMs take split fp16 operands (gemm_h2_fwd_ok with K = N = H): tall M >= 4096 at H % 128 == 0, or the
    short-operand kernel from M >= 256 at H % 256 == 0"""
    return H % 128 == 0 and (n >= 4096 or (n >= 256 and H % 256 == 0))


def branches(H, Le, E, act, n):
    """the branches of edge_ops.hip a training forward + backward of this shape takes, from the launch arithmetic alone"""
    nb, rows = plan(n)
    tr = trips(n)
    br = {f"act{act}", f"Le{Le}", f"nb{nb}", f"rows{rows}", f"nz{nb}", f"rbf_trips{ew_trips(n * (H // 4))}",
          "bwd_col2" if H > 256 else "bwd_col1", f"fwd_k{H // 16}"}
    br.add(f"out<{E}>" if E <= MAX_E else "wide")
    if E > MAX_E:
        br.add(f"mask_trips{ew_trips(n * E)}")
    br.add("fwd_wg_full" if n % 64 == 0 else f"fwd_wg_ragged{n % 64}")
    if n > 64:
        br.add("fwd_wgs>1")
    if tr and tr[-1] < 64:
        br.add(f"bwd_last_trip{tr[-1]}")
    if all(t == 64 for t in tr):
        br.add("bwd_trips_full")
    if any(r0 >= n for r0, _ in block_ranges(n)):
        br.add("bwd_empty_blocks")
    if split_gemm(H, n):
        br.add("split")
    return br


# ------------------------------------------------------------------------------------------------------------- float64 statement
def rbf(d_src, d_eff, centers, gap):
    """masked RBF rows, the exponent's argument (0 on dead rows, whose d_eff may be NaN) and the live mask"""
    live = np.asarray(d_src) > 0
    d = np.where(live, d_eff, 0.0)
    arg = -(d[:, None] - centers[None, :]) ** 2 / gap
    arg = np.where(live[:, None], arg, 0.0)
    return np.where(live[:, None], np.exp(arg), 0.0), arg, live


def ref_forward(c, mutate=None, round_tape=True):
    """float64 forward on inputs already rounded to float32: ({"x0", "z": [Le - 1], "e"}, the same keys' magnitudes).
    mutate = "reverse_tape": the wrong emulation that stores the tape layers in reversed order; round_tape = False keeps the chain in
    float64 throughout (the smooth function the difference quotients of the host test need)"""
    code, Ws, bs = c["act"], c["Ws"], c["bs"]
    R, arg, live = rbf(c["d_src"], c["d_eff"], c["centers"], c["gap"])
    x, mx = R, R * (1.0 + np.abs(arg))
    v, mg = {"x0": R, "z": []}, {"x0": mx, "z": []}
    for W, b in zip(Ws[:-1], bs[:-1]):
        z = act_fwd(code, x @ W + b)
        mx = mx @ np.abs(W) + np.abs(b) + np.abs(z)
        v["z"].append(z)
        mg["z"].append(mx)
        x = f32(z) if round_tape else z                     # the next layer reads what the tape holds
    m = live[:, None]
    v["e"] = np.where(m, x @ Ws[-1] + bs[-1], 0.0)          # a dead row is +0
    mg["e"] = np.where(m, mx @ np.abs(Ws[-1]) + np.abs(bs[-1]), 0.0)
    if mutate == "reverse_tape":
        v["z"] = v["z"][::-1]
    else:
        assert mutate is None
    return v, mg


def ref_backward(c, zs32, mz=None, mutate=None, chunk=CHUNK):
    """float64 weight / bias gradients from the float32-rounded tape zs32: ({"dW": [Le], "db": [Le], "G": [Le]}, magnitudes of dW and
    db); G[t] is the gradient at layer t's pre-activation (G[Le - 1] = m de), kept only for a single-slice call.  mz: the forward's
    magnitudes of the tape layers (ref_forward), which stand for |x| in the magnitudes as in tests/test_gpu_edge_layered.py; without
    them |tape|.  The sums over the edges run in slices of `chunk` rows.  mutate: one of the wrong emulations
      "drop_row"      the last row of every 64-row trip of edge_out_bwd_kernel is left out of dW[Le - 1] and db[Le - 1]
      "skip_col2"     the thread's second weight column (k >= 256) of dW[Le - 1] is never accumulated
      "reverse_tape"  the tape layers are read in reversed order"""
    assert mutate in (None, "drop_row", "skip_col2", "reverse_tape")
    code, Ws = c["act"], c["Ws"]
    Le, n, H = len(Ws), len(c["d_src"]), Ws[0].shape[0]
    if mutate == "reverse_tape":
        zs32 = list(zs32)[::-1]
    v = {"dW": [np.zeros(W.shape) for W in Ws], "db": [np.zeros(W.shape[1]) for W in Ws], "G": [None] * Le}
    mg = {"dW": [np.zeros(W.shape) for W in Ws], "db": [np.zeros(W.shape[1]) for W in Ws]}
    dropped = np.zeros(n, bool)
    if mutate == "drop_row":
        dropped[last_rows_of_trips(n)] = True
    for a in range(0, n, chunk):
        s = slice(a, min(a + chunk, n))
        R, arg, live = rbf(c["d_src"][s], c["d_eff"][s], c["centers"], c["gap"])
        xs = [R] + [np.asarray(z[s], np.float64) for z in zs32]
        mxs = [R * (1.0 + np.abs(arg))] + ([np.abs(x) for x in xs[1:]] if mz is None else [m[s] for m in mz])
        g = np.where(live[:, None], np.asarray(c["de"][s], np.float64), 0.0)
        gm = np.abs(g)
        for t in range(Le - 1, -1, -1):
            if t < Le - 1:
                slope = act_grad_from_out(code, xs[t + 1])
                g, gm = g * slope, gm * np.abs(slope)
            gw = g
            if t == Le - 1 and mutate == "drop_row":
                gw = np.where(dropped[s][:, None], 0.0, g)
            v["dW"][t] += xs[t].T @ gw
            v["db"][t] += gw.sum(0)
            mg["dW"][t] += mxs[t].T @ gm
            mg["db"][t] += gm.sum(0)
            if n <= chunk:
                v["G"][t] = g
            g, gm = g @ Ws[t].T, gm @ np.abs(Ws[t]).T
    if mutate == "skip_col2":
        v["dW"][Le - 1][256:] = 0.0
    return v, mg


# ------------------------------------------------------------------------------------------------------- float32 evaluations
def _rows(c, order):
    t = np.float32
    ds, dn = np.asarray(c["d_src"], t), np.asarray(c["d_eff"], t)
    return (ds, dn) if order is None else (ds[order], dn[order])


def f32_forward(c, order=None):
    """plain float32 NumPy evaluation of ref_forward (every operand and intermediate float32) with the edges taken in `order`;
    results in the caller's order"""
    t = np.float32
    ds, dn = _rows(c, order)
    x, _, live = rbf(ds, dn, c["centers"].astype(t), t(c["gap"]))
    x = x.astype(t)
    zs = []
    for W, b in zip(c["Ws"][:-1], c["bs"][:-1]):
        x = act_fwd(c["act"], x @ W.astype(t) + b.astype(t)).astype(t)
        zs.append(x)
    e = np.where(live[:, None], x @ c["Ws"][-1].astype(t) + c["bs"][-1].astype(t), t(0))
    assert e.dtype == t and all(z.dtype == t for z in zs)
    if order is not None:
        back = np.argsort(order)
        e, zs = e[back], [z[back] for z in zs]
    return {"z": zs, "e": e}


def f32_backward(c, zs32, order=None, chunk=CHUNK):
    """plain float32 NumPy evaluation of ref_backward with the sums running over the edges in `order`"""
    t = np.float32
    Ws = [W.astype(t) for W in c["Ws"]]
    Le, n = len(Ws), len(c["d_src"])
    idx = np.arange(n) if order is None else np.asarray(order)
    dW, db = [np.zeros(W.shape, t) for W in Ws], [np.zeros(W.shape[1], t) for W in Ws]
    for a in range(0, n, chunk):
        s = idx[a:a + chunk]
        R, _, live = rbf(np.asarray(c["d_src"], t)[s], np.asarray(c["d_eff"], t)[s], c["centers"].astype(t), t(c["gap"]))
        xs = [R.astype(t)] + [np.asarray(z, t)[s] for z in zs32]
        g = np.where(live[:, None], np.asarray(c["de"], t)[s], t(0))
        for l in range(Le - 1, -1, -1):
            if l < Le - 1:
                g = (g * act_grad_from_out(c["act"], xs[l + 1]).astype(t)).astype(t)
            dW[l] = dW[l] + xs[l].T @ g
            db[l] = db[l] + g.sum(0, dtype=t)
            g = g @ Ws[l].T
    assert all(a.dtype == t for a in dW + db)
    return {"dW": dW, "db": db}


def rbf_f32(d_src, d_eff, centers, gap):
    """rbf_kernel's expression rounding by rounding in NumPy float32: (d - mu)^2 * float(-1 / gap), times log2(e), then an exponential
    correctly rounded to float32 (the hardware's is within one ulp), flushed to zero below the smallest normal number"""
    t = np.float32
    live = np.asarray(d_src, t) > 0
    d = np.where(live, np.asarray(d_eff, t), t(0)).astype(t)
    a = d[:, None] - centers.astype(t)[None, :]
    x = (a * a) * t(-1.0 / float(gap))
    y = x * t(np.log2(np.e))
    assert y.dtype == t
    with np.errstate(under="ignore"):
        r = np.exp2(y.astype(np.float64)).astype(t)
    r = np.where(np.abs(r) < t(RBF_FLOOR), t(0), r)
    return np.where(live[:, None], r, t(0)).astype(t)


def rbf_bound(R, arg):
    return C_RBF * U * R * (1.0 + np.abs(arg)) + RBF_FLOOR


# -------------------------------------------------------------------------------------------------------------------- comparisons
def tensors(v):
    """(name, array) of a result dictionary, in a fixed order"""
    out = []
    for k in ("e", "z", "dW", "db"):
        if k in v:
            out += [(k, v[k])] if k == "e" else [(f"{k}{l}", a) for l, a in enumerate(v[k])]
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def check(name, got, ref, mag, c_rel=C_REL):
    """the per-element bound; returns (max |err| / max mag, max |err| / bound)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    top = float(mag.max()) if mag.size else 0.0
    bound = c_rel * mag + 1e-7 * top
    bad = ~(err <= bound)                                      # NaN fails
    if bad.any():
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries outside the bound; first at flat {k}: "
                             f"got {got.reshape(-1)[k]!r} ref {ref.reshape(-1)[k]!r} mag {mag.reshape(-1)[k]!r}")
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max()) if mag.size else 0.0
    return (float(err.max()) / top if top > 0 else 0.0), ratio


def hold(fam, got, v, mg, failures):
    """every tensor of `got` against float64 by the family's criterion; failures are appended as text.  Returns
    {tensor: (max err / max mag, max err / bound)} (normal family)"""
    errs = {}
    ref, M = dict(tensors(v)), dict(tensors(mg))
    for name, g in tensors(got):
        r = ref[name]
        if fam == "exact":
            want = r.astype(np.float32)
            if not same_bits(g, want):
                bad = np.ascontiguousarray(g, np.float32).reshape(-1).view(np.int32) != want.reshape(-1).view(np.int32)
                k = int(np.flatnonzero(bad)[0])
                failures.append(f"{name}: {int(bad.sum())} of {bad.size} elements differ from float64; first at flat {k}: "
                                f"got {np.asarray(g).reshape(-1)[k]!r} ref {want.reshape(-1)[k]!r}")
        else:
            try:
                errs[name] = check(name, g, r, M[name])
            except AssertionError as err:
                failures.append(str(err))
    return errs


# -------------------------------------------------------------------------------------------------------------------------- cases
def _seed(H, Le, E, act, n, salt):
    return [H, Le, E, act, n, salt]


def normal_case(H, Le, E, act, n, p_dead=0.3):
    """random inputs as in tests/test_gpu_edge_layered.py: d_src uniform in (0.05, 1.2), p_dead of the slots at 0, d_eff = d_src +
    0.025 noise (!= d_src), centres linspace(0, 1.2, H) with gap their spacing, Glorot-scale weights"""
    rng = np.random.default_rng(_seed(H, Le, E, act, n, 1))
    d_src = rng.uniform(0.05, 1.2, n)
    d_src[rng.random(n) < p_dead] = 0.0
    d_src = f32(d_src)
    d_eff = f32(np.where(d_src > 0, d_src + 0.025 * rng.standard_normal(n), d_src))
    centers = f32(np.linspace(0.0, 1.2, H))
    gap = float(np.float32(centers[1] - centers[0]))
    Ws = [f32(rng.standard_normal((H, H)) * (1.5 / np.sqrt(H))) for _ in range(Le - 1)]
    Ws.append(f32(rng.standard_normal((H, E)) / np.sqrt(H)))
    bs = [f32(0.1 * rng.standard_normal(H)) for _ in range(Le - 1)] + [f32(0.1 * rng.standard_normal(E))]
    return dict(family="normal", n=n, H=H, Le=Le, E=E, act=act, d_src=d_src, d_eff=d_eff, centers=centers, gap=gap, Ws=Ws, bs=bs,
                de=f32(rng.standard_normal((n, E))))


def _two_perms(rng, H, vals):
    """sum of two signed, scaled permutation matrices [H][H]: two entries per row and per column"""
    W = np.zeros((H, H))
    for _ in range(2):
        W[np.arange(H), rng.permutation(H)] += rng.choice(vals, H) * rng.choice([-1.0, 1.0], H)
    return W


def on_centres(rng, n, H, p_dead, dtype=np.float64):
    """distances on a centre of centers = 64 arange(H) with index >= 1 (gap 1: a one-hot RBF row, exp(0) = 1 and exp(-4096) = 0 in
    float32's fast exponential and in float64); p_dead of the slots dead with d_src from {0, -0.0, -1}, d_eff = NaN on half of them"""
    centers = 64.0 * np.arange(H)
    d = centers[rng.integers(1, H, n)].astype(dtype)
    dead = rng.random(n) < p_dead
    d[dead] = rng.choice(np.asarray([0.0, -0.0, -1.0], dtype), int(dead.sum()))
    d_eff = d.copy()
    d_eff[dead & (rng.random(n) < 0.5)] = np.nan
    return centers, d, d_eff


def exact_case(H, Le, E, act, n, p_dead=0.15):
    """exact family (activations none and relu).  Forward: one-hot RBF rows; hidden weights two signed permutation matrices with
    entries +-{1/2, 1}, hidden biases integers in [-2, 2]; output weights in {0, +-1/2, +-1}, output biases integers in [-4, 4].
    Backward: the tape is chosen directly — integers 1..3, about a quarter nonzero — and de integers in [-2, 2], about half zero: every
    value of the float64 statement is a short dyadic number"""
    assert act in (ACT["none"], ACT["relu"])
    rng = np.random.default_rng(_seed(H, Le, E, act, n, 2))
    centers, d_src, d_eff = on_centres(rng, n, H, p_dead)
    Ws = [_two_perms(rng, H, [0.5, 1.0]) for _ in range(Le - 1)] + [rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], (H, E))]
    bs = [rng.integers(-2, 3, H).astype(np.float64) for _ in range(Le - 1)] + [rng.integers(-4, 5, E).astype(np.float64)]
    zs32 = [rng.integers(1, 4, (n, H)) * (rng.random((n, H)) < 0.25) * 1.0 for _ in range(Le - 1)]
    de = rng.integers(-2, 3, (n, E)) * (rng.random((n, E)) < 0.6) * 1.0
    return dict(family="exact", n=n, H=H, Le=Le, E=E, act=act, d_src=d_src, d_eff=d_eff, centers=centers, gap=1.0, Ws=Ws, bs=bs,
                zs32=zs32, de=de)


BIG_N = 2048 * 2048 + 1
BIG_PERIOD = 65521              # a prime: the rows repeat out of step with the 64-row trips and the 2112-row blocks


def big_exact_case():
    """the exact backward case above the partition's cap: n = 2048^2 + 1, H = 16, Le = 2, E = 1, relu.  float32 arrays; the rows
    repeat with period BIG_PERIOD so that building them stays cheap (the reference still sums every row)"""
    H, Le, E, act, n = 16, 2, 1, ACT["relu"], BIG_N
    base = exact_case(H, Le, E, act, BIG_PERIOD)
    t = np.float32
    tile = lambda a: np.resize(np.asarray(a, t), (n,) + np.asarray(a).shape[1:])
    return dict(base, n=n, d_src=tile(base["d_src"]), d_eff=tile(base["d_eff"]), zs32=[tile(z) for z in base["zs32"]],
                de=tile(base["de"]))


def make_case(fam, H, Le, E, act, n, p_dead=None):
    if fam == "exact":
        return exact_case(H, Le, E, act, n, 0.15 if p_dead is None else p_dead)
    return normal_case(H, Le, E, act, n, 0.3 if p_dead is None else p_dead)


def is_f32(a):
    return np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), np.asarray(a, np.float64))


def pieces_ok(x):
    x = np.asarray(x, np.float64)
    return bool((np.abs(x) < FP16_MAX).all() and two_piece(x).all())


def exact_conditions(c, forward=True, order=None):
    """asserts, for an exact case, what makes `bit for bit` a fair demand:
      every float64 value is a float32 number; a float32 evaluation in the caller's and in a shuffled row order gives those bits;
      every sum of |terms|, in units of the terms' common granule, stays below 2^24 (so every partial sum of every order is an
      integer below 2^24 on that grid); where a split-operand GEMM can run, every operand is the sum of two fp16 pieces"""
    n, H, Le = c["n"], c["H"], c["Le"]
    split = H % 128 == 0                                     # stricter than split_gemm: at every n
    if order is None:
        order = np.random.default_rng(n).permutation(n)
    same = lambda a, b: np.array_equal(np.asarray(a, np.float64), b)
    if forward:
        v, _ = ref_forward(c)
        g32, g32p = f32_forward(c), f32_forward(c, order)
        assert ((v["x0"] == 0) | (v["x0"] == 1)).all() and (v["x0"].sum(1) == (c["d_src"] > 0)).all()
        x = v["x0"]
        for l in range(Le):
            W, b = c["Ws"][l], c["bs"][l]
            ref = v["z"][l] if l < Le - 1 else v["e"]
            a32, a32p = (g32["z"][l], g32p["z"][l]) if l < Le - 1 else (g32["e"], g32p["e"])
            assert is_f32(ref) and same(a32, ref) and same(a32p, ref), l
            top = (np.abs(x) @ np.abs(W) + np.abs(b)).max()
            gran = min(granule(x) * granule(W), granule(b))
            assert top / gran < 2.0 ** 24, (l, top, gran)
            if split:
                assert pieces_ok(x) and pieces_ok(W) and pieces_ok(256.0 * W), l
            x = ref
        assert not np.signbit(v["e"][c["d_src"] <= 0]).any()
    zs32 = c["zs32"]
    v, mg = ref_backward(c, zs32)
    g32, g32p = f32_backward(c, zs32), f32_backward(c, zs32, order)
    for l in range(Le):
        for key in ("dW", "db"):
            ref = v[key][l]
            assert is_f32(ref) and same(g32[key][l], ref) and same(g32p[key][l], ref), (key, l)
    if n <= CHUNK:
        R0, _, _ = rbf(c["d_src"], c["d_eff"], c["centers"], c["gap"])
        xs = [R0] + [np.asarray(z, np.float64) for z in zs32]
        for l in range(Le):
            G = v["G"][l]
            gG = granule(G)
            assert (np.abs(xs[l]).T @ np.abs(G)).max() / (granule(xs[l]) * gG) < 2.0 ** 24, ("dW", l)
            assert np.abs(G).sum(0).max() / gG < 2.0 ** 24, ("db", l)
            if l:
                assert (np.abs(G) @ np.abs(c["Ws"][l]).T).max() / (gG * granule(c["Ws"][l])) < 2.0 ** 24, ("dZ", l)
            if split:
                assert pieces_ok(G) and pieces_ok(xs[l]), l
    else:       # the big case: one-hot RBF rows, tape in 0..3, |G| <= 2 in halves
        assert mg["dW"][Le - 1].max() < 2.0 ** 24 and mg["db"][Le - 1].max() < 2.0 ** 24
        assert 2.0 * mg["dW"][0].max() < 2.0 ** 24 and 2.0 * mg["db"][0].max() < 2.0 ** 24
    return v
