"""ng_dense_fwd / ng_dense_bwd (csrc/gemm_ops.hip) on every branch of their dispatch, against float64.

One call goes to one of five kernel families, chosen by shape and by the NG_DENSE_PATH / NG_GEMM_MATH switches:
the register-resident tall kernels (tall_gemm.hip, tall_tn.hip), the split-operand long and short GEMMs
(gemm_h2.hip), the split-operand 256 x 256 weight-gradient kernel (dw8) and the f32-input MFMA tile GEMM with its
split-K weight gradient and column sums (mfma_gemm.cuh).  Every case runs under four switch settings; the id of a
case names the branch the default setting takes.  Shapes sit on tile, chunk and grid boundaries, derived from the CU
count where the dispatch depends on it.

Two families of data:
  exact   X, dY in {-3..3}, W in {-4..4}/8, b in {-8..8}/8, activation none or relu: every partial sum is a multiple
          of 1/8 below 2^21 (an integer below 2^24 for dW), every value has at most 11 significant bits, so the fp16
          pieces and the power-of-two gradient scalings are exact.  Y, s_save, dX, dW and db must equal float64 bit
          for bit: a dropped or doubled row, column, K block or split-K chunk cannot hide.
  normal  random normal data, all four activations, residual where Kin == Nout; |got - ref| <= C mag + 1e-7 max(mag)
          per element, mag the same expression on absolute values, C = 3e-5 max(1, sqrt(n / 1024)) for a
          contraction of length n; where a split-operand GEMM runs, the RMS error stays within 8x that of the
          f32-input GEMM (NG_GEMM_MATH=fp32).  Repeated calls give the same bits, and dX = NULL / db = NULL leave the
          other gradients' bits unchanged.
Every output is pre-filled with NaN, so an entry left unwritten fails."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE, SOFTPLUS, RELU, TANH = 0, 1, 2, 3
SETTINGS = [("default", {}), ("generic", {"NG_DENSE_PATH": "generic"}), ("fp32", {"NG_GEMM_MATH": "fp32"}),
            ("both", {"NG_DENSE_PATH": "generic", "NG_GEMM_MATH": "fp32"})]
ERR_INVALID = -1


def use(monkeypatch, env):
    for k in ("NG_DENSE_PATH", "NG_GEMM_MATH"):
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def num_cu(dev):
    import torch
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def rows(spec, cu, nout):
    """row counts that sit on a boundary of the launch geometry for this CU count"""
    if isinstance(spec, int):
        return spec
    return {"trip2": 2 * cu * 64 + 1,                           # tall kernels: first tile of the persistent grid's 2nd trip
            "tile-": 128 * 128 * cu // nout,                     # dense_fwd: M Nout <= 128 128 num_cu -> 64 x 64 tiles
            "tile+": 128 * 128 * cu // nout + 1,                 #            above -> 128 x 128 / 128 x 64 tiles
            "big": 128 * 128 * cu // 64 + 1,                     # above the 64 x 64 threshold for every Nout >= 64
            # two 256-column tiles of a 128 x 256 kernel: a multiple of 8 row tiles above the short kernel's range
            # (row tiles x 2 column tiles x 2 > cu) -> the permuted (row tile, column tile) mapping; one row more -> the plain one
            "perm8": 128 * 8 * (cu // 32 + 1), "perm8+": 128 * 8 * (cu // 32 + 1) + 1}[spec]


def dw8_plan(cu, M, Kin, Nout):
    """(row chunks, rows per chunk) of dw_plan (gemm_ops.hip) for the 256 x 256 weight-gradient tiles"""
    tiles = (Kin // 256) * (Nout // 256)
    nz = max(cu // tiles, 1)
    if tiles > 1 and nz >= 16:
        nz = nz // 8 * 8
    nz = max(min(nz, max(-(-M // 32), 1)), 1)
    k_chunk = max(-(-(-(-M // nz)) // 32) * 32, 32)
    pnz = max(-(-M // k_chunk), 1)
    if tiles > 1 and nz % 8 == 0 and pnz <= nz:
        pnz = nz
    return pnz, k_chunk


# ------------------------------------------------------------------------------------------------- cases
# (id, M, Kin, Nout, flags)   flags: "h2" a split-operand GEMM runs by default, "nodb" db = NULL (Nout > 1024),
#                                    "exact" the exact family only (float64 work of the random family too large)
def _cases():
    c = []
    tall = [("tall64x64", 36, 60), ("tall128x64", 100, 4), ("tall192x64", 188, 12), ("tall192x64-full", 192, 64),
            ("tall64x64-tn2d", 4, 64),
            ("tall64x128", 4, 100),                              # dX tall (kpad 128), dW generic (Nout > 64)
            ("tall64x192-dx132", 60, 132)]                       # dX generic with a contraction of 132 = 4 (mod 8)
    for name, k, n in tall:
        for m in (1, 63, 65, "trip2", 100003):
            c.append((f"{name}-M{m}", m, k, n, ""))
    for k in (36, 64):                                           # residual (Kin == Nout) on the tall kernels
        for m in (65, "trip2"):
            c.append((f"tall-res{k}-M{m}", m, k, k, ""))
    c.append(("tall64x192-dx136-gen", 5000, 64, 136, ""))       # dX generic 128 x 64 (Kin <= 64)
    c.append(("tall128x192-dx136-gen", 5000, 72, 136, ""))      # dX generic 128 x 128 (Kin > 64)
    # split-operand, long (M >= 4096; (64,128): the tall kernels by default, the split GEMM under NG_DENSE_PATH=generic)
    for k, n in ((64, 128), (96, 384), (256, 256)):
        for m in (4095, 4096, 4097, 70001):
            c.append((f"h2long-{k}x{n}-M{m}", m, k, n, "h2"))
    # two 256-column tiles: the forward (256 x 512) and dX (512 x 256) on the (row tile, column tile) mappings of the 128 x 256
    # kernel; at 4096 / 4097 rows (32 / 33 row tiles) a 256-CU device still takes the short kernel
    for m in (4096, 4097, "perm8", "perm8+"):
        c.append((f"h2long-256x512-M{m}", m, 256, 512, "h2"))
    for m in ("perm8", "perm8+"):
        c.append((f"dw8-512x256-M{m}", m, 512, 256, "h2"))
    for m in (4097, 70001):                                     # 128-column tiles: dX split, dW on 128 x 128 tiles
        c.append((f"h2long-384x128-dw128-M{m}", m, 384, 128, "h2"))
    for k in (128, 768):                                         # split-operand, short (M >= 256, N % 256, K % 128)
        for m in (255, 256, 257, 2770):
            c.append((f"h2short-{k}x256-M{m}", m, k, 256, "h2"))
    for m in (4096, 4100):                                       # 256 x 256 dW tiles (4100: empty trailing row chunks)
        c.append((f"dw8-512x256-M{m}", m, 512, 256, "h2"))
    c.append(("dw8-512x256-M300000", 300000, 512, 256, "h2 exact"))
    # the f32-input MFMA GEMM: contraction tails, tile-choice thresholds, column-sum block cap
    c += [("gen-k8-n260", 1000, 8, 260, ""), ("gen-k24-n1028-nodb", 4097, 24, 1028, "nodb"),
          ("gen-k200-n4", 5000, 200, 4, ""), ("gen-k264-n68", 3001, 264, 68, ""), ("gen-k1000-n132", 777, 1000, 132, ""),
          ("gen-k4-n260", 2049, 4, 260, ""), ("gen-k8-n1024", 3000, 8, 1024, ""),
          ("gen64x64tile-k200-n132", "tile-", 200, 132, ""), ("gen128x128tile-k200-n132", "tile+", 200, 132, ""),
          ("gen128x64tile-k264-n64", "big", 264, 64, ""), ("gen128x128tile-k264-n68", "big", 264, 68, ""),
          ("tall-colsumcap-k8-n4", 1100000, 8, 4, "")]           # NG_DENSE_PATH=generic: colsum_kernel at 2048 blocks
    return c


CASES = _cases()


# ------------------------------------------------------------------------------------------------- GPU calls
class Dense:
    def __init__(self, dev):
        import torch
        from nmrgnn_amd import _lib
        self.torch, self.dev = torch, dev
        self.ctx = _lib.get_context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)

    def nan(self, *shape):
        return self.torch.full(shape, float("nan"), device=self.dev)

    def fwd(self, M, K, N, act, res, X, W, b, save=True):
        from nmrgnn_amd._lib import ptr
        Y = self.nan(max(M, 1), N)
        S = self.nan(max(M, 1), N) if save else None
        rc = self.lib.ng_dense_fwd(self.h, self.st, M, K, N, act, res, ptr(X), ptr(W), ptr(b), ptr(Y), ptr(S))
        return rc, Y, S

    def bwd(self, M, K, N, act, res, X, W, S, dY, dx=True, db=True):
        from nmrgnn_amd._lib import ptr
        dX = self.nan(max(M, 1), K) if dx else None
        dW, dB = self.nan(K, N), (self.nan(N) if db else None)
        rc = self.lib.ng_dense_bwd(self.h, self.st, M, K, N, act, res, ptr(X), ptr(W), ptr(S), ptr(dY), ptr(dX), ptr(dW),
                                   ptr(dB))
        return rc, dX, dW, dB

    def ok(self, rc, what):
        self.ctx.check(rc, what)


def host(t):
    return None if t is None else t.cpu().numpy()


# ------------------------------------------------------------------------------------------------- float64 statements
def act_fwd(act, x):
    if act == SOFTPLUS:
        return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
    if act == RELU:
        return np.maximum(x, 0)
    if act == TANH:
        return np.tanh(x)
    return x


def act_grad_from_out(act, s):
    if act == SOFTPLUS:
        return -np.expm1(-s)
    if act == RELU:
        return (s > 0).astype(np.float64)
    if act == TANH:
        return 1.0 - s * s
    return np.ones_like(s)


def ref_fwd(X, W, b, act, res):
    """(S, Y) and their magnitudes"""
    pre = X @ W + b
    S = act_fwd(act, pre)
    mS = np.abs(X) @ np.abs(W) + np.abs(b) + (np.abs(S) if act != NONE else 0.0)   # + the activation's own rounding
    Y, mY = (S + X, mS + np.abs(X)) if res else (S, mS)
    return S, Y, mS, mY


def ref_bwd(X, W, S32, dY, act, res):
    """(dX, dW, db) and their magnitudes; S32 = the saved activation output the kernels are handed"""
    g = act_grad_from_out(act, S32)
    dP = dY * g
    eps = 1e-2 if act in (SOFTPLUS, TANH) else 0.0           # absolute rounding of the slope recovered from s
    mP = np.abs(dY) * (np.abs(g) + eps)
    dX, mX = dP @ W.T, mP @ np.abs(W).T
    if res:
        dX, mX = dX + dY, mX + np.abs(dY)
    return dX, X.T @ dP, dP.sum(0), mX, np.abs(X).T @ mP, mP.sum(0)


def c_rel(n):
    return 3e-5 * max(1.0, np.sqrt(n / 1024.0))


def check_close(name, got, ref, mag, n):
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    top = float(mag.max()) if mag.size else 0.0
    bad = ~(err <= c_rel(n) * mag + 1e-7 * top)               # NaN fails
    if bad.any():
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries outside the bound; first at flat {k}: "
                             f"got {got.reshape(-1)[k]!r} ref {ref.reshape(-1)[k]!r} mag {mag.reshape(-1)[k]!r}")
    return float(np.sqrt(np.mean((got - ref) ** 2))) if ref.size else 0.0


def check_exact(name, got, ref):
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref), f"{name}: the reference is not exact in float32 (test data)"
    if not np.array_equal(got, ref32):                        # NaN fails
        bad = ~(got == ref32)
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries differ from float64; first at flat {k}: "
                             f"got {got.reshape(-1)[k]!r} ref {ref.reshape(-1)[k]!r}")


def exact_data(rng, M, K, N):
    X = rng.integers(-3, 4, (M, K)).astype(np.float64)
    W = rng.integers(-4, 5, (K, N)) / 8.0
    b = rng.integers(-8, 9, N) / 8.0
    dY = rng.integers(-3, 4, (M, N)).astype(np.float64)
    return X, W, b, dY


def normal_data(rng, M, K, N):
    f = lambda a: a.astype(np.float32).astype(np.float64)
    return (f(rng.standard_normal((M, K))), f(rng.standard_normal((K, N)) / np.sqrt(K)), f(0.1 * rng.standard_normal(N)),
            f(rng.standard_normal((M, N))))


# ------------------------------------------------------------------------------------------------- the case tests
@pytest.mark.parametrize("cid,Mspec,K,N,flags", CASES, ids=[c[0] for c in CASES])
def test_dense_exact_integers(gpu_device, monkeypatch, cid, Mspec, K, N, flags):
    """Y, s_save, dX, dW, db bit for bit equal to float64 under every switch setting (activations none and relu)"""
    g = Dense(gpu_device)
    M = rows(Mspec, num_cu(gpu_device), N)
    rng = np.random.default_rng([M, K, N, 1])
    X, W, b, dY = exact_data(rng, M, K, N)
    tX, tW, tb, tdY = g.up(X), g.up(W), g.up(b), g.up(dY)
    db_on = "nodb" not in flags
    for act in (NONE, RELU):
        res = int(K == N and act == RELU)
        S, Y, _, _ = ref_fwd(X, W, b, act, res)
        dX, dW, db, _, _, _ = ref_bwd(X, W, S, dY, act, res)
        tS = g.up(S)
        for sname, env in SETTINGS:
            use(monkeypatch, env)
            rc, gY, gS = g.fwd(M, K, N, act, res, tX, tW, tb)
            g.ok(rc, "ng_dense_fwd")
            rc, gdX, gdW, gdb = g.bwd(M, K, N, act, res, tX, tW, tS, tdY, db=db_on)
            g.ok(rc, "ng_dense_bwd")
            tag = f"{sname} act {act}"
            check_exact(f"Y ({tag})", host(gY), Y)
            check_exact(f"s_save ({tag})", host(gS), S)
            check_exact(f"dX ({tag})", host(gdX), dX)
            check_exact(f"dW ({tag})", host(gdW), dW)
            if db_on:
                check_exact(f"db ({tag})", host(gdb), db)


@pytest.mark.parametrize("cid,Mspec,K,N,flags", [c for c in CASES if "exact" not in c[4]],
                         ids=[c[0] for c in CASES if "exact" not in c[4]])
def test_dense_random_vs_float64(gpu_device, monkeypatch, cid, Mspec, K, N, flags):
    """element-wise bound against float64 for all four activations and every switch setting; the split-operand
    GEMMs within 8x the RMS error of the f32-input GEMM; identical bits on a repeated call, with dX = NULL (dW, db)
    and with db = NULL (dX, dW)"""
    g = Dense(gpu_device)
    M = rows(Mspec, num_cu(gpu_device), N)
    rng = np.random.default_rng([M, K, N, 2])
    X, W, b, dY = normal_data(rng, M, K, N)
    tX, tW, tb, tdY = g.up(X), g.up(W), g.up(b), g.up(dY)
    db_on = "nodb" not in flags
    for act in (NONE, SOFTPLUS, RELU, TANH):
        res = int(K == N and act in (RELU, TANH))
        S, Y, mS, mY = ref_fwd(X, W, b, act, res)
        S32 = S.astype(np.float32).astype(np.float64)
        dX, dW, db, mX, mW, mb = ref_bwd(X, W, S32, dY, act, res)
        tS = g.up(S32)
        rms = {}
        for sname, env in SETTINGS:
            use(monkeypatch, env)
            rc, gY, gS = g.fwd(M, K, N, act, res, tX, tW, tb)
            g.ok(rc, "ng_dense_fwd")
            rc, gY2, _ = g.fwd(M, K, N, act, res, tX, tW, tb, save=False)
            g.ok(rc, "ng_dense_fwd (again, no s_save)")
            rc, gdX, gdW, gdb = g.bwd(M, K, N, act, res, tX, tW, tS, tdY, db=db_on)
            g.ok(rc, "ng_dense_bwd")
            rc, gdX2, gdW2, gdb2 = g.bwd(M, K, N, act, res, tX, tW, tS, tdY, db=db_on)
            g.ok(rc, "ng_dense_bwd (again)")
            rc, _, gdW3, gdb3 = g.bwd(M, K, N, act, res, tX, tW, tS, tdY, dx=False, db=db_on)
            g.ok(rc, "ng_dense_bwd (dX = NULL)")
            rc, gdX4, gdW4, _ = g.bwd(M, K, N, act, res, tX, tW, tS, tdY, db=False)
            g.ok(rc, "ng_dense_bwd (db = NULL)")
            tag = f"{sname} act {act}"
            assert g.torch.equal(gY, gY2), f"Y: two calls differ ({tag})"
            assert g.torch.equal(gdX, gdX2) and g.torch.equal(gdW, gdW2), f"dX / dW: two calls differ ({tag})"
            assert g.torch.equal(gdW, gdW3), f"dW: dX = NULL changes its bits ({tag})"
            assert g.torch.equal(gdX, gdX4) and g.torch.equal(gdW, gdW4), f"dX / dW: db = NULL changes their bits ({tag})"
            if db_on:
                assert g.torch.equal(gdb, gdb2) and g.torch.equal(gdb, gdb3), f"db: bits differ between calls ({tag})"
            e = {"Y": check_close(f"Y ({tag})", host(gY), Y, mY, K),
                 "S": check_close(f"s_save ({tag})", host(gS), S, mS, K),
                 "dX": check_close(f"dX ({tag})", host(gdX), dX, mX, N),
                 "dW": check_close(f"dW ({tag})", host(gdW), dW, mW, M)}
            if db_on:
                e["db"] = check_close(f"db ({tag})", host(gdb), db, mb, M)
            rms[sname] = e
        if "h2" in flags:
            mags = {"Y": mY, "S": mS, "dX": mX, "dW": mW, "db": mb}
            for k, v in rms["default"].items():
                floor = 1e-9 * float(np.sqrt(np.mean(mags[k] ** 2)))
                assert v <= 8.0 * rms["fp32"][k] + floor, (k, act, v, rms["fp32"][k])


# ------------------------------------------------------------------------------------------------- M = 0
ZERO_SHAPES = [("tall", 36, 60), ("tall-dx132", 60, 132), ("h2long", 96, 384), ("h2short", 768, 256),
               ("dw8", 512, 256), ("gen", 200, 132), ("gen-nodb", 24, 1028)]


@pytest.mark.parametrize("cid,K,N", ZERO_SHAPES, ids=[s[0] for s in ZERO_SHAPES])
def test_dense_zero_rows(gpu_device, monkeypatch, cid, K, N):
    """M = 0: the forward writes nothing, dW and db become exactly 0, dX is untouched"""
    g = Dense(gpu_device)
    rng = np.random.default_rng(K + N)
    X, W, b, dY = exact_data(rng, 1, K, N)
    tX, tW, tb, tdY = g.up(X), g.up(W), g.up(b), g.up(dY)
    db_on = N <= 1024
    for sname, env in SETTINGS:
        use(monkeypatch, env)
        for act in (NONE, RELU):
            rc, gY, gS = g.fwd(0, K, N, act, 0, tX, tW, tb)
            g.ok(rc, "ng_dense_fwd (M = 0)")
            rc, gdX, gdW, gdb = g.bwd(0, K, N, act, 0, tX, tW, tdY, tdY, db=db_on)
            g.ok(rc, "ng_dense_bwd (M = 0)")
            g.torch.cuda.synchronize()
            assert g.torch.isnan(gY).all() and g.torch.isnan(gS).all(), f"forward wrote with M = 0 ({sname})"
            assert g.torch.isnan(gdX).all(), f"dX written with M = 0 ({sname})"
            assert not host(gdW).any() and not np.signbit(host(gdW)).any(), f"dW != +0 with M = 0 ({sname})"
            if db_on:
                assert not host(gdb).any() and not np.signbit(host(gdb)).any(), f"db != +0 with M = 0 ({sname})"


# ------------------------------------------------------------------------------------------------- properties
def test_dense_dw8_empty_chunks_after_stale_partials(gpu_device, monkeypatch):
    """dw8 with empty trailing row chunks right after a call whose partials were all non-zero: an empty chunk must
    write its zero partial, not leave the previous call's one in the shared workspace"""
    g = Dense(gpu_device)
    cu = num_cu(gpu_device)
    K, N = 512, 256
    nz, _ = dw8_plan(cu, 1 << 20, K, N)
    M_full, M_tail = nz * 512, max(nz * 32, 4096) + 4
    assert dw8_plan(cu, M_full, K, N) == (nz, 512)            # every chunk full
    pnz, kc = dw8_plan(cu, M_tail, K, N)
    assert (pnz - 1) * kc >= M_tail, (pnz, kc, M_tail)        # at least one trailing chunk empty
    use(monkeypatch, {})
    rng = np.random.default_rng(8)
    for M in (M_full, M_tail):
        X, W, b, dY = exact_data(rng, M, K, N)
        tX, tW, tdY = g.up(X), g.up(W), g.up(dY)
        rc, _, gdW, gdb = g.bwd(M, K, N, NONE, 0, tX, tW, None, tdY, dx=False)
        g.ok(rc, "ng_dense_bwd")
        check_exact(f"dW (M = {M})", host(gdW), X.T @ dY)
        check_exact(f"db (M = {M})", host(gdb), dY.sum(0))


DEFER_SHAPES = [("tall_tn", 5000, 36, 60), ("gen-splitk", 3000, 200, 132), ("dw128", 4097, 384, 128),
                ("dw8", 4100, 512, 256)]


@pytest.mark.parametrize("cid,M,K,N", DEFER_SHAPES, ids=[s[0] for s in DEFER_SHAPES])
def test_dense_deferred_reduction_bits(gpu_device, monkeypatch, cid, M, K, N):
    """between ng_defer_reductions(ctx, st, 1) and ng_flush_reductions, dW and db get the bits of the eager call"""
    g = Dense(gpu_device)
    rng = np.random.default_rng(M + K + N)
    X, W, b, dY = normal_data(rng, M, K, N)
    S = act_fwd(SOFTPLUS, X @ W + b).astype(np.float32)
    tX, tW, tS, tdY = g.up(X), g.up(W), g.up(S), g.up(dY)
    for sname, env in SETTINGS:
        use(monkeypatch, env)
        rc, eX, eW, eb = g.bwd(M, K, N, SOFTPLUS, 0, tX, tW, tS, tdY)
        g.ok(rc, "ng_dense_bwd (eager)")
        g.ok(g.lib.ng_defer_reductions(g.h, g.st, 1), "ng_defer_reductions")
        rc, dX, dW, db = g.bwd(M, K, N, SOFTPLUS, 0, tX, tW, tS, tdY)
        g.ok(rc, "ng_dense_bwd (deferred)")
        g.ok(g.lib.ng_flush_reductions(g.h, g.st), "ng_flush_reductions")
        g.ok(g.lib.ng_defer_reductions(g.h, g.st, 0), "ng_defer_reductions")
        assert g.torch.equal(eX, dX) and g.torch.equal(eW, dW) and g.torch.equal(eb, db), sname


NONFINITE_SHAPES = [("tall", 1000, 36, 60), ("tall-dx128", 1000, 4, 100), ("h2long", 4097, 384, 128),
                    ("h2long-fwdr", 70001, 256, 256), ("h2short", 2770, 768, 256), ("gen", 3000, 200, 132),
                    ("gen-dx64", 3000, 64, 136)]


@pytest.mark.parametrize("cid,M,K,N", NONFINITE_SHAPES, ids=[s[0] for s in NONFINITE_SHAPES])
def test_dense_nonfinite_rows_stay_in_their_rows(gpu_device, monkeypatch, cid, M, K, N):
    """an inf in one row and a NaN in another of X (dY) make exactly the float64-non-finite entries of Y (dX)
    non-finite: the range-guard fallback of the split-operand GEMMs and gemm_grad_scale's rule for inf / NaN keep the
    other rows finite and correct"""
    g = Dense(gpu_device)
    rng = np.random.default_rng(M + 3 * K + N)
    X, W, b, dY = exact_data(rng, M, K, N)
    i, j = M // 3, M - 1
    X[i, K // 2], X[j, 0] = np.inf, np.nan
    dY[i, N - 1], dY[j, N // 2] = -np.inf, np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        Y, dX = X @ W + b, dY @ W.T
    assert (~np.isfinite(Y)).sum() == 2 * N and (~np.isfinite(dX)).sum() == 2 * K
    tX, tW, tb, tdY = g.up(X), g.up(W), g.up(b), g.up(dY)
    fin_Y, fin_dX = np.isfinite(Y), np.isfinite(dX)
    for sname, env in SETTINGS:
        use(monkeypatch, env)
        rc, gY, _ = g.fwd(M, K, N, NONE, 0, tX, tW, tb, save=False)
        g.ok(rc, "ng_dense_fwd")
        rc, gdX, _, _ = g.bwd(M, K, N, NONE, 0, tX, tW, None, tdY)
        g.ok(rc, "ng_dense_bwd")
        hY, hdX = host(gY), host(gdX)
        assert np.array_equal(np.isfinite(hY), fin_Y), f"Y: non-finite pattern ({sname})"
        assert np.array_equal(np.isfinite(hdX), fin_dX), f"dX: non-finite pattern ({sname})"
        check_exact(f"Y finite rows ({sname})", np.where(fin_Y, hY, 0), np.where(fin_Y, Y, 0))
        check_exact(f"dX finite rows ({sname})", np.where(fin_dX, hdX, 0), np.where(fin_dX, dX, 0))


RANGE_SHAPES = [("h2short-fwd", 2770, 128, 256, "X"), ("h2short-dx", 2770, 768, 256, "dY"),
                ("dw8", 4100, 512, 256, "X")]


@pytest.mark.parametrize("cid,M,K,N,where", RANGE_SHAPES, ids=[s[0] for s in RANGE_SHAPES])
def test_dense_beyond_fp16_range_matches_fp32(gpu_device, monkeypatch, cid, M, K, N, where):
    """one operand of 2^17 (beyond the fp16 range) on the short and dw8 split-operand branches: every output equals
    the NG_GEMM_MATH=fp32 result bit for bit, and both equal float64 (exact data)"""
    g = Dense(gpu_device)
    rng = np.random.default_rng(M + K)
    X, W, b, dY = exact_data(rng, M, K, N)
    if where == "X":
        X[M // 2, K - 1] = 2.0 ** 17
    else:
        dY[M // 2, N - 1] = 2.0 ** 17
    tX, tW, tb, tdY = g.up(X), g.up(W), g.up(b), g.up(dY)
    ref = {"Y": X @ W + b, "dX": dY @ W.T, "dW": X.T @ dY, "db": dY.sum(0)}
    got = {}
    for sname, env in (SETTINGS[0], SETTINGS[2]):
        use(monkeypatch, env)
        rc, gY, _ = g.fwd(M, K, N, NONE, 0, tX, tW, tb, save=False)
        g.ok(rc, "ng_dense_fwd")
        rc, gdX, gdW, gdb = g.bwd(M, K, N, NONE, 0, tX, tW, None, tdY)
        g.ok(rc, "ng_dense_bwd")
        got[sname] = {"Y": host(gY), "dX": host(gdX), "dW": host(gdW), "db": host(gdb)}
        for k, r in ref.items():
            check_exact(f"{k} ({sname})", got[sname][k], r)
    for k in ref:
        assert np.array_equal(got["default"][k], got["fp32"][k]), k


def test_dense_refuses_shapes_outside_the_contract(gpu_device, monkeypatch):
    """Kin or Nout not a multiple of 4, and db with Nout > 1024: NG_ERR_INVALID, and no output written"""
    g = Dense(gpu_device)
    M = 300
    for sname, env in SETTINGS:
        use(monkeypatch, env)
        for K, N in ((6, 8), (8, 6), (66, 64), (64, 66), (130, 256), (256, 130)):
            X, W, b, dY = (g.up(a) for a in exact_data(np.random.default_rng(K * N), M, K, N))
            rc, Y, S = g.fwd(M, K, N, RELU, 0, X, W, b)
            assert rc == ERR_INVALID, ("fwd", K, N, sname, rc)
            for dx in (True, False):
                rc, dX, dW, db = g.bwd(M, K, N, NONE, 0, X, W, None, dY, dx=dx)
                assert rc == ERR_INVALID, ("bwd", K, N, dx, sname, rc)
                g.torch.cuda.synchronize()
                assert all(t is None or g.torch.isnan(t).all() for t in (Y, S, dX, dW, db)), ("written", K, N, sname)
        for K, N, m in ((64, 1028, M), (512, 1280, 4096), (8, 1028, 0)):
            X, W, b, dY = (g.up(a) for a in exact_data(np.random.default_rng(K + N), max(m, 1), K, N))
            for dx in (True, False):
                rc, dX, dW, db = g.bwd(m, K, N, NONE, 0, X, W, None, dY, dx=dx)
                assert rc == ERR_INVALID, ("bwd db", K, N, m, dx, sname, rc)
                g.torch.cuda.synchronize()
                assert all(t is None or g.torch.isnan(t).all() for t in (dX, dW, db)), ("written", K, N, m, sname)
