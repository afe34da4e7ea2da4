"""The kernels at both ends of a training step against float64, on every branch of their dispatch: the embedding
(ng_embed_fwd / ng_embed_bwd), the output head (ng_head_fwd, ng_head_fwd_dropout, ng_head_bwd), the fused head + L2
loss + head backward (ng_head_loss_bwd / ng_head_loss_reduce) and the losses (ng_loss_l2, ng_loss_name); csrc/head_ops.hip
and csrc/node_ops.hip, reference nmrgnn/model.py:262,266-273 and losses.py:30-39.

    h0[i][f]     = sum_c a_ic Wemb[c][f]                      dWemb[c][f] = sum_i a_ic dh0_i[f]
    peaks_i      = sum_c a_ic (std_c ((x_i @ Wout)[c] + b_c) + avg_c),   x = g * mask
    dg_i[f]      = mask_if dpeaks_i sum_c a_ic std_c Wout[f][c]
    dWout[f][c]  = sum_i x_if dpeaks_i a_ic std_c             dbout[c] = sum_i dpeaks_i a_ic std_c

Each case id names the branch the default setting takes; every case also runs with NG_HEAD_PATH=generic and, for the
weight gradients, inside ng_defer_reductions(ctx, st, 1) ... ng_flush_reductions.  Row counts sit on the row-lane count,
the odd tail of the two-rows-per-trip loops and one row past each grid cap (derived from the CU count).  Fh = F / 2.

  entry point           branch (default setting)                       cases
  ng_embed_fwd          embed_fwd_rows_kernel<16/32/64>  efrows*       C <= 16, F in {64, 128, 256}
                        embed_fwd_kernel                 efgen         F in {16, 32}, C >= 17; every case under generic
                        (a non-finite Wemb row)                        test_embed_nonfinite_weight_row
  ng_embed_bwd          embed_bwd_fast_kernel<16>        ebfast        C <= 16 (F = 16 .. 256)
                        small_tn_kernel + reduce_z       ebgen         C >= 17; every case under generic
                        deferred outer job                             every case with N <= 2048, deferred setting
  ng_head_fwd(_dropout) head_fwd_fast_kernel<8/16/32>    hf8/16/32     Fh in {32, 64, 128}; mask read, drawn, none
                        head_fwd_kernel                  hfgen         Fh in {16, 48}; every case under generic
                        ng_dropout_mask + head           hfgen         the dropout call on a generic shape
  ng_head_bwd           head_bwd_fast_kernel<LPR, 16>    hb*cm16       C <= 16
                        head_bwd_fast_kernel<LPR, 32>    hb*cm32       C = 17 .. 23
                        head_bwd_dg_kernel + small_tn    hbgen         C >= 24, Fh in {16, 48}; every case under generic
                        dg only (dWout = dbout = NULL)                 every case, both families
                        deferred partials                              every fast case, deferred setting
  ng_head_loss_bwd      head_loss_kernel<LPR, DRAW>      hl*-gpw1/2    graphs of 1 .. 256 atoms, empty and unweighted
                                                                       graphs, one and two graphs per workgroup
  ng_loss_l2 / _name    loss_graph / loss_name + final   loss-G*       G in {1, 5, 257, 300}, graphs of 63 .. 200 atoms

Two families of data:
  exact   atoms in {-2..2} (half the rows one-hot), Wemb in {-8..8}/8, dh0 and g in {-4..4}/4, mask in {0, 2} (keep 0.5),
          Wout in {-4..4}/8, bout in {-8..8}/8, std in {1/2, 1, 2}, avg in {-12..480}/4, dpeaks in {-2..2}/8.  Every
          output then is a multiple of 1/8 (h0), 1/4 (dWemb), 1/64 (peaks, dWout), 1/128 (dg) or 1/16 (dbout), and the
          test asserts that the sum of the absolute values of its terms stays below 2^24 such units: every partial sum in
          any order has at most 24 significant bits, so h0, dWemb, peaks, dg, dWout and dbout must equal float64 bit for
          bit on every branch (deferred jobs included).  A dropped, doubled or misplaced row, column, element or tail
          cannot hide.
  normal  random normal features, one-hot and dense atoms, std in 0.5..40, avg in -3..120, keep 0.8;
          |got - ref| <= c(n) mag + 1e-7 max(mag) per element, mag the same expression on absolute values,
          c(n) = 3e-5 max(1, sqrt(n / 1024)) for a contraction of length n (the dense-GEMM tests' bound).
The keep-mask a head kernel draws equals ng_dropout_mask(seed, offset, keep) bit for bit (odd offsets, every LPR, row
tails, generic shapes).  Every output is pre-filled with NaN, so an entry left unwritten fails."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SETTINGS = [("default", {}, False), ("generic", {"NG_HEAD_PATH": "generic"}, False), ("deferred", {}, True)]
EW_CAP = 2048                                   # ew_grid: at most 2048 workgroups of 256 threads


def use(monkeypatch, env):
    if "NG_HEAD_PATH" in env:
        monkeypatch.setenv("NG_HEAD_PATH", env["NG_HEAD_PATH"])
    else:
        monkeypatch.delenv("NG_HEAD_PATH", raising=False)


def num_cu(dev):
    import torch
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


# ------------------------------------------------------------------------------------------------- cases
def head_rows(spec, cu, Fh):
    """row counts on a boundary of the head kernels' launch geometry (row lanes rl = 256 / LPR, LPR = Fh / 4)"""
    if isinstance(spec, int):
        return spec
    rl = 1024 // Fh
    return {"rl-1": rl - 1, "rl+1": rl + 1,
            "2rl+1": 2 * rl + 1,
            "fcap+1": cu * 8 * rl + 1,                   # head_fwd_fast: grid capped at 8 per CU, a second grid-stride pass
            "bcap+1": cu * 2 * rl + 1,                   # head_bwd_fast: 2 per CU, two rows per trip, a 1-row last block
            "bcap+odd": cu * 2 * rl + rl + 3,            #   ... last block rl + 3 rows: 3 lanes take the second row
            "ewcap+1": EW_CAP * 256 // Fh + 1}[spec]     # head_bwd_dg_kernel: second grid-stride pass


def embed_rows(spec, cu, F):
    if isinstance(spec, int):
        return spec
    rl = 1024 // F
    return {"rl-1": rl - 1, "rl+1": rl + 1, "2rl+1": 2 * rl + 1,
            "pass+1": EW_CAP * rl + 1,                   # embed_fwd_*: past the first grid pass (rows kernel: 2nd row of the trip)
            "trip2": 4 * EW_CAP * rl + 1,                # embed_fwd_rows_kernel: a second four-row trip
            "bcap+1": cu * 4 * rl + 1,                   # embed_bwd_fast: grid capped at 4 per CU, two rows per trip
            "bcap+odd": cu * 4 * rl + rl + 3}[spec]


def head_branch(Fh, C):
    lpr = Fh // 4
    fast = Fh in (32, 64, 128)
    fwd = f"hf{lpr}" if fast else "hfgen"
    bwd = f"hb{lpr}cm16" if fast and C <= 16 else f"hb{lpr}cm32" if fast and C <= 23 else "hbgen"
    return f"{fwd}-{bwd}"


def embed_branch(F, C):
    fwd = f"efrows{F // 4}" if F in (64, 128, 256) and C <= 16 else "efgen"
    return f"{fwd}-{'ebfast' if C <= 16 else 'ebgen'}"


def _head_cases():
    c = []
    add = lambda Fh, C, ns: c.extend((f"Fh{Fh}-C{C}-N{n}-{head_branch(Fh, C)}", Fh, C, n) for n in ns)
    add(32, 10, [1, 3, "rl-1", "rl+1", "2rl+1", "fcap+1", "bcap+1", "bcap+odd", 2048, 2049])
    add(32, 1, [65])
    add(32, 16, ["2rl+1"])
    add(32, 17, [3, "bcap+1", "bcap+odd"])
    add(32, 23, ["2rl+1"])
    add(32, 24, [3, "bcap+1"])
    add(32, 32, ["rl+1", 2049])
    add(64, 16, [1, "rl-1", "rl+1", "fcap+1", "bcap+odd", 2049])
    add(64, 23, [65, "bcap+odd"])
    add(64, 24, [65])
    add(64, 32, ["fcap+1"])
    add(128, 10, [1, 3, "rl-1", "rl+1", "2rl+1", "fcap+1", "bcap+1", "bcap+odd", 2048])
    add(128, 17, [9, "bcap+odd"])
    add(128, 32, [2049])
    add(16, 10, [1, 3, 2049, "ewcap+1"])
    add(16, 32, [300])
    add(48, 16, [3, 2049, "ewcap+1"])
    add(48, 24, [513])
    return c


def _embed_cases():
    c = []
    add = lambda F, C, ns: c.extend((f"F{F}-C{C}-N{n}-{embed_branch(F, C)}", F, C, n) for n in ns)
    add(64, 10, [1, 3, "rl-1", "rl+1", "2rl+1", "pass+1", "bcap+1", "bcap+odd", 2048, 2049])
    add(64, 16, ["2rl+1", "trip2"])
    add(64, 1, [65])
    add(64, 17, [3, 2049])
    add(64, 32, ["bcap+1"])
    add(128, 16, [3, "rl+1", "pass+1", "bcap+odd", 2049])
    add(128, 24, [100])
    add(256, 10, [1, "rl-1", "rl+1", "2rl+1", "bcap+1", "bcap+odd", 2048])
    add(256, 32, [5])
    add(32, 10, [1, 3, "2rl+1", "bcap+odd", "pass+1", 2049])
    add(32, 23, [77])
    add(16, 16, [3, "rl+1", "bcap+1", "bcap+odd", 2048])
    add(16, 1, [9])
    return c


HEAD_CASES = _head_cases()
EMBED_CASES = _embed_cases()


# ------------------------------------------------------------------------------------------------- GPU calls
class Gpu:
    def __init__(self, dev):
        import torch
        from nmrgnn_amd import _lib
        self.torch, self.dev = torch, dev
        self.ctx = _lib.get_context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def up(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)

    def nan(self, *shape):
        return self.torch.full(shape, float("nan"), device=self.dev)

    def ok(self, rc, what):
        self.ctx.check(rc, what)

    def run(self, defer, fn):
        """fn() between ng_defer_reductions(ctx, st, 1) and the flush when defer is set (its inputs stay alive here)"""
        if not defer:
            return fn()
        self.ok(self.lib.ng_defer_reductions(self.h, self.st, 1), "ng_defer_reductions")
        out = fn()
        self.ok(self.lib.ng_flush_reductions(self.h, self.st), "ng_flush_reductions")
        self.ok(self.lib.ng_defer_reductions(self.h, self.st, 0), "ng_defer_reductions")
        return out

    def embed_fwd(self, N, Cn, F, atoms, Wemb):
        from nmrgnn_amd._lib import ptr
        h0 = self.nan(max(N, 1), F)
        self.ok(self.lib.ng_embed_fwd(self.h, self.st, N, Cn, F, ptr(atoms), ptr(Wemb), ptr(h0)), "ng_embed_fwd")
        return h0

    def embed_bwd(self, N, Cn, F, atoms, dh0, defer=False):
        from nmrgnn_amd._lib import ptr
        dW = self.nan(Cn, F)
        self.run(defer, lambda: self.ok(self.lib.ng_embed_bwd(self.h, self.st, N, Cn, F, ptr(atoms), ptr(dh0), ptr(dW)),
                                        "ng_embed_bwd"))
        return dW

    def head_fwd(self, N, Fh, Cn, g, mask, W, b, atoms, std, avg):
        from nmrgnn_amd._lib import ptr
        pk = self.nan(max(N, 1))
        self.ok(self.lib.ng_head_fwd(self.h, self.st, N, Fh, Cn, ptr(g), ptr(mask), ptr(W), ptr(b), ptr(atoms), ptr(std),
                                     ptr(avg), ptr(pk)), "ng_head_fwd")
        return pk

    def head_fwd_dropout(self, N, Fh, Cn, g, seed, offset, keep, W, b, atoms, std, avg):
        from nmrgnn_amd._lib import ptr
        pk, m = self.nan(max(N, 1)), self.nan(max(N, 1), Fh)
        self.ok(self.lib.ng_head_fwd_dropout(self.h, self.st, N, Fh, Cn, ptr(g), seed, offset, keep, ptr(m), ptr(W), ptr(b),
                                             ptr(atoms), ptr(std), ptr(avg), ptr(pk)), "ng_head_fwd_dropout")
        return pk, m

    def head_bwd(self, N, Fh, Cn, g, mask, W, atoms, std, dp, dw=True, defer=False):
        from nmrgnn_amd._lib import ptr
        dg = self.nan(max(N, 1), Fh)
        dW, db = (self.nan(Fh, Cn), self.nan(Cn)) if dw else (None, None)
        self.run(defer, lambda: self.ok(self.lib.ng_head_bwd(self.h, self.st, N, Fh, Cn, ptr(g), ptr(mask), ptr(W), ptr(atoms),
                                                             ptr(std), ptr(dp), ptr(dg), ptr(dW), ptr(db)), "ng_head_bwd"))
        return dg, dW, db

    def dropout_mask(self, seed, offset, keep, n):
        from nmrgnn_amd._lib import ptr
        m = self.nan(max(n, 1))
        self.ok(self.lib.ng_dropout_mask(self.h, self.st, seed, offset, keep, ptr(m), n), "ng_dropout_mask")
        return m


def host(t):
    return None if t is None else t.cpu().numpy()


# ------------------------------------------------------------------------------------------------- float64 statements
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


def check_exact(name, got, ref):
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref), f"{name}: the reference is not exact in float32 (test data)"
    if not np.array_equal(got, ref32):                        # NaN fails
        bad = ~(got == ref32)
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries differ from float64; first at flat {k}: "
                             f"got {got.reshape(-1)[k]!r} ref {ref.reshape(-1)[k]!r}")


def check_range(name, mag, unit):
    """every partial sum of an output whose terms are multiples of `unit` is exact in float32"""
    top = float(mag.max()) if mag.size else 0.0
    assert top / unit < 2.0 ** 24, f"{name}: test data outside the exact range ({top / unit:.3g} units)"


def ref_embed(atoms, Wemb, dh0):
    """(h0, dWemb) and their magnitudes"""
    aa = np.abs(atoms)
    return atoms @ Wemb, atoms.T @ dh0, aa @ np.abs(Wemb), aa.T @ np.abs(dh0)


def ref_head_fwd(atoms, x, W, b, std, avg):
    """peaks and their magnitudes; x = g * mask"""
    peaks = np.sum((x @ W + b) * atoms * std + atoms * avg, axis=1)
    mag = np.sum((np.abs(x) @ np.abs(W) + np.abs(b)) * np.abs(atoms) * std + np.abs(atoms * avg), axis=1)
    return peaks, mag


def ref_head_bwd(atoms, x, mask, W, std, dp, mdp=None):
    """(dg, dWout, dbout) and their magnitudes; mdp: the magnitude of dp (|dp| when dp is exact)"""
    mdp = np.abs(dp) if mdp is None else mdp
    u, mu = (atoms * std) @ W.T, (np.abs(atoms) * std) @ np.abs(W).T
    dfull, mfull = dp[:, None] * atoms * std, mdp[:, None] * np.abs(atoms) * std
    return (mask * dp[:, None] * u, x.T @ dfull, dfull.sum(0),
            np.abs(mask) * mdp[:, None] * mu, np.abs(x).T @ mfull, mfull.sum(0))


def mixed_atoms(rng, N, Cn, dense):
    """half the rows one-hot, the other half `dense` rows"""
    a = np.asarray(dense, np.float64).copy()
    one = np.arange(N) % 2 == 0
    a[one] = 0.0
    a[np.flatnonzero(one), rng.integers(0, Cn, int(one.sum()))] = 1.0
    return a


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def head_data(rng, N, Fh, Cn, family):
    if family == "exact":
        return dict(atoms=mixed_atoms(rng, N, Cn, rng.integers(-2, 3, (N, Cn))), g=rng.integers(-4, 5, (N, Fh)) / 4.0,
                    mask=2.0 * rng.integers(0, 2, (N, Fh)), W=rng.integers(-4, 5, (Fh, Cn)) / 8.0,
                    b=rng.integers(-8, 9, Cn) / 8.0, std=2.0 ** rng.integers(-1, 2, Cn), avg=rng.integers(-12, 481, Cn) / 4.0,
                    dp=rng.integers(-2, 3, N) / 8.0)
    return dict(atoms=mixed_atoms(rng, N, Cn, f32(rng.standard_normal((N, Cn)))), g=f32(rng.standard_normal((N, Fh))),
                mask=1.25 * (rng.uniform(size=(N, Fh)) < 0.8), W=f32(rng.standard_normal((Fh, Cn)) / np.sqrt(Fh)),
                b=f32(0.1 * rng.standard_normal(Cn)), std=f32(rng.uniform(0.5, 40.0, Cn)), avg=f32(rng.uniform(-3.0, 120.0, Cn)),
                dp=f32(rng.standard_normal(N)))


# ------------------------------------------------------------------------------------------------- embedding
def _embed_case(gpu_device, monkeypatch, F, Cn, Nspec, family):
    g = Gpu(gpu_device)
    N = embed_rows(Nspec, num_cu(gpu_device), F)
    rng = np.random.default_rng([N, Cn, F, int(family == "exact")])
    if family == "exact":
        atoms = mixed_atoms(rng, N, Cn, rng.integers(-2, 3, (N, Cn)))
        Wemb, dh0 = rng.integers(-8, 9, (Cn, F)) / 8.0, rng.integers(-4, 5, (N, F)) / 4.0
    else:
        atoms = mixed_atoms(rng, N, Cn, f32(rng.standard_normal((N, Cn))))
        Wemb, dh0 = f32(rng.standard_normal((Cn, F))), f32(rng.standard_normal((N, F)))
    h0, dW, mh0, mdW = ref_embed(atoms, Wemb, dh0)
    if family == "exact":
        check_range("h0", mh0, 1 / 8)
        check_range("dWemb", mdW, 1 / 4)
    ta, tW, tdh = g.up(atoms), g.up(Wemb), g.up(dh0)
    for sname, env, defer in SETTINGS:
        use(monkeypatch, env)
        gh = g.embed_fwd(N, Cn, F, ta, tW)
        gdW = g.embed_bwd(N, Cn, F, ta, tdh, defer=defer)
        if family == "exact":
            check_exact(f"h0 ({sname})", host(gh), h0)
            check_exact(f"dWemb ({sname})", host(gdW), dW)
        else:
            check_close(f"h0 ({sname})", host(gh), h0, mh0, Cn)
            check_close(f"dWemb ({sname})", host(gdW), dW, mdW, N)


@pytest.mark.parametrize("cid,F,Cn,Nspec", EMBED_CASES, ids=[c[0] for c in EMBED_CASES])
def test_embed_exact(gpu_device, monkeypatch, cid, F, Cn, Nspec):
    """h0 and dWemb bit for bit equal to float64 under every setting (general integer atoms)"""
    _embed_case(gpu_device, monkeypatch, F, Cn, Nspec, "exact")


@pytest.mark.parametrize("cid,F,Cn,Nspec", EMBED_CASES, ids=[c[0] for c in EMBED_CASES])
def test_embed_random_vs_float64(gpu_device, monkeypatch, cid, F, Cn, Nspec):
    _embed_case(gpu_device, monkeypatch, F, Cn, Nspec, "normal")


NONFINITE_EMBED = [("efrows16", 64, 10), ("efrows64", 256, 16), ("efgen-F32", 32, 10), ("efgen-C17", 64, 17)]


@pytest.mark.parametrize("cid,F,Cn", NONFINITE_EMBED, ids=[s[0] for s in NONFINITE_EMBED])
def test_embed_nonfinite_weight_row(gpu_device, monkeypatch, cid, F, Cn):
    """a Wemb row holding inf and NaN: the dense product's result on both forward kernels — 0 * inf = NaN in every row
    whose atoms column is zero, inf where it is 1 — and exact elsewhere"""
    g = Gpu(gpu_device)
    N, c0 = 300, Cn // 2
    rng = np.random.default_rng(F + Cn)
    atoms = mixed_atoms(rng, N, Cn, rng.integers(-2, 3, (N, Cn)))
    atoms[:, c0] = 0.0
    atoms[7, :] = 0.0
    atoms[7, c0] = 1.0
    Wemb = rng.integers(-8, 9, (Cn, F)) / 8.0
    Wemb[c0, 3], Wemb[c0, F - 1], Wemb[c0, F // 2] = np.inf, -np.inf, np.nan
    with np.errstate(invalid="ignore"):
        ref = (atoms[:, :, None] * Wemb[None, :, :]).sum(1)          # term by term: IEEE 0 * inf
    assert np.isnan(ref[0, 3]) and ref[7, 3] == np.inf and np.isnan(ref[7, F // 2])
    ta, tW = g.up(atoms), g.up(Wemb)
    for sname, env, _ in SETTINGS[:2]:
        use(monkeypatch, env)
        got = host(g.embed_fwd(N, Cn, F, ta, tW))
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"NaN pattern ({sname})"
        fin = ~np.isnan(ref)
        assert np.array_equal(got[fin], ref[fin].astype(np.float32)), f"inf / finite entries ({sname})"


# ------------------------------------------------------------------------------------------------- head
def _head_case(gpu_device, monkeypatch, Fh, Cn, Nspec, family):
    g = Gpu(gpu_device)
    N = head_rows(Nspec, num_cu(gpu_device), Fh)
    rng = np.random.default_rng([N, Cn, Fh, int(family == "exact")])
    d = head_data(rng, N, Fh, Cn, family)
    exact = family == "exact"
    keep = 0.5 if exact else 0.8
    seed, offset = 1000 + N, 2 * N + 7                       # odd Philox counter offset
    t = {k: g.up(v) for k, v in d.items()}
    ones = np.ones((N, Fh))
    # the keep-mask every dropout form must draw
    mref = host(g.dropout_mask(seed, offset, keep, N * Fh)).reshape(N, Fh)
    assert np.isin(mref, [0.0, np.float32(1.0 / np.float32(keep))]).all(), "ng_dropout_mask: values"
    fwd = {"mask": ref_head_fwd(d["atoms"], d["g"] * d["mask"], d["W"], d["b"], d["std"], d["avg"]),
           "no mask": ref_head_fwd(d["atoms"], d["g"], d["W"], d["b"], d["std"], d["avg"]),
           "drawn": ref_head_fwd(d["atoms"], d["g"] * mref, d["W"], d["b"], d["std"], d["avg"])}
    bwd = {"mask": ref_head_bwd(d["atoms"], d["g"] * d["mask"], d["mask"], d["W"], d["std"], d["dp"]),
           "no mask": ref_head_bwd(d["atoms"], d["g"], ones, d["W"], d["std"], d["dp"])}
    if exact:
        for k, (_, mag) in fwd.items():
            check_range(f"peaks ({k})", mag, 1 / 64)
        for k, r in bwd.items():
            check_range(f"dg ({k})", r[3], 1 / 128)
            check_range(f"dWout ({k})", r[4], 1 / 64)
            check_range(f"dbout ({k})", r[5], 1 / 16)
    check = ((lambda name, got, ref, mag, n: check_exact(name, got, ref)) if exact else check_close)
    for sname, env, defer in SETTINGS:
        use(monkeypatch, env)
        for k, mask in (("mask", t["mask"]), ("no mask", None)):
            pk = g.head_fwd(N, Fh, Cn, t["g"], mask, t["W"], t["b"], t["atoms"], t["std"], t["avg"])
            check(f"peaks, {k} ({sname})", host(pk), fwd[k][0], fwd[k][1], Fh * Cn)
        pk, m = g.head_fwd_dropout(N, Fh, Cn, t["g"], seed, offset, keep, t["W"], t["b"], t["atoms"], t["std"], t["avg"])
        assert np.array_equal(host(m), mref.astype(np.float32)), f"drawn mask != ng_dropout_mask ({sname})"
        check(f"peaks, drawn mask ({sname})", host(pk), fwd["drawn"][0], fwd["drawn"][1], Fh * Cn)
        for k, mask in (("mask", t["mask"]), ("no mask", None)):
            dg, dW, db = g.head_bwd(N, Fh, Cn, t["g"], mask, t["W"], t["atoms"], t["std"], t["dp"], defer=defer)
            rdg, rdW, rdb, mdg, mdW, mdb = bwd[k]
            check(f"dg, {k} ({sname})", host(dg), rdg, mdg, Cn)
            check(f"dWout, {k} ({sname})", host(dW), rdW, mdW, N)
            check(f"dbout, {k} ({sname})", host(db), rdb, mdb, N)
            dg2, _, _ = g.head_bwd(N, Fh, Cn, t["g"], mask, t["W"], t["atoms"], t["std"], t["dp"], dw=False, defer=defer)
            assert g.torch.equal(dg, dg2), f"dg: dWout = dbout = NULL changes its bits, {k} ({sname})"


@pytest.mark.parametrize("cid,Fh,Cn,Nspec", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_exact(gpu_device, monkeypatch, cid, Fh, Cn, Nspec):
    """peaks (mask read, none, drawn), dg, dWout, dbout bit for bit equal to float64 under every setting; the drawn mask
    is ng_dropout_mask's; the dg-only call gives the full call's dg bits"""
    _head_case(gpu_device, monkeypatch, Fh, Cn, Nspec, "exact")


@pytest.mark.parametrize("cid,Fh,Cn,Nspec", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_random_vs_float64(gpu_device, monkeypatch, cid, Fh, Cn, Nspec):
    _head_case(gpu_device, monkeypatch, Fh, Cn, Nspec, "normal")


# ------------------------------------------------------------------------------------------------- N = 0
ZERO_SHAPES = [("hf8-hb8cm16-ebfast", 32, 10), ("hf16-hb16cm32-ebgen", 64, 17), ("hf32-hbgen-ebgen", 128, 24),
               ("hfgen-hbgen-ebgen", 48, 16)]


@pytest.mark.parametrize("cid,Fh,Cn", ZERO_SHAPES, ids=[s[0] for s in ZERO_SHAPES])
def test_zero_rows(gpu_device, monkeypatch, cid, Fh, Cn):
    """N = 0: h0, peaks, the drawn mask and dg are untouched; dWemb, dWout and dbout become +0"""
    g = Gpu(gpu_device)
    F = 2 * Fh
    d = {k: g.up(v) for k, v in head_data(np.random.default_rng(Fh + Cn), 1, Fh, Cn, "exact").items()}
    Wemb, dh0 = g.up(np.ones((Cn, F))), g.up(np.ones((1, F)))
    plus0 = lambda a: not a.any() and not np.signbit(a).any()
    for sname, env, defer in SETTINGS:
        use(monkeypatch, env)
        h0 = g.embed_fwd(0, Cn, F, d["atoms"], Wemb)
        dWe = g.embed_bwd(0, Cn, F, d["atoms"], dh0, defer=defer)
        pk = g.head_fwd(0, Fh, Cn, d["g"], d["mask"], d["W"], d["b"], d["atoms"], d["std"], d["avg"])
        pk2, m = g.head_fwd_dropout(0, Fh, Cn, d["g"], 5, 3, 0.5, d["W"], d["b"], d["atoms"], d["std"], d["avg"])
        dg, dW, db = g.head_bwd(0, Fh, Cn, d["g"], d["mask"], d["W"], d["atoms"], d["std"], d["dp"], defer=defer)
        dg2, _, _ = g.head_bwd(0, Fh, Cn, d["g"], d["mask"], d["W"], d["atoms"], d["std"], d["dp"], dw=False, defer=defer)
        g.torch.cuda.synchronize()
        for name, x in (("h0", h0), ("peaks", pk), ("peaks (dropout)", pk2), ("mask", m), ("dg", dg), ("dg (dg only)", dg2)):
            assert g.torch.isnan(x).all(), f"{name} written with N = 0 ({sname})"
        for name, x in (("dWemb", dWe), ("dWout", dW), ("dbout", db)):
            assert plus0(host(x)), f"{name} != +0 with N = 0 ({sname})"


# ------------------------------------------------------------------------------------------------- fused head + loss
def graph_sizes(spec, cu, Fh):
    """(sizes, graphs per workgroup the dispatch must choose): the graphs of one workgroup hold at most 256 atoms"""
    k = 2 if Fh == 32 else 1                            # workgroups per CU (head_loss_graphs_per_wg)
    if spec == "edges":                                 # one graph per workgroup; two trailing workgroups own only empty graphs
        return [1, 63, 64, 65, 255, 256, 0, 17, 0, 0], 1
    if spec == "full":                                  # one graph per workgroup, the whole chip
        return [(1, 63, 64, 65, 255, 256, 0, 130)[i % 8] for i in range(cu * k)], 1
    cyc = (63, 64, 65, 1, 0, 128, 30)                   # two graphs per workgroup: at most 128 atoms each
    s = [cyc[i % len(cyc)] for i in range(2 * cu * k)]
    s[-1] = s[-2] = 0                                   # the last workgroup owns two empty graphs
    return s, 2


HL_CASES = [("hl8-gpw1-C10-draw", 32, 10, "edges", 1.0, 0.5), ("hl8-gpw2-C16-gw0.5", 32, 16, "gpw2", 0.5, 1.0),
            ("hl8-gpw1-full-C1-draw", 32, 1, "full", 1.0, 0.5),
            ("hl16-gpw1-C16-gw0.5", 64, 16, "edges", 0.5, 1.0), ("hl16-gpw2-C10-draw", 64, 10, "gpw2", 1.0, 0.5),
            ("hl32-gpw1-C10-draw-gw0.5", 128, 10, "edges", 0.5, 0.5), ("hl32-gpw2-C1", 128, 1, "gpw2", 1.0, 1.0),
            ("hl32-gpw1-full-C16", 128, 16, "full", 1.0, 1.0)]


def _head_loss_case(gpu_device, monkeypatch, Fh, Cn, spec, gw, keep, family):
    from nmrgnn_amd._lib import ptr
    from oracle import nmrgnn_oracle as O
    g = Gpu(gpu_device)
    cu = num_cu(gpu_device)
    sizes, gpw = graph_sizes(spec, cu, Fh)
    G, N = len(sizes), int(sum(sizes))
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    longest = max(sizes)
    nb = g.lib.ng_head_loss_blocks(g.h, G, Fh, Cn, longest)
    assert nb == -(-G // gpw), (nb, G, gpw)
    rng = np.random.default_rng([G, N, Fh, Cn, int(family == "exact")])
    d = head_data(rng, N, Fh, Cn, family)
    if family == "exact":
        y = rng.integers(-400, 401, N) / 4.0
    else:
        y = f32(60.0 + 30.0 * rng.standard_normal(N))
    w = rng.choice([0.0, 0.5, 1.0, 2.0], N, p=[0.2, 0.3, 0.3, 0.2])
    w[gp[2]:gp[3]] = 0.0                                # a graph without a labelled atom (divide_no_nan)
    seed, offset = 77 + G, 2 * G + 1
    t = {k: g.up(v) for k, v in d.items()}
    ty, tw, tgp = g.up(y), g.up(w), g.up(gp, np.int32)
    mask = host(g.dropout_mask(seed, offset, keep, N * Fh)).reshape(N, Fh).astype(np.float64) if keep < 1 else np.ones((N, Fh))
    x = d["g"] * mask
    peaks, mp = ref_head_fwd(d["atoms"], x, d["W"], d["b"], d["std"], d["avg"])
    loss, dp = O.batch_loss_s1(y, w, peaks, gp)
    dp = dp * gw
    sw_i = np.repeat([w[a:b].sum() for a, b in zip(gp[:-1], gp[1:])], np.diff(gp))
    inv = np.divide(1.0, sw_i, out=np.zeros_like(sw_i), where=sw_i != 0)
    mdp = 2.0 * w * (np.abs(y) + mp) * inv / G * gw
    mloss = float(np.sum(w * (np.abs(y) + mp) ** 2 * inv)) / G
    rdg, rdW, rdb, mdg, mdW, mdb = ref_head_bwd(d["atoms"], x, mask, d["W"], d["std"], dp, mdp)
    n_in = max(longest, Fh * Cn)
    for sname, defer in (("default", False), ("deferred", True)):
        use(monkeypatch, {})
        pk, dg = g.nan(N), g.nan(N, Fh)
        mo = g.nan(N, Fh) if keep < 1 else None
        part = g.nan(nb, Fh * Cn + Cn + 1)
        dW, db, lo = g.nan(Fh, Cn), g.nan(Cn), g.nan(1)

        def call():
            g.ok(g.lib.ng_head_loss_bwd(g.h, g.st, N, G, Fh, Cn, longest, ptr(t["g"]), seed, offset, keep, ptr(mo),
                                        ptr(t["W"]), ptr(t["b"]), ptr(t["atoms"]), ptr(t["std"]), ptr(t["avg"]), ptr(tgp),
                                        ptr(ty), ptr(tw), gw, ptr(pk), ptr(dg), ptr(part)), "ng_head_loss_bwd")
            g.ok(g.lib.ng_head_loss_reduce(g.h, g.st, ptr(part), nb, Fh, Cn, ptr(dW), ptr(db), ptr(lo)), "ng_head_loss_reduce")
        g.run(defer, call)
        if mo is not None:
            assert np.array_equal(host(mo), mask.astype(np.float32)), f"mask_out != ng_dropout_mask ({sname})"
        if family == "exact":
            check_exact(f"peaks ({sname})", host(pk), peaks)
        else:
            check_close(f"peaks ({sname})", host(pk), peaks, mp, Fh * Cn)
        check_close(f"dg ({sname})", host(dg), rdg, mdg, n_in)
        check_close(f"dWout ({sname})", host(dW), rdW, mdW, N)
        check_close(f"dbout ({sname})", host(db), rdb, mdb, N)
        check_close(f"loss ({sname})", host(lo), np.array([loss]), np.array([mloss]), max(n_in, G))


@pytest.mark.parametrize("cid,Fh,Cn,spec,gw,keep", HL_CASES, ids=[c[0] for c in HL_CASES])
@pytest.mark.parametrize("family", ["exact", "normal"])
def test_head_loss_vs_float64(gpu_device, monkeypatch, family, cid, Fh, Cn, spec, gw, keep):
    """ng_head_loss_bwd + ng_head_loss_reduce against float64 (O.batch_loss_s1): peaks (bit for bit on exact data), dg,
    dWout, dbout and the loss; mask_out is ng_dropout_mask's; graphs of 1 .. 256 atoms, interior and trailing empty graphs,
    an unlabelled graph, a shard weight of 0.5, one and two graphs per workgroup for each LPR"""
    _head_loss_case(gpu_device, monkeypatch, Fh, Cn, spec, gw, keep, family)


# ------------------------------------------------------------------------------------------------- losses
def loss_sizes(G):
    if G == 1:
        return [65], []
    if G == 5:
        return [63, 0, 64, 200, 65], [3]
    cyc = (63, 64, 65, 200, 0, 1, 130)
    return [cyc[i % len(cyc)] for i in range(G)], list(range(2, G, 9))


@pytest.mark.parametrize("G", [1, 5, 257, 300], ids=lambda G: f"loss-G{G}")
def test_losses_vs_float64(gpu_device, G):
    """ng_loss_l2 against O.batch_loss_s1 and ng_loss_name (s = 0, 0.3, 1) against O.batch_loss_name on carbon-like
    shifts (120 +- 3): loss and dpred; graphs of several lane trips, empty and unlabelled graphs, G beyond one
    final-kernel pass"""
    from nmrgnn_amd._lib import ptr
    from oracle import nmrgnn_oracle as O
    g = Gpu(gpu_device)
    sizes, unlabelled = loss_sizes(G)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N = int(gp[-1])
    rng = np.random.default_rng(G)
    y = f32(120.0 + 3.0 * rng.standard_normal(N))
    pred = f32(y + 0.7 * rng.standard_normal(N))
    w = f32(rng.uniform(0.5, 2.0, N) * (rng.uniform(size=N) < 0.85))
    for k in unlabelled:
        w[gp[k]:gp[k + 1]] = 0.0
    ty, tw, tp, tgp = g.up(y), g.up(w), g.up(pred), g.up(gp, np.int32)
    longest = max(sizes)
    runs = [("l2", None, O.batch_loss_s1(y, w, pred, gp))] + [("name", s, O.batch_loss_name(y, w, pred, gp, s))
                                                              for s in (0.0, 0.3, 1.0)]
    for kind, s, (rl, rd) in runs:
        lo, dp = g.nan(1), g.nan(max(N, 1))
        if kind == "l2":
            rc = g.lib.ng_loss_l2(g.h, g.st, N, G, ptr(tgp), ptr(ty), ptr(tw), ptr(tp), ptr(lo), ptr(dp))
        else:
            rc = g.lib.ng_loss_name(g.h, g.st, N, G, ptr(tgp), ptr(ty), ptr(tw), ptr(tp), s, ptr(lo), ptr(dp))
        g.ok(rc, f"ng_loss_{kind}")
        tag = f"{kind} s={s}"
        check_close(f"dpred ({tag})", host(dp)[:N], rd, np.abs(rd), longest)
        check_close(f"loss ({tag})", host(lo), np.array([rl]), np.array([abs(rl)]), G)
