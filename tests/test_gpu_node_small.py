"""The three small kernel groups of csrc/node_ops.hip against statements that do not come from the kernels: the counter RNG
(csrc/rng.cuh and ng_randn, ng_dropout_mask, ng_add_scaled, ng_add_noise, ng_add_noise_live), ng_adam_step, and the AMP
attention aggregation (ng_amp_attend, ng_amp_attend_bwd).  References: tests/node_small_ref.py (NumPy, float64 and exact
integers), itself checked on the CPU in tests/test_node_small_ref_host.py against the published Philox4x32-10 vectors, the
oracle's Adam and AMPLayer, and central differences.  Every entry point is called through the C ABI; every output is
pre-filled with NaN and, for the RNG and Adam, is longer than n: an element left unwritten or written past the end fails.

    words     element 4 q + k = word k of Philox4x32-10(counter (lo32, hi32, 0, 0) of offset + q, key (lo32, hi32) of seed)
    u01(x)    = ((x >> 8) + 1) 2^-24  in (0, 1], exact in float32
    mask      = float32(1) / keep where u01 <= keep, else 0
    normals   z = (r0 cos t0, r0 sin t0, r1 cos t1, r1 sin t1), r = sqrt(-2 ln u), t = float32(float32(2 pi) u),
              words (0, 1) for pair 0 and (2, 3) for pair 1
    Adam      g' = g gscale, m = b1 m + (1 - b1) g', v = b2 v + (1 - b2) g' g', p -= lr_t m / (sqrt(v) + eps),
              lr_t = float32(lr sqrt(1 - b2^step) / (1 - b1^step))
    attention q = h_i wq, u = wk q, s_j = inv_i <e_ij, u>, b = softmax(s), agg_i = sum_j b_j h[nl_ij];
              db_j = <dA, h[nl_ij]>, ds_j = b_j (db_j - sum_k b_k db_k), de_ij = inv_i ds_j u, du = inv_i sum_j ds_j e_ij,
              dq = wk^T du, dwk = sum_i du q^T, dwq = sum_i h_i dq^T, dh_t = sum_{nl_ij = t} b_ij dA_i + dq_t wq^T

  entry point         branch or edge                                   cases
  ng_dropout_mask     seed with a high key word, offsets 0 / 5 /       test_dropout_mask[RNG_CASES]: keep 0.5, 0.8, 1.0 and
                      2^32 - 3 (low counter word carries inside the    keep = u01 of a word of the draw (<= against <),
                      draw) / 2^40, n = 1 .. 5 (tails), 1023,          bit for bit
  ng_randn            4*256*2048 (full grid), + 5 (second grid-        test_randn[RNG_CASES]: finite, per-element bound
  ng_add_noise        stride pass and a tail)                          test_add_noise[RNG_CASES]: alpha 0.025, -1.5, 0; bound,
                                                                       and the bits of ng_randn + ng_add_scaled
  ng_add_scaled       the same n and 256*2048 + 1 (its own grid)       test_add_scaled[n]: alpha 0, 0.025, -1.5
  ng_add_noise_live   dead share 0 / 0.3 / 1, n = 5 with the tail      test_add_noise_live[LIVE_CASES]: drawn and supplied
                      slot dead and live, a second grid-stride pass    noise; entries pos does not name stay NaN
  refusals            keep = 0, 1.5; n = 0 with NULL buffers           test_rng_refusals_and_empty
  ng_adam_step        exact family: n = 1, 255, 257, 256*2048,         test_adam_exact[n, gscale]: p, m, v bit for bit
                      256*2048 + 1 (second pass), gscale 1 and 1/4
                      normal family: (b1, b2), step 1 / 2 / 1000 /     test_adam_normal[b1-b2-step]: eps, gscale, lr inside,
                      10^6, eps, gscale, lr; grid-stride size          three chained calls; test_adam_normal_grid_stride
                      g = m = v = 0; NaN gradient; step = 0; n = 0     test_adam_edges
  ng_amp_attend(_bwd) node_small_ref.AMP_CASES: N 1 .. 769 (one to     test_amp_exact[case, wq0 / wk0] (K a power of two),
                      four partial blocks), K 1 .. 64, E 1 .. 64       test_amp_normal[case], test_amp_wide[case, span 80 /
                      (E > K, E < K), F 1 .. 256 (below, on and        10^4]: agg, dh, de, dwq, dwk element by element;
                      across a 64-lane trip); random, hub, self-loop   every backward twice, bit-identical
                      and duplicate-target graphs; inv = 0 row
                      K = 0, 65; E = 0, 65; F = 0; N = 0               test_amp_refusals_and_empty

Bounds.  One float32 rounding is U = 2^-24 relative.
  ng_randn       |z - z_ref| <= c U max(r_ref, U) per element, c = max(8, 4 c_host) = 12.64: c_host = 3.160 is the largest
                 such ratio of a float32 host evaluation (NumPy log, sqrt, cos, sin) against the float64 reference over 2^20
                 draws, measured on the CPU (test_node_small_ref_host.py); the factor 4 leaves room for the device's logf / sinf /
                 cosf (about two ulp where the host gives under one) and for fused multiply-adds.  A wrong word, pair or counter
                 is an error of order 1.
  ng_add_scaled  |out - (x + alpha y)| <= 2 U (|x| + |alpha y|); alpha = 0 returns the bits of x.
  ng_add_noise   |out - (x + alpha z_ref)| <= U (2 (|x| + |alpha z_ref|) + c |alpha| r_ref).
  ng_adam_step   counted in the kernel's expressions (g' carries one rounding unless gscale = 1):
                 m within 2 U |b1 m| + 3 U |(1 - b1) g'|          (product, sum; g' scaling, product, sum)
                 v within 2 U b2 v + 5 U (1 - b2) g'^2            (g' enters twice, two products, sum: one more than a count of 4)
                 p within U |p| + 10.5 U lr_t (|b1 m| + |(1 - b1) g'|) / (sqrt(v) + eps): 3 (m) + 1 (lr_t m) + 2.5 + 1 (v under
                 the root, the root) + 1 (+ eps) + 1 (quotient) on the update, and the final difference on |p| + |update|.
                 Exact family: b1 = 1/2, b2 = 3/4, step = 1, lr = 2^-6 (lr_t = lr), eps = 0, g' = +-2^a, v = g'^2, m in Z/8,
                 p in Z/4096: every product, sum, root and quotient is exact, p, m, v equal float64 bit for bit.
  attention      exact family: integers, inv in {1/2, 1}, wq = 0 or wk = 0, so all logits are 0, b = 1/K, and every sum is
                 exact (asserted stage by stage, node_small_ref.amp_exact_in_range): agg, dh, dwq, dwk equal float64 bit
                 for bit and de is exactly 0.  Normal and wide families: |got - ref| <= (c(n) + 4 U L) mag + 1e-7 max(mag),
                 mag the same expression on absolute values, c(n) = 3e-5 max(1, sqrt(n / 1024)) for the longest contraction
                 n feeding the output, L the largest logit on absolute values of the row (agg, de), of the rows feeding a dh row,
                 or of all rows (dwq, dwk).
The e and nlist arrays carry one guard row behind the last atom (NaN and 0): a lane that reads slot K of the last atom reads
NaN, not another allocation."""
import ctypes as C
import functools

import numpy as np
import pytest

import node_small_ref as R

pytestmark = pytest.mark.gpu

U = R.U24
BIG_SEED = 0x9E3779B97F4A7C15                     # non-zero high key word
CARRY = (1 << 32) - 3                             # the low counter word carries at q = 3
NFULL = 4 * 256 * 2048                            # ew_grid: 2048 workgroups of 256 threads, four elements each
GUARD = 8                                         # elements behind n that must stay NaN

RNG_CASES = [(0, 0, 1), (77, 5, 2), (BIG_SEED, CARRY, 3), (0, 1 << 40, 4), (77, 0, 5), (BIG_SEED, 5, 1023), (0, CARRY, 1023),
             (BIG_SEED, 1 << 40, NFULL), (77, CARRY, NFULL + 5)]


def rng_id(c):
    return "seed%x-off%x-n%d" % c


# ------------------------------------------------------------------------------------------------- GPU calls
class Gpu:
    def __init__(self, dev):
        import torch
        from nmrgnn_amd import _lib
        self.torch, self.dev, self.ptr = torch, dev, _lib.ptr
        self.ctx = _lib.get_context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def up(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)

    def nan(self, *shape):
        return self.torch.full(shape, float("nan"), device=self.dev)

    def ok(self, rc, what):
        self.ctx.check(rc, what)

    # RNG: outputs of n + GUARD elements
    def randn(self, seed, offset, n):
        out = self.nan(n + GUARD)
        self.ok(self.lib.ng_randn(self.h, self.st, seed, offset, self.ptr(out), n), "ng_randn")
        return out

    def dropout(self, seed, offset, keep, n):
        out = self.nan(n + GUARD)
        self.ok(self.lib.ng_dropout_mask(self.h, self.st, seed, offset, keep, self.ptr(out), n), "ng_dropout_mask")
        return out

    def add_scaled(self, n, x, y, alpha):
        out = self.nan(n + GUARD)
        self.ok(self.lib.ng_add_scaled(self.h, self.st, n, self.ptr(x), self.ptr(y), alpha, self.ptr(out)), "ng_add_scaled")
        return out

    def add_noise(self, seed, offset, n, x, alpha):
        out = self.nan(n + GUARD)
        self.ok(self.lib.ng_add_noise(self.h, self.st, seed, offset, n, self.ptr(x), alpha, self.ptr(out)), "ng_add_noise")
        return out

    def add_noise_live(self, seed, offset, n, x, y, alpha, pos, n_out):
        out = self.nan(n_out)
        self.ok(self.lib.ng_add_noise_live(self.h, self.st, seed, offset, n, self.ptr(x), self.ptr(y), alpha, self.ptr(pos),
                                           self.ptr(out)), "ng_add_noise_live")
        return out

    def adam(self, n, p, g, m, v, lr, b1, b2, eps, step, gscale):
        return self.lib.ng_adam_step(self.h, self.st, n, self.ptr(p), self.ptr(g), self.ptr(m), self.ptr(v), lr, b1, b2, eps,
                                     step, gscale)

    # attention: d holds device tensors (amp_up)
    def amp_up(self, d, N, K, E):
        in_ptr, in_slot = R.incoming_lists(d["nlist"], N)
        t = {k: self.up(d[k]) for k in ("h", "inv", "wq", "wk", "dagg")}
        t["e"] = self.up(np.concatenate([d["e"].reshape(N, K, E), np.full((1, K, E), np.nan)]))       # guard row
        t["nlist"] = self.up(np.concatenate([d["nlist"], np.zeros((1, K))]), np.int32)
        t["in_ptr"], t["in_slot"] = self.up(in_ptr, np.int32), self.up(in_slot, np.int32)
        return t

    def amp_fwd(self, t, N, K, F, E, agg=None):
        agg = self.nan(max(N, 1), max(F, 1)) if agg is None else agg
        rc = self.lib.ng_amp_attend(self.h, self.st, N, K, F, E, self.ptr(t["h"]), self.ptr(t["nlist"]), self.ptr(t["e"]),
                                    self.ptr(t["inv"]), self.ptr(t["wq"]), self.ptr(t["wk"]), self.ptr(agg))
        return rc, agg

    def amp_bwd(self, t, N, K, F, E, shape=None):
        n_, k_, f_, e_ = shape or (max(N, 1), K, F, E)
        out = dict(dh=self.nan(n_, f_), de=self.nan(n_, k_, e_), dwq=self.nan(f_, e_), dwk=self.nan(e_, e_))
        rc = self.lib.ng_amp_attend_bwd(self.h, self.st, N, K, F, E, self.ptr(t["h"]), self.ptr(t["nlist"]), self.ptr(t["e"]),
                                        self.ptr(t["inv"]), self.ptr(t["wq"]), self.ptr(t["wk"]), self.ptr(t["in_ptr"]),
                                        self.ptr(t["in_slot"]), self.ptr(t["dagg"]), self.ptr(out["dh"]), self.ptr(out["de"]),
                                        self.ptr(out["dwq"]), self.ptr(out["dwk"]))
        return rc, out


def host(t):
    return t.cpu().numpy()


def body(out, n, what):
    """the first n elements; the guard behind them is untouched"""
    a = host(out)
    assert np.isnan(a[n:]).all(), f"{what}: written past n = {n}"
    return a[:n]


def first_bad(name, bad, *arrays):
    if bad.any():
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        vals = ", ".join(repr(np.asarray(a).reshape(-1)[k]) for a in arrays)
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries fail; first at flat {k}: {vals}")


def check_bits(name, got, ref32):
    assert got.dtype == np.float32 and ref32.dtype == np.float32
    first_bad(name, ~(got == ref32), got, ref32)                    # NaN fails


def check_exact(name, got, ref):
    ref32 = np.asarray(ref, np.float64).astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref), f"{name}: the reference is not exact in float32 (test data)"
    first_bad(name, ~(got == ref32), got, ref)


def check_within(name, got, ref, bound):
    first_bad(name, ~(np.abs(np.asarray(got, np.float64) - ref) <= bound), got, ref, bound)                    # NaN fails


# ------------------------------------------------------------------------------------------------- RNG
@functools.lru_cache(maxsize=None)
def ref_words(seed, offset, n):
    return R.draw_words(seed, offset, n)


@functools.lru_cache(maxsize=None)
def ref_normals(seed, offset, n):
    return R.randn_ref(seed, offset, n)


def data_x(n, tag=0):
    return R.f32(np.random.default_rng([n, tag]).standard_normal(n))


@pytest.mark.parametrize("case", RNG_CASES, ids=rng_id)
def test_dropout_mask(gpu_device, case):
    """the keep-mask bit for bit, at keep 0.5 / 0.8 / 1.0 and at keep = u01 of a word of this draw (that element is kept)"""
    g = Gpu(gpu_device)
    seed, offset, n = case
    w = ref_words(seed, offset, n)
    edge = float(np.float32(R.u01(w[n // 2])))
    for keep in (0.5, 0.8, 1.0, edge):
        ref = R.dropout_ref(seed, offset, keep, n)
        assert ref[n // 2] != 0 or keep != edge
        check_bits(f"mask, keep {keep!r}", body(g.dropout(seed, offset, keep, n), n, "ng_dropout_mask"), ref)
    assert (R.dropout_ref(seed, offset, 1.0, n) == 1).all()


@pytest.mark.parametrize("case", RNG_CASES, ids=rng_id)
def test_randn(gpu_device, case):
    g = Gpu(gpu_device)
    seed, offset, n = case
    z_ref, r_ref = ref_normals(seed, offset, n)
    z = body(g.randn(seed, offset, n), n, "ng_randn")
    assert np.isfinite(z).all()
    ratio = R.randn_ratio(z, z_ref, r_ref)
    print(f"ng_randn {rng_id(case)}: largest ratio {ratio.max():.3f} (bound {R.C_RANDN})")
    first_bad("ng_randn", ~(ratio <= R.C_RANDN), z, z_ref, r_ref)


@pytest.mark.parametrize("case", RNG_CASES, ids=rng_id)
def test_add_noise(gpu_device, case):
    g = Gpu(gpu_device)
    seed, offset, n = case
    z_ref, r_ref = ref_normals(seed, offset, n)
    x = data_x(n)
    tx = g.up(x)
    tz = g.randn(seed, offset, n)
    for alpha in (0.025, -1.5, 0.0):
        a = float(np.float32(alpha))
        out = g.add_noise(seed, offset, n, tx, alpha)
        got = body(out, n, "ng_add_noise")
        check_within(f"ng_add_noise, alpha {alpha}", got, x + a * z_ref,
                     U * (2 * (np.abs(x) + np.abs(a * z_ref)) + R.C_RANDN * abs(a) * r_ref))
        two = g.add_scaled(n, tx, tz, alpha)
        assert g.torch.equal(out[:n], two[:n]), f"ng_add_noise != ng_randn + ng_add_scaled, alpha {alpha}"
        if alpha == 0.0:
            check_bits("ng_add_noise, alpha 0", got, x.astype(np.float32))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 256 * 2048 + 1, NFULL, NFULL + 5])
def test_add_scaled(gpu_device, n):
    g = Gpu(gpu_device)
    x, y = data_x(n, 1), data_x(n, 2)
    tx, ty = g.up(x), g.up(y)
    for alpha in (0.0, 0.025, -1.5):
        a = float(np.float32(alpha))
        got = body(g.add_scaled(n, tx, ty, alpha), n, "ng_add_scaled")
        check_within(f"ng_add_scaled, alpha {alpha}", got, x + a * y, 2 * U * (np.abs(x) + np.abs(a * y)))
        if alpha == 0.0:
            check_bits("ng_add_scaled, alpha 0", got, x.astype(np.float32))


LIVE_CASES = [("n5-tail-dead", 77, 0, 5, "tail-dead"), ("n5-tail-live", 77, 0, 5, "tail-live"), ("n1023-dead0", BIG_SEED, 5, 1023, 0.0),
              ("n1023-dead0.3", 0, CARRY, 1023, 0.3), ("n1023-dead1", 77, 1 << 40, 1023, 1.0),
              ("stride-dead0.3", 77, CARRY, NFULL + 5, 0.3)]


@pytest.mark.parametrize("cid,seed,offset,n,dead", LIVE_CASES, ids=[c[0] for c in LIVE_CASES])
def test_add_noise_live(gpu_device, cid, seed, offset, n, dead):
    """out_c[pos[g]] = x[g] + alpha noise[g] for the live slots (pos a random injective map), drawn or supplied noise;
    every entry of out_c that pos does not name is still NaN"""
    g = Gpu(gpu_device)
    rng = np.random.default_rng([n, len(cid)])
    if isinstance(dead, str):
        live = np.array([True, False, True, True, dead == "tail-live"])
    else:
        live = rng.uniform(size=n) >= dead
    n_live, n_out = int(live.sum()), int(live.sum()) + 7
    pos = np.full(n, -1, np.int64)
    pos[live] = rng.permutation(n_out)[:n_live]                   # injective, not onto
    assert pos.max(initial=-1) < n_out and len(set(pos[live].tolist())) == n_live
    x, y = data_x(n, 3), data_x(n, 4)
    z_ref, r_ref = ref_normals(seed, offset, n)
    tx, ty, tpos = g.up(x), g.up(y), g.up(pos, np.int32)
    named = np.zeros(n_out, bool)
    named[pos[live]] = True
    alpha = 0.025
    a = float(np.float32(alpha))
    for kind, ty_, ref, bound in (("drawn", None, x + a * z_ref, U * (2 * (np.abs(x) + np.abs(a * z_ref)) + R.C_RANDN * abs(a) * r_ref)),
                                  ("supplied", ty, x + a * y, 2 * U * (np.abs(x) + np.abs(a * y)))):
        out = host(g.add_noise_live(seed, offset, n, tx, ty_, alpha, tpos, n_out))
        assert np.isnan(out[~named]).all(), f"{kind}: an entry pos does not name was written"
        check_within(f"ng_add_noise_live, {kind}", out[pos[live]], ref[live], bound[live])


def test_rng_refusals_and_empty(gpu_device):
    g = Gpu(gpu_device)
    for keep in (0.0, 1.5):
        out = g.nan(16)
        assert g.lib.ng_dropout_mask(g.h, g.st, 1, 0, keep, g.ptr(out), 16) != 0, keep
        assert g.torch.isnan(out).all(), f"keep {keep}: output written by a refused call"
    null = None
    assert g.lib.ng_randn(g.h, g.st, 1, 0, null, 0) == 0
    assert g.lib.ng_dropout_mask(g.h, g.st, 1, 0, 0.5, null, 0) == 0
    assert g.lib.ng_add_scaled(g.h, g.st, 0, null, null, 0.5, null) == 0
    assert g.lib.ng_add_noise(g.h, g.st, 1, 0, 0, null, 0.5, null) == 0
    assert g.lib.ng_add_noise_live(g.h, g.st, 1, 0, 0, null, null, 0.5, null, null) == 0
    g.torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- Adam
class AdamState:
    """p, g, m, v on the device, n + GUARD long with NaN behind n"""

    def __init__(self, g, n, p, grad, m, v):
        self.g, self.n = g, n
        pad = lambda a: g.up(np.concatenate([a, np.full(GUARD, np.nan)]))
        self.t = [pad(p), pad(grad), pad(m), pad(v)]

    def step(self, *args):
        return self.g.adam(self.n, *self.t, *args)

    def read(self):
        return [body(x, self.n, "ng_adam_step").astype(np.float64) for x in (self.t[0], self.t[2], self.t[3])]


@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("n", [1, 255, 257, 256 * 2048, 256 * 2048 + 1])
def test_adam_exact(gpu_device, n, gscale):
    g = Gpu(gpu_device)
    rng = np.random.default_rng([n, int(gscale * 4)])
    gs = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-3, 4, n)          # g gscale = +-2^a
    grad, v = gs / gscale, gs * gs
    m, p = rng.integers(-32, 33, n) / 8.0, rng.integers(-32768, 32769, n) / 4096.0
    lr, b1, b2, eps, step = 2.0 ** -6, 0.5, 0.75, 0.0, 1
    assert R.adam_constants(lr, b1, b2, step) == (lr, 0.5, 0.25)
    pr, mr, vr, _ = R.adam_ref(p, grad, m, v, lr, b1, b2, eps, step, gscale)
    assert np.array_equal(vr, v) and (n < 100 or (pr != p).any())
    s = AdamState(g, n, p, grad, m, v)
    g.ok(s.step(lr, b1, b2, eps, step, gscale), "ng_adam_step")
    gp, gm, gv = s.read()
    check_exact("p", gp.astype(np.float32), pr)
    check_exact("m", gm.astype(np.float32), mr)
    check_exact("v", gv.astype(np.float32), vr)


def adam_data(rng, n):
    return (R.f32(rng.standard_normal(n)), R.f32(rng.standard_normal(n)), R.f32(0.1 * rng.standard_normal(n)),
            R.f32((0.1 * rng.standard_normal(n)) ** 2))


def adam_chain(g, n, rng, lr, b1, b2, eps, step, gscale, tag):
    """three calls at step, step + 1, step + 2, each on the state the one before left, each held to float64 on that state"""
    p, grad, m, v = adam_data(rng, n)
    s = AdamState(g, n, p, grad, m, v)
    tiny = 2.0 ** -149
    for k in range(3):
        pr, mr, vr, mag = R.adam_ref(p, grad, m, v, lr, b1, b2, eps, step + k, gscale)
        g.ok(s.step(lr, b1, b2, eps, step + k, gscale), "ng_adam_step")
        p_in = p
        p, m, v = s.read()
        name = f"{tag}, call {k}"
        check_within(f"m ({name})", m, mr, U * (2 * mag["m1"] + 3 * mag["m2"]) + tiny)
        check_within(f"v ({name})", v, vr, U * (2 * mag["v1"] + 5 * mag["v2"]) + tiny)
        check_within(f"p ({name})", p, pr, U * (np.abs(p_in) + 10.5 * mag["upd"]) + tiny)


@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
@pytest.mark.parametrize("b1,b2", [(0.9, 0.999), (0.5, 0.75), (0.0, 0.999)])
def test_adam_normal(gpu_device, b1, b2, step):
    g = Gpu(gpu_device)
    rng = np.random.default_rng([int(1000 * b1), step])
    for eps in (1e-7, 1e-3):
        for gscale in (1.0, 1.0 / 1024, 3.7):
            for lr in (1e-3, 1e-4):
                adam_chain(g, 1031, rng, lr, b1, b2, eps, step, gscale, f"eps {eps} gscale {gscale} lr {lr}")


def test_adam_normal_grid_stride(gpu_device):
    g = Gpu(gpu_device)
    adam_chain(g, 256 * 2048 + 259, np.random.default_rng(5), 1e-3, 0.9, 0.999, 1e-7, 2, 3.7, "second pass")


def test_adam_edges(gpu_device):
    """an all-zero element keeps its p bits (no 0 / 0); a NaN gradient stays in its element; step = 0 is refused with
    p, m, v untouched; n = 0 is accepted"""
    g = Gpu(gpu_device)
    n, args = 300, (1e-3, 0.9, 0.999, 1e-7, 3, 1.0)
    p, grad, m, v = adam_data(np.random.default_rng(9), n)
    grad[7] = m[7] = v[7] = 0.0
    s = AdamState(g, n, p, grad, m, v)
    g.ok(s.step(*args), "ng_adam_step")
    base = s.read()
    assert base[0][7] == p[7] and base[1][7] == 0 and base[2][7] == 0 and np.isfinite(base[0]).all()
    bad = grad.copy()
    bad[200] = np.nan
    s2 = AdamState(g, n, p, bad, m, v)
    g.ok(s2.step(*args), "ng_adam_step")
    other = np.arange(n) != 200
    for name, a, b in zip("pmv", s2.read(), base):
        assert np.isnan(a[200]) and np.array_equal(a[other], b[other]), name
    s3 = AdamState(g, n, p, grad, m, v)
    assert s3.step(1e-3, 0.9, 0.999, 1e-7, 0, 1.0) != 0, "step = 0 accepted"
    for name, a, b in zip("pmv", s3.read(), (p, m, v)):
        assert np.array_equal(a, b), f"{name} changed by a refused call"
    assert g.lib.ng_adam_step(g.h, g.st, 0, None, None, None, None, 1e-3, 0.9, 0.999, 1e-7, 1, 1.0) == 0
    g.torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- AMP attention
def c_rel(n):
    return 3e-5 * max(1.0, np.sqrt(n / 1024.0))


def check_amp(name, got, ref, mag, n, L):
    top = float(mag.max()) if mag.size else 0.0
    check_within(name, got, ref, (c_rel(n) + 4 * U * L) * mag + 1e-7 * top)


def amp_run_twice(g, t, N, K, F, E):
    rc, out = g.amp_bwd(t, N, K, F, E)
    g.ok(rc, "ng_amp_attend_bwd")
    rc, again = g.amp_bwd(t, N, K, F, E)
    g.ok(rc, "ng_amp_attend_bwd")
    for k in out:
        a, b = host(out[k]), host(again[k])
        assert np.array_equal(a, b, equal_nan=True), f"{k}: two runs differ"
    return {k: host(v) for k, v in out.items()}


@pytest.mark.parametrize("setting", ["wq0", "wk0"])
@pytest.mark.parametrize("case", R.AMP_EXACT_CASES, ids=R.amp_id)
def test_amp_exact(gpu_device, case, setting):
    """uniform softmax on integers: agg, dh, dwq, dwk equal float64 bit for bit, de is exactly 0"""
    g = Gpu(gpu_device)
    N, K, E, F, pattern = case
    rng = R.amp_rng(case, 2 + (setting == "wk0"))
    d = R.amp_exact_data(rng, N, K, F, E, R.amp_nlist(rng, N, K, pattern), setting)
    for name, units in R.amp_exact_in_range(d, K).items():
        assert units < 2.0 ** 24, f"{name}: test data outside the exact range ({units:.3g} units)"
    args = (d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"])
    agg, _, _ = R.amp_ref(*args)
    ref, _, _ = R.amp_bwd_ref(*args, d["dagg"])
    t = g.amp_up(d, N, K, E)
    rc, gagg = g.amp_fwd(t, N, K, F, E)
    g.ok(rc, "ng_amp_attend")
    check_exact("agg", host(gagg), agg)
    out = amp_run_twice(g, t, N, K, F, E)
    for k in ("dh", "dwq", "dwk"):
        check_exact(k, out[k], ref[k])
    assert not ref["de"].any()
    first_bad("de", ~(out["de"] == 0), out["de"])


def amp_vs_float64(g, case, d):
    N, K, E, F, pattern = case
    args = (d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"])
    agg, b, fm = R.amp_ref(*args)
    ref, mag, L = R.amp_bwd_ref(*args, d["dagg"])
    assert np.isfinite(agg).all() and all(np.isfinite(v).all() for v in ref.values())
    Ls = R.row_logit_scale(d["nlist"], L)
    indeg = int(np.bincount(d["nlist"].reshape(-1), minlength=N).max())
    n_row = max(F, E, K)
    t = g.amp_up(d, N, K, E)
    rc, gagg = g.amp_fwd(t, N, K, F, E)
    g.ok(rc, "ng_amp_attend")
    check_amp("agg", host(gagg), agg, fm["agg"], n_row, Ls["agg"])
    out = amp_run_twice(g, t, N, K, F, E)
    check_amp("dh", out["dh"], ref["dh"], mag["dh"], max(n_row, indeg), Ls["dh"])
    check_amp("de", out["de"], ref["de"], mag["de"], n_row, Ls["de"])
    check_amp("dwq", out["dwq"], ref["dwq"], mag["dwq"], max(n_row, N), Ls["dwq"])
    check_amp("dwk", out["dwk"], ref["dwk"], mag["dwk"], max(n_row, N), Ls["dwk"])
    return b, fm


@pytest.mark.parametrize("case", R.AMP_CASES, ids=R.amp_id)
def test_amp_normal(gpu_device, case):
    """random normal data, inv = 1 / degree and one row with inv = 0 (uniform weights)"""
    N, K, E, F, pattern = case
    rng = R.amp_rng(case, 5)
    d = R.amp_normal_data(rng, N, K, F, E, R.amp_nlist(rng, N, K, pattern), zero_inv_row=N >= 4)
    amp_vs_float64(Gpu(gpu_device), case, d)


@pytest.mark.parametrize("span", [80.0, 1e4], ids=["span80", "span1e4"])
@pytest.mark.parametrize("case", R.AMP_WIDE_CASES, ids=R.amp_id)
def test_amp_wide(gpu_device, case, span):
    """weights scaled until the logits reach about +-span: the softmax saturates, nothing overflows, no NaN"""
    N, K, E, F, pattern = case
    rng = R.amp_rng(case, 4)
    d = R.amp_widen(R.amp_normal_data(rng, N, K, F, E, R.amp_nlist(rng, N, K, pattern)), span)
    b, fm = amp_vs_float64(Gpu(gpu_device), case, d)
    assert fm["L"].max() >= 0.5 * span and (b.max(axis=1) > 0.99).any()
    if span > 1e3:
        assert (b == 0).any()


def test_amp_refusals_and_empty(gpu_device):
    """K = 0, 65, E = 0, 65 and F = 0 are refused by both entry points with every output untouched; N = 0 is accepted, the
    backward then zero-fills dwq and dwk"""
    g = Gpu(gpu_device)
    case = (5, 4, 8, 64, "random")
    N, K, E, F, pattern = case
    rng = R.amp_rng(case, 6)
    d = R.amp_normal_data(rng, N, K, F, E, R.amp_nlist(rng, N, K, pattern))
    t = g.amp_up(d, N, K, E)
    for k_, f_, e_ in ((0, F, E), (65, F, E), (K, F, 0), (K, F, 65), (K, 0, E)):
        rc, agg = g.amp_fwd(t, N, k_, f_, e_, agg=g.nan(N, F))
        assert rc != 0 and g.torch.isnan(agg).all(), ("ng_amp_attend", k_, f_, e_)
        rc, out = g.amp_bwd(t, N, k_, f_, e_, shape=(N, K, F, E))
        assert rc != 0 and all(g.torch.isnan(v).all() for v in out.values()), ("ng_amp_attend_bwd", k_, f_, e_)
    rc, agg = g.amp_fwd(t, 0, K, F, E)
    assert rc == 0 and g.torch.isnan(agg).all()
    rc, out = g.amp_bwd(t, 0, K, F, E)
    assert rc == 0 and g.torch.isnan(out["dh"]).all() and g.torch.isnan(out["de"]).all()
    for k in ("dwq", "dwk"):
        a = host(out[k])
        assert not a.any() and not np.signbit(a).any(), f"{k} != +0 with N = 0"
