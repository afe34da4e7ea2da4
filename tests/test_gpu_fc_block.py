"""ng_fc_block_fwd / ng_fc_block_bwd (csrc/fc_fused.hip; FCBlock of nmrgnn/model.py:179-196, all layers in one call) on every
branch of their dispatch against the float64 statement of tests/fc_block_ref.py, element by element, bit for bit and by a
statistic.  Every output (y[l], g, dx, dW, db, the scratch) is filled with NaN before each call.

Settings: default | NG_GEMM_MATH=fp32 | NG_FC_PATH=layered | frozen (ng_weights_frozen, fresh owner, two rounds); the weight
gradients also inside ng_defer_reductions(ctx, st, 1) ... ng_flush_reductions (bits of the eager call), and dx alone (dW = db =
NULL; bits of the full call).  Depths L = 2 .. 6.  Row counts from the device's CU count (nrows): the forward grid is
min(tiles, 2 cu) workgroups, the backward grid min(tiles, cu); the trips per workgroup a case aims at are asserted (TRIPS).

  branch (F = 64 unless said)                                               cases
  fc_fwd_body_h2<NL, softplus>, <NL, -1>    default, frozen, L <= 5         exact / normal [*-L2..L5], act none, relu, tanh: <NL, -1>
  fc_fwd_body_f32<NL>                        fp32; L = 6; weight guard       [*-L6], fp32 setting, test_weight_beyond_the_piece_range
    second and later trip, FC_FETCH(tile + grid), ragged last tile          [f2+ f2mix b3 f3], forward trips 2 and 3
  fc_fwd_repair inside a multi-trip run                                     test_repair_inside_a_multi_trip_forward
  fc_bwd_body<NL, H2, DW = true>             default, frozen, L <= 4        [*-L2..L4]; trips 2, 3 and 5: [b2+ b2mix f2- f2+ f2mix b3 f3]
  fc_bwd_body<NL, H2 = false>                fp32; weight guard             fp32 setting, test_weight_beyond_the_piece_range
  fc_bwd_body<.., DW = false>  (dx only)     both bodies                    every case: dx bits == the full call's
  layered backward over the piece forward's tape (L = 5, 6)                 [*-L5], [*-L6]
  layered forward / backward, fc_dp_kernel   NG_FC_PATH=layered             layered setting (F = 64); test_layered_geometry:
    c4n = No / 4, RL * c4n < 256, RL = 1, nblk at its cap, short last block   F in {8, 24, 40, 128, 256, 1024}; F = 32 in test_fc_block_vs_numpy
  reduce_seg_or_defer / reduce_or_defer in a deferred window                every case (fused: L <= 4; layered: L >= 5, layered setting)
  N = 0                                                                     test_zero_rows (F = 64 and 32)
  PK_FC image kept over calls, flag word raised and lowered again           test_weight_beyond_the_piece_range[*-frozen*]
  per-row dP scale, column scale of x beyond 2^15                           test_piece_backward_with_gradient_rows_... (one and two trips)

Two families of data:
  exact   (act none, relu) x0 in {-2..2}, W with about 4 non-zeros per column from {-1, +1}, b in {-1, 0, 1}, dg in {-2..2} on 256
          rows.  fc_block_ref.exact_conditions asserts on the CPU that every abs-sum stays below 2^24, max|x_l| < FC_XMAX and every
          operand has at most 11 significant bits; y_l, g, dx, dW_l, db_l then must equal float64 bit for bit on every branch and
          setting, deferred and dx-only included: a dropped or doubled row or tile cannot hide.
  normal  (all four activations) forward: each layer against the float64 layer applied to the GPU's own previous output,
          |got - ref| <= C_REL mag + 1e-7 max(mag), C_REL = 3e-5; and the whole chain with the bound times the layer index.
          backward on the float64 tape rounded to float32: k c mag + 1e-7 max(mag), k the number of matrix products between dg
          and the quantity (dx: L, dW_l and db_l: L - l); c = C_REL for dx; for dW, db on the fused kernel
          c = max(C_REL, (64 tiles_per_workgroup + grid) 2^-24), on the layered path c = C_REL max(1, sqrt(N / 1024)).
          statistic r = rms(got - ref) / rms(mag) <= sqrt(r32 r_drop) where a piece body runs (act none, relu asserted; softplus,
          tanh printed; N >= 64), and rms error within 8x that of the same call under NG_GEMM_MATH=fp32.

Findings: none in the kernels; every case passed on the unchanged library.  The statistic of the piece bodies sits at r32 (the
largest r / sqrt(r32 r_drop) over all cases is 0.06), so the float32 scale is met and a missing piece product would stand 20 to 50
times above the threshold.  Two notes on the plan of these tests, not on a bound.  The last layer's dW [64][32] has 2048 elements at every N, and g has
fewer than 4096 below N = 128: for these two the statistic is held with a floor of 2048 elements, for every other tensor with
STAT_MIN = 4096 (stat_floor).  And the float64 matrix products are called by one thread at a time: numpy's OpenBLAS (0.3.29)
returns wrong products when several Python threads call matmul at once ([261889, 8] @ [8, 8] from eight threads: 35 of 320 calls
differ from the serial result, by up to 6.5 relative; serial calls repeat bit for bit), so only the element-wise comparisons, which
do not enter BLAS, run side by side.

Sharpness, on scratch copies of the library, this file run once against each (256 CUs):
  (a) without the `wh x xl` MFMAs of hidden layer 1 in fc_fwd_body_h2: 37 cases fail — all 21 normal cases with L in {3, 4, 5}
      (per element, e.g. [n63-L3] y1: 1539 of 4032 entries outside C_REL mag; |err| / mag = 3.3e-5 .. 6.9e-5 at the first failing
      entries, the size of r_drop),
      test_weight_beyond_the_piece_range for L in {4, 5} (12), test_fc_block_vs_numpy (3) and the repair test (1); the exact
      family cannot see it (its small pieces are zero) and does not.
  (b) with the forward prefetch fetching `tile` instead of `tile + gridDim.x`: 29 cases fail — the 20 exact cases with a second
      forward trip ([f2+ f2mix b3 f3] x L, first difference at flat 2097152 = row 2 cu 64, the first row of the second trip), the
      6 normal cases of those row counts and the 3 repair cases.
  (c) with relu's slope replaced by softplus's in fc_bwd_body: 73 cases fail — the 36 exact cases with L <= 4 (dx: 51 of 64
      entries at N = 1, 16148 of 4198464 at f3), the 22 normal cases with L <= 4 and the 15 weight cases with L <= 4.
  (d) without `bad |= fc_out_of_range(y)` on the hidden layers' outputs in fc_fwd_body_h2: the 3 cases of
      test_repair_inside_a_multi_trip_forward fail (NaN in the 64 entries of the `grow` row, tile 3) and nothing else does: no other
      data has a row inside the range at the input and outside it later."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from fc_block_ref import (ACT, C_REL, FC_XMAX, STAT_MIN, bwd_stats, check, exact_conditions, exact_data, f32, fwd_stats,
                          normal_data, ref_bwd, ref_fwd, ref_layer_fwd, rstat)

pytestmark = pytest.mark.gpu

F64 = 64
POOL = ThreadPoolExecutor(8)         # the element-wise float64 comparisons of one call's tensors side by side; no BLAS call inside


def stat_floor(name, N, L):
    """elements a tensor needs to carry the statistic: STAT_MIN, but 2048 for the two tensors that cannot have it — the last layer's
    dW is [64][32] at every N, and g is [N][32] with N in 64 .. 127"""
    return STAT_MIN // 2 if name == f"dW{L - 1}" or (name == "g" and N < 128) else STAT_MIN
SETTINGS = [("default", {}, False), ("fp32", {"NG_GEMM_MATH": "fp32"}, False), ("layered", {"NG_FC_PATH": "layered"}, False),
            ("frozen", {}, True)]


def use(monkeypatch, env):
    for k in ("NG_GEMM_MATH", "NG_FC_PATH"):
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def cdiv(a, b):
    return -(-a // b)


def num_cu(dev):
    import torch
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


# spec -> (N, forward trips of the busiest workgroup, backward trips); "mix": some workgroups have one tile more than others and the
# last tile is ragged
def nrows(spec, cu):
    k = max(cu // 3, 1)
    return {"n1": 1, "n63": 63, "n64": 64, "n65": 65,
            "b2-": cu * 64 - 1, "b2+": cu * 64 + 1, "b2mix": cu * 64 + 64 * k + 17, "b3": 2 * cu * 64 + 65,
            "f2-": 2 * cu * 64 - 1, "f2+": 2 * cu * 64 + 1, "f2mix": 2 * cu * 64 + 64 * k + 17, "f3": 4 * cu * 64 + 65}[spec]


TRIPS = {"n1": (1, 1), "n63": (1, 1), "n64": (1, 1), "n65": (1, 1), "b2-": (1, 1), "b2+": (1, 2), "b2mix": (1, 2), "b3": (2, 3),
         "f2-": (1, 2), "f2+": (2, 3), "f2mix": (2, 3), "f3": (3, 5)}
SPECS = list(TRIPS)


def trips(N, cu):
    t = cdiv(N, 64)
    return cdiv(t, min(t, 2 * cu)), cdiv(t, min(t, cu))


def rows_for(spec, dev):
    cu = num_cu(dev)
    N = nrows(spec, cu)
    assert trips(N, cu) == TRIPS[spec], (spec, N, cu, trips(N, cu))
    if "mix" in spec:
        t = cdiv(N, 64)
        assert N % 64 and t % (2 * cu if spec[0] == "f" else cu)        # ragged; some workgroups one tile short
    return N


def fused_dw_c(N, cu):
    """dW / db of fc_bwd_body: one accumulator per workgroup over its tiles of 64 rows, then the grid's partials one after the other"""
    t = cdiv(N, 64)
    grid = min(t, cu)
    return max(C_REL, (64 * cdiv(t, grid) + grid) * 2.0 ** -24)


def layered_dw_c(N):
    return C_REL * max(1.0, np.sqrt(N / 1024.0))


# ------------------------------------------------------------------------------------------------- GPU calls
class Block:
    owner = 52000

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

    def ok(self, rc, what):
        self.ctx.check(rc, what)

    def fwd(self, N, F, L, act, tx, tW, tb):
        from nmrgnn_amd._lib import ptr, ptr_array
        ty = [self.nan(max(N, 1), F) for _ in range(L - 1)]
        tg = self.nan(max(N, 1), F // 2)
        rc = self.lib.ng_fc_block_fwd(self.h, self.st, N, F, L, act, ptr(tx), ptr_array(tW), ptr_array(tb), ptr_array(ty), ptr(tg))
        return rc, ty, tg

    def bwd(self, N, F, L, act, tape, tg, tW, tdg, want=True, defer=False):
        from nmrgnn_amd._lib import ptr, ptr_array
        dx = self.nan(max(N, 1), F)
        dW = [self.nan(*w.shape) for w in tW] if want else None
        db = [self.nan(w.shape[1]) for w in tW] if want else None
        scratch = self.nan(3, max(N, 1), F)
        if defer:
            self.ok(self.lib.ng_defer_reductions(self.h, self.st, 1), "ng_defer_reductions")
        try:
            rc = self.lib.ng_fc_block_bwd(self.h, self.st, N, F, L, act, ptr_array(tape), ptr(tg), ptr_array(tW), ptr(tdg), ptr(dx),
                                          ptr_array(dW) if want else None, ptr_array(db) if want else None, ptr(scratch))
            if defer and rc == 0:
                self.ok(self.lib.ng_flush_reductions(self.h, self.st), "ng_flush_reductions")
        finally:
            if defer:                                          # whatever happened, the tests that follow run eagerly
                self.lib.ng_defer_reductions(self.h, self.st, 0)
        return rc, dx, dW, db

    def freeze(self):
        # a fresh owner per case: the cache is keyed by weight ADDRESSES, and torch hands the addresses of an earlier case's
        # (freed) weights to this one
        Block.owner += 1
        self.ok(self.lib.ng_weights_frozen(self.h, Block.owner), "ng_weights_frozen")

    def thaw(self):
        self.lib.ng_weights_frozen(self.h, 0)

    def everything(self, N, F, L, act, tx, tW, tb, tdg, tape, tgt, frozen, tag):
        """forward and backward twice (frozen: both rounds inside the window; the second is served from the kept image), dx alone
        and the deferred window; asserts the bit identities and returns the host arrays of the last round"""
        if frozen:
            self.freeze()
        try:
            rc, ty, tg = self.fwd(N, F, L, act, tx, tW, tb)
            self.ok(rc, f"ng_fc_block_fwd ({tag})")
            rc, dx, dW, db = self.bwd(N, F, L, act, tape, tgt, tW, tdg)
            self.ok(rc, f"ng_fc_block_bwd ({tag})")
            rc, ty2, tg2 = self.fwd(N, F, L, act, tx, tW, tb)
            self.ok(rc, f"ng_fc_block_fwd again ({tag})")
            rc, dx2, dW2, db2 = self.bwd(N, F, L, act, tape, tgt, tW, tdg)
            self.ok(rc, f"ng_fc_block_bwd again ({tag})")
            rc, dx3, _, _ = self.bwd(N, F, L, act, tape, tgt, tW, tdg, want=False)
            self.ok(rc, f"ng_fc_block_bwd dx only ({tag})")
            rc, dx4, dW4, db4 = self.bwd(N, F, L, act, tape, tgt, tW, tdg, defer=True)
            self.ok(rc, f"ng_fc_block_bwd deferred ({tag})")
        finally:
            if frozen:
                self.thaw()
        same = self.torch.equal
        assert all(same(a, b) for a, b in zip(ty + [tg], ty2 + [tg2])), f"forward: two calls differ ({tag})"
        assert same(dx, dx2) and all(same(a, b) for a, b in zip(dW + db, dW2 + db2)), f"backward: two calls differ ({tag})"
        assert same(dx, dx3), f"dx: dW = db = NULL changes its bits ({tag})"
        assert same(dx, dx4) and all(same(a, b) for a, b in zip(dW + db, dW4 + db4)), f"deferred window: bits differ ({tag})"
        return dict(ys=[host(v) for v in ty2], g=host(tg2), dx=host(dx2), dW=[host(v) for v in dW2], db=[host(v) for v in db2])


def host(t):
    return None if t is None else t.cpu().numpy()


def check_exact(name, got, ref32):
    """ref32: the float64 result as float32 (exact_conditions has asserted that nothing is lost on the way)"""
    if not np.array_equal(got, ref32):                        # NaN fails
        bad = ~(got == ref32)
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries differ from float64; first at flat {k}: "
                             f"got {got.reshape(-1)[k]!r} ref {ref32.reshape(-1)[k]!r}")


def exact_refs(xs, g, dx, dWs, dbs):
    L = len(dWs)
    named = [(f"y{l}", xs[l + 1]) for l in range(L - 1)] + [("g", g), ("dx", dx)] + \
        [(f"dW{l}", dWs[l]) for l in range(L)] + [(f"db{l}", dbs[l]) for l in range(L)]
    return [(n, v.astype(np.float32)) for n, v in named]


def check_all_exact(tag, r, refs):
    L = len(r["dW"])
    got = r["ys"] + [r["g"], r["dx"]] + r["dW"] + r["db"]
    assert len(got) == len(refs) == 3 * L + 1
    for (name, ref32), v in zip(refs, got):
        check_exact(f"{name} ({tag})", v, ref32)


def rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if a.size else 0.0


# ------------------------------------------------------------------------------------------------- exact family
CASES = [(f"{s}-L{L}", s, L) for s in SPECS for L in (2, 3, 4, 5, 6)]


@pytest.mark.parametrize("cid,spec,L", CASES, ids=[c[0] for c in CASES])
def test_fc_block_exact_integers(gpu_device, monkeypatch, cid, spec, L):
    """y_l, g, dx, dW_l, db_l bit for bit equal to float64 under every setting, dx-only and deferred included"""
    gpu = Block(gpu_device)
    N = rows_for(spec, gpu_device)
    for act in (ACT["none"], ACT["relu"]):
        rng = np.random.default_rng([N, L, act, 1])
        x, Ws, bs, dg = exact_data(rng, N, F64, L)
        xs, g, dx, dWs, dbs = exact_conditions(x, Ws, bs, dg, act)       # fails here, on the CPU, if the data leave the exact set
        tx, tW, tb, tdg = gpu.up(x), [gpu.up(w) for w in Ws], [gpu.up(b) for b in bs], gpu.up(dg)
        tape, tgt = [gpu.up(v) for v in xs], gpu.up(g)
        refs = exact_refs(xs, g, dx, dWs, dbs)
        for sname, env, frozen in SETTINGS:
            use(monkeypatch, env)
            tag = f"{sname} act {act}"
            r = gpu.everything(N, F64, L, act, tx, tW, tb, tdg, tape, tgt, frozen, tag)
            check_all_exact(tag, r, refs)


# ------------------------------------------------------------------------------------------------- normal family
def piece_forward(sname, L):
    return sname in ("default", "frozen") and L <= 5


def piece_backward(sname, L):
    return sname in ("default", "frozen") and L <= 4


def check_forward(tag, x, Ws, bs, act, r, chain, stats=None):
    """each layer on its own against float64 of the GPU's previous output, the whole chain against `chain` = ref_fwd's (xs, g,
    mags); stats: [(r32, r_drop)] per layer to hold the statistic against; returns the rms errors of the chain comparison"""
    L = len(Ws)
    xs, g, mags = chain

    # the matrix products one after the other (BLAS is entered by one thread at a time), the element-wise comparisons side by side
    refs = [ref_layer_fwd(x if l == 0 else f32(r["ys"][l - 1]), Ws[l], bs[l], act, l == L - 1) for l in range(L)]

    def layer(l):
        last = l == L - 1
        got = r["g"] if last else r["ys"][l]
        name = "g" if last else f"y{l}"
        ref, mag = refs[l]
        check(f"{name} ({tag})", got, ref, mag)
        whole = g if last else xs[l + 1]
        check(f"{name} chain ({tag})", got, whole, mags[l], c_rel=(l + 1) * C_REL)
        return name, got.size, rms(got - whole), rstat(got, ref, mag) if stats is not None else None

    out = []
    for l, (name, size, e, rr) in enumerate(POOL.map(layer, range(L))):
        out.append(e)
        if stats is not None:
            r32, r_drop = stats[l]
            print(f"  r({name}) = {rr:.3e}   r32 {r32:.3e}  r_drop {r_drop:.3e}   ({tag})")
            if act in (ACT["none"], ACT["relu"]):
                assert size >= stat_floor(name, x.shape[0], L), (name, size)
                assert rr <= np.sqrt(r32 * r_drop), (name, tag, rr, r32, r_drop)
    return out


def check_backward(tag, L, r, ref, mags, c_dw, stats=None, act=0):
    """dx, dW_l, db_l against ref_bwd's values and magnitudes; stats: bwd_stats' thresholds; returns the rms errors"""
    (dx, dWs, dbs), (mx, mWs, mbs) = ref, mags
    items = [("dx", r["dx"], dx, mx, L * C_REL)]
    for l in range(L):
        items.append((f"dW{l}", r["dW"][l], dWs[l], mWs[l], (L - l) * c_dw))
        items.append((f"db{l}", r["db"][l], dbs[l], mbs[l], (L - l) * c_dw))

    def one(it):
        name, got, want, mag, c = it
        check(f"{name} ({tag})", got, want, mag, c_rel=c)
        return name, rms(got - want), rstat(got, want, mag), got.size

    res = {name: (e, rr, size) for name, e, rr, size in POOL.map(one, items)}
    if stats is not None:
        for name, (r32, r_drop) in [("dx", stats["dx"])] + [(f"dW{l}", stats["dW"][l]) for l in range(L)]:
            _, rr, size = res[name]
            print(f"  r({name}) = {rr:.3e}   r32 {r32:.3e}  r_drop {r_drop:.3e}   ({tag})")
            if act in (ACT["none"], ACT["relu"]):
                assert size >= stat_floor(name, r["dx"].shape[0], L), (name, size)
                assert rr <= np.sqrt(r32 * r_drop), (name, tag, rr, r32, r_drop)
    return {k: v[0] for k, v in res.items()}


# the float64 work of this family grows with N * L * 4 activations * 4 settings: every depth at the small row counts and at b2mix
# (backward trips 1 and 2 mixed, ragged), the longer runs at the depths whose bodies differ (L = 4: all fused, 5: piece forward +
# layered backward, 6: fp32 forward) and a second forward trip also at L = 2 and 3; the exact family above runs every row count at
# every depth
NORMAL_CASES = [c for c in CASES if c[1] in ("n1", "n63", "n64", "n65", "b2mix")] + \
    [c for c in CASES if (c[1], c[2]) in (("b2+", 2), ("b2+", 4), ("f2+", 2), ("f2+", 3), ("f2-", 3), ("f2+", 5), ("f2mix", 4), ("b3", 6), ("f3", 4))]


@pytest.mark.parametrize("cid,spec,L", NORMAL_CASES, ids=[c[0] for c in NORMAL_CASES])
def test_fc_block_normal_vs_float64(gpu_device, monkeypatch, cid, spec, L):
    """per element and by the statistic against float64, all four activations, every setting; the piece bodies within 8x the rms
    error of the fp32 bodies; identical bits on a repeated call, with dx alone and in a deferred window"""
    gpu = Block(gpu_device)
    cu = num_cu(gpu_device)
    N = rows_for(spec, gpu_device)
    rng = np.random.default_rng([N, L, 2])
    x, Ws, bs, dg = normal_data(rng, N, F64, L)
    tx, tW, tb, tdg = gpu.up(x), [gpu.up(w) for w in Ws], [gpu.up(b) for b in bs], gpu.up(dg)
    for aname, act in ACT.items():
        chain = ref_fwd(x, Ws, bs, act)
        tape64, g64 = [f32(v) for v in chain[0]], f32(chain[1])           # independent of the GPU forward
        ref, mags = ref_bwd(tape64, g64, Ws, dg, act)
        want_stats = N >= 64
        fst = fwd_stats(tape64, Ws, bs, act) if want_stats else None
        bst = bwd_stats(tape64, g64, Ws, dg, act, ref=(ref, mags)) if want_stats else None
        tape, tgt = [gpu.up(v) for v in tape64], gpu.up(g64)
        ef, eb = {}, {}
        for sname, env, frozen in SETTINGS:
            use(monkeypatch, env)
            tag = f"{sname} {aname}"
            r = gpu.everything(N, F64, L, act, tx, tW, tb, tdg, tape, tgt, frozen, tag)
            ef[sname] = check_forward(tag, x, Ws, bs, act, r, chain, fst if piece_forward(sname, L) else None)
            fused = sname != "layered" and L <= 4
            eb[sname] = check_backward(tag, L, r, ref, mags, fused_dw_c(N, cu) if fused else layered_dw_c(N),
                                       bst if piece_backward(sname, L) else None, act)
        # the piece bodies within 8x the rms error of the fp32 bodies on the same inputs (no floor: an exact fp32 result asks the same)
        for sname in ("default", "frozen"):
            if piece_forward(sname, L):
                for l, (v, w) in enumerate(zip(ef[sname], ef["fp32"])):
                    assert v <= 8.0 * w, ("forward", l, aname, sname, v, w)
            if piece_backward(sname, L):
                for k, v in eb[sname].items():
                    assert v <= 8.0 * eb["fp32"][k], (k, aname, sname, v, eb["fp32"][k])


# ------------------------------------------------------------------------------------------------- N = 0
@pytest.mark.parametrize("F", [64, 32])
def test_zero_rows(gpu_device, monkeypatch, F):
    """N = 0: the forward returns NG_OK and writes nothing; the backward zeroes dW and db and leaves dx alone"""
    gpu = Block(gpu_device)
    rng = np.random.default_rng(F)
    for L in (2, 4, 6):
        x, Ws, bs, dg = exact_data(rng, 1, F, L)
        tx, tW, tb, tdg = gpu.up(x), [gpu.up(w) for w in Ws], [gpu.up(b) for b in bs], gpu.up(dg)
        for sname, env, frozen in SETTINGS:
            use(monkeypatch, env)
            if frozen:
                gpu.freeze()
            try:
                rc, ty, tg = gpu.fwd(0, F, L, 1, tx, tW, tb)
                gpu.ok(rc, "ng_fc_block_fwd (N = 0)")
                rc, dx, dW, db = gpu.bwd(0, F, L, 1, [tx] + ty, tg, tW, tdg)
                gpu.ok(rc, "ng_fc_block_bwd (N = 0)")
                rc, dx2, _, _ = gpu.bwd(0, F, L, 1, [tx] + ty, tg, tW, tdg, want=False)
                gpu.ok(rc, "ng_fc_block_bwd (N = 0, dx only)")
            finally:
                if frozen:
                    gpu.thaw()
            gpu.torch.cuda.synchronize()
            assert all(bool(t.isnan().all()) for t in ty + [tg, dx, dx2]), f"written with N = 0 ({sname}, L {L})"
            for t in dW + db:
                a = host(t)
                assert not a.any() and not np.signbit(a).any(), f"dW / db != +0 with N = 0 ({sname}, L {L})"


# ------------------------------------------------------------------------------------------------- layered geometry
def dp_geometry(N, No, cu):
    """(rl, rows per block, blocks) of fc_dp_kernel's launch in ng_fc_block_bwd"""
    c4n = No // 4
    rl = max(256 // c4n, 1)
    nb = min(cdiv(N, rl), 4 * cu)
    rows = cdiv(cdiv(N, nb), rl) * rl
    return rl, rows, cdiv(N, rows)


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("F", [8, 24, 40, 128, 256, 1024])
def test_layered_geometry(gpu_device, monkeypatch, F, L):
    """the layer-by-layer path at feature sizes other than 64: fc_dp_kernel with c4n = F / 4 and F / 8 column chunks, row lanes
    that do not fill the block (F = 24, 40), one row lane (F = 1024), the block count at its cap 4 cu and a last block of one row.  Activations none and relu on the exact
    family (bit for bit), softplus and tanh on the normal one (per element; contraction F <= 1024, so C_REL as it is)"""
    gpu = Block(gpu_device)
    cu = num_cu(gpu_device)
    rl = max(256 // (F // 4), 1)
    N = (4 * cu - 1) * 2 * rl + 1
    assert dp_geometry(N, F, cu) == (rl, 2 * rl, 4 * cu)                 # the cap is reached; the last block holds one row
    if F in (24, 40):
        assert rl * (F // 4) < 256
    rng = np.random.default_rng([F, L])
    for family in ("exact", "normal"):
        # activations none and relu on the exact family, softplus and tanh on the normal one
        for aname, act in (("none", 0), ("relu", 2)) if family == "exact" else (("softplus", 1), ("tanh", 3)):
            if family == "exact":
                x, Ws, bs, dg = exact_data(rng, N, F, L, nnz=min(4, F // 2))
                xs, g, dx, dWs, dbs = exact_conditions(x, Ws, bs, dg, act)
                tape64, g64 = xs, g
            else:
                x, Ws, bs, dg = normal_data(rng, N, F, L)
                chain = ref_fwd(x, Ws, bs, act)
                tape64, g64 = [f32(v) for v in chain[0]], f32(chain[1])
                ref, mags = ref_bwd(tape64, g64, Ws, dg, act)
            tx, tW, tb, tdg = gpu.up(x), [gpu.up(w) for w in Ws], [gpu.up(b) for b in bs], gpu.up(dg)
            tape, tgt = [gpu.up(v) for v in tape64], gpu.up(g64)
            for sname, env, frozen in SETTINGS[:2]:                      # (every setting takes the layered path here)
                use(monkeypatch, env)
                tag = f"F {F} {family} {sname} {aname}"
                r = gpu.everything(N, F, L, act, tx, tW, tb, tdg, tape, tgt, frozen, tag)
                if family == "exact":
                    check_all_exact(tag, r, exact_refs(xs, g, dx, dWs, dbs))
                else:
                    check_forward(tag, x, Ws, bs, act, r, chain)
                    check_backward(tag, L, r, ref, mags, layered_dw_c(N))


# ------------------------------------------------------------------------------------------------- range and repair
def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def ref_fc(x, Ws, bs, act):
    f = softplus if act == 1 else (lambda v: v)
    xs = [x]
    for W, b in zip(Ws[:-1], bs[:-1]):
        xs.append(f(xs[-1] @ W + b) + xs[-1])
    return xs, f(xs[-1] @ Ws[-1] + bs[-1])


def ref_fc_bwd(xs, g, Ws, dg, act):
    dact = (lambda s: 1 - np.exp(-s)) if act == 1 else (lambda s: np.ones_like(s))
    L = len(Ws)
    dWs, dbs = [None] * L, [None] * L
    dP = dg * dact(g)
    dWs[L - 1], dbs[L - 1] = xs[L - 1].T @ dP, dP.sum(0)
    d = dP @ Ws[L - 1].T
    for l in range(L - 2, -1, -1):
        s = xs[l + 1] - xs[l]
        dP = d * dact(s)
        dWs[l], dbs[l] = xs[l].T @ dP, dP.sum(0)
        d = d + dP @ Ws[l].T
    return d, dWs, dbs


@pytest.mark.parametrize("N,F,L,act", [(1000, 64, 4, 1), (64, 64, 2, 1), (777, 64, 3, 0), (2049, 64, 6, 1),
                                       (1, 64, 4, 1), (500, 32, 4, 1)])
def test_fc_block_vs_numpy(gpu_device, N, F, L, act):
    rng = np.random.default_rng(N + L)
    Fh = F // 2
    x = rng.standard_normal((N, F))
    Ws = [rng.standard_normal((F, F)) * 0.2 for _ in range(L - 1)] + [rng.standard_normal((F, Fh)) * 0.2]
    bs = [rng.standard_normal(F) * 0.1 for _ in range(L - 1)] + [rng.standard_normal(Fh) * 0.1]
    dg = rng.standard_normal((N, Fh))
    xs, g = ref_fc(x, Ws, bs, act)
    dx, dWs, dbs = ref_fc_bwd(xs, g, Ws, dg, act)
    ys, gg, tdx, tdW, tdb = _run_block(gpu_device, x, Ws, bs, dg, act)
    for l in range(L - 1):
        np.testing.assert_allclose(ys[l], xs[l + 1], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(gg, g, rtol=2e-5, atol=2e-5)
    scale = lambda a: max(1.0, np.abs(a).max())
    assert np.abs(tdx - dx).max() < 2e-4 * scale(dx)
    for l in range(L):
        assert np.abs(tdW[l] - dWs[l]).max() < 2e-4 * scale(dWs[l]), l
        assert np.abs(tdb[l] - dbs[l]).max() < 2e-4 * scale(dbs[l]), l


def _run_block(dev, x, Ws, bs, dg, act, xs_tape=None, g_tape=None):
    """forward + backward through the C ABI; xs_tape / g_tape: feed the backward these tapes instead of the forward's"""
    gpu = Block(dev)
    N, F = x.shape
    L = len(Ws)
    tx, tW, tb, tdg = gpu.up(x), [gpu.up(w) for w in Ws], [gpu.up(b) for b in bs], gpu.up(dg)
    rc, ty, tg = gpu.fwd(N, F, L, act, tx, tW, tb)
    gpu.ok(rc, "fwd")
    tape = [tx] + ty if xs_tape is None else [gpu.up(v) for v in xs_tape]
    tgt = tg if g_tape is None else gpu.up(g_tape)
    rc, tdx, tdW, tdb = gpu.bwd(N, F, L, act, tape, tgt, tW, tdg)
    gpu.ok(rc, "bwd")
    return [host(v) for v in ty], host(tg), host(tdx), [host(w) for w in tdW], [host(b) for b in tdb]


def _weights(rng, F, L, s=0.2):
    Fh = F // 2
    return ([rng.standard_normal((F, F)) * s for _ in range(L - 1)] + [rng.standard_normal((F, Fh)) * s],
            [rng.standard_normal(F) * 0.1 for _ in range(L - 1)] + [rng.standard_normal(Fh) * 0.1])


def test_piece_forward_redoes_a_tile_whose_activations_leave_the_fp16_range(gpu_device):
    """fc_fused.hip, piece body: activations are taken as two fp16 pieces UNSCALED; a tile with a value at or beyond 65504
    (input row, or a hidden layer's output) is redone by the same workgroup with the fp32 layers.  Rows of 3e5, a row that
    only overflows in layer 2 (6e4 growing past 65504 through the residual), inf and nan rows, next to ordinary tiles.
    (Every such row here is already beyond FC_XMAX = 65504 / 16 at the input; rows that only the flag on a hidden layer's output
    sees are in test_repair_inside_a_multi_trip_forward, held to a bound that scales with the sum of absolute terms.)"""
    rng = np.random.default_rng(7)
    N, F, L = 1000, 64, 4
    x = rng.standard_normal((N, F))
    x[70] *= 3e5                      # tile 1: beyond the range at the input
    x[200] = 6.0e4 + 100.0 * rng.random(F)   # tile 3: inside at the input, outside after a residual layer or two
    x[900, 5] = 2.0e5                 # tile 14: one element
    Ws, bs = _weights(rng, F, L)
    Ws[0][:, :] = np.abs(Ws[0])       # positive weights: row 200 grows
    dg = rng.standard_normal((N, F // 2))
    xs, g = ref_fc(x, Ws, bs, 1)
    assert np.abs(xs[2][200]).max() > 65504 > np.abs(xs[0][200]).max()
    ys, gg, *_ = _run_block(gpu_device, x, Ws, bs, dg, 1)
    for l in range(L - 1):
        np.testing.assert_allclose(ys[l], xs[l + 1], rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(gg, g, rtol=3e-5, atol=3e-5)
    # non-finite inputs come out non-finite in their own rows and nowhere else
    x2 = x.copy()
    x2[300, 3] = np.inf
    x2[301, 4] = np.nan
    xs2, g2 = ref_fc(np.where(np.isfinite(x2), x2, 0.0), Ws, bs, 1)
    ys2, gg2, *_ = _run_block(gpu_device, x2, Ws, bs, dg, 1)
    assert not np.all(np.isfinite(ys2[0][300])) and not np.all(np.isfinite(ys2[0][301]))
    keep = np.ones(N, bool)
    keep[[300, 301]] = False
    np.testing.assert_allclose(ys2[-1][keep], xs2[-1][keep], rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(gg2[keep], g2[keep], rtol=3e-5, atol=3e-5)


@pytest.mark.parametrize("L", [2, 4, 5])
def test_repair_inside_a_multi_trip_forward(gpu_device, L):
    """Three trips per workgroup (grid 2 cu).  A tile is flagged at two places of fc_fwd_body_h2: by its input rows (FC_PUT) and by a
    hidden layer's output (`bad |= fc_out_of_range(y)`).  Rows of each kind:
      grow    max|x_0| < FC_XMAX = 4094 <= max|x_1| < 65504: in range at the input, only the hidden layer's flag sees it
      grow2   (L >= 3) max|x_0|, max|x_1| < FC_XMAX <= max|x_2|: the flag of the second hidden layer
      in6e4   FC_XMAX <= |x_0| < 65504 <= |x_1|;  mid  one element of 5000;  big  a row times 3e5 (>= 65504 at the input)
    placed in a workgroup's first tile with more following, in a workgroup's last tile, in two consecutive tiles of one workgroup
    (t and t + grid, twice: input-flagged and output-flagged), and in row N - 1 of the ragged last tile (the row the clamped
    loads repeat).  The repair overwrites X0 and the planes while the next tile's rows wait in registers.  Tiles without such a
    row keep the bits of the same launch without the bad rows; every tile is held to the float64 bound, layer by layer."""
    gpu = Block(gpu_device)
    cu = num_cu(gpu_device)
    N = rows_for("f3", gpu_device)
    grid, ntiles = 2 * cu, cdiv(N, 64)
    assert ntiles == 2 * grid + 2 and N - 1 == (ntiles - 1) * 64          # workgroup 1's third tile holds the one row N - 1
    assert grid >= 12                                                      # workgroups 0, 1, 3, 7 and 10 below are five
    rng = np.random.default_rng([L, 77])
    x, Ws, bs, dg = normal_data(rng, N, F64, L)
    for l in range(min(2, L - 1)):
        Ws[l] = np.abs(Ws[l])                                              # positive weights: the grow rows grow
    clean = x.copy()
    second = "grow2" if L >= 3 else "grow"
    bad = {3 * 64 + 5: "grow", (grid + 3) * 64 + 40: second,               # tiles 3 and 3 + grid of workgroup 3, a third following
           (grid + 7) * 64 + 63: "big", (2 * grid) * 64: "mid",            # last tile of workgroup 7; third tile of workgroup 0
           10 * 64 + 31: "in6e4", (grid + 10) * 64 + 32: "big",            # tiles 10 and 10 + grid of workgroup 10
           N - 1: "big"}
    ramp = np.arange(F64, dtype=np.float64)
    for row, kind in bad.items():
        if kind == "mid":
            x[row, 9] = 5000.0
        elif kind == "big":
            x[row] *= 3e5
        elif kind == "in6e4":
            x[row] = f32(6.0e4 + 100.0 * rng.random(F64))
        else:
            x[row] = (3000.0 if kind == "grow" else 150.0) + ramp
    assert FC_XMAX <= 5000.0 < 65504.0
    flagged = np.zeros(ntiles, bool)
    flagged[[r // 64 for r in bad]] = True
    assert flagged[ntiles - 1] and flagged[3] and flagged[3 + grid] and flagged[10] and flagged[10 + grid] and flagged.sum() == 7
    for act in (1, 2):
        chain = ref_fwd(x, Ws, bs, act)
        top = lambda l, row: float(np.abs(chain[0][l][row]).max())        # max|x_l[row]|, l <= L - 1
        for row, kind in bad.items():                                      # which flag each row needs, asserted on the CPU
            if kind == "grow":
                assert top(0, row) < FC_XMAX <= top(1, row) < 65504.0, (row, top(0, row), top(1, row))
            elif kind == "grow2":
                assert max(top(0, row), top(1, row)) < FC_XMAX <= top(2, row), (row, top(0, row), top(1, row), top(2, row))
            elif kind == "in6e4":
                assert FC_XMAX <= top(0, row) < 65504.0 < top(1, row)
        tW, tb = [gpu.up(w) for w in Ws], [gpu.up(b) for b in bs]
        rc, ty, tg = gpu.fwd(N, F64, L, act, gpu.up(x), tW, tb)
        gpu.ok(rc, "forward")
        rc, cy, cg = gpu.fwd(N, F64, L, act, gpu.up(clean), tW, tb)
        gpu.ok(rc, "forward (clean)")
        r = dict(ys=[host(v) for v in ty], g=host(tg))
        c = dict(ys=[host(v) for v in cy], g=host(cg))
        check_forward(f"repair act {act}", x, Ws, bs, act, r, chain)
        keep = np.repeat(~flagged, 64)[:N]
        for a, b in zip(r["ys"] + [r["g"]], c["ys"] + [c["g"]]):
            assert np.array_equal(a[keep], b[keep]), "a tile without a bad row changed its bits"


WEIGHT_CASES = [(L, l) for L in (2, 4, 5) for l in sorted({0, L // 2, L - 1})]


def _flat(r):
    return r["ys"] + [r["g"], r["dx"]] + r["dW"] + r["db"]


@pytest.mark.parametrize("mode", ["eager", "frozen-out-first", "frozen-in-first"])
@pytest.mark.parametrize("L,layer", WEIGHT_CASES, ids=[f"L{L}-w{l}" for L, l in WEIGHT_CASES])
def test_weight_beyond_the_piece_range(gpu_device, monkeypatch, L, layer, mode):
    """2^8 |w| >= 65504 in the first, a middle or the last layer: the pack launch raises the guard (or the flag word of a kept image) and
    the fp32 bodies run behind it, so every output carries the bits of the same call under NG_GEMM_MATH=fp32.  Inside a frozen
    window the weight is then set back into range and ng_weights_changed announced: the flag word must be lowered again (the
    outputs leave the fp32 bits and meet the piece body's statistic); and the reverse order."""
    gpu = Block(gpu_device)
    N = 4099
    rng = np.random.default_rng([L, layer, 5])
    x, Ws, bs, dg = normal_data(rng, N, F64, L)
    x = f32(x * 0.1)
    W_in = [w.copy() for w in Ws]
    W_out = [w.copy() for w in Ws]
    W_out[layer][3, 5] = 400.0
    assert 256.0 * 400.0 >= 65504.0
    act = ACT["relu"]
    tx, tb, tdg = gpu.up(x), [gpu.up(b) for b in bs], gpu.up(dg)

    def run(tW, Wcur):
        chain = ref_fwd(x, Wcur, bs, act)
        tape64, g64 = [f32(v) for v in chain[0]], f32(chain[1])
        ref, mags = ref_bwd(tape64, g64, Wcur, dg, act)
        tape, tgt = [gpu.up(v) for v in tape64], gpu.up(g64)
        r = gpu.everything(N, F64, L, act, tx, tW, tb, tdg, tape, tgt, False, f"L {L} layer {layer} {mode}")
        return r, chain, (tape64, g64, ref, mags)

    def held_to_float64(r, Wcur, chain, bw, piece):
        tape64, g64, ref, mags = bw
        fst = fwd_stats(tape64, Wcur, bs, act) if piece else None
        bst = bwd_stats(tape64, g64, Wcur, dg, act, ref=(ref, mags)) if piece and L <= 4 else None
        check_forward(f"weights {mode}", x, Wcur, bs, act, r, chain, fst)
        check_backward(f"weights {mode}", L, r, ref, mags, fused_dw_c(N, num_cu(gpu_device)) if L <= 4 else layered_dw_c(N), bst, act)

    same = lambda a, b: all(np.array_equal(u, v) for u, v in zip(_flat(a), _flat(b)))
    fwd_same = lambda a, b: all(np.array_equal(u, v) for u, v in zip(a["ys"] + [a["g"]], b["ys"] + [b["g"]]))
    # the fp32 setting's bits for both weight sets
    use(monkeypatch, {"NG_GEMM_MATH": "fp32"})
    f_out, chain_out, bw_out = run([gpu.up(w) for w in W_out], W_out)
    f_in, chain_in, bw_in = run([gpu.up(w) for w in W_in], W_in)
    held_to_float64(f_out, W_out, chain_out, bw_out, False)
    use(monkeypatch, {})
    if mode == "eager":
        r, *_ = run([gpu.up(w) for w in W_out], W_out)
        assert same(r, f_out), "a weight beyond the range: not the fp32 body's bits"
        r, *_ = run([gpu.up(w) for w in W_in], W_in)
        assert not fwd_same(r, f_in), "in range: the piece body was expected"
        return
    first, second = (W_out, W_in) if mode == "frozen-out-first" else (W_in, W_out)
    tW = [gpu.up(w) for w in first]
    gpu.freeze()
    try:
        for rnd, Wcur in enumerate((first, second, first)):
            if rnd:
                tW[layer][3, 5] = float(Wcur[layer][3, 5])                 # in place: the image's key is the address
                gpu.ok(gpu.lib.ng_weights_changed(gpu.h), "ng_weights_changed")
            r, chain, bw = run(tW, Wcur)
            if Wcur is W_out:
                assert same(r, f_out), f"round {rnd}: beyond the range, not the fp32 body's bits (flag word not raised)"
            else:
                assert not fwd_same(r, f_in), f"round {rnd}: in range, still the fp32 body's bits (flag word not lowered)"
                if L <= 4:
                    assert not np.array_equal(r["dx"], f_in["dx"]), f"round {rnd}: backward still on the fp32 body"
                held_to_float64(r, W_in, chain, bw, True)
    finally:
        gpu.thaw()


@pytest.mark.parametrize("cache", [False, True])
def test_piece_kernels_take_the_fp32_body_when_a_weight_leaves_the_range(gpu_device, cache):
    """2^8 * 400 > 65504: no fp16 pieces of that weight; the pack launch raises the guard (or sets the flag word of a cached
    image) and both kernels run their fp32 bodies for the whole launch"""
    from nmrgnn_amd import _lib
    rng = np.random.default_rng(8)
    N, F, L = 777, 64, 3
    x = rng.standard_normal((N, F)) * 0.1
    Ws, bs = _weights(rng, F, L, s=0.05)
    Ws[1][3, 5] = 400.0
    dg = rng.standard_normal((N, F // 2))
    xs, g = ref_fc(x, Ws, bs, 1)
    dx, dWs, dbs = ref_fc_bwd(xs, g, Ws, dg, 1)
    ctx = _lib.get_context(0)
    if cache:
        ctx.lib.ng_weights_frozen(ctx.handle, 12345)
    try:
        for _ in range(2 if cache else 1):      # second round: the cached image and its flag word
            ys, gg, tdx, tdW, tdb = _run_block(gpu_device, x, Ws, bs, dg, 1)
            np.testing.assert_allclose(ys[-1], xs[-1], rtol=3e-5, atol=3e-5)
            np.testing.assert_allclose(gg, g, rtol=3e-5, atol=3e-5)
            sc = lambda a: max(1.0, np.abs(a).max())
            assert np.abs(tdx - dx).max() < 1e-4 * sc(dx)
            for l in range(L):
                assert np.abs(tdW[l] - dWs[l]).max() < 1e-4 * sc(dWs[l]), l
                assert np.abs(tdb[l] - dbs[l]).max() < 1e-4 * sc(dbs[l]), l
    finally:
        if cache:
            ctx.lib.ng_weights_frozen(ctx.handle, 0)


def _decades(gpu_device, monkeypatch, N, step1_tile=None):
    rng = np.random.default_rng(9)
    F, L = 64, 4
    x = rng.standard_normal((N, F))
    x[:, 7] *= 4.0e4                          # a feature column beyond 2^15 in the tape
    x[40:50] *= 300.0
    if step1_tile is not None:                # a second large column, in step 1 (rows 32..63) of one tile only
        x[step1_tile * 64 + 32:step1_tile * 64 + 64, 11] *= 4.0e4
    Ws, bs = _weights(rng, F, L, s=0.1)
    dg = rng.standard_normal((N, F // 2)) * 10.0 ** rng.uniform(-6, 0, (N, 1))
    dg[rng.random(N) < 0.3] = 0.0
    dg[5] *= 1e4
    xs, g = ref_fc(x, Ws, bs, 1)
    dx, dWs, dbs = ref_fc_bwd(xs, g, Ws, dg, 1)
    res = {}
    for mode in ("f16x2", "fp32"):
        monkeypatch.setenv("NG_GEMM_MATH", mode)
        # the float64 tapes (rounded to fp32) for both modes: the backward is compared on identical inputs
        res[mode] = _run_block(gpu_device, x, Ws, bs, dg, 1, xs_tape=xs, g_tape=g)[2:]
    ref = [dx] + dWs + dbs
    names = ["dx"] + ["dW%d" % l for l in range(L)] + ["db%d" % l for l in range(L)]
    flat = lambda r: [r[0]] + list(r[1]) + list(r[2])
    for name, want, got2, got1 in zip(names, ref, flat(res["f16x2"]), flat(res["fp32"])):
        mx = np.abs(want).max()
        e2, e1 = np.abs(got2 - want).max() / mx, np.abs(got1 - want).max() / mx
        print(f"  {name}: piece {e2:.3e}  fp32 {e1:.3e}")
        assert e2 < 2e-5 and e2 <= 8.0 * e1 + 2e-6, (name, e2, e1)
    # rows with tiny upstream gradients keep their relative accuracy in dx (own scale per row)
    small = np.nonzero((np.abs(dg).max(1) > 0) & (np.abs(dg).max(1) < 1e-4))[0]
    got = flat(res["f16x2"])[0]
    for i in small[:50]:
        assert np.abs(got[i] - dx[i]).max() <= 2e-5 * np.abs(dx[i]).max() + 1e-30, i


def test_piece_backward_with_gradient_rows_spanning_decades_and_large_inputs(gpu_device, monkeypatch):
    """The dP rows go into the fp16 planes with a power-of-two scale of their own (a labelled atom's gradient next to rows 1e-6
    of it, and all-zero rows), the x operand of the dW product takes the inverse and — for a feature column with entries
    beyond 2^15 — a column scale.  Every gradient against float64, to 2e-5 of the tensor's largest entry and no worse than
    8 x the f32-input kernels on the same inputs (2^-21 against 2^-24; + rounding floor)."""
    _decades(gpu_device, monkeypatch, 1500)


def test_piece_backward_decades_and_large_inputs_over_two_trips(gpu_device, monkeypatch):
    """the same at a row count that gives workgroups a second tile, with a second large column that sits in the second 32-row
    step of one tile only (a tile some workgroup meets on its second trip)"""
    cu = num_cu(gpu_device)
    N = rows_for("b2mix", gpu_device)
    _decades(gpu_device, monkeypatch, N, step1_tile=cu + 3)
