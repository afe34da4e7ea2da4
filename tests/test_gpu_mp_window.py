"""The F = 64 window kernels of the MPLayer (csrc/mp_win.hip, mp_win_bwd.hip, mp_win16.hip, mp_win16_bwd.hip, mp_wave.hip)
through the C ABI against the float64 statement of tests/mp_layer_ref.py, element by element and by a statistic.

Every output is filled with NaN before the call.  Inputs are rounded to float32 first.  Two criteria per output:
  per element   |got - ref| <= C_REL * mag + 1e-7 * max(mag), C_REL = 3e-5 (the bound of test_gpu_mp_generic.py).  For dw the
                chain of float32 additions into one element runs over atoms: the node kernel (mp_win_bwd_node_kernel) keeps
                one MFMA accumulator per workgroup over its whole run of tiles_per_wg 32-atom tiles, then reduce_partials
                adds the `grid` partials of the workgroups one after the other.  chain = 32 * tiles_per_wg + grid; the bound
                uses max(C_REL, chain * 2^-24) (dw_chain below; 288 + 244 = 532 -> 3.2e-5 at N = 69985 on 256 CUs).
  statistical   r = rms(got - ref) / rms(mag) <= sqrt(r32 * r_drop), both numbers from the CPU emulations of mp_layer_ref.py
                (float32 evaluation; float64 with the `lo x hi` piece product of one operand missing: A in P = inv * (A Wp),
                dP in dA = dP Wp^T, B in dh = dH + B Wn, B in dw = h^T B).  Asserted where the arithmetic is products and sums
                (activation none and relu) on s_save, h_out, dh_in, de and dw of every kernel body; printed for softplus and
                tanh.  A_save comes from the aggregate kernel (float32 FMAs, no piece product): per element only.
                Not applied to the cases with N < 64: n1, n7, n15.  Every other case must give each tensor at least 4096
                selected elements, or it fails.

Variants (kernel bodies), each forward and backward against float64:
  wave  NG_MP_WAVE=1       mp_wave_fwd_kernel            + mp_win16_bwd_edge_kernel + mp_win_bwd_node_kernel
  w16   NG_MP_WAVE=0       mp_win16_fwd_kernel           + the same
  w8    NG_MP_W16=0        mp_win_fwd_kernel<E, K4, 1>   + mp_win_bwd_edge_kernel<E, 1> + node
  f32   NG_GEMM_MATH=fp32  mp_win_fwd_kernel<E, K4, 0>   + <E, 0> edge and node bodies
  the `guard` case (|2^8 w| >= 65504) reaches the f32-input body inside each guarded kernel of wave / w16 / w8.
K in 17..32 or K % 4 != 0: window forward (win_gather with K4 true and false) and the generic backward in one layer, with the
aggregate kept as ng_mp_layer_wants_aggregate asks.

Run lengths follow the library's own rule (win_tiles_per_wg): the N of the cases long, two32, two64 and one
is searched from the device's compute-unit count (n_with) and the length reached is asserted.  The wave kernel walks 256-atom
groups of a run of win_tiles_per_wg * 64 atoms: on 256 CUs that is a part of one group below N = 16384 and two groups
(256 + 64 atoms) at N = 69985.  A fifth (partial) group per workgroup needs more than 1024 atoms per run, N > 262,144 on 256 CUs,
five whole ones N > 311,296: beyond the size this file may use, so that length is not reached.
The forward kernels' power-of-two row scale (aggregates that reach 2^15) is the subject of test_gpu_mp_range.py and
test_gpu_mp_wave.py ("features") and is not repeated here.

Window model used by the asserts (window_walk, wave_walk): the eight-wave kernels (32-atom tiles) take a tile's row range over ALL
slots, dead ones and the zero index of the slots beyond N of a ragged last tile included (WinLists::issue / commit); the
sixteen-wave kernels (64-atom tiles) clamp those rows to row N - 1 instead, so their ragged tail stays in its window (window_walk
takes the rule of the tile size it is asked for); the wave kernel places a window around each
256-atom group without looking at the lists and checks each 16-atom micro-tile against it.

Found by these tests (no kernel change needed):
  test_a_source_from_memory_...[w8], [f32]   mp_win_fwd_kernel adds an atom's entries in rotation order from the window and in list
      order from memory: it does not keep the bits of unchanged atoms when their tile flips; held to the float64 bound there.
Sharpness, on scratch libraries: without the `wh x xl` MFMA of mp_win16_fwd_kernel r(s_save) of `long` is 7.477e-6 = r_drop to
four digits (threshold 2.6e-7; the per-element bound catches 261 of 4.5 M elements) and the 22 cases that run it fail; with relu's slope
replaced by softplus's in mp_win16_bwd_edge_kernel the 17 relu cases that run it fail."""
import numpy as np
import pytest

from mp_layer_gpu import GpuLayer, de_slots
from mp_layer_ref import ACT, C_REL, STAT_KEYS, STAT_MIN, check, f32, layer_stats, ref_layer, rstat

pytestmark = pytest.mark.gpu

F = 64
WROWS = 288
NREC_CAP = 768
VARIANTS = {"wave": {"NG_MP_WAVE": "1"}, "w16": {"NG_MP_WAVE": "0"}, "w8": {"NG_MP_W16": "0"}, "f32": {"NG_GEMM_MATH": "fp32"}}
ALL4 = ("wave", "w16", "w8", "f32")
WIN3 = ("w16", "w8", "f32")
OUT_NAME = {"s": "s_save", "h_out": "h_out", "dh": "dh_in", "de": "de", "dw": "dw"}


# ------------------------------------------------------------------------------------- the library's run-length rule
def cdiv(a, b):
    return -(-a // b)


def tiles_per_wg(ntiles, num_cu, first_align):
    """win_tiles_per_wg of csrc/ng_internal.h: first_align 8 for 32-atom tiles, 4 for 64-atom tiles"""
    base = max(cdiv(ntiles, num_cu), 1)
    want = min(num_cu, ntiles)
    align = first_align
    while align > 1:
        per = cdiv(base, align) * align
        if cdiv(ntiles, per) * 10 >= want * 9:
            return per
        align >>= 1
    return base


def runs(N, num_cu):
    """tiles per workgroup of the 32-atom kernels, of the 64-atom kernels, and 256-atom groups per workgroup of the wave kernel"""
    p32 = tiles_per_wg(cdiv(N, 32), num_cu, 8)
    p64 = tiles_per_wg(cdiv(N, 64), num_cu, 4)
    return min(p32, cdiv(N, 32)), min(p64, cdiv(N, 64)), cdiv(min(p64 * 64, N), 256)


def n_with(want, rem, lo=64, hi=72000):
    """the smallest N >= lo with N % 64 == rem whose run lengths satisfy `want`, for the device's compute-unit count; hi: the size
    this file may use (N of about 70,000)"""
    def find(num_cu):
        for N in range(lo - lo % 64 + rem, hi, 64):
            if N >= max(lo, 1) and want(*runs(N, num_cu)):
                return N
        raise AssertionError(f"no N below {hi} reaches the wanted run length on {num_cu} compute units")
    return find


def dw_chain(N, num_cu):
    p32 = tiles_per_wg(cdiv(N, 32), num_cu, 8)
    return 32 * p32 + cdiv(cdiv(N, 32), p32)


def used_lists(case):
    """the indices the kernels are handed: the compute-side list points dead slots at their own atom"""
    if case.get("raw_lists"):
        return case["nl"]
    return np.where(case["live"], case["nl"], np.arange(case["N"], dtype=np.int32)[:, None])


def window_walk(nl, N, T, per):
    """win_decide over every run of `per` tiles of T atoms: per tile (width over ALL slots, mode, restaged, wlo).  T = 32, the
    eight-wave kernels: the slots beyond N of a ragged last tile count as index 0.  T = 64, the sixteen-wave kernels: those rows
    are read as row N - 1, which the tile holds anyway."""
    out = []
    ntiles = cdiv(N, T)
    for t0 in range(0, ntiles, per):
        wlo = -(1 << 30)
        for t in range(t0, min(t0 + per, ntiles)):
            rows = nl[t * T:(t + 1) * T]
            lo, hi = int(rows.min()), int(rows.max())
            if T == 32 and (t + 1) * T > N:
                lo = min(lo, 0)
            mode, restaged = 0, False
            if not (lo >= wlo and hi < wlo + WROWS):
                if hi - lo + 1 > WROWS:
                    mode = 1
                else:
                    wlo = max(0, lo - (WROWS - (hi - lo + 1)) // 2)
                    restaged = True
            out.append((hi - lo + 1, mode, restaged, wlo))
    return out


def wave_walk(nl, N, apw):
    """mp_wave.hip: per 16-atom micro-tile, do its sources lie in the window its 256-atom group placed around its own rows?"""
    out = []
    for a0 in range(0, N, apw):
        a1 = min(a0 + apw, N)
        for g0 in range(a0, a1, 256):
            wlo = max(0, min(g0 - (WROWS - 256) // 2, N - WROWS))
            for r0 in range(g0, min(g0 + 256, a1), 16):
                rows = nl[r0:min(r0 + 16, N)]
                out.append((r0, wlo, bool(rows.min() >= wlo and rows.max() < wlo + WROWS)))
    return out


# ------------------------------------------------------------------------------------------------------- list builders
def local(spread):
    def build(rng, N, K, cu):
        return np.clip(np.arange(N)[:, None] + rng.integers(-spread, spread + 1, (N, K)), 0, N - 1), {}
    return build


def exact(width):
    """every 32-atom tile (and 64-atom tile) spans exactly `width` rows: 288 fits the window, 289 must gather from memory; the
    range creeps by 64 rows per tile, so a window that fits is restaged at every tile"""
    def build(rng, N, K, cu):
        t64 = np.arange(N) // 64
        lo = np.clip(t64 * 64 - (width - 64) // 2, 0, N - width)
        nl = lo[:, None] + rng.integers(0, width, (N, K))
        first = np.arange(0, N, 32)
        nl[first, 0], nl[first, 1] = lo[first], lo[first] + width - 1
        return nl, {"force_live": (first, (0, 1)), "width": width}
    return build


def wave_exact(over):
    """every micro-tile of the wave kernel touches row wlo and row wlo + 287 of its group's window; with `over` every second one
    reaches one row beyond it (wlo + 288, or wlo - 1 where the window ends at row N)"""
    def build(rng, N, K, cu):
        apw = tiles_per_wg(cdiv(N, 64), cu, 4) * 64
        nl = np.zeros((N, K), np.int64)
        first, out_rows = [], []
        for r0, wlo, _ in wave_walk(nl, N, apw):
            r1 = min(r0 + 16, N)
            nl[r0:r1] = wlo + rng.integers(0, WROWS, (r1 - r0, K))
            nl[r0, 0], nl[r0, 1] = wlo, wlo + WROWS - 1
            if over and (r0 // 16) % 2:
                nl[r0, 1] = wlo + WROWS if wlo + WROWS < N else wlo - 1
                out_rows.append(r0)
            first.append(r0)
        return nl, {"force_live": (np.array(first), (0, 1)), "wave_out": out_rows, "apw": apw}
    return build


def hub(total, near=False):
    """the 32-atom tile of rows 96 .. 127 receives exactly `total` live records: row 97 a fifth of them (in-degree far above 16),
    rows 98 .. 100 none, the rest spread over the other rows; atom 5 lists one source K times; atom 11 has no live slot.
    The records' sources lie all over the batch (the node kernel's tile gathers dP rows from memory) or, with `near`, within the
    first 288 rows (the tile stays in window mode, so the staging limit is crossed on the window path too)"""
    def build(rng, N, K, cu):
        nl = np.clip(np.arange(N)[:, None] + rng.integers(-60, 61, (N, K)), 0, N - 1)
        nl[(nl >= 96) & (nl < 128)] += 32
        nl[5, :] = 9
        return nl, {"hub": total, "near": near}
    return build


def finish_hub(case, rng, total, near):
    nl, live = case["nl"], case["live"]
    live[5, :] = True
    live[11, :] = False
    slots = np.flatnonzero(live.reshape(-1))
    slots = slots[(slots // case["K"] != 5)]
    if near:
        slots = slots[slots // case["K"] < WROWS]
    pick = rng.choice(slots, total, replace=False)
    others = np.array([r for r in range(96, 128) if r not in (97, 98, 99, 100)])
    tgt = others[rng.integers(0, len(others), total)]
    tgt[:total // 5] = 97
    nl.reshape(-1)[pick] = tgt


# --------------------------------------------------------------------------------------------------------------- cases
CASES = [
    # name, N, K, E, act, residual, lists, variants                       meant to reach
    ("long", n_with(lambda a, b, g: a >= 5 and b >= 5 and g >= 2, 33, lo=69950), 16, 3, "none", 1, local(100), ALL4),
    #                                                         # runs of >= 5 tiles (32- and 64-atom), two wave groups; N % 64 = 33
    #                                                           (69985 on 256 CUs)
    ("two32", n_with(lambda a, b, g: a == 2, 1), 12, 3, "relu", 0, local(60), ALL4),      # exactly two 32-atom tiles per workgroup; N % 64 = 1; K = 12
    ("two64", n_with(lambda a, b, g: b == 2, 31), 8, 2, "relu", 1, local(60), WIN3),      # exactly two 64-atom tiles per workgroup; N % 64 = 31; E = 2, K = 8
    ("one", n_with(lambda a, b, g: (a, b, g) == (1, 1, 1), 0, lo=1536), 16, 3, "softplus", 1, local(60), ALL4),   # one tile per workgroup; softplus epilogue; window clamped at row 0
    #                                                           and hanging over row N
    ("tanh", 1000, 16, 3, "tanh", 0, local(60), ALL4),        # epilogue branch act != none, != softplus; residual = 0
    ("relu_e1", 2100, 4, 1, "relu", 1, local(30), WIN3),      # E = 1, K = 4
    ("k4_e3", 2500, 4, 3, "relu", 0, local(30), ALL4),        # K = 4 at E = 3: one quad per atom in the wave kernel's strips (nq = 1)
    ("none_e2", 2083, 12, 2, "none", 0, local(40), WIN3),     # E = 2, K = 12, residual = 0 without activation
    ("tanh_e1", 700, 8, 1, "tanh", 1, local(40), WIN3),       # tanh slope 1 - S^2 in the E = 1 edge bodies
    ("n1", 1, 4, 3, "none", 1, local(0), ALL4),               # N = 1
    ("n7", 7, 8, 3, "relu", 0, local(3), ALL4),               # N below one micro-tile of 16
    ("n15", 15, 16, 1, "softplus", 1, local(7), WIN3),        # the same at E = 1
    ("fits288", 40005, 16, 3, "none", 1, exact(288), WIN3),   # win_decide: range exactly 288 rows: window; runs of 5 and 3
    #                                                           tiles whose range creeps: restaged at every 64-atom tile
    ("wide289", 1029, 16, 3, "relu", 1, exact(289), WIN3),    # win_decide: 289 rows: every tile gathers from memory
    ("far_tail", 5003, 16, 3, "none", 0, exact(200), WIN3),   # ragged last tile far from row 0: its zero-filled slots force memory
    #                                                           in the eight-wave kernels; the sixteen-wave ones stay in the window
    ("wv_fits", 1200, 16, 3, "none", 1, wave_exact(0), ("wave",)),   # wave: rows wlo and wlo + 287 of the group window
    ("wv_over", 1200, 8, 3, "relu", 0, wave_exact(1), ("wave",)),    # wave: every second micro-tile one row outside: from memory
    ("raw", 3000, 16, 3, "relu", 1, local(60), ALL4),         # raw padded list: dead slots at row 0, N - 1, anywhere: memory gather
    ("hub767", 700, 16, 3, "none", 1, hub(NREC_CAP - 1), ("w16", "f32")),     # node kernel: records of a tile one below the staging limit
    ("hub768", 700, 16, 3, "relu", 1, hub(NREC_CAP), ("w16", "f32")),     # exactly NREC_CAP
    ("hub769", 700, 16, 3, "none", 0, hub(NREC_CAP + 1), ("w16", "f32")),     # one above: records read from memory
    ("hub768w", 700, 16, 3, "relu", 0, hub(NREC_CAP, True), ("w16", "f32")),    # NREC_CAP with the sources inside one window
    ("hub769w", 700, 16, 3, "none", 1, hub(NREC_CAP + 1, True), ("w16", "f32")),    # one above, leaving the window path
    ("hub5000", 700, 16, 3, "relu", 1, hub(5000), ("w16", "w8", "f32")),   # far above; in-degree 1000 next to in-degree 0
    ("k1", 2000, 1, 3, "relu", 1, local(40), WIN3),            # K = 1: scalar list loads (K4 false); generic backward
    ("k5", 601, 5, 2, "none", 0, local(40), WIN3),            # K = 5
    ("k7", 1000, 7, 1, "tanh", 1, local(40), WIN3),            # K = 7
    ("k13", 2000, 13, 3, "softplus", 0, local(40), WIN3),     # K = 13
    ("k20", 1000, 20, 3, "relu", 1, local(60), ("w8", "f32")),       # K = 20 > 16: eight-wave forward by dispatch, K4 true
    ("k32", 777, 32, 2, "none", 1, local(60), ("w8", "f32")),        # K = 32, the largest the window forward takes
    ("guard", 1500, 16, 3, "relu", 1, local(60), ("wave", "w16", "w8")),   # weights beyond the piece range: f32-input bodies
    ("guard_e1", 900, 8, 1, "none", 0, local(40), ("w16", "w8")),    # the same at E = 1
]
CASE = {c[0]: c for c in CASES}
SMALL = ("n1", "n7", "n15")                                   # per-element bound alone (N < 64)


def build_case(name, num_cu):
    _, N, K, E, act, residual, lists, _ = CASE[name]
    N = N(num_cu) if callable(N) else N
    rng = np.random.default_rng(sum(map(ord, name)) * 1000 + N)
    nl, info = lists(rng, N, K, num_cu)
    live = rng.random((N, K)) >= 0.1
    if "force_live" in info:
        rows, cols = info["force_live"]
        for c in cols:
            live[rows, c] = True
    case = dict(kind="padded", F=F, E=E, K=K, N=N, span=0, act=ACT[act], residual=residual, nl=nl.astype(np.int32), live=live,
                info=info, name=name)
    if "hub" in info:
        finish_hub(case, rng, info["hub"], info["near"])
    if name == "raw":
        dead = ~live
        where = rng.integers(0, 3, (N, K))
        nl = case["nl"]
        nl[dead & (where == 0)] = 0
        nl[dead & (where == 1)] = N - 1
        nl[dead & (where == 2)] = rng.integers(0, N, int((dead & (where == 2)).sum()))
        case["raw_lists"] = True
    live = case["live"]
    case["e"] = f32(rng.standard_normal((N, K, E)) * np.where(live, 1.0, 0.0)[:, :, None])
    case["h"] = f32(rng.standard_normal((N, F)) * 0.5)
    case["inv"] = f32(rng.uniform(0.05, 1.0, N))
    case["w"] = f32(rng.standard_normal((F, F, E)) / np.sqrt(F * E * K))
    case["dH"] = f32(rng.standard_normal((N, F)))
    if name.startswith("guard"):
        case["w"][3, 5, 0] = 400.0                   # 2^8 w = 102400: no fp16 piece holds it
        case["w"][40, 63, E - 1] = -300.0
    assert case["nl"].min() >= 0 and case["nl"].max() < N
    return case


def assert_branch(case, num_cu):
    """the quantity each case was built for"""
    name, N, info = case["name"], case["N"], case["info"]
    p32, p64, groups = runs(N, num_cu)
    nl = used_lists(case)
    if name == "long":
        assert p32 >= 5 and p64 >= 5 and groups >= 2 and N % 64 == 33, (p32, p64, groups)
    if name == "two32":
        assert p32 == 2 and N % 64 == 1, (p32, p64, groups)
    if name == "two64":
        assert p64 == 2 and N % 64 == 31, (p32, p64, groups)
    if name == "one":
        assert (p32, p64, groups) == (1, 1, 1)
    if name == "one":
        w = window_walk(nl, N, 64, p64)
        assert w[0][3] == 0 and w[0][2] and w[-1][2] and w[-1][3] + WROWS > N       # clamped at row 0; hangs over row N
    if "width" in info:
        for T, per in ((32, p32), (64, p64)):
            w = window_walk(nl, N, T, per)
            full = w[:N // T]
            if name == "fits288":
                # the two 32-atom tiles of a 64-atom tile share their range: the second one is a window hit
                assert per >= 3 and all(x[0] == 288 and x[1] == 0 for x in full), T
                assert sum(x[2] for x in full) >= len(full) * T // 64 - 6, T
            elif name == "wide289":
                assert all(x[0] == 289 and x[1] == 1 for x in full), T
            else:
                # only the ragged tail of the eight-wave kernels leaves the window
                assert N % T and w[-1][1] == (1 if T == 32 else 0) and all(x[1] == 0 for x in full), T
    if "apw" in info:
        w = wave_walk(nl, N, info["apw"])
        outside = [r0 for r0, _, ok in w if not ok]
        assert outside == info["wave_out"] and (len(outside) > 10) == (name == "wv_over")
        assert all(nl[r0:r0 + 16].min() == wlo for r0, wlo, ok in w if ok)
    if name == "raw":
        assert sum(x[1] for x in window_walk(nl, N, 64, p64)) > N // 64 // 2            # most tiles gather from memory
    if "hub" in info:
        tgt = case["nl"][case["live"]]
        assert int(((tgt >= 96) & (tgt < 128)).sum()) == info["hub"]
        deg = np.bincount(tgt, minlength=N)
        assert deg[97] == info["hub"] // 5 and (deg[98:101] == 0).all()
        src = np.nonzero(case["live"] & (case["nl"] >= 96) & (case["nl"] < 128))[0]
        assert (int(src.max() - src.min()) + 1 <= WROWS) == info["near"]      # the node tile's window decision
        assert not case["live"][11].any() and (case["nl"][5] == 9).all()


# ------------------------------------------------------------------------------------------- reference, once per case
_SLOT = {"name": None}


def reference(name, num_cu, stats=False):
    """case, float64 values, magnitudes (and the two emulated statistics) of the case — kept for the variants that follow"""
    if _SLOT["name"] != name:
        _SLOT.clear()
        case = build_case(name, num_cu)
        assert_branch(case, num_cu)
        v, mg = ref_layer(case["h"], case["nl"], case["e"], case["inv"], case["w"], case["dH"], case["act"], case["residual"])
        _SLOT.update(name=name, case=case, v=v, mg=mg, st=None)
    s = _SLOT
    if stats and s["st"] is None:
        c = s["case"]
        s["st"] = layer_stats(c["h"], c["nl"], c["e"], c["inv"], c["w"], c["dH"], c["act"], c["residual"], s["v"], s["mg"], c["live"])
    return s["case"], s["v"], s["mg"], s["st"]


def num_cu_of(dev):
    import torch
    return torch.cuda.get_device_properties(dev).multi_processor_count


def set_variant(monkeypatch, variant):
    for k, val in VARIANTS[variant].items():
        monkeypatch.setenv(k, val)


def window_backward(case):
    return case["K"] % 4 == 0 and 4 <= case["K"] <= 16


def run_layer(g, v):
    """forward, and the backward handed the reference's s_save (float64 S rounded to float32) and the forward's aggregate"""
    import torch
    c = g.c
    wants_A = bool(g.ctx.lib.ng_mp_layer_wants_aggregate(c["F"], c["E"], c["K"]))
    assert wants_A == (not window_backward(c))
    h_out, A, s = g.fwd()
    dh, de, dw = g.bwd(A if wants_A else None, g.t(v["s_in"]), g.t(c["dH"]))
    torch.cuda.synchronize()
    return {"h_out": h_out.cpu().numpy(), "A": A.cpu().numpy(), "s": s.cpu().numpy(), "dh": dh.cpu().numpy(),
            "de": de_slots(c, de), "dw": dw.cpu().numpy()}


PAIRS = [(c[0], var) for c in CASES for var in c[7]]


@pytest.mark.parametrize("name,variant", PAIRS)
def test_window_layer_vs_float64(gpu_device, monkeypatch, name, variant):
    """every element of h_out, s_save, A_save, dh_in, de (live slots) and dw within the float64 bound, and (activation none /
    relu, N >= 64) the statistic r of each output below sqrt(r32 * r_drop); prints r, r32, r_drop per output"""
    cu = num_cu_of(gpu_device)
    stat_case = name not in SMALL
    case, v, mg, st = reference(name, cu, stats=stat_case)
    assert (case["N"] < 64) == (not stat_case)
    set_variant(monkeypatch, variant)
    got = run_layer(GpuLayer(case, gpu_device), v)
    live = case["live"]
    if "hub" in case["info"]:
        assert (got["A"][11] == 0).all() and (v["A"][11] == 0).all()                # no live slot: A = 0
    c_dw = max(C_REL, dw_chain(case["N"], cu) * 2.0 ** -24) if window_backward(case) else C_REL
    failures = []
    for key in ("h_out", "s", "A", "dh", "de", "dw"):
        sel = live if key == "de" else None
        try:
            check(OUT_NAME.get(key, "A_save"), got[key], v[key], mg[key], sel=sel, c_rel=c_dw if key == "dw" else C_REL)
        except AssertionError as err:
            failures.append(str(err))
    if stat_case:
        for key in STAT_KEYS:
            sel = live if key == "de" else None
            n_sel = int(live.sum()) * case["E"] if key == "de" else got[key].size
            r = rstat(got[key], v[key], mg[key], sel)
            r32, r_drop = st[key]
            thr = float(np.sqrt(r32 * r_drop))
            assert n_sel >= STAT_MIN, f"{name}: {OUT_NAME[key]} has {n_sel} selected elements, too few to carry the statistic"
            asserted = case["act"] in (ACT["none"], ACT["relu"])
            print(f"RSTAT {name:9s} {variant:4s} {OUT_NAME[key]:6s} r {r:.3e} r32 {r32:.3e} r_drop {r_drop:.3e} thr {thr:.3e} "
                  f"{'assert' if asserted else 'print'}{'  WITHIN 2x' if asserted and 2 * r > thr else ''}")
            if asserted and not r <= thr:
                failures.append(f"{OUT_NAME[key]}: r = {r:.3e} above sqrt(r32 * r_drop) = {thr:.3e} (r32 {r32:.3e}, r_drop {r_drop:.3e})")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------ call forms
def _mid_case(cu, act="relu"):
    c = build_case("raw", cu)
    c.pop("raw_lists")
    c["act"] = ACT[act]
    return c


@pytest.mark.parametrize("variant", ["w16", "w8", "f32"])
def test_call_forms_give_the_same_bits(gpu_device, monkeypatch, variant):
    """records supplied == rebuilt; de_accum: de1 == prior + de0 with one rounding; dw = NULL leaves dh_in and de alone; dw
    after the flush of an ng_defer_reductions window == the undeferred dw — all bit for bit"""
    import torch
    cu = num_cu_of(gpu_device)
    case = _mid_case(cu)
    set_variant(monkeypatch, variant)
    g = GpuLayer(case, gpu_device)
    live = torch.from_numpy(case["live"].reshape(-1)).to(gpu_device)
    _, _, S = g.fwd()
    dH = g.t(case["dH"])
    dh, de, dw = g.bwd(None, S, dH)
    assert bool(torch.isfinite(dh).all() and torch.isfinite(dw).all() and torch.isfinite(de[live]).all())
    dh2, de2, dw2 = g.bwd(None, S, dH, rec=g.records())
    assert torch.equal(dh2, dh) and torch.equal(dw2, dw) and torch.equal(de2[live], de[live])
    prior = g.t(np.random.default_rng(1).standard_normal((g.n_ent, case["E"])))
    dh3, de3, dw3 = g.bwd(None, S, dH, de_prior=prior)
    assert torch.equal(de3[live], (prior + de)[live]) and torch.equal(dh3, dh) and torch.equal(dw3, dw)
    dh4, de4, dw4 = g.bwd(None, S, dH, want_dw=False)
    assert dw4 is None and torch.equal(dh4, dh) and torch.equal(de4[live], de[live])
    ctx = g.ctx
    ctx.check(ctx.lib.ng_defer_reductions(ctx.handle, g.st, 1), "defer")
    try:
        dh5, de5, dw5 = g.bwd(None, S, dH)
        ctx.check(ctx.lib.ng_flush_reductions(ctx.handle, g.st), "flush")
    finally:
        ctx.check(ctx.lib.ng_defer_reductions(ctx.handle, g.st, 0), "defer off")
    torch.cuda.synchronize()
    assert torch.equal(dw5, dw) and torch.equal(dh5, dh) and torch.equal(de5[live], de[live])


@pytest.mark.parametrize("variant", ["wave", "w16", "w8"])
def test_kept_weight_images_serve_both_bodies(gpu_device, monkeypatch, variant):
    """ng_weights_frozen: the second call, served from the kept image, repeats the first bit for bit (and the unfrozen call);
    then the weights leave the piece range (announced with ng_weights_changed): the f32-input bodies run from the kept image,
    twice the same bits, every element within the float64 bound of the new weights"""
    import torch
    cu = num_cu_of(gpu_device)
    case = _mid_case(cu)
    set_variant(monkeypatch, variant)
    g = GpuLayer(case, gpu_device)
    ctx = g.ctx
    live = torch.from_numpy(case["live"].reshape(-1)).to(gpu_device)
    dH = g.t(case["dH"])
    big = dict(case, w=case["w"].copy())
    big["w"][3, 5, 0], big["w"][40, 63, 2] = 400.0, -300.0
    refs = [ref_layer(c["h"], c["nl"], c["e"], c["inv"], c["w"], c["dH"], c["act"], c["residual"]) for c in (case, big)]

    def call(k):
        S = g.t(refs[k][0]["s_in"])
        h_out, _, s = g.fwd(keep_A=False)
        dh, de, dw = g.bwd(None, S, dH)
        torch.cuda.synchronize()
        return [h_out, s, dh, de[live], dw]

    free = call(0)
    # (an owner of its own per variant: the images are keyed by address, and the allocator hands this test's weight tensor the
    # address the previous variant's had)
    ctx.check(ctx.lib.ng_weights_frozen(ctx.handle, 515151 + ["wave", "w16", "w8"].index(variant)), "freeze")
    try:
        first, second = call(0), call(0)
        g.tw.copy_(g.t(big["w"]))
        ctx.check(ctx.lib.ng_weights_changed(ctx.handle), "changed")
        third, fourth = call(1), call(1)
    finally:
        ctx.check(ctx.lib.ng_weights_frozen(ctx.handle, 0), "thaw")
    for a, b, c in zip(free, first, second):
        assert torch.equal(a, b) and torch.equal(b, c)
    for a, b in zip(third, fourth):
        assert torch.equal(a, b)
    v, mg = refs[1]
    lv = case["live"]
    c_dw = max(C_REL, dw_chain(case["N"], cu) * 2.0 ** -24)
    check("h_out", third[0].cpu().numpy(), v["h_out"], mg["h_out"])
    check("s_save", third[1].cpu().numpy(), v["s"], mg["s"])
    check("dh_in", third[2].cpu().numpy(), v["dh"], mg["dh"])
    check("de", third[3].cpu().numpy().astype(np.float64), v["de"][lv], mg["de"][lv])
    check("dw", third[4].cpu().numpy(), v["dw"], mg["dw"], c_rel=c_dw)


@pytest.mark.parametrize("shift", [-20, 12])
def test_long_run_backward_scales_exactly_with_the_upstream_gradient(gpu_device, shift):
    """the long-run case (>= 5 tiles per workgroup): dH * 2^shift gives dh_in (hence dh_in - dH), de and dw times 2^shift bit
    for bit — the per-row power-of-two scales of the piece operands and the per-tile scale of the dw product cancel exactly"""
    import torch
    cu = num_cu_of(gpu_device)
    case, v, _, _ = reference("long", cu)
    g = GpuLayer(case, gpu_device)
    S = g.t(v["s_in"])
    base = g.bwd(None, S, g.t(case["dH"]))
    moved = g.bwd(None, S, g.t(case["dH"] * 2.0 ** shift))
    torch.cuda.synchronize()
    live = torch.from_numpy(case["live"].reshape(-1)).to(gpu_device)
    for k, (a, b) in enumerate(zip(moved, base)):
        if k == 1:
            a, b = a[live], b[live]
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(a, b * 2.0 ** shift), k


# ------------------------------------------------------------------------------------------------ window against memory
@pytest.mark.parametrize("variant", ["wave", "w16", "w8", "f32"])
def test_a_source_from_memory_gives_the_sum_of_one_from_the_window(gpu_device, monkeypatch, variant):
    """a case in window mode; then one live neighbour of one atom per 64-atom tile moves far away, which flips its tile (its
    wave micro-tile) to the memory gather.  The kernels promise the same sums in the same order from either source
    (mp_wave.hip header; mp_win16.hip gather / gather_global; the edge dots of both backward kernels): every atom whose list did not change keeps the bits
    of h_out, s_save and de.  dh_in: the node kernel sums a target's records in CSC order from either source, so every row
    that neither lost nor gained a record keeps its bits too."""
    import torch
    cu = num_cu_of(gpu_device)
    N, K, E = 4099, 16, 3
    rng = np.random.default_rng(77)
    nl = np.clip(np.arange(N)[:, None] + rng.integers(-16, 17, (N, K)), 0, N - 1).astype(np.int32)
    live = rng.random((N, K)) >= 0.1
    movers = np.arange(5, N - 64, 64)
    live[movers, 3] = True
    base = dict(kind="padded", F=F, E=E, K=K, N=N, span=0, act=ACT["relu"], residual=1, nl=nl, live=live, info={}, name="wm",
                e=f32(rng.standard_normal((N, K, E)) * live[:, :, None]), h=f32(rng.standard_normal((N, F)) * 0.5),
                inv=f32(rng.uniform(0.05, 1.0, N)), w=f32(rng.standard_normal((F, F, E)) / np.sqrt(F * E * K)),
                dH=f32(rng.standard_normal((N, F))))
    moved = dict(base, nl=nl.copy())
    old = nl[movers, 3].copy()
    new = ((movers + 1500) % N).astype(np.int32)
    moved["nl"][movers, 3] = new
    p32, p64, _ = runs(N, cu)
    apw = p64 * 64
    for T, per in ((32, p32), (64, p64)):
        full = N // T
        assert not any(x[1] for x in window_walk(used_lists(base), N, T, per)[:full])
        flipped = [x[1] for x in window_walk(used_lists(moved), N, T, per)]
        assert all(flipped[m // T] == 1 for m in movers)
    assert all(ok for r0, _, ok in wave_walk(used_lists(base), N, apw) if r0 + 16 <= N)
    assert not any(ok for r0, _, ok in wave_walk(used_lists(moved), N, apw) if ((r0 <= movers) & (movers < r0 + 16)).any())
    set_variant(monkeypatch, variant)
    v, _ = ref_layer(base["h"], base["nl"], base["e"], base["inv"], base["w"], base["dH"], base["act"], 1)
    outs = []
    for c in (base, moved):
        g = GpuLayer(c, gpu_device)
        h_out, _, s = g.fwd(keep_A=False)
        dh, de, _ = g.bwd(None, g.t(v["s_in"]), g.t(c["dH"]))      # the same s_save for both: dP does not move
        torch.cuda.synchronize()
        outs.append((h_out.cpu().numpy(), s.cpu().numpy(), dh.cpu().numpy(), de.cpu().numpy().reshape(N, K, E)))
    same_atom = np.ones(N, bool)
    same_atom[movers] = False
    same_row = np.ones(N, bool)
    same_row[old] = False
    same_row[new] = False
    a, b = outs
    if variant in ("wave", "w16"):
        assert np.array_equal(a[0][same_atom], b[0][same_atom]) and np.array_equal(a[1][same_atom], b[1][same_atom])
    else:
        # mp_win_fwd_kernel does not promise it for K <= 16: from the window it adds an atom's entries in rotation order
        # (win_gather_rot: lane c starts at slot c), from memory in list order (win_gather_global).  Found by this test; the
        # unchanged atoms of a flipped tile differ in the last bit and are held to the float64 bound instead.
        for c, o in ((base, a), (moved, b)):
            vv, mm = ref_layer(c["h"], c["nl"], c["e"], c["inv"], c["w"], c["dH"], c["act"], 1)
            check("h_out", o[0], vv["h_out"], mm["h_out"])
            check("s_save", o[1], vv["s"], mm["s"])
        calm = np.ones(N, bool)                                     # atoms of tiles that did not flip keep their bits
        for m in movers:
            calm[m // 32 * 32:m // 32 * 32 + 32] = False
        assert np.array_equal(a[0][calm], b[0][calm]) and np.array_equal(a[1][calm], b[1][calm])
    keep = live & same_atom[:, None]
    assert np.array_equal(a[3][keep], b[3][keep])
    assert np.array_equal(a[2][same_row], b[2][same_row])
    assert not np.array_equal(a[0][movers], b[0][movers])          # and the moved sources did change their atoms


@pytest.mark.parametrize("variant", ["wave", "w16"])
def test_raw_and_compute_side_lists_give_the_same_bits(gpu_device, monkeypatch, variant):
    """the `raw` case (dead slots at row 0, row N - 1, anywhere: most tiles gather from memory) against the same lists in the
    engine's compute-side form (dead slots at their own atom: every tile in its window).  A dead slot adds 0 * h[row] in list
    order in either form, so where the kernels promise the same sums from window and memory (the wave and sixteen-wave forward,
    both backward kernels) h_out, s_save, dh_in, dw and de on live slots keep their bits.  The eight-wave forward makes no such
    promise (see the test above); both of its forms are held to float64 in test_window_layer_vs_float64[raw-*] and [one-*]."""
    import torch
    cu = num_cu_of(gpu_device)
    raw = build_case("raw", cu)
    side = dict(raw)
    side.pop("raw_lists")
    p32, p64, _ = runs(raw["N"], cu)
    assert not any(x[1] for x in window_walk(used_lists(side), raw["N"], 64, p64)[:raw["N"] // 64])
    assert sum(x[1] for x in window_walk(used_lists(raw), raw["N"], 64, p64)) > raw["N"] // 128
    set_variant(monkeypatch, variant)
    v, _ = ref_layer(raw["h"], raw["nl"], raw["e"], raw["inv"], raw["w"], raw["dH"], raw["act"], raw["residual"])
    live = torch.from_numpy(raw["live"].reshape(-1)).to(gpu_device)
    outs = []
    for c in (raw, side):
        g = GpuLayer(c, gpu_device)
        h_out, _, s = g.fwd(keep_A=False)
        dh, de, dw = g.bwd(None, g.t(v["s_in"]), g.t(c["dH"]))
        torch.cuda.synchronize()
        outs.append((h_out, s, dh, de[live], dw))
    for k, (a, b) in enumerate(zip(*outs)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), k
