"""One MPLayer at the reference's default width (atom_feature_size = 256) through the C entry points ng_mp_layer_fwd[_csr],
ng_mp_layer_bwd[_rec|_csr], ng_mp_aggregate[_csr] and ng_mp_edge_records, against the float64 statement of tests/mp_layer_ref.py.
The kernels that serve no other width: the two-slab agg_win_kernel / egrad_win_kernel (mp_win.hip), pull_win_kernel<1|2|3>,
csr_edge_grad_wide_kernel<E,16> / csr_scatter_pull_wide_kernel<E,16> and mp_dp_kernel (mp_csr.hip), and the window gather-GEMM
mp_gw_kernel<PADDED|CSR|REC, 3, GRAD, 6|8> (mp_gg.hip).

Every output is filled with NaN before the call; the graph span is announced per case and reset behind it.  Two families:
  exact   inputs on coarse binary grids (mp_layer_ref.exact_inputs): every output must equal the float64 statement BIT FOR BIT —
          a dropped, doubled or misplaced entry, record, row block, slab, k-step or piece product cannot hide.  That the float64
          values are float32 numbers, that a float32 evaluation in any order reaches them and that the split-product operands
          fit two fp16 pieces is checked on the CPU for every exact case of this file (test_mp_layer_ref_host.py).
  normal  the random family of padded_case / csr_case: per element |got - ref| <= C_REL * mag + 1e-7 * max(mag) (check);
          where a split-operand product runs on at least STAT_MIN elements (dense_fwd / dense_dw / dense_dx at N >= 4096, the
          gather-GEMM at any N) also r = rms(got - ref) / rms(mag) <= sqrt(r32 * r_drop) (layer_stats; asserted for activation
          none / relu, printed for softplus / tanh, as in test_gpu_mp_window.py; de is left out where the call accumulates onto
          a prior, which the emulations do not model); where NG_GEMM_MATH=fp32 gives a second path, error <= 8 x that run + 1e-6.
de is compared on live slots only.  The backward is handed the reference's s_save (float64 S rounded to float32) and the aggregate
of ng_mp_aggregate, which the forward's A_save must equal bit for bit wherever both come from the aggregate kernels.

Dispatch, from the conditions in the sources (no hook needed; `span` = the announced graph span):
  forward, A kept       span in 1..272 and N >= 4096 -> agg_win_kernel (AW_ROWS = 272), else aggregate_kernel; then dense_fwd
  forward, A not kept   span in 1..256, N >= NG_MP_GG_MIN_ROWS (8192), E = 3, K <= 16 -> mp_gw_kernel<PADDED, 3, false, 6>;
                        NG_MP_GG=1 sends every E = 3 call there (CSR: <CSR, 3, false, 8>), A_save then a by-product
  backward de           padded, span in 1..272, N >= 4096 -> egrad_win_kernel, else csr_edge_grad_wide_kernel<E,16>
  backward dh           NG_MP_GG=1 (E = 3) -> mp_gw_kernel<REC, 3, true, 8>; else records given, span in 1..288, N >= 4096 ->
                        pull_win_kernel<E> (PW_SPAN = 288); else csr_scatter_pull_wide_kernel<E,16> (records, or the
                        csc_edge -> e chain without them and at E = 4)
  so at span 288 with records and N >= 4096 pull_win_kernel runs while de takes the wide kernel (272 < 288 <= 288).

Not reachable: mp_gg_repair_kernel<LK, 1|2> — gw_shape_ok demands E = 3, so only the E = 3 instantiations ever launch.
The range guard of the pull form (mp_gw_kernel<REC, 3, true, 8>): the gathered sums are scaled by S 2^-x with S the power-of-two
scale of max|dP| and 2^x >= the row's sum |e_n|, so every scaled sum is bounded by the fp16 range whatever finite dP and e hold;
only sum |e_n| >= 3e38 switches the row scale off, and there the result itself has left float32.  Nothing a test could state
in float64 raises it, so the repair of the pull form is not exercised here; the forward's is (range_* cases)."""
import zlib

import numpy as np
import pytest

from mp_layer_gpu import GpuLayer, de_slots
from mp_layer_ref import (ACT, EXACT_HUB, STAT_MIN, check, csr_case, exact_inputs, f32, host_records, layer_stats, padded_case,
                          ref_layer, rstat, sub_case)

pytestmark = pytest.mark.gpu

F = 256
PW_T, PW_REC, GW_BM, GW_CAPB = 256, 4096, 256, 480
EXACT_ACT = {"none": "none", "softplus": "none", "relu": "relu", "tanh": "relu"}
GG = {"NG_MP_GG": "1", "NG_MP_GG_MIN_ROWS": "1"}
OUT_NAME = {"s": "s_save", "h_out": "h_out", "A": "A_save", "A_only": "aggregate", "dh": "dh_in", "de": "de", "dw": "dw",
            "dh_perm": "dh_in (permuted records)"}


def S(**kw):
    d = dict(kind="padded", E=3, K=16, span=0, act="relu", res=1, fwd="train", bwd=None, accum=0, env={}, hub=0, p_dead=0.1,
             bias=None, tweaks=(), perm=False, fp32=False, big_h=False, scale=False, fams=("exact", "normal"))
    d.update(kw)
    return d


# --------------------------------------------------------------------------------------------------------------- list tweaks
def orphan(c):
    """target 5 has no incoming edge"""
    c["nl"][c["nl"] == 5] = 6


def lonely(c):
    """target 9 has exactly one incoming edge (sum |e_n| <= 1 in the exact family: the unscaled branch of the pull's row scale)"""
    hit = np.flatnonzero(((c["nl"] == 9) & c["live"]).reshape(-1))
    if len(hit):
        c["nl"].reshape(-1)[hit[1:]] = 10
    else:
        j = int(np.flatnonzero(c["live"][10])[0])
        c["nl"][10, j] = 9
    e = c["e"][c["live"] & (c["nl"] == 9)]
    e *= 0.25 / max(1.0, float(np.abs(e).max()))                 # (normal family; the exact family draws its own e)
    c["e"][c["live"] & (c["nl"] == 9)] = f32(e)


def one_dead(c):
    """graphs of 256 without dead slots give every 256-target tile exactly PW_REC records; this one slot of graph 2 leaves
    tile 2 with PW_REC - 1"""
    c["live"][2 * 256 + 3, 0] = False
    c["e"][2 * 256 + 3, 0] = 0.0


def first_graph_4097(c):
    """graph 0 has 257 atoms and no dead slot: 4112 records, of which exactly 15 go to its last atom: tile 0 (targets 0..255)
    receives PW_REC + 1"""
    rng = np.random.default_rng(1)
    blk = c["nl"][:257]
    at = blk == 256
    blk[at] = rng.integers(0, 256, int(at.sum()))
    blk.reshape(-1)[rng.choice(blk.size, 15, replace=False)] = 256


TWEAK = {"orphan": orphan, "lonely": lonely, "one_dead": one_dead, "first_graph_4097": first_graph_4097}


def small_degrees(rng, N):
    d = rng.integers(0, 21, N)
    d[:4] = [0, 1, 2, 17]
    return rng.permutation(d)


def tile_degrees(rng, N):
    """degrees 0..60 for the CSR gather-GEMM, by 256-row tile: tails (entries 16 and beyond) totalling exactly GW_CAPB = 480;
    481; 256 rows of degree 60 (far beyond the staging area); 256 empty rows; random 0..60 with a ragged last tile"""
    d = rng.integers(0, 61, N)
    d[:1024] = rng.integers(0, 17, 1024)
    d[0:48] = 26
    d[256:304] = 26
    d[304] = 17
    d[512:768] = 60
    d[768:1024] = 0
    return d


def tile_tails(deg):
    t = np.maximum(np.asarray(deg) - 16, 0)
    return [int(t[i:i + GW_BM].sum()) for i in range(0, len(t), GW_BM)]


def tile_records(case):
    """incoming-edge records per pull_win tile of 256 targets"""
    tgt = case["nl"][case["live"]]
    return np.bincount(tgt // PW_T, minlength=-(-case["N"] // PW_T))


# ----------------------------------------------------------------------------------------------------------------- cases
CASES = {
    # 1. aggregate_kernel<E> at F = 256 (span 0) -> dense_fwd; 7. backward at N < 4096: csr_edge_grad_wide_kernel<E,16> and
    #    csr_scatter_pull_wide_kernel<E,16>, with records and with the csc_edge -> e chain (bwd "both": same bits)
    "s33_e1": S(N=33, E=1, act="relu", bwd="both", accum=1),                 # aggregate_kernel<1>, wide <1,16>; ragged block
    "s700_e2": S(N=700, E=2, act="tanh", res=0, bwd="both"),                 # aggregate_kernel<2>, wide <2,16>
    "s700_e3k5": S(N=700, K=5, act="softplus", bwd="both", accum=1, tweaks=("orphan",)),   # aggregate_kernel<3>, K = 5; orphan target
    "s33_e3": S(N=33, act="none", res=0, bwd="both"),                        # act none: mp_dp_kernel with S = NULL
    "s700_e4": S(N=700, E=4, act="relu", bwd="none"),                        # wide <4,16>: the chain is the only source of e
    "s700_hub": S(N=700, act="relu", bwd="both", hub=3000),                  # one CSC segment of 3000 entries in the wide pull
    # 7. the same kernels over CSR lists (csr_aggregate_kernel; RowRange rows in the wide kernels)
    "c700_e1": S(kind="csr", N=700, E=1, act="softplus", deg=small_degrees, bwd="none"),
    "c700_e2hub": S(kind="csr", N=700, E=2, act="relu", res=0, deg=small_degrees, bwd="none", accum=1, hub=2500),
    "c700_e3": S(kind="csr", N=700, act="tanh", deg=small_degrees, bwd="none"),
    "c700_e4": S(kind="csr", N=700, E=4, act="none", deg=small_degrees, bwd="none"),
    # 2. agg_win_kernel<E>, two slabs (N >= 4096, span <= 272); 6. the default training backward with records: mp_dp_kernel ->
    #    dense_dw / dense_dx (split operands) -> egrad_win_kernel<E> -> pull_win_kernel<E>
    "w256": S(N=4351, span=256, act="relu", bwd="dev", accum=1, tweaks=("orphan",), perm=True, fp32=True),
    #         window hits (graph = window); N % 32 = 31, N % 256 = 255; de_accum = 1; permuted records: "behind the block"
    "w200": S(N=4097, E=2, K=8, span=200, act="softplus", res=0, bwd="dev", fp32=True),
    #         32-atom tiles straddle graphs: the slab window is restaged; N % 32 = 1, N % 256 = 1; <2> bodies
    "w272": S(N=4161, E=1, K=4, span=272, act="tanh", bwd="dev", accum=1),
    #         a straddling tile spans up to 2 x 272 rows > AW_ROWS: gather from global memory; N % 256 = 65; <1> bodies
    "w288": S(N=4160, span=288, act="none", res=0, bwd="dev", p_dead=0.0, bias=("ends", 3.0), perm=True),
    #         span 288: forward on aggregate_kernel, de on the wide kernel, dh on pull_win_kernel (PW_SPAN); crowded targets on
    #         both sides of every second graph boundary: tiles of about 6000 records, read-from-memory tail; N % 256 = 64
    "r4096": S(N=4353, span=256, act="relu", bwd="dev", p_dead=0.0, tweaks=("one_dead",)),
    #         tiles of exactly PW_REC = 4096 records and one of 4095; last tile of one target
    "r4097": S(N=4353, span=[257, 256], act="none", bwd="dev", accum=1, p_dead=0.0, tweaks=("first_graph_4097",)),
    #         tile 0 has 4097 records: one read from memory; mixed spans, every later tile straddles two graphs
    "aw_long": S(N=lambda cu: 64 * cu + 45, K=4, span=256, act="relu", res=0),
    #         agg_win_kernel with two or more 32-atom tiles per workgroup
    # 3. mp_gw_kernel<PADDED, 3, false, 6> by default: no switch, aggregate not kept, span 256, N >= 8192
    "gw_def": S(N=8192 + 40, span=256, act="softplus", fwd="infer"),
    # 4. the same kernel under NG_MP_GG=1 / NG_MP_GG_MIN_ROWS=1 (NG_MP_GW=nowin must give the same bits)
    "gg40": S(N=40, act="relu", fwd="infer", env=GG),                        # one ragged tile; 16-byte staging (K = 16)
    "gg256_k12": S(N=256, K=12, act="none", res=0, fwd="infer", env=GG),     # exactly one tile; generic staging
    "gg257_k4": S(N=257, K=4, act="tanh", fwd="infer", env=GG),              # a second tile of one row; K = 4
    "gg700": S(N=700, span=256, act="relu", fwd="infer", env=GG),            # ragged third tile, window tiles
    "ggmix": S(N=1300, span=[100, 100, 100, 500], act="relu", res=0, fwd="infer", env=GG),
    #         graphs of 100 rows (window tiles) and of 500 rows (wider than the 320-row window: memory tiles) in one launch
    "range_p": S(N=700, span=256, act="none", fwd="infer", env=GG, big_h=True, fams=("normal",)),   # |A| beyond 65504: repair kernel
    # 5. mp_gw_kernel<CSR, 3, false, 8> with the aggregate as a by-product; 8. backward through mp_gw_kernel<REC, 3, true, 8>
    "ggc": S(kind="csr", N=1357, span=256, act="relu", deg=tile_degrees, bwd="none", env=GG),
    "range_c": S(kind="csr", N=600, span=256, act="none", deg=small_degrees, env=GG, big_h=True, fams=("normal",)),
    "ggt700": S(N=700, span=256, act="relu", bwd="both", accum=1, env=GG, hub=1500, tweaks=("orphan", "lonely"), scale=True),
    #         records supplied == records built inside; hub; orphan; a target with sum |e| <= 1 beside targets above 1; dH 2^k
    "ggt_none": S(N=300, span=0, act="none", res=0, bwd="dev", env=GG),      # the pull behind mp_dp_kernel with S = NULL
}
PAIRS = [(n, f) for n, sp in CASES.items() for f in sp["fams"]]
EXACT_CASES = [n for n, f in PAIRS if f == "exact"]


def build(name, fam, cu=256):
    sp = CASES[name]
    N = sp["N"](cu) if callable(sp["N"]) else sp["N"]
    act = sp["act"] if fam == "normal" else EXACT_ACT[sp["act"]]
    seed = zlib.crc32(name.encode()) % 100000
    hub = min(sp["hub"], EXACT_HUB) if fam == "exact" else sp["hub"]
    if sp["kind"] == "padded":
        c = padded_case(F, sp["E"], sp["K"], N, sp["span"], act, sp["res"], seed, hub=hub, p_dead=sp["p_dead"], bias=sp["bias"],
                        hub_local=bool(np.max(sp["span"])))
        for t in sp["tweaks"]:
            TWEAK[t](c)
    else:
        c = csr_case(F, sp["E"], N, sp["deg"](np.random.default_rng(seed + 1), N), act, sp["res"], seed, hub=hub, local=sp["span"])
    if fam == "exact":
        c = exact_inputs(c, seed + 7)
    if sp["big_h"]:
        flat = c["h"].reshape(-1)
        rng = np.random.default_rng(2)
        flat[rng.choice(flat.size, 40, replace=False)] = 3e5 * rng.choice([-1.0, 1.0], 40)
    c.update(name=name, family=fam)
    assert c["nl"].min() >= 0 and c["nl"].max() < N
    assert_shape(name, c)
    return c


def assert_shape(name, c):
    """the quantity each case was built for"""
    if c["kind"] == "padded" and "orphan" in CASES[name]["tweaks"]:
        assert not (c["nl"] == 5).any()
    if name == "w288":
        assert tile_records(c).max() > 5500
    if name == "r4096":
        r = tile_records(c)
        assert r[2] == PW_REC - 1 and (np.delete(r, 2)[:-1] == PW_REC).all() and r[-1] == 16
    if name == "r4097":
        assert tile_records(c)[0] == PW_REC + 1
    if name == "w256":
        assert tile_records(c).max() < PW_REC
    if name == "ggc":
        t = tile_tails(np.diff(c["row_ptr"]))
        assert t[0] == GW_CAPB and t[1] == GW_CAPB + 1 and t[2] == 256 * 44 and t[3] == 0 and c["N"] % GW_BM
    if name == "ggt700":
        _, rec = host_records(c)
        ptr, _ = host_records(c)
        sm = np.array([np.abs(rec[a:b, 1:]).sum(0).max() if b > a else 0.0 for a, b in zip(ptr[:-1], ptr[1:])])
        deg = np.diff(ptr)
        assert (sm > 1).any() and ((sm <= 1) & (deg > 0)).any() and deg[5] == 0 and deg[9] == 1 and deg.max() >= EXACT_HUB


def _ref(c):
    return ref_layer(c["h"], c["nl"], c["e"], c["inv"], c["w"], c["dH"], c["act"], c["residual"])


def stat_keys(name, c):
    """the outputs behind a split-operand product (module docstring)"""
    sp = CASES[name]
    gw = bool(sp["env"]) or name == "gw_def"
    keys = ["s", "h_out"] if c["N"] >= 4096 or gw else []
    if sp["bwd"]:
        keys += ["dh", "de", "dw"] if c["N"] >= 4096 else (["dh"] if gw else [])
    if sp["accum"] and "de" in keys:
        keys.remove("de")
    return keys


_SLOT = {}


def reference(name, fam, cu):
    """case, float64 values, magnitudes and (normal family) the two emulated statistics, computed once"""
    if _SLOT.get("key") != (name, fam, cu):
        _SLOT.clear()
        c = build(name, fam, cu)
        v, mg = _ref(c)
        keys = stat_keys(name, c) if fam == "normal" else []
        st = layer_stats(c["h"], c["nl"], c["e"], c["inv"], c["w"], c["dH"], c["act"], c["residual"], v, mg, c["live"],
                         keys=keys) if keys else {}
        _SLOT.update(key=(name, fam, cu), val=(c, v, mg, st))
    return _SLOT["val"]


def num_cu_of(dev):
    import torch
    return torch.cuda.get_device_properties(dev).multi_processor_count


def prior_of(c):
    """the de a call accumulates onto, in the padded form of the reference and as the kernels take it"""
    rng = np.random.default_rng(c["N"])
    shape = (c["N"], c["K"], c["E"])
    p = rng.integers(-3, 4, shape).astype(np.float64) if c["family"] == "exact" else f32(rng.standard_normal(shape))
    return p, (p.reshape(-1, c["E"]) if c["kind"] == "padded" else p[c["rows"], c["slot"]])


def run_calls(g, sp, v, monkeypatch):
    """the calls of one case; returns the outputs to hold against float64 and the list of broken same-bits promises"""
    import torch
    c = g.c
    gw = bool(sp["env"]) or c["name"] == "gw_def"
    broken, out = [], {}
    live = torch.from_numpy(c["live"].reshape(-1) if c["kind"] == "padded" else np.ones(g.n_ent, bool)).to(g.dev)

    def same(what, a, b):
        if not torch.equal(a, b):
            broken.append(f"{what}: not the same bits ({int((a != b).sum())} of {a.numel()} elements differ)")

    A_only = None
    if sp["fwd"] == "train":
        h_out, A, s = g.fwd()
        A_only = g.aggregate()
        out.update(h_out=h_out, A=A, s=s)
        if sp["env"]:
            out["A_only"] = A_only          # A_save is the gather-GEMM's by-product, another order of sums
        else:
            same("ng_mp_aggregate against A_save", A_only, A)
    else:
        h_out, _, s = g.fwd(keep_A=False)
        out.update(h_out=h_out, s=s)
    if gw:
        monkeypatch.setenv("NG_MP_GW", "nowin")
        h2, _, s2 = g.fwd(keep_A=False)
        monkeypatch.delenv("NG_MP_GW")
        h3, _, s3 = g.fwd(keep_A=False)
        same("h_out without the window", h2, h3)
        same("s_save without the window", s2, s3)
        if sp["fwd"] == "infer":
            same("h_out of a second run", h3, h_out)
    if sp["bwd"]:
        tS, dH = g.t(v["s_in"]), g.t(c["dH"])
        prior_p, prior_flat = prior_of(c) if sp["accum"] else (None, None)
        prior = g.t(prior_flat) if sp["accum"] else None
        rec = g.records() if sp["bwd"] in ("dev", "both") else None
        dh, de, dw = g.bwd(A_only, tS, dH, rec=rec, de_prior=prior)
        out.update(dh=dh, de=de, dw=dw)
        dh2, de2, dw2 = g.bwd(A_only, tS, dH, rec=rec, de_prior=prior, want_dw=False)           # 9. dw = NULL
        assert dw2 is None
        same("dh_in with dw = NULL", dh2, dh)
        same("de with dw = NULL", de2[live], de[live])
        _, _, dw3 = g.bwd(None, tS, dH, rec=rec, de_prior=prior)                                # 10. aggregate rebuilt
        same("dw with A_save = NULL", dw3, dw)
        if sp["bwd"] == "both":             # records supplied against the csc_edge -> e chain / the records built inside
            dh4, de4, dw4 = g.bwd(A_only, tS, dH, rec=None, de_prior=prior)
            same("dh_in without records", dh4, dh)
            same("de without records", de4[live], de[live])
            same("dw without records", dw4, dw)
        if sp["perm"] or sp["bwd"] == "both":
            ptr_h, rec_h = host_records(c)
            same("csc_ptr against the host's", g.csc_ptr.cpu(), torch.from_numpy(ptr_h))
            same("ng_mp_edge_records against the host's", rec[:len(rec_h)].cpu().view(torch.int32),
                 torch.from_numpy(rec_h).view(torch.int32))
        if sp["perm"]:                      # caller-built records, shuffled inside each target's segment
            _, rec_p = host_records(c, permute=3)
            dh5, de5, dw5 = g.bwd(A_only, tS, dH, rec=g.records(host=rec_p), de_prior=prior)
            out["dh_perm"] = dh5
            same("de with permuted records", de5[live], de[live])
            same("dw with permuted records", dw5, dw)
        if gw:
            monkeypatch.setenv("NG_MP_GW", "nowin")
            dh6, _, _ = g.bwd(A_only, tS, dH, rec=rec, de_prior=prior, want_dw=False)
            monkeypatch.delenv("NG_MP_GW")
            same("dh_in without the window", dh6, dh)
        if sp["scale"]:
            for k in (-40, 24):
                dhk, _, _ = g.bwd(A_only, tS, g.t(c["dH"] * 2.0 ** k), rec=rec, de_prior=prior, want_dw=False)
                same(f"dh_in of dH 2^{k}", dhk, dh * 2.0 ** k)
        out["prior"] = prior_p
    torch.cuda.synchronize()
    res = {k: (a.cpu().numpy() if hasattr(a, "cpu") else a) for k, a in out.items() if k != "de"}
    if "de" in out:
        res["de"] = de_slots(c, out["de"])
    return res, broken


def hold(c, got, v, mg, failures):
    """every output against float64 by the family's criterion; returns the normalised errors (normal family)"""
    errs = {}
    prior = got.get("prior")
    for key in ("h_out", "s", "A", "A_only", "dh", "dh_perm", "de", "dw"):
        if key not in got:
            continue
        rk = {"A_only": "A", "dh_perm": "dh"}.get(key, key)
        ref, mag = v[rk], mg[rk]
        if key == "de" and prior is not None:
            ref, mag = ref + prior, mag + np.abs(prior)
        sel = c["live"] if key == "de" else None
        g64 = np.asarray(got[key], np.float64).reshape(ref.shape)
        if c["family"] == "exact":
            a, b = (g64[sel], ref[sel]) if sel is not None else (g64, ref)
            bad = ~(a == b)
            if bad.any():
                k = int(np.flatnonzero(bad.reshape(-1))[0])
                failures.append(f"{OUT_NAME[key]}: {int(bad.sum())} of {bad.size} elements differ from float64; first at flat {k}: "
                                f"got {a.reshape(-1)[k]!r} ref {b.reshape(-1)[k]!r}")
        else:
            try:
                errs[key] = check(OUT_NAME[key], g64, ref, mag, sel=sel)
            except AssertionError as err:
                failures.append(str(err))
    return errs


@pytest.mark.parametrize("name,fam", PAIRS)
def test_default_width_layer_vs_float64(gpu_device, monkeypatch, name, fam):
    """every element of every output of the case's calls against the float64 statement (exact family: the same bits), the
    same-bits promises between call forms, and (normal family) the rms statistic and the f32-input comparison"""
    sp = CASES[name]
    c, v, mg, st = reference(name, fam, num_cu_of(gpu_device))
    for k, val in sp["env"].items():
        monkeypatch.setenv(k, val)
    g = GpuLayer(c, gpu_device)
    with g.graph_span():
        got, failures = run_calls(g, sp, v, monkeypatch)
        errs = hold(c, got, v, mg, failures)
        for key, (r32, r_drop) in st.items():
            sel = c["live"] if key == "de" else None
            n_sel = int(c["live"].sum()) * c["E"] if key == "de" else got[key].size
            assert n_sel >= STAT_MIN, (key, n_sel)
            r = rstat(np.asarray(got[key], np.float64).reshape(v[key].shape), v[key], mg[key], sel)
            thr = float(np.sqrt(r32 * r_drop))
            asserted = c["act"] in (ACT["none"], ACT["relu"])
            print(f"RSTAT {name:10s} {OUT_NAME[key]:6s} r {r:.3e} r32 {r32:.3e} r_drop {r_drop:.3e} thr {thr:.3e} "
                  f"{'assert' if asserted else 'print'}")
            if asserted and not r <= thr:
                failures.append(f"{OUT_NAME[key]}: r = {r:.3e} above sqrt(r32 * r_drop) = {thr:.3e} (r32 {r32:.3e}, r_drop {r_drop:.3e})")
        if sp["fp32"] and fam == "normal" and not failures:
            monkeypatch.setenv("NG_GEMM_MATH", "fp32")
            got32, broken32 = run_calls(g, sp, v, monkeypatch)
            failures += broken32
            errs32 = hold(c, got32, v, mg, failures)
            print("ERR", name, {k: (f"{errs[k]:.2e}", f"{errs32.get(k, 0):.2e}") for k in errs})
            failures += [f"{OUT_NAME[k]}: error {errs[k]:.3e} above 8 x the f32-input run's {errs32[k]:.3e} + 1e-6"
                         for k in errs if k in errs32 and errs[k] > 8.0 * errs32[k] + 1e-6]
    assert not failures, "\n".join(failures)


# --------------------------------------------------------------------------------------------- two tiles per workgroup, dw = NULL
def big_case(fam, cu):
    """N = 256 cu + 300 in graphs of 256 (pull_win_kernel: ceil(ntiles / cu) >= 2 tiles of 256 targets per workgroup) and the
    graphs the float64 reference is evaluated on: the first two, the last two (the last one partial) and the graphs on both
    sides of the first, a middle and the last tile boundary between two workgroups.  Graphs are independent, so dh_in and de
    of those rows are complete"""
    N = 256 * cu + 300
    c = padded_case(F, 3, 16, N, 256, "none", 0, seed=cu)
    c.update(name="big", family=fam)
    if fam == "exact":
        c = exact_inputs(c, cu + 7)
    ntiles = -(-N // PW_T)
    per = -(-ntiles // cu)
    nwg = -(-ntiles // per)
    assert per >= 2 and nwg >= 3
    graphs = {0, 1, ntiles - 2, ntiles - 1}
    for b in (per, per * (nwg // 2), per * (nwg - 1)):
        graphs |= {b - 1, b}
    rows = np.concatenate([np.arange(t * 256, min(t * 256 + 256, N)) for t in sorted(graphs)])
    return c, rows


@pytest.mark.parametrize("fam", ["exact", "normal"])
def test_two_tiles_per_workgroup_with_dw_null(gpu_device, fam):
    """6. records given, span 256, dw = NULL at N = 256 cu + 300: mp_dp_kernel (S = NULL) -> dense_dx -> egrad_win_kernel<3> ->
    pull_win_kernel<3> with two or more tiles per workgroup; dh_in and de of the sampled graphs against float64, every other
    element written (no NaN left)"""
    import torch
    c, rows = big_case(fam, num_cu_of(gpu_device))
    sub = sub_case(c, rows)
    v, mg = _ref(sub)
    g = GpuLayer(c, gpu_device)
    with g.graph_span():
        dh, de, dw = g.bwd(None, None, g.t(c["dH"]), rec=g.records(), want_dw=False)
        torch.cuda.synchronize()
    assert dw is None
    live = torch.from_numpy(c["live"].reshape(-1)).to(gpu_device)
    assert bool(torch.isfinite(dh).all()) and bool(torch.isfinite(de[live]).all())
    got = {"dh": dh.cpu().numpy()[rows], "de": de_slots(c, de)[rows]}
    failures = []
    hold(sub, got, v, mg, failures)
    assert not failures, "\n".join(failures)
