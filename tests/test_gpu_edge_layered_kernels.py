"""The layered edge MLP of csrc/edge_ops.hip through the C entry points ng_edge_mlp_fwd, ng_edge_mlp_bwd, ng_edge_mlp_bwd_tape and
ng_rbf_expand, element by element against the float64 statement of tests/edge_layered_ref.py (checked on the CPU by
tests/test_edge_layered_ref_host.py, which also proves from the launch arithmetic that every case reaches the branch it is listed
under here).

Every output — e, the tape, dW, db, the RBF tile — is filled with NaN before the call and allocated with GUARD = 64 extra rows that
must still hold the fill afterwards.  Every call is made twice into fresh buffers; the second must give the same bits.  Two families:
  exact   edge_layered_ref.exact_case: every output equals the float64 statement BIT FOR BIT (float64 value rounded to float32;
          dead rows of e are +0).  Activations none and relu.
  normal  edge_layered_ref.normal_case: per element |got - ref| <= C_REL * mag + 1e-7 * max(mag); where the split-operand GEMMs run
          also max err / max mag <= 8 x that of the same call under NG_GEMM_MATH=fp32 + 1e-6.  All four activations.
ng_rbf_expand's normal family is held to the counted bound C_RBF * 2^-24 * R (1 + |arg|) + 2^-126.

Dispatch, from the conditions in edge_ops.hip, and the case ids that reach each (test_chain[<id>-exact|normal] unless another test
is named; CLAIMS below is this table in the form the CPU test checks against edge_layered_ref.branches):
  forward
    rbf_kernel: one trip / a second grid-stride trip (items = n H / 4 > 524288)   test_rbf_expand[H16-n131072] / [H16-n131073]
      H / 4 = 1, 5, 4, 32, 128 float4 columns per row                            test_rbf_expand[H4|H20|H16|H128|H512-n1|n257]
    hidden layers: dense_fwd per layer, into the tape (z_save) / into the two ping-pong buffers (z_save = NULL)
                                                                                   every case / infer-* (H512-n32768: more
                                                                                   GEMM tiles than are resident at once)
      tape layer t at offset t n H                                                 tape-H64-L6-E3-relu-n65
      activation none / softplus / relu / tanh                                     act-H32-*, act-H128-* (split GEMMs at n4097)
    E <= 8: edge_out_fwd_kernel<E>, 64 rows per workgroup                          out-H48-L2-E<1..8>-*-n65, out-H272-L2-E<1..8>-*-n65
      n = 1 / 63 / 64 / 65 / 4097 (ragged and full last workgroup)                 rows-H<16|48|128|272|512>-*-n<n>
      H = 16: a single k0 trip                                                     rows-H16-*
    E > 8: dense_fwd + mask_rows_kernel; items = n E below / at / above 524288     wide-H16|H64-L2-E12|E64|E256-*-n257,
                                                                                   wide-H16-L2-E256-relu-n2047|n2048|n2049
  backward
    E <= 8: edge_out_bwd_kernel<E> + sum_partials2_kernel
      one weight column per thread (H <= 256) / two (H in 272..512)               rows-H16|H256-* / rows-H272|H512-*, out-H272-*
      nb = 1: n = 1, 63, 64, 65, 2048 (32 full trips)                              rows-*-n1|n63|n64|n65|n2048
      nb = 2, rows 1088, last trip one row / nb = 4, rows 1600                     rows-*-n2049 / rows-*-n6145
      nb capped at 2048, rows 2112, 62 trailing blocks without rows               test_capped_partition_exact
      sum_partials2_kernel nz = 1 / 2 / 4 / 2048                                   n <= 2048 / n2049 / n6145 / test_capped_partition_exact
    E > 8: mask_rows_kernel into dE, dense_dw, dense_dx                            wide-*
    hidden layers: dense_dw (+ dense_dx for t > 0), rbf_kernel again for t = 0     every case
  NG_EDGE_PATH=layered at the fused architecture (H128, Le4, softplus)            layered-env-H128-L4-E3-softplus-n257-normal
  every slot dead / no slot dead                                                   alldead-H272-L2-E5-relu-n65 / nodead-H272-L2-E5-relu-n65
  refused before any launch                                                        test_refused[*], test_rbf_refused[*]
  n = 0                                                                            test_no_edges_*"""
import ctypes as C

import numpy as np
import pytest

import edge_layered_ref as R
from edge_layered_ref import ACT, f32, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
SCOPES = {"rbf", "edge_dense_fwd", "edge_dense_dw", "edge_dense_dx", "edge_out_fwd", "edge_out_bwd"}


# ------------------------------------------------------------------------------------------------------------------ case table
def _cases():
    t = {}

    def add(tag, H, Le, E, act, n, fams=("exact", "normal"), p_dead=None, infer=False, env=None):
        t[f"{tag}-H{H}-L{Le}-E{E}-{act}-n{n}"] = dict(H=H, Le=Le, E=E, act=act, n=n, fams=fams, p_dead=p_dead, infer=infer,
                                                   env=env or {})

    for E in range(1, 9):
        for H in (48, 272):
            add("out", H, 2, E, "relu" if E % 2 else "none", 65)
    rows = {16: (1, 63, 64, 65, 4097, 2048, 2049, 6145), 48: (1, 63, 64, 4097), 128: (1, 63, 64, 65, 4097),
            256: (1, 63, 64, 65, 2048, 2049, 6145), 272: (1, 63, 64, 4097, 2048, 2049, 6145),
            512: (1, 63, 64, 65, 4097, 2048, 2049, 6145)}
    k = 0
    for H, ns in rows.items():
        for n in ns:
            add("rows", H, 2, 1 + k % 8, "none" if k % 2 else "relu", n)
            k += 3
    for E in (12, 64, 256):
        for H in (16, 64):
            add("wide", H, 2, E, "relu" if H == 16 else "none", 257)
    for n in (2047, 2048, 2049):
        add("wide", 16, 2, 256, "relu", n)
    for Le, act in ((2, "relu"), (3, "none"), (4, "relu"), (6, "none")):
        add("infer", 32, Le, 2, act, 255, infer=True)
        add("infer", 128, Le, 3, act, 4097, infer=True)
    # the in-place GEMM a missing ping-pong would run is wrong only once workgroups of a later column tile start after an earlier
    # tile of their rows has been stored: 256 x 4 tiles of 128 x 128, more than are resident at once
    add("infer", 512, 3, 2, "relu", 32768, infer=True)
    add("tape", 64, 6, 3, "relu", 65)
    for act in ("none", "softplus", "relu", "tanh"):
        fams = ("exact", "normal") if act in ("none", "relu") else ("normal",)
        add("act", 32, 3, 2, act, 255, fams)
        add("act", 128, 3, 2, act, 4097, fams)
    add("layered-env", 128, 4, 3, "softplus", 257, ("normal",), env={"NG_EDGE_PATH": "layered"})
    add("alldead", 272, 2, 5, "relu", 65, p_dead=1.0)
    add("nodead", 272, 2, 5, "relu", 65, p_dead=0.0)
    return t


CASES = _cases()
PAIRS = [(cid, fam) for cid, sp in CASES.items() for fam in sp["fams"]]
RBF_CASES = [(4, 1), (4, 257), (20, 1), (20, 257), (16, 1), (16, 257), (128, 1), (128, 257), (512, 1), (512, 257), (16, 131072),
             (16, 131073)]

# branch of edge_layered_ref.branches -> the cases listed under it in the table above
CLAIMS = {
    **{f"out<{E}>": [f"out-H48-L2-E{E}-{'relu' if E % 2 else 'none'}-n65", f"out-H272-L2-E{E}-{'relu' if E % 2 else 'none'}-n65"]
       for E in range(1, 9)},
    "fwd_k1": [c for c in CASES if c.startswith("rows-H16-")],
    "fwd_wg_ragged1": [c for c in CASES if c.startswith("rows-") and c.endswith(("-n1", "-n65", "-n4097"))],
    "fwd_wg_ragged63": [c for c in CASES if c.startswith("rows-") and c.endswith("-n63")],
    "fwd_wg_full": [c for c in CASES if c.startswith("rows-") and c.endswith(("-n64", "-n2048"))],
    "fwd_wgs>1": [c for c in CASES if c.startswith("rows-") and c.endswith(("-n65", "-n4097", "-n2049", "-n6145"))],
    "bwd_col1": [c for c in CASES if c.startswith(("rows-H16-", "rows-H256-", "out-H48-"))],
    "bwd_col2": [c for c in CASES if c.startswith(("rows-H272-", "rows-H512-", "out-H272-"))],
    "nb1": [c for c in CASES if c.startswith("rows-") and c.endswith(("-n1", "-n63", "-n64", "-n65", "-n2048"))],
    "nz1": [c for c in CASES if c.startswith("rows-") and c.endswith("-n2048")],
    "bwd_trips_full": [c for c in CASES if c.startswith("rows-") and c.endswith(("-n64", "-n2048"))],
    "bwd_last_trip63": [c for c in CASES if c.startswith("rows-") and c.endswith("-n63")],
    "bwd_last_trip1": [c for c in CASES if c.startswith("rows-") and c.endswith(("-n1", "-n65", "-n2049", "-n6145"))],
    "nb2": [c for c in CASES if c.startswith("rows-") and c.endswith("-n2049")],
    "rows1088": [c for c in CASES if c.startswith("rows-") and c.endswith("-n2049")],
    "nz2": [c for c in CASES if c.startswith("rows-") and c.endswith("-n2049")],
    "nb4": [c for c in CASES if c.startswith("rows-") and c.endswith("-n6145")],
    "rows1600": [c for c in CASES if c.startswith("rows-") and c.endswith("-n6145")],
    "nz4": [c for c in CASES if c.startswith("rows-") and c.endswith("-n6145")],
    "wide": [c for c in CASES if c.startswith("wide-")],
    "mask_trips1": ["wide-H16-L2-E256-relu-n2047", "wide-H16-L2-E256-relu-n2048"],
    "mask_trips2": ["wide-H16-L2-E256-relu-n2049"],
    "split": [c for c in CASES if c.startswith(("infer-H128-", "act-H128-", "rows-H128-")) and c.endswith("-n4097")]
             + [c for c in CASES if c.startswith(("rows-H256-", "rows-H512-")) and c.endswith(("-n2048", "-n2049", "-n4097", "-n6145"))],
    "Le6": ["tape-H64-L6-E3-relu-n65", "infer-H32-L6-E2-none-n255", "infer-H128-L6-E3-none-n4097"],
    **{f"Le{Le}": [f"infer-H32-L{Le}-E2-{a}-n255", f"infer-H128-L{Le}-E3-{a}-n4097"] for Le, a in ((2, "relu"), (3, "none"), (4, "relu"))},
    **{f"act{ACT[a]}": [f"act-H32-L3-E2-{a}-n255", f"act-H128-L3-E2-{a}-n4097"] for a in ACT},
}
BIG_CLAIMS = ("nb2048", "rows2112", "nz2048", "bwd_empty_blocks", "out<1>")      # test_capped_partition_exact


# ---------------------------------------------------------------------------------------------------------------- device side
def _ctx():
    from nmrgnn_amd import _lib
    return _lib.get_context(0)


def _st(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _t(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _nan(dev, *shape):
    import torch
    return torch.full(shape, float("nan"), device=dev)


def _untouched(name, t, first):
    import torch
    assert bool(torch.isnan(t[first:]).all()), f"{name}: a store past the end of the output"


def _all_nan(ts):
    import torch
    return all(bool(torch.isnan(t).all()) for t in ts)


def _inputs(dev, c):
    return dict(d=_t(dev, c["d_src"]), f=_t(dev, c["d_eff"]), c=_t(dev, c["centers"]), W=[_t(dev, w) for w in c["Ws"]],
                b=[_t(dev, b) for b in c["bs"]])


def run_fwd(dev, c, save, repeat=2):
    """ng_edge_mlp_fwd, `repeat` times into fresh NaN-filled buffers with guard rows -> {"e": [n, E], "z": [Le - 1] of [n, H]}
    (z only with save) of the first call; the later calls must give the same bits"""
    import torch
    from nmrgnn_amd._lib import ptr, ptr_array
    n, H, E, Le = c["n"], c["H"], c["E"], c["Le"]
    ctx, t = _ctx(), _inputs(dev, c)
    assert int(ctx.lib.ng_edge_tape_layout(H, E, Le, c["act"], n)) == 0 and ctx.lib.ng_edge_live_supported(H, E, Le, c["act"]) == 0
    outs = []
    for _ in range(repeat):
        e = _nan(dev, n + GUARD, E)
        z = _nan(dev, (Le - 1) * n + GUARD, H) if save else None
        ctx.check(ctx.lib.ng_edge_mlp_fwd(ctx.handle, _st(dev), n, H, E, Le, c["act"], ptr(t["d"]), ptr(t["f"]), ptr(t["c"]),
                                          float(c["gap"]), ptr_array(t["W"]), ptr_array(t["b"]), ptr(e), ptr(z)), "ng_edge_mlp_fwd")
        torch.cuda.synchronize()
        _untouched("e", e, n)
        out = {"e": e[:n].cpu().numpy()}
        if save:
            _untouched("tape", z, (Le - 1) * n)
            zz = z[:(Le - 1) * n].reshape(Le - 1, n, H).cpu().numpy()
            out["z"] = [zz[l] for l in range(Le - 1)]
        outs.append(out)
    for o in outs[1:]:
        for (name, a), (_, b) in zip(R.tensors(outs[0]), R.tensors(o)):
            assert same_bits(a, b), f"{name}: a second call gave other bits"
    return outs[0]


def run_bwd(dev, c, zs32, repeat=2):
    """ng_edge_mlp_bwd with the tape zs32 (row-major, layer t at offset t n H), `repeat` times -> {"dW": [Le], "db": [Le]}"""
    import torch
    from nmrgnn_amd._lib import ptr, ptr_array
    n, H, E, Le = c["n"], c["H"], c["E"], c["Le"]
    ctx, t = _ctx(), _inputs(dev, c)
    tz = torch.empty((Le - 1, n, H), device=dev)
    for l in range(Le - 1):
        tz[l].copy_(_t(dev, zs32[l]))
    tde = _t(dev, c["de"])
    kouts = [H] * (Le - 1) + [E]
    outs = []
    for _ in range(repeat):
        dW = [_nan(dev, H + GUARD, k) for k in kouts]
        db = [_nan(dev, k + GUARD) for k in kouts]
        ctx.check(ctx.lib.ng_edge_mlp_bwd(ctx.handle, _st(dev), n, H, E, Le, c["act"], ptr(t["d"]), ptr(t["f"]), ptr(t["c"]),
                                          float(c["gap"]), ptr_array(t["W"]), ptr(tz), ptr(tde), ptr_array(dW), ptr_array(db)),
                  "ng_edge_mlp_bwd")
        torch.cuda.synchronize()
        for l in range(Le):
            _untouched(f"dW{l}", dW[l], H)
            _untouched(f"db{l}", db[l], kouts[l])
        outs.append({"dW": [w[:H].cpu().numpy() for w in dW], "db": [b[:k].cpu().numpy() for b, k in zip(db, kouts)]})
    for o in outs[1:]:
        for (name, a), (_, b) in zip(R.tensors(outs[0]), R.tensors(o)):
            assert same_bits(a, b), f"{name}: a second call gave other bits"
    return outs[0]


def _zero(a):
    return same_bits(a, np.zeros_like(np.asarray(a, np.float32)))


# ------------------------------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("cid,fam", PAIRS, ids=[f"{c}-{f}" for c, f in PAIRS])
def test_chain(gpu_device, monkeypatch, cid, fam):
    """training forward (e and every tape layer) and backward (every dW[t], db[t]) of the case, element by element against float64"""
    sp = CASES[cid]
    for k, val in sp["env"].items():
        monkeypatch.setenv(k, val)
    c = R.make_case(fam, sp["H"], sp["Le"], sp["E"], ACT[sp["act"]], sp["n"], sp["p_dead"])
    v, mg = R.ref_forward(c)
    zs32 = c["zs32"] if fam == "exact" else [f32(z) for z in v["z"]]
    vb, mgb = R.ref_backward(c, zs32, mz=None if fam == "exact" else mg["z"])
    ref, mag = dict(v, **vb), dict(mg, **mgb)
    Le = sp["Le"]
    if Le > 2:                                                   # the layers differ, so a misplaced layer cannot pass
        assert all(not np.array_equal(v["z"][a], v["z"][b]) for a in range(Le - 1) for b in range(a)) or sp["p_dead"] == 1.0

    def run():
        got = run_fwd(gpu_device, c, True)
        got.update(run_bwd(gpu_device, c, zs32))
        return got

    got = run()
    failures = []
    errs = R.hold(fam, got, ref, mag, failures)
    dead = np.asarray(c["d_src"]) <= 0
    if not _zero(got["e"][dead]):
        failures.append("e: a dead row is not +0")
    if sp["p_dead"] == 1.0:
        assert dead.all() and np.isfinite(np.stack(got["z"])).all()
        failures += [f"{name}: not exactly zero with every slot dead" for name, g in R.tensors(got) if name[0] != "z" and not _zero(g)]
    if sp["p_dead"] == 0.0:
        assert not dead.any()
    if sp["infer"]:                                              # z_save = NULL: the ping-pong buffers
        e_inf = run_fwd(gpu_device, c, False)["e"]
        if not same_bits(e_inf, got["e"]):
            failures.append("e: the inference forward (z_save = NULL) does not give the bits of the training forward")
        R.hold(fam, {"e": e_inf}, ref, mag, failures)
    if fam == "normal":
        print("RATIO", cid, {k: f"{r[1]:.4f}" for k, r in errs.items()})
        if R.split_gemm(sp["H"], sp["n"]) and not failures:
            monkeypatch.setenv("NG_GEMM_MATH", "fp32")
            errs32 = R.hold(fam, run(), ref, mag, failures)
            print("ERR", cid, {k: (f"{errs[k][0]:.2e}", f"{errs32[k][0]:.2e}") for k in errs if k in errs32})
            failures += [f"{k}: error {errs[k][0]:.3e} above 8 x the f32-input run's {errs32[k][0]:.3e} + 1e-6"
                         for k in errs if k in errs32 and errs[k][0] > 8.0 * errs32[k][0] + 1e-6]
    assert not failures, "\n".join(failures)


_BIG = {}


def big_reference():
    """the 4.2 M-row case and its float64 gradients (summed in row slices), computed once"""
    if not _BIG:
        c = R.big_exact_case()
        _BIG["c"], (_BIG["v"], _BIG["mg"]) = c, R.ref_backward(c, c["zs32"])
    return _BIG["c"], _BIG["v"], _BIG["mg"]


def test_capped_partition_exact(gpu_device):
    """n = 2048^2 + 1 rows at H = 16, Le = 2, E = 1, relu: edge_out_bwd's partition is capped at 2048 workgroups of 2112 rows, the last
    62 of which have no row and must still write zero partials for sum_partials2_kernel (nz = 2048).  Exact family, backward only:
    every dW[t], db[t] bit for bit"""
    c, v, mg = big_reference()
    assert set(BIG_CLAIMS) <= R.branches(16, 2, 1, c["act"], c["n"])
    got = run_bwd(gpu_device, c, c["zs32"])
    failures = []
    R.hold("exact", got, v, mg, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------- ng_rbf_expand
def rbf_case(fam, H, n):
    rng = np.random.default_rng([H, n, 3 if fam == "exact" else 4])
    if fam == "exact":
        centers, d_src, d_eff = R.on_centres(rng, n, H, 0.15 if n > 1 else 0.0)
        return d_src, d_eff, centers, 1.0
    d_src = rng.uniform(0.05, 1.2, n)
    d_src[rng.random(n) < (0.3 if n > 1 else 0.0)] = 0.0
    d_eff = np.where(d_src > 0, d_src + 0.025 * rng.standard_normal(n), d_src)
    live = np.flatnonzero(d_src > 0)
    if len(live) >= 8:                                           # a few below the first and past the last centre
        pick = rng.choice(live, 4, replace=False)
        d_eff[pick[:2]] = -rng.uniform(0.001, 0.03, 2)
        d_eff[pick[2:]] = 1.2 + rng.uniform(0.001, 0.05, 2)
    centers = f32(np.linspace(0.0, 1.2, H))
    return f32(d_src), f32(d_eff), centers, float(np.float32(centers[1] - centers[0]))


def run_rbf(dev, H, d_src, d_eff, centers, gap, repeat=2):
    import torch
    from nmrgnn_amd._lib import ptr
    n = len(d_src)
    ctx = _ctx()
    td, tf, tc = _t(dev, d_src), _t(dev, d_eff), _t(dev, centers)
    outs = []
    for _ in range(repeat):
        out = _nan(dev, n + GUARD, H)
        ctx.check(ctx.lib.ng_rbf_expand(ctx.handle, _st(dev), n, H, ptr(td), ptr(tf), ptr(tc), float(gap), ptr(out)), "ng_rbf_expand")
        torch.cuda.synchronize()
        _untouched("rbf", out, n)
        outs.append(out[:n].cpu().numpy())
    assert all(same_bits(outs[0], o) for o in outs[1:]), "a second call gave other bits"
    return outs[0]


@pytest.mark.parametrize("fam", ["exact", "normal"])
@pytest.mark.parametrize("H,n", RBF_CASES, ids=[f"H{H}-n{n}" for H, n in RBF_CASES])
def test_rbf_expand(gpu_device, H, n, fam):
    """rbf_kernel alone: dead rows +0 bits; live rows one-hot bit for bit on the centres (exact), within the counted bound (normal)"""
    d_src, d_eff, centers, gap = rbf_case(fam, H, n)
    got = run_rbf(gpu_device, H, d_src, d_eff, centers, gap)
    ref, arg, live = R.rbf(d_src, d_eff, centers, gap)
    assert _zero(got[~live]), "a dead row is not +0"
    if fam == "exact":
        assert ((ref == 0) | (ref == 1)).all() and same_bits(got, ref.astype(np.float32))
        return
    err, bound = np.abs(got.astype(np.float64) - ref), R.rbf_bound(ref, arg)
    big = ref > 2.0 ** -100                                     # away from the flush-to-zero floor: the counted part alone
    print("RATIO rbf", H, n, f"all {float((err / bound).max()):.3f} normal-range {float((err / bound)[big].max()) if big.any() else 0:.3f}")
    bad = ~(err <= bound)
    assert not bad.any(), (int(bad.sum()), float((err / bound).max()))


# -------------------------------------------------------------------------------------------------------------------- refusals
BASE = dict(H=32, Le=2, E=2, act=2, gap=0.5, n=8)
MSG_H = "edge_mlp: edge_hidden_size % 16 == 0, <= 512"
MSG_E = "edge_mlp: edge_feature_size <= 8, or a multiple of 4 up to 256"
REFUSED = {
    # id: (overrides, calls the refusal holds for, message)
    "H24": (dict(H=24), ("fwd", "bwd"), MSG_H),
    "H528": (dict(H=528), ("fwd", "bwd"), MSG_H),
    "E0": (dict(E=0), ("fwd", "bwd"), MSG_E),
    "E9": (dict(E=9), ("fwd", "bwd"), MSG_E),
    "E10": (dict(E=10), ("fwd", "bwd"), MSG_E),
    "E260": (dict(E=260), ("fwd", "bwd"), MSG_E),
    "Le1": (dict(Le=1), ("fwd", "bwd"), "edge_mlp: edge_fc_layers >= 2"),
    "act4": (dict(act=4), ("fwd", "bwd"), "edge_mlp: unknown activation code"),
    "gap0": (dict(gap=0.0), ("fwd",), "edge_mlp: rbf gap > 0"),
    "gap-neg": (dict(gap=-0.5), ("fwd",), "edge_mlp: rbf gap > 0"),
    "no-tape": (dict(z_null=True), ("bwd",), "edge_mlp_bwd: saved activations required"),
    "blocked-tape": (dict(H=64, layout=1), ("bwd",), "edge_mlp_bwd: a blocked tape needs the fused edge path"),
    "ctx-null": (dict(ctx_null=True), ("fwd", "bwd"), None),
}


def _refused_call(dev, which, o):
    """the call with NaN-filled outputs -> (rc, message, outputs)"""
    import torch
    from nmrgnn_amd._lib import ptr, ptr_array
    p = dict(BASE, **{k: val for k, val in o.items() if k in BASE})
    n, H, E, Le = p["n"], p["H"], p["E"], max(p["Le"], 1)
    Ea = max(E, 1)
    ctx = _ctx()
    h = None if o.get("ctx_null") else ctx.handle
    td, tc = torch.full((n,), 0.5, device=dev), torch.linspace(0, 1, H, device=dev)
    tW = [torch.zeros(H, H, device=dev) for _ in range(Le - 1)] + [torch.zeros(H, Ea, device=dev)]
    tb = [torch.zeros(H, device=dev) for _ in range(Le - 1)] + [torch.zeros(Ea, device=dev)]
    if which == "fwd":
        outs = [_nan(dev, n, Ea), _nan(dev, max(Le - 1, 1) * n, H)]
        rc = ctx.lib.ng_edge_mlp_fwd(h, _st(dev), n, H, E, p["Le"], p["act"], ptr(td), ptr(td), ptr(tc), p["gap"], ptr_array(tW),
                                     ptr_array(tb), ptr(outs[0]), ptr(outs[1]))
    else:
        tz = None if o.get("z_null") else torch.ones(max(Le - 1, 1) * n, H, device=dev)
        tde = torch.ones(n, Ea, device=dev)
        outs = [_nan(dev, *w.shape) for w in tW] + [_nan(dev, *b.shape) for b in tb]
        rc = ctx.lib.ng_edge_mlp_bwd_tape(h, _st(dev), n, H, E, p["Le"], p["act"], ptr(td), ptr(td), ptr(tc), p["gap"],
                                          ptr_array(tW), ptr(tz), ptr(tde), ptr_array(outs[:Le]), ptr_array(outs[Le:]),
                                          o.get("layout", -1))
    torch.cuda.synchronize()
    return rc, (ctx.lib.ng_last_error(ctx.handle) or b"").decode(), outs


@pytest.mark.parametrize("rid,which", [(r, w) for r, (_, ws, _) in REFUSED.items() for w in ws], ids=lambda x: x)
def test_refused(gpu_device, rid, which):
    """NG_ERR_INVALID with the sources' message, every output left with its fill, no kernel of the edge path launched"""
    o, _, msg = REFUSED[rid]
    ctx = _ctx()
    ctx.prof_enable(True)
    ctx.prof_reset()
    rc, text, outs = _refused_call(gpu_device, which, o)
    names = set(ctx.prof_read())
    ctx.prof_enable(False)
    assert rc == -1 and (msg is None or msg in text), (rc, text)
    assert _all_nan(outs), "a refused call wrote an output"
    assert not names & SCOPES, names


@pytest.mark.parametrize("rid,H,gap", [("H6", 6, 0.5), ("gap0", 16, 0.0), ("ctx-null", 16, 0.5)])
def test_rbf_refused(gpu_device, rid, H, gap):
    import torch
    from nmrgnn_amd._lib import ptr
    ctx = _ctx()
    td, tc, out = torch.full((8,), 0.5, device=gpu_device), torch.linspace(0, 1, 16, device=gpu_device), _nan(gpu_device, 8, 16)
    ctx.prof_enable(True)
    ctx.prof_reset()
    rc = ctx.lib.ng_rbf_expand(None if rid == "ctx-null" else ctx.handle, _st(gpu_device), 8, H, ptr(td), ptr(td), ptr(tc), gap,
                               ptr(out))
    torch.cuda.synchronize()
    names = set(ctx.prof_read())
    ctx.prof_enable(False)
    text = (ctx.lib.ng_last_error(ctx.handle) or b"").decode()
    assert rc == -1 and (rid == "ctx-null" or "rbf_expand: H % 4 == 0, gap > 0" in text), (rc, text)
    assert _all_nan([out]) and not names & SCOPES, names


def test_no_edges_forward_and_rbf_write_nothing(gpu_device):
    """n_edges = 0 at a layered shape: NG_OK, nothing written, nothing launched"""
    import torch
    from nmrgnn_amd._lib import ptr, ptr_array
    H, E, Le = 64, 12, 3
    ctx, dev = _ctx(), gpu_device
    tc = torch.linspace(0, 1, H, device=dev)
    tW = [torch.zeros(H, H, device=dev) for _ in range(Le - 1)] + [torch.zeros(H, E, device=dev)]
    tb = [torch.zeros(H, device=dev) for _ in range(Le - 1)] + [torch.zeros(E, device=dev)]
    e, z, x0, d = _nan(dev, GUARD, E), _nan(dev, GUARD, H), _nan(dev, GUARD, H), torch.ones(4, device=dev)
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.check(ctx.lib.ng_edge_mlp_fwd(ctx.handle, _st(dev), 0, H, E, Le, 2, ptr(d), ptr(d), ptr(tc), 0.5, ptr_array(tW),
                                      ptr_array(tb), ptr(e), ptr(z)), "ng_edge_mlp_fwd")
    ctx.check(ctx.lib.ng_rbf_expand(ctx.handle, _st(dev), 0, H, ptr(d), ptr(d), ptr(tc), 0.5, ptr(x0)), "ng_rbf_expand")
    torch.cuda.synchronize()
    names = set(ctx.prof_read())
    ctx.prof_enable(False)
    assert _all_nan([e, z, x0]) and not names & SCOPES, names


def test_no_edges_backward_zero_fills_the_gradients(gpu_device):
    """ng_edge_mlp_bwd with n_edges = 0 at H = 64, E = 12, Le = 3: exactly dW[t] and db[t] are zero-filled, the guard rows behind
    them keep their fill"""
    import torch
    from nmrgnn_amd._lib import ptr, ptr_array
    H, E, Le = 64, 12, 3
    ctx, dev = _ctx(), gpu_device
    tc, d = torch.linspace(0, 1, H, device=dev), torch.ones(4, device=dev)
    kouts = [H] * (Le - 1) + [E]
    tW = [torch.zeros(H, k, device=dev) for k in kouts]
    dW, db = [_nan(dev, H + GUARD, k) for k in kouts], [_nan(dev, k + GUARD) for k in kouts]
    tz, tde = torch.ones(4, H, device=dev), torch.ones(4, E, device=dev)
    ctx.check(ctx.lib.ng_edge_mlp_bwd(ctx.handle, _st(dev), 0, H, E, Le, 2, ptr(d), ptr(d), ptr(tc), 0.5, ptr_array(tW), ptr(tz),
                                      ptr(tde), ptr_array(dW), ptr_array(db)), "ng_edge_mlp_bwd")
    torch.cuda.synchronize()
    for l, k in enumerate(kouts):
        _untouched(f"dW{l}", dW[l], H)
        _untouched(f"db{l}", db[l], k)
        assert _zero(dW[l][:H].cpu().numpy()) and _zero(db[l][:k].cpu().numpy()), l
