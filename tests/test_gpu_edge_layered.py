"""The layered edge MLP (csrc/edge_ops.hip: edge_mlp_fwd_layered / edge_mlp_bwd_layered — RBF tile, one dense GEMM per
hidden layer, edge_out_fwd_kernel / edge_out_bwd_kernel for E <= 8, a plain GEMM + mask_rows_kernel for wider E) against a
float64 numpy statement of nmrgnn/model.py:251-261 + layers.py:137-140 + model.py:111-138 and its backward, element by element.

The layered path serves every edge shape but H = 128 / Le = 4 / softplus (the fused kernels), among them fc_activation = relu at
H = 128.  Outputs are pre-filled with NaN; e, every z_save layer (in the order ng_edge_tape_layout names) and every dW[t] /
db[t] are held to |got - ref| <= C_REL * mag + 1e-7 * max(mag), mag the same expression on absolute values (activation slopes
bounded by 1, plus |act| for the activation's own rounding).  Row counts sit on both sides of the split-operand GEMMs'
thresholds (M >= 256 / M >= 4096, gemm_h2_fwd_ok)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C_REL = 3e-5
ACT = {"softplus": 1, "relu": 2}


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def act_fwd(act, x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x))) if act == 1 else np.maximum(x, 0)


def act_grad_from_out(act, z):
    return -np.expm1(-z) if act == 1 else (z > 0).astype(np.float64)


def ref_edge(d_src, d_eff, centers, gap, Ws, bs, de, act):
    """forward (e, hidden outputs z) and backward (dW, db) in float64 with the magnitudes of each; the backward is handed
    z rounded to float32, as the kernels are"""
    m = (d_src > 0).astype(np.float64)
    x0 = np.exp(-(d_eff[:, None] - centers[None, :]) ** 2 / gap) * m[:, None]
    v, mg = {"z": [], "z_in": []}, {"z": []}
    x, mx = x0, x0
    for W, b in zip(Ws[:-1], bs[:-1]):
        x = act_fwd(act, x @ W + b)
        mx = mx @ np.abs(W) + np.abs(b) + np.abs(x)       # + the activation's own rounding (softplus(0) = log 2)
        v["z"].append(x)
        v["z_in"].append(f32(x))
        mg["z"].append(mx)
        x = v["z_in"][-1]                       # the next layer of the reference reads what the tape holds
    v["e"] = m[:, None] * (x @ Ws[-1] + bs[-1])
    mg["e"] = m[:, None] * (mx @ np.abs(Ws[-1]) + np.abs(bs[-1]))
    # backward
    Le = len(Ws)
    v["dW"], v["db"], mg["dW"], mg["db"] = [None] * Le, [None] * Le, [None] * Le, [None] * Le
    ins = [x0] + v["z_in"][:-1]
    mins = [x0] + mg["z"][:-1]
    g, mgg = m[:, None] * de, m[:, None] * np.abs(de)
    for t in range(Le - 1, -1, -1):
        if t < Le - 1:
            slope = act_grad_from_out(act, v["z_in"][t])
            g, mgg = g * slope, mgg * np.abs(slope)
        xin = v["z_in"][-1] if t == Le - 1 else ins[t]
        mxin = mg["z"][-1] if t == Le - 1 else mins[t]
        v["dW"][t], v["db"][t] = xin.T @ g, g.sum(0)
        mg["dW"][t], mg["db"][t] = mxin.T @ mgg, mgg.sum(0)
        g, mgg = g @ Ws[t].T, mgg @ np.abs(Ws[t]).T
    return v, mg


def check(name, got, ref, mag):
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    top = float(mag.max()) if mag.size else 0.0
    bad = ~(err <= C_REL * mag + 1e-7 * top)                   # NaN fails
    if bad.any():
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries outside the bound; first at flat {k}: "
                             f"got {got.reshape(-1)[k]!r} ref {ref.reshape(-1)[k]!r} mag {mag.reshape(-1)[k]!r}")
    return float(err.max()) / top if top > 0 else 0.0


def run_gpu(dev, H, E, Le, act, d_src, d_eff, centers, gap, Ws, bs, z_in, de):
    """ng_edge_mlp_fwd (e, z_save) and ng_edge_mlp_bwd handed z_in (the float64 tape rounded to float32); z_save in
    row-major order whatever ng_edge_tape_layout says"""
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr, ptr_array
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    n = len(d_src)
    ctx = _lib.get_context(0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    td, tf, tc = t(d_src), t(d_eff), t(centers)
    tW, tb = [t(w) for w in Ws], [t(b) for b in bs]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    e, z = nan(n, E), nan(Le - 1, n, H)
    layout = int(ctx.lib.ng_edge_tape_layout(H, E, Le, act, n))
    ctx.check(ctx.lib.ng_edge_mlp_fwd(ctx.handle, st, n, H, E, Le, act, ptr(td), ptr(tf), ptr(tc), float(gap), ptr_array(tW),
                                      ptr_array(tb), ptr(e), ptr(z)), "ng_edge_mlp_fwd")
    zt = np.stack(z_in).astype(np.float32)
    if layout == 1:                                   # row-major -> the blocked order the kernels read
        from test_gpu_edge_h2 import tape_perm
        perm = tape_perm(n)
        blk = np.empty_like(zt.reshape(Le - 1, -1))
        for l in range(Le - 1):
            blk[l][perm] = zt[l].reshape(-1)
        zt = blk.reshape(zt.shape)
    dW = [nan(*w.shape) for w in Ws]
    db = [nan(*b.shape) for b in bs]
    tz, tde = t(zt), t(de)                            # held until the backward has run
    ctx.check(ctx.lib.ng_edge_mlp_bwd(ctx.handle, st, n, H, E, Le, act, ptr(td), ptr(tf), ptr(tc), float(gap), ptr_array(tW),
                                      ptr(tz), ptr(tde), ptr_array(dW), ptr_array(db)), "ng_edge_mlp_bwd")
    torch.cuda.synchronize()
    zz = z.cpu().numpy().astype(np.float64)
    if layout == 1:
        zz = np.stack([zz[l].reshape(-1)[tape_perm(n)].reshape(n, H) for l in range(Le - 1)])
    as64 = lambda x: x.cpu().numpy().astype(np.float64)
    return as64(e), zz, [as64(x) for x in dW], [as64(x) for x in db]


CASES = [
    # H, Le, E, act, n, dead fraction      meant to reach
    (16, 2, 1, "relu", 4097, 0.3),          # H = 16: a contraction over K = 16, under the GEMM's 32-deep k-tile, M >= 4096
    (32, 3, 2, "softplus", 255, 0.3),       # small f32 GEMMs below M = 256
    (64, 6, 3, "relu", 1, 0.0),             # one edge, six layers
    (128, 4, 3, "softplus", 4095, 0.3),     # the fused architecture through NG_EDGE_PATH=layered, just under M = 4096
    (128, 4, 8, "relu", 70001, 0.3),        # relu at H = 128 (layered by default): split fwd / dw / dx, edge_out E = 8
    (256, 3, 64, "softplus", 4097, 0.3),    # H = 256: split GEMMs with dw8; E > 8: dense output layer + mask_rows
    (256, 2, 8, "relu", 255, 1.0),          # every slot dead: e and every gradient exactly 0
    (64, 2, 64, "relu", 4095, 0.0),         # E = 64 over H = 64, no dead slot
    (32, 4, 1, "softplus", 70001, 1.0),     # every slot dead at many rows
    (256, 4, 2, "softplus", 255, 0.0),      # H = 256 at M = 255: below the short-operand threshold of the split GEMM
    (128, 2, 2, "relu", 256, 0.3),          # M = 256 exactly
    (64, 3, 12, "relu", 4097, 0.3),         # E = 12 and 20 (a multiple of 4, not of 8): the wide output layer's dX GEMM
    (32, 2, 20, "softplus", 1001, 0.3),     #   contracts over E
]


@pytest.mark.parametrize("H,Le,E,act,n,dead", CASES)
def test_layered_edge_mlp_vs_float64(gpu_device, monkeypatch, H, Le, E, act, n, dead):
    """ng_edge_mlp_fwd / ng_edge_mlp_bwd on the layered path: e, z_save and every dW[t] / db[t] per element against float64,
    with d_eff != d_src (training noise); where the split-operand GEMMs run, no worse than 8 x the f32-input GEMMs' error
    (NG_GEMM_MATH=fp32) + 1e-6"""
    from nmrgnn_amd import _lib
    code = ACT[act]
    if H == 128 and Le == 4 and code == 1:
        monkeypatch.setenv("NG_EDGE_PATH", "layered")
    assert _lib.get_context(0).lib.ng_edge_live_supported(H, E, Le, code) == 0      # not the fused path
    rng = np.random.default_rng(H * 31 + Le * 7 + E + n)
    d_src = rng.uniform(0.05, 1.2, n)
    d_src[rng.random(n) < dead] = 0.0
    d_src = f32(d_src)
    d_eff = f32(np.where(d_src > 0, d_src + 0.025 * rng.standard_normal(n), d_src))
    assert dead == 1.0 or np.any(d_eff != d_src)
    centers = f32(np.linspace(0.0, 1.2, H))
    gap = float(np.float32(centers[1] - centers[0]))
    Ws = [f32(rng.standard_normal((H, H)) * (1.5 / np.sqrt(H))) for _ in range(Le - 1)]
    Ws.append(f32(rng.standard_normal((H, E)) / np.sqrt(H)))
    bs = [f32(0.1 * rng.standard_normal(H)) for _ in range(Le - 1)] + [f32(0.1 * rng.standard_normal(E))]
    de = f32(rng.standard_normal((n, E)))
    v, mg = ref_edge(d_src, d_eff, centers, gap, Ws, bs, de, code)

    def run():
        e, z, dW, db = run_gpu(gpu_device, H, E, Le, code, d_src, d_eff, centers, gap, Ws, bs, v["z_in"], de)
        if dead == 1.0:
            assert not np.any(e) and not any(np.any(x) for x in dW + db)
            assert not np.isnan(z).any()
        errs = {"e": check("e", e, v["e"], mg["e"])}
        for l in range(Le - 1):
            errs[f"z{l}"] = check(f"z_save[{l}]", z[l], v["z"][l], mg["z"][l])
        for l in range(Le):
            errs[f"dW{l}"] = check(f"dW[{l}]", dW[l], v["dW"][l], mg["dW"][l])
            errs[f"db{l}"] = check(f"db[{l}]", db[l], v["db"][l], mg["db"][l])
        return errs

    errs = run()
    if H >= 128 and n >= 4096:                  # split-operand GEMMs (gemm_h2_fwd_ok: H % 128 == 0, M >= 4096)
        monkeypatch.setenv("NG_GEMM_MATH", "fp32")
        ref32 = run()
        bad = {k: (errs[k], ref32[k]) for k in errs if errs[k] > 8.0 * ref32[k] + 1e-6}
        assert not bad, bad
