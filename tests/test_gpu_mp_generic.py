"""The generic MPLayer (csrc/mp_csr.hip: mp_generic_fwd / mp_generic_bwd, and aggregate() of csrc/node_ops.hip) against a
float64 numpy statement of nmrgnn/layers.py:26-46 + model.py:165-167 and its backward, element by element.

The generic path serves every (F, E) the window kernels do not take: F in {32, 128}, E outside {1, 2, 3} at F = 64, E = 8 / 64
at F = 256, and every CSR list.  Each case below names the branch it exists for.  Every output is filled with NaN before the
call, so an entry the kernels never write fails.  Bound per element: |got - ref| <= C_REL * mag + 1e-7 * max(mag), where mag is
the same expression evaluated on absolute values (activation slopes bounded by 1, plus |act(P)| for the activation's own
rounding).  Inputs are rounded to float32 first, so the reference is the exact value of what the kernels were handed."""
import numpy as np
import pytest

# the float64 reference, the case builders and the device wrapper are shared with test_gpu_mp_window.py
from mp_layer_gpu import GpuLayer, de_slots
from mp_layer_ref import check, csr_case, degrees_with, padded_case, ref_layer

pytestmark = pytest.mark.gpu


def uses_split_gemms(case):
    """gemm_h2_fwd_ok / gemm_h2_dw_ok on the layer's products (M = N rows, E*F by F)"""
    return case["N"] >= 4096 and case["F"] % 128 == 0


def run_and_check(case, dev, exact_props=True):
    """forward and backward against float64 (the backward handed the forward's A_save); returns the normalised error of
    every tensor.  exact_props: also the bit-for-bit properties of the backward's variants."""
    import torch
    g = GpuLayer(case, dev)
    ctx = g.ctx
    live = torch.from_numpy(case["live"].reshape(-1) if case["kind"] == "padded" else np.ones(g.n_ent, bool)).to(dev)
    v, mg = ref_layer(case["h"], case["nl"], case["e"], case["inv"], case["w"], case["dH"], case["act"], case["residual"])
    ctx.check(ctx.lib.ng_ctx_set_graph_span(ctx.handle, case["span"]), "span")
    try:
        h_out, A, s = g.fwd()
        A_only = g.aggregate()
        tS, tdH = g.t(v["s_in"]), g.t(case["dH"])
        dh, de, dw = g.bwd(A, tS, tdH)
        torch.cuda.synchronize()
        errs = {"h_out": check("h_out", h_out.cpu().numpy(), v["h_out"], mg["h_out"]),
                "s_save": check("s_save", s.cpu().numpy(), v["s"], mg["s"]),
                "A_save": check("A_save", A.cpu().numpy(), v["A"], mg["A"]),
                "dh_in": check("dh_in", dh.cpu().numpy(), v["dh"], mg["dh"]),
                "de": check("de", de_slots(case, de), v["de"], mg["de"], sel=case["live"]),
                "dw": check("dw", dw.cpu().numpy(), v["dw"], mg["dw"])}
        check("aggregate", A_only.cpu().numpy(), v["A"], mg["A"])
        if exact_props:
            # the aggregate rebuilt inside the backward (A_save = NULL) is the forward's: same bits
            dh2, de2, dw2 = g.bwd(None, tS, tdH)
            assert torch.equal(dh2, dh) and torch.equal(dw2, dw) and torch.equal(de2[live], de[live])
            # de_accum = 1 adds the de_accum = 0 result to the prior, one rounding per element
            prior = g.t(np.random.default_rng(1).standard_normal((g.n_ent, case["E"])))
            dh3, de3, dw3 = g.bwd(A, tS, tdH, de_prior=prior)
            assert torch.equal(de3[live], (prior + de)[live]) and torch.equal(dh3, dh) and torch.equal(dw3, dw)
            # the two source-read branches of the wide pull: supplied records or the csc_edge -> e chain
            if case["kind"] == "padded" and case["E"] <= 3:
                dh4, de4, dw4 = g.bwd(A, tS, tdH, rec=g.records())
                assert torch.equal(dh4, dh) and torch.equal(dw4, dw) and torch.equal(de4[live], de[live])
    finally:
        ctx.check(ctx.lib.ng_ctx_set_graph_span(ctx.handle, 0), "span")
    return errs


PADDED = [
    # F, E, K, N, span, act, residual, hub       meant to reach
    (128, 3, 16, 1000, 0, "softplus", 1, 0),     # aggregate_kernel; wide edge-grad and pull at LPA 8, EC 3
    (128, 1, 8, 4801, 200, "relu", 0, 0),        # agg_win_kernel, egrad_win_kernel at F = 128; split dense fwd / dw / dx
    (128, 2, 12, 4500, 300, "tanh", 1, 0),       # span above the window: wide kernels at split-GEMM size
    (128, 3, 16, 5000, 256, "softplus", 0, 4097),  # one hub target: a long CSC segment in the wide pull
    (128, 8, 16, 700, 0, "softplus", 1, 0),      # generic kernels EC 8 at 32 lanes per atom
    (128, 64, 9, 300, 0, "tanh", 0, 0),          # E chunk loop at F = 128
    (32, 2, 16, 4099, 256, "tanh", 1, 0),        # F = 32 (32 atoms per block); f32 dense with Nout = 32 < tile
    (32, 3, 5, 33, 0, "relu", 0, 0),             # K not a multiple of 4; ragged last block
    (32, 64, 16, 1000, 0, "softplus", 1, 0),     # E = 64 beyond the 150-atom model tests
    (64, 8, 16, 5000, 256, "softplus", 0, 0),    # F = 64 off the window kernels (they take E <= 3)
    (256, 8, 16, 4100, 256, "softplus", 1, 0),   # generic EC 8 at one atom per wave; dw8 on Kin = 2048
]


@pytest.mark.parametrize("F,E,K,N,span,act,residual,hub", PADDED)
def test_generic_layer_padded_vs_float64(gpu_device, monkeypatch, F, E, K, N, span, act, residual, hub):
    """padded lists through ng_mp_layer_fwd / ng_mp_layer_bwd(_rec) / ng_mp_aggregate: every output element against the
    float64 statement; A_save NULL == given, records == none, de_accum = prior + overwrite, all bit for bit.  Where the
    split-operand GEMMs run, the error is also no worse than 8 x that of the f32-input GEMMs (NG_GEMM_MATH=fp32) + 1e-6."""
    case = padded_case(F, E, K, N, span, act, residual, seed=F * 7 + E * 3 + N, hub=hub)
    errs = run_and_check(case, gpu_device)
    if uses_split_gemms(case):
        monkeypatch.setenv("NG_GEMM_MATH", "fp32")
        ref32 = run_and_check(case, gpu_device, exact_props=False)
        bad = {k: (errs[k], ref32[k]) for k in errs if errs[k] > 8.0 * ref32[k] + 1e-6}
        assert not bad, bad


def _csr_cases():
    rng = np.random.default_rng(11)
    return [
        # F, E, N, degrees, act, residual, hub              meant to reach
        (128, 3, 5000, degrees_with(rng, 5000, 40, [0, 1, 3, 4, 5, 7, 8, 9]), "relu", 1, 0),   # csr_aggregate_kernel tails;
        #                                                   wide kernels with unequal rows in one wave
        (32, 8, 2000, degrees_with(rng, 2000, 33, [0, 1, 8, 33]), "tanh", 0, 0),   # generic CSR kernels, EC 8, 8-lane reduce
        (64, 64, 800, degrees_with(rng, 800, 20, [0, 1, 20]), "softplus", 1, 0),   # E chunk loop over RowRange rows
        (256, 1, 3000, degrees_with(rng, 3000, 16, [0, 1, 2]), "none", 0, 700),    # wide kernels at LPA 16 over CSR; hub
    ]


@pytest.mark.parametrize("ci", range(4))
def test_generic_layer_csr_vs_float64(gpu_device, ci):
    """CSR lists through ng_mp_layer_fwd_csr / ng_mp_layer_bwd_csr / ng_mp_aggregate_csr: every output element against the
    float64 statement of the same rows padded to the longest one; A_save NULL == given and de_accum bit for bit"""
    F, E, N, deg, act, residual, hub = _csr_cases()[ci]
    case = csr_case(F, E, N, deg, act, residual, seed=100 + ci, hub=hub)
    run_and_check(case, gpu_device)


def test_padded_and_csr_forms_agree_bit_for_bit_at_f128(gpu_device):
    """F = 128: the same rows as a padded list (dead slots e = 0) and as CSR (dead slots dropped) give the same bits on
    the generic kernels (aggregate_kernel / csr_aggregate_kernel, the wide edge-grad and pull at LPA 8)"""
    import torch
    case = padded_case(128, 3, 16, 1200, 0, "softplus", 1, seed=5, p_dead=0.25)
    live = case["live"]
    deg = live.sum(1)
    rows, slots = np.nonzero(live)
    cc = dict(case, kind="csr", row_ptr=np.concatenate([[0], np.cumsum(deg)]).astype(np.int32),
              col=case["nl"][rows, slots].astype(np.int32), e_flat=case["e"][rows, slots], rows=rows, slot=slots)
    gp, gc = GpuLayer(case, gpu_device), GpuLayer(cc, gpu_device)
    hp, Ap, sp = gp.fwd()
    hc, Ac, sc = gc.fwd()
    assert torch.equal(hp, hc) and torch.equal(Ap, Ac) and torch.equal(sp, sc)
    dH = gp.t(case["dH"])
    dhp, dep, dwp = gp.bwd(Ap, sp, dH)
    dhc, dec, dwc = gc.bwd(Ac, sc, dH)
    assert torch.equal(dhp, dhc) and torch.equal(dwp, dwc)
    assert torch.equal(dep[torch.from_numpy(live.reshape(-1)).to(gpu_device)], dec)


def _window_case(seed=9):
    return padded_case(128, 3, 16, 4801, 200, "softplus", 1, seed=seed)


@pytest.mark.parametrize("shift", [-20, 12])
def test_generic_backward_scales_exactly_with_the_upstream_gradient(gpu_device, shift):
    """F = 128 / E = 3 / N = 4801 with the window kernels and the split-operand GEMMs (power-of-two gradient scale):
    dH * 2^shift gives dh_in, de and dw times 2^shift bit for bit"""
    import torch
    case = _window_case()
    g = GpuLayer(case, gpu_device)
    ctx = g.ctx
    ctx.check(ctx.lib.ng_ctx_set_graph_span(ctx.handle, case["span"]), "span")
    try:
        _, A, S = g.fwd()
        base = g.bwd(A, S, g.t(case["dH"]))
        moved = g.bwd(A, S, g.t(case["dH"] * 2.0 ** shift))
        torch.cuda.synchronize()
    finally:
        ctx.check(ctx.lib.ng_ctx_set_graph_span(ctx.handle, 0), "span")
    live = torch.from_numpy(case["live"].reshape(-1)).to(gpu_device)
    for k, (a, b) in enumerate(zip(moved, base)):
        if k == 1:
            a, b = a[live], b[live]
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(a, b * 2.0 ** shift), k


def test_operands_beyond_the_fp16_range_meet_the_float64_bound(gpu_device):
    """the same shape with 50 features of h at +-3e5 (A entries beyond the fp16 range of the split-operand pieces): the
    products' range guard hands them to the f32-input kernel, and every element still meets the float64 bound"""
    case = _window_case(seed=13)
    rng = np.random.default_rng(2)
    flat = case["h"].reshape(-1)
    flat[rng.choice(flat.size, 50, replace=False)] = 3e5 * rng.choice([-1.0, 1.0], 50)
    run_and_check(case, gpu_device, exact_props=False)
