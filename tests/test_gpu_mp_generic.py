"""The generic MPLayer (csrc/mp_csr.hip: mp_generic_fwd / mp_generic_bwd, and aggregate() of csrc/node_ops.hip) against a
float64 numpy statement of nmrgnn/layers.py:26-46 + model.py:165-167 and its backward, element by element.

The generic path serves every (F, E) the window kernels do not take: F in {32, 128}, E outside {1, 2, 3} at F = 64, E = 8 / 64
at F = 256, and every CSR list.  Each case below names the branch it exists for.  Every output is filled with NaN before the
call, so an entry the kernels never write fails.  Bound per element: |got - ref| <= C_REL * mag + 1e-7 * max(mag), where mag is
the same expression evaluated on absolute values (activation slopes bounded by 1, plus |act(P)| for the activation's own
rounding).  Inputs are rounded to float32 first, so the reference is the exact value of what the kernels were handed."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C_REL = 3e-5
ACT = {"none": 0, "softplus": 1, "relu": 2, "tanh": 3}


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def act_fwd(act, P):
    if act == 1:
        return np.maximum(P, 0) + np.log1p(np.exp(-np.abs(P)))
    if act == 2:
        return np.maximum(P, 0)
    if act == 3:
        return np.tanh(P)
    return P


def act_grad_from_out(act, S):
    if act == 1:
        return -np.expm1(-S)
    if act == 2:
        return (S > 0).astype(np.float64)
    if act == 3:
        return 1.0 - S * S
    return np.ones_like(S)


def scatter_matrix(nl):
    """[N, N*K] sparse 0/1 matrix: row t sums the slots (i, j) with nl[i, j] == t"""
    from scipy.sparse import csr_matrix
    N, K = nl.shape
    return csr_matrix((np.ones(N * K), (nl.reshape(-1).astype(np.int64), np.arange(N * K))), shape=(N, N * K))


def ref_layer(h, nl, e, inv, w, dH, act, residual):
    """float64 forward and backward of one MPLayer over padded lists, with the per-element magnitudes of every output.
    The backward is handed s_save = the float64 S rounded to float32, as the kernels are."""
    N, K = nl.shape
    E, F = e.shape[2], h.shape[1]
    Wp = w.transpose(2, 0, 1).reshape(E * F, F)                 # Wp[n F + l][m] = w[l][m][n]
    Sc = scatter_matrix(nl)
    v, mg = {}, {}
    slope = None
    for out, hh, ee, WW, dd in ((v, h, e, Wp, dH), (mg, np.abs(h), np.abs(e), np.abs(Wp), np.abs(dH))):
        hg = hh[nl]                                             # [N, K, F]
        A = np.matmul(ee.transpose(0, 2, 1), hg)                # [N, E, F]
        P = inv[:, None] * (A.reshape(N, E * F) @ WW)
        out["A"] = A
        out["s"] = act_fwd(act, P) if out is v else P + np.abs(v["s"])   # + the activation's own rounding
        out["h_out"] = out["s"] + (hh if residual else 0.0)
        if slope is None:
            v["s_in"] = f32(out["s"])
            slope = act_grad_from_out(act, v["s_in"])
        dP = dd * (slope if out is v else np.abs(slope)) * inv[:, None]
        out["dw"] = (A.reshape(N, E * F).T @ dP).reshape(E, F, F).transpose(1, 2, 0)
        dA = (dP @ WW.T).reshape(N, E, F)
        out["de"] = np.matmul(hg, dA.transpose(0, 2, 1))        # [N, K, E]
        out["dh"] = dd + Sc @ np.matmul(ee, dA).reshape(N * K, F)
    return v, mg


def check(name, got, ref, mag, sel=None):
    """per-element bound; returns max|err| / max(mag) for the comparison with the f32-input GEMM run"""
    got = np.asarray(got, np.float64)
    if sel is not None:
        got, ref, mag = got[sel], ref[sel], mag[sel]
    err = np.abs(got - ref)
    top = float(mag.max()) if mag.size else 0.0
    bad = ~(err <= C_REL * mag + 1e-7 * top)                   # NaN fails
    if bad.any():
        k = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries outside the bound; first at flat {k}: "
                             f"got {got.reshape(-1)[k]!r} ref {ref.reshape(-1)[k]!r} mag {mag.reshape(-1)[k]!r}")
    return float(err.max()) / top if top > 0 else 0.0


# ---------------------------------------------------------------------------------------------------------- cases
def padded_case(F, E, K, N, span, act, residual, seed, hub=0, p_dead=0.1):
    """padded lists: graphs of `span` atoms (one graph when span == 0), neighbours inside the own graph; a `hub` > 0 sends
    that many live slots of every graph to one target"""
    rng = np.random.default_rng(seed)
    g = span if span else N
    base = (np.arange(N) // g) * g
    size = np.minimum(base + g, N) - base
    nl = (base[:, None] + (rng.random((N, K)) * size[:, None]).astype(np.int64)).astype(np.int32)
    live = rng.random((N, K)) >= p_dead
    if hub:
        t = min(300, N - 2)
        nl[(nl == t) & live] = t + 1
        slots = np.flatnonzero(live.reshape(-1))
        nl.reshape(-1)[rng.choice(slots, hub, replace=False)] = t
        assert int(((nl == t) & live).sum()) == hub
    e = f32(rng.standard_normal((N, K, E)) * np.where(live, 1.0, 0.0)[:, :, None])
    return dict(kind="padded", F=F, E=E, K=K, N=N, span=span, act=ACT[act], residual=residual, nl=nl, e=e, live=live,
                **_node_inputs(rng, N, F, E, K))


def csr_case(F, E, N, degrees, act, residual, seed, hub=0):
    """CSR lists with the given row lengths; neighbours anywhere in the batch; `hub` extra entries into one target"""
    rng = np.random.default_rng(seed)
    deg = np.asarray(degrees, np.int64)
    col = rng.integers(0, N, int(deg.sum())).astype(np.int32)
    if hub:
        t = N // 2
        col[col == t] = t + 1
        col[rng.choice(len(col), hub, replace=False)] = t
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(row_ptr[-1])
    e = f32(rng.standard_normal((nnz, E)))
    # the reference runs on the padded form with K = the longest row
    K = max(1, int(deg.max()))
    rows = np.repeat(np.arange(N), deg)
    slot = np.arange(nnz) - np.repeat(row_ptr[:-1], deg)
    nl = np.zeros((N, K), np.int32)
    nl[rows, slot] = col
    ep = np.zeros((N, K, E))
    ep[rows, slot] = e
    live = np.zeros((N, K), bool)
    live[rows, slot] = True
    return dict(kind="csr", F=F, E=E, K=K, N=N, span=0, act=ACT[act], residual=residual, nl=nl, e=ep, live=live,
                row_ptr=row_ptr, col=col, e_flat=e, rows=rows, slot=slot, **_node_inputs(rng, N, F, E, K))


def _node_inputs(rng, N, F, E, K):
    # weights scaled so that P stays O(1): activation slopes away from 0 (their float32 form is then good to a few ulp)
    return dict(h=f32(rng.standard_normal((N, F)) * 0.5), inv=f32(rng.uniform(0.05, 1.0, N)),
                w=f32(rng.standard_normal((F, F, E)) / np.sqrt(F * E * K)), dH=f32(rng.standard_normal((N, F))))


def degrees_with(rng, N, hi, must):
    d = rng.integers(0, hi + 1, N)
    d[:len(must)] = must
    return rng.permutation(d)


class GpuLayer:
    """the case's tensors on the device and the C entry points of its list form"""

    def __init__(self, case, dev):
        import torch
        from nmrgnn_amd import _lib
        from nmrgnn_amd.graph import GraphBatch
        self.c, self.dev = case, dev
        t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.t = t
        N, E = case["N"], case["E"]
        atoms = np.eye(10, dtype=np.float32)[np.arange(N) % 10]
        if case["kind"] == "padded":
            gb = GraphBatch(atoms, case["nl"], case["live"].astype(np.float32), case["inv"], device=dev)
            self.nlist = gb.nlist_c
            self.te = t(case["e"])
        else:
            gb = GraphBatch.from_csr(atoms, case["row_ptr"], case["col"], np.ones(len(case["col"]), np.float32),
                                     inv_degree=case["inv"], device=dev)
            self.row_ptr, self.col, self.row_of = gb.row_ptr, gb.nlist, gb.row_of
            self.te = t(case["e_flat"])
        self.csc_ptr, self.csc_edge = gb.csc()
        self.th, self.tinv, self.tw = t(case["h"]), t(case["inv"]), t(case["w"])
        self.ctx = _lib.get_context(0)
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.n_ent = N * case["K"] if case["kind"] == "padded" else len(case["col"])

    def nan(self, *shape):
        import torch
        return torch.full(shape, float("nan"), device=self.dev)

    def records(self):
        from nmrgnn_amd._lib import ptr
        c = self.c
        rec = self.nan(c["N"] * c["K"], 4)
        self.ctx.check(self.ctx.lib.ng_mp_edge_records(self.ctx.handle, self.st, c["N"], c["K"], c["E"], ptr(self.csc_ptr),
                                                       ptr(self.csc_edge), ptr(self.te), ptr(rec)), "records")
        return rec

    def aggregate(self):
        from nmrgnn_amd._lib import ptr
        c = self.c
        A = self.nan(c["N"], c["E"], c["F"])
        if c["kind"] == "padded":
            rc = self.ctx.lib.ng_mp_aggregate(self.ctx.handle, self.st, c["N"], c["K"], c["F"], c["E"], ptr(self.th),
                                              ptr(self.nlist), ptr(self.te), ptr(A))
        else:
            rc = self.ctx.lib.ng_mp_aggregate_csr(self.ctx.handle, self.st, c["N"], c["F"], c["E"], ptr(self.th),
                                                  ptr(self.row_ptr), ptr(self.col), ptr(self.te), ptr(A))
        self.ctx.check(rc, "aggregate")
        return A

    def fwd(self, h=None, keep_A=True):
        from nmrgnn_amd._lib import ptr
        c = self.c
        N, F, E = c["N"], c["F"], c["E"]
        h_out, s, A = self.nan(N, F), self.nan(N, F), (self.nan(N, E, F) if keep_A else None)
        th = self.th if h is None else h
        if c["kind"] == "padded":
            rc = self.ctx.lib.ng_mp_layer_fwd(self.ctx.handle, self.st, N, c["K"], F, E, c["act"], c["residual"], ptr(th),
                                              ptr(self.nlist), ptr(self.te), ptr(self.tinv), ptr(self.tw), ptr(h_out),
                                              ptr(A), ptr(s))
        else:
            rc = self.ctx.lib.ng_mp_layer_fwd_csr(self.ctx.handle, self.st, N, self.n_ent, F, E, c["act"], c["residual"],
                                                  ptr(th), ptr(self.row_ptr), ptr(self.col), ptr(self.te), ptr(self.tinv),
                                                  ptr(self.tw), ptr(h_out), ptr(A), ptr(s))
        self.ctx.check(rc, "fwd")
        return h_out, A, s

    def bwd(self, A, S, dH, h=None, rec=None, de_prior=None):
        """dh_in, de [entries, E], dw; de accumulates onto de_prior when given"""
        from nmrgnn_amd._lib import ptr
        c = self.c
        N, F, E = c["N"], c["F"], c["E"]
        dh, dw = self.nan(N, F), self.nan(F, F, E)
        de = self.nan(self.n_ent, E) if de_prior is None else de_prior.clone()
        acc = 0 if de_prior is None else 1
        th = self.th if h is None else h
        if c["kind"] == "csr":
            rc = self.ctx.lib.ng_mp_layer_bwd_csr(self.ctx.handle, self.st, N, self.n_ent, F, E, c["act"], ptr(th),
                                                  ptr(self.row_ptr), ptr(self.col), ptr(self.row_of), ptr(self.te),
                                                  ptr(self.tinv), ptr(self.tw), ptr(A), ptr(S), ptr(self.csc_ptr),
                                                  ptr(self.csc_edge), ptr(dH), ptr(dh), ptr(de), acc, ptr(dw))
        elif rec is None:
            rc = self.ctx.lib.ng_mp_layer_bwd(self.ctx.handle, self.st, N, c["K"], F, E, c["act"], ptr(th), ptr(self.nlist),
                                              ptr(self.te), ptr(self.tinv), ptr(self.tw), ptr(A), ptr(S), ptr(self.csc_ptr),
                                              ptr(self.csc_edge), ptr(dH), ptr(dh), ptr(de), acc, ptr(dw))
        else:
            rc = self.ctx.lib.ng_mp_layer_bwd_rec(self.ctx.handle, self.st, N, c["K"], F, E, c["act"], ptr(th),
                                                  ptr(self.nlist), ptr(self.te), ptr(self.tinv), ptr(self.tw), ptr(A),
                                                  ptr(S), ptr(self.csc_ptr), ptr(self.csc_edge), ptr(dH), ptr(dh), ptr(de),
                                                  acc, ptr(dw), ptr(rec))
        self.ctx.check(rc, "bwd")
        return dh, de, dw


def de_slots(case, de):
    """de of the kernels ([entries, E]) in the padded [N, K, E] form of the reference"""
    de = de.cpu().numpy().astype(np.float64)
    if case["kind"] == "padded":
        return de.reshape(case["N"], case["K"], case["E"])
    out = np.zeros((case["N"], case["K"], case["E"]))
    out[case["rows"], case["slot"]] = de
    return out


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
