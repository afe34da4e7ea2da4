"""Molecule-sized inference kernels (csrc/frame_fused.hip): the FC block + head in one launch against the layered path
(ng_fc_block_fwd + ng_head_fwd) and against a float64 statement of nmrgnn/model.py:191-196,268-273; one MPLayer in one launch
(padded and CSR lists) against ng_mp_layer_fwd(_csr) and float64.  Outputs are filled with NaN before every call.

  ng_fc_head_fwd (fc_head_short_kernel)     C in {1, 10, 16}; one-hot and dense atoms (an all-zero row); N in {1, 32, 16384} and the
                                            sizes of a molecule; N = 16385 and C = 17 refused (ng_fc_head_ok agrees); rows beyond
                                            the fp16 range and a weight beyond the piece range in layer 0 / layer 3 (every row takes
                                            the in-kernel fp32 recomputation), unfrozen and frozen
  mp_layer_short_kernel<E, CSR, NS>         all twelve instances: E in {1, 2, 3} x padded / CSR x two workgroups per tile (NS = 2,
                                            2 tiles <= num_cu) / one; N from the CU count on both sides of the rule, the side
                                            asserted; residual 0 / 1, act 0 .. 3, K in {1, 5, 32}; frozen, two rounds; a weight
                                            beyond the piece range; an exact family (act none and relu: integers, sparse +-1
                                            weights, inv a power of two) that must equal float64 bit for bit
Criteria: 3e-5 of max(sum_c |a_c| std_c, 1) for the head (one-hot atoms: max(std, 1)); 5e-6 of max(mag, 1) for the MPLayer, mag =
inv (|A| @ |w|) + |h| with A the signed aggregate (|h| only with the residual)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F, Lf, NC = 256, 4, 10


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


STD = np.array([0, 0, 10.6, 50.9, 6.04, 0, 1, 2, 0.5, 1, 3.0, 0.25, 40.0, 1.5, 0, 7.0], np.float32)
AVG = np.array([0, 0, 126.0, 118.9, 5.63, 0, 1, -2, 3, 0, 60.0, -1.0, 100.0, 4.0, 2.5, 30.0], np.float32)


def _case(N, seed, big_rows=0, C=NC, dense=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, F)).astype(np.float32)
    if big_rows:
        rows = rng.choice(N, big_rows, replace=False)
        x[rows, rng.integers(0, F, big_rows)] = 2.0e5            # beyond the fp16 range of a piece
    W = [(rng.standard_normal((F, F)) * 0.06).astype(np.float32) for _ in range(3)] + \
        [(rng.standard_normal((F, F // 2)) * 0.06).astype(np.float32)]
    b = [(rng.standard_normal(F) * 0.1).astype(np.float32) for _ in range(3)] + [(rng.standard_normal(F // 2) * 0.1).astype(np.float32)]
    Wout = (rng.standard_normal((F // 2, C)) * 0.1).astype(np.float32)
    bout = (rng.standard_normal(C) * 0.1).astype(np.float32)
    elem = rng.integers(0, C, N)
    atoms = np.eye(C, dtype=np.float32)[elem]
    if dense:                                                     # rows that are not one-hot, and an all-zero row
        atoms = np.where(rng.random((N, C)) < 0.5, rng.standard_normal((N, C)), 0.0).astype(np.float32)
        atoms[N // 2] = 0.0
    std, avg = (STD[2:3], AVG[2:3]) if C == 1 else (STD[:C].copy(), AVG[:C].copy())
    return x, W, b, Wout, bout, atoms, std, avg


def _ref(x, W, b, Wout, bout, atoms, std, avg):
    h = x.astype(np.float64)
    for l in range(3):
        h = softplus(h @ W[l].astype(np.float64) + b[l]) + h
    g = softplus(h @ W[3].astype(np.float64) + b[3])
    full = g @ Wout.astype(np.float64) + bout
    return (atoms * (full * std + avg)).sum(1)


def _run(dev, case, frozen):
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr, ptr_array
    x, W, b, Wout, bout, atoms, std, avg = case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tx, tW, tb = t(x), [t(w) for w in W], [t(v) for v in b]
    tWo, tbo, ta, ts, tv = t(Wout), t(bout), t(atoms), t(std), t(avg)
    N, C_ = x.shape[0], Wout.shape[1]
    ctx = _lib.get_context(0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    peaks = torch.full((N,), float("nan"), device=dev)
    if frozen:
        # a fresh owner per case: the cache is keyed by weight ADDRESSES, and torch hands the addresses of the previous
        # case's (freed) weights to this one
        _run.owner = getattr(_run, "owner", 40000) + 1
        ctx.check(ctx.lib.ng_weights_frozen(ctx.handle, _run.owner), "freeze")
    try:
        for _ in range(2 if frozen else 1):        # second call: images served from the cache
            ctx.check(ctx.lib.ng_fc_head_fwd(ctx.handle, st, N, F, Lf, C_, 1, ptr(tx), ptr_array(tW), ptr_array(tb), ptr(tWo), ptr(tbo),
                                             ptr(ta), ptr(ts), ptr(tv), ptr(peaks)), "ng_fc_head_fwd")
    finally:
        ctx.lib.ng_weights_frozen(ctx.handle, 0)
    # the layered path on the same inputs
    ys = [torch.full((N, F), float("nan"), device=dev) for _ in range(3)]
    g = torch.full((N, F // 2), float("nan"), device=dev)
    ctx.check(ctx.lib.ng_fc_block_fwd(ctx.handle, st, N, F, Lf, 1, ptr(tx), ptr_array(tW), ptr_array(tb), ptr_array(ys), ptr(g)), "fc")
    lay = torch.full((N,), float("nan"), device=dev)
    ctx.check(ctx.lib.ng_head_fwd(ctx.handle, st, N, F // 2, C_, ptr(g), None, ptr(tWo), ptr(tbo), ptr(ta), ptr(ts), ptr(tv),
                                  ptr(lay)), "head")
    torch.cuda.synchronize()
    return peaks.cpu().numpy().astype(np.float64), lay.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("N,frozen", [(2770, True), (2770, False), (31, False), (33, True), (8000, True)])
def test_fused_fc_head_equals_float64_and_the_layered_path(gpu_device, N, frozen):
    case = _case(N, seed=N)
    ref = _ref(*case)
    fused, lay = _run(gpu_device, case, frozen)
    std_of = case[6][np.argmax(case[5], 1)].astype(np.float64)
    scale = np.maximum(std_of, 1.0)
    assert np.isfinite(fused).all()
    assert np.max(np.abs(fused - ref) / scale) < 3e-5
    assert np.max(np.abs(fused - lay) / scale) < 3e-5
    assert np.all(fused[std_of == 0] == case[7][np.argmax(case[5], 1)][std_of == 0])     # std = 0: exactly avg


def test_fused_fc_head_repairs_rows_beyond_the_fp16_range(gpu_device):
    case = _case(2770, seed=5, big_rows=40)
    ref = _ref(*case)
    fused, lay = _run(gpu_device, case, True)
    std_of = case[6][np.argmax(case[5], 1)].astype(np.float64)
    scale = np.maximum(std_of, 1.0) * np.maximum(1.0, np.abs(ref) / 100.0)
    assert np.isfinite(fused).all() and np.isfinite(lay).all()
    assert np.max(np.abs(fused - ref) / scale) < 1e-3 * 1.0
    assert np.max(np.abs(fused - ref) / np.maximum(np.abs(ref), 1.0)) < 1e-4


def _mp_case(N, K, E, seed, big_rows=0):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((N, F)).astype(np.float32)
    if big_rows:
        h[rng.choice(N, big_rows, replace=False), 7] = 3.0e5
    nlist = rng.integers(0, N, (N, K)).astype(np.int32)
    e = (rng.standard_normal((N, K, E)) * 0.3).astype(np.float32)
    e[rng.random((N, K)) < 0.1] = 0.0
    inv = (1.0 / rng.integers(1, K + 1, N)).astype(np.float32)
    w = (rng.standard_normal((F, F, E)) * 0.02).astype(np.float32)
    return h, nlist, e, inv, w


@pytest.mark.parametrize("N,K,E,act,big", [(2770, 16, 3, 1, 0), (100, 16, 3, 1, 0), (33, 5, 2, 3, 0), (2770, 16, 3, 1, 25),
                                           (6000, 32, 1, 2, 0)])
def test_fused_mp_layer_equals_float64_and_the_layered_path(gpu_device, N, K, E, act, big):
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    h, nlist, e, inv, w = _mp_case(N, K, E, N + K, big)
    A = np.einsum("ijn,ijl->inl", e.astype(np.float64), h.astype(np.float64)[nlist])            # [N][E][F]
    pre = inv[:, None].astype(np.float64) * np.einsum("inl,lmn->im", A, w.astype(np.float64))
    actf = {1: softplus, 2: lambda x: np.maximum(x, 0), 3: np.tanh}[act]
    ref = actf(pre) + h
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    th, tn, te, ti, tw = t(h), t(nlist), t(e), t(inv), t(w)
    ctx = _lib.get_context(0)
    st = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    out = torch.full((N, F), float("nan"), device=gpu_device)
    ctx.check(ctx.lib.ng_mp_layer_fwd_short(ctx.handle, st, N, K, F, E, act, 1, ptr(th), ptr(tn), ptr(te), ptr(ti), ptr(tw), ptr(out)),
              "ng_mp_layer_fwd_short")
    lay = torch.full((N, F), float("nan"), device=gpu_device)
    ctx.check(ctx.lib.ng_mp_layer_fwd(ctx.handle, st, N, K, F, E, act, 1, ptr(th), ptr(tn), ptr(te), ptr(ti), ptr(tw), ptr(lay),
                                      None, None), "ng_mp_layer_fwd")
    torch.cuda.synchronize()
    got, lay = out.cpu().numpy().astype(np.float64), lay.cpu().numpy().astype(np.float64)
    # an output is a 768-term sum: its rounding error scales with the sum of |terms| (large aggregates cancel), not with
    # the result
    mag = np.maximum(inv[:, None] * np.einsum("inl,lmn->im", np.abs(A), np.abs(w.astype(np.float64))) + np.abs(h), 1.0)
    assert np.isfinite(got).all()
    assert np.max(np.abs(got - ref) / mag) < 5e-6        # (repaired rows: a plain fp32 chain over 768 terms)
    assert np.max(np.abs(lay - ref) / mag) < 5e-6
    # in-place use is refused (other atoms still gather the input rows)
    assert ctx.lib.ng_mp_layer_fwd_short(ctx.handle, st, N, K, F, E, act, 1, ptr(th), ptr(tn), ptr(te), ptr(ti), ptr(tw), ptr(th)) != 0


@pytest.mark.parametrize("N,E", [(2770, 3), (77, 2)])
def test_fused_mp_layer_over_csr_lists(gpu_device, N, E):
    """variable degree (0 ... 40 entries per row, one row with 300): the CSR form of the one-launch MPLayer"""
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    rng = np.random.default_rng(N)
    deg = rng.integers(0, 41, N)
    deg[3] = 0
    deg[N // 2] = 300
    row_ptr = np.zeros(N + 1, np.int32)
    row_ptr[1:] = np.cumsum(deg)
    nnz = int(row_ptr[-1])
    col = rng.integers(0, N, nnz).astype(np.int32)
    e = (rng.standard_normal((nnz, E)) * 0.3).astype(np.float32)
    h = rng.standard_normal((N, F)).astype(np.float32)
    inv = (1.0 / np.maximum(deg, 1)).astype(np.float32)
    w = (rng.standard_normal((F, F, E)) * 0.02).astype(np.float32)
    rows = np.repeat(np.arange(N), deg)
    A = np.zeros((N, E, F))
    np.add.at(A, rows, e.astype(np.float64)[:, :, None] * h.astype(np.float64)[col][:, None, :])
    pre = inv[:, None].astype(np.float64) * np.einsum("inl,lmn->im", A, w.astype(np.float64))
    ref = softplus(pre) + h
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    th, tr, tc, te, ti, tw = t(h), t(row_ptr), t(col), t(e), t(inv), t(w)
    ctx = _lib.get_context(0)
    st = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    out = torch.full((N, F), float("nan"), device=gpu_device)
    ctx.check(ctx.lib.ng_mp_layer_fwd_short_csr(ctx.handle, st, N, F, E, 1, 1, ptr(th), ptr(tr), ptr(tc), ptr(te), ptr(ti), ptr(tw),
                                                ptr(out)), "ng_mp_layer_fwd_short_csr")
    lay = torch.full((N, F), float("nan"), device=gpu_device)
    ctx.check(ctx.lib.ng_mp_layer_fwd_csr(ctx.handle, st, N, nnz, F, E, 1, 1, ptr(th), ptr(tr), ptr(tc), ptr(te), ptr(ti), ptr(tw),
                                          ptr(lay), None, None), "ng_mp_layer_fwd_csr")
    torch.cuda.synchronize()
    mag = np.maximum(inv[:, None] * np.einsum("inl,lmn->im", np.abs(A), np.abs(w.astype(np.float64))) + np.abs(h), 1.0)
    for got in (out.cpu().numpy().astype(np.float64), lay.cpu().numpy().astype(np.float64)):
        assert np.isfinite(got).all()
        assert np.max(np.abs(got - ref) / mag) < 5e-6


# ------------------------------------------------------------------------------------------------- the remaining head branches
NG_ERR_UNSUPPORTED = -4


def _head_scale(case):
    """max(sum_c |a_c| std_c, 1): max(std, 1) of the row's element for one-hot atoms"""
    atoms, std = case[5].astype(np.float64), case[6].astype(np.float64)
    return np.maximum(np.abs(atoms) @ std, 1.0)


@pytest.mark.parametrize("dense", [False, True], ids=["onehot", "dense"])
@pytest.mark.parametrize("C", [1, 10, 16])
@pytest.mark.parametrize("N", [1, 32, 16384])
def test_fused_fc_head_element_counts_atom_rows_and_sizes(gpu_device, N, C, dense):
    """C = 1 and C = 16 (the last supported), atom rows that are not one-hot and one that is all zero, one row, one tile and the
    last supported N; unfrozen for the one-hot cases, frozen (two rounds) for the dense ones"""
    case = _case(N, seed=1000 * C + N % 977 + int(dense), C=C, dense=dense)
    ref = _ref(*case)
    fused, lay = _run(gpu_device, case, frozen=dense)
    scale = _head_scale(case)
    assert np.isfinite(fused).all() and np.isfinite(lay).all()
    assert np.max(np.abs(fused - ref) / scale) < 3e-5
    assert np.max(np.abs(fused - lay) / scale) < 3e-5
    if dense:
        assert fused[N // 2] == 0.0                                          # the all-zero atom row
    else:
        std_of = case[6][np.argmax(case[5], 1)]
        assert np.all(fused[std_of == 0] == case[7][np.argmax(case[5], 1)][std_of == 0])     # std = 0: exactly avg


@pytest.mark.parametrize("N,C", [(16385, 10), (16384, 17), (16385, 17)])
def test_fused_fc_head_refuses_what_it_does_not_support(gpu_device, N, C):
    import ctypes

    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr, ptr_array
    ctx = _lib.get_context(0)
    assert ctx.lib.ng_fc_head_ok(16384, F, Lf, 16, 1) == 1
    assert ctx.lib.ng_fc_head_ok(N, F, Lf, C, 1) == 0
    rng = np.random.default_rng(N + C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu_device)
    tx = t(rng.standard_normal((N, F)))
    tW = [t(rng.standard_normal((F, F)) * 0.06) for _ in range(3)] + [t(rng.standard_normal((F, F // 2)) * 0.06)]
    tb = [t(np.zeros(F)) for _ in range(3)] + [t(np.zeros(F // 2))]
    tWo, tbo, ta, ts, tv = t(np.zeros((F // 2, C))), t(np.zeros(C)), t(np.zeros((N, C))), t(np.ones(C)), t(np.zeros(C))
    peaks = torch.full((N,), float("nan"), device=gpu_device)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    rc = ctx.lib.ng_fc_head_fwd(ctx.handle, st, N, F, Lf, C, 1, ptr(tx), ptr_array(tW), ptr_array(tb), ptr(tWo), ptr(tbo), ptr(ta), ptr(ts),
                                ptr(tv), ptr(peaks))
    torch.cuda.synchronize()
    assert rc == NG_ERR_UNSUPPORTED
    assert bool(peaks.isnan().all())


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("layer", [0, 3])
def test_fused_fc_head_weight_beyond_the_piece_range(gpu_device, layer, frozen):
    """2^8 * 300 >= 65504: that weight has no fp16 pieces (its image entry is inf), every row's accumulator is non-finite and every
    row takes the in-kernel fp32 recomputation (ff_repair_rows).  Layer 0: on an input column of 1e-2; layer 3: negative, on a
    hidden column that is positive in nearly every row — the outputs stay O(1) and the file's criterion holds as it is."""
    N = 2770
    x, W, b, Wout, bout, atoms, std, avg = _case(N, seed=17 + layer)
    if layer == 0:
        x[:, 3] *= 0.01
        W[0][3, 5] = 300.0
    else:
        W[3][3, 5] = -300.0
    assert 256.0 * 300.0 >= 65504.0
    case = (x, W, b, Wout, bout, atoms, std, avg)
    ref = _ref(*case)
    fused, lay = _run(gpu_device, case, frozen)
    scale = _head_scale(case)
    assert np.isfinite(fused).all() and np.isfinite(lay).all()
    print("max err / scale: fused", np.max(np.abs(fused - ref) / scale), "layered", np.max(np.abs(lay - ref) / scale))
    assert np.max(np.abs(fused - ref) / scale) < 3e-5
    assert np.max(np.abs(fused - lay) / scale) < 3e-5


# ------------------------------------------------------------------------------------------------- every MPLayer instance
ACTF = {0: lambda v: v, 1: softplus, 2: lambda v: np.maximum(v, 0), 3: np.tanh}


def _num_cu(dev):
    import torch
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def _n_for(split, cu):
    """a ragged N on the wanted side of `2 * tiles <= num_cu` (two workgroups per tile while that fits the chip in one round)"""
    tiles = cu // 2 if split else cu // 2 + 1
    N = 32 * tiles - 5
    assert -(-N // 32) == tiles and (2 * tiles <= cu) == split and 0 < N <= 16384
    return N


def _mp_lists(rng, N, K, E, csr, exact=False):
    """(nl [N][Kp], e [N][Kp][E] padded form for the reference; row_ptr, col, e_flat for the CSR call or None)"""
    draw_e = (lambda *sh: rng.integers(-1, 2, sh).astype(np.float32)) if exact else \
        (lambda *sh: (rng.standard_normal(sh) * 0.3).astype(np.float32))
    if not csr:
        nl = rng.integers(0, N, (N, K)).astype(np.int32)
        e = draw_e(N, K, E)
        e[rng.random((N, K)) < 0.1] = 0.0
        deg = np.full(N, K)
        return nl, e, deg, None
    deg = rng.integers(0, 41, N)
    deg[3 % N] = 0
    deg[N // 2] = 300
    row_ptr = np.zeros(N + 1, np.int32)
    row_ptr[1:] = np.cumsum(deg)
    nnz = int(row_ptr[-1])
    col = rng.integers(0, N, nnz).astype(np.int32)
    ef = draw_e(nnz, E)
    rows = np.repeat(np.arange(N), deg)
    slot = np.arange(nnz) - np.repeat(row_ptr[:-1], deg)
    nl = np.zeros((N, 300), np.int32)
    e = np.zeros((N, 300, E), np.float32)
    nl[rows, slot], e[rows, slot] = col, ef
    return nl, e, deg, (row_ptr, col, ef, nnz)


class _Mp:
    def __init__(self, dev):
        import torch
        from nmrgnn_amd import _lib
        self.torch, self.dev = torch, dev
        self.ctx = _lib.get_context(0)
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def run(self, N, K, E, act, residual, th, lists, ti, tw, layered=True):
        """(short kernel's output, layered path's output) as float64"""
        from nmrgnn_amd._lib import ptr
        ctx, st = self.ctx, self.st
        nan = lambda: self.torch.full((N, F), float("nan"), device=self.dev)
        out, lay = nan(), nan()
        if len(lists) == 2:
            tn, te = lists
            ctx.check(ctx.lib.ng_mp_layer_fwd_short(ctx.handle, st, N, K, F, E, act, residual, ptr(th), ptr(tn), ptr(te), ptr(ti), ptr(tw),
                                                    ptr(out)), "ng_mp_layer_fwd_short")
            if layered:
                ctx.check(ctx.lib.ng_mp_layer_fwd(ctx.handle, st, N, K, F, E, act, residual, ptr(th), ptr(tn), ptr(te), ptr(ti), ptr(tw),
                                                  ptr(lay), None, None), "ng_mp_layer_fwd")
        else:
            tr, tc, te, nnz = lists
            ctx.check(ctx.lib.ng_mp_layer_fwd_short_csr(ctx.handle, st, N, F, E, act, residual, ptr(th), ptr(tr), ptr(tc), ptr(te), ptr(ti),
                                                        ptr(tw), ptr(out)), "ng_mp_layer_fwd_short_csr")
            if layered:
                ctx.check(ctx.lib.ng_mp_layer_fwd_csr(ctx.handle, st, N, nnz, F, E, act, residual, ptr(th), ptr(tr), ptr(tc), ptr(te),
                                                      ptr(ti), ptr(tw), ptr(lay), None, None), "ng_mp_layer_fwd_csr")
        self.torch.cuda.synchronize()
        return out.cpu().numpy().astype(np.float64), (lay.cpu().numpy().astype(np.float64) if layered else None)

    def lists(self, nl, e, csr):
        if csr is None:
            return (self.up(nl), self.up(e))
        row_ptr, col, ef, nnz = csr
        return (self.up(row_ptr), self.up(col), self.up(ef), nnz)


def _mp_ref(h, nl, e, inv, w):
    """(pre-activation, its magnitude inv * (|A| @ |w|) with A the signed aggregate, as in the tests above, and the sum of the absolute
    values of every term, for the exact family's 2^24 condition) in float64"""
    h64, w64 = h.astype(np.float64), w.astype(np.float64)
    N, E = h.shape[0], e.shape[2]
    A, Am = np.zeros((N, E, F)), np.zeros((N, E, F))
    for j in range(nl.shape[1]):                                   # slot by slot: no [N][K][E][F] intermediate
        live = np.any(e[:, j] != 0, axis=1)
        if not live.any():
            continue
        hj = h64[nl[live, j]]
        A[live] += e[live, j].astype(np.float64)[:, :, None] * hj[:, None, :]
        Am[live] += np.abs(e[live, j]).astype(np.float64)[:, :, None] * np.abs(hj)[:, None, :]
    Wp = w64.transpose(2, 0, 1).reshape(E * F, F)
    i64 = inv.astype(np.float64)[:, None]
    A2, Wa = A.reshape(N, E * F), np.abs(Wp)
    return i64 * (A2 @ Wp), i64 * (np.abs(A2) @ Wa), i64 * (Am.reshape(N, E * F) @ Wa)


INSTANCES = [(E, csr, split) for E in (1, 2, 3) for csr in (False, True) for split in (True, False)]
INST_IDS = [f"E{E}-{'csr' if c else 'padded'}-{'split' if s else 'unsplit'}" for E, c, s in INSTANCES]


@pytest.mark.parametrize("E,csr,split", INSTANCES, ids=INST_IDS)
def test_every_short_mp_layer_instance(gpu_device, E, csr, split):
    """mp_layer_short_kernel<E, CSR, NS> for all twelve (E, CSR, NS), residual 0 and 1, the four activations, K in {1, 5, 32} (padded
    form): float64 and the layered path to 5e-6 of max(mag, 1)"""
    gpu = _Mp(gpu_device)
    N = _n_for(split, _num_cu(gpu_device))
    for K in ((None,) if csr else (1, 5, 32)):
        rng = np.random.default_rng([E, int(csr), int(split), K or 0])
        nl, e, deg, lists = _mp_lists(rng, N, K, E, csr)
        h = rng.standard_normal((N, F)).astype(np.float32)
        inv = (1.0 / np.maximum(rng.integers(1, 33, N) if not csr else deg, 1)).astype(np.float32)
        w = (rng.standard_normal((F, F, E)) * 0.02).astype(np.float32)
        pre, pmag, _ = _mp_ref(h, nl, e, inv, w)
        th, ti, tw, tl = gpu.up(h), gpu.up(inv), gpu.up(w), gpu.lists(nl, e, lists)
        for act in (0, 1, 2, 3):
            for residual in (0, 1):
                ref = ACTF[act](pre) + (h if residual else 0.0)
                mag = np.maximum(pmag + (np.abs(h) if residual else 0.0), 1.0)
                got, lay = gpu.run(N, K or 1, E, act, residual, th, tl, ti, tw)
                tag = (K, act, residual)
                assert np.isfinite(got).all() and np.isfinite(lay).all(), tag
                assert np.max(np.abs(got - ref) / mag) < 5e-6, tag
                assert np.max(np.abs(lay - ref) / mag) < 5e-6, tag


@pytest.mark.parametrize("E,csr,split", INSTANCES, ids=INST_IDS)
def test_short_mp_layer_exact_integers(gpu_device, E, csr, split):
    """h in {-2..2}, e in {-1, 0, 1}, w with about four +-1 per output column, inv a power of two, act none and relu: every
    aggregate is an integer of at most 11 bits (one fp16 piece holds it) and every sum stays below 2^24 units, so the output must
    equal float64 bit for bit — a dropped or doubled neighbour, k-step or column block cannot hide"""
    gpu = _Mp(gpu_device)
    N = _n_for(split, _num_cu(gpu_device))
    K = None if csr else 16
    rng = np.random.default_rng([E, int(csr), int(split), 9])
    nl, e, deg, lists = _mp_lists(rng, N, K, E, csr, exact=True)
    h = rng.integers(-2, 3, (N, F)).astype(np.float32)
    inv = np.exp2(-rng.integers(0, 4, N)).astype(np.float32)
    w = np.where(rng.random((F, F, E)) < 4.0 / (E * F), rng.choice([-1.0, 1.0], (F, F, E)), 0.0).astype(np.float32)
    pre, _, pmag = _mp_ref(h, nl, e, inv, w)
    A_top = np.abs(e).astype(np.float64).sum(1).max() * 2.0                # |A| <= sum_j |e_j| max|h|
    assert A_top < 2048 and pmag.max() / inv.min() < 2.0 ** 24 and (pmag + np.abs(h)).max() * 8 < 2.0 ** 24
    th, ti, tw, tl = gpu.up(h), gpu.up(inv), gpu.up(w), gpu.lists(nl, e, lists)
    for act in (0, 2):
        for residual in (0, 1):
            ref = ACTF[act](pre) + (h if residual else 0.0)
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
            got, _ = gpu.run(N, K or 1, E, act, residual, th, tl, ti, tw, layered=False)
            bad = ~(got == ref)
            assert not bad.any(), (act, residual, int(bad.sum()), np.argwhere(bad)[:3].tolist())


@pytest.mark.parametrize("E,csr", [(1, False), (2, True), (3, False), (3, True), (1, True)])
def test_short_mp_layer_frozen_rounds_and_a_weight_beyond_the_range(gpu_device, E, csr):
    """ng_weights_frozen: the second call, served from the kept image, repeats the first and the unfrozen call bit for bit.  Then a
    weight with 2^8 |w| >= 65504 (inf in the image): the rows it reaches are recomputed in fp32 inside the kernel and meet the
    float64 bound, frozen and unfrozen."""
    gpu = _Mp(gpu_device)
    ctx = gpu.ctx
    N, K = 2770, (None if csr else 16)
    rng = np.random.default_rng([E, int(csr), 21])
    nl, e, deg, lists = _mp_lists(rng, N, K, E, csr)
    h = rng.standard_normal((N, F)).astype(np.float32)
    inv = (1.0 / np.maximum(deg, 1)).astype(np.float32)
    w = (rng.standard_normal((F, F, E)) * 0.02).astype(np.float32)
    th, ti, tl = gpu.up(h), gpu.up(inv), gpu.lists(nl, e, lists)
    for big in (False, True):
        if big:
            w = w.copy()
            w[3, 5, E - 1] = 300.0
        pre, pmag, _ = _mp_ref(h, nl, e, inv, w)
        ref, mag = softplus(pre) + h, np.maximum(pmag + np.abs(h), 1.0)
        tw = gpu.up(w)
        plain, _ = gpu.run(N, K or 1, E, 1, 1, th, tl, ti, tw, layered=False)
        _run.owner = getattr(_run, "owner", 40000) + 1
        ctx.check(ctx.lib.ng_weights_frozen(ctx.handle, _run.owner), "freeze")
        try:
            rounds = [gpu.run(N, K or 1, E, 1, 1, th, tl, ti, tw, layered=False)[0] for _ in range(2)]
        finally:
            ctx.lib.ng_weights_frozen(ctx.handle, 0)
        for got in [plain] + rounds:
            assert np.isfinite(got).all()
            assert np.max(np.abs(got - ref) / mag) < 5e-6, big
        assert np.array_equal(rounds[0], plain) and np.array_equal(rounds[1], plain), big
