"""Library calls on a context whose scratch is EMPTY (tests/cold_ctx.py): the state a new user meets on a first call, and the
one no other test sees — every other file shares one context per pytest process, whose workspaces are as large as the largest
shape any earlier test ran.

Oracle everywhere: the bits of the same call on the warm shared context.  The library is bitwise deterministic
(tests/test_gpu_determinism.py), and scratch offsets, num_cu and split counts do not depend on how a block came to exist, so a
difference is a defect (a pointer kept across a growth of its block, a block read before it was filled), never rounding.  The
shapes of each case come from a float64 test of its family (named beside it), which pins the warm bits to the reference.

Every cold run proves its own precondition from ng_ctx_scratch_info (the context really was cold, a block really grew, the
arena really held two chunks, the queue really overflowed): a scenario whose precondition fails, FAILS.

Scenarios: A first call, B steady state (the header's "allocates nothing once its scratch is sized"), C grow in place,
D grow under load, E arena born inside a deferral window, F reduction queue overflow, G ng_ctx_reserve, H engine level
(training step, shape order, frozen weights, graph replays).

STEADY_STATE_EXCEPTIONS lists the allocations in steady state that are by design (none of ws / aux may ever be listed)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from cold_ctx import assert_same, cold_context, set_state, stream_ptr, to_host, warm_reference

pytestmark = pytest.mark.gpu

SOFTPLUS, RELU = 1, 2
MIB = 1 << 20
NG_SMALL_BYTES = 64 * 1024
RB_MAX_JOBS = 24          # capi.hip

# case name -> (file:line that allocates, why) for cases allowed to allocate in steady state (scenario B).  Growth of the main or
# the aux workspace may never be listed here.
STEADY_STATE_EXCEPTIONS = {}


# ------------------------------------------------------------------------------------------------------------------ device helpers
def _up(dev, a, dt=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def _nan(dev, *shape):
    import torch
    return torch.full(shape, float("nan"), device=dev)


def _ints(dev, *shape):
    import torch
    return torch.full(shape, -7, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------------------------ the cases
# A case: prepare(dev, big) -> inputs on the device (built ONCE per shape, on the warm context, never written afterwards), and
# run(ctx, dev, s) -> {name: device tensor(s)}: launches only, no host synchronisation (scenario D relies on it).
class Case:
    def __init__(self, name, prepare, run, span=0, env=None, needs=("ws_bytes",)):
        """needs: the blocks the issue's table lists for the case: scenario A asserts that the first call gave birth to each"""
        self.name, self.prepare, self.run, self.span, self.env, self.needs = name, prepare, run, span, env or {}, tuple(needs)


@contextlib.contextmanager
def switches(env):
    """NG_* path switches of a case for the calls inside (the library parses them once: ng_reload_env), the previous values
    behind them"""
    from nmrgnn_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    if env:
        _lib.reload_env()
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if env:
            _lib.reload_env()


def _dense_prepare(K, N, Ms):
    """K: the contraction, or (small, big) where the scratch does not depend on the row count"""
    Ks = K if isinstance(K, tuple) else (K, K)

    def prepare(dev, big):
        M, K = (Ms[1], Ks[1]) if big else (Ms[0], Ks[0])
        rng = np.random.default_rng([M, K, N])
        return dict(M=M, K=K, N=N, X=_up(dev, rng.standard_normal((M, K))), W=_up(dev, rng.standard_normal((K, N)) / np.sqrt(K)),
                    b=_up(dev, 0.1 * rng.standard_normal(N)), dY=_up(dev, rng.standard_normal((M, N))))
    return prepare


def _dense_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr
    M, K, N = s["M"], s["K"], s["N"]
    st = stream_ptr(dev)
    Y, S, dX, dW, dB = _nan(dev, M, N), _nan(dev, M, N), _nan(dev, M, K), _nan(dev, K, N), _nan(dev, N)
    ctx.check(ctx.lib.ng_dense_fwd(ctx.handle, st, M, K, N, SOFTPLUS, 0, ptr(s["X"]), ptr(s["W"]), ptr(s["b"]), ptr(Y), ptr(S)),
              "ng_dense_fwd")
    ctx.check(ctx.lib.ng_dense_bwd(ctx.handle, st, M, K, N, SOFTPLUS, 0, ptr(s["X"]), ptr(s["W"]), ptr(S), ptr(s["dY"]), ptr(dX),
                                   ptr(dW), ptr(dB)), "ng_dense_bwd")
    return dict(Y=Y, S=S, dX=dX, dW=dW, dB=dB)


def _mp_prepare(kind, F, E, Ns, span, K=16):
    def prepare(dev, big):
        from mp_layer_gpu import GpuLayer
        from mp_layer_ref import csr_case, degrees_with, padded_case
        N = Ns[1] if big else Ns[0]
        if kind == "padded":
            case = padded_case(F, E, K, N, span, "softplus", 1, seed=F * 7 + E * 3 + N)
        else:
            deg = degrees_with(np.random.default_rng(N), N, 20, [0, 1, 3, 20])
            case = csr_case(F, E, N, deg, "softplus", 1, seed=100 + N)
        g = GpuLayer(case, dev)              # (its lists are built here, on the warm context)
        rec = g.records() if kind == "padded" and E <= 3 else None
        return dict(g=g, case=case, dH=g.t(case["dH"]), rec=rec)
    return prepare


def _mp_run(ctx, dev, s):
    g = s["g"]
    g.ctx, g.st = ctx, stream_ptr(dev)
    h_out, A, S = g.fwd()
    out = dict(h_out=h_out, A=A, S=S)
    h_inf, _, _ = g.fwd(keep_A=False)                            # inference form: no aggregate kept
    out["h_inf"] = h_inf
    live = None
    variants = [("given", dict(A=A)), ("rebuilt", dict(A=None)), ("no_dw", dict(A=A, want_dw=False))]
    if s["rec"] is not None:
        variants.append(("rec", dict(A=A, rec=s["rec"])))
    for tag, kw in variants:
        A_in = kw.pop("A")
        dh, de, dw = g.bwd(A_in, S, s["dH"], **kw)
        out[f"dh_{tag}"], out[f"dw_{tag}"] = dh, dw
        # dead slots of de are unspecified in the padded form: compare the live ones
        if s["case"]["kind"] == "padded":
            import torch
            if live is None:
                live = torch.from_numpy(s["case"]["live"].reshape(-1)).to(dev)
            de = de[live]
        out[f"de_{tag}"] = de
    return out


def _edge_prepare(H, Le, E, ns, act=RELU, fused=False, out_of_range=False):
    """fused: the shape of the fused kernels (tape in their own layout, same size).  out_of_range: one hidden weight beyond the
    fp16 piece range (2^8 |w| >= 65504): the pack launch raises the range guard and the call runs its fp32-input bodies"""
    def prepare(dev, big):
        import edge_layered_ref as R
        n = ns[1] if big else ns[0]
        c = R.normal_case(H, Le, E, act, n)
        if out_of_range:
            c["Ws"][1][3, 5] = np.float32(400.0)
        return dict(fused=fused, c=c, d=_up(dev, c["d_src"]), f=_up(dev, c["d_eff"]), cen=_up(dev, c["centers"]),
                    W=[_up(dev, w) for w in c["Ws"]],
                    b=[_up(dev, b) for b in c["bs"]], de=_up(dev, c["de"]))
    return prepare


def _edge_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr, ptr_array
    c = s["c"]
    n, H, E, Le = c["n"], c["H"], c["E"], c["Le"]
    lib, st = ctx.lib, stream_ptr(dev)
    assert bool(lib.ng_edge_live_supported(H, E, Le, c["act"])) == s["fused"]
    assert s["fused"] or int(lib.ng_edge_tape_layout(H, E, Le, c["act"], n)) == 0
    e, z, e_inf = _nan(dev, n, E), _nan(dev, (Le - 1) * n, H), _nan(dev, n, E)
    args = (n, H, E, Le, c["act"], ptr(s["d"]), ptr(s["f"]), ptr(s["cen"]), float(c["gap"]), ptr_array(s["W"]))
    ctx.check(lib.ng_edge_mlp_fwd(ctx.handle, st, *args, ptr_array(s["b"]), ptr(e), ptr(z)), "ng_edge_mlp_fwd")
    ctx.check(lib.ng_edge_mlp_fwd(ctx.handle, st, *args, ptr_array(s["b"]), ptr(e_inf), None), "ng_edge_mlp_fwd (no tape)")
    kouts = [H] * (Le - 1) + [E]
    dW, db = [_nan(dev, H, k) for k in kouts], [_nan(dev, k) for k in kouts]
    ctx.check(lib.ng_edge_mlp_bwd(ctx.handle, st, *args, ptr(z), ptr(s["de"]), ptr_array(dW), ptr_array(db)), "ng_edge_mlp_bwd")
    return dict(e=e, z=z, e_inf=e_inf, dW=dW, db=db)


def _fc_prepare(F, L, Ns):
    def prepare(dev, big):
        import fc_block_ref as FR
        N = Ns[1] if big else Ns[0]
        x, Ws, bs, dg = FR.normal_data(np.random.default_rng([N, F, L]), N, F, L)
        return dict(N=N, F=F, L=L, x=_up(dev, x), W=[_up(dev, w) for w in Ws], b=[_up(dev, b) for b in bs], dg=_up(dev, dg))
    return prepare


def _fc_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr, ptr_array
    N, F, L = s["N"], s["F"], s["L"]
    lib, st = ctx.lib, stream_ptr(dev)
    ys, g = [_nan(dev, N, F) for _ in range(L - 1)], _nan(dev, N, F // 2)
    ctx.check(lib.ng_fc_block_fwd(ctx.handle, st, N, F, L, SOFTPLUS, ptr(s["x"]), ptr_array(s["W"]), ptr_array(s["b"]), ptr_array(ys),
                                  ptr(g)), "ng_fc_block_fwd")
    dx, dW, db = _nan(dev, N, F), [_nan(dev, *w.shape) for w in s["W"]], [_nan(dev, w.shape[1]) for w in s["W"]]
    scratch = _nan(dev, max(int(lib.ng_fc_block_scratch_floats(N, F, L)), 3 * N * F))
    tape = [s["x"]] + ys
    ctx.check(lib.ng_fc_block_bwd(ctx.handle, st, N, F, L, SOFTPLUS, ptr_array(tape), ptr(g), ptr_array(s["W"]), ptr(s["dg"]), ptr(dx),
                                  ptr_array(dW), ptr_array(db), ptr(scratch)), "ng_fc_block_bwd")
    return dict(ys=ys, g=g, dx=dx, dW=dW, db=db)


def _head_prepare(Ns, Fh=32, Cn=10):
    def prepare(dev, big):
        N = Ns[1] if big else Ns[0]
        rng = np.random.default_rng([N, Fh, Cn])
        atoms = np.eye(Cn, dtype=np.float32)[rng.integers(0, Cn, N)]
        return dict(N=N, Fh=Fh, C=Cn, g=_up(dev, rng.standard_normal((N, Fh))), Wout=_up(dev, rng.standard_normal((Fh, Cn)) / 6),
                    atoms=_up(dev, atoms), std=_up(dev, rng.uniform(0.5, 2.0, Cn)), dp=_up(dev, rng.standard_normal(N)),
                    dh0=_up(dev, rng.standard_normal((N, 2 * Fh))), mask=_up(dev, 1.25 * (rng.uniform(size=(N, Fh)) < 0.8)))
    return prepare


def _head_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr
    N, Fh, Cn = s["N"], s["Fh"], s["C"]
    lib, st = ctx.lib, stream_ptr(dev)
    dg, dW, db = _nan(dev, N, Fh), _nan(dev, Fh, Cn), _nan(dev, Cn)
    ctx.check(lib.ng_head_bwd(ctx.handle, st, N, Fh, Cn, ptr(s["g"]), ptr(s["mask"]), ptr(s["Wout"]), ptr(s["atoms"]), ptr(s["std"]), ptr(s["dp"]),
                              ptr(dg), ptr(dW), ptr(db)), "ng_head_bwd")
    return dict(dg=dg, dWout=dW, dbout=db)


def _embed_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr
    N, F, Cn = s["N"], 2 * s["Fh"], s["C"]
    dW = _nan(dev, Cn, F)
    ctx.check(ctx.lib.ng_embed_bwd(ctx.handle, stream_ptr(dev), N, Cn, F, ptr(s["atoms"]), ptr(s["dh0"]), ptr(dW)), "ng_embed_bwd")
    return dict(dWemb=dW)


def _restraint_prepare(ns, R=3):
    def prepare(dev, big):
        n = ns[1] if big else ns[0]
        rng = np.random.default_rng([n, R])
        return dict(n=n, R=R, peaks=_up(dev, rng.standard_normal(R * n)), y=_up(dev, rng.standard_normal(n)),
                    w=_up(dev, rng.uniform(0, 1, n)))
    return prepare


def _restraint_run(ctx, dev, s):
    import torch
    from nmrgnn_amd._lib import ptr
    energy = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    dp = _nan(dev, s["R"] * s["n"])
    ctx.check(ctx.lib.ng_restraint_loss(ctx.handle, stream_ptr(dev), s["R"], s["n"], ptr(s["peaks"]), ptr(s["y"]), ptr(s["w"]),
                                        ptr(energy), ptr(dp)), "ng_restraint_loss")
    return dict(energy=energy, dpeaks=dp)


def _restraint_ex_run(ctx, dev, s):
    """independent replicas (NG_RESTRAINT_INDEPENDENT = 1) with a flat bottom: one energy per replica"""
    import torch
    from nmrgnn_amd._lib import ptr
    energy = torch.full((s["R"],), float("nan"), dtype=torch.float64, device=dev)
    dp = _nan(dev, s["R"] * s["n"])
    ctx.check(ctx.lib.ng_restraint_loss_ex(ctx.handle, stream_ptr(dev), s["R"], s["n"], 1, ptr(s["peaks"]), ptr(s["y"]), ptr(s["w"]),
                                           None, ptr(s["w"]), 0.0, None, None, ptr(energy), ptr(dp)), "ng_restraint_loss_ex")
    return dict(energy=energy, dpeaks=dp)


def _moments_prepare(ns, n_ids=40, K=8, Kc=50):
    def prepare(dev, big):
        N = ns[1] if big else ns[0]
        rng = np.random.default_rng([N, n_ids, K])
        return dict(N=N, n_ids=n_ids, K=K, Kc=Kc, y=_up(dev, rng.standard_normal(N)), w=_up(dev, rng.random(N) * (rng.random(N) > 0.2)),
                    pred=_up(dev, rng.standard_normal(N)), names=_up(dev, rng.integers(-1, n_ids + 1, N), np.int32),
                    member=_up(dev, rng.integers(0, 1 << K, n_ids), np.uint32).view(__import__("torch").int32),
                    class_of=_up(dev, rng.integers(-1, Kc, (2, n_ids)), np.int32))
    return prepare


def _name_metrics_run(ctx, dev, s):
    import torch
    from nmrgnn_amd._lib import ptr
    mom = torch.full((s["K"], 7), float("nan"), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.ng_name_metrics(ctx.handle, stream_ptr(dev), s["N"], ptr(s["y"]), ptr(s["w"]), ptr(s["names"]), ptr(s["pred"]),
                                      s["n_ids"], ptr(s["member"]), s["K"], 0, ptr(mom)), "ng_name_metrics")
    return dict(moments=mom)


def _class_moments_run(ctx, dev, s):
    import torch
    from nmrgnn_amd._lib import ptr
    mom = torch.full((s["Kc"], 7), float("nan"), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.ng_class_moments(ctx.handle, stream_ptr(dev), s["N"], ptr(s["y"]), ptr(s["w"]), ptr(s["names"]), ptr(s["pred"]),
                                       s["n_ids"], 2, ptr(s["class_of"]), s["Kc"], 0, ptr(mom)), "ng_class_moments")
    return dict(moments=mom)


def _reweight_prepare(Ts, M=64):
    def prepare(dev, big):
        T = Ts[1] if big else Ts[0]
        rng = np.random.default_rng([T, M])
        return dict(T=T, M=M, S=_up(dev, rng.standard_normal((T, M))), y=_up(dev, 0.1 * rng.standard_normal(M)),
                    lam=_up(dev, 0.05 * rng.standard_normal(M), np.float64))
    return prepare


def _reweight_run(ctx, dev, s):
    import torch
    from nmrgnn_amd._lib import ptr
    out = torch.full((1 + s["M"],), float("nan"), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.ng_reweight_eval(ctx.handle, stream_ptr(dev), s["T"], s["M"], ptr(s["S"]), ptr(s["y"]), None, ptr(s["lam"]),
                                       ptr(out)), "ng_reweight_eval")
    # the weights at the logZ just computed (a device double), and their two statistics
    p = torch.full((s["T"],), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.ng_reweight_weights(ctx.handle, stream_ptr(dev), s["T"], s["M"], ptr(s["S"]), ptr(s["y"]), None, ptr(s["lam"]),
                                          ptr(out), ptr(p), ptr(stats)), "ng_reweight_weights")
    return dict(out=out, p=p, stats=stats)


def _table_prepare(ns, E=3, T=4096):
    def prepare(dev, big):
        n = ns[1] if big else ns[0]
        rng = np.random.default_rng([n, E, T])
        d = rng.uniform(0.05, 1.2, n) * (rng.random(n) >= 0.2)
        d_eff = np.where(d > 0, d + 0.01 * rng.standard_normal(n), d)
        return dict(n=n, E=E, T=T, d=_up(dev, d), f=_up(dev, d_eff), de=_up(dev, rng.standard_normal((n, E))))
    return prepare


def _table_run(ctx, dev, s):
    """ng_edge_table_range (aux) of the call's distances and gradients, then ng_edge_table_scatter (ws partials) onto that range"""
    from nmrgnn_amd._lib import ptr
    n, E, T = s["n"], s["E"], s["T"]
    lib, st = ctx.lib, stream_ptr(dev)
    rng4, de_tab = _nan(dev, 4), _nan(dev, 2 * T, E)
    ctx.check(lib.ng_edge_table_range(ctx.handle, st, n, E, ptr(s["d"]), ptr(s["f"]), None, ptr(s["de"]), 0.0, ptr(rng4)),
              "ng_edge_table_range")
    ctx.check(lib.ng_edge_table_scatter(ctx.handle, st, n, E, T, 2 * T, ptr(s["d"]), ptr(s["f"]), None, ptr(rng4), ptr(s["de"]),
                                        ptr(de_tab)), "ng_edge_table_scatter")
    return dict(range=rng4[:3], de_tab=de_tab)


def _labels_prepare(Rs, Cc=10):
    def prepare(dev, big):
        import torch
        R = Rs[1] if big else Rs[0]
        rng = np.random.default_rng([R, Cc])
        sizes = rng.integers(1, 300, R)
        rec_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(rec_ptr[-1])
        atoms = np.zeros((n, Cc), np.float32)
        atoms[np.arange(n), rng.integers(0, Cc, n)] = 1.0
        y = np.stack([rng.normal(100.0, 30.0, n), rng.integers(0, 50, n), rng.random(n) < 0.7], axis=1).astype(np.float32)
        return dict(R=R, n=n, C=Cc, atoms=_up(dev, atoms), y=_up(dev, y), rec_ptr=torch.from_numpy(rec_ptr).to(dev),
                    ids=_up(dev, rng.permutation(R), np.int32))
    return prepare


def _labels_run(ctx, dev, s):
    import torch
    from nmrgnn_amd._lib import ptr
    out = torch.full((s["C"], 3), float("nan"), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.ng_label_moments(ctx.handle, stream_ptr(dev), s["R"], s["n"], s["C"], ptr(s["atoms"]), ptr(s["y"]),
                                       ptr(s["rec_ptr"]), ptr(s["ids"]), s["R"], ptr(out)), "ng_label_moments")
    return dict(moments=out)


def _box_prepare(Gs, n=100, K=16):
    def prepare(dev, big):
        G = Gs[1] if big else Gs[0]
        N = G * n
        rng = np.random.default_rng([G, n, K])
        i = np.arange(N)[:, None]
        nlist = (i // n) * n + (i % n + rng.integers(1, n, (N, K))) % n      # inside the frame, never the atom itself
        edges = rng.uniform(0.05, 1.2, (N, K)) * (rng.random((N, K)) >= 0.2)
        return dict(N=N, K=K, G=G, pos=_up(dev, rng.uniform(0, 20, (N, 3))), nlist=_up(dev, nlist, np.int32), edges=_up(dev, edges),
                    dd=_up(dev, rng.standard_normal((N, K))), gp=_up(dev, np.arange(G + 1) * n, np.int32))
    return prepare


def _box_run(ctx, dev, s):
    """open boundaries (triclinic = -1: no box, no dvec): the strain of every frame"""
    import torch
    from nmrgnn_amd._lib import ptr
    strain = torch.full((s["G"], 9), float("nan"), dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.ng_box_grad(ctx.handle, stream_ptr(dev), s["N"], s["K"], ptr(s["pos"]), ptr(s["nlist"]), ptr(s["edges"]),
                                  ptr(s["dd"]), 0.1, s["G"], ptr(s["gp"]), None, -1, ptr(strain), None), "ng_box_grad")
    return dict(strain=strain)


def _knn_prepare(ns, K=16):
    def prepare(dev, big):
        n = ns[1] if big else ns[0]
        side = 3.0 * n ** (1.0 / 3.0)
        return dict(n=n, K=K, pos=_up(dev, np.random.default_rng([n, K]).uniform(0, side, (1, n, 3))))
    return prepare


def _knn_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr
    n, K = s["n"], s["K"]
    nl, ed, inv = _ints(dev, n, K), _nan(dev, n, K), _nan(dev, n)
    ctx.check(ctx.lib.ng_knn_graph(ctx.handle, stream_ptr(dev), 1, n, K, 0.1, ptr(s["pos"]), ptr(nl), ptr(ed), ptr(inv)), "ng_knn_graph")
    return dict(nlist=nl, edges=ed, inv_degree=inv)


def _mp_short_prepare(Es, Ns, F=256, K=16):
    """the frame-fused MPLayer: its image (aux) is sized by E, not by the rows: the big shape has E = 3"""
    def prepare(dev, big):
        from mp_layer_gpu import GpuLayer
        from mp_layer_ref import padded_case
        E, N = (Es[1], Ns[1]) if big else (Es[0], Ns[0])
        case = padded_case(F, E, K, N, 0, "softplus", 1, seed=F + E + N)
        return dict(g=GpuLayer(case, dev), case=case)
    return prepare


def _mp_short_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr
    g, c = s["g"], s["case"]
    assert ctx.lib.ng_mp_layer_short_ok(c["N"], c["K"], c["F"], c["E"]) == 1
    out = _nan(dev, c["N"], c["F"])
    ctx.check(ctx.lib.ng_mp_layer_fwd_short(ctx.handle, stream_ptr(dev), c["N"], c["K"], c["F"], c["E"], c["act"], 1, ptr(g.th),
                                            ptr(g.nlist), ptr(g.te), ptr(g.tinv), ptr(g.tw), ptr(out)), "ng_mp_layer_fwd_short")
    return dict(h_out=out)


def _clip_prepare(ns):
    def prepare(dev, big):
        n = ns[1] if big else ns[0]
        return dict(n=n, g=_up(dev, np.random.default_rng(n).standard_normal(n)))
    return prepare


def _clip_run(ctx, dev, s):
    import torch
    from nmrgnn_amd._lib import ptr
    out2 = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    b, e, sc = (C.c_int64 * 1)(0), (C.c_int64 * 1)(s["n"]), (C.c_float * 1)(1.0)
    ctx.check(ctx.lib.ng_grad_clip_factor(ctx.handle, stream_ptr(dev), s["n"], ptr(s["g"]), 1.0, 1, b, e, sc, 1.0, ptr(out2)),
              "ng_grad_clip_factor")
    return dict(out2=out2)


def _lists_prepare(ns, K=16):
    def prepare(dev, big):
        N = ns[1] if big else ns[0]
        rng = np.random.default_rng([N, K])
        edges = rng.uniform(0.05, 1.2, (N, K)) * (rng.random((N, K)) >= 0.2)
        return dict(N=N, K=K, edges=_up(dev, edges), nlist=_up(dev, rng.integers(0, N, (N, K)), np.int32),
                    deg=_up(dev, rng.integers(0, 40, N * K), np.int32))
    return prepare


def _live_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr
    n = s["N"] * s["K"]
    perm, pos, d_c, n_live = _ints(dev, n), _ints(dev, n), _nan(dev, n), _ints(dev, 1)
    ctx.check(ctx.lib.ng_build_live_edges(ctx.handle, stream_ptr(dev), n, ptr(s["edges"]), ptr(perm), ptr(pos), ptr(d_c), ptr(n_live)),
              "ng_build_live_edges")
    return dict(perm=perm, pos=pos, d_c=d_c, n_live=n_live)      # (prefilled: rows the call leaves alone compare equal too)


def _scan_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr
    n = s["N"] * s["K"]
    out = _ints(dev, n + 1)
    ctx.check(ctx.lib.ng_exclusive_scan_i32(ctx.handle, stream_ptr(dev), n, ptr(s["deg"]), ptr(out)), "ng_exclusive_scan_i32")
    return dict(row_ptr=out)


def _incoming_run(ctx, dev, s):
    from nmrgnn_amd._lib import ptr
    N, K = s["N"], s["K"]
    nlist_c, csc_ptr, csc_edge = _ints(dev, N, K), _ints(dev, N + 1), _ints(dev, N * K)
    ctx.check(ctx.lib.ng_build_incoming_lists(ctx.handle, stream_ptr(dev), N, K, N * K, ptr(s["nlist"]), ptr(s["edges"]), ptr(nlist_c),
                                              ptr(csc_ptr), ptr(csc_edge)), "ng_build_incoming_lists")
    return dict(nlist_c=nlist_c, csc_ptr=csc_ptr, csc_edge=csc_edge)


_HEAD = _head_prepare((100, 3000))
_RESTRAINT = _restraint_prepare((1000, 200000))
_MOMENTS = _moments_prepare((500, 200000))
# (up to 16384 slots the list builders run in one launch without scratch: graph_ops.hip GL_SMALL_SLOTS)
_LISTS = _lists_prepare((1100, 20000))
CASES = [
    # tests/test_gpu_dense.py: the tall kernels (Kin, Nout <= 64: "tall64x64") — two workspace requests in one entry point.
    # Their scratch is sized by num_cu and the padded contraction, not by the rows (tall_tn.hip: tall_tn_scratch_floats):
    # the big shape is "tall192x64"
    Case("dense_tall_64x32", _dense_prepare((64, 192), 32, (300, 2048)), _dense_run),
    # the same 64 x 32 product on the generic kernels (tests/test_gpu_dense.py SETTINGS "generic"): split-K partials + db
    Case("dense_generic_64x32", _dense_prepare(64, 32, (300, 2048)), _dense_run, env={"NG_DENSE_PATH": "generic"}),
    # tests/test_gpu_dense.py "h2short-768x256": split-operand GEMM (range-guard word of the small scratch), dW partials + db
    Case("dense_768x256", _dense_prepare(768, 256, (300, 2048)), _dense_run, needs=("ws_bytes", "aux_bytes", "small_bytes")),
    # tests/test_gpu_mp_generic.py PADDED (32, 3, ...) / test_gpu_mp_default_width.py: ws held over the nested dense_* calls
    Case("mp_f32", _mp_prepare("padded", 32, 3, (150, 1357), 0), _mp_run),
    Case("mp_f256", _mp_prepare("padded", 256, 3, (150, 1357), 0), _mp_run),
    # the gather-GEMM / window forms of the default width want the graph span: tests/test_gpu_mp_gg.py (span 256)
    # (NG_MP_GG_MIN_ROWS: the gather-GEMM, whose image and tiles live in the aux workspace, at these row counts)
    Case("mp_f256_span256", _mp_prepare("padded", 256, 3, (150, 1357), 256), _mp_run, span=256, env={"NG_MP_GG_MIN_ROWS": "1"},
         needs=("ws_bytes", "aux_bytes", "small_bytes")),
    # tests/test_gpu_mp_generic.py _csr_cases
    Case("mp_f32_csr", _mp_prepare("csr", 32, 3, (150, 1357), 0), _mp_run),
    # tests/test_gpu_mp_window.py: the F = 64 window kernels (IK_MPW_* images in ws, partials).  The weight-gradient partials
    # are sized by num_cu (13 MB at 256 CUs); the rows add 512 bytes each (mp_win_bwd.hip: dP + records): 20000 rows outgrow
    # the 1.5 x headroom of the first call
    Case("mp_f64_window", _mp_prepare("padded", 64, 3, (150, 20000), 0), _mp_run, needs=("ws_bytes", "small_bytes")),
    # tests/test_gpu_edge_layered_kernels.py ("tape-H64-...", H = 64: no fused kernels): ws + aux images
    Case("edge_layered_h64", _edge_prepare(64, 3, 3, (200, 5000)), _edge_run),
    # tests/test_gpu_edge_h2.py (H = 128, four layers, softplus; n = 255 / 5000): the fused kernels and their weight images,
    # and the same call with a weight beyond the piece range (tests/test_gpu_edge_fused.py: the guarded fall-back)
    # The f32 fall-back launch of the split-operand forward is issued on EVERY call (its workgroups return at once unless the
    # guard word is up: the host cannot know), so its IMG_AUX image is born in both cases (edge_fused.hip: edge_fused_fwd_f32)
    Case("edge_fused_h128", _edge_prepare(128, 4, 3, (255, 5000), SOFTPLUS, fused=True), _edge_run,
         needs=("ws_bytes", "aux_bytes", "small_bytes")),
    Case("edge_fused_h128_guard", _edge_prepare(128, 4, 3, (255, 5000), SOFTPLUS, fused=True, out_of_range=True), _edge_run,
         needs=("ws_bytes", "aux_bytes", "small_bytes")),
    # tests/test_gpu_fc_block.py: fused (F = 64, L = 4), layered by depth (L = 5) and by width (F = 256)
    Case("fc_fused_f64_l4", _fc_prepare(64, 4, (100, 3000)), _fc_run, needs=("ws_bytes", "small_bytes")),
    Case("fc_layered_f64_l5", _fc_prepare(64, 5, (100, 3000)), _fc_run),
    Case("fc_layered_f256_l2", _fc_prepare(256, 2, (100, 3000)), _fc_run),
    # tests/test_gpu_head_embed.py: ws partials
    Case("head_bwd", _HEAD, _head_run),
    Case("embed_bwd", _HEAD, _embed_run),
    Case("head_bwd_generic", _HEAD, _head_run, env={"NG_HEAD_PATH": "generic"}),
    Case("embed_bwd_generic", _HEAD, _embed_run, env={"NG_HEAD_PATH": "generic"}),
    # tests/test_gpu_restraint.py (three replicas), tests/test_gpu_finetune.py (clip norm): ws partials
    Case("restraint_r3", _RESTRAINT, _restraint_run),
    # tests/test_gpu_restraint_forms.py (independent replicas, flat bottom)
    Case("restraint_independent_r3", _RESTRAINT, _restraint_ex_run),
    # tests/test_gpu_metrics.py, test_gpu_class_moments.py, test_gpu_reweight_kernels.py: ws partials
    Case("name_metrics", _MOMENTS, _name_metrics_run),
    Case("class_moments", _MOMENTS, _class_moments_run),
    Case("reweight_eval", _reweight_prepare((200, 40000)), _reweight_run),
    # tests/test_gpu_edge_table_kernels.py (T = 4096 points, E = 3): range reduction in aux, scatter partials in ws
    Case("edge_table_range_scatter", _table_prepare((5000, 300000)), _table_run, needs=("ws_bytes", "aux_bytes")),
    # tests/test_gpu_records.py (label moments over a record store), tests/test_gpu_box_grad.py (open frames of 100 atoms),
    # tests/test_gpu_knn_cells.py (NG_KNN=cells: the cell grid at every frame size)
    Case("label_moments", _labels_prepare((8, 2000)), _labels_run),
    Case("box_grad_open", _box_prepare((5, 1000)), _box_run),
    Case("knn_cells", _knn_prepare((300, 20000)), _knn_run, env={"NG_KNN": "cells"}),
    # tests/test_gpu_frame_fused.py: the molecule-sized MPLayer in one launch, its weight image in aux
    Case("mp_short_f256", _mp_short_prepare((1, 3), (150, 1357)), _mp_short_run, needs=("aux_bytes",)),
    Case("grad_clip_norm", _clip_prepare((5000, 3000000)), _clip_run),
    # tests/test_gpu_live_edges.py, test_gpu_csr.py, test_gpu_graph_lists_exact.py: aux
    Case("build_live_edges", _LISTS, _live_run, needs=("aux_bytes",)),
    Case("exclusive_scan", _LISTS, _scan_run, needs=("aux_bytes",)),
    Case("build_incoming_lists", _LISTS, _incoming_run, needs=("aux_bytes",)),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
# cases that really use no context scratch at the small shape: scenario A asserts allocs == 0 for them, B-D still run them
NO_SCRATCH_SMALL = set()

_INPUTS, _WARM = {}, {}


def inputs(case, dev, big):
    key = (case.name, big)
    if key not in _INPUTS:
        _INPUTS[key] = case.prepare(dev, big)
    return _INPUTS[key]


def warm(case, dev, big):
    """the warm bits of (case, shape): computed once, shared by every scenario"""
    key = (case.name, big)
    if key not in _WARM:
        s = inputs(case, dev, big)
        with switches(case.env):
            _WARM[key], _ = warm_reference(lambda ctx: case.run(ctx, dev, s), dev, case.span)
    return _WARM[key]


def cold_run(ctx, case, dev, big):
    """one run of the case on `ctx` in the explicit state -> (host arrays, scratch_info before, scratch_info after)"""
    import torch
    s = inputs(case, dev, big)
    set_state(ctx, dev, case.span)
    before = ctx.scratch_info()
    with switches(case.env):
        out = case.run(ctx, dev, s)
    after = ctx.scratch_info()
    torch.cuda.synchronize(dev)
    return to_host(out), before, after


# ------------------------------------------------------------------------------------------------------------------ A, B
@pytest.mark.parametrize("name", NAMES)
def test_first_call_and_steady_state(gpu_device, name):
    """A: the first call on a fresh context gives the warm bits and really allocated.  B: the same call again gives them too and
    allocates and synchronises nothing (include/nmrgnn_hip.h: "allocates nothing once its scratch is sized")."""
    case, dev = BY_NAME[name], gpu_device
    ref = warm(case, dev, False)
    with cold_context(0) as ctx:
        got, b0, a0 = cold_run(ctx, case, dev, False)
        assert b0["allocs"] == 0 and b0["ws_bytes"] == b0["aux_bytes"] == b0["small_bytes"] == 0, b0
        if name in NO_SCRATCH_SMALL:
            assert a0["allocs"] == 0, a0
        else:
            assert a0["allocs"] > 0, f"{name} is listed as a scratch user but allocated nothing: {a0}"
            unborn = [k for k in case.needs if a0[k] == 0]
            assert not unborn, f"{name}: the first call did not give birth to {unborn}: {a0}"
            assert a0["small_bytes"] in (0, NG_SMALL_BYTES)
        assert_same(got, ref, f"{name}: first call on a cold context")
        got2, b1, a1 = cold_run(ctx, case, dev, False)
        assert_same(got2, ref, f"{name}: second call")
        if name in STEADY_STATE_EXCEPTIONS:
            assert a1["ws_bytes"] == b1["ws_bytes"] and a1["aux_bytes"] == b1["aux_bytes"], (name, b1, a1)
        else:
            assert (a1["allocs"], a1["syncs"]) == (b1["allocs"], b1["syncs"]), f"{name}: steady state allocates: {b1} -> {a1}"
            assert a1 == b1 or {k for k in a1 if a1[k] != b1[k]} <= {"jobs", "early_runs"}, (b1, a1)


# ------------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("name", NAMES)
def test_grow_in_place(gpu_device, name):
    """C: small, big, small on one fresh context: the big call grows a workspace that already exists (synchronise, free,
    allocate) — asserted — and all three results carry the warm bits."""
    case, dev = BY_NAME[name], gpu_device
    ref_s, ref_b = warm(case, dev, False), warm(case, dev, True)
    with cold_context(0) as ctx:
        g1, _, a1 = cold_run(ctx, case, dev, False)
        g2, _, a2 = cold_run(ctx, case, dev, True)
        g3, b3, a3 = cold_run(ctx, case, dev, False)
        grew = [k for k in ("ws_bytes", "aux_bytes") if a2[k] > a1[k] > 0]
        assert grew, f"{name}: the big shape grew no existing workspace: {a1} -> {a2}"
        assert a2["syncs"] > a1["syncs"] and a2["allocs"] > a1["allocs"]
        assert_same(g1, ref_s, f"{name}: small, first")
        assert_same(g2, ref_b, f"{name}: big, after growing {grew}")
        assert_same(g3, ref_s, f"{name}: small again")
        assert (a3["allocs"], a3["syncs"]) == (b3["allocs"], b3["syncs"]), "the small shape allocates in scratch sized for the big one"


# ------------------------------------------------------------------------------------------------------------------ D
def test_grow_under_load(gpu_device):
    """D: every (case, shape) on ONE fresh context and one stream, in ascending order of main-workspace need, with no host
    synchronisation in between: a call grows a block while the kernels of the call before it may still be running.  Then the
    same calls in descending order.  Every result carries the warm bits.

    Order and expectation come from each call's need measured alone on a context of its own (cap_i: ws_bytes after it = 1.5 x
    its largest growing request, capi.hip: workspace()).  On the shared ladder the running size never exceeds 1.5 x the largest
    cap so far, and call i asks for at least cap_i / 1.5: a call whose cap exceeds 2.25 x every earlier cap MUST grow the block.
    Those calls are the rungs; allocs must rise at every rung on the way up (at least 4 rungs, 10 calls), and not at all on the
    way down."""
    import torch
    dev = gpu_device
    calls = [(c, big) for c in CASES for big in (False, True)]
    caps = {}
    for c, big in calls:
        warm(c, dev, big)
        with cold_context(0) as ctx:
            _, _, a = cold_run(ctx, c, dev, big)
            caps[(c.name, big)] = a["ws_bytes"]
    order = sorted(calls, key=lambda cb: caps[(cb[0].name, cb[1])])
    rungs, top = set(), 0
    for c, big in order:
        cap = caps[(c.name, big)]
        if cap > 2.25 * top:
            rungs.add((c.name, big))
        top = max(top, cap)
    assert len(order) >= 10 and len(rungs) >= 4, (len(order), sorted(rungs))
    with cold_context(0) as ctx:
        set_state(ctx, dev, 0)
        outs, rose = [], {}
        for c, big in order:
            s = inputs(c, dev, big)
            ctx.check(ctx.lib.ng_ctx_set_graph_span(ctx.handle, c.span), "span")
            n0 = ctx.scratch_info()
            with switches(c.env):
                outs.append(c.run(ctx, dev, s))
            n1 = ctx.scratch_info()
            rose[(c.name, big)] = n1["ws_bytes"] > n0["ws_bytes"] and n1["allocs"] > n0["allocs"]
        top_info = ctx.scratch_info()
        for c, big in order[::-1]:
            s = inputs(c, dev, big)
            ctx.check(ctx.lib.ng_ctx_set_graph_span(ctx.handle, c.span), "span")
            with switches(c.env):
                outs.append(c.run(ctx, dev, s))
        down_info = ctx.scratch_info()
        torch.cuda.synchronize(dev)
        missing = [r for r in sorted(rungs) if not rose[r]]
        assert not missing, f"no growth of the main workspace at {missing}; caps {caps}"
        assert (down_info["allocs"], down_info["syncs"]) == (top_info["allocs"], top_info["syncs"]), (top_info, down_info)
        for (c, big), out in zip(order + order[::-1], outs):
            assert_same(to_host(out), warm(c, dev, big), f"{c.name} ({'big' if big else 'small'}) under load")


# ------------------------------------------------------------------------------------------------------------------ E
def _bwd_only(ctx, dev, s, dY, dW):
    from nmrgnn_amd._lib import ptr
    M, K, N = s["M"], s["K"], s["N"]
    dX, dB = _nan(dev, M, K), _nan(dev, N)
    ctx.check(ctx.lib.ng_dense_bwd(ctx.handle, stream_ptr(dev), M, K, N, SOFTPLUS, 0, ptr(s["X"]), ptr(s["W"]), ptr(s["S"]), ptr(dY),
                                   ptr(dX), ptr(dW), ptr(dB)), "ng_dense_bwd")
    return dX, dB


def _dense_bwd_inputs(dev, M, K, N, count):
    import torch
    rng = np.random.default_rng([M, K, N, count])
    X, W = rng.standard_normal((M, K)), rng.standard_normal((K, N)) / np.sqrt(K)
    S = np.log1p(np.exp(X @ W))
    s = dict(M=M, K=K, N=N, X=_up(dev, X), W=_up(dev, W), S=_up(dev, S))
    dY0 = _up(dev, rng.standard_normal((M, N)))
    return s, [torch.roll(dY0, k, 0).contiguous() * (1.0 + k) for k in range(count)]      # distinct gradients per call


@pytest.mark.parametrize("reduce", ["wide", "narrow"])
def test_arena_born_inside_a_window(gpu_device, monkeypatch, reduce):
    """E: the deferred-reduction arena does not exist when the window opens.  Generic ng_dense_bwd calls (768 x 256, M = 1024:
    about 25 MiB of partials each by the code, first chunk = 2 x the first request, so the THIRD call should overflow it) until
    a second chunk exists — counted, not assumed.  The flush gives every dW the eager bits and merges the chunks; a second,
    identical window gives the same bits without allocating or synchronising."""
    import torch
    dev = gpu_device
    if reduce == "narrow":
        monkeypatch.setenv("NG_REDUCE", "narrow")
    MAX_CALLS = 8
    s, dYs = _dense_bwd_inputs(dev, 1024, 768, 256, MAX_CALLS)

    def eager(ctx):
        out = {}
        for k, dY in enumerate(dYs):
            dW = _nan(dev, 768, 256)
            dX, dB = _bwd_only(ctx, dev, s, dY, dW)
            out[f"dW{k}"], out[f"dB{k}"], out[f"dX{k}"] = dW, dB, dX
        return out

    ref, _ = warm_reference(eager, dev)
    with cold_context(0) as ctx:
        set_state(ctx, dev, 0)
        st = stream_ptr(dev)

        def window(limit):
            ctx.check(ctx.lib.ng_defer_reductions(ctx.handle, st, 1), "ng_defer_reductions")
            out, n = {}, 0
            try:
                while n < limit:
                    dW = _nan(dev, 768, 256)
                    dX, dB = _bwd_only(ctx, dev, s, dYs[n], dW)
                    out[f"dW{n}"], out[f"dB{n}"], out[f"dX{n}"] = dW, dB, dX
                    n += 1
                    if limit == MAX_CALLS and ctx.scratch_info()["chunks"] >= 2:
                        break
                before_flush = ctx.scratch_info()
                ctx.check(ctx.lib.ng_flush_reductions(ctx.handle, st), "ng_flush_reductions")
            finally:
                ctx.lib.ng_defer_reductions(ctx.handle, st, 0)
            torch.cuda.synchronize(dev)
            return to_host(out), n, before_flush

        got, n_calls, bf = window(MAX_CALLS)
        print(f"ARENA {reduce}: second chunk opened by call {n_calls}; before the flush {bf}")
        assert bf["chunks"] >= 2, f"{MAX_CALLS} calls did not overflow the first arena chunk: {bf}"
        assert bf["jobs"] >= n_calls
        after = ctx.scratch_info()
        assert after["chunks"] == 1 and after["arena_bytes"] == bf["arena_bytes"], after
        want = {k: v for k, v in ref.items() if int(k[2:]) < n_calls}
        assert_same(got, want, "first window (arena born inside it, two chunks)")
        got2, n2, bf2 = window(n_calls)
        end = ctx.scratch_info()
        assert bf2["chunks"] == 1 and end["chunks"] == 1
        assert (end["allocs"], end["syncs"]) == (after["allocs"], after["syncs"]), (after, end)
        assert_same(got2, want, "second window (merged arena)")


# ------------------------------------------------------------------------------------------------------------------ F
def test_reduction_queue_overflow(gpu_device):
    """F: more than RB_MAX_JOBS deferred reductions in one window: the queue is run early when the 25th job arrives, and the
    arena must keep what the early run consumed and what is queued behind it.  30 generic-size dense backwards into 30 distinct
    dW and a 13-layer layered FC block backward; every gradient — queued before and after the overflow — has the eager bits."""
    import torch
    dev = gpu_device
    M, K, N, COUNT = 300, 64, 32, 30
    s, dYs = _dense_bwd_inputs(dev, M, K, N, COUNT)
    fc = _fc_prepare(64, 13, (100, 100))(dev, False)

    def chain(ctx):
        out = {}
        for k, dY in enumerate(dYs):
            dW = _nan(dev, K, N)
            dX, dB = _bwd_only(ctx, dev, s, dY, dW)
            out[f"dW{k}"], out[f"dB{k}"] = dW, dB
        out.update({f"fc_{k}": v for k, v in _fc_run(ctx, dev, fc).items()})
        return out

    ref, _ = warm_reference(chain, dev)
    with cold_context(0) as ctx:
        set_state(ctx, dev, 0)
        st = stream_ptr(dev)
        ctx.check(ctx.lib.ng_defer_reductions(ctx.handle, st, 1), "ng_defer_reductions")
        try:
            out = chain(ctx)
            mid = ctx.scratch_info()
            ctx.check(ctx.lib.ng_flush_reductions(ctx.handle, st), "ng_flush_reductions")
        finally:
            ctx.lib.ng_defer_reductions(ctx.handle, st, 0)
        torch.cuda.synchronize(dev)
        assert mid["jobs"] > RB_MAX_JOBS and mid["early_runs"] >= 1, f"the queue never overflowed: {mid}"
        assert_same(to_host(out), ref, "one window of more than 24 jobs")


# ------------------------------------------------------------------------------------------------------------------ G
def test_reserve_sizes_the_main_workspace_and_the_small_scratch(gpu_device):
    """G: what ng_ctx_reserve guarantees (include/nmrgnn_hip.h): the main workspace holds at least the reserved bytes and the
    small scratch exists; calls whose main-workspace need is below the reservation never touch that block again.  What it does
    not: aux workspace, arena and images are born in the calls — every allocation after the reservation is one of those."""
    dev = gpu_device
    R = 256 * MIB
    names = ["dense_768x256", "mp_f256", "edge_layered_h64", "fc_layered_f64_l5", "build_incoming_lists", "exclusive_scan"]
    for n in names:
        warm(BY_NAME[n], dev, True)
    with cold_context(0) as ctx:
        ctx.check(ctx.lib.ng_ctx_reserve(ctx.handle, R), "ng_ctx_reserve")
        r = ctx.scratch_info()
        assert r["ws_bytes"] >= R and r["small_bytes"] == NG_SMALL_BYTES and r["allocs"] == 2 and r["aux_bytes"] == 0, r
        aux_born = False
        for n in names:
            got, b, a = cold_run(ctx, BY_NAME[n], dev, True)
            assert_same(got, warm(BY_NAME[n], dev, True), f"{n} in reserved scratch")
            assert a["ws_bytes"] == r["ws_bytes"] and a["small_bytes"] == NG_SMALL_BYTES, (n, a)
            others = any(a[k] != b[k] for k in ("aux_bytes", "chunks", "arena_bytes", "image_bytes"))
            assert others or a["allocs"] == b["allocs"], f"{n}: an allocation that is none of aux / arena / images: {b} -> {a}"
            aux_born = aux_born or a["aux_bytes"] > b["aux_bytes"]
        assert aux_born, "no call grew the aux workspace: reserve is not shown to leave it out"
        # a second pass in the scratch the first one sized: nothing at all is allocated (reserve + one warm-up call per shape)
        sized = ctx.scratch_info()
        for n in names:
            got, _, _ = cold_run(ctx, BY_NAME[n], dev, True)
            assert_same(got, warm(BY_NAME[n], dev, True), f"{n}, second pass")
        end = ctx.scratch_info()
        assert all(end[k] == sized[k] for k in ("allocs", "syncs", "ws_bytes", "aux_bytes", "arena_bytes", "image_bytes")), (sized, end)


# ------------------------------------------------------------------------------------------------------------------ H
def _hp(F, H=128, Le=4):
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    return declare_gnn_space(HyperParameters(atom_feature_size=F, edge_feature_size=3, edge_hidden_size=H, mp_layers=4, fc_layers=4,
                                             edge_fc_layers=Le))


def _shared_state(dev):
    """the shared context in the explicit state, for a warm run of engine-level code"""
    from nmrgnn_amd import _lib
    set_state(_lib.get_context(0), dev, 0)


def _batch(dev, b):
    import torch
    from nmrgnn_amd.graph import GraphBatch
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    return gb, torch.from_numpy(b["y"]).to(dev), torch.from_numpy(b["w"]).to(dev)


def _train_steps(dev, F, batches, steps_info=None):
    """a fresh engine (fixed seed) on whatever context is installed: inference + one training step per batch, in order;
    returns every loss, prediction, gradient and the parameters after each step"""
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.train import Trainer
    eng = Engine(_hp(F), 10, device=dev, seed=77)
    tr = Trainer(eng, lr=1e-3)
    out = {}
    for k, b in enumerate(batches):
        gb, y, w = _batch(dev, b)
        out[f"peaks{k}"] = eng.forward(gb).clone()
        out[f"loss{k}"] = tr.step(gb, y, w).clone()
        out[f"grad{k}"] = eng.params.grad.clone()
        out[f"flat{k}"] = eng.params.flat.clone()
        if steps_info is not None:
            torch.cuda.synchronize(dev)
            steps_info.append(_lib.get_context(0).scratch_info())
    torch.cuda.synchronize(dev)
    return to_host(out)


@pytest.mark.parametrize("F", [64, 256])
def test_training_step_on_a_cold_context(gpu_device, F):
    """H.1: forward, backward inside a deferral window and the Adam step with refreshed images (Trainer) on a cold context:
    loss, every gradient and the parameters are the warm bits; a second step of the same shape allocates nothing."""
    from helpers import small_batch
    dev = gpu_device
    b = small_batch(4, 61)
    _shared_state(dev)
    ref = _train_steps(dev, F, [b, b])
    with cold_context(0) as ctx:
        info = []
        got = _train_steps(dev, F, [b, b], info)
        assert info[0]["allocs"] > 0 and info[0]["ws_bytes"] > 0 and info[0]["image_bytes"] > 0 and info[0]["chunks"] == 1, info[0]
        assert_same(got, ref, f"F = {F}: two training steps")
        same = {k: (info[0][k], info[1][k]) for k in ("allocs", "ws_bytes", "aux_bytes", "arena_bytes", "image_bytes")}
        assert all(a == b for a, b in same.values()), f"the second step allocates: {same}"


@pytest.mark.parametrize("order", ["small-large-small", "large-small-large"])
@pytest.mark.parametrize("F", [64, 256])
def test_shape_order_on_a_cold_context(gpu_device, F, order):
    """H.2: inference and training on batches of 4 x 61 and 40 x 256 atoms in both orders on one cold context: every block of
    scratch grows (or not) between steps of one engine; bits equal the warm context's."""
    from helpers import small_batch
    from nmrgnn_amd import synth
    dev = gpu_device
    small, large = small_batch(4, 61), synth.make_batch(40, 256, 16, 10, 0.05, seed=9)
    seq = [small, large, small] if order == "small-large-small" else [large, small, large]
    _shared_state(dev)
    ref = _train_steps(dev, F, seq)
    with cold_context(0):
        info = []
        got = _train_steps(dev, F, seq, info)
        if order == "small-large-small":
            assert info[1]["ws_bytes"] > info[0]["ws_bytes"] > 0, info
        else:
            assert info[1]["ws_bytes"] == info[0]["ws_bytes"] > 0, info
        assert_same(got, ref, f"F = {F}, {order}")


@pytest.mark.parametrize("F", [64, 256])
def test_frozen_inference_on_a_cold_context(gpu_device, F):
    """H.3: frozen-weight inference: the image cache's buffers are born inside the first call; the second allocates nothing;
    bits equal those of the engine that keeps no images."""
    import torch
    from helpers import small_batch
    from nmrgnn_amd.engine import Engine
    dev = gpu_device
    b = small_batch(4, 61)
    _shared_state(dev)
    plain = Engine(_hp(F), 10, device=dev, seed=31)
    gb, _, _ = _batch(dev, b)
    ref = to_host({"peaks": plain.forward(gb).clone()})
    with cold_context(0) as ctx:
        eng = Engine(_hp(F), 10, device=dev, seed=31)
        gb, _, _ = _batch(dev, b)
        eng.freeze_weights(True)
        p1 = eng.forward(gb).clone()
        torch.cuda.synchronize(dev)
        i1 = ctx.scratch_info()
        p2 = eng.forward(gb).clone()
        torch.cuda.synchronize(dev)
        i2 = ctx.scratch_info()
        eng.freeze_weights(False)
        assert i1["image_bytes"] > 0 and i1["allocs"] > 0, i1
        assert (i2["allocs"], i2["syncs"], i2["image_bytes"]) == (i1["allocs"], i1["syncs"], i1["image_bytes"]), (i1, i2)
        assert_same(to_host({"peaks": p1}), ref, "frozen, first call")
        assert_same(to_host({"peaks": p2}), ref, "frozen, second call")


def test_edge_table_step_on_a_cold_context(gpu_device):
    """the edge-function table (device-guarded: fused kernels at H = 128) sized at the small batch: its range reduction (aux),
    its scatter partials (ws) and the table's own tensors are born on a cold context; bits equal the warm context's"""
    import torch
    from helpers import small_batch
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.train import Trainer
    dev = gpu_device
    b = small_batch(4, 61)

    def run():
        eng = Engine(_hp(64), 10, device=dev, seed=78)
        eng.edge_table, eng.edge_table_min_edges = True, 1
        tr = Trainer(eng, lr=1e-3)
        gb, y, w = _batch(dev, b)
        out = {"peaks": eng.forward(gb).clone()}
        out["peaks_train"] = eng.forward(gb, training=True, seed=11).clone()
        assert eng.tape.edge_path == "table", eng.tape.edge_path      # the precondition: the table really ran
        out["loss"] = tr.step(gb, y, w).clone()
        out["grad"], out["flat"] = eng.params.grad.clone(), eng.params.flat.clone()
        torch.cuda.synchronize(dev)
        return to_host(out)

    _shared_state(dev)
    ref = run()
    with cold_context(0) as ctx:
        got = run()
        assert ctx.scratch_info()["aux_bytes"] > 0 and ctx.scratch_info()["ws_bytes"] > 0
        assert_same(got, ref, "edge-table training step")


def _graphs(n, atoms=256, K=16):
    from nmrgnn_amd import synth
    out = []
    for g in range(n):
        b = synth.make_batch(1, atoms, K, 10, 0.05, seed=500 + g)
        out.append(((b["atoms"], b["nlist"], b["edges"], b["inv_degree"]), b["graph_ptr"], b["y"], b["w"]))
    return out


def _train_replay_case(dev, hp, table_on_replayed, eager_table, n_atoms=256):
    """tests/test_gpu_replay.py's trajectory test on a cold context: engine `eb` steps through a TrainStepReplay built there,
    engine `ea` steps eagerly; returns (the replay object, scratch_info after the construction)"""
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.graph import GraphBatch
    from nmrgnn_amd.replay import TrainStepReplay
    from nmrgnn_amd.train import Trainer
    gs = _graphs(4, atoms=n_atoms)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(device=dev, dtype=torch.float32)
    ea, eb = Engine(hp, 10, device=dev, seed=77), Engine(hp, 10, device=dev, seed=77)
    ea.edge_table = eager_table
    if table_on_replayed:
        eb.edge_table, eb.edge_table_min_edges = True, 1
    ta, tb = Trainer(ea, lr=1e-3), Trainer(eb, lr=1e-3)
    raw0, gp0, y0, w0 = gs[0]
    rp = TrainStepReplay(tb, raw0, y0, w0, graph_ptr=gp0)
    info = _lib.get_context(0).scratch_info()
    assert torch.equal(ea.params.flat, eb.params.flat) and eb.adam_t == 0
    for step in range(5):
        raw, gp, y, w = gs[step % len(gs)]
        la = ta.step(GraphBatch(*raw, graph_ptr=gp, device=dev), t(y), t(w))
        lb = rp.step(raw, y, w)
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (step, la, lb)
        assert torch.equal(ea.params.flat, eb.params.flat), step
    return rp, info


@pytest.mark.parametrize("F", [64, 256])
def test_train_step_replay_built_on_a_cold_context(gpu_device, F):
    """H.4: the warm-up steps of TrainStepReplay size everything the captured step needs: no allocation between the end of the
    warm-up and the end of the capture, and the replayed trajectory is the eager one (as tests/test_gpu_replay.py asserts)."""
    with cold_context(0):
        rp, info = _train_replay_case(gpu_device, _hp(F), False, True)
        assert info["allocs"] > 0 and info["ws_bytes"] > 0, info
        assert rp.capture_allocs == 0, f"the capture allocated {rp.capture_allocs} blocks"
        assert rp.warmup_edge_paths == [rp.captured_edge_path] * 2, (rp.warmup_edge_paths, rp.captured_edge_path)


def _frames():
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(os.path.join(os.path.dirname(__file__), "data", "108M.pdb"))
    atoms = atoms_onehot(s.elements)
    rng = np.random.default_rng(3)
    return atoms, [s.frames[0] + rng.normal(0, 0.2, s.frames[0].shape).astype(np.float32) for _ in range(3)]


def test_forward_replay_built_on_a_cold_context(gpu_device):
    """H.4: ForwardReplay with the shapes of tests/test_gpu_replay.py, built on a cold context"""
    import torch
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    from nmrgnn_amd.replay import ForwardReplay
    dev = gpu_device
    atoms, frames = _frames()
    with cold_context(0) as ctx:
        eng = Engine(declare_gnn_space(HyperParameters()), atoms.shape[1], device=dev, seed=5)
        eng.freeze_weights(True)
        rp = ForwardReplay(eng, atoms, frames[0])
        assert ctx.scratch_info()["allocs"] > 0
        assert rp.capture_allocs == 0, f"the capture allocated {rp.capture_allocs} blocks"
        at = torch.from_numpy(atoms).to(dev)
        for f in frames[::-1]:
            ref = eng.forward(frames_to_batch(at, torch.from_numpy(f).to(dev)[None], 16, device=dev)).clone()
            got = rp(f)
            torch.cuda.synchronize()
            assert torch.equal(ref, got)


# ------------------------------------------------------------------------------------------- the warm-up runs the captured chain
WARMUP_ATOMS = 1024      # 16384 edge slots: more than the 2T = 8192 rows of the edge-function table (Engine.EDGE_TABLE_POINTS)


def _table_engine(dev, n_elem, seed=5):
    from nmrgnn_amd.engine import Engine
    eng = Engine(_hp(64, H=64), n_elem, device=dev, seed=seed)
    assert eng.lib.ng_edge_live_supported(eng.H, eng.E, eng.Le, eng.fc_act) == 0
    eng.edge_table, eng.edge_table_min_edges = True, 1
    eng.edge_table_tol = 1.0      # the guard stays down whatever the seeded weights: the eager call really takes the table
    assert WARMUP_ATOMS * 16 > 2 * eng._table_points()
    return eng


def test_forward_replay_warm_up_takes_the_captured_edge_path(gpu_device):
    """An edge shape without the fused kernels (H = 64) with the edge-function table sized at one 1024-atom frame: an eager call
    takes the host-guarded table ("table_host": the layered MLP over the table's 2T = 8192 rows), a captured one cannot read the
    guard on the host and goes per edge ("slots": the layered MLP over all 16384 slots, a larger workspace — both asserted
    first, on a context of their own).  The warm-up of a replay must run the latter, or the capture grows the workspace inside
    a stream capture: the warm-up took "slots", nothing was allocated during the capture, and the replayed peaks are those of
    the per-edge path."""
    import torch
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.replay import ForwardReplay
    dev = gpu_device
    atoms, frames = _frames()
    assert len(atoms) >= WARMUP_ATOMS
    atoms, frames = atoms[:WARMUP_ATOMS], [f[:WARMUP_ATOMS] for f in frames]
    at = torch.from_numpy(atoms).to(dev)
    batch = lambda f: frames_to_batch(at, torch.from_numpy(f).to(dev)[None], 16, device=dev)
    with cold_context(0) as ctx:      # the precondition: a plain eager call takes the table and sizes LESS than the per-edge call
        eng = _table_engine(dev, atoms.shape[1])
        eng.forward(batch(frames[0]))
        torch.cuda.synchronize()
        assert eng.last_edge_path == "table_host", eng.last_edge_path
        ws_table = ctx.scratch_info()["ws_bytes"]
        eng.edge_table = False
        eng.forward(batch(frames[0]))
        torch.cuda.synchronize()
        assert eng.last_edge_path == "slots"
        assert ctx.scratch_info()["ws_bytes"] > ws_table > 0, (ws_table, ctx.scratch_info())
    with cold_context(0) as ctx:
        eng = _table_engine(dev, atoms.shape[1])
        rp = ForwardReplay(eng, atoms, frames[0])
        assert ctx.scratch_info()["allocs"] > 0
        assert rp.captured_edge_path == "slots" and rp.warmup_edge_paths == ["slots", "slots"], (rp.warmup_edge_paths, rp.captured_edge_path)
        assert rp.capture_allocs == 0, f"the capture allocated {rp.capture_allocs} blocks: the warm-up ran another chain"
        got = [rp(f).clone() for f in frames]
        eng.edge_table = False
        for f, g in zip(frames, got):
            ref = eng.forward(batch(f))
            torch.cuda.synchronize()
            assert torch.equal(ref, g)


def test_train_step_replay_warm_up_takes_the_captured_edge_path(gpu_device):
    """the same architecture through TrainStepReplay on 1024-atom graphs: the warm-up steps took "slots", nothing was allocated
    during the capture, and the replayed trajectory is the eager one of an engine that goes per edge (edge_table = False)"""
    with cold_context(0):
        rp, info = _train_replay_case(gpu_device, _hp(64, H=64), True, False, n_atoms=WARMUP_ATOMS)
        assert info["allocs"] > 0
        assert rp.eng.edge_table and rp.eng.edge_table_min_edges == 1 and WARMUP_ATOMS * 16 > 2 * rp.eng._table_points()
        assert rp.captured_edge_path == "slots" and rp.warmup_edge_paths == ["slots", "slots"], (rp.warmup_edge_paths, rp.captured_edge_path)
        assert rp.capture_allocs == 0, f"the capture allocated {rp.capture_allocs} blocks: the warm-up ran another chain"
