"""Every packed weight image the context keeps (ng_ctx::wimg, csrc/repack.hip image_slot) through its life, at the C ABI: after
each step the consumer's outputs must be, bit for bit, those of the same call with the cache off (ng_weights_frozen(ctx, 0):
the image is packed in front of the use) on the weights as they are now.  "The images are the same bits whichever launch
builds them", so no tolerance is involved.  Every output is filled with NaN before the call and compared as bit patterns, and
no element of an output may still hold the prefill (de of the MPLayer: the live slots).

Cases (tests/weight_cache_cases.py: CASES; one row per `image_slot(` call of csrc/, "#n" = the n-th call of the file):

  site                    kind(s)      PackKind                  entry point                      reached by               cases
  mp_win.hip#0            7            PK_MPW_FWD   (flag pair)  ng_mp_layer_fwd, F = 64          default                  win_e3_k16, win_e1_k8, win_w8_e3_k16
  mp_win.hip#0            4            PK_MPW_F32                ng_mp_layer_fwd, F = 64          NG_GEMM_MATH=fp32        win_fp32_e3_k16
  mp_win_bwd.hip#0        8            PK_MPW_BWD   (flag pair)  ng_mp_layer_bwd, F = 64          default                  win_*
  mp_win_bwd.hip#0        14           none (mpw_pack2, no job)  ng_mp_layer_bwd, F = 64          NG_GEMM_MATH=fp32        win_fp32_e3_k16
  fc_fused.hip#0          5            PK_FC        (flag pair)  ng_fc_block_fwd / _bwd, F = 64   default; L sources       fc_l4, fc_l2
  edge_fwd_h2.hip#0       6            PK_EDGE_H2                ng_edge_mlp_fwd, H = 128         default; W0..W3          edge_h2_e3, edge_h2_e1
  edge_bwd_h2.hip#0       13           PK_EDGE_WT + 3 row sums   ng_edge_mlp_bwd_tape             default; W1, W2, W3      edge_h2_*
  edge_fused.hip#0        11           PK_EDGE_F32               ng_edge_mlp_fwd                  NG_EDGE_MATH=fp32; W0..W2 edge_fp32_e3
  edge_fused_bwd.hip#0    12           PK_EDGE_F32 (transposed)  ng_edge_mlp_bwd_tape             NG_EDGE_MATH=fp32        edge_fp32_e3
  frame_fused.hip#0       9            none (ff_pack_kernel)     ng_fc_head_fwd, F = 256          ng_fc_head_ok; 4 images  fc_head
  frame_fused.hip#1       10           none (ff_pack_mp_kernel)  ng_mp_layer_fwd_short, F = 256   ng_mp_layer_short_ok     mp_short_e3, mp_short_e1
  node_ops.hip#0          1            PK_MP_PLAIN               ng_mp_layer_fwd / _bwd           F = 256 and 128          mp_plain_256, mp_plain_128
  gemm_h2.hip#1           3+16t+32nbw  PK_GX from w (prepack)    the same calls                   nbw 4 (F 256) / 2 (F 128, N >= 4096), t = 0 / 1
  gemm_h2.hip#0           3+16t+32nbw  PK_GX                     ng_dense_fwd / _bwd, and above   M 256 | 4096: dense_256, dense_4096 (dense_255,
                                                                                                  dense_4095: below gemm_h2_fwd_ok, no image kept)
  mp_gg.hip#0             15 / 16      PK_GG                     ng_mp_layer_fwd / _bwd, F = 256  NG_MP_GG=1, NG_MP_GG_MIN_ROWS=256   mp_gg

Weights are views into ONE flat float32 tensor at 16-byte-aligned offsets, as Engine lays them out, with a block of 64 other
parameters in front and behind, and flat g, m, v beside it: ng_adam_step(p + off, n) over a part of it is what a trainer with
parameter groups does.

Life cycle per case (weight_cache_cases.steps_of):
  1  frozen under a fresh owner: first call (packs), second call (served from the image).  The profile scopes of the first call
     are those the row names
  2  new values written into the same tensors, ng_weights_changed
  3  ng_adam_step over the whole flat buffer at a rate that moves every weight by about 1e-2: the cache-off outputs before and
     after differ; exactly one repack_all record where the kind keeps a PackJob, none where it does not (kinds 9, 10, 14: the
     image is rebuilt at its next use; the dense cases below the row threshold keep nothing)
  4  more than one source: ng_adam_step over a block holding only the first source — the image must not be rebuilt from the
     half-updated set and served as current: no repack_all record — the call, then the step over the rest (a record only
     where an image has all its sources there: kind 13), the call
  5  ng_adam_step over a block holding none of the sources: the version moves, the weights do not; no repack_all record
  6  flag pairs (kinds 7, 8, 5): one weight at 255.88 (2^8 w >= 65504: out), announced; one Adam step with a positive gradient
     at rate 1e-2 brings it to about 255.87, inside: the rebuilt image must lower its flag; then 400.0 and back through
     ng_weights_changed
  7  the tensors overwritten in place WITHOUT an announcement, then another owner: its first call inherits nothing; back to the
     first owner
  8  cache off again
Steps 4 and 6 run where the kind has a second source / a flag; every other step runs for every case."""
import ctypes as C
import itertools
import zlib

import numpy as np
import pytest
import torch

import weight_cache_cases as wc
from mp_layer_gpu import GpuLayer

pytestmark = pytest.mark.gpu
_owner = itertools.count(7310001, 2)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    assert len(a) == len(b)
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _parr(ts):
    from nmrgnn_amd._lib import ptr_array
    return ptr_array(ts)


# ---------------------------------------------------------------------------------------------------------- consumers
class Mp:
    """ng_mp_layer_fwd + ng_mp_layer_bwd on a padded list (local neighbours, a tenth of the slots dead)"""

    def __init__(self, ctx, dev, case, rng):
        s = case["shape"]
        N, K, E, F = s["N"], s["K"], s["E"], s["F"]
        nl = np.clip(np.arange(N)[:, None] + rng.integers(-20, 21, (N, K)), 0, N - 1).astype(np.int32)
        live = rng.random((N, K)) >= 0.1
        live[:, 0] = True
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        c = dict(kind="padded", F=F, E=E, K=K, N=N, span=0, act=s["act"], residual=1, nl=nl, live=live,
                 e=f32(rng.standard_normal((N, K, E)) * live[:, :, None]), h=f32(rng.standard_normal((N, F)) * 0.5),
                 inv=f32(1.0 / np.maximum(live.sum(1), 1)), w=np.zeros((F, F, E), np.float32))
        self.g = GpuLayer(c, dev)
        self.dH = self.g.t(f32(rng.standard_normal((N, F))))
        self.keep_A = bool(ctx.lib.ng_mp_layer_wants_aggregate(F, E, K))
        self.live = torch.from_numpy(live.reshape(-1)).to(dev)      # de of a dead slot is not an output

    def __call__(self, W):
        h_out, A, s = self.g.fwd(keep_A=self.keep_A, w=W["w"])
        dh, de, dw = self.g.bwd(A, s, self.dH, w=W["w"])
        return [h_out, s, dh, de[self.live], dw] + ([A] if A is not None else [])


class MpShort:
    """ng_mp_layer_fwd_short: aggregate + update of a layer in one launch (molecule-sized inference)"""

    def __init__(self, ctx, dev, case, rng):
        self.mp = Mp(ctx, dev, case, rng)
        self.ctx, self.dev, self.s = ctx, dev, case["shape"]
        s = self.s
        assert ctx.lib.ng_mp_layer_short_ok(s["N"], s["K"], s["F"], s["E"]) == 1

    def __call__(self, W):
        from nmrgnn_amd._lib import ptr
        s, g = self.s, self.mp.g
        out = _nan(self.dev, s["N"], s["F"])
        self.ctx.check(self.ctx.lib.ng_mp_layer_fwd_short(self.ctx.handle, g.st, s["N"], s["K"], s["F"], s["E"], s["act"], 1, ptr(g.th),
                                                          ptr(g.nlist), ptr(g.te), ptr(g.tinv), ptr(W["w"]), ptr(out)), "short")
        return [out]


class Fc:
    """ng_fc_block_fwd + ng_fc_block_bwd"""

    def __init__(self, ctx, dev, case, rng):
        self.ctx, self.dev, self.s = ctx, dev, case["shape"]
        s = self.s
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.x = t(rng.standard_normal((s["N"], s["F"])) * 0.5)
        self.dg = t(rng.standard_normal((s["N"], s["F"] // 2)))
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def __call__(self, W):
        from nmrgnn_amd._lib import ptr
        s, lib, h = self.s, self.ctx.lib, self.ctx.handle
        N, F, L = s["N"], s["F"], s["L"]
        Ws, Bs = [W[f"W{t}"] for t in range(L)], [W[f"b{t}"] for t in range(L)]
        ys = [_nan(self.dev, N, F) for _ in range(L - 1)]
        g = _nan(self.dev, N, F // 2)
        self.ctx.check(lib.ng_fc_block_fwd(h, self.st, N, F, L, s["act"], ptr(self.x), _parr(Ws), _parr(Bs), _parr(ys), ptr(g)), "fc fwd")
        dx = _nan(self.dev, N, F)
        dW, dB = [torch.full_like(w, float("nan")) for w in Ws], [torch.full_like(b, float("nan")) for b in Bs]
        ns = int(lib.ng_fc_block_scratch_floats(N, F, L))
        scratch = torch.empty(max(ns, 1), device=self.dev)
        self.ctx.check(lib.ng_fc_block_bwd(h, self.st, N, F, L, s["act"], _parr([self.x] + ys), ptr(g), _parr(Ws), ptr(self.dg), ptr(dx),
                                           _parr(dW), _parr(dB), ptr(scratch)), "fc bwd")
        return ys + [g, dx] + dW + dB


class FcHead:
    """ng_fc_head_fwd: FC block + head in one launch (molecule-sized inference)"""

    def __init__(self, ctx, dev, case, rng):
        self.ctx, self.dev, self.s = ctx, dev, case["shape"]
        s = self.s
        assert ctx.lib.ng_fc_head_ok(s["N"], s["F"], s["L"], s["C"], s["act"]) == 1
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.x = t(rng.standard_normal((s["N"], s["F"])) * 0.5)
        self.atoms = t(np.eye(s["C"])[np.arange(s["N"]) % s["C"]])
        self.std, self.avg = t(1.0 + rng.random(s["C"])), t(rng.standard_normal(s["C"]))
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def __call__(self, W):
        from nmrgnn_amd._lib import ptr
        s = self.s
        L = s["L"]
        peaks = _nan(self.dev, s["N"])
        self.ctx.check(self.ctx.lib.ng_fc_head_fwd(self.ctx.handle, self.st, s["N"], s["F"], L, s["C"], s["act"], ptr(self.x),
                                                   _parr([W[f"W{t}"] for t in range(L)]), _parr([W[f"b{t}"] for t in range(L)]),
                                                   ptr(W["Wout"]), ptr(W["bout"]), ptr(self.atoms), ptr(self.std), ptr(self.avg),
                                                   ptr(peaks)), "fc head")
        return [peaks]


class Edge:
    """ng_edge_mlp_fwd with its tape + ng_edge_mlp_bwd_tape"""

    def __init__(self, ctx, dev, case, rng):
        from nmrgnn_amd.engine import rbf_grid
        self.ctx, self.dev, self.s = ctx, dev, case["shape"]
        s = self.s
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.d = t(0.1 + 0.5 * rng.random(s["n"]))
        c, self.gap = rbf_grid(0.0, 0.8, s["H"])
        self.centers = t(c)
        self.de = t(rng.standard_normal((s["n"], s["E"])))
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def __call__(self, W):
        from nmrgnn_amd._lib import ptr
        s, lib, h = self.s, self.ctx.lib, self.ctx.handle
        n, H, E, Le = s["n"], s["H"], s["E"], s["Le"]
        Ws, Bs = [W[f"W{t}"] for t in range(Le)], [W[f"b{t}"] for t in range(Le)]
        e, z = _nan(self.dev, n, E), _nan(self.dev, Le - 1, n, H)
        layout = int(lib.ng_edge_tape_layout(H, E, Le, s["act"], n))
        self.ctx.check(lib.ng_edge_mlp_fwd(h, self.st, n, H, E, Le, s["act"], ptr(self.d), ptr(self.d), ptr(self.centers), self.gap,
                                           _parr(Ws), _parr(Bs), ptr(e), ptr(z)), "edge fwd")
        dW, dB = [torch.full_like(w, float("nan")) for w in Ws], [torch.full_like(b, float("nan")) for b in Bs]
        self.ctx.check(lib.ng_edge_mlp_bwd_tape(h, self.st, n, H, E, Le, s["act"], ptr(self.d), ptr(self.d), ptr(self.centers), self.gap,
                                                _parr(Ws), ptr(z), ptr(self.de), _parr(dW), _parr(dB), layout), "edge bwd")
        return [e, z] + dW + dB


class Dense:
    """ng_dense_fwd + ng_dense_bwd"""

    def __init__(self, ctx, dev, case, rng):
        self.ctx, self.dev, self.s = ctx, dev, case["shape"]
        s = self.s
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.x = t(rng.standard_normal((s["M"], s["Kin"])) * 0.5)
        self.dy = t(rng.standard_normal((s["M"], s["Nout"])))
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def __call__(self, W):
        from nmrgnn_amd._lib import ptr
        s, lib, h = self.s, self.ctx.lib, self.ctx.handle
        M, Kin, Nout = s["M"], s["Kin"], s["Nout"]
        y, sv = _nan(self.dev, M, Nout), _nan(self.dev, M, Nout)
        self.ctx.check(lib.ng_dense_fwd(h, self.st, M, Kin, Nout, s["act"], 0, ptr(self.x), ptr(W["W"]), ptr(W["b"]), ptr(y), ptr(sv)),
                       "dense fwd")
        dx, dw, db = _nan(self.dev, M, Kin), _nan(self.dev, Kin, Nout), _nan(self.dev, Nout)
        self.ctx.check(lib.ng_dense_bwd(h, self.st, M, Kin, Nout, s["act"], 0, ptr(self.x), ptr(W["W"]), ptr(sv), ptr(self.dy), ptr(dx),
                                        ptr(dw), ptr(db)), "dense bwd")
        return [y, sv, dx, dw, db]


CALLS = {"mp": Mp, "mp_short": MpShort, "fc": Fc, "fc_head": FcHead, "edge": Edge, "dense": Dense}


# ---------------------------------------------------------------------------------------------------------- life cycle
@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_weight_image_life_cycle(gpu_device, monkeypatch, name):
    from nmrgnn_amd import _lib
    case = wc.CASES[wc.CASE_NAMES.index(name)]
    dev = gpu_device
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    ctx = _lib.get_context(0)
    lib, h = ctx.lib, ctx.handle
    ok = lambda rc, what: ctx.check(rc, what)
    ok(lib.ng_ctx_set_graph_span(h, 0), "span")
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    total, table = wc.layout(case)
    blocks = wc.blocks(case)
    steps = wc.steps_of(case)
    flat, grad, m, v = (torch.zeros(total, device=dev) for _ in range(4))
    W = {n: flat[off:off + int(np.prod(shape))].view(shape) for n, (off, shape) in table.items()}
    assert all(t.data_ptr() % 16 == 0 for t in W.values())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def values():
        out = np.zeros(total, np.float32)
        for n, (off, shape) in table.items():
            k = int(np.prod(shape))
            out[off:off + k] = rng.standard_normal(k) * (0.1 if len(shape) > 1 else 0.05)
        return torch.from_numpy(out).to(dev)

    def adam(block, sign=None):
        """one first Adam step (m = v = 0) over `block` at rate 1e-2: every weight in it moves by about 1e-2 against its gradient"""
        off, n = block
        gr = rng.standard_normal(total).astype(np.float32)
        gr = np.where(np.abs(gr) < 0.1, 0.1, gr) if sign is None else np.full(total, sign, np.float32)
        grad.copy_(torch.from_numpy(gr).to(dev))
        m.zero_()
        v.zero_()
        p = lambda t: C.c_void_p(t.data_ptr() + 4 * off)
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            ok(lib.ng_adam_step(h, st, n, p(flat), p(grad), p(m), p(v), 1e-2, 0.9, 0.999, 1e-7, 1, 1.0), "ng_adam_step")
            torch.cuda.synchronize()
            recs = ctx.prof_read()
        finally:
            ctx.prof_enable(False)
        assert recs.get("adam", (0.0, 0))[1] == 1, recs
        return recs.get("repack_all", (0.0, 0))[1]

    call = CALLS[case["call"]](ctx, dev, case, rng)
    owner = [next(_owner), next(_owner)]
    cur = [owner[0]]

    def run():
        out = call(W)
        torch.cuda.synchronize()
        return out

    def ref():
        ok(lib.ng_weights_frozen(h, 0), "thaw")
        try:
            return run()
        finally:
            ok(lib.ng_weights_frozen(h, cur[0]), "freeze")

    def hold(step, what=""):
        """the cached call against the cache-off call on the weights as they are now; returns the latter"""
        got = run()
        want = ref()
        assert _same(got, want), f"{name}: step {step} {what}: the cached call is not the cache-off call"
        for k, t in enumerate(want):       # (bit patterns compare equal where both runs left the NaN prefill: nothing may)
            assert bool(torch.isfinite(t).all()), f"{name}: step {step} {what}: output {k} holds a value nobody wrote, or none"
        return want

    flat.copy_(values())
    try:
        # ---- 1
        ok(lib.ng_weights_frozen(h, cur[0]), "freeze")
        ctx.prof_enable(True)
        ctx.prof_reset()
        first = run()
        seen = set(ctx.prof_read())
        ctx.prof_enable(False)
        assert case["names"] <= seen and not (case["absent"] & seen), (name, sorted(seen))
        second = run()
        r1 = ref()
        assert _same(first, r1), f"{name}: step 1: the first frozen call is not the cache-off call"
        assert _same(second, r1), f"{name}: step 1: the call served from the image is not the cache-off call"
        # ---- 2
        flat.copy_(values())
        ok(lib.ng_weights_changed(h), "ng_weights_changed")
        r2 = hold(2)
        assert not _same(r2, r1)
        # ---- 3
        assert adam(blocks["all"]) == (1 if case["registered"] else 0), f"{name}: step 3: repack_all records"
        r3 = hold(3)
        assert not _same(r3, r2), f"{name}: step 3 moved no output: it proved nothing"
        last = r3
        # ---- 4
        if 4 in steps:
            assert adam(blocks["some"]) == 0, f"{name}: step 4: an image was rebuilt from a half-updated set of sources"
            r4 = hold(4, "(some of the sources updated)")
            assert not _same(r4, last)
            assert adam(blocks["rest"]) == case.get("rest_repacks", 0), f"{name}: step 4: repack_all records of the second call"
            last = hold(4, "(the rest updated)")
            assert not _same(last, r4)
        # ---- 5
        assert adam(blocks["none"]) == 0, f"{name}: step 5: an image was rebuilt although none of its sources moved"
        r5 = hold(5)
        assert _same(r5, last), f"{name}: step 5: a step over none of the sources changed the outputs"
        # ---- 6
        if 6 in steps:
            wname, idx = case["edge"]
            W[wname][idx] = 255.88
            ok(lib.ng_weights_changed(h), "ng_weights_changed")
            assert float(W[wname][idx]) * 256.0 >= 65504.0
            hold(6, "(one weight at 255.88: out of the piece range)")
            hold(6, "(the same, served from the image)")
            assert adam(blocks["all"], sign=1.0) == 1
            back = float(W[wname][idx])
            assert 255.86 < back < 255.875 and back * 256.0 < 65504.0, back
            hold(6, "(Adam brought the weight to 255.87: the rebuilt image must lower its flag)")
            W[wname][idx] = 400.0
            ok(lib.ng_weights_changed(h), "ng_weights_changed")
            hold(6, "(400.0)")
            W[wname][idx] = 0.25
            ok(lib.ng_weights_changed(h), "ng_weights_changed")
            hold(6, "(back at 0.25)")
        # ---- 7
        flat.copy_(values())                      # in place, NOT announced
        cur[0] = owner[1]
        ok(lib.ng_weights_frozen(h, cur[0]), "freeze")
        r7 = hold(7, "(another owner)")
        cur[0] = owner[0]
        ok(lib.ng_weights_frozen(h, cur[0]), "freeze")
        assert _same(hold(7, "(the first owner again)"), r7)
        # ---- 8
        ok(lib.ng_weights_frozen(h, 0), "thaw")
        assert _same(run(), r7), f"{name}: step 8"
    finally:
        lib.ng_weights_frozen(h, 0)
        lib.ng_prof_enable(h, 0)
        lib.ng_ctx_set_graph_span(h, 0)
