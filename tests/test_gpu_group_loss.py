"""The ensemble-averaged loss on the GPU (csrc/group_loss.hip, Engine.loss_groups).

ng_group_mean / ng_group_spread through the C ABI, BIT FOR BIT against the float32 restatement of tests/group_loss_ref.py (the
operation order is fully specified: no tolerance): mean_out, y_out, w_out, names_out and dpred.  The kernels run one thread per
flat mean index in workgroups of 256, so the cases put group sizes at 1, 5, 255, 256 and 257 atoms with 1, 2, 3 and 8 members,
group boundaries inside a workgroup, a smallest last group, member weights with a zero, scale 1 and 0.25, names NULL; every
batch holds fewer than 2,000 atoms.  Every output is pre-filled with NaN (names with -1): a row left unwritten fails.

Engine.loss_groups: singleton groups give the bits of the ungrouped loss, and a 3-group batch agrees with float64."""
import ctypes as C

import numpy as np
import pytest

import group_loss_ref as R

pytestmark = pytest.mark.gpu

WG = 256                                        # GL_THREADS of csrc/group_loss.hip

# (n_q, R_q) per group
CASES = {
    "Q1-n1": [[(1, r)] for r in (1, 2, 3, 8)],
    "Q1-n5": [[(5, r)] for r in (1, 2, 3, 8)],
    "Q1-wg-1": [[(WG - 1, r)] for r in (1, 2, 3)],
    "Q1-wg": [[(WG, r)] for r in (1, 2, 3)],
    "Q1-wg+1": [[(WG + 1, r)] for r in (1, 2, 3)],
    "Q1-R8-n240": [[(240, 8)]],
    # mixed R and n in one batch, boundaries at mean indices 5 and 262 (inside workgroups 0 and 1), the last group the smallest
    "Q3-mixed": [[(5, 2), (WG + 1, 3), (1, 8)], [(WG - 1, 1), (3, 3), (WG, 2), (2, 1)], [(130, 3), (200, 2), (1, 1)]],
    # many one-atom groups: a workgroup's 256 indices touch 256 groups
    "Q300-n1": [[(1, 1 + q % 3) for q in range(300)]],
}


class Gpu:
    def __init__(self, dev):
        import torch
        from nmrgnn_amd import _lib
        self.torch, self.dev = torch, dev
        self.ctx = _lib.get_context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def up(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)

    def nan(self, n):
        return self.torch.full((n,), float("nan"), device=self.dev)

    def err(self):
        return self.lib.ng_last_error(self.h).decode()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(name, got, ref):
    got = got.cpu().numpy()
    assert got.shape == ref.shape, name
    bad = np.flatnonzero(_bits(got) != _bits(ref))
    assert len(bad) == 0, f"{name}: {len(bad)} of {ref.size} entries differ; first at {bad[0]}: got {got[bad[0]]!r} ref {ref[bad[0]]!r}"


@pytest.mark.parametrize("case", list(CASES))
def test_kernels_bit_for_bit(gpu_device, case):
    from nmrgnn_amd._lib import ptr
    g = Gpu(gpu_device)
    for k, groups in enumerate(CASES[case]):
        gp, qp, pred, y, w, names = R.make_case(100 + k, groups)
        pred[0] = np.float32(-0.0)
        N, G, Q = int(gp[-1]), len(gp) - 1, len(qp) - 1
        assert N < 2000
        mp = R.mean_ptr_of(gp, qp)
        M = int(mp[-1])
        tgp, tqp, tmp = g.up(gp, np.int32), g.up(qp, np.int32), g.up(mp, np.int32)
        tp, ty, tw, tn = g.up(pred), g.up(y), g.up(w), g.up(names, np.int32)
        dmean = np.random.default_rng(k).standard_normal(M).astype(np.float32)
        td = g.up(dmean)
        for c in (None, R.member_weights(7 + k, qp)):
            tc = None if c is None else g.up(c)
            for with_names in (True, False):
                mo, yo, wo = g.nan(M), g.nan(M), g.nan(M)
                no = g.torch.full((M,), -1, dtype=g.torch.int32, device=g.dev) if with_names else None
                rc = g.lib.ng_group_mean(g.h, g.st, N, G, Q, ptr(tgp), ptr(tqp), ptr(tmp), ptr(tp), ptr(tc), ptr(ty), ptr(tw),
                                         ptr(tn) if with_names else None, ptr(mo), ptr(yo), ptr(wo), ptr(no))
                assert rc == 0, g.err()
                rm, ry, rw, rn = R.group_mean_f32(gp, qp, pred, y, w, c=c, names=names)
                tag = f"{case}[{k}] c={'yes' if c is not None else 'NULL'}"
                _same(f"mean_out {tag}", mo, rm)
                _same(f"y_out {tag}", yo, ry)
                _same(f"w_out {tag}", wo, rw)
                if with_names:
                    assert np.array_equal(no.cpu().numpy(), rn), f"names_out {tag}"
            if all(r == 1 for _, r in groups) and c is None:
                _same(f"singleton mean {case}[{k}]", mo, pred)          # R_q = 1: exactly the bits of pred
            for scale in (1.0, 0.25):
                dp = g.nan(N)
                rc = g.lib.ng_group_spread(g.h, g.st, N, G, Q, ptr(tgp), ptr(tqp), ptr(tmp), ptr(td), ptr(tc), scale, ptr(dp))
                assert rc == 0, g.err()
                _same(f"dpred {case}[{k}] c={'yes' if c is not None else 'NULL'} scale={scale}", dp,
                      R.group_spread_f32(gp, qp, dmean, c=c, scale=scale))


def test_refusals(gpu_device):
    from nmrgnn_amd._lib import ptr
    g = Gpu(gpu_device)
    gp, qp, pred, y, w, names = R.make_case(1, [(5, 2), (3, 1)])
    N, G, Q = 13, 3, 2
    mp = R.mean_ptr_of(gp, qp)
    t = dict(gp=g.up(gp, np.int32), qp=g.up(qp, np.int32), mp=g.up(mp, np.int32), p=g.up(pred), y=g.up(y), w=g.up(w),
             n=g.up(names, np.int32), mo=g.nan(8), yo=g.nan(8), wo=g.nan(8), no=g.up(np.zeros(8), np.int32), d=g.up(np.ones(8)),
             dp=g.nan(N))

    def mean(N=N, G=G, Q=Q, **kw):
        a = {k: ptr(kw.get(k, t[k])) for k in t}
        return g.lib.ng_group_mean(g.h, g.st, N, G, Q, a["gp"], a["qp"], a["mp"], a["p"], None, a["y"], a["w"], a["n"], a["mo"],
                                   a["yo"], a["wo"], a["no"])

    def spread(N=N, G=G, Q=Q, **kw):
        a = {k: ptr(kw.get(k, t[k])) for k in t}
        return g.lib.ng_group_spread(g.h, g.st, N, G, Q, a["gp"], a["qp"], a["mp"], a["d"], None, 1.0, a["dp"])

    for call in (mean, spread):
        for kw, text in ((dict(Q=0), "at least one group"), (dict(Q=G + 1), "more groups than graphs"),
                         (dict(N=1 << 31), "2^31 atoms or more"), (dict(N=2), "fewer atoms than graphs"),
                         (dict(gp=None), "graph_ptr, group_ptr and mean_ptr required"),
                         (dict(qp=None), "graph_ptr, group_ptr and mean_ptr required"),
                         (dict(mp=None), "graph_ptr, group_ptr and mean_ptr required")):
            assert call(**kw) != 0, (call.__name__, kw)
            assert text in g.err(), (call.__name__, kw, g.err())
    for kw, text in ((dict(n=None), "names and names_out go together"), (dict(no=None), "names and names_out go together"),
                     (dict(p=None), "pred, y, w and their outputs required"), (dict(mo=None), "pred, y, w and their outputs required")):
        assert mean(**kw) != 0 and text in g.err(), (kw, g.err())
    for kw in (dict(d=None), dict(dp=None)):
        assert spread(**kw) != 0 and "dmean and dpred required" in g.err(), (kw, g.err())
    g.torch.cuda.synchronize(gpu_device)
    assert bool(g.torch.isnan(t["mo"]).all()) and bool(g.torch.isnan(t["dp"]).all())        # nothing was launched
    assert mean() == 0 and spread() == 0


# ------------------------------------------------------------------------------------------------- Engine.loss_groups
def _engine(dev):
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    return Engine(declare_gnn_space(HyperParameters(atom_feature_size=64)), 10, device=dev, seed=5)


def _batch(dev, gp):
    """a GraphBatch whose graphs are the rows ``gp`` of one synthetic graph: only the partition matters to the loss"""
    from nmrgnn_amd import synth
    from nmrgnn_amd.graph import GraphBatch
    b = synth.make_batch(1, int(gp[-1]), 16, 10, 0.05, seed=3)
    return GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=gp, device=dev, validate=False)


def test_singleton_groups_are_the_ungrouped_loss(gpu_device):
    """group_ptr = arange(G + 1): loss and dpred are the bits of the ungrouped loss on the same peaks, one graph with all
    weights zero (divide_no_nan).  s = 0.5: Engine.loss_name.  s = 1.0: Engine.loss_groups takes ng_loss_l2 there, as the plain
    training step does, so the bits are those of Engine.loss_l2; ng_loss_name(s = 1) keeps its sums in float64 and differs from
    ng_loss_l2 in the last bits (tests/test_gpu_head_embed.py bounds both by 3e-5 of each entry), so against
    Engine.loss_name(s = 1) the comparison is that bound, twice (one for each kernel)."""
    import torch
    g = Gpu(gpu_device)
    eng = _engine(gpu_device)
    gp, qp, pred, y, w, _ = R.make_case(21, [(7, 1), (63, 1), (129, 1), (101, 1)], zero_weight_group=2)
    batch = _batch(gpu_device, gp)
    ty, tw, tp = g.up(y), g.up(w), g.up(pred)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    for s, plain in ((0.5, lambda: eng.loss_name(batch, ty, tw, tp, 0.5)), (1.0, lambda: eng.loss_l2(batch, ty, tw, tp))):
        loss, dpred, means, (yg, wg) = eng.loss_groups(batch, ty, tw, tp, np.arange(batch.G + 1), s=s)
        rl, rd = plain()
        assert torch.equal(bits(loss), bits(rl)) and torch.equal(bits(dpred), bits(rd)), s
        assert torch.equal(bits(means), bits(tp)) and torch.equal(bits(yg), bits(ty)) and torch.equal(bits(wg), bits(tw))
        assert bool((dpred[gp[2]:gp[3]] == 0).all())
    nl, nd = eng.loss_name(batch, ty, tw, tp, 1.0)
    assert abs(float(loss) - float(nl)) <= 6e-5 * abs(float(nl))
    assert bool(((dpred - nd).abs() <= 6e-5 * nd.abs() + 2e-7 * nd.abs().max()).all())


@pytest.mark.parametrize("s", [1.0, 0.5])
@pytest.mark.parametrize("weighted", [False, True])
def test_three_groups_against_float64(gpu_device, s, weighted):
    """R = 2, 3, 1 members of 70, 33 and 129 atoms, carbon-like shifts (120 +- 3, members 0.7 around the label).  The bound of
    tests/test_gpu_head_embed.py for ng_loss_l2 / ng_loss_name (3e-5 of each |dpred| entry) does not transfer: there y - pred is
    exact in float32, here the float32 MEAN near 120 carries up to 1e-5 of rounding into a difference near 0.7, whatever the
    entry's size.  So the bound is measured as the issue of this feature prescribes: the error of the float32 restatement
    (group_loss_ref.ensemble_loss_f32: float32 mean and spread; the loss in float32 for s = 1 as ng_loss_l2 works, in float64
    for s < 1 as ng_loss_name does) against the float64 one on the same inputs, times four for the device's summation order.
    Measured on the CPU (the test computes them again on its inputs; grad_weight 0.25, largest |dpred| 4e-3 at s = 1):
        plain mean     s = 1.0: max |dpred32 - dpred64| = 1.51e-8, |loss32 - loss64| = 4.60e-7 (loss 0.306)
                       s = 0.5: max |dpred32 - dpred64| = 8.37e-9, |loss32 - loss64| = 2.57e-7 (loss 0.164)
        member weights s = 1.0: 3.23e-8 and 1.93e-7;  s = 0.5: 1.80e-8 and 1.04e-7
    The device's errors on the MI355X were these to three digits (loss at s = 1 with weights: 1.63e-7).
    A single loss can round luckily, so its measured error counts as at least half a float32 ulp of the loss."""
    g = Gpu(gpu_device)
    eng = _engine(gpu_device)
    gp, qp, pred, y, w, _ = R.make_case(11, [(70, 2), (33, 3), (129, 1)])
    c = R.member_weights(12, qp) if weighted else None
    batch = _batch(gpu_device, gp)
    loss, dpred, means, _ = eng.loss_groups(batch, g.up(y), g.up(w), g.up(pred), qp, s=s, member_weights=c, grad_weight=0.25)
    l64, d64, m64 = R.ensemble_loss_f64(gp, qp, pred, y, w, s=s, c=c, scale=0.25)
    l32, d32 = R.ensemble_loss_f32(gp, qp, pred, y, w, s=s, c=c, scale=0.25, loss_dtype=np.float32 if s == 1.0 else np.float64)
    d_err = float(np.max(np.abs(d32 - d64)))
    l_err = max(abs(float(l32) - l64), 2.0 ** -24 * abs(l64))
    got_d, got_l = dpred.cpu().numpy().astype(np.float64), float(loss)
    print(f"s={s} weighted={weighted}: restatement dpred err {d_err:.3e} loss err {l_err:.3e}; device dpred err "
          f"{np.max(np.abs(got_d - d64)):.3e} loss err {abs(got_l - l64):.3e}")
    assert d_err > 0 and np.max(np.abs(got_d - d64)) <= 4 * d_err
    assert abs(got_l - l64) <= 4 * l_err
    _same("means", means, R.group_mean_f32(gp, qp, pred, y, w, c=c)[0])


def test_host_checks_before_any_launch(gpu_device):
    g = Gpu(gpu_device)
    eng = _engine(gpu_device)
    gp = np.array([0, 5, 10, 14], np.int32)
    batch = _batch(gpu_device, gp)
    y = w = p = g.up(np.ones(14))
    with pytest.raises(ValueError, match="group 0: graph 2 has 4 atoms"):
        eng.loss_groups(batch, y, w, p, [0, 3])
    for bad in ([0, 2], [1, 3], [0, 2, 2, 3], [0, 3, 2], [0], np.array([0.0, 3.0])):
        with pytest.raises(ValueError, match="group_ptr"):
            eng.loss_groups(batch, y, w, p, bad)
    with pytest.raises(ValueError, match="member_weights has 2 entries"):
        eng.loss_groups(batch, y, w, p, [0, 2, 3], member_weights=np.ones(2, np.float32))
    with pytest.raises(ValueError, match="balance"):
        eng.loss_groups(batch, y, w, p, [0, 2, 3], s=1.5)
    loss, dpred, means, _ = eng.loss_groups(batch, y, w, p, [0, 2, 3])
    assert means.shape == (9,) and dpred.shape == (14,) and float(loss) == 0.0
