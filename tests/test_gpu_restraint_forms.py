"""Shift-restraint forms on the GPU: ng_restraint_loss_ex against a NumPy restatement of its float32 expressions (replica
weights, independent replicas, flat-bottom tolerance, running average over three calls), its defaults against
ng_restraint_loss bit for bit, ShiftRestraint's forms against float64 torch autograd through oracle/torch_ref (R = 4 108M
frames, open and orthorhombic), replay against the eager chain over 5 calls, reset(), and the call-time refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import hp_to_oracle
from test_gpu_restraint import _box_dims, _frames, _mic_images, _model, _structure

pytestmark = pytest.mark.gpu
f32 = np.float32


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


# ------------------------------------------------------------------------------------------------ 1: the kernel
def _loss_ex(ctx, R, n, indep, peaks, y, w, c, tol, lam, avg, primed):
    from nmrgnn_amd._lib import ptr
    G = R if indep else 1
    e = torch.full((G,), np.nan, dtype=torch.float64, device=_dev())
    dp = torch.full((R * n,), np.nan, dtype=torch.float32, device=_dev())
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    ctx.check(ctx.lib.ng_restraint_loss_ex(ctx.handle, st, R, n, int(indep), ptr(peaks), ptr(y), ptr(w), ptr(c), ptr(tol),
                                           float(lam), ptr(avg), ptr(primed), ptr(e), ptr(dp)), "ng_restraint_loss_ex")
    torch.cuda.synchronize()
    return e, dp


def _ref_ex(R, n, indep, peaks, y, w, c, tol, lam, avg, primed):
    """the header's float32 expressions in NumPy: (float32 terms [G, n], dpeaks [R*n], avg after the call [G*n] or None)"""
    P = peaks.reshape(R, n)
    if indep:
        m = P.copy()
    elif c is not None:
        m = c[0] * P[0]
        for r in range(1, R):
            m = m + c[r] * P[r]
        m = m[None]
    else:
        s = P[0].copy()
        for r in range(1, R):
            s = s + P[r]
        m = (s / f32(R))[None]
    G = m.shape[0]
    a, da = m, f32(1)
    if lam > 0 and primed:
        da = f32(1) - f32(lam)
        a = f32(lam) * avg.reshape(G, n) + da * m
    d = a - y
    e = np.abs(d)
    if tol is not None:
        x = e - tol
        e = np.where(x < 0, f32(0), x).astype(f32)
    terms = (e * e) * w
    q = w * (f32(2) * np.copysign(e, d))
    if da != 1:
        q = q * da
    if indep:
        dp = q.reshape(-1)
    elif c is not None:
        dp = np.concatenate([q[0] * c[r] for r in range(R)])
    else:
        dp = np.tile(q[0] / f32(R), R)
    for x in (m, a, terms, q, dp):
        assert x.dtype == np.float32
    return terms, dp, (a.reshape(-1).copy() if lam > 0 else None), d


# (independent, replica weights, tolerance, lambda)
FORMS = [(False, False, False, 0.0), (False, True, False, 0.0), (False, False, True, 0.0), (False, True, True, 0.7),
         (False, False, True, 0.7), (True, False, False, 0.0), (True, False, True, 0.0), (True, False, True, 0.9)]


@pytest.mark.parametrize("form", FORMS, ids=["ens", "ens-c", "ens-tol", "ens-c-tol-avg", "ens-tol-avg", "ind", "ind-tol",
                                             "ind-tol-avg"])
@pytest.mark.parametrize("n", [1, 2770, 100000])
@pytest.mark.parametrize("R", [1, 2, 8])
def test_restraint_loss_ex_against_numpy(R, n, form):
    from nmrgnn_amd import _lib
    indep, use_c, use_tol, lam = form
    lam = float(f32(lam))
    ctx = _lib.get_context(0)
    rng = np.random.default_rng(R * 1000 + n + 17 * FORMS.index(form))
    G = R if indep else 1
    y = (rng.standard_normal(n) * 30.0 + 50.0).astype(f32)
    w = rng.random(n).astype(f32)
    w[rng.random(n) < 0.3] = 0.0
    c = rng.random(R).astype(f32) if use_c else None
    tol = (rng.random(n) * 40.0).astype(f32) if use_tol else None
    if tol is not None:
        tol[rng.random(n) < 0.2] = 0.0
    seq = [(rng.standard_normal(R * n) * 30.0 + 50.0).astype(f32) for _ in range(3)]

    def run():
        avg = torch.full((G * n,), np.nan, dtype=torch.float32, device=_dev()) if lam > 0 else None
        primed = torch.zeros(1, dtype=torch.int32, device=_dev()) if lam > 0 else None
        out = []
        for peaks in seq:
            e, dp = _loss_ex(ctx, R, n, indep, _t(peaks), _t(y), _t(w), _t(c), _t(tol), lam, avg, primed)
            out.append((e.clone(), dp.clone(), None if avg is None else avg.clone(),
                        None if primed is None else int(primed.item())))
        return out

    first, again = run(), run()
    avg_h, primed_h, inside_seen = None, 0, False
    for call, peaks in enumerate(seq):
        e, dp, avg_d, primed_d = first[call]
        terms, dp_ref, avg_ref, d = _ref_ex(R, n, indep, peaks, y, w, c, tol, lam, avg_h, primed_h)
        assert np.array_equal(dp.cpu().numpy().view(np.int32), dp_ref.view(np.int32)), call
        if lam > 0:
            assert np.array_equal(avg_d.cpu().numpy().view(np.int32), avg_ref.view(np.int32)), call
            assert primed_d == 1
            avg_h, primed_h = avg_ref, 1
        ref = terms.astype(np.float64).sum(axis=1)
        got = e.cpu().numpy()
        assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), (call, got, ref)
        if tol is not None:                                  # inside the band: exactly no energy and no force
            inside = np.abs(d) < tol
            inside_seen |= bool(inside.any())
            assert (terms[inside] == 0).all()
            dpr = dp.cpu().numpy().reshape(R, n)
            if indep:
                assert (dpr[inside] == 0).all()
            else:
                assert (dpr[:, inside[0]] == 0).all()
        # the same inputs give the same bits
        e2, dp2, avg2, _ = again[call]
        assert torch.equal(_bits(e), _bits(e2)) and torch.equal(_bits(dp), _bits(dp2))
        if lam > 0:
            assert torch.equal(_bits(avg_d), _bits(avg2))
    if tol is not None and n > 1:
        assert inside_seen


@pytest.mark.parametrize("n", [1, 2770, 100000])
@pytest.mark.parametrize("R", [1, 2, 8])
def test_restraint_loss_ex_defaults_are_restraint_loss(R, n):
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    ctx = _lib.get_context(0)
    rng = np.random.default_rng(R * 7 + n)
    peaks = _t((rng.standard_normal(R * n) * 30.0 + 50.0).astype(f32))
    y = _t((rng.standard_normal(n) * 30.0 + 50.0).astype(f32))
    w = rng.random(n).astype(f32)
    w[rng.random(n) < 0.3] = 0.0
    w = _t(w)
    e0 = torch.full((1,), np.nan, dtype=torch.float64, device=_dev())
    dp0 = torch.full((R * n,), np.nan, dtype=torch.float32, device=_dev())
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    ctx.check(ctx.lib.ng_restraint_loss(ctx.handle, st, R, n, ptr(peaks), ptr(y), ptr(w), ptr(e0), ptr(dp0)), "ng_restraint_loss")
    for tol in (None, torch.zeros(n, dtype=torch.float32, device=_dev())):
        e, dp = _loss_ex(ctx, R, n, False, peaks, y, w, None, tol, 0.0, None, None)
        assert torch.equal(_bits(e), _bits(e0)) and torch.equal(_bits(dp), _bits(dp0))


def test_restraint_loss_ex_refusals():
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    ctx = _lib.get_context(0)
    n, R = 8, 2
    p, y, w = (torch.zeros(R * n, device=_dev()), torch.zeros(n, device=_dev()), torch.ones(n, device=_dev()))
    c = torch.ones(R, device=_dev())
    avg, primed = torch.zeros(R * n, device=_dev()), torch.zeros(1, dtype=torch.int32, device=_dev())
    e, dp = torch.zeros(R, dtype=torch.float64, device=_dev()), torch.zeros(R * n, device=_dev())
    st = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    call = lambda R_, n_, mode, c_, lam, a, pr: ctx.lib.ng_restraint_loss_ex(
        ctx.handle, st, R_, n_, mode, ptr(p), ptr(y), ptr(w), ptr(c_), None, lam, ptr(a), ptr(pr), ptr(e), ptr(dp))
    assert call(R, n, 0, c, 0.5, avg, primed) == 0
    for bad in [(2, 1 << 30, 0, None, 0.0, None, None),         # R * n = 2^31
                (R, n, 0, None, 1.0, avg, primed), (R, n, 0, None, -0.1, avg, primed),
                (R, n, 0, None, float("nan"), avg, primed),     # lambda outside [0, 1)
                (R, n, 1, c, 0.0, None, None),                  # c in independent mode
                (R, n, 0, None, 0.5, None, primed), (R, n, 0, None, 0.5, avg, None),   # no state with lambda > 0
                (R, n, 2, None, 0.0, None, None)]:              # no such mode
        assert call(*bad) != 0, bad
    torch.cuda.synchronize()
    assert int(primed.item()) == 1                              # only the accepted call ran


# ------------------------------------------------------------------------------------------------ ShiftRestraint helpers
class _RefPeaks:
    """float64 torch peaks [R, n] (pos [R*n, 3], h [R, 3, 3]) over the restraint's lists of the LAST call (read back from
    its batch) and the float64 minimum images of those positions, both held fixed"""

    def __init__(self, model, atoms, batch, frames, vecs):
        from oracle import torch_ref
        self.R, self.n = frames.shape[:2]
        N = self.R * self.n
        self.nlist = batch.nlist.cpu().numpy().astype(np.int64)
        self.live = batch.edges.detach().cpu().numpy() > 0
        self.src = np.broadcast_to(np.arange(N)[:, None], self.nlist.shape)
        self.frame = torch.from_numpy(np.arange(N) // self.n)
        p = frames.reshape(N, 3).astype(np.float64)
        d = p[self.nlist] - p[self.src]
        img = np.zeros_like(d)
        if vecs is not None:
            for g in range(self.R):
                rows = slice(g * self.n, (g + 1) * self.n)
                img[rows] = _mic_images(d[rows].reshape(-1, 3), vecs[g]).reshape(d[rows].shape)
        self.vecs = np.zeros((self.R, 3, 3)) if vecs is None else vecs
        self.img = torch.from_numpy(img)
        self.params = torch_ref.to_torch_params(model.get_weights())
        self.hp = hp_to_oracle(model.hypers)
        C_ = atoms.shape[1]
        self.std, self.avg = model.peak_std[:C_], model.peak_avg[:C_]
        self.atoms = np.tile(atoms, (self.R, 1))
        self.inv = batch.inv_degree.cpu().numpy()
        self.fwd = torch_ref.forward

    def peaks(self, frames):
        """(peaks [R, n] as a function of positions and a per-replica strain, positions, strain) at these positions"""
        eps = torch.zeros(self.R, 3, 3, dtype=torch.float64, requires_grad=True)
        T = torch.eye(3, dtype=torch.float64) + eps
        pos = torch.from_numpy(frames.reshape(-1, 3).astype(np.float64)).requires_grad_(True)
        x = torch.einsum("nc,ncd->nd", pos, T[self.frame])
        h = torch.einsum("gkc,gcd->gkd", torch.from_numpy(self.vecs), T)
        nl, src = torch.from_numpy(self.nlist), torch.from_numpy(np.ascontiguousarray(self.src))
        u = x[nl] - x[src] + torch.einsum("nkc,ncd->nkd", self.img, h[self.frame])
        dist = torch.sqrt((u * u).sum(-1).clamp_min(1e-300)) * 0.1
        dd = torch.where(torch.from_numpy(self.live), dist, torch.zeros_like(dist))
        pk = self.fwd((self.atoms, self.nlist, dd, self.inv), self.params, self.hp, peak_std=self.std, peak_avg=self.avg)
        return pk.reshape(self.R, self.n), pos, eps


def _setup(R, kind, seed):
    from nmrgnn_amd.pbc import triclinic_vectors
    atoms, p = _structure("108M.pdb")
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    targets = (rng.standard_normal(n) * 3.0).astype(f32)
    w = rng.random(n).astype(f32)
    w[rng.random(n) < 0.2] = 0.0
    box = _box_dims(p, kind)
    boxes = None if box is None else np.stack([box * np.array([1 + 0.02 * r] * 3 + [1] * 3) for r in range(R)])
    vecs = None if boxes is None else np.stack([triclinic_vectors(b).astype(f32).astype(np.float64) for b in boxes])

    def frames_at(call):
        fr = _frames(p, R, rng, sigma=0.1 + 0.02 * call)
        if vecs is not None:            # every replica wrapped into its box with the protein across the faces
            for k in range(R):
                c = fr[k] - fr[k].mean(0) + np.array([0.4, -0.7, 0.3])
                f = c @ np.linalg.inv(vecs[k])
                fr[k] = ((f - np.floor(f)) @ vecs[k]).astype(f32)
        return fr
    return atoms, p, n, rng, targets, w, boxes, vecs, frames_at


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


# ------------------------------------------------------------------------------------------------ 3: vs float64 autograd
FORM_KINDS = ["flat", "weighted", "independent", "averaged"]


@pytest.mark.parametrize("kind", ["none", "ortho"])
@pytest.mark.parametrize("form", FORM_KINDS)
def test_forms_against_float64_autograd(form, kind):
    from nmrgnn_amd.library import ShiftRestraint
    R = 4
    atoms, p, n, rng, targets, w, boxes, vecs, frames_at = _setup(R, kind, seed=4)
    model = _model()
    model.build(atoms.shape[1])
    kw, calls = {}, 1
    tol = None
    if form == "flat":      # about half of the atoms inside their band: tol = |mean - y| times U(0, 2) at these frames
        frames = frames_at(0)
        r0 = ShiftRestraint(model, atoms, targets, w, replicas=R, box=boxes, replay=False)
        r0(frames, box=boxes)
        torch.cuda.synchronize()
        m0 = _RefPeaks(model, atoms, r0._batch, frames, vecs).peaks(frames)[0].mean(0).detach().numpy()
        tol = (np.abs(m0 - targets) * rng.uniform(0.0, 2.0, n)).astype(f32)
        kw = dict(tolerance=tol)
        frames_at = lambda call: frames
    elif form == "weighted":
        cs = [np.array([0.1, 0.4, 0.2, 0.3]), np.array([3.0, 1.0, 0.5, 0.0])]
        kw, calls = dict(replica_weights=cs[0]), 2
    elif form == "independent":
        kw = dict(independent=True)
    else:
        kw, calls = dict(tau=4.0), 5
    lam = float(f32(np.exp(-1.0 / 4.0)))
    r = ShiftRestraint(model, atoms, targets, w, replicas=R, box=boxes, virial=True, **kw)
    y64, w64 = torch.from_numpy(targets.astype(np.float64)), torch.from_numpy(w.astype(np.float64))
    a_prev = None
    worst = [0.0, 0.0, 0.0]
    for call in range(calls):
        frames = frames_at(call)
        ck = None
        if form == "weighted":
            ck = cs[call] / cs[call].sum()
            e, f, v = r(frames, box=boxes, replica_weights=None if call == 0 else cs[call])
        else:
            e, f, v = r(frames, box=boxes)
        torch.cuda.synchronize()
        ref = _RefPeaks(model, atoms, r._batch, frames, vecs)
        pk, pos, eps = ref.peaks(frames)
        if form == "independent":
            m = pk
        elif ck is not None:
            m = (torch.from_numpy(ck)[:, None] * pk).sum(0, keepdim=True)
        else:
            m = pk.mean(0, keepdim=True)
        a = m if a_prev is None else lam * a_prev + (1.0 - lam) * m
        if form == "averaged":
            a_prev = a.detach()
        d = a - y64
        e_ = torch.relu(d.abs() - torch.from_numpy(tol.astype(np.float64))) if tol is not None else d.abs()
        Er = (e_ * e_ * w64).sum(1)
        Er.sum().backward()
        E = Er.detach().numpy()
        dpos, strain = pos.grad.numpy().reshape(frames.shape), eps.grad.numpy()
        if form == "independent":
            got = r.energies.cpu().numpy()
            assert got.shape == (R,) and got.dtype == np.float64
            errs = (_rel(got, E), _rel(f.cpu().numpy(), -dpos), _rel(v.cpu().numpy(), -strain))
            assert abs(float(e) - E.sum()) <= 1e-4 * abs(E.sum())
        else:
            errs = (abs(float(e) - E[0]) / abs(E[0]), _rel(f.cpu().numpy(), -dpos), _rel(v.cpu().numpy(), -strain))
        worst = [max(x, y) for x, y in zip(worst, errs)]
        assert max(errs) <= 1e-4, (call, errs)
        if form == "flat":
            inside = (np.abs(d.detach().numpy()) < tol)
            assert 0.1 < inside.mean() < 0.9
    print(f"R=4 {form} {kind}: energy {worst[0]:.2e} forces {worst[1]:.2e} virial {worst[2]:.2e}")


# ------------------------------------------------------------------------------------------------ 4: replay vs eager
REPLAY_FORMS = {"flat": dict(tolerance=0.3), "weighted": dict(replica_weights=[1.0, 2.0, 3.0]),
                "independent": dict(independent=True), "averaged": dict(tau=3.0),
                "all-ensemble": dict(tolerance=0.2, replica_weights=[0.5, 0.2, 0.3], tau=2.0),
                "all-independent": dict(tolerance=0.2, independent=True, tau=2.0)}


@pytest.mark.parametrize("form", list(REPLAY_FORMS))
def test_forms_replay_equals_eager_over_calls(form):
    from nmrgnn_amd.library import ShiftRestraint
    R = 3
    atoms, p, n, rng, targets, w, boxes, vecs, frames_at = _setup(R, "ortho", seed=6)
    model = _model()
    model.build(atoms.shape[1])
    kw = REPLAY_FORMS[form]
    ra = ShiftRestraint(model, atoms, targets, w, replicas=R, box=boxes, virial=True, **kw)
    rb = ShiftRestraint(model, atoms, targets, w, replicas=R, box=boxes, virial=True, replay=False, **kw)
    outs = []
    for call in range(5):
        frames = frames_at(call)
        cw = {}
        if "replica_weights" in kw and call in (1, 3):
            cw = dict(replica_weights=rng.random(R) + 0.1)
        outa = [t.clone() for t in ra(frames, box=boxes, **cw)] + [ra.energies.clone()]
        outb = [t.clone() for t in rb(frames, box=boxes, **cw)] + [rb.energies.clone()]
        torch.cuda.synchronize()
        for x, y in zip(outa, outb):
            assert torch.equal(_bits(x), _bits(y)), call
        assert torch.isfinite(outa[1]).all() and float(outa[0]) > 0
        outs.append((frames, outa))
    if "tau" in kw:         # reset(): the next call is the first call of a fresh object
        cw = dict(replica_weights=kw["replica_weights"]) if "replica_weights" in kw else {}
        for r in (ra, rb):
            r.reset()
            out = [t.clone() for t in r(outs[0][0], box=boxes, **cw)] + [r.energies.clone()]
            torch.cuda.synchronize()
            for x, y in zip(out, outs[0][1]):
                assert torch.equal(_bits(x), _bits(y))


# ------------------------------------------------------------------------------------------------ 2: defaults change nothing
def test_defaults_are_bitwise_the_harmonic_restraint():
    from nmrgnn_amd.library import ShiftRestraint
    R = 2
    atoms, p, n, rng, targets, w, boxes, vecs, frames_at = _setup(R, "ortho", seed=8)
    model = _model()
    model.build(atoms.shape[1])
    r0 = ShiftRestraint(model, atoms, targets, w, replicas=R, box=boxes, virial=True)
    r1 = ShiftRestraint(model, atoms, targets, w, replicas=R, box=boxes, virial=True, tolerance=None, replica_weights=None,
                        independent=False, tau=None)
    r2 = ShiftRestraint(model, atoms, targets, w, replicas=R, box=boxes, virial=True, tolerance=0.0)   # the _ex kernel
    assert not r0._ex and not r1._ex and r2._ex
    for call in range(3):
        frames = frames_at(call)
        o0 = [t.clone() for t in r0(frames, box=boxes)]
        for r in (r1, r2):
            o = [t.clone() for t in r(frames, box=boxes)]
            torch.cuda.synchronize()
            for x, y in zip(o, o0):
                assert torch.equal(_bits(x), _bits(y)), call


# ------------------------------------------------------------------------------------------------ 5: call-time refusals
def test_call_refusals_leave_the_state_alone():
    from nmrgnn_amd.library import ShiftRestraint
    atoms, p = _structure("108M.pdb")
    n = p.shape[0]
    targets = np.zeros(n, np.float32)
    model = _model()
    model.build(atoms.shape[1])
    fr = _frames(p, 2, np.random.default_rng(9), sigma=0.1)
    r1 = ShiftRestraint(model, atoms, targets)
    with pytest.raises(ValueError):
        r1(p, replica_weights=[1.0])                      # R = 1
    r2 = ShiftRestraint(model, atoms, targets, replicas=2)
    with pytest.raises(ValueError):
        r2(fr, replica_weights=[1.0, 1.0])                # built without weights
    rw = ShiftRestraint(model, atoms, targets, replicas=2, replica_weights=[1.0, 3.0])
    e0 = rw(fr)[0].clone()
    for bad in ([1.0, 1.0, 1.0], [0.0, 0.0], [1.0, -1.0], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            rw(fr, replica_weights=bad)
    assert torch.equal(_bits(rw(fr)[0]), _bits(e0))     # the staged weights are still [0.25, 0.75]
    assert torch.equal(_bits(rw.s_c), _bits(torch.tensor([0.25, 0.75], device=_dev())))
    assert not torch.equal(_bits(rw(fr, replica_weights=[1.0, 1.0])[0]), _bits(e0))
    with pytest.raises(ValueError):
        ShiftRestraint(model, atoms, targets, replicas=2, replica_weights=[1.0, 1.0], independent=True)
