"""ng_adam_step_groups and ng_grad_clip_factor (csrc/optim.hip) through the C ABI, against ng_adam_step
itself, the float64 references of finetune_ref.py and exact cases.  Every buffer is n + GUARD long with NaN behind n: an
element written past the end fails.

Sizes: n = 1, 255, 257 and 256 * 2048 + 259 (more elements than the 2048 x 256 threads of the grid: the second pass of the
grid stride).  Segment tables ("layouts", boundaries off multiples of four):
  three   first at 0, last ending at n, a one-element segment between them
  gap     two ranges separated by one element
  whole   [0, n)
n = 1 has room for the single range alone (with empty ranges beside it).

Bounds.  One float32 rounding is U = 2^-24 relative.
  scale 1 / 0.5 / 2   p, m, v bit for bit those of ng_adam_step at lr / lr * scale on the segment's elements.
  scale 0, no segment every bit of p, m, v as it was, with NaN in g, m and v there.
  scale 0.3           the count of test_gpu_node_small.py for ng_adam_step, plus one rounding for the rate product:
                      m within 2 U |b1 m| + 3 U |(1 - b1) g'|, v within 2 U b2 v + 5 U (1 - b2) g'^2,
                      p within U |p| + 11.5 U rate (|b1 m| + |(1 - b1) g'|) / (sqrt(v) + eps), rate = float32(lr_t * 0.3).
  clip factor         the same bits on two runs; the norm within n 2^-53 relative of the float64 reference (the squares of
                      float32 values are exact in float64: only the n - 1 additions round, the root halves their relative
                      error and adds one rounding of its own; for n = 1 the sum is one exact square and its root is exact);
                      the factor within twice that (the quotient rounds once more), exactly 1 below the threshold, for a
                      zero gradient and for a NaN gradient."""
import ctypes as C

import numpy as np
import pytest

import finetune_ref as FR
import node_small_ref as R

pytestmark = pytest.mark.gpu

U = R.U24
GUARD = 8
NBIG = 256 * 2048 + 259
SIZES = [1, 255, 257, NBIG]
ARGS = (1e-3, 0.9, 0.999, 1e-7, 3)            # lr, b1, b2, eps, step
NG_ERR_INVALID, NG_ERR_UNSUPPORTED = -1, -4


def layouts(n):
    if n == 1:
        return {"whole": [(0, 1)], "empties": [(0, 0), (0, 1), (1, 1)]}
    return {"three": [(0, 101), (130, 131), (133, n)], "gap": [(0, 77), (78, n)], "whole": [(0, n)]}


CASES = [(n, name) for n in SIZES for name in layouts(n)]


class Gpu:
    def __init__(self, dev):
        import torch
        from nmrgnn_amd import _lib
        self.torch, self.dev, self.ptr = torch, dev, _lib.ptr
        self.ctx = _lib.get_context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def up(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)

    def ok(self, rc, what):
        self.ctx.check(rc, what)


def table(segs):
    """(n_seg, begin, end, scale) as the entry points take them; segs: [(begin, end, scale)]"""
    k = max(len(segs), 1)
    return (len(segs), (C.c_int64 * k)(*[s[0] for s in segs]), (C.c_int64 * k)(*[s[1] for s in segs]),
            (C.c_float * k)(*[s[2] for s in segs]))


class State:
    """p, g, m, v on the device, n + GUARD long with NaN behind n"""

    def __init__(self, g, n, p, grad, m, v):
        self.g, self.n = g, n
        pad = lambda a: g.up(np.concatenate([np.asarray(a, np.float32), np.full(GUARD, np.nan, np.float32)]))
        self.t = [pad(p), pad(grad), pad(m), pad(v)]

    def plain(self, lr, b1, b2, eps, step, gscale=1.0):
        g = self.g
        g.ok(g.lib.ng_adam_step(g.h, g.st, self.n, *[g.ptr(x) for x in self.t], lr, b1, b2, eps, step, gscale), "ng_adam_step")
        return self

    def grouped_rc(self, lr, b1, b2, eps, step, segs, gscale=1.0, clip=None):
        g = self.g
        return g.lib.ng_adam_step_groups(g.h, g.st, self.n, *[g.ptr(x) for x in self.t], lr, b1, b2, eps, step, gscale,
                                         *table(segs), g.ptr(clip))

    def grouped(self, *a, **kw):
        self.g.ok(self.grouped_rc(*a, **kw), "ng_adam_step_groups")
        return self

    def read(self):
        """p, m, v: the first n elements as float32; the guard behind them must be untouched"""
        out = []
        for x in (self.t[0], self.t[2], self.t[3]):
            a = x.cpu().numpy()
            assert np.isnan(a[self.n:]).all(), f"written past n = {self.n}"
            out.append(a[:self.n])
        return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(name, got, want, where=None):
    bad = bits(got) != bits(want)
    if where is not None:
        bad &= where
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} elements differ; first at {k}: {got[k]!r} != {want[k]!r}")


def within(name, got, ref, bound, where):
    bad = ~(np.abs(np.asarray(got, np.float64) - ref) <= bound) & where
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} elements fail; first at {k}: {got[k]!r}, {ref[k]!r}, bound {bound[k]!r}")


def data(n, tag):
    rng = np.random.default_rng([n, tag])
    return (R.f32(rng.standard_normal(n)), R.f32(rng.standard_normal(n)), R.f32(0.1 * rng.standard_normal(n)),
            R.f32((0.1 * rng.standard_normal(n)) ** 2))


def mask_of(n, segs):
    on = np.zeros(n, bool)
    for b, e, *sc in segs:
        if not sc or sc[0] > 0:
            on[b:e] = True
    return on


@pytest.mark.parametrize("n,layout", CASES)
def test_scale_one_is_adam_step(gpu_device, n, layout):
    """all scales 1: the segments' elements carry the bits of ng_adam_step, every other element those it had"""
    g = Gpu(gpu_device)
    p, grad, m, v = data(n, 1)
    segs = [(b, e, 1.0) for b, e in layouts(n)[layout]]
    on = mask_of(n, segs)
    want = State(g, n, p, grad, m, v).plain(*ARGS, 3.7).read()
    got = State(g, n, p, grad, m, v).grouped(*ARGS, segs, gscale=3.7).read()
    assert on.any() and (bits(want[0]) != bits(p)).any()
    for name, a, w, x in zip("pmv", got, want, (p, m, v)):
        same_bits(name + " (updated)", a, w, on)
        same_bits(name + " (kept)", a, x, ~on)


@pytest.mark.parametrize("n,layout", CASES)
def test_power_of_two_scales(gpu_device, n, layout):
    """scales 0.5 and 2, alternating over the segments: the bits of ng_adam_step(lr * scale)"""
    g = Gpu(gpu_device)
    p, grad, m, v = data(n, 2)
    segs = [(b, e, (0.5, 2.0)[i % 2]) for i, (b, e) in enumerate(layouts(n)[layout])]
    if layout == "whole":
        segs = [(0, n // 2, 2.0), (n // 2, n, 0.5)]        # touching ranges of different scales
    lr = ARGS[0]
    got = State(g, n, p, grad, m, v).grouped(*ARGS, segs).read()
    kept = np.ones(n, bool)
    for sc in (0.5, 2.0):
        want = State(g, n, p, grad, m, v).plain(float(np.float32(lr) * np.float32(sc)), *ARGS[1:]).read()
        on = mask_of(n, [s for s in segs if s[2] == sc])
        kept &= ~on
        for name, a, w in zip("pmv", got, want):
            same_bits(f"{name} (scale {sc})", a, w, on)
    for name, a, x in zip("pmv", got, (p, m, v)):
        same_bits(name + " (kept)", a, x, kept)


@pytest.mark.parametrize("n", SIZES[1:])
def test_scale_zero_keeps_every_bit(gpu_device, n):
    """a segment of scale 0 and the element of a gap, with NaN in g, m and v there (and an odd NaN payload in p): no bit of
    p, m or v changes, and the NaN gradient reaches nothing; the neighbours are updated as ng_adam_step updates them"""
    g = Gpu(gpu_device)
    p, grad, m, v = data(n, 3)
    segs = [(0, 61, 1.0), (61, 131, 0.0), (133, n, 1.0)]        # frozen [61, 131), nobody's [131, 133)
    off = slice(61, 133)
    want = State(g, n, p, grad, m, v).plain(*ARGS).read()
    grad[off] = m[off] = v[off] = np.nan
    p[70] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    got = State(g, n, p, grad, m, v).grouped(*ARGS, segs).read()
    on = mask_of(n, segs)
    assert not on[off].any() and on.sum() == n - 72
    for name, a, w, x in zip("pmv", got, want, (p, m, v)):
        same_bits(name + " (kept)", a, x, ~on)
        same_bits(name + " (updated)", a, w, on)


@pytest.mark.parametrize("n,layout", [c for c in CASES if c[1] != "whole" or c[0] == 1])
def test_generic_scale_against_float64(gpu_device, n, layout):
    g = Gpu(gpu_device)
    p, grad, m, v = data(n, 4)
    segs = [(b, e, 0.3) for b, e in layouts(n)[layout]]
    gscale = 3.7
    pr, mr, vr, mag, on = FR.adam_groups_ref(p, grad, m, v, *ARGS, gscale, segs)
    gp, gm, gv = State(g, n, p, grad, m, v).grouped(*ARGS, segs, gscale=gscale).read()
    tiny = 2.0 ** -149
    within("m", gm, mr, U * (2 * mag["m1"] + 3 * mag["m2"]) + tiny, on)
    within("v", gv, vr, U * (2 * mag["v1"] + 5 * mag["v2"]) + tiny, on)
    within("p", gp, pr, U * (np.abs(p) + 11.5 * mag["upd"]) + tiny, on)
    assert (np.abs(gp.astype(np.float64) - p)[on] > 0).any()
    for name, a, x in zip("pmv", (gp, gm, gv), (p, m, v)):
        same_bits(name + " (kept)", a, x, ~on)


REFUSALS = {
    "unsorted": [(100, 120, 1.0), (10, 20, 1.0)],
    "overlap": [(10, 60, 1.0), (59, 80, 1.0)],
    "past n": [(10, 20, 1.0), (200, 301, 1.0)],
    "negative begin": [(-1, 20, 1.0)],
    "end before begin": [(30, 20, 1.0)],
    "65 ranges": [(4 * i, 4 * i + 3, 1.0) for i in range(65)],
    "negative scale": [(10, 20, -0.5)],
    "nan scale": [(10, 20, float("nan"))],
    "inf scale": [(10, 20, float("inf"))],
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(gpu_device, what):
    """NG_ERR_INVALID with a message, p, m, v untouched — from both entry points"""
    g = Gpu(gpu_device)
    n = 300
    p, grad, m, v = data(n, 5)
    s = State(g, n, p, grad, m, v)
    assert s.grouped_rc(*ARGS, REFUSALS[what]) == NG_ERR_INVALID, what
    assert g.lib.ng_last_error(g.h), what
    for name, a, x in zip("pmv", s.read(), (p, m, v)):
        same_bits(f"{name} after the refused call", a, x)
    out2 = g.up(np.array([7.0, 7.0]), np.float64)
    rc = g.lib.ng_grad_clip_factor(g.h, g.st, n, g.ptr(s.t[1]), 1.0, *table(REFUSALS[what]), 1.0, g.ptr(out2))
    assert rc == NG_ERR_INVALID and out2.cpu().tolist() == [7.0, 7.0], what


def test_refusals_other_and_empty(gpu_device):
    """64 ranges are accepted; step 0 and a clipnorm that is not positive are refused; an armed replay context is refused
    with NG_ERR_UNSUPPORTED and nothing changes; n_seg = 0 and n = 0 succeed and change nothing"""
    g = Gpu(gpu_device)
    n = 300
    p, grad, m, v = data(n, 6)
    s = State(g, n, p, grad, m, v)
    segs64 = [(4 * i, 4 * i + 3, 1.0) for i in range(64)]
    want = State(g, n, p, grad, m, v).plain(*ARGS).read()
    got = State(g, n, p, grad, m, v).grouped(*ARGS, segs64).read()
    on = mask_of(n, segs64)
    for name, a, w, x in zip("pmv", got, want, (p, m, v)):
        same_bits(name, a, np.where(on, w, x))
    assert s.grouped_rc(*ARGS[:4], 0, [(0, n, 1.0)]) == NG_ERR_INVALID
    out2 = g.up(np.array([7.0, 7.0]), np.float64)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert g.lib.ng_grad_clip_factor(g.h, g.st, n, g.ptr(s.t[1]), 1.0, *table([(0, n, 1.0)]), bad,
                                         g.ptr(out2)) == NG_ERR_INVALID
    g.ok(g.lib.ng_replay_arm(g.h, 1), "ng_replay_arm")
    try:
        assert s.grouped_rc(*ARGS, [(0, n, 1.0)]) == NG_ERR_UNSUPPORTED
        assert b"replay" in g.lib.ng_last_error(g.h)
    finally:
        g.ok(g.lib.ng_replay_arm(g.h, 0), "ng_replay_arm")
    s.grouped(*ARGS, [])
    s.grouped(*ARGS, [(0, 0, 1.0), (300, 300, 2.0)])
    for name, a, x in zip("pmv", s.read(), (p, m, v)):
        same_bits(f"{name} after refused and empty calls", a, x)
    assert out2.cpu().tolist() == [7.0, 7.0]
    assert g.lib.ng_adam_step_groups(g.h, g.st, 0, None, None, None, None, *ARGS, 1.0, *table([]), None) == 0
    g.ok(g.lib.ng_grad_clip_factor(g.h, g.st, 0, None, 1.0, *table([]), 1.0, g.ptr(out2)), "ng_grad_clip_factor")
    assert out2.cpu().tolist() == [1.0, 0.0]
    g.torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- clip factor
def clip_factor(g, n, grad_dev, gscale, segs, clipnorm):
    out2 = g.up(np.array([np.nan, np.nan]), np.float64)
    g.ok(g.lib.ng_grad_clip_factor(g.h, g.st, n, g.ptr(grad_dev), gscale, *table(segs), clipnorm, g.ptr(out2)),
         "ng_grad_clip_factor")
    return out2


@pytest.mark.parametrize("n,layout", CASES)
def test_clip_factor(gpu_device, n, layout):
    g = Gpu(gpu_device)
    grad = data(n, 7)[1]
    segs = [(b, e, (1.0, 0.3)[i % 2]) for i, (b, e) in enumerate(layouts(n)[layout])]
    if layout == "three":
        segs[1] = (segs[1][0], segs[1][1], 0.0)        # the one-element segment is frozen: it does not count
        grad[130] = np.nan
    gd = g.up(np.concatenate([grad, np.full(GUARD, np.nan, np.float32)]))
    gscale = 0.37
    f_ref, norm_ref = FR.clip_ref(grad, gscale, segs, 1e-3)
    a = clip_factor(g, n, gd, gscale, segs, 1e-3).cpu().numpy()
    b = clip_factor(g, n, gd, gscale, segs, 1e-3).cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "two runs differ"
    rel = n * 2.0 ** -53
    assert abs(a[1] - norm_ref) <= rel * norm_ref, (a[1], norm_ref)
    assert norm_ref > 1e-3 and abs(a[0] - f_ref) <= 2 * rel * f_ref and a[0] < 1.0
    # below the threshold: exactly 1, the norm as before
    c = clip_factor(g, n, gd, gscale, segs, 1e6).cpu().numpy()
    assert c[0] == 1.0 and c[1] == a[1]


def test_clip_factor_exact_and_edges(gpu_device):
    """3-4-5: norm and factor exact; a zero gradient and a NaN or inf gradient give factor 1 (norm 0, NaN, inf)"""
    g = Gpu(gpu_device)
    n = 257
    grad = np.zeros(n, np.float32)
    grad[3], grad[200] = 6.0, 8.0
    segs = [(0, 131, 1.0), (133, n, 2.0)]
    assert clip_factor(g, n, g.up(grad), 0.5, segs, 2.5).cpu().tolist() == [0.5, 5.0]
    assert clip_factor(g, n, g.up(grad), 0.5, segs, 5.0).cpu().tolist() == [1.0, 5.0]
    assert clip_factor(g, n, g.up(np.zeros(n)), 1.0, segs, 1.0).cpu().tolist() == [1.0, 0.0]
    for bad in (np.nan, np.inf):
        grad[50] = bad
        f, norm = clip_factor(g, n, g.up(grad), 1.0, segs, 1.0).cpu().tolist()
        assert f == 1.0 and (np.isnan(norm) if np.isnan(bad) else norm == np.inf)
    grad[50] = 0.0
    grad[132] = np.nan            # in no segment: not read
    assert clip_factor(g, n, g.up(grad), 0.5, segs, 2.5).cpu().tolist() == [0.5, 5.0]


@pytest.mark.parametrize("n", [257, NBIG])
def test_adam_with_clip(gpu_device, n):
    """clip[0] = 1: the bits of clip = NULL; clip[0] = 0.25 with grad_scale s: the bits of unclipped Adam at 0.25 s; and the
    factor ng_grad_clip_factor wrote is the one Adam applies (a gradient of norm 4 x clipnorm in exact numbers)"""
    g = Gpu(gpu_device)
    p, grad, m, v = data(n, 8)
    segs = [(0, 101, 1.0), (130, 131, 0.3), (133, n, 0.5)]
    s = 3.7
    plain = State(g, n, p, grad, m, v).grouped(*ARGS, segs, gscale=s).read()
    one = State(g, n, p, grad, m, v).grouped(*ARGS, segs, gscale=s, clip=g.up(np.array([1.0, 0.0]), np.float64)).read()
    for name, a, w in zip("pmv", one, plain):
        same_bits(f"{name} (clip 1)", a, w)
    quarter = State(g, n, p, grad, m, v).grouped(*ARGS, segs, gscale=s, clip=g.up(np.array([0.25, 0.0]), np.float64)).read()
    want = State(g, n, p, grad, m, v).grouped(*ARGS, segs, gscale=float(np.float32(s) * np.float32(0.25))).read()
    assert (bits(want[0]) != bits(plain[0])).any()
    for name, a, w in zip("pmv", quarter, want):
        same_bits(f"{name} (clip 1/4)", a, w)
    # end to end: |g| = 4 on one element of each live segment ... norm = sqrt(3) * 4 is not exact, so use two: 3-4-5 scaled
    grad2 = np.zeros(n, np.float32)
    grad2[5], grad2[140] = 12.0, 16.0                  # norm 20 = 4 x clipnorm 5: factor exactly 1/4
    st = State(g, n, p, grad2, m, v)
    out2 = clip_factor(g, n, st.t[1], 1.0, segs, 5.0)
    assert out2.cpu().tolist() == [0.25, 20.0]
    got = st.grouped(*ARGS, segs, clip=out2).read()
    want = State(g, n, p, grad2, m, v).grouped(*ARGS, segs, gscale=0.25).read()
    for name, a, w in zip("pmv", got, want):
        same_bits(f"{name} (measured factor)", a, w)
