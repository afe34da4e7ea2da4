"""ng_class_moments (csrc/class_moments.hip) through the C entry point, against tests/class_moments_ref.py.

An exact family (y and p multiples of 1/4 below 512: every term and every sum is a multiple of 1/16 that float64 holds exactly,
so any order of summation gives the same number) is compared element by element; a float family of realistic shifts is held
to the bound of a float64 summation in any order.  ``moments`` sits between guard rows, every call is made twice for the bitwise
check, and every refusal must leave output and guards alone."""

import numpy as np
import pytest
import torch

import class_moments_ref as R

pytestmark = pytest.mark.gpu

TILE = 256                 # atoms per tile
CAP = 512                  # stage-1 workgroups at most (CM_MAX_BLOCKS): beyond CAP tiles a workgroup takes a second tile
SECOND_TILE = CAP * TILE + 1
GUARD = -6.02e23
STALE = 4242.5             # what `moments` holds before an overwriting call
NG_ERR_INVALID = -1


class _Lib:
    def __init__(self, dev):
        from nmrgnn_amd import _lib
        self.ctx = _lib.get_context(dev.index)
        self.dev = dev

    def raw(self, N, y, w, names, pred, n_ids, M, class_of, K, accumulate, moments, handle=True):
        from nmrgnn_amd._lib import ptr, _vp
        st = torch.cuda.current_stream(self.dev).cuda_stream
        return self.ctx.lib.ng_class_moments(self.ctx.handle if handle else None, _vp(st), N, ptr(y), ptr(w), ptr(names),
                                             ptr(pred), n_ids, M, ptr(class_of), K, accumulate, ptr(moments))

    def error(self):
        return (self.ctx.lib.ng_last_error(self.ctx.handle) or b'').decode()


def _dev(x, dev, dt):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dt).contiguous()


def _run(L, y, w, names, pred, class_of, K, accumulate=0, start=None):
    """one checked call, made twice: the [K][7] result; guards intact, both calls the same bits"""
    dev = L.dev
    class_of = np.asarray(class_of, np.int32).reshape(len(class_of), -1)
    M, n_ids = class_of.shape
    args = (_dev(y, dev, torch.float32), _dev(w, dev, torch.float32), _dev(names, dev, torch.int32),
            _dev(pred, dev, torch.float32))
    table = _dev(class_of, dev, torch.int32) if n_ids else None
    outs = []
    for _ in range(2):
        buf = torch.full((K + 2, 7), GUARD, dtype=torch.float64, device=dev)
        buf[1:K + 1] = torch.as_tensor(start, dtype=torch.float64) if start is not None else STALE
        rc = L.raw(len(y), *args, n_ids, M, table, K, accumulate, buf[1:])
        assert rc == 0, L.error()
        out = buf.cpu().numpy()
        assert (out[0] == GUARD).all() and (out[-1] == GUARD).all()
        outs.append(out[1:-1])
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def _quarters(rng, n):
    return rng.integers(0, 2048, n).astype(np.float32) / 4          # multiples of 1/4 below 512


def _table(K, M, n_extra=3):
    """[M][K + n_extra]: grouping m maps id < K to row (id + 17 m) mod K; the ids behind K are in no class"""
    ids = np.arange(K + n_extra)
    return np.stack([np.where(ids < K, (ids + 17 * m) % K, -1) for m in range(M)]).astype(np.int32)


def _exact(L, N, K, M, names, w=None, seed=0, class_of=None):
    rng = np.random.default_rng([seed, N, K, M])
    y, p = _quarters(rng, N), _quarters(rng, N)
    if w is None:                                                      # most atoms of a real record carry no label
        w = rng.choice(np.array([0.0, 1.0, 0.5, 2.0], np.float32), N, p=[0.6, 0.2, 0.1, 0.1] if N > 4096 else [0.1, 0.5, 0.2, 0.2])
    class_of = _table(K, M) if class_of is None else class_of
    want, _, counts = R.class_moments_ref(y, w, names, p, class_of, K)
    got = _run(L, y, w, names, p, class_of, K)
    np.testing.assert_array_equal(got, want)
    return got, counts


N_SHAPES = [0, 1, 255, 256, 257, SECOND_TILE]
K_SHAPES = [1, 255, 256, 257, 1024]


@pytest.mark.parametrize("N", N_SHAPES)
@pytest.mark.parametrize("K", K_SHAPES)
def test_exact_shapes(gpu_device, N, K):
    """every N with every K; M runs through 1..4 along both axes, ids at random (some outside the table)"""
    M = 1 + (N_SHAPES.index(N) + K_SHAPES.index(K)) % 4
    rng = np.random.default_rng([N, K])
    names = rng.integers(-1, K + 4, N).astype(np.int32)
    _exact(_Lib(gpu_device), N, K, M, names)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_exact_groupings(gpu_device, M):
    """M = 1..4 at one shape with more than one tile and a thread's second class; an atom adds once per grouping"""
    N, K = 3 * TILE + 5, 257
    names = (np.arange(N) % (K + 2)).astype(np.int32)
    got, counts = _exact(_Lib(gpu_device), N, K, M, names, w=np.ones(N, np.float32))
    assert counts.sum() == M * int((names < K).sum()) and got[:, 0].sum() == counts.sum()


@pytest.mark.parametrize("pattern,N,K", [
    ("one", SECOND_TILE, 1), ("one", 5 * TILE + 1, 1024), ("own", 257, 257), ("own", 1024, 1024),
    ("tile", 7 * TILE + 3, 8), ("tile", 300 * TILE, 300), ("spread", 5 * TILE + 9, 255), ("spread", SECOND_TILE, 120)])
def test_exact_placements(gpu_device, pattern, N, K):
    i = np.arange(N)
    names = {"one": np.full(N, K - 1), "own": i, "tile": i // TILE, "spread": i % K}[pattern].astype(np.int32)
    w = np.ones(N, np.float32) if N <= 4096 or pattern == "one" else None
    got, counts = _exact(_Lib(gpu_device), N, K, 1, names, w=w)
    if pattern == "one":
        assert counts[K - 1] == N and got[K - 1, 0] == N and (got[:K - 1] == 0).all()
    if pattern == "own":
        assert (got[:, 0] == 1).all()


def test_exact_accumulate(gpu_device):
    L = _Lib(gpu_device)
    N, K, M = 2 * TILE + 7, 40, 3
    rng = np.random.default_rng(5)
    class_of = _table(K, M)
    first = None
    for accumulate in (0, 1, 1):
        y, p = _quarters(rng, N), _quarters(rng, N)
        names = rng.integers(0, K + 3, N).astype(np.int32)
        w = np.ones(N, np.float32)
        want, _, _ = R.class_moments_ref(y, w, names, p, class_of, K, start=first if accumulate else None)
        first = _run(L, y, w, names, p, class_of, K, accumulate=accumulate, start=first)
        np.testing.assert_array_equal(first, want)
    # N == 0: zeros when overwriting, nothing added when accumulating
    e = np.zeros(0, np.float32)
    assert (_run(L, e, e, e.astype(np.int32), e, class_of, K) == 0).all()
    np.testing.assert_array_equal(_run(L, e, e, e.astype(np.int32), e, class_of, K, accumulate=1, start=first), first)


def test_exact_weights_count_once(gpu_device):
    """w of 0, -0.0, -1 and NaN do not count; 0.5 and 2 count ONCE each"""
    w = np.array([0.0, -0.0, -1.0, np.nan, 0.5, 2.0], np.float32)
    y = np.array([1, 2, 3, 4, 5.25, 7.5], np.float32)
    p = np.array([9, 9, 9, 9, 6.0, 7.0], np.float32)
    got = _run(_Lib(gpu_device), y, w, np.zeros(6, np.int32), p, [[1]], 3)
    want, _, counts = R.class_moments_ref(y, w, np.zeros(6, np.int32), p, [[1]], 3)
    np.testing.assert_array_equal(got, want)
    assert counts.tolist() == [0, 2, 0]
    np.testing.assert_array_equal(got[1], [2, 0.75 ** 2 + 0.25, 12.75, 13.0, 5.25 ** 2 + 7.5 ** 2, 85.0, 5.25 * 6 + 7.5 * 7])


def test_exact_ids_and_table_values_outside(gpu_device):
    """ids of -1, n_ids and 2^24 are in no class; table values of -1, -7, K and 2^30 are no class and never an index"""
    L = _Lib(gpu_device)
    K, n_ids = 5, 6
    class_of = np.array([[0, -1, -7, K, 1 << 30, 4], [4, 4, 4, 4, 4, -1]], np.int32)
    names = np.array([-1, n_ids, 1 << 24, 0, 1, 2, 3, 4, 5, -2147483648, 2147483647], np.int32)
    N = len(names)
    rng = np.random.default_rng(9)
    y, p, w = _quarters(rng, N), _quarters(rng, N), np.ones(N, np.float32)
    got = _run(L, y, w, names, p, class_of, K)
    want, _, counts = R.class_moments_ref(y, w, names, p, class_of, K)
    np.testing.assert_array_equal(got, want)
    assert counts.tolist() == [1, 0, 0, 0, 6]            # row 0: id 0; row 4: id 5 by grouping 0, ids 0..4 by grouping 1
    # n_ids == 0: no table at all (NULL), every atom is in no class
    assert (_run(L, y, w, names, p, np.zeros((2, 0), np.int32), K) == 0).all()


@pytest.mark.parametrize("N,K,M", [(257, 7, 1), (1000, 13, 3), (SECOND_TILE, 120, 3), (3 * TILE, 1024, 4)])
def test_float_family(gpu_device, N, K, M):
    """shifts like real ones (H near 8, N near 120), predictions = label + noise:
    |S - S_ref| <= n_c 2^-52 sum |term| for every sum of every class"""
    rng = np.random.default_rng([N, K, M])
    centre = np.where(rng.random(N) < 0.5, 8.0, 120.0)
    y = (centre + np.where(centre < 50, 1.0, 5.0) * rng.standard_normal(N)).astype(np.float32)
    p = (y + 0.4 * rng.standard_normal(N)).astype(np.float32)
    w = (rng.random(N) < (0.3 if N > 4096 else 0.8)).astype(np.float32)
    names = rng.integers(0, K + 3, N).astype(np.int32)
    class_of = _table(K, M)
    want, abs_sums, counts = R.class_moments_ref(y, w, names, p, class_of, K)
    got = _run(_Lib(gpu_device), y, w, names, p, class_of, K)
    err, bound = np.abs(got - want), R.float_bound(abs_sums, counts)
    print(f"N={N} K={K} M={M}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}, counts up to {counts.max()}")
    assert (got[:, 0] == counts).all()
    assert (err <= bound).all(), (err - bound).max()


def test_refusals_leave_everything_alone(gpu_device):
    L = _Lib(gpu_device)
    dev = gpu_device
    N, K, M, n_ids = 300, 9, 2, 12
    y = torch.ones(N, device=dev)
    names = torch.zeros(N, dtype=torch.int32, device=dev)
    table = torch.zeros(M, n_ids, dtype=torch.int32, device=dev)
    buf = torch.full((K + 2, 7), GUARD, dtype=torch.float64, device=dev)
    buf[1:K + 1] = STALE
    before = buf.cpu().numpy()
    out = buf[1:]
    good = dict(N=N, y=y, w=y, names=names, pred=y, n_ids=n_ids, M=M, class_of=table, K=K, accumulate=0, moments=out)
    bad = [dict(handle=False), dict(moments=None), dict(y=None), dict(w=None), dict(names=None), dict(pred=None),
           dict(class_of=None), dict(class_of=None, N=0), dict(M=0), dict(M=5), dict(K=0), dict(K=1025), dict(n_ids=-1),
           dict(n_ids=(1 << 24) + 1), dict(N=-1), dict(N=(1 << 31) - 256), dict(accumulate=2), dict(accumulate=-1)]
    for change in bad:
        a = dict(good, **change)
        handle = a.pop('handle', True)
        rc = L.raw(a['N'], a['y'], a['w'], a['names'], a['pred'], a['n_ids'], a['M'], a['class_of'], a['K'], a['accumulate'],
                   a['moments'], handle=handle)
        assert rc == NG_ERR_INVALID, change
        if handle:
            assert L.error().startswith("class moments: "), (change, L.error())
    torch.cuda.synchronize(dev)
    np.testing.assert_array_equal(buf.cpu().numpy(), before)
    # the limits themselves are accepted: N == 0 without inputs, n_ids == 0 without a table
    assert L.raw(0, None, None, None, None, n_ids, M, table, K, 1, out) == 0, L.error()
    assert L.raw(N, y, y, names, y, 0, M, None, K, 1, out) == 0, L.error()
    np.testing.assert_array_equal(buf.cpu().numpy(), before)          # both added nothing
    # and the context still works: one good call
    assert L.raw(**{k: good[k] for k in good}) == 0, L.error()
    got = buf.cpu().numpy()
    assert (got[0] == GUARD).all() and (got[-1] == GUARD).all()
    want = np.zeros((K, 7))
    want[0] = [2 * N, 0, 2 * N, 2 * N, 2 * N, 2 * N, 2 * N]            # both groupings map id 0 to row 0: every atom adds twice
    np.testing.assert_array_equal(got[1:-1], want)
