"""csrc/records.hip on the GPU: ``ng_store_from_batch`` and ``ng_label_moments`` through the C entry points
against tests/records_ref.py, bit for bit, then ``ShiftDataset.from_structures`` / ``standards()`` end to end.

Launch arithmetic restated (csrc/records.hip): ``ng_store_from_batch`` gives a workgroup of 256 threads a tile of RC_TILE = 256
batch rows per trip; grid = min(ceil(N / 256), RC_MAX_BLOCKS = 1024) workgroups stride over the tiles, so N > 262144 rows
gives some workgroup a second trip.  Every row finds its structure by binary search over the G + 1 boundaries.  List rows move
in 16-byte chunks when K % 4 == 0 and the four list arrays are 16-byte aligned (K = 16 here), word by word otherwise (K = 1,
3); the atom rows of a tile are one flat run moved in 16-byte chunks when b_atoms and s_atoms + row0 * C are 16-byte aligned
(any C at row0 = 0; C = 10 at an even row0), in 8-byte chunks when both are 8-byte aligned (C = 10 at an odd row0), word by word
otherwise (C = 1 at an odd row0), the run's last words one by one (255 and 257 rows of C = 1 or 10 leave some).
``ng_label_moments``: workgroup b of min(Rv, 256) takes the records ids[b], ids[b + nb], ... in 256-row tiles (1025 records:
a fifth trip for workgroup 0; a 600-row record: three tiles); 256 / C thread groups share a tile's rows when C <= 256."""
import ctypes as C
import os

import numpy as np
import pytest

import records_ref as RR

pytestmark = pytest.mark.gpu

RC_TILE, RC_MAX_BLOCKS = 256, 1024
GUARD = 4                     # guard rows before and after every store array: 4 rows keep the interior 16-byte aligned
I_SENT = -7777777
KEYS = ("atoms", "nlist", "edges", "inv_degree", "y", "w")
NG_ERR_INVALID = -1
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
PDB1, PDB10 = os.path.join(DATA, "108M.pdb"), os.path.join(DATA, "7lgi.pdb.gz")


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _make_batch(sizes, K, Cc, seed):
    """a ragged batch on the host: batch-global neighbours of the row's own structure; edges > 0 on most slots, +0.0, -0.0 and
    NaN on the rest; shifts finite, NaN, +inf and -inf; name ids up to 2^24 - 1"""
    rng = np.random.default_rng(seed)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N = int(gp[-1])
    g = np.searchsorted(gp, np.arange(N), side="right") - 1
    off, n = gp[g].astype(np.int64), (gp[g + 1] - gp[g]).astype(np.int64)
    nlist = (off[:, None] + rng.integers(0, n[:, None], size=(N, K))).astype(np.int32)
    edges = rng.uniform(0.09, 0.45, size=(N, K)).astype(np.float32)
    kind = rng.integers(0, 10, size=(N, K))
    edges[kind == 0] = 0.0
    edges[kind == 1] = -0.0
    edges[kind == 2] = np.nan
    atoms = rng.standard_normal((N, Cc)).astype(np.float32)
    shift = rng.normal(60.0, 50.0, N).astype(np.float32)
    what = rng.integers(0, 8, size=N)
    shift[what == 0] = np.nan
    shift[what == 1] = np.inf
    shift[what == 2] = -np.inf
    name_id = rng.integers(0, 2 ** 24, size=N).astype(np.int32)
    name_id[rng.integers(0, N)] = 2 ** 24 - 1
    return dict(gp=gp, atoms=atoms, nlist=nlist, edges=edges, shift=shift, name_id=name_id, N=N, G=len(sizes))


def _store_buffers(Ncap, K, Cc, dev):
    """{name: (whole buffer with guard rows, the Ncap store rows)} filled with NaN / the integer sentinel"""
    import torch
    tails = {"atoms": (Cc,), "nlist": (K,), "edges": (K,), "inv_degree": (), "y": (3,), "w": ()}
    out = {}
    for k, tail in tails.items():
        integer = k == "nlist"
        whole = torch.full((Ncap + 2 * GUARD,) + tail, I_SENT if integer else float("nan"),
                           dtype=torch.int32 if integer else torch.float32, device=dev)
        out[k] = (whole, whole[GUARD:GUARD + Ncap])
    return out


def _call_store(ctx, b, K, Cc, row0, Ncap, st, counters, **over):
    import torch
    from nmrgnn_amd._lib import ptr
    a = dict(N=b["N"], K=K, C=Cc, G=b["G"], gp=ptr(b["gp"]), atoms=ptr(b["atoms"]), nlist=ptr(b["nlist"]), edges=ptr(b["edges"]),
             shift=ptr(b["shift"]), name_id=ptr(b["name_id"]), row0=row0, Ncap=Ncap, s_atoms=ptr(st["atoms"][1]),
             s_nlist=ptr(st["nlist"][1]), s_edges=ptr(st["edges"][1]), s_inv=ptr(st["inv_degree"][1]), s_y=ptr(st["y"][1]),
             s_w=ptr(st["w"][1]), counters=ptr(counters))
    a.update(over)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return ctx.lib.ng_store_from_batch(ctx.handle, s, *a.values())


def _to_dev(host, dev):
    import torch
    return {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in host.items()}


def _check_store(st, ref, row0, N, Ncap):
    """rows [row0, row0 + N) == reference bit for bit; every other store row and the guard rows still hold the fill"""
    import torch
    dev = st["atoms"][0].device
    for k in KEYS:
        whole, rows = st[k]
        want = torch.from_numpy(np.ascontiguousarray(ref[k])).to(dev)
        got = rows[row0:row0 + N]
        assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), k
        assert torch.equal(_bits(got), _bits(want)), f"{k} differs from the reference"
        for rest in (whole[:GUARD + row0], whole[GUARD + row0 + N:]):
            assert bool((rest == I_SENT).all() if k == "nlist" else torch.isnan(rest).all()), f"{k}: rows outside the call were written"


def _run_store(dev, sizes, K, Cc, row0, seed=0, tail=5, host=None):
    """two calls into separate stores with ONE pair of counters (which must add); returns (N, counters of the reference)"""
    import torch
    from nmrgnn_amd import _lib
    ctx = _lib.get_context(dev.index)
    host = _make_batch(sizes, K, Cc, seed) if host is None else host
    ref = RR.store_from_batch_ref(host["gp"], host["atoms"], host["nlist"], host["edges"], host["shift"], host["name_id"])
    b = _to_dev(host, dev)
    N, Ncap = host["N"], row0 + host["N"] + tail
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    first, second = _store_buffers(Ncap, K, Cc, dev), _store_buffers(Ncap, K, Cc, dev)
    for st in (first, second):
        rc = _call_store(ctx, b, K, Cc, row0, Ncap, st, counters)
        assert rc == 0, ctx.lib.ng_last_error(ctx.handle)
    torch.cuda.synchronize(dev)
    _check_store(first, ref, row0, N, Ncap)
    for k in KEYS:            # the second call's bits are the first's, guards and all
        assert torch.equal(_bits(first[k][0]), _bits(second[k][0])), k
    assert counters.cpu().tolist() == (2 * ref["counters"]).tolist()       # added to, never reset
    return N, ref["counters"]


SIZES = [255, 256, 257, 1, 2, 17, 1, 300]


@pytest.mark.parametrize("row0", [0, 3])
@pytest.mark.parametrize("Cc", [1, 10])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_store_from_batch_widths_and_alignment(gpu_device, K, Cc, row0):
    N, cnt = _run_store(gpu_device, SIZES, K, Cc, row0, seed=10 * K + Cc)
    assert N == sum(SIZES) and cnt[0] == 0 and 0 < cnt[1] < N


@pytest.mark.parametrize("n", [255, 256, 257])
def test_store_from_batch_one_structure_around_a_tile(gpu_device, n):
    _run_store(gpu_device, [n], 16, 10, 1, seed=n)            # G = 1, odd row0


def test_store_from_batch_513_one_atom_structures(gpu_device):
    host = _make_batch([1] * 513, 16, 10, seed=4)
    N, cnt = _run_store(gpu_device, None, 16, 10, 0, host=host)
    assert N == 513 and cnt[0] == 0                            # every live slot points at the atom itself: local index 0


def test_store_from_batch_past_the_grid_cap(gpu_device):
    N, _ = _run_store(gpu_device, [300] * 873 + [245], 16, 10, 2, seed=6)
    assert N == RC_TILE * RC_MAX_BLOCKS + 1 and -(-N // RC_TILE) == RC_MAX_BLOCKS + 1


def test_store_from_batch_slot_outside_its_structure(gpu_device):
    """one live slot of structure 1 points at the last atom of structure 0, one of structure 0 one past its end (the first atom
    of structure 1): each call counts 2, the slots hold (0, +0.0), every other word is the reference's"""
    host = _make_batch([40, 30, 50], 16, 10, seed=8)
    host["nlist"][45, 3], host["edges"][45, 3] = 39, 0.25
    host["nlist"][7, 0], host["edges"][7, 0] = 40, 0.125
    host["nlist"][100, 5], host["edges"][100, 5] = 0, 0.0       # a dead slot pointing outside is padding, not an error
    ref = RR.store_from_batch_ref(host["gp"], host["atoms"], host["nlist"], host["edges"], host["shift"], host["name_id"])
    assert ref["counters"][0] == 2 and ref["nlist"][45, 3] == 0 and ref["edges"][7, 0] == 0
    _, cnt = _run_store(gpu_device, None, 16, 10, 0, host=host)
    assert cnt[0] == 2
    one = _make_batch([40, 30, 50], 16, 10, seed=8)
    one["nlist"][45, 3], one["edges"][45, 3] = 39, 0.25
    _, cnt = _run_store(gpu_device, None, 16, 10, 0, host=one)
    assert cnt[0] == 1


def test_store_from_batch_labels(gpu_device):
    """NaN, +inf and -inf shifts are rows without a label; name id 2^24 - 1 survives the float"""
    import torch
    from nmrgnn_amd import _lib
    dev = gpu_device
    host = _make_batch([6], 3, 2, seed=1)
    host["shift"][:] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 3.5]
    host["name_id"][:] = [2 ** 24 - 1, 1, 2, 3, 4, 0]
    ctx = _lib.get_context(dev.index)
    st = _store_buffers(6, 3, 2, dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    assert _call_store(ctx, _to_dev(host, dev), 3, 2, 0, 6, st, counters) == 0
    y, w = st["y"][1].cpu().numpy(), st["w"][1].cpu().numpy()
    assert w.tolist() == [0, 0, 0, 1, 1, 1] and y[:, 2].tolist() == w.tolist()
    assert np.array_equal(y[:, 0].view(np.int32), np.array([0, 0, 0, 0, -0.0, 3.5], np.float32).view(np.int32))
    assert y[:, 1].tolist() == [float(2 ** 24 - 1), 1, 2, 3, 4, 0] and int(y[0, 1]) == 2 ** 24 - 1
    assert counters.cpu().tolist() == [RR.store_from_batch_ref(host["gp"], host["atoms"], host["nlist"], host["edges"],
                                                                host["shift"], host["name_id"])["counters"][0], 3]


def test_store_from_batch_refusals_and_empty_batch(gpu_device):
    import torch
    from nmrgnn_amd import _lib
    dev, K, Cc = gpu_device, 16, 10
    ctx = _lib.get_context(dev.index)
    host = _make_batch([2, 1], K, Cc, seed=2)
    b = _to_dev(host, dev)
    Ncap = 8
    st = _store_buffers(Ncap, K, Cc, dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    from nmrgnn_amd._lib import ptr
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(N=3, K=K, C=Cc, G=2, gp=ptr(b["gp"]), atoms=ptr(b["atoms"]), nlist=ptr(b["nlist"]), edges=ptr(b["edges"]),
                shift=ptr(b["shift"]), name_id=ptr(b["name_id"]), row0=2, Ncap=Ncap, s_atoms=ptr(st["atoms"][1]),
                s_nlist=ptr(st["nlist"][1]), s_edges=ptr(st["edges"][1]), s_inv=ptr(st["inv_degree"][1]), s_y=ptr(st["y"][1]),
                s_w=ptr(st["w"][1]), counters=ptr(counters))

    def call(handle=ctx.handle, **over):
        a = dict(base)
        a.update(over)
        return ctx.lib.ng_store_from_batch(handle, s, *a.values())

    assert call(handle=None) == NG_ERR_INVALID                                  # NULL context
    bad = [dict(K=0), dict(K=4097), dict(C=0), dict(C=4097), dict(K=-1), dict(N=-1), dict(N=2 ** 31 - 256), dict(N=2 ** 31),
           dict(G=0), dict(G=4), dict(row0=-1), dict(row0=6), dict(Ncap=4), dict(row0=2 ** 62, Ncap=2 ** 62 + 1)]
    bad += [{k: None} for k in base if isinstance(base[k], C.c_void_p)]
    assert len(bad) == 14 + 13
    for over in bad:
        assert call(**over) == NG_ERR_INVALID, over
        assert ctx.lib.ng_last_error(ctx.handle)
    assert call(N=0, G=0) == 0                                                   # N == 0: OK, nothing launched
    assert call(N=0, G=0, atoms=None, s_y=None, counters=None, gp=None) == 0
    torch.cuda.synchronize(dev)
    for k in KEYS:                              # every refusal and the empty batch left the store as it was
        whole = st[k][0]
        assert bool((whole == I_SENT).all() if k == "nlist" else torch.isnan(whole).all()), k
    assert counters.cpu().tolist() == [0, 0]
    assert call() == 0                          # and the same arguments unchanged do run
    torch.cuda.synchronize(dev)
    ref = RR.store_from_batch_ref(host["gp"], host["atoms"], host["nlist"], host["edges"], host["shift"], host["name_id"])
    _check_store(st, ref, 2, 3, Ncap)
    assert call(row0=5) == 0                    # the last rows of the store: row0 + N == Ncap
    torch.cuda.synchronize(dev)
    for k in KEYS:
        assert torch.equal(_bits(st[k][1][5:8]), _bits(st[k][1][2:5])), k
        assert bool((st[k][0][GUARD + Ncap:] == I_SENT).all() if k == "nlist" else torch.isnan(st[k][0][GUARD + Ncap:]).all()), k


# ---------------------------------------------------------------------------------------------- ng_label_moments
def _moments_store(sizes, Cc, seed, exact, labelled=0.7, empty_rows=0.1):
    """host arrays of a store: one-hot atom rows (scaled, so 'non-zero' is not '== 1'; some rows all zero), y0 either
    multiples of 2^-8 with |y0| < 2^8 (exact) or normal around 100"""
    rng = np.random.default_rng(seed)
    rec_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(rec_ptr[-1])
    atoms = np.zeros((n, Cc), np.float32)
    atoms[np.arange(n), rng.integers(0, Cc, n)] = rng.choice([1.0, -2.0, 0.5], n)
    second = rng.random(n) < 0.2                  # a later non-zero column as well: the FIRST one names the element
    atoms[second, Cc - 1] = 1.0
    atoms[rng.random(n) < empty_rows] = 0.0
    if exact:
        y0 = (rng.integers(-2 ** 16 + 1, 2 ** 16, n) / 256.0).astype(np.float32)
    else:
        y0 = rng.normal(100.0, 30.0, n).astype(np.float32)
    mask = (rng.random(n) < labelled).astype(np.float32)
    y = np.stack([y0, rng.integers(0, 50, n).astype(np.float32), mask], axis=1).astype(np.float32)
    return atoms, y, rec_ptr


def _moments(dev, atoms, y, rec_ptr, ids, Cc, R=None, **over):
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    ctx = _lib.get_context(dev.index)
    t = dict(atoms=torch.from_numpy(atoms).to(dev), y=torch.from_numpy(y).to(dev), rec_ptr=torch.from_numpy(rec_ptr).to(dev),
             ids=torch.tensor(list(ids), dtype=torch.int32, device=dev))
    outs = []
    for _ in range(2):
        whole = torch.full((Cc + 2, 3), float("nan"), dtype=torch.float64, device=dev)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = ctx.lib.ng_label_moments(ctx.handle, s, len(rec_ptr) - 1 if R is None else R, int(rec_ptr[-1]), Cc, ptr(t["atoms"]),
                                      ptr(t["y"]), ptr(t["rec_ptr"]), ptr(t["ids"]), len(t["ids"]), ptr(whole[1:Cc + 1]))
        assert rc == 0, ctx.lib.ng_last_error(ctx.handle)
        outs.append(whole)
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(outs[0][0]).all()) and bool(torch.isnan(outs[0][Cc + 1]).all())     # guard rows
    assert torch.equal(outs[0][1:Cc + 1].view(torch.int64), outs[1][1:Cc + 1].view(torch.int64))  # two runs, the same bits
    return outs[0][1:Cc + 1].cpu().numpy()


MOMENT_CASES = {
    "c10": (10, [30, 1, 255, 256, 257, 600, 2, 64], None),
    "c1": (1, [5, 300, 40], None),
    "c3_view": (3, [20, 30, 40, 50, 60, 70], [4, 1, 5]),
    "c10_repeats_and_ids_outside": (10, [40, 50, 60], [2, 3, -1, 0, 2, 100, 1]),
    "c300": (300, [10, 400, 3], None),
    "r1025": (10, [3] * 1000 + [1, 2, 7, 300, 5] * 5, None),
}


@pytest.mark.parametrize("name", list(MOMENT_CASES))
def test_label_moments_exact_family(gpu_device, name):
    """labels are multiples of 2^-8 with |y| < 2^8: a term of sum y^2 has 32 significant bits at most, so every partial sum of
    up to 2^20 terms fits the 53 bits of a float64 and the result does not depend on the order: equal to NumPy bit for bit"""
    Cc, sizes, ids = MOMENT_CASES[name]
    atoms, y, rec_ptr = _moments_store(sizes, Cc, seed=len(sizes), exact=True)
    assert rec_ptr[-1] < 2 ** 20
    ids = list(range(len(sizes))) if ids is None else ids
    got = _moments(gpu_device, atoms, y, rec_ptr, ids, Cc)
    want = RR.label_moments_ref(atoms, y, rec_ptr, ids)
    assert want[:, 0].sum() > 0
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("name", ["c10", "c3_view", "r1025"])
def test_label_moments_general_family(gpu_device, name):
    """any float32 labels: each moment within n * 2^-53 * sum |term| of the sum, the float64 summation bound for n terms in any
    order ((n - 1) u sum |term| to first order, u = 2^-53).  The terms are exact in float64 (a float32, or the 48-bit product
    of two), and the reference here is ``math.fsum`` of them, the correctly rounded sum (within u |sum| of it: the one u that
    n has over n - 1); the count is exact"""
    import math
    Cc, sizes, ids = MOMENT_CASES[name]
    atoms, y, rec_ptr = _moments_store(sizes, Cc, seed=77, exact=False)
    ids = list(range(len(sizes))) if ids is None else ids
    got = _moments(gpu_device, atoms, y, rec_ptr, ids, Cc)
    rows = np.concatenate([np.arange(rec_ptr[i], rec_ptr[i + 1]) for i in ids])
    nz = atoms[rows] != 0
    use = (y[rows, 2] > 0) & nz.any(axis=1)
    el, y0 = np.argmax(nz, axis=1)[use], y[rows, 0][use].astype(np.float64)
    for c in range(Cc):
        t1 = y0[el == c]
        n = len(t1)
        assert got[c, 0] == n
        for j, terms in ((1, t1), (2, t1 * t1)):
            want, bound = math.fsum(terms), n * 2.0 ** -53 * math.fsum(np.abs(terms))
            err = abs(got[c, j] - want)
            print(name, "element", c, "moment", j, "n", n, "err", err, "bound", bound)
            assert err <= bound, (c, j, err, bound)
    assert np.allclose(got, RR.label_moments_ref(atoms, y, rec_ptr, ids), rtol=1e-12, atol=0)


def test_label_moments_nothing_to_count(gpu_device):
    atoms, y, rec_ptr = _moments_store([40, 300], 10, seed=3, exact=True)
    unl = y.copy()
    unl[:, 2] = 0.0
    assert not _moments(gpu_device, atoms, unl, rec_ptr, [0, 1], 10).any()            # all rows unlabelled
    unl[:, 2] = -1.0
    assert not _moments(gpu_device, atoms, unl, rec_ptr, [0, 1], 10).any()            # y2 > 0 is the test, not y2 != 0
    assert not _moments(gpu_device, np.zeros_like(atoms), y, rec_ptr, [0, 1], 10).any()   # no row has an element
    assert not _moments(gpu_device, atoms, y, rec_ptr, [], 10).any()                  # Rv == 0 writes zeros
    assert not _moments(gpu_device, atoms, y, rec_ptr, [2, -5, 2 ** 31 - 1], 10).any()    # only ids outside the store
    # R smaller than the store's: the ids at or past it are skipped
    got = _moments(gpu_device, atoms, y, rec_ptr, [0, 1], 10, R=1)
    assert np.array_equal(got, RR.label_moments_ref(atoms, y, rec_ptr[:2], [0]))


def test_label_moments_refusals(gpu_device):
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    dev = gpu_device
    ctx = _lib.get_context(dev.index)
    atoms, y, rec_ptr = _moments_store([4, 5], 10, seed=3, exact=True)
    t = [torch.from_numpy(a).to(dev) for a in (atoms, y, rec_ptr)] + [torch.tensor([0, 1], dtype=torch.int32, device=dev)]
    out = torch.full((10, 3), float("nan"), dtype=torch.float64, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(R=2, Ntot=9, C=10, atoms=ptr(t[0]), y=ptr(t[1]), rec_ptr=ptr(t[2]), ids=ptr(t[3]), Rv=2, out=ptr(out))

    def call(handle=ctx.handle, **over):
        a = dict(base)
        a.update(over)
        return ctx.lib.ng_label_moments(handle, s, *a.values())

    assert call(handle=None) == NG_ERR_INVALID
    for over in [dict(C=0), dict(C=4097), dict(R=-1), dict(Ntot=1), dict(Rv=-1), dict(Rv=2 ** 31), dict(out=None),
                 dict(atoms=None), dict(y=None), dict(rec_ptr=None), dict(ids=None)]:
        assert call(**over) == NG_ERR_INVALID, over
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out).all())
    assert call(Rv=0, atoms=None, y=None, rec_ptr=None, ids=None) == 0
    torch.cuda.synchronize(dev)
    assert not out.cpu().numpy().any()
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert np.array_equal(out.cpu().numpy(), RR.label_moments_ref(atoms, y, rec_ptr, [0, 1]))


# ---------------------------------------------------------------------------------------------- end to end
def _synthetic_structure(n, seed, frames=1):
    from nmrgnn_amd.structure import Structure
    rng = np.random.default_rng(seed)
    names = [f"{'HCNO'[i % 4]}{i}" for i in range(n)]
    side = 3.0 * n ** (1 / 3) + 2.0
    return Structure(names, [("ALA", "GLY", "SER")[i % 3] for i in range(n)], [i // 7 for i in range(n)],
                     ["HCNO"[i % 4] for i in range(n)], [rng.uniform(0, side, (n, 3)) for _ in range(frames)])


def _tables(structs, tmp_path):
    rows = [RR.synthetic_labels(s, seed=20 + k) for k, s in enumerate(structs)]
    return rows, [RR.write_table(str(tmp_path / f"t{k}.csv"), r) for k, r in enumerate(rows)]


def _store_equal(a, b):
    import torch
    assert np.array_equal(a.rec_ptr_host, b.rec_ptr_host) and np.array_equal(a.file_ptr, b.file_ptr)
    for k in KEYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y)), k


def test_from_structures_equals_from_records_over_one_structure_batches(gpu_device, tmp_path):
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.graph import structures_to_batch
    from nmrgnn_amd.structure import atoms_onehot, inv_degree_of, name_ids, name_table, read_pdb
    structs = [read_pdb(PDB1), read_pdb(PDB10)]
    rows, paths = _tables(structs, tmp_path)
    ds = ShiftDataset.from_structures([PDB1, PDB10], paths, frames="all", device=gpu_device)
    assert ds.R == 11 and ds.atoms.is_cuda and ds.file_ptr.tolist() == [0, 11]
    table = name_table(structs)
    assert ds.name_table == table
    records = []
    for k, s in enumerate(structs):
        sh = RR.join_ref(s.resids, s.names, rows[k])
        has = np.isfinite(sh)
        y = np.stack([np.where(has, sh, 0), name_ids(s, table).astype(np.float32), has], axis=1).astype(np.float32)
        for fr in range(len(s)):
            gb = structures_to_batch([atoms_onehot(s.elements)], [s.frames[fr]], 16, device=gpu_device)     # G = 1
            e = gb.edges.cpu().numpy()
            nl = np.where(e > 0, gb.nlist.cpu().numpy(), 0).astype(np.int32)                                # offset 0: local
            assert (e > 0).all()
            records.append(((atoms_onehot(s.elements), nl, e, inv_degree_of(nl)), y, has.astype(np.float32)))
    _store_equal(ds, ShiftDataset.from_records(records, device=gpu_device))
    assert ds.join_report["labelled"] == sum(len(r) * len(s) for r, s in zip(rows, structs))
    assert ds.join_report["labelled"] == int(ds.w.sum().item())


def test_from_structures_chunks_and_batch(gpu_device, tmp_path):
    """chunk_atoms = 1000: [300 + 1 + 500 atoms], [108M: 2482 atoms, larger than a chunk], [7lgi: 2770] — the bits of one chunk;
    and the store's batch of all records is the structures_to_batch batch on live slots, edges and inv_degree"""
    import torch
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.graph import structures_to_batch
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    structs = [_synthetic_structure(300, 1), _synthetic_structure(1, 2), _synthetic_structure(500, 3), read_pdb(PDB1),
               read_pdb(PDB10)]
    _, paths = _tables(structs, tmp_path)
    paths[1] = None
    one = ShiftDataset.from_structures(structs, paths, device=gpu_device)
    _store_equal(ShiftDataset.from_structures(structs, paths, chunk_atoms=1000, device=gpu_device), one)
    _store_equal(ShiftDataset.from_structures(structs, paths, chunk_atoms=1, device=gpu_device), one)      # a chunk each
    assert one.R == 5 and one.rec_ptr_host.tolist() == [0, 300, 301, 801, 3283, 6053]
    want = structures_to_batch([atoms_onehot(s.elements) for s in structs], [s.frames[0] for s in structs], 16,
                               device=gpu_device)
    gb, y, w, names = one.batch(range(5))
    live = want.edges > 0
    assert bool(live[:300].all()) and not bool(live[300].any())
    assert torch.equal(gb.nlist[live], want.nlist[live]) and bool((one.nlist[~live] == 0).all())
    assert torch.equal(_bits(gb.edges), _bits(want.edges)) and torch.equal(_bits(gb.inv_degree), _bits(want.inv_degree))
    assert torch.equal(_bits(gb.atoms), _bits(want.atoms)) and np.array_equal(gb.graph_ptr_host, want.graph_ptr_host)
    assert float(w[300].item()) == 0.0 and float(w.sum().item()) == one.join_report["labelled"] > 100


def test_from_structures_boxes(gpu_device):
    import torch
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.graph import structures_to_batch
    from nmrgnn_amd.structure import Structure, atoms_onehot, read_pdb
    s = read_pdb(PDB1)
    assert s.dimensions[0] is not None
    small = Structure(s.names, s.resnames, s.resids, s.elements, s.frames, [np.array([30.0, 28.0, 26.0, 90.0, 90.0, 90.0])])
    open_ = ShiftDataset.from_structures([s], [None], device=gpu_device)
    for st in (s, small):
        ds = ShiftDataset.from_structures([st], [None], boxes=True, device=gpu_device)
        want = structures_to_batch([atoms_onehot(st.elements)], [st.frames[0]], 16, device=gpu_device, boxes=[st.dimensions[0]])
        assert torch.equal(ds.nlist, want.nlist) and torch.equal(_bits(ds.edges), _bits(want.edges))
        assert torch.equal(_bits(ds.inv_degree), _bits(want.inv_degree))
    assert not torch.equal(ds.edges, open_.edges)              # the 30 x 28 x 26 box folds the protein onto itself


def _labelled_set(dev, tmp_path):
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(PDB10)
    rows = RR.synthetic_labels(s, seed=31)
    return ShiftDataset.from_structures([s], [RR.write_table(str(tmp_path / "t.csv"), rows)], frames="all", device=dev)


def test_standards_to_fit(gpu_device, tmp_path):
    import torch
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.library import load_model
    from nmrgnn_amd.model import build_GNNModel
    from nmrgnn_amd.standards import load_standards
    ds = _labelled_set(gpu_device, tmp_path)
    train, val = ds.split(0.2)
    assert len(train) == 8 and len(val) == 2
    st = train.standards()
    # the device moments are those of the host path over the same records, to the summation bound; counts exactly
    host = ShiftDataset.from_records([((ds.atoms[a:b].cpu().numpy(), ds.nlist[a:b].cpu().numpy(), ds.edges[a:b].cpu().numpy(),
                                        ds.inv_degree[a:b].cpu().numpy()), ds.y[a:b].cpu().numpy(), ds.w[a:b].cpu().numpy())
                                      for a, b in zip(ds.rec_ptr_host[:-1], ds.rec_ptr_host[1:])], device="cpu")
    hs = host.split(0.2)[0].standards()
    assert sorted(st) == list(range(10))
    for c in range(10):
        assert st[c][0] == hs[c][0] and st[c][1] == pytest.approx(hs[c][1], rel=1e-12, abs=1e-12)
        assert st[c][2] == pytest.approx(hs[c][2], rel=1e-9, abs=1e-9)
    assert st[4][2] > 1.0 and st[2][2] > 1.0 and st[8] == ("F", 0.0, 0.0) and st != load_standards()
    model = build_GNNModel(device=gpu_device, peak_standards=st)
    model.build(ds.C)
    before = model.engine.params.flat.clone()
    hist = model.fit(train, epochs=1, validation_data=val, verbose=0)
    after = model.engine.params.flat
    assert np.isfinite(hist.history["loss"][0]) and np.isfinite(hist.history["val_loss"][0])
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    ev = model.evaluate(val.eval_batches(1))
    assert np.isfinite(ev["loss"])
    # save / load_model carry the standards
    model.save(str(tmp_path / "m"))
    back = load_model(str(tmp_path / "m"), device=gpu_device)
    assert back.peak_standards == st
    assert np.array_equal(back.peak_std[:10], model.peak_std[:10]) and np.array_equal(back.peak_avg[:10], model.peak_avg[:10])
    gb, yt = next(iter(val.eval_batches(1)))
    assert torch.equal(back(gb), model(gb))


def test_make_records_then_train_commands(gpu_device, tmp_path):
    import json
    from click.testing import CliRunner
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.library import load_model
    from nmrgnn_amd.main import main
    from nmrgnn_amd.standards import load_standards
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(PDB10)
    t = RR.write_table(str(tmp_path / "t.csv"), RR.synthetic_labels(s, seed=31))
    out, emb, name = str(tmp_path / "r.npz"), str(tmp_path / "emb.json"), str(tmp_path / "model")
    res = CliRunner().invoke(main, ["make-records", out, "--pair", PDB10, t, "--frames", "all", "--embeddings-out", emb])
    assert res.exit_code == 0, res.output + repr(res.exception)
    assert "10 records" in res.output and json.load(open(emb))["name"]["X"] == 0
    _store_equal(ShiftDataset.load(out, device=gpu_device), _labelled_set(gpu_device, tmp_path))
    res = CliRunner().invoke(main, ["train", out, name, "1", "--checkpoint-path", str(tmp_path / "ckpt"), "--validation", "0.2",
                                    "--standards", "data"])
    assert res.exit_code == 0, res.output + repr(res.exception)
    m = load_model(name, device=gpu_device)
    want = ShiftDataset.load(out, device=gpu_device).split(0.2)[0].standards()
    assert m.peak_standards == want and m.peak_standards != load_standards() and m.engine.adam_t == 8
    res = CliRunner().invoke(main, ["train", out, name + "d", "1", "--checkpoint-path", str(tmp_path / "ckpt2"), "--validation", "0.2"])
    assert res.exit_code == 0, res.output + repr(res.exception)
    assert load_model(name + "d", device=gpu_device).peak_standards == load_standards()
