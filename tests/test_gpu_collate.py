"""ng_collate_batch (csrc/collate.hip) against tests/collate_ref.py, element by element and bit for bit, through the C entry
point: outputs pre-filled with NaN / sentinels between guard rows, two calls, every branch of the kernel.

Launch arithmetic restated (csrc/collate.hip): a workgroup of 256 threads owns a tile of CL_TILE = 256 output atoms per trip;
grid = min(ceil(N / 256), CL_MAX_BLOCKS = 1024) workgroups stride over the tiles, so N > 262144 atoms gives some workgroup a
second trip.  Per tile each atom finds its graph by binary search over the G + 1 boundaries.  A thread copies one chunk of a
row at a time, four chunks in flight (a tile of K = 16 list rows is 1024 16-byte chunks: one round; K = 5 is 1280 words: a
second, partly filled round).  List rows are copied in 16-byte chunks when K % 4 == 0 and the four list arrays (store and
batch, nlist and edges) are 16-byte aligned, word by word otherwise; atom rows in 16-byte chunks for C % 4 == 0 and 16-byte
aligned atoms arrays, in 8-byte chunks for C % 2 == 0 and 8-byte alignment, word by word otherwise.  So the branches are:
K = 16 / C = 10 aligned (16-byte lists, 8-byte atoms), K = 5 / C = 3 (words), K = 4 / C = 1 (one chunk per list row, words),
K = 8 / C = 4 (16 bytes for both), and K = 16 / C = 10, K = 8 / C = 4 with the store or the batch arrays starting 4 bytes
(words everywhere) or 8 bytes (words for the lists, 8-byte atoms) past a 16-byte boundary."""
import ctypes as C
import functools

import numpy as np
import pytest

import collate_ref as R

pytestmark = pytest.mark.gpu

CL_TILE, CL_MAX_BLOCKS = 256, 1024
SIZES = [1, 2, 15, 16, 17, 255, 256, 257, 300]
GUARD = 3                     # guard rows before and after every output
I_SENT = -7777777
STORE_KEYS = ("atoms", "nlist", "edges", "inv_degree", "y", "w")
OUT_KEYS = ("atoms", "nlist", "edges", "inv_degree", "y", "w", "names", "y_true")


@functools.lru_cache(maxsize=None)
def _store(K, Cc):
    recs = R.make_records(SIZES, K=K, C=Cc, seed=100 + K)
    return recs, R.store_of(recs)


def _dev(a, dev, shift):
    """a device copy of host array ``a`` that starts ``shift`` elements past its allocation (shift = 1: 4 bytes off 16)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=dev)
    v = buf[shift:].view(t.shape)
    v.copy_(t)
    return v


def _outputs(N, K, Cc, dev, shift):
    """{name: (whole buffer with guards, interior view)} filled with NaN / the integer sentinel"""
    import torch
    shapes = {"atoms": (Cc,), "nlist": (K,), "edges": (K,), "inv_degree": (), "y": (), "w": (), "names": (), "y_true": (3,)}
    out = {}
    for k, tail in shapes.items():
        integer = k in ("nlist", "names")
        rows = N + 2 * GUARD
        width = int(np.prod(tail)) if tail else 1
        buf = torch.full((rows * width + shift,), I_SENT if integer else float("nan"),
                         dtype=torch.int32 if integer else torch.float32, device=dev)
        whole = buf[shift:].view((rows,) + tail)
        out[k] = (whole, whole[GUARD:GUARD + N])
    return out


def _call(ctx, st, ids_dev, gp_dev, N, K, Cc, G, out, y_true=True, R_=None, stream=None):
    import torch
    from nmrgnn_amd._lib import ptr
    R_ = len(st["rec_ptr"]) - 1 if R_ is None else R_
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return ctx.lib.ng_collate_batch(ctx.handle, s, R_, int(st["rec_ptr_host"][-1]), ptr(st["atoms"]), ptr(st["nlist"]),
                                    ptr(st["edges"]), ptr(st["inv_degree"]), ptr(st["y"]), ptr(st["w"]), ptr(st["rec_ptr"]),
                                    ptr(ids_dev), ptr(gp_dev), N, K, Cc, G, ptr(out["atoms"][1]), ptr(out["nlist"][1]),
                                    ptr(out["edges"][1]), ptr(out["inv_degree"][1]), ptr(out["y"][1]), ptr(out["w"][1]),
                                    ptr(out["names"][1]), ptr(out["y_true"][1]) if y_true else None)


def _upload(host, dev, shift=0):
    import torch
    st = {k: _dev(host[k], dev, shift) for k in STORE_KEYS}
    st["rec_ptr"] = torch.from_numpy(host["rec_ptr"]).to(dev)
    st["rec_ptr_host"] = host["rec_ptr"]
    return st


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _check(out, ref, N, y_true=True):
    """interior == reference bit for bit; guards and (without y_true) the y_true buffer still hold the fill"""
    import torch
    dev = out["atoms"][0].device
    for k in OUT_KEYS:
        whole, inner = out[k]
        integer = k in ("nlist", "names")
        if k == "y_true" and not y_true:
            assert bool(torch.isnan(whole).all()), "y_true written although NULL was passed"
            continue
        want = torch.from_numpy(np.ascontiguousarray(ref[k])).to(dev)
        assert inner.dtype == want.dtype and tuple(inner.shape) == tuple(want.shape), k
        assert torch.equal(_bits(inner), _bits(want)), f"{k} differs from the reference"
        for g in (whole[:GUARD], whole[GUARD + N:]):
            assert bool((g == I_SENT).all() if integer else torch.isnan(g).all()), f"guard rows of {k} were written"


def _run_case(dev, K, Cc, ids, src_shift=0, dst_shift=0, y_true=True):
    import torch
    from nmrgnn_amd import _lib
    ctx = _lib.get_context(dev.index)
    _, host = _store(K, Cc)
    ref = R.collate_ref(host, ids)
    N, G = int(ref["graph_ptr"][-1]), len(ids)
    st = _upload(host, dev, src_shift)
    ids_dev = torch.tensor(list(ids), dtype=torch.int32, device=dev)
    gp_dev = torch.from_numpy(ref["graph_ptr"]).to(dev)
    first = _outputs(N, K, Cc, dev, dst_shift)
    second = _outputs(N, K, Cc, dev, dst_shift)
    for out in (first, second):
        rc = _call(ctx, st, ids_dev, gp_dev, N, K, Cc, G, out, y_true=y_true)
        assert rc == 0, ctx.lib.ng_last_error(ctx.handle)
    torch.cuda.synchronize(dev)
    _check(first, ref, N, y_true)
    for k in OUT_KEYS:        # the second call's bits are the first's, guards and all
        assert torch.equal(_bits(first[k][0]), _bits(second[k][0])), k
    return N


def _id_lists():
    rng = np.random.default_rng(42)
    mixed = rng.integers(0, len(SIZES), size=40).tolist()            # random order, repeats: nothing sorted
    return {
        "first": [0], "last": [8], "in_order": list(range(9)), "reversed": list(range(8, -1, -1)), "thrice": [5, 5, 5],
        "one_tile": [0, 5], "tile_minus_1": [5], "tile_plus_1": [1, 5], "tiles_3_plus": [8, 7, 6, 0], "random_order": mixed,
        "513_one_atom_graphs": [0] * 513,
    }


def test_id_lists_hit_the_sizes_they_name():
    sz = np.asarray(SIZES)
    L = _id_lists()
    assert sz[L["one_tile"]].sum() == CL_TILE and sz[L["tile_minus_1"]].sum() == CL_TILE - 1
    assert sz[L["tile_plus_1"]].sum() == CL_TILE + 1 and sz[L["513_one_atom_graphs"]].sum() == 513
    assert L["random_order"] != sorted(L["random_order"])


@pytest.mark.parametrize("name", list(_id_lists()))
def test_collate_k16_c10(gpu_device, name):
    _run_case(gpu_device, 16, 10, _id_lists()[name])


@pytest.mark.parametrize("K,Cc", [(5, 3), (4, 1), (8, 4)])
@pytest.mark.parametrize("name", ["in_order", "reversed", "thrice", "tile_plus_1", "random_order", "513_one_atom_graphs"])
def test_collate_other_widths(gpu_device, K, Cc, name):
    _run_case(gpu_device, K, Cc, _id_lists()[name])


@pytest.mark.parametrize("K,Cc", [(16, 10), (8, 4)])
@pytest.mark.parametrize("src_shift,dst_shift", [(1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 2)])
def test_collate_misaligned_rows(gpu_device, K, Cc, src_shift, dst_shift):
    for name in ("random_order", "tile_plus_1"):
        _run_case(gpu_device, K, Cc, _id_lists()[name], src_shift=src_shift, dst_shift=dst_shift)


def test_collate_without_y_true(gpu_device):
    _run_case(gpu_device, 16, 10, _id_lists()["random_order"], y_true=False)


def test_collate_past_the_grid_cap(gpu_device):
    ids = [8] * 873 + [7, 0]                      # 873 * 300 + 257 + 1 = 262158 atoms: 1025 tiles for 1024 workgroups
    N = _run_case(gpu_device, 16, 10, ids)
    assert -(-N // CL_TILE) == CL_MAX_BLOCKS + 1


def test_rows_that_do_not_fit_the_store_are_skipped(gpu_device):
    """ids and graph_ptr are device data the host never reads: an id outside [0, R), or a graph longer than its record, must
    leave its rows untouched and read nothing"""
    import torch
    from nmrgnn_amd import _lib
    dev, K, Cc = gpu_device, 16, 10
    ctx = _lib.get_context(dev.index)
    _, host = _store(K, Cc)
    st = _upload(host, dev)
    # graph 0: record 2 (15 atoms); graph 1: id 9 == R, 4 rows; graph 2: id -1, 2 rows; graph 3: record 1 (2 atoms) given 5 rows
    ids, gp = [2, 9, -1, 1], [0, 15, 19, 21, 26]
    N, G = 26, 4
    out = _outputs(N, K, Cc, dev, 0)
    rc = _call(ctx, st, torch.tensor(ids, dtype=torch.int32, device=dev), torch.tensor(gp, dtype=torch.int32, device=dev), N, K, Cc,
               G, out)
    assert rc == 0
    torch.cuda.synchronize(dev)
    ok = R.collate_ref(host, [2])
    tail = R.collate_ref(host, [1])
    for k in OUT_KEYS:
        whole, inner = out[k]
        integer = k in ("nlist", "names")
        assert torch.equal(_bits(inner[:15]), _bits(torch.from_numpy(np.ascontiguousarray(ok[k])).to(dev))), k
        want = np.ascontiguousarray(tail[k] + 21 if k == "nlist" else tail[k])
        assert torch.equal(_bits(inner[21:23]), _bits(torch.from_numpy(want).to(dev))), k
        for skipped in (inner[15:21], inner[23:], whole[:GUARD], whole[GUARD + N:]):
            assert bool((skipped == I_SENT).all() if integer else torch.isnan(skipped).all()), k


def test_refusals_and_empty_batch(gpu_device):
    import torch
    from nmrgnn_amd import _lib
    from nmrgnn_amd._lib import ptr
    dev, K, Cc = gpu_device, 16, 10
    ctx = _lib.get_context(dev.index)
    _, host = _store(K, Cc)
    st = _upload(host, dev)
    ids = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    gp = torch.tensor([0, 2, 3], dtype=torch.int32, device=dev)
    N, G = 3, 2
    out = _outputs(N, K, Cc, dev, 0)
    NG_ERR_INVALID = -1
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def args(**over):
        a = dict(R=9, Ntot=int(host["rec_ptr"][-1]), s_atoms=ptr(st["atoms"]), s_nlist=ptr(st["nlist"]), s_edges=ptr(st["edges"]),
                 s_inv=ptr(st["inv_degree"]), s_y=ptr(st["y"]), s_w=ptr(st["w"]), rec_ptr=ptr(st["rec_ptr"]), ids=ptr(ids),
                 gp=ptr(gp), N=N, K=K, C=Cc, G=G, atoms=ptr(out["atoms"][1]), nlist=ptr(out["nlist"][1]),
                 edges=ptr(out["edges"][1]), inv=ptr(out["inv_degree"][1]), y0=ptr(out["y"][1]), w=ptr(out["w"][1]),
                 names=ptr(out["names"][1]), y_true=ptr(out["y_true"][1]))
        a.update(over)
        return list(a.values())

    assert ctx.lib.ng_collate_batch(None, s, *args()) == NG_ERR_INVALID            # NULL context
    bad = [dict(K=0), dict(C=0), dict(K=-1), dict(G=0), dict(G=4), dict(N=-1), dict(N=2 ** 31), dict(R=0), dict(Ntot=8)]
    bad += [{k: None} for k in ("s_atoms", "s_nlist", "s_edges", "s_inv", "s_y", "s_w", "rec_ptr", "ids", "gp", "atoms", "nlist",
                                "edges", "inv", "y0", "w", "names")]
    for over in bad:
        assert ctx.lib.ng_collate_batch(ctx.handle, s, *args(**over)) == NG_ERR_INVALID, over
        assert ctx.lib.ng_last_error(ctx.handle)
    # N == 0: OK, nothing launched, whatever the pointers are
    assert ctx.lib.ng_collate_batch(ctx.handle, s, *args(N=0, G=0)) == 0
    assert ctx.lib.ng_collate_batch(ctx.handle, s, *args(N=0, G=0, atoms=None, ids=None, s_y=None)) == 0
    torch.cuda.synchronize(dev)
    for k in OUT_KEYS:                          # every refusal and the empty batch left the outputs as they were
        whole = out[k][0]
        assert bool((whole == I_SENT).all() if k in ("nlist", "names") else torch.isnan(whole).all()), k
    # and the same arguments unchanged do run
    assert ctx.lib.ng_collate_batch(ctx.handle, s, *args()) == 0
    torch.cuda.synchronize(dev)
    _check(out, R.collate_ref(host, [1, 0]), N)


@pytest.mark.parametrize("K,Cc", [(16, 10), (5, 3)])
def test_dataset_batch_builds_the_lists_of_concat_graphs(gpu_device, K, Cc):
    import torch
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.graph import concat_graphs
    recs, host = _store(K, Cc)
    ds = ShiftDataset.from_records(recs, device=gpu_device)
    assert ds.rec_ptr.is_cuda and ds.rec_ptr.dtype == torch.int64
    for ids in ([4], [8, 0, 3, 3, 7], _id_lists()["random_order"]):
        gb, y, w, names = ds.batch(ids)
        ref = R.collate_ref(host, ids)
        want = concat_graphs([recs[i][0] for i in ids], device=gpu_device)
        for k in ("atoms", "nlist", "edges", "inv_degree", "nlist_c", "graph_ptr"):
            assert torch.equal(_bits(getattr(gb, k)), _bits(getattr(want, k))), k
        assert np.array_equal(gb.graph_ptr_host, want.graph_ptr_host) and gb.G == want.G and gb.N == want.N
        n_in = int(want.csc()[0][-1])
        assert torch.equal(gb.csc()[0], want.csc()[0]) and torch.equal(gb.csc()[1][:n_in], want.csc()[1][:n_in])
        lv, lr = gb.live_edges(), want.live_edges()
        n_live = int(lr[3])
        assert int(lv[3]) == n_live and torch.equal(lv[0][:n_live], lr[0][:n_live]) and torch.equal(lv[1], lr[1])
        assert torch.equal(_bits(lv[2][:n_live]), _bits(lr[2][:n_live]))
        for got, k in ((y, "y"), (w, "w"), (names, "names")):
            assert torch.equal(_bits(got), _bits(torch.from_numpy(ref[k]).to(gpu_device))), k
    got = list(ds.eval_batches(4))
    assert [g.G for g, _ in got] == [4, 4, 1]
    assert torch.equal(_bits(torch.cat([yt for _, yt in got])), _bits(torch.from_numpy(host["y"]).to(gpu_device)))
