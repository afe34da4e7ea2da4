"""tests/collate_ref.py (the NumPy statement of ShiftDataset.batch) against graph.concat_graphs' arrays and hand-written
cases, and nmrgnn_amd/dataset.py on the CPU device against it: bit-for-bit batches, the file round trip, the split, every
refusal of from_records, and the epoch iterator's order."""
import numpy as np
import pytest
import torch

import collate_ref as R

KEYS = ("atoms", "nlist", "edges", "inv_degree")


def _concat_arrays(records, ids):
    """the arrays graph.concat_graphs builds (its GraphBatch on the host device)"""
    from nmrgnn_amd.graph import concat_graphs
    gb = concat_graphs([records[i][0] for i in ids], device="cpu")
    return gb


def _hand_store():
    # two records of 2 and 3 atoms at K = 2, C = 1; record 0 has a padded slot in its second row
    a0 = np.array([[1.0], [2.0]], np.float32)
    n0 = np.array([[1, 1], [0, 0]], np.int32)
    e0 = np.array([[0.5, 0.25], [0.5, 0.0]], np.float32)
    a1 = np.array([[3.0], [4.0], [5.0]], np.float32)
    n1 = np.array([[1, 2], [2, 0], [0, 0]], np.int32)
    e1 = np.array([[0.1, 0.2], [0.3, 0.4], [0.0, 0.0]], np.float32)
    y0 = np.array([[10, 7.75, 1], [11, 8, 0]], np.float32)
    y1 = np.array([[12, 1, 1], [13, 2.5, 1], [14, 3, 0]], np.float32)
    recs = [((a0, n0, e0, np.array([1.0, 0.0], np.float32)), y0, np.array([1.0, 0.5], np.float32)),
            ((a1, n1, e1, np.array([0.5, 1.0, 0.0], np.float32)), y1, np.array([2.0, 3.0, 4.0], np.float32))]
    return recs


def test_hand_cases():
    recs = _hand_store()
    st = R.store_of(recs)
    assert st["rec_ptr"].tolist() == [0, 2, 5]
    b = R.collate_ref(st, [1, 0])
    assert b["graph_ptr"].tolist() == [0, 3, 5]
    assert b["atoms"].reshape(-1).tolist() == [3, 4, 5, 1, 2]
    # record 0 lands behind the three atoms of record 1: every slot + 3, the padded ones too
    assert b["nlist"].tolist() == [[1, 2], [2, 0], [0, 0], [4, 4], [3, 3]]
    assert b["edges"].tolist() == np.array([[0.1, 0.2], [0.3, 0.4], [0, 0], [0.5, 0.25], [0.5, 0]], np.float32).tolist()
    assert b["inv_degree"].tolist() == [0.5, 1.0, 0.0, 1.0, 0.0]
    assert b["y"].tolist() == [12, 13, 14, 10, 11]
    assert b["names"].tolist() == [1, 2, 3, 7, 8] and b["names"].dtype == np.int32
    assert b["w"].tolist() == [2, 3, 4, 1, 0.5]
    assert b["y_true"][3].tolist() == [10, 7.75, 1]
    b = R.collate_ref(st, [0, 0])
    assert b["graph_ptr"].tolist() == [0, 2, 4]
    assert b["atoms"].reshape(-1).tolist() == [1, 2, 1, 2]
    assert b["nlist"].tolist() == [[1, 1], [0, 0], [3, 3], [2, 2]]
    assert b["w"].tolist() == [1, 0.5, 1, 0.5]


@pytest.mark.parametrize("K,C,seed", [(16, 10, 0), (5, 3, 1), (4, 1, 2)])
def test_reference_equals_concat_graphs(K, C, seed):
    recs = R.make_records([1, 2, 15, 16, 17, 40, 33], K=K, C=C, seed=seed)
    st = R.store_of(recs)
    rng = np.random.default_rng(seed)
    for ids in ([0], [6], list(range(7)), list(range(6, -1, -1)), [3, 3, 3], rng.integers(0, 7, size=12).tolist()):
        b = R.collate_ref(st, ids)
        gb = _concat_arrays(recs, ids)
        for k in KEYS:
            got, want = b[k], getattr(gb, k).numpy()
            assert got.dtype == want.dtype and np.array_equal(got.view(np.int32), want.view(np.int32)), (k, ids)
        assert np.array_equal(b["graph_ptr"], gb.graph_ptr_host)


def _check_batch(out, ref):
    gb, y, w, names = out
    for k in KEYS:
        got = getattr(gb, k)
        assert torch.equal(got.view(torch.int32), torch.from_numpy(ref[k]).view(torch.int32)), k
    assert np.array_equal(gb.graph_ptr_host, ref["graph_ptr"])
    assert torch.equal(y.view(torch.int32), torch.from_numpy(ref["y"]).view(torch.int32))
    assert torch.equal(w.view(torch.int32), torch.from_numpy(ref["w"]).view(torch.int32))
    assert names.dtype == torch.int32 and torch.equal(names, torch.from_numpy(ref["names"]))


@pytest.mark.parametrize("K,C,seed", [(16, 10, 3), (5, 3, 4)])
def test_cpu_dataset_equals_reference(K, C, seed):
    from nmrgnn_amd.dataset import ShiftDataset
    recs = R.make_records([1, 2, 15, 16, 17, 40, 33], K=K, C=C, seed=seed)
    st = R.store_of(recs)
    ds = ShiftDataset.from_records(recs, device="cpu")
    assert len(ds) == 7 and ds.C == C and ds.K == K and ds.rec_ptr_host.tolist() == st["rec_ptr"].tolist()
    assert ds.rec_ptr.dtype == torch.int64 and ds.file_ptr.tolist() == [0, 7]
    for ids in ([0], [6], list(range(7)), list(range(6, -1, -1)), [3, 3, 3], [5, 0, 5, 2]):
        _check_batch(ds.batch(ids), R.collate_ref(st, ids))
    # the hand cases through the class
    hs = ShiftDataset.from_records(_hand_store(), device="cpu")
    gb, y, w, names = hs.batch([1, 0])
    assert gb.nlist.tolist() == [[1, 2], [2, 0], [0, 0], [4, 4], [3, 3]] and names.tolist() == [1, 2, 3, 7, 8]
    # eval_batches: store order, y_true whole
    got = list(ds.eval_batches(3))
    assert [g.G for g, _ in got] == [3, 3, 1]
    assert torch.equal(torch.cat([yt for _, yt in got]), torch.from_numpy(st["y"]))
    with pytest.raises(ValueError):
        ds.batch([7])
    with pytest.raises(ValueError):
        ds.batch([])


def test_save_load_round_trip_and_split(tmp_path):
    from nmrgnn_amd.dataset import FORMAT_VERSION, ShiftDataset
    ra = R.make_records([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], K=4, C=2, seed=5)        # 12 records
    rb = R.make_records([2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 9, 9, 9, 9, 9], K=4, C=2, seed=6)   # 25 records
    a, b = ShiftDataset.from_records(ra, device="cpu"), ShiftDataset.from_records(rb, device="cpu")
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    a.save(pa)
    b.save(pb)
    z = np.load(pa)
    assert sorted(z.files) == sorted(["atoms", "nlist", "edges", "inv_degree", "y", "w", "rec_ptr", "file_ptr", "format_version"])
    assert int(z["format_version"]) == FORMAT_VERSION and z["rec_ptr"].dtype == np.int64
    one = ShiftDataset.load(pa, device="cpu")
    sa = R.store_of(ra)
    for k in ("atoms", "nlist", "edges", "inv_degree", "y", "w"):
        assert getattr(one, k).numpy().dtype == sa[k].dtype
        assert np.array_equal(getattr(one, k).numpy().view(np.int32), sa[k].view(np.int32)), k
    assert one.rec_ptr_host.tolist() == sa["rec_ptr"].tolist()
    both = ShiftDataset.load([pa, pb], device="cpu")
    sab = R.store_of(ra + rb)
    assert both.file_ptr.tolist() == [0, 12, 37] and both.rec_ptr_host.tolist() == sab["rec_ptr"].tolist()
    _check_batch(both.batch([36, 0, 12, 11]), R.collate_ref(sab, [36, 0, 12, 11]))
    # split(0.1): int(0.1 * 12) = 1 of the first source, int(0.1 * 25) = 2 of the second
    train, val = both.split(0.1)
    assert val.record_ids.tolist() == [0, 12, 13]
    assert train.record_ids.tolist() == list(range(1, 12)) + list(range(14, 37))
    assert train.atoms.data_ptr() == both.atoms.data_ptr() and val.nlist.data_ptr() == both.nlist.data_ptr()     # views
    _check_batch(val.batch([2, 0]), R.collate_ref(sab, [13, 0]))         # ids count within the view
    _check_batch(train.batch([11]), R.collate_ref(sab, [14]))
    assert len(both.split(0.0)[1]) == 0 and len(both.split(0.0)[0]) == 37
    # a view saves its own records
    pv = str(tmp_path / "v.npz")
    val.save(pv)
    v = ShiftDataset.load(pv, device="cpu")
    assert len(v) == 3 and v.file_ptr.tolist() == [0, 3]
    _check_batch(v.batch([0, 1, 2]), R.collate_ref(sab, [0, 12, 13]))
    # a file of another version is refused
    np.savez(str(tmp_path / "old.npz"), **{**{k: z[k] for k in z.files}, "format_version": np.asarray(0)})
    with pytest.raises(ValueError):
        ShiftDataset.load(str(tmp_path / "old.npz"), device="cpu")


def _rec(n=4, K=3, C=2, **over):
    (atoms, nlist, edges, inv), y, w = R.make_records([n], K=K, C=C, seed=9)[0]
    d = dict(atoms=atoms, nlist=nlist, edges=edges, inv=inv, y=y, w=w)
    d.update(over)
    return ((d["atoms"], d["nlist"], d["edges"], d["inv"]), d["y"], d["w"])


def test_from_records_refusals():
    from nmrgnn_amd.dataset import ShiftDataset
    good = _rec()
    ShiftDataset.from_records([good, _rec(6)], device="cpu")
    bad_nlist_hi = good[0][1].copy()
    bad_nlist_hi[2, 1] = 4                       # == n
    bad_nlist_lo = good[0][1].copy()
    bad_nlist_lo[0, 0] = -1
    e_neg, e_nan, e_inf = (good[0][2].copy() for _ in range(3))
    e_neg[1, 1], e_nan[1, 1], e_inf[1, 1] = -0.1, np.nan, np.inf
    cases = {
        "C differs": [good, _rec(C=3)],
        "K differs": [good, _rec(K=4)],
        "nlist == n": [good, _rec(nlist=bad_nlist_hi)],
        "nlist < 0": [good, _rec(nlist=bad_nlist_lo)],
        "negative edge": [good, _rec(edges=e_neg)],
        "nan edge": [good, _rec(edges=e_nan)],
        "inf edge": [good, _rec(edges=e_inf)],
        "edges rows": [good, _rec(edges=good[0][2][:3])],
        "nlist rows": [good, _rec(nlist=good[0][1][:3])],
        "inv rows": [good, _rec(inv=good[0][3][:3])],
        "y rows": [good, _rec(y=good[1][:3])],
        "w rows": [good, _rec(w=good[2][:3])],
        "y columns": [good, _rec(y=good[1][:, :2])],
        "n == 0": [good, _rec(atoms=good[0][0][:0], nlist=good[0][1][:0], edges=good[0][2][:0], inv=good[0][3][:0],
                              y=good[1][:0], w=good[2][:0])],
    }
    for what, recs in cases.items():
        with pytest.raises(ValueError, match="record 1"):
            ShiftDataset.from_records(recs, device="cpu")
    with pytest.raises(ValueError):
        ShiftDataset.from_records([], device="cpu")

    class Arr:                                  # anything with __array__ is taken
        def __init__(self, a):
            self.a = a

        def __array__(self, dtype=None, copy=None):
            return self.a if dtype is None else self.a.astype(dtype)
    (x, y, w) = good
    ds = ShiftDataset.from_records([(tuple(Arr(t) for t in x), Arr(y), Arr(w))], device="cpu")
    assert torch.equal(ds.atoms, torch.from_numpy(x[0]))


def test_epoch_iterator_order():
    from nmrgnn_amd.dataset import ShiftDataset
    sizes = [2 + (i % 5) for i in range(23)]
    recs = R.make_records(sizes, K=4, C=2, seed=11)
    st = R.store_of(recs)
    ds = ShiftDataset.from_records(recs, device="cpu")
    e0 = ds.epoch_ids(4, shuffle=True, seed=7, epoch=0)
    assert [len(c) for c in e0] == [4, 4, 4, 4, 4, 3]
    flat0 = np.concatenate(e0)
    assert sorted(flat0.tolist()) == list(range(23))                       # every record exactly once
    assert flat0.tolist() == np.random.default_rng([7, 0]).permutation(23).tolist()      # the documented permutation
    assert np.concatenate(ds.epoch_ids(4, seed=7, epoch=0)).tolist() == flat0.tolist()
    flat1 = np.concatenate(ds.epoch_ids(4, seed=7, epoch=1))
    assert sorted(flat1.tolist()) == list(range(23)) and flat1.tolist() != flat0.tolist()
    assert np.concatenate(ds.epoch_ids(4, seed=8, epoch=0)).tolist() != flat0.tolist()
    assert np.concatenate(ds.epoch_ids(4, shuffle=False)).tolist() == list(range(23))
    assert [len(c) for c in ds.epoch_ids(4, drop_remainder=True)] == [4] * 5
    assert [len(c) for c in ds.epoch_ids(23, drop_remainder=True)] == [23]
    with pytest.raises(ValueError):
        ds.epoch_ids(0)
    # the iterator collates exactly these lists
    got = list(ds.batches(4, shuffle=True, seed=7, epoch=0))
    assert len(got) == 6
    for ids, out in zip(e0, got):
        _check_batch(out, R.collate_ref(st, ids.tolist()))
    got = list(ds.batches(5, shuffle=False, drop_remainder=True))
    assert [g[0].G for g in got] == [5, 5, 5, 5]
    _check_batch(got[1], R.collate_ref(st, [5, 6, 7, 8, 9]))
    # a view iterates over its own records
    train, val = ds.split(0.25)
    assert val.record_ids.tolist() == [0, 1, 2, 3, 4]
    seen = np.concatenate([train.record_ids[c] for c in train.epoch_ids(4, seed=1, epoch=2)])
    assert sorted(seen.tolist()) == list(range(5, 23))
