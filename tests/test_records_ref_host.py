"""Record sets from structures and shift tables, on the host: the NumPy statements of the two kernels
(tests/records_ref.py) against cases written out by hand, ``ShiftDataset.from_structures`` on a CPU device against
``from_records`` over ``universe2graph`` tuples plus labels, the label join and its refusals, the name table, the shift-table
reader, ``standards()`` and the standards' way through ``save`` / ``load_model``."""
import json
import os

import numpy as np
import pytest

import records_ref as RR

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
PDB1, PDB10 = os.path.join(DATA, "108M.pdb"), os.path.join(DATA, "7lgi.pdb.gz")
NAN = float("nan")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---------------------------------------------------------------------------------------------- the refs, by hand
def _hand_batch():
    """two structures: 3 atoms (rows 0-2) and 1 atom (row 3), K = 3"""
    gp = np.array([0, 3, 4], np.int32)
    atoms = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float32)
    nlist = np.array([[1, 2, 0],      # row 0: neighbours 1, 2, padding
                      [0, 2, 1],      # row 1: local index 0 (never counted in the degree), 2, and a -0.0 edge
                      [1, 0, 3],      # row 2: 1, a NaN edge, and a live slot that points into the OTHER structure
                      [3, 3, 3]], np.int32)   # row 3: the one-atom structure, padding only
    edges = np.array([[0.1, 0.2, 0.0],
                      [0.3, 0.4, -0.0],
                      [0.5, NAN, 0.6],
                      [0.0, 0.0, 0.0]], np.float32)
    shift = np.array([8.25, NAN, np.inf, -3.5], np.float32)
    name_id = np.array([5, 0, 2 ** 24 - 1, 7], np.int32)
    return gp, atoms, nlist, edges, shift, name_id


def test_store_from_batch_ref_by_hand():
    ref = RR.store_from_batch_ref(*_hand_batch())
    assert ref["nlist"].tolist() == [[1, 2, 0], [0, 2, 0], [1, 0, 0], [0, 0, 0]]
    want_e = np.array([[0.1, 0.2, 0], [0.3, 0.4, 0], [0.5, 0, 0], [0, 0, 0]], np.float32)
    assert np.array_equal(_bits(ref["edges"]), _bits(want_e))          # +0.0 bits: neither -0.0 nor NaN survives
    # row 1 keeps its live slot at local index 0, but the degree counts nlist > 0 only: 1 slot -> 1.0
    assert ref["inv_degree"].tolist() == [0.5, 1.0, 1.0, 0.0]
    assert ref["y"].tolist() == [[8.25, 5.0, 1.0], [0.0, 0.0, 0.0], [0.0, float(2 ** 24 - 1), 0.0], [-3.5, 7.0, 1.0]]
    assert ref["w"].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert ref["counters"].tolist() == [1, 2]
    assert ref["atoms"].tolist() == _hand_batch()[1].tolist()


def test_store_from_batch_ref_inv_degree_is_inv_degree_of():
    from nmrgnn_amd.structure import inv_degree_of
    rng = np.random.default_rng(3)
    gp = np.array([0, 40, 41, 100], np.int32)
    g = np.searchsorted(gp, np.arange(100), side="right") - 1
    nlist = (gp[g][:, None] + rng.integers(0, (gp[g + 1] - gp[g])[:, None], size=(100, 16))).astype(np.int32)
    edges = np.where(rng.random((100, 16)) < 0.7, rng.uniform(0.1, 0.4, (100, 16)), 0).astype(np.float32)
    ref = RR.store_from_batch_ref(gp, np.ones((100, 2), np.float32), nlist, edges, np.zeros(100, np.float32),
                                  np.zeros(100, np.int32))
    assert ref["counters"][0] == 0
    assert np.array_equal(_bits(ref["inv_degree"]), _bits(inv_degree_of(ref["nlist"])))


def test_label_moments_ref_by_hand():
    atoms = np.array([[0, 1, 0], [0, 1, 0], [0, 0, 2], [0, 0, 0], [0, 1, 0], [3, 1, 0]], np.float32)
    y = np.array([[2, 0, 1], [4, 0, 1], [10, 0, 1], [7, 0, 1], [100, 0, 0], [-1.5, 0, 1]], np.float32)
    rec_ptr = np.array([0, 2, 5, 6], np.int64)
    out = RR.label_moments_ref(atoms, y, rec_ptr, [0, 1, 2])
    # element 1: rows 0, 1 (row 4 has no label); element 2: row 2; row 3 has no element; element 0: row 5 (first non-zero)
    assert out.tolist() == [[1, -1.5, 2.25], [2, 6, 20], [1, 10, 100]]
    assert RR.label_moments_ref(atoms, y, rec_ptr, [0, 7, -1]).tolist() == [[0, 0, 0], [2, 6, 20], [0, 0, 0]]
    assert RR.label_moments_ref(atoms, y, rec_ptr, [0, 0]).tolist() == [[0, 0, 0], [4, 12, 40], [0, 0, 0]]
    assert RR.label_moments_ref(atoms, y, rec_ptr, []).tolist() == [[0, 0, 0]] * 3
    from nmrgnn_amd.dataset import label_moments_host
    assert np.array_equal(label_moments_host(atoms, y), out)


# ---------------------------------------------------------------------------------------------- tables and names
def test_read_shift_table(tmp_path):
    from nmrgnn_amd.structure import read_shift_table
    p = tmp_path / "t.csv"
    p.write_text("Name, shift ,resid,note\nCA,56.25,3,x\n H , ,4,\nN,n/a,5,y\n\nHA,inf,6,\nCB,-1.5e1,7,z\n")
    t = read_shift_table(str(p))
    assert t["resid"].tolist() == [3, 4, 5, 6, 7] and t["resid"].dtype == np.int64
    assert t["name"].tolist() == ["CA", "H", "N", "HA", "CB"]
    assert t["shift"].dtype == np.float32 and t["resname"] is None
    assert np.array_equal(np.isnan(t["shift"]), [False, True, True, True, False])       # blank, text, non-finite: no label
    assert t["shift"][0] == 56.25 and t["shift"][4] == -15.0
    q = tmp_path / "r.csv"
    q.write_text("resid,name,shift,resname\n1,N,120.5,ALA\n")
    assert read_shift_table(str(q))["resname"].tolist() == ["ALA"]
    (tmp_path / "bad.csv").write_text("resid,atom,shift\n1,N,2\n")
    with pytest.raises(ValueError, match="name"):
        read_shift_table(str(tmp_path / "bad.csv"))
    (tmp_path / "bad2.csv").write_text("resid,name,shift\nx,N,2\n")
    with pytest.raises(ValueError, match="line 2"):
        read_shift_table(str(tmp_path / "bad2.csv"))
    (tmp_path / "empty.csv").write_text("")
    with pytest.raises(ValueError, match="empty"):
        read_shift_table(str(tmp_path / "empty.csv"))


def _tiny(names=("N", "CA", "HA", "C"), resnames=("ALA", "ALA", "GLY", "GLY"), resids=(1, 1, 2, 2), frames=1, seed=0):
    from nmrgnn_amd.structure import Structure
    rng = np.random.default_rng(seed)
    el = [n[0] for n in names]
    return Structure(list(names), list(resnames), list(resids), el, [rng.uniform(0, 5, (len(names), 3)) for _ in range(frames)])


def test_name_table_order_and_id_0():
    from nmrgnn_amd.structure import MAX_NAME_IDS, name_ids, name_keys, name_table
    a = _tiny()
    b = _tiny(names=("N", "X1"), resnames=("ZZZ", "ALA"), resids=(1, 2))
    assert name_keys(a) == ["ALA-N", "ALA-CA", "GLY-HA", "GLY-C"]
    t = name_table([a, b])
    assert t == {"X": 0, "ALA-CA": 1, "ALA-N": 2, "ALA-X1": 3, "GLY-C": 4, "GLY-HA": 5, "ZZZ-N": 6}
    assert list(t)[0] == "X"
    assert all(len(k.split("-")) == 2 for k in t if k != "X")           # the shape nmrgnn/main.py:124-135 splits
    assert name_ids(a, t).tolist() == [2, 1, 5, 4] and name_ids(a, t).dtype == np.int32
    assert name_ids(b, name_table([a])).tolist() == [0, 0]              # keys the table lacks: 'X'
    assert MAX_NAME_IDS == 2 ** 24
    with pytest.raises(ValueError, match="2\\^24"):
        name_ids(a, {"ALA-N": 2 ** 24})


def test_name_table_refuses_more_than_2_24_ids(monkeypatch):
    from nmrgnn_amd import structure
    monkeypatch.setattr(structure, "MAX_NAME_IDS", 4)
    with pytest.raises(ValueError, match="name ids"):
        structure.name_table([_tiny()])                                 # 4 keys + 'X'
    assert len(structure.name_table([_tiny(names=("N", "CA", "C"), resnames=("A",) * 3, resids=(1, 1, 1))])) == 4


def _table(rows, resname=None):
    return {"resid": np.asarray([r[0] for r in rows], np.int64), "name": np.asarray([r[1] for r in rows], dtype=str),
            "shift": np.asarray([r[2] for r in rows], np.float32),
            "resname": None if resname is None else np.asarray(resname, dtype=str)}


def test_join_refusals_and_report():
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.structure import join_shifts
    s = _tiny(names=("N", "CA", "CA", "C"), resids=(1, 1, 1, 2))
    sh, rep = join_shifts(s, _table([(1, "N", 118.5), (2, "C", 176.0)]))
    assert np.array_equal(np.isnan(sh), [False, True, True, False]) and sh[0] == 118.5 and sh[3] == 176.0
    assert not any(rep.values())
    assert np.array_equal(_bits(sh), _bits(RR.join_ref(s.resids, s.names, [(1, "N", 118.5), (2, "C", 176.0)])))
    with pytest.raises(ValueError, match=r"mol-7.*row 1 \(resid 3, name N\).*no atom"):
        join_shifts(s, _table([(1, "N", 1.0), (3, "N", 2.0)]), label="mol-7")
    with pytest.raises(ValueError, match=r"row 0 \(resid 1, name CA\).*2 atoms"):
        join_shifts(s, _table([(1, "CA", 1.0)]))
    with pytest.raises(ValueError, match="GLY"):
        join_shifts(s, _table([(1, "N", 1.0)], resname=["GLY"]))
    with pytest.raises(ValueError, match="earlier row"):
        join_shifts(s, _table([(1, "N", 1.0), (1, "N", 2.0)]))
    rows = [(1, "N", 1.0), (3, "N", 2.0), (1, "CA", 3.0), (1, "N", 4.0), (2, "C", 5.0), (9, "Q", 6.0)]
    sh, rep = join_shifts(s, _table(rows, resname=["ALA", "ALA", "ALA", "ALA", "ALA", "ALA"]), strict=False)
    assert rep == {"unmatched": 2, "ambiguous": 1, "duplicate": 1, "resname_mismatch": 1}
    assert sh[0] == 1.0 and np.isnan(sh[1:]).all()
    # through from_structures: the structure is named, and the report lands on the store
    with pytest.raises(ValueError, match=r"structure 1: shift table row 0"):
        ShiftDataset.from_structures([_tiny(), s], [None, _table([(5, "N", 1.0)])], neighbor_number=3, device="cpu")
    ds = ShiftDataset.from_structures([_tiny(), s], [None, _table(rows)], neighbor_number=3, strict=False, device="cpu")
    assert ds.join_report == {"structures": 2, "rows": 6, "unmatched": 2, "ambiguous": 1, "duplicate": 1,
                              "resname_mismatch": 0, "labelled": 2}
    train, _ = ds.split(0.0)
    assert train.join_report is ds.join_report and train.name_table is ds.name_table
    with pytest.raises(ValueError, match="2 structures but 1"):
        ShiftDataset.from_structures([_tiny(), s], [None], device="cpu")
    with pytest.raises(ValueError, match="frames"):
        ShiftDataset.from_structures([s], [None], frames="some", device="cpu")


# ---------------------------------------------------------------------------------------------- from_structures on the CPU
def test_from_structures_cpu_equals_from_records_over_universe2graph(tmp_path):
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.library import universe2graph
    from nmrgnn_amd.structure import name_ids, name_table, read_pdb
    structs = [read_pdb(PDB1), read_pdb(PDB10)]
    assert [len(s) for s in structs] == [1, 10]
    rows = [RR.synthetic_labels(s, seed=k) for k, s in enumerate(structs)]
    paths = [RR.write_table(str(tmp_path / f"t{k}.csv"), rows[k], s if k == 0 else None) for k, s in enumerate(structs)]
    ds = ShiftDataset.from_structures([PDB1, PDB10], paths, frames="all", device="cpu")
    table = name_table(structs)
    assert ds.name_table == table and ds.file_ptr.tolist() == [0, 11] and ds.R == 11 and ds.K == 16 and ds.C == 10
    records = []
    for k, s in enumerate(structs):
        sh = RR.join_ref(s.resids, s.names, rows[k])
        has = np.isfinite(sh)
        y = np.stack([np.where(has, sh, 0), name_ids(s, table).astype(np.float32), has], axis=1).astype(np.float32)
        for _ in s.trajectory():
            records.append((universe2graph(s), y, has.astype(np.float32)))
    want = ShiftDataset.from_records(records, device="cpu")
    assert np.array_equal(ds.rec_ptr_host, want.rec_ptr_host)
    for k in ("atoms", "nlist", "edges", "inv_degree", "y", "w"):
        a, b = getattr(ds, k).numpy(), getattr(want, k).numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k
    assert ds.join_report["labelled"] == sum(len(r) * len(s) for r, s in zip(rows, structs)) > 1000
    # the frames of the second structure differ in their lists and share their labels
    r1, r2 = int(ds.rec_ptr_host[1]), int(ds.rec_ptr_host[2])
    assert not np.array_equal(ds.edges[r1:r2].numpy(), ds.edges[r2:r2 + (r2 - r1)].numpy())
    assert np.array_equal(ds.y[r1:r2].numpy(), ds.y[r2:r2 + (r2 - r1)].numpy())
    first = ShiftDataset.from_structures(structs, paths, device="cpu")      # Structure objects, frames='first'
    assert first.R == 2 and np.array_equal(_bits(first.edges.numpy()), _bits(ds.edges[:r2].numpy()))
    # file round trip: layout and version unchanged
    ds.save(str(tmp_path / "s.npz"))
    with np.load(str(tmp_path / "s.npz")) as z:
        assert sorted(z.files) == sorted(["atoms", "nlist", "edges", "inv_degree", "y", "w", "rec_ptr", "file_ptr", "format_version"])
        assert int(z["format_version"]) == 1
    back = ShiftDataset.load(str(tmp_path / "s.npz"), device="cpu")
    assert np.array_equal(_bits(back.y.numpy()), _bits(ds.y.numpy()))


def test_from_structures_cpu_zeroes_slots_without_a_distance():
    """two coincident atoms: the slot between them has distance 0, so it is padding in the store"""
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.structure import Structure, inv_degree_of
    pos = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    s = Structure(["N", "CA", "C", "O"], ["ALA"] * 4, [1] * 4, ["N", "C", "C", "O"], [pos])
    ds = ShiftDataset.from_structures([s], [None], neighbor_number=3, device="cpu")
    e, nl = ds.edges.numpy(), ds.nlist.numpy()
    assert (e[0] > 0).sum() == 2 and (e[1] > 0).sum() == 2 and (e[2:] > 0).all()
    assert (nl[e == 0] == 0).all() and np.array_equal(ds.inv_degree.numpy(), inv_degree_of(nl))
    assert float(ds.w.sum()) == 0 and ds.join_report["labelled"] == 0


# ---------------------------------------------------------------------------------------------- standards
def test_standards_against_numpy():
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.standards import ELEMENTS, load_standards
    import collate_ref as CR
    recs = CR.make_records([30, 1, 17, 64, 5, 40], K=4, C=10, seed=9, onehot=True)
    rng = np.random.default_rng(1)
    for (x, y, w) in recs:
        y[:, 0] = rng.normal(100.0, 20.0, len(y)).astype(np.float32)
    ds = ShiftDataset.from_records(recs, device="cpu")
    train, val = ds.split(0.34)
    assert len(val) == 2 and len(train) == 4
    for view, ids in ((ds, range(6)), (train, [2, 3, 4, 5]), (val, [0, 1])):
        atoms = np.concatenate([recs[i][0][0] for i in ids])
        y = np.concatenate([recs[i][1] for i in ids])
        got = view.standards()
        assert sorted(got) == list(range(10)) and sorted(load_standards()) == list(range(10))
        for c in range(10):
            sel = (y[:, 2] > 0) & (atoms[:, c] != 0)
            v = y[sel, 0].astype(np.float64)
            assert got[c][0] == ELEMENTS[c] == load_standards()[c][0]
            if len(v) < 2:
                assert got[c][1:] == (0.0, 0.0)
            else:
                assert got[c][1] == pytest.approx(v.mean(), rel=1e-12) and got[c][2] == pytest.approx(v.std(), rel=1e-9)
                assert isinstance(got[c][1], float) and isinstance(got[c][2], float)
    assert train.standards() != ds.standards()


def test_standards_std_is_never_negative_under_the_root():
    from nmrgnn_amd.dataset import ShiftDataset
    n = 50
    atoms = np.zeros((n, 10), np.float32)
    atoms[:, 4] = 1
    y = np.stack([np.full(n, 8.1, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32)], axis=1)
    rec = ((atoms, np.zeros((n, 2), np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32)), y, np.ones(n, np.float32))
    st = ShiftDataset.from_records([rec], device="cpu").standards()
    assert st[4][1] == pytest.approx(float(np.float32(8.1))) and 0.0 <= st[4][2] < 1e-6
    assert st[2] == ("C", 0.0, 0.0)


def test_peak_standards_reach_the_model_and_its_config():
    """build_GNNModel(peak_standards=) sets the model's tables; the engine-free half of the save / load_model round trip
    (the GPU file does the rest): get_config and the json that save writes from it"""
    from nmrgnn_amd.model import build_GNNModel
    from nmrgnn_amd.standards import load_standards
    st = {c: (s, 0.0, 0.0) for c, (s, _, _) in load_standards().items()}
    st[7] = ("P", 3.25, 1.5)
    st[4] = ("H", 8.0, 0.5)
    m = build_GNNModel(device="cpu", peak_standards=st)
    assert m.peak_standards == st and m.peak_avg[7] == 3.25 and m.peak_std[7] == 1.5 and m.peak_std[4] == 0.5
    assert m.peak_std[2] == 0.0                                     # not the bundled C
    cfg = json.loads(json.dumps({str(k): list(v) for k, v in m.get_config()["peak_standards"].items()}))
    assert {int(k): tuple(v) for k, v in cfg.items()} == st
    d = build_GNNModel(device="cpu")
    assert d.peak_standards == load_standards() and d.peak_std[7] == 0.0


def test_make_records_cli_on_the_cpu(tmp_path):
    """make-records end to end with --device cpu (training needs the GPU: tests/test_gpu_records.py runs the chain)"""
    from click.testing import CliRunner
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.main import _load_embeddings, main
    from nmrgnn_amd.structure import name_table, read_pdb
    s = read_pdb(PDB10)
    rows = RR.synthetic_labels(s, seed=5)
    t = RR.write_table(str(tmp_path / "t.csv"), rows)
    out, emb = str(tmp_path / "r.npz"), str(tmp_path / "emb.json")
    res = CliRunner().invoke(main, ["make-records", out, "--pair", PDB10, t, "--frames", "all", "--neighbor-number", "8",
                                    "--embeddings-out", emb, "--device", "cpu"])
    assert res.exit_code == 0, res.output
    ds = ShiftDataset.load(out, device="cpu")
    assert ds.R == 10 and ds.K == 8 and int(ds.w.sum()) == 10 * len(rows)
    e = _load_embeddings(emb)
    assert e["name"] == name_table([s]) and e["atom"]["H"] == 4
    # the table of an embeddings file: ids from it, keys it lacks -> 0
    with open(emb, "w") as f:
        json.dump({"name": {"X": 0, "ALA-CA": 41}}, f)
    out2 = str(tmp_path / "r2.npz")
    res = CliRunner().invoke(main, ["make-records", out2, "--pair", PDB10, t, "--embeddings", emb, "--device", "cpu"])
    assert res.exit_code == 0, res.output
    assert set(np.unique(ShiftDataset.load(out2, device="cpu").y[:, 1].numpy()).tolist()) == {0.0, 41.0}
    # a row that joins nothing: an error message, or a count with --keep-going
    bad = RR.write_table(str(tmp_path / "bad.csv"), rows + [(99999, "QQ", 1.0)])
    res = CliRunner().invoke(main, ["make-records", out2, "--pair", PDB10, bad, "--device", "cpu"])
    assert res.exit_code != 0 and "resid 99999" in res.output
    res = CliRunner().invoke(main, ["make-records", out2, "--pair", PDB10, bad, "--keep-going", "--device", "cpu"])
    assert res.exit_code == 0 and "unmatched: 1" in res.output
    assert CliRunner().invoke(main, ["make-records", out2]).exit_code != 0
