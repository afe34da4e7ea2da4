"""Binary trajectory readers, writers and the host stream of nmrgnn_amd.trajectory against independent tools: DCD bytes built
with struct / NumPy and read back with scipy.io.FortranFile, NetCDF files written and read by scipy.io.netcdf_file
(tests/traj_ref.py).  No GPU."""
import os
import sys
import warnings

import numpy as np
import pytest

from traj_ref import cell_record, dcd_bytes, write_dcd_ref, write_netcdf_ref

HERE = os.path.dirname(os.path.abspath(__file__))
PDB10 = os.path.join(HERE, "data", "7lgi.pdb.gz")

T, N = 7, 13


def _frames(T=T, n=N, seed=0):
    fr = np.random.default_rng(seed).normal(scale=20.0, size=(T, n, 3)).astype(np.float32)
    w = fr.view(np.uint32)
    w[0, 0, 0], w[0, 1, 1], w[-1, -1, 2] = 0x80000000, 0x00000001, 0x807fffff      # -0.0 and two subnormals
    return fr


def _dims(T=T):
    d = np.tile(np.array([31.5, 42.25, 53.125, 90.0, 100.5, 61.25]), (T, 1))
    d[:, 0] += np.arange(T)
    return d


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def _open(path):
    from nmrgnn_amd.trajectory import open_trajectory
    return open_trajectory(str(path))


# ---------------------------------------------------------------------------------------------------------------- DCD
@pytest.mark.parametrize("big", [False, True], ids=["little", "big"])
@pytest.mark.parametrize("cell", [False, True], ids=["nocell", "cell"])
@pytest.mark.parametrize("fourth", [False, True], ids=["xyz", "xyzw"])
@pytest.mark.parametrize("ntitle", [0, 2])
def test_dcd_forms(tmp_path, big, cell, fourth, ntitle):
    from nmrgnn_amd.trajectory import DCDTrajectory
    fr, d = _frames(), _dims()
    p = tmp_path / "a.bin"          # the suffix says nothing: the reader is chosen by the magic bytes
    write_dcd_ref(p, fr, cells=[cell_record(x) for x in d] if cell else None, big=big, fourth=fourth, ntitle=ntitle)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t = _open(p)
    assert isinstance(t, DCDTrajectory)
    assert (t.n_atoms, t.n_frames, t.has_box, t.big_endian) == (N, T, cell, big)
    _same_bits(t.read(), fr)
    _same_bits(t.read([5, 0, 5]), fr[[5, 0, 5]])
    if cell:
        np.testing.assert_array_equal(t.dimensions(), d)
        np.testing.assert_array_equal(t.dimensions([3]), d[[3]])
    else:
        assert t.dimensions() is None
    lay = t.layout()
    rec = 4 * N + 8
    base = 56 if cell else 0
    assert lay["frame_stride"] == base + (4 if fourth else 3) * rec
    assert lay["off"] == (base + 4, base + rec + 4, base + 2 * rec + 4) and lay["elem_stride"] == 4
    assert lay["first"] == 92 + (12 + 80 * ntitle) + 12
    assert lay["swap"] == int(big != (sys.byteorder == "big"))


def test_dcd_frame_count_comes_from_the_file_size(tmp_path):
    fr = _frames()
    p = tmp_path / "nset.dcd"
    write_dcd_ref(p, fr, nset=T + 5)
    with pytest.warns(RuntimeWarning, match=f"announces {T + 5} frames"):
        t = _open(p)
    assert t.n_frames == T
    _same_bits(t.read(), fr)
    write_dcd_ref(p, fr, nset=0)        # a writer that never went back to the header
    with pytest.warns(RuntimeWarning, match="announces 0 frames"):
        assert _open(p).n_frames == T


def test_dcd_truncated_last_frame_is_dropped(tmp_path):
    fr = _frames()
    p = tmp_path / "cut.dcd"
    write_dcd_ref(p, fr, cut=20)
    with pytest.warns(RuntimeWarning, match="truncated"):
        t = _open(p)
    assert t.n_frames == T - 1
    _same_bits(t.read(), fr[:-1])
    with pytest.raises(IndexError):
        t.read([T - 1])


def test_dcd_cell_cosines_and_degrees(tmp_path):
    fr = _frames(T=4)
    # frame 0: cosines (NAMD); 1: degrees; 2: degrees of a box with one angle of exactly 1 degree — two of three lie outside
    # [-1, 1], so none is a cosine; 3: zero lengths, no box
    boxes = np.array([[30.0, 40.0, 50.0, 90.0, 75.0, 120.0],
                      [30.0, 40.0, 50.0, 90.0, 75.0, 120.0],
                      [30.0, 40.0, 50.0, 1.0, 89.5, 90.0],
                      [0.0, 0.0, 0.0, 90.0, 90.0, 90.0]])
    cells = [cell_record(boxes[0], cosines=True), cell_record(boxes[1]), cell_record(boxes[2]), cell_record(boxes[3])]
    p = tmp_path / "cell.dcd"
    write_dcd_ref(p, fr, cells=cells)
    d = _open(p).dimensions()
    np.testing.assert_array_equal(d[1], boxes[1])
    np.testing.assert_array_equal(d[2], boxes[2])
    np.testing.assert_array_equal(d[0, :3], boxes[0, :3])
    # 90 - asin(cos(x)) in float64: a few ulp of 90
    np.testing.assert_allclose(d[0, 3:], boxes[0, 3:], rtol=0, atol=1e-12)
    assert np.isnan(d[3]).all()
    assert _open(p).dimensions([3, 1])[1, 5] == 120.0


def test_dcd_refusals(tmp_path):
    from nmrgnn_amd.trajectory import TrajectoryError
    fr = _frames(T=2)
    p = tmp_path / "bad.dcd"
    p.write_bytes(dcd_bytes(fr, wide_markers=True))
    with pytest.raises(TrajectoryError, match="64-bit record markers"):
        _open(p)
    p.write_bytes(dcd_bytes(fr, wide_markers=True, big=True))
    with pytest.raises(TrajectoryError, match="64-bit record markers"):
        _open(p)
    p.write_bytes(dcd_bytes(fr, fixed=3))
    with pytest.raises(TrajectoryError, match="fixed atoms"):
        _open(p)
    blob = bytearray(dcd_bytes(fr))
    blob[0:4] = (85).to_bytes(4, "little")
    p.write_bytes(bytes(blob))
    with pytest.raises(TrajectoryError, match="84 in neither byte order"):
        _open(p)


@pytest.mark.parametrize("big", [False, True], ids=["little", "big"])
@pytest.mark.parametrize("cell", [False, True], ids=["nocell", "cell"])
def test_write_dcd_read_back_with_fortranfile(tmp_path, big, cell):
    from scipy.io import FortranFile
    from nmrgnn_amd.trajectory import write_dcd
    fr, d = _frames(), _dims()
    p = tmp_path / "w.dcd"
    write_dcd(str(p), fr, d if cell else None, big_endian=big)
    e = ">" if big else "<"
    f = FortranFile(str(p), "r", header_dtype=np.dtype(e + "u4"))
    head = f.read_record(np.dtype([("cord", "S4"), ("icntrl", e + "i4", (20,))]))
    ic = head["icntrl"][0]
    assert head["cord"][0] == b"CORD" and ic[0] == T and ic[8] == 0 and bool(ic[10]) == cell and ic[11] == 0 and ic[19] != 0
    title = f.read_record(np.uint8)
    ntitle = int(title[:4].view(e + "i4")[0])
    assert len(title) == 4 + 80 * ntitle
    assert f.read_ints(e + "i4")[0] == N
    for t in range(T):
        if cell:
            c = f.read_reals(e + "f8")
            np.testing.assert_array_equal(c, cell_record(d[t]))
        for k in range(3):
            got = f.read_record(e + "u4").astype(np.uint32)
            np.testing.assert_array_equal(got, fr[t, :, k].view(np.uint32))
    with pytest.raises(Exception):      # nothing behind the last frame
        f.read_record(np.uint8)
    f.close()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t = _open(p)
    _same_bits(t.read(), fr)
    if cell:
        np.testing.assert_array_equal(t.dimensions(), d)


# ------------------------------------------------------------------------------------------------------------- NetCDF
@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("extra", [((), ()), (("time", "velocities"), ("forces",))], ids=["alone", "among-others"])
@pytest.mark.parametrize("cell", [False, True], ids=["nocell", "cell"])
def test_netcdf_forms(tmp_path, version, extra, cell):
    from scipy.io import netcdf_file
    from nmrgnn_amd.trajectory import NetCDFTrajectory
    fr, d = _frames(), _dims()
    p = tmp_path / "a.bin"
    write_netcdf_ref(p, fr, d if cell else None, version=version, before=extra[0], after=extra[1])
    assert p.read_bytes()[:4] == b"CDF" + bytes([version])
    t = _open(p)
    assert isinstance(t, NetCDFTrajectory)
    assert (t.n_atoms, t.n_frames, t.has_box) == (N, T, cell)
    f = netcdf_file(str(p), "r", mmap=False)
    theirs = np.array(f.variables["coordinates"][:], dtype=np.float32)
    f.close()
    _same_bits(t.read(), theirs)
    _same_bits(t.read(), fr)
    _same_bits(t.read([6, 2]), fr[[6, 2]])
    lay = t.layout()
    assert lay["elem_stride"] == 12 and lay["off"][1] == lay["off"][0] + 4 and lay["off"][2] == lay["off"][0] + 8
    record = 12 * N + (4 + 12 * N + 12 * N if extra[0] else 0) + (48 if cell else 0)
    assert lay["frame_stride"] == record
    if extra[0]:
        assert lay["off"][0] == 4 + 12 * N      # time and velocities lie in front of the coordinates
    if cell:
        np.testing.assert_array_equal(t.dimensions(), d)
    else:
        assert t.dimensions() is None


def test_netcdf_zero_frames(tmp_path):
    p = tmp_path / "empty.nc"
    write_netcdf_ref(p, np.zeros((0, N, 3), np.float32), before=("time",))
    t = _open(p)
    assert (t.n_atoms, t.n_frames) == (N, 0)
    assert t.read().shape == (0, N, 3)
    from nmrgnn_amd.trajectory import TrajectoryStream
    assert list(TrajectoryStream(t, device="cpu")) == []


@pytest.mark.parametrize("cell", [False, True], ids=["nocell", "cell"])
def test_write_netcdf_read_back_with_scipy(tmp_path, cell):
    from scipy.io import netcdf_file
    from nmrgnn_amd.trajectory import write_netcdf
    fr, d = _frames(), _dims()
    p = tmp_path / "w.nc"
    write_netcdf(str(p), fr, d if cell else None)
    f = netcdf_file(str(p), "r", mmap=False)
    assert f.Conventions == b"AMBER"
    assert f.dimensions["frame"] is None and f.dimensions["atom"] == N and f.dimensions["spatial"] == 3
    co = f.variables["coordinates"]
    assert co.dimensions == ("frame", "atom", "spatial") and co.units == b"angstrom"
    _same_bits(np.array(co[:], dtype=np.float32), fr)
    np.testing.assert_array_equal(f.variables["time"][:], np.arange(T, dtype=np.float32))
    if cell:
        np.testing.assert_array_equal(f.variables["cell_lengths"][:], d[:, :3])
        np.testing.assert_array_equal(f.variables["cell_angles"][:], d[:, 3:])
    else:
        assert "cell_lengths" not in f.variables
    f.close()
    t = _open(p)
    _same_bits(t.read(), fr)
    if cell:
        np.testing.assert_array_equal(t.dimensions(), d)


def test_netcdf_refusals(tmp_path):
    from nmrgnn_amd.trajectory import TrajectoryError
    fr = _frames(T=2)
    p = tmp_path / "bad.nc"
    p.write_bytes(b"\x89HDF\r\n\x1a\n" + bytes(64))
    with pytest.raises(TrajectoryError, match="NetCDF-4 trajectories must be converted to NetCDF-3"):
        _open(p)
    write_netcdf_ref(p, fr, scale_factor=0.5)
    with pytest.raises(TrajectoryError, match="scale_factor"):
        _open(p)
    write_netcdf_ref(p, fr, scale_factor=1.0)
    assert _open(p).n_frames == 2
    write_netcdf_ref(p, fr, coordinates="positions")
    with pytest.raises(TrajectoryError, match="no 'coordinates' variable"):
        _open(p)
    write_netcdf_ref(p, fr, spatial=2)
    with pytest.raises(TrajectoryError, match="spatial"):
        _open(p)


# ------------------------------------------------------------------------------------------------- stream on the CPU
def _collect(stream):
    ids, pos, dims = [], [], []
    for i, p, d in stream:
        assert p.shape[0] == len(i)
        ids.append(np.asarray(i))
        pos.append(p.numpy())
        dims.append(d)
    return ids, pos, dims


@pytest.mark.parametrize("fmt", ["dcd", "nc"])
def test_stream_on_the_cpu_device(tmp_path, fmt):
    from nmrgnn_amd.trajectory import TrajectoryStream
    fr, d = _frames(T=11, seed=4), _dims(11)
    p = tmp_path / ("s." + fmt)
    if fmt == "dcd":
        write_dcd_ref(p, fr, cells=[cell_record(x) for x in d], big=True)
    else:
        write_netcdf_ref(p, fr, d, before=("time",))
    t = _open(p)
    ref = t.read()
    _same_bits(ref, fr)
    for stride, chunk in ((1, 4), (3, 2), (1, 64), (1, 11), (3, 1)):
        ids, pos, dims = _collect(TrajectoryStream(t, stride=stride, chunk_frames=chunk, device="cpu"))
        want = np.arange(0, 11, stride)
        assert [len(i) for i in ids] == [min(chunk, len(want) - k) for k in range(0, len(want), chunk)]
        np.testing.assert_array_equal(np.concatenate(ids), want)
        _same_bits(np.concatenate(pos), ref[want])
        np.testing.assert_array_equal(np.concatenate(dims), d[want])
    sub = [9, 2, 2, 7, 0]
    ids, pos, _ = _collect(TrajectoryStream(t, frames=sub, chunk_frames=2, device="cpu"))
    np.testing.assert_array_equal(np.concatenate(ids), sub)
    _same_bits(np.concatenate(pos), ref[sub])
    ids, pos, _ = _collect(TrajectoryStream(t, frames=sub, stride=2, chunk_frames=2, device="cpu"))
    np.testing.assert_array_equal(np.concatenate(ids), sub[::2])
    sel = [5, 0, 12, 5, 3]          # permuted, with a repeat
    ids, pos, _ = _collect(TrajectoryStream(t, select=sel, chunk_frames=3, device="cpu"))
    _same_bits(np.concatenate(pos), ref[:, sel])
    mask = np.zeros(N, bool)
    mask[[1, 4]] = True
    _, pos, _ = _collect(TrajectoryStream(t, select=mask, device="cpu"))
    _same_bits(np.concatenate(pos), ref[:, [1, 4]])
    with pytest.raises(IndexError):
        TrajectoryStream(t, select=[0, N], device="cpu")
    with pytest.raises(IndexError):
        TrajectoryStream(t, frames=[11], device="cpu")


# ---------------------------------------------------------------------------------------------------- _open_structure
def test_open_structure_with_binary_trajectories(tmp_path):
    from nmrgnn_amd.main import _open_structure, eval_structure
    from nmrgnn_amd.structure import Structure, read_pdb
    from nmrgnn_amd.trajectory import load_structure
    s = read_pdb(PDB10)
    fr = np.stack(s.frames)[[7, 3, 5]] + np.float32(0.25)
    dcd, nc = tmp_path / "t.dcd", tmp_path / "t.nc"
    write_dcd_ref(dcd, fr)
    write_netcdf_ref(nc, fr[:2])
    u = _open_structure([PDB10, str(dcd)])
    assert len(u) == 3 and u.n_atoms == s.n_atoms          # the DCD's frames only: the topology gives the names
    assert list(u.names) == list(s.names) and list(u.resids) == list(s.resids)
    for k in range(3):
        _same_bits(u.frames[k], fr[k])
    assert u.dimensions == [None] * 3
    u = _open_structure([PDB10, str(dcd), str(nc)])         # trajectory files in order
    assert len(u) == 5
    _same_bits(u.frames[3], fr[0])
    _same_bits(u.frames[4], fr[1])
    ls = load_structure(PDB10, str(dcd), str(nc), stride=2)
    assert isinstance(ls, Structure) and len(ls) == 3
    _same_bits(np.stack(ls.frames), np.concatenate([fr, fr[:2]])[::2])
    small = tmp_path / "small.dcd"
    write_dcd_ref(small, fr[:, :100])
    with pytest.raises(ValueError, match=f"100 atoms, but .* has {s.n_atoms}"):
        _open_structure([PDB10, str(small)])
    with pytest.raises(ValueError, match="cannot be mixed"):
        _open_structure([PDB10, str(dcd), PDB10])
    with pytest.raises(ValueError, match="cannot be mixed"):
        _open_structure([PDB10, PDB10, str(nc)])
    with pytest.raises(ValueError, match="--separate takes PDB files"):
        eval_structure([PDB10, str(dcd)], str(tmp_path / "x.csv"), separate=True)
    from click.testing import CliRunner
    from nmrgnn_amd.main import main
    res = CliRunner().invoke(main, ["eval-struct", "--separate", PDB10, str(dcd), str(tmp_path / "x.csv")])
    assert res.exit_code != 0 and "--separate takes PDB files" in res.output
    # PDB-only calls are what they were
    one, two = _open_structure([PDB10]), _open_structure([PDB10, PDB10])
    assert isinstance(one, Structure) and len(one) == len(s) and len(two) == 2 * len(s)
    _same_bits(np.stack(one.frames), np.stack(s.frames))
    _same_bits(np.stack(two.frames[len(s):]), np.stack(s.frames))


# ------------------------------------------------------------------------------------------------------- make-records
def test_make_records_takes_a_topology_and_trajectory_files(tmp_path):
    """--pair top.pdb,traj.dcd,more.nc: the store of the same frames given as a PDB (--device cpu)"""
    import csv
    from click.testing import CliRunner
    from nmrgnn_amd.dataset import ShiftDataset
    from nmrgnn_amd.main import main
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(PDB10)
    fr = np.stack(s.frames)
    dcd, nc = tmp_path / "a.dcd", tmp_path / "b.nc"
    write_dcd_ref(dcd, fr[:6], big=True)
    write_netcdf_ref(nc, fr[6:], before=("time",))
    keys = list(zip(np.asarray(s.resids).tolist(), [str(x) for x in s.names]))
    table = tmp_path / "t.csv"
    with open(table, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["resid", "name", "shift"])
        for k in range(0, s.n_atoms, 7):
            if keys.count(keys[k]) == 1:
                wr.writerow([keys[k][0], keys[k][1], f"{1.0 + 0.01 * k:.2f}"])
    common = ["--frames", "all", "--ensembles", "--neighbor-number", "8", "--device", "cpu"]
    ref, out = str(tmp_path / "ref.npz"), str(tmp_path / "out.npz")
    res = CliRunner().invoke(main, ["make-records", ref, "--pair", PDB10, str(table)] + common)
    assert res.exit_code == 0, res.output
    res = CliRunner().invoke(main, ["make-records", out, "--pair", f"{PDB10},{dcd},{nc}", str(table)] + common)
    assert res.exit_code == 0, res.output
    a, b = ShiftDataset.load(ref, device="cpu"), ShiftDataset.load(out, device="cpu")
    assert a.R == b.R == 10 and list(a.group_ptr) == list(b.group_ptr) == [0, 10]
    for k in ("atoms", "nlist", "edges", "inv_degree", "y", "w"):
        assert np.array_equal(getattr(a, k).numpy(), getattr(b, k).numpy()), k
    res = CliRunner().invoke(main, ["make-records", out, "--pair", f"{PDB10},{tmp_path / 'none.dcd'}", str(table)] + common)
    assert res.exit_code != 0 and "does not exist" in res.output
