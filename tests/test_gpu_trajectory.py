"""Binary trajectories on the GPU (nmrgnn_amd.trajectory, csrc/traj.hip): eval-struct from a DCD or NetCDF file writes the CSV
of the same frames given as a PDB, byte for byte; the stream over its two staging buffers against the host reader; the
device consumers (predict_trajectory, reweight_trajectory); a non-finite coordinate.  The files are written by the test-side
builders of tests/traj_ref.py."""
import os

import numpy as np
import pytest
import torch

from helpers import make_hp, randomize_biases
from nmrgnn_amd.trajectory import TrajectoryError, TrajectoryStream, open_trajectory
from traj_ref import cell_record, write_dcd_ref, write_netcdf_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PDB10 = os.path.join(HERE, "data", "7lgi.pdb.gz")
QUIET = dict(keep_going=True, echo=lambda *a: None)
KINDS = ["dcd-little", "dcd-big", "netcdf"]


def _write(kind, path, frames, dims=None):
    if kind == "netcdf":
        write_netcdf_ref(path, frames, dims, before=("time",))
    else:
        write_dcd_ref(path, frames, cells=None if dims is None else [cell_record(d) for d in dims], big=kind == "dcd-big")
    return str(path)


def _same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------- the same CSV as the PDB
VARIANTS = {"plain": {}, "average": dict(average=True), "stride": dict(stride=3, frames_per_batch=3),
            "names": dict(atom_names=["H", "N", "CA"])}


@pytest.fixture(scope="module")
def pdb_csv(tmp_path_factory):
    """the CSV bytes of every variant from the PDB itself, once for the module"""
    from nmrgnn_amd.main import eval_structure
    d = tmp_path_factory.mktemp("pdb")
    out = {}
    for name, kw in VARIANTS.items():
        eval_structure([PDB10], str(d / f"{name}.csv"), **kw, **QUIET)
        out[name] = (d / f"{name}.csv").read_bytes()
    return out


@pytest.fixture(scope="module")
def frames10():
    from nmrgnn_amd.structure import read_pdb
    return np.stack(read_pdb(PDB10).frames)


@pytest.mark.parametrize("kind", KINDS)
def test_eval_struct_csv_is_that_of_the_pdb(tmp_path, pdb_csv, frames10, kind):
    from nmrgnn_amd.main import eval_structure
    path = _write(kind, tmp_path / ("t.nc" if kind == "netcdf" else "t.dcd"), frames10)
    for name, kw in VARIANTS.items():
        eval_structure([PDB10, path], str(tmp_path / "out.csv"), **kw, **QUIET)
        got = (tmp_path / "out.csv").read_bytes()
        assert got == pdb_csv[name], f"{kind}: the {name} CSV differs from the PDB's"


def test_eval_struct_two_trajectory_files_are_one_trajectory(tmp_path, pdb_csv, frames10):
    """the frames of the files in order; a batch may span two files (7 + 3 frames, 3 per batch)"""
    from nmrgnn_amd.main import eval_structure
    a = _write("dcd-big", tmp_path / "a.dcd", frames10[:7])
    b = _write("netcdf", tmp_path / "b.ncdf", frames10[7:])
    eval_structure([PDB10, a, b], str(tmp_path / "out.csv"), average=True, frames_per_batch=3, **QUIET)
    eval_structure([PDB10], str(tmp_path / "ref.csv"), average=True, frames_per_batch=3, **QUIET)
    assert (tmp_path / "out.csv").read_bytes() == (tmp_path / "ref.csv").read_bytes()
    eval_structure([PDB10, a, b], str(tmp_path / "out.csv"), stride=3, frames_per_batch=3, **QUIET)
    assert (tmp_path / "out.csv").read_bytes() == pdb_csv["stride"]


# ----------------------------------------------------------------------------------------- a small periodic system
def _periodic_system(T=5):
    """343 atoms on a jittered 7 x 7 x 7 grid in an orthorhombic box that changes from frame to frame; every number has at
    most three decimals (two for angles), so the PDB text holds the same float32 values as the binary files"""
    rng = np.random.default_rng(12)
    grid = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    n = len(grid)
    frames, dims = [], []
    for t in range(T):
        L = np.round(np.array([19.6, 20.3, 21.0]) + 0.1 * t, 3)
        p = grid * (L / 7.0) + rng.uniform(-0.6, 0.6, size=(n, 3)) + rng.uniform(-30, 30, size=3)     # anywhere: nothing is wrapped
        frames.append(np.round(p, 3))
        dims.append(np.array([L[0], L[1], L[2], 90.0, 90.0, 90.0]))
    elements = [("C", "N", "H", "O", "H", "C", "H")[k % 7] for k in range(n)]
    names = [{"C": "CA", "N": "N", "H": "H", "O": "O"}[e] for e in elements]
    return dict(names=names, resnames=["ALA"] * n, resids=list(range(1, n + 1)), elements=elements,
                frames=np.asarray(frames).astype(np.float32), text=frames, dims=np.asarray(dims))


def _write_pdb(path, s, boxes=True):
    lines = []
    for m, (fr, d) in enumerate(zip(s["text"], s["dims"])):
        if boxes:
            lines.append("CRYST1%9.3f%9.3f%9.3f%7.2f%7.2f%7.2f P 1           1\n" % tuple(d))
        lines.append(f"MODEL     {m + 1:4d}\n")
        for k in range(len(s["names"])):
            lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s\n"
                         % (k + 1, " " + s["names"][k], s["resnames"][k], s["resids"][k], fr[k, 0], fr[k, 1], fr[k, 2],
                            s["elements"][k]))
        lines.append("ENDMDL\n")
    path.write_text("".join(lines))
    return str(path)


@pytest.fixture(scope="module")
def periodic(tmp_path_factory):
    from nmrgnn_amd.structure import read_pdb
    d = tmp_path_factory.mktemp("periodic")
    s = _periodic_system()
    s["pdb"] = _write_pdb(d / "boxed.pdb", s)
    u = read_pdb(s["pdb"])
    _same_bits(np.stack(u.frames), s["frames"])                 # the text and the binary files hold the same numbers
    np.testing.assert_array_equal(np.stack(u.dimensions), s["dims"])
    return s


@pytest.mark.parametrize("kind", KINDS)
def test_eval_struct_pbc_and_the_other_options(tmp_path, periodic, kind):
    import csv
    from nmrgnn_amd.main import eval_structure
    s = periodic
    path = _write(kind, tmp_path / ("t.nc" if kind == "netcdf" else "t.dcd"), s["frames"], s["dims"])
    table = tmp_path / "shifts.csv"
    with open(table, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["resid", "name", "shift"])
        for k in range(0, len(s["names"]), 5):
            wr.writerow([s["resids"][k], s["names"][k], f"{3.0 + 0.01 * k:.3f}"])
    runs = {"pbc": dict(pbc=True), "pbc-stride": dict(pbc=True, stride=2, frames_per_batch=2),
            "uncertainty": dict(uncertainty=3, stride=2, pbc=True),
            "reweight": dict(reweight=str(table), theta=5.0, sigma=0.5, pbc=True, frames_per_batch=2)}
    for name, kw in runs.items():
        eval_structure([s["pdb"]], str(tmp_path / "ref.csv"), **kw, **QUIET)
        eval_structure([s["pdb"], path], str(tmp_path / "out.csv"), **kw, **QUIET)
        assert (tmp_path / "out.csv").read_bytes() == (tmp_path / "ref.csv").read_bytes(), f"{kind}: {name}"
        if name == "reweight":
            assert (tmp_path / "out.weights.csv").read_bytes() == (tmp_path / "ref.weights.csv").read_bytes()
    # the box matters: the open-boundary run of the same frames gives other shifts
    eval_structure([s["pdb"], path], str(tmp_path / "open.csv"), **QUIET)
    eval_structure([s["pdb"]], str(tmp_path / "ref.csv"), pbc=True, **QUIET)
    assert (tmp_path / "open.csv").read_bytes() != (tmp_path / "ref.csv").read_bytes()
    # a frame without a box is the error it is for a PDB
    bare = _write(kind, tmp_path / ("bare.nc" if kind == "netcdf" else "bare.dcd"), s["frames"])
    with pytest.raises(ValueError, match="frame 0 has no box"):
        eval_structure([s["pdb"], bare], str(tmp_path / "x.csv"), pbc=True, **QUIET)
    with pytest.raises(ValueError, match="--separate takes PDB files"):
        eval_structure([s["pdb"], path], str(tmp_path / "x.csv"), separate=True, **QUIET)


# ------------------------------------------------------------------------------------------------- the stream itself
@pytest.mark.parametrize("kind", KINDS)
def test_stream_reuses_its_two_buffers_correctly(tmp_path, kind):
    """seven chunks over two staging buffers, every frame distinct: a buffer refilled before its copy completed, or a chunk
    decoded from the wrong buffer, shows up as wrong data"""
    n, T = 257, 26
    rng = np.random.default_rng(2)
    frames = rng.normal(scale=30.0, size=(T, n, 3)).astype(np.float32)
    dims = np.tile(np.array([40.0, 41.0, 42.0, 90.0, 90.0, 90.0]), (T, 1)) + np.arange(T)[:, None] * np.array([1, 0, 0, 0, 0, 0])
    traj = open_trajectory(_write(kind, tmp_path / "s.bin", frames, dims))
    ref = traj.read()
    _same_bits(ref, frames)
    sel = np.array([256, 0, 17, 17, 100])
    cases = [dict(frames=range(13), chunk_frames=2),                      # consecutive frames: one read per chunk
             dict(stride=2, chunk_frames=2),                              # every second frame: one span per frame
             dict(chunk_frames=4, select=sel),                            # 26 = 6 x 4 + 2
             dict(frames=[25, 3, 3, 4, 5, 20, 0, 1, 2, 9, 8, 7, 6], chunk_frames=2, select=sel)]
    for kw in cases:
        stream = TrajectoryStream(traj, device="cuda", **kw)
        assert len(stream) == 7
        seen = []
        for ids, pos, d in stream:
            assert pos.device.type == "cuda" and pos.shape == (len(ids), len(sel) if "select" in kw else n, 3)
            want = ref[ids][:, sel] if "select" in kw else ref[ids]
            _same_bits(pos, want)
            np.testing.assert_array_equal(d, dims[ids])
            seen.extend(int(i) for i in ids)
        assert seen == [int(i) for i in stream.frame_ids] and len(seen) == (13 if "frames" in kw or "stride" in kw else 26)
    # kept chunks stay what they were while later chunks go through the same buffers
    kept = [(ids, pos) for ids, pos, _ in TrajectoryStream(traj, chunk_frames=4, device="cuda")]
    torch.cuda.synchronize()
    for ids, pos in kept:
        _same_bits(pos, ref[ids])


@pytest.mark.parametrize("kind", KINDS)
def test_non_finite_coordinate_raises_and_names_the_frame(tmp_path, kind):
    n, T = 70, 9
    frames = np.random.default_rng(3).normal(scale=10.0, size=(T, n, 3)).astype(np.float32)
    frames[6, 41, 1] = np.inf
    traj = open_trajectory(_write(kind, tmp_path / "bad.bin", frames))
    got = []
    with pytest.raises(TrajectoryError, match="frame 6 holds a coordinate that is not finite"):
        for ids, pos, _ in TrajectoryStream(traj, chunk_frames=2, device="cuda"):
            got.extend(int(i) for i in ids)
    assert got == [0, 1, 2, 3, 4, 5]                # the chunks in front of the bad one arrived
    chunks = list(TrajectoryStream(traj, chunk_frames=2, select=[0, 5, 40], device="cuda"))      # atom 41 is not selected
    assert len(chunks) == 5


# --------------------------------------------------------------------------------------------------- device consumers
def _model(dev, num_elem):
    from nmrgnn_amd.model import GNNModel
    rng = np.random.default_rng(5)
    std, avg = rng.uniform(0.5, 2.0, 10).astype(np.float32), rng.uniform(-1.0, 1.0, 10).astype(np.float32)
    model = GNNModel(make_hp(atom_feature_size=64), {k: ("X", float(avg[k]), float(std[k])) for k in range(10)}, device=dev, seed=3)
    model.build(num_elem)
    randomize_biases(model.engine)
    return model


@pytest.mark.parametrize("kind", ["dcd-big", "netcdf"])
def test_predict_trajectory_equals_the_per_chunk_calls(tmp_path, periodic, gpu_device, kind):
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.library import predict_trajectory
    from nmrgnn_amd.structure import atoms_onehot
    s = periodic
    atoms = atoms_onehot(s["elements"])
    n, T = atoms.shape[0], len(s["frames"])
    model = _model(gpu_device, atoms.shape[1])
    model.freeze()
    path = _write(kind, tmp_path / "p.bin", s["frames"], s["dims"])
    mask = np.zeros(n, bool)
    mask[::9] = True
    for pbc in (False, True):
        own, own_sel = [], []
        for b0 in range(0, T, 2):
            batch = frames_to_batch(atoms, s["frames"][b0:b0 + 2], 16, device=gpu_device, box=s["dims"][b0:b0 + 2] if pbc else None)
            G = len(s["frames"][b0:b0 + 2])
            own.append(model(batch).detach().reshape(G, n))
            own_sel.append(model.predict_selected(batch, np.tile(mask, G)).detach().reshape(G, -1))
        got = predict_trajectory(model, atoms, path, pbc=pbc, frames_per_batch=2)
        assert got.device.type == "cuda" and tuple(got.shape) == (T, n)
        assert torch.equal(got, torch.cat(own))
        got = predict_trajectory(model, atoms, open_trajectory(path), pbc=pbc, select=np.nonzero(mask)[0], frames_per_batch=2)
        assert tuple(got.shape) == (T, int(mask.sum())) and torch.equal(got, torch.cat(own_sel))
    # a stream keeps its own frames and chunks
    got = predict_trajectory(model, atoms, TrajectoryStream(path, frames=[4, 0], chunk_frames=1, device=gpu_device))
    want = torch.cat([model(frames_to_batch(atoms, s["frames"][[k]], 16, device=gpu_device)).detach().reshape(1, n) for k in (4, 0)])
    assert torch.equal(got, want)
    bare = _write(kind, tmp_path / "bare.bin", s["frames"])
    with pytest.raises(ValueError, match="frame 0 has no box"):
        predict_trajectory(model, atoms, bare, pbc=True)


def test_reweight_trajectory_takes_a_trajectory(tmp_path, periodic, gpu_device):
    from nmrgnn_amd.library import reweight_trajectory
    from nmrgnn_amd.structure import atoms_onehot
    s = periodic
    atoms = atoms_onehot(s["elements"])
    n = atoms.shape[0]
    model = _model(gpu_device, atoms.shape[1])
    rng = np.random.default_rng(6)
    labelled = np.zeros(n, bool)
    labelled[rng.choice(n, n // 3, replace=False)] = True
    from nmrgnn_amd.graph import frames_to_batch
    own = model(frames_to_batch(atoms, s["frames"], 16, device=gpu_device)).detach().reshape(-1, n).cpu().numpy().astype(np.float64)
    spread = float(own.std(axis=0)[labelled].mean())
    assert spread > 0
    targets = np.where(labelled, own.mean(axis=0) + 0.5 * spread * rng.standard_normal(n), np.nan)
    want, shifts = reweight_trajectory(model, atoms, s["frames"], targets, spread, 2.0, frames_per_batch=2, tol=1e-8)
    for kind in KINDS:
        path = _write(kind, tmp_path / f"{kind}.bin", s["frames"])
        for traj in (path, open_trajectory(path)):
            got, got_shifts = reweight_trajectory(model, atoms, traj, targets, spread, 2.0, frames_per_batch=2, tol=1e-8)
            assert torch.equal(got_shifts, shifts)
            assert torch.equal(got.weights, want.weights) and torch.equal(got.lam, want.lam) and got.converged == want.converged
    small = _write("dcd-little", tmp_path / "small.bin", s["frames"][:, :100])
    with pytest.raises(ValueError, match=f"frames of {n} atoms"):
        reweight_trajectory(model, atoms, small, targets, spread, 2.0)
