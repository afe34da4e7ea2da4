"""Periodic boxes on the host (nmrgnn_amd.pbc, read_pdb's CRYST1): box conversion against hand values, the boxes that are
refused — before any device work — and the per-frame boxes of a PDB file.  No GPU needed."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OCT = float(np.degrees(np.arccos(1.0 / 3.0)))          # truncated-octahedron angle, 70.5288 degrees


def test_cryst1_of_108m():
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(os.path.join(HERE, "data", "108M.pdb"))
    assert len(s.dimensions) == len(s.frames) == 1
    np.testing.assert_array_equal(s.dimensions[0], [91.622, 79.347, 45.984, 90.0, 90.0, 90.0])


def test_nmr_placeholder_cube_means_no_box():
    from nmrgnn_amd.structure import read_pdb
    s = read_pdb(os.path.join(HERE, "data", "7lgi.pdb.gz"))
    assert len(s.dimensions) == len(s.frames) and all(d is None for d in s.dimensions)


def _atom(k, x, y, z):
    return f"ATOM  {k + 1:5d}  CA  ALA A{k + 1:4d}    {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00           C  \n"


def test_per_model_boxes(tmp_path):
    from nmrgnn_amd.structure import read_pdb
    lines = ["CRYST1   30.000   31.000   32.000  90.00  90.00  90.00 P 1           1\n"]
    boxes = [None, None, (40.0, 40.0, 40.0, 60.0, 60.0, 90.0)]
    for m in range(4):
        if m == 2:
            lines.append("CRYST1   40.000   40.000   40.000  60.00  60.00  90.00 P 1           1\n")
        lines.append(f"MODEL     {m + 1:4d}\n")
        lines += [_atom(k, k + m, 2.0 * k, -k) for k in range(3)]
        lines.append("ENDMDL\n")
    p = tmp_path / "boxes.pdb"
    p.write_text("".join(lines))
    s = read_pdb(str(p))
    assert len(s.frames) == 4
    np.testing.assert_array_equal(s.dimensions[0], [30, 31, 32, 90, 90, 90])
    np.testing.assert_array_equal(s.dimensions[1], [30, 31, 32, 90, 90, 90])
    np.testing.assert_array_equal(s.dimensions[2], boxes[2])
    np.testing.assert_array_equal(s.dimensions[3], boxes[2])
    np.testing.assert_array_equal(s.frames[3][1], [4.0, 2.0, -1.0])


@pytest.mark.parametrize("dims,vecs", [
    ((20.0, 20.0, 20.0, 90.0, 90.0, 90.0), [[20, 0, 0], [0, 20, 0], [0, 0, 20]]),
    # GROMACS rhombic dodecahedron (xy-square): d = 10
    ((10.0, 10.0, 10.0, 60.0, 60.0, 90.0), [[10, 0, 0], [0, 10, 0], [5, 5, 10 * np.sqrt(0.5)]]),
    # GROMACS truncated octahedron: d = 9
    ((9.0, 9.0, 9.0, OCT, 180.0 - OCT, OCT),
     [[9, 0, 0], [3, 6 * np.sqrt(2), 0], [-3, 3 * np.sqrt(2), 3 * np.sqrt(6)]]),
], ids=["cube", "dodecahedron", "octahedron"])
def test_dims_to_vectors(dims, vecs):
    from nmrgnn_amd.pbc import check_reduced, prepare, triclinic_vectors
    v = triclinic_vectors(dims)
    np.testing.assert_allclose(v, vecs, rtol=0, atol=1e-12)
    assert v[0, 1] == v[0, 2] == v[1, 2] == 0.0
    assert check_reduced(v) == (dims[3:] != (90.0, 90.0, 90.0))
    b, tric, w = prepare(dims, 3)                      # one box broadcast over three frames
    assert b.shape == (3, 9) and b.dtype == np.float32
    np.testing.assert_allclose(b[2].reshape(3, 3), vecs, rtol=1e-6, atol=1e-6)
    assert np.allclose(w, np.abs(np.linalg.det(v)) / np.max([np.linalg.norm(np.cross(v[1], v[2])),
                                                            np.linalg.norm(np.cross(v[2], v[0])),
                                                            np.linalg.norm(np.cross(v[0], v[1]))]))


@pytest.mark.parametrize("dims", [
    (20.0, 20.0, 20.0, 90.0, 90.0, 40.0),              # |b_x| = 15.3 > a_x / 2
    (20.0, 0.0, 20.0, 90.0, 90.0, 90.0),
    (-5.0, 20.0, 20.0, 90.0, 90.0, 90.0),
    (20.0, 20.0, float("nan"), 90.0, 90.0, 90.0),
    (20.0, 20.0, 20.0, 10.0, 100.0, 90.0),             # no cell
    (20.0, 20.0, 20.0, 0.0, 90.0, 90.0),
], ids=["skewed", "zero-length", "negative-length", "nan", "no-cell", "zero-angle"])
def test_refused_boxes_raise_before_device_work(dims):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    atoms = np.eye(4, dtype=np.float32)[np.arange(40) % 4]
    frames = np.random.default_rng(0).random((2, 40, 3)).astype(np.float32) * 10
    # device "cpu": anything past the host check would fail with another error
    with pytest.raises(ValueError, match="box"):
        frames_to_batch(atoms, frames, box=dims, device="cpu")
    with pytest.raises(ValueError, match="box"):
        frames_to_batch_cutoff(atoms, frames, box=np.stack([dims, dims]), device="cpu")


def test_cutoff_at_half_the_smallest_width_is_refused():
    from nmrgnn_amd.graph import frames_to_batch_cutoff
    atoms = np.eye(4, dtype=np.float32)[np.arange(40) % 4]
    frames = np.random.default_rng(0).random((2, 40, 3)).astype(np.float32) * 10
    boxes = np.array([(30.0, 30.0, 30.0, 90.0, 90.0, 90.0), (30.0, 30.0, 12.0, 90.0, 90.0, 90.0)])
    with pytest.raises(ValueError, match="cutoff"):
        frames_to_batch_cutoff(atoms, frames, cutoff=6.0, box=boxes, device="cpu")
    # the dodecahedron's smallest width is d / sqrt(2)... of its c face pair: cz = d sqrt(0.5) = 7.07 for d = 10
    with pytest.raises(ValueError, match="cutoff"):
        frames_to_batch_cutoff(atoms, frames, cutoff=3.6, box=(10.0, 10.0, 10.0, 60.0, 60.0, 90.0), device="cpu")


def test_box_shape_must_match_frames():
    from nmrgnn_amd.graph import frames_to_batch
    atoms = np.eye(4, dtype=np.float32)[np.arange(40) % 4]
    frames = np.zeros((3, 40, 3), np.float32)
    with pytest.raises(ValueError, match="box"):
        frames_to_batch(atoms, frames, box=np.full((2, 6), 20.0), device="cpu")
