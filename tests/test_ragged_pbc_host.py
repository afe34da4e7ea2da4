"""Periodic boxes on ragged batches without a GPU: pbc.prepare_ragged, and every refusal of structures_to_batch(boxes=) and
eval-struct --boxes on the host, before any device work (the GPU side is tests/test_gpu_ragged_pbc.py)."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OCT = float(np.degrees(np.arccos(1.0 / 3.0)))          # truncated-octahedron angle, 70.5288 degrees
CUBE = (12.0, 12.0, 12.0, 90.0, 90.0, 90.0)
DODECAHEDRON = (10.0, 10.0, 10.0, 60.0, 60.0, 90.0)
OCTAHEDRON = (9.0, 9.0, 9.0, OCT, 180.0 - OCT, OCT)
UNREDUCED = (10.0, 10.0, 10.0, 90.0, 90.0, 40.0)       # b_x = 10 cos 40 = 7.66 > a_x / 2


def _mols(sizes, C=10, seed=0):
    rng = np.random.default_rng(seed)
    atoms = [np.eye(C, dtype=np.float32)[rng.integers(0, C, n)] for n in sizes]
    pos = [rng.uniform(0, 5, (n, 3)).astype(np.float32) for n in sizes]
    return atoms, pos


def test_prepare_ragged_mixed_list():
    from nmrgnn_amd.pbc import prepare, prepare_ragged
    boxes = [None, CUBE, DODECAHEDRON, OCTAHEDRON]
    vecs, kinds, w = prepare_ragged(boxes, 4)
    assert vecs.shape == (4, 9) and vecs.dtype == np.float32
    assert kinds.dtype == np.int32 and kinds.tolist() == [-1, 0, 1, 1]
    assert w.shape == (4,)
    assert not vecs[0].any() and np.isinf(w[0]) and w[0] > 0
    for g in (1, 2, 3):
        v1, tric, w1 = prepare(np.asarray(boxes[g]), 1)
        assert np.array_equal(vecs[g].view(np.uint32), v1[0].view(np.uint32)), g
        assert bool(tric) == (kinds[g] == 1)
        assert w[g] == w1[0]
    # an orthorhombic structure keeps its own kind beside triclinic ones (prepare's any() rule is per batch, not carried over)
    assert prepare(np.asarray([CUBE, DODECAHEDRON]), 2)[1] is True
    assert prepare_ragged([CUBE, DODECAHEDRON], 2)[1].tolist() == [0, 1]


def test_prepare_ragged_array_and_tensor_forms():
    import torch
    from nmrgnn_amd.pbc import prepare_ragged
    arr = np.array([CUBE, DODECAHEDRON, OCTAHEDRON])
    a = prepare_ragged(arr, 3)
    b = prepare_ragged(torch.tensor(arr, requires_grad=True), 3)
    c = prepare_ragged([tuple(r) for r in arr], 3)
    for x, y in ((a, b), (a, c)):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert a[1].tolist() == [0, 1, 1]
    v, k, w = prepare_ragged([None, None], 2)
    assert k.tolist() == [-1, -1] and not v.any() and np.isinf(w).all()


@pytest.mark.parametrize("bad, match", [
    ((10.0, 10.0, float("nan"), 90.0, 90.0, 90.0), "structure 2: box: non-finite"),
    ((10.0, float("inf"), 10.0, 90.0, 90.0, 90.0), "structure 2: box: non-finite"),
    ((10.0, 0.0, 10.0, 90.0, 90.0, 90.0), "structure 2: box: lengths must be > 0"),
    ((10.0, 10.0, -1.0, 90.0, 90.0, 90.0), "structure 2: box: lengths must be > 0"),
    ((10.0, 10.0, 10.0, 0.0, 90.0, 90.0), r"structure 2: box: angles must lie in \(0, 180\)"),
    ((10.0, 10.0, 10.0, 90.0, 180.0, 90.0), r"structure 2: box: angles must lie in \(0, 180\)"),
    ((10.0, 10.0, 10.0, 10.0, 80.0, 120.0), "structure 2: box: angles .* give no cell"),
    (UNREDUCED, "structure 2: box: only orthorhombic and reduced triclinic"),
    ((10.0, 10.0, 10.0, 90.0, 90.0), "structure 2: box: .* expected, got 5 values"),
], ids=["nan", "inf", "zero_length", "negative_length", "angle0", "angle180", "no_cell", "unreduced", "five_values"])
def test_prepare_ragged_refusals_name_the_structure(bad, match):
    from nmrgnn_amd.pbc import prepare_ragged
    with pytest.raises(ValueError, match=match):
        prepare_ragged([None, CUBE, bad, DODECAHEDRON], 4)


def test_prepare_ragged_refuses_count_and_form():
    from nmrgnn_amd.pbc import prepare_ragged
    with pytest.raises(ValueError, match="3 entries for 4 structures"):
        prepare_ragged([None, CUBE, None], 4)
    with pytest.raises(ValueError, match="2 entries for 3 structures"):
        prepare_ragged(np.array([CUBE, CUBE]), 3)
    with pytest.raises(ValueError, match=r"\[G, 6\] array expected"):
        prepare_ragged(np.array(CUBE), 1)
    with pytest.raises(ValueError, match="sequence of G entries"):
        prepare_ragged(12.0, 1)


@pytest.mark.parametrize("form", ["list", "sizes", "graph_ptr"])
def test_structures_to_batch_boxes_wrong_count(form):
    from nmrgnn_amd.graph import structures_to_batch
    atoms, pos = _mols([3, 5, 4])
    boxes = [CUBE, None]
    with pytest.raises(ValueError, match="2 entries for 3 structures"):
        if form == "list":
            structures_to_batch(atoms, pos, boxes=boxes, device="cpu")
        elif form == "sizes":
            structures_to_batch(np.concatenate(atoms), np.concatenate(pos), sizes=[3, 5, 4], boxes=boxes, device="cpu")
        else:
            structures_to_batch(np.concatenate(atoms), np.concatenate(pos), graph_ptr=[0, 3, 8, 12], boxes=boxes, device="cpu")


@pytest.mark.parametrize("cutoff", [None, 3.0])
def test_structures_to_batch_boxes_unreduced(cutoff):
    from nmrgnn_amd.graph import structures_to_batch
    atoms, pos = _mols([3, 5, 4])
    with pytest.raises(ValueError, match="structure 1: box: only orthorhombic and reduced triclinic"):
        structures_to_batch(atoms, pos, cutoff=cutoff, boxes=[None, UNREDUCED, CUBE], device="cpu")


def test_structures_to_batch_boxes_cutoff_against_half_width():
    from nmrgnn_amd.graph import structures_to_batch
    atoms, pos = _mols([3, 5, 4])
    # structure 2's smallest width is 6: a cutoff of exactly half of it is refused, and so is a larger one; the open structure
    # and the 12 A cube do not object
    boxes = [None, CUBE, (6.0, 8.0, 10.0, 90.0, 90.0, 90.0)]
    for cutoff in (3.0, 4.5):
        with pytest.raises(ValueError, match=r"structure 2: cutoff .* must be below half the smallest box width \(3\)"):
            structures_to_batch(atoms, pos, cutoff=cutoff, boxes=boxes, device="cpu")
    # the dodecahedron's smallest width is 10 sqrt(1/2) = 7.07, not its edge length
    with pytest.raises(ValueError, match=r"structure 0: cutoff .* \(3\.53553\)"):
        structures_to_batch(atoms, pos, cutoff=3.6, boxes=[DODECAHEDRON, None, None], device="cpu")


def test_structures_to_batch_still_refuses_box():
    from nmrgnn_amd.graph import structures_to_batch
    atoms, pos = _mols([4, 6])
    for kw in (dict(), dict(cutoff=4.0), dict(boxes=[CUBE, None])):
        with pytest.raises(ValueError, match="periodic boxes are not supported") as e:
            structures_to_batch(atoms, pos, box=list(CUBE), device="cpu", **kw)
        assert "boxes=" in str(e.value)


def test_ragged_pbc_entry_points_are_bound():
    from nmrgnn_amd import _lib
    for name in ("ng_knn_graph_ragged_pbc", "ng_cutoff_count_ragged_pbc", "ng_cutoff_fill_rows_ragged_pbc",
                 "ng_positions_grad_ragged_pbc", "ng_positions_grad_csr_ragged_pbc", "ng_box_grad_ragged",
                 "ng_box_grad_csr_ragged"):
        assert name in _lib.SIGNATURES


def test_eval_struct_boxes_without_separate_is_a_usage_error(tmp_path):
    from click.testing import CliRunner
    from nmrgnn_amd.main import eval_structure, main
    pdb = os.path.join(HERE, "data", "108M.pdb")
    res = CliRunner().invoke(main, ["eval-struct", "--help"])
    assert res.exit_code == 0 and "--boxes" in res.output
    res = CliRunner().invoke(main, ["eval-struct", "--boxes", pdb, str(tmp_path / "o.csv")])
    assert res.exit_code == 2
    assert "--boxes goes with --separate" in res.output
    assert not (tmp_path / "o.csv").exists()
    with pytest.raises(ValueError, match="--boxes goes with --separate"):
        eval_structure([pdb], str(tmp_path / "o.csv"), boxes=True, echo=lambda *a: None)
    # --separate --pbc stays the usage error it was, and now names --boxes
    res = CliRunner().invoke(main, ["eval-struct", "--separate", "--pbc", pdb, str(tmp_path / "o.csv")])
    assert res.exit_code == 2
    assert "--separate and --pbc cannot be combined" in res.output and "--boxes" in res.output
