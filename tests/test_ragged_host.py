"""structures_to_batch and eval-struct --separate without a GPU: every refusal happens on the host, before any device
work (the GPU side is tests/test_gpu_ragged_lists.py)."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _mols(sizes, C=10, seed=0):
    rng = np.random.default_rng(seed)
    atoms = [np.eye(C, dtype=np.float32)[rng.integers(0, C, n)] for n in sizes]
    pos = [rng.uniform(0, 5, (n, 3)).astype(np.float32) for n in sizes]
    return atoms, pos


@pytest.mark.parametrize("case, match", [
    ("length", "2 atom arrays but 3"),
    ("rows", "atom rows but"),
    ("empty_list", "has no atoms"),
    ("no_structures", "no structures"),
    ("k0", r"neighbor_number must be in \[1, 64\]"),
    ("k65", r"neighbor_number must be in \[1, 64\]"),
    ("cutoff0", "cutoff must be > 0"),
    ("cutoff_neg", "cutoff must be > 0"),
    ("sizes_sum", "the structures hold"),
    ("sizes_zero", "has no atoms"),
    ("ptr_start", "graph_ptr must start at 0"),
    ("ptr_zero", "has no atoms"),
    ("neither", "exactly one of sizes= or graph_ptr="),
    ("both", "exactly one of sizes= or graph_ptr="),
    ("mixed", "must both be lists"),
    ("list_sizes", "go with concatenated arrays"),
    ("pos_shape", r"positions \[N, 3\]"),
])
def test_structures_to_batch_refuses_bad_input(case, match):
    from nmrgnn_amd.graph import structures_to_batch
    atoms, pos = _mols([3, 5, 1])
    cat_a, cat_p = np.concatenate(atoms), np.concatenate(pos)
    kw = dict(device="cpu")
    args = {
        "length": lambda: structures_to_batch(atoms[:2], pos, **kw),
        "rows": lambda: structures_to_batch(atoms, [pos[0], pos[1][:4], pos[2]], **kw),
        "empty_list": lambda: structures_to_batch(atoms + [atoms[0][:0]], pos + [pos[0][:0]], **kw),
        "no_structures": lambda: structures_to_batch([], [], **kw),
        "k0": lambda: structures_to_batch(atoms, pos, neighbor_number=0, **kw),
        "k65": lambda: structures_to_batch(atoms, pos, neighbor_number=65, **kw),
        "cutoff0": lambda: structures_to_batch(atoms, pos, cutoff=0.0, **kw),
        "cutoff_neg": lambda: structures_to_batch(atoms, pos, cutoff=-2.0, **kw),
        "sizes_sum": lambda: structures_to_batch(cat_a, cat_p, sizes=[3, 5, 2], **kw),
        "sizes_zero": lambda: structures_to_batch(cat_a, cat_p, sizes=[3, 0, 5, 1], **kw),
        "ptr_start": lambda: structures_to_batch(cat_a, cat_p, graph_ptr=[1, 3, 8, 9], **kw),
        "ptr_zero": lambda: structures_to_batch(cat_a, cat_p, graph_ptr=[0, 3, 3, 8, 9], **kw),
        "neither": lambda: structures_to_batch(cat_a, cat_p, **kw),
        "both": lambda: structures_to_batch(cat_a, cat_p, sizes=[3, 5, 1], graph_ptr=[0, 3, 8, 9], **kw),
        "mixed": lambda: structures_to_batch(atoms, cat_p, **kw),
        "list_sizes": lambda: structures_to_batch(atoms, pos, sizes=[3, 5, 1], **kw),
        "pos_shape": lambda: structures_to_batch(cat_a, cat_p[:, :2], sizes=[3, 5, 1], **kw),
    }[case]
    with pytest.raises(ValueError, match=match):
        args()


def test_structures_to_batch_refuses_a_box():
    from nmrgnn_amd.graph import structures_to_batch
    atoms, pos = _mols([4, 6])
    with pytest.raises(ValueError, match="periodic boxes are not supported"):
        structures_to_batch(atoms, pos, box=[20.0, 20.0, 20.0, 90.0, 90.0, 90.0], device="cpu")
    with pytest.raises(ValueError, match="periodic boxes are not supported"):
        structures_to_batch(atoms, pos, cutoff=4.0, box=[20.0, 20.0, 20.0, 90.0, 90.0, 90.0], device="cpu")


def test_structures_to_batch_is_exported():
    import nmrgnn_amd
    from nmrgnn_amd.graph import structures_to_batch
    assert nmrgnn_amd.structures_to_batch is structures_to_batch


def test_ragged_entry_points_are_bound():
    from nmrgnn_amd import _lib
    for name in ("ng_knn_graph_ragged", "ng_cutoff_count_ragged", "ng_cutoff_fill_rows_ragged"):
        assert name in _lib.SIGNATURES


def test_eval_struct_separate_in_help():
    from click.testing import CliRunner
    from nmrgnn_amd.main import main
    res = CliRunner().invoke(main, ["eval-struct", "--help"])
    assert res.exit_code == 0
    assert "--separate" in res.output


def test_eval_struct_separate_pbc_is_a_usage_error(tmp_path):
    from click.testing import CliRunner
    from nmrgnn_amd.main import eval_structure, main
    pdb = os.path.join(HERE, "data", "108M.pdb")
    res = CliRunner().invoke(main, ["eval-struct", "--separate", "--pbc", pdb, str(tmp_path / "o.csv")])
    assert res.exit_code == 2
    assert "--separate and --pbc cannot be combined" in res.output
    assert not (tmp_path / "o.csv").exists()
    with pytest.raises(ValueError, match="cannot be combined"):
        eval_structure([pdb], str(tmp_path / "o.csv"), separate=True, pbc=True, echo=lambda *a: None)
