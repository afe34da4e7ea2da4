"""Host-side contract of the input-gradient surface (no GPU)."""
import numpy as np
import pytest


def test_positions_grad_needs_a_batch_built_from_positions():
    import torch
    from nmrgnn_amd.graph import GraphBatch
    atoms = np.eye(3, dtype=np.float32)
    nlist = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    edges = np.full((3, 2), 0.1, np.float32)
    gb = GraphBatch(atoms, nlist, edges, np.full(3, 0.5, np.float32), device="cpu")
    assert gb.positions is None and gb.scale is None
    with pytest.raises(ValueError, match="positions"):
        gb.positions_grad(torch.zeros(3, 2))


def test_input_grad_entry_points_are_bound():
    from nmrgnn_amd import _lib
    for name in ("ng_edge_mlp_dinput", "ng_positions_grad", "ng_positions_grad_csr"):
        assert name in _lib.SIGNATURES
    from nmrgnn_amd.library import shift_restraint
    assert "ppm^2" in shift_restraint.__doc__
