"""Box gradients on the host (no GPU): the float64 torch restatement of the box conversion (nmrgnn_amd.pbc) against
triclinic_vectors and against central differences, and the requests that are refused before any device work."""
import numpy as np
import pytest
import torch

OCT = float(np.degrees(np.arccos(1.0 / 3.0)))


def _dims_of(v):
    v = np.asarray(v, np.float64)
    L = np.linalg.norm(v, axis=1)
    ang = lambda x, y: np.degrees(np.arccos(np.dot(x, y) / np.linalg.norm(x) / np.linalg.norm(y)))
    return np.array([L[0], L[1], L[2], ang(v[1], v[2]), ang(v[0], v[2]), ang(v[0], v[1])])


BOXES = {
    "cube": (20.0, 20.0, 20.0, 90.0, 90.0, 90.0),
    "flat": (31.0, 25.5, 4.75, 90.0, 90.0, 90.0),
    "gamma90": (20.0, 22.0, 24.0, 75.0, 80.0, 90.0),
    "alpha_beta90": (20.0, 22.0, 24.0, 90.0, 90.0, 70.0),
    "dodecahedron": (10.0, 10.0, 10.0, 60.0, 60.0, 90.0),
    "octahedron": (9.0, 9.0, 9.0, OCT, 180.0 - OCT, OCT),
    "extreme": tuple(_dims_of([[20.0, 0, 0], [10.0, 18.0, 0], [-10.0, 9.0, 16.0]])),
}


@pytest.mark.parametrize("kind", list(BOXES))
def test_torch_restatement_equals_triclinic_vectors(kind):
    from nmrgnn_amd.pbc import triclinic_vectors, triclinic_vectors_torch
    d = np.array(BOXES[kind])
    ref = triclinic_vectors(d)
    got = triclinic_vectors_torch(torch.tensor(d)).numpy()
    assert got.dtype == np.float64 and got.shape == (3, 3)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # batched [G, 6] -> [G, 3, 3]
    both = triclinic_vectors_torch(torch.tensor(np.stack([d, d * [1.1, 1.0, 0.9, 1, 1, 1]])))
    assert both.shape == (2, 3, 3)
    assert np.abs(both[0].numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("kind", list(BOXES))
def test_torch_restatement_jacobian_matches_central_differences(kind):
    from nmrgnn_amd.pbc import triclinic_vectors, triclinic_vectors_torch
    d = np.array(BOXES[kind])
    jac = torch.autograd.functional.jacobian(triclinic_vectors_torch, torch.tensor(d)).numpy()   # [3, 3, 6]
    assert np.isfinite(jac).all()
    for k in range(6):
        h = 1e-6 * (abs(d[k]) if k < 3 else 1.0)
        dp, dm = d.copy(), d.copy()
        dp[k] += h
        dm[k] -= h
        # the numpy conversion (exact zeros at 90 degrees) away from the point itself
        fd = (triclinic_vectors(dp) - triclinic_vectors(dm)) / (2 * h)
        np.testing.assert_allclose(jac[..., k], fd, rtol=1e-6, atol=1e-7 * np.abs(triclinic_vectors(d)).max())


@pytest.mark.parametrize("shape", [(5,), (7,), (2, 6), (3, 3, 6)])
def test_box_tensor_of_the_wrong_shape_raises_before_device_work(shape):
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    atoms = np.eye(4, dtype=np.float32)
    frames = np.zeros((3, 4, 3), np.float32)
    box = torch.full(shape, 20.0, dtype=torch.float64, requires_grad=True)
    with pytest.raises(ValueError, match="box"):
        frames_to_batch(atoms, frames, box=box, device="cpu")
    with pytest.raises(ValueError, match="box"):
        frames_to_batch_cutoff(atoms, frames, cutoff=2.0, box=box, device="cpu")


def test_box_grad_needs_a_batch_built_from_positions():
    from nmrgnn_amd.graph import GraphBatch
    atoms = np.eye(3, dtype=np.float32)
    nlist = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    edges = np.full((3, 2), 0.1, np.float32)
    gb = GraphBatch(atoms, nlist, edges, np.full(3, 0.5, np.float32), device="cpu")
    with pytest.raises(ValueError, match="positions"):
        gb.box_grad(torch.zeros(3, 2))
    csr = GraphBatch.from_csr(atoms, [0, 2, 4, 6], nlist.reshape(-1), edges.reshape(-1), device="cpu")
    with pytest.raises(ValueError, match="positions"):
        csr.box_grad(torch.zeros(6))


def test_box_grad_entry_points_are_bound():
    from nmrgnn_amd import _lib
    for name in ("ng_box_grad", "ng_box_grad_csr"):
        assert name in _lib.SIGNATURES
    import inspect
    from nmrgnn_amd.library import shift_restraint
    assert inspect.signature(shift_restraint).parameters["virial"].default is False
