"""Host side of the replica-averaged shift restraint (no GPU): the call and construction refusals of
library.ShiftRestraint, which come before any device work, Engine.backward(param_grad=False)'s argument checks, and the
ng_restraint_loss binding."""
import os

import numpy as np
import pytest

from nmrgnn_amd.library import ShiftRestraint, _restraint_box, _restraint_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_positions_shapes():
    p = np.zeros((5, 3), np.float32)
    pos, flat = _restraint_positions(p, 1, 5)
    assert flat and tuple(pos.shape) == (1, 5, 3)
    pos, flat = _restraint_positions(np.zeros((4, 5, 3), np.float32), 4, 5)
    assert not flat and tuple(pos.shape) == (4, 5, 3)
    for bad, R in [(p, 2), (np.zeros((3, 5, 3)), 4), (np.zeros((4, 6, 3)), 4), (np.zeros((4, 5, 2)), 4),
                   (np.zeros((5, 3, 1)), 1), (np.zeros(15), 1), (np.zeros((6, 3)), 1)]:
        with pytest.raises(ValueError):
            _restraint_positions(bad, R, 5)


def test_box_checks():
    ortho = np.array([30.0, 31.0, 32.0, 90.0, 90.0, 90.0])
    tric = np.array([30.0, 30.0, 30.0, 60.0, 60.0, 90.0])
    v, t = _restraint_box(ortho, 2)
    assert v.shape == (2, 9) and v.dtype == np.float32 and t is False
    v, t = _restraint_box(np.stack([tric, tric * [1.1, 1.1, 1.1, 1, 1, 1]]), 2)
    assert v.shape == (2, 9) and t is True
    with pytest.raises(ValueError):
        _restraint_box(np.stack([ortho] * 3), 2)            # [R', 6]
    with pytest.raises(ValueError):
        _restraint_box(ortho[:5], 1)                         # not [6]
    with pytest.raises(ValueError):
        _restraint_box(np.array([30.0, 30.0, 30.0, 90.0, 90.0, 40.0]), 1)      # not reduced
    with pytest.raises(ValueError):
        _restraint_box(tric, 1, triclinic=False)             # built for an orthorhombic box
    with pytest.raises(ValueError):
        _restraint_box(ortho, 1, triclinic=True)             # built for a triclinic box
    assert _restraint_box(tric, 1, triclinic=True)[1] is True


@pytest.mark.parametrize("kw", [dict(replicas=0), dict(replicas=1.5), dict(targets=np.zeros(4)), dict(weights=np.ones(6)),
                                dict(atoms=np.zeros(5)), dict(neighbor_number=0),
                                dict(box=np.array([30.0, 30.0, 30.0, 90.0, 90.0, 40.0])), dict(box=np.zeros((3, 6)))])
def test_construction_refusals_come_before_device_work(kw):
    args = dict(atoms=np.eye(4, dtype=np.float32)[np.arange(5) % 4], targets=np.zeros(5, np.float32))
    args.update(kw)
    atoms, targets = args.pop("atoms"), args.pop("targets")
    with pytest.raises(ValueError):
        ShiftRestraint(None, atoms, targets, **args)          # no model is touched: the checks come first


def test_engine_backward_param_grad_false_checks_first():
    from nmrgnn_amd.engine import Engine
    with pytest.raises(ValueError):
        Engine.backward(object(), None, edge_grad=None, param_grad=False)
    with pytest.raises(ValueError):
        Engine.backward(object(), np.zeros(3), edge_grad=None, param_grad=False)
    with pytest.raises(ValueError):
        Engine.backward(object(), np.zeros(3), edge_grad=np.zeros(3), param_grad=False, on_node_grads=lambda: None)


def test_restraint_loss_is_bound_and_declared():
    from nmrgnn_amd import _lib
    assert "ng_restraint_loss" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "nmrgnn_hip.h")) as f:
        assert "int ng_restraint_loss(" in f.read()
