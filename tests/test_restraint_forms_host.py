"""Host side of the shift-restraint forms (no GPU): the refusals of ShiftRestraint's tolerance / replica_weights /
independent / tau, which come before any device work, the float64 normalisation of the replica weights, lambda from tau,
and the ng_restraint_loss_ex binding and declaration."""
import os
import re
import types

import numpy as np
import pytest

from nmrgnn_amd.library import (ShiftRestraint, _restraint_lambda, _restraint_replica_weights, _restraint_tolerance)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tolerance_checks():
    t = _restraint_tolerance(0.5, 4)
    assert t.dtype == np.float32 and t.shape == (4,) and (t == np.float32(0.5)).all()
    t = _restraint_tolerance(np.array([0.0, 1.0, 2.5, 0.25]), 4)
    assert t.dtype == np.float32 and np.array_equal(t, np.array([0.0, 1.0, 2.5, 0.25], np.float32))
    for bad in [-0.1, np.nan, np.inf, np.ones(3), np.ones((4, 1)), np.array([0.0, 1.0, -1.0, 0.0])]:
        with pytest.raises(ValueError):
            _restraint_tolerance(bad, 4)


def test_replica_weights_are_normalised_in_float64():
    c = np.array([1.0, 3.0, 0.0, 2.0])
    got = _restraint_replica_weights(c, 4)
    assert got.dtype == np.float32
    assert np.array_equal(got, (c / 6.0).astype(np.float32))
    got = _restraint_replica_weights([0.1] * 3, 3)
    assert np.array_equal(got, np.full(3, 1.0 / 3.0).astype(np.float32))
    for bad in [np.ones(3), np.ones((4, 1)), np.zeros(4), np.array([1.0, -1.0, 1.0, 1.0]), np.array([1.0, np.nan, 1, 1]),
                np.array([1.0, np.inf, 1, 1])]:
        with pytest.raises(ValueError):
            _restraint_replica_weights(bad, 4)


def test_lambda_from_tau():
    for tau in (0.5, 1, 3.0, 100, 1e6):
        lam = _restraint_lambda(tau)
        assert lam == float(np.float32(np.exp(-1.0 / tau))) and 0 <= lam < 1
    for bad in (0, -1.0, np.nan, np.inf, 1e9, "x", np.ones(2)):
        with pytest.raises(ValueError):
            _restraint_lambda(bad)


@pytest.mark.parametrize("kw", [dict(tolerance=-1.0), dict(tolerance=np.ones(4)), dict(tolerance=np.nan),
                                dict(replicas=2, replica_weights=np.ones(3)), dict(replicas=2, replica_weights=np.zeros(2)),
                                dict(replicas=2, replica_weights=np.array([1.0, -0.5])),
                                dict(replicas=2, replica_weights=np.ones(2), independent=True),
                                dict(tau=0), dict(tau=-2.0), dict(tau=np.inf), dict(tau=1e12)])
def test_form_refusals_come_before_device_work(kw):
    atoms, targets = np.eye(4, dtype=np.float32)[np.arange(5) % 4], np.zeros(5, np.float32)
    with pytest.raises(ValueError):
        ShiftRestraint(None, atoms, targets, **kw)        # no model is touched: the checks come first


def test_call_time_replica_weights_refusals():
    # the call's check reads only R and whether the restraint was built with weights
    one = types.SimpleNamespace(R=1, s_c=np.ones(1, np.float32))
    unweighted = types.SimpleNamespace(R=3, s_c=None)
    weighted = types.SimpleNamespace(R=3, s_c=np.ones(3, np.float32))
    with pytest.raises(ValueError):
        ShiftRestraint._call_weights(one, np.ones(1))                 # R = 1
    with pytest.raises(ValueError):
        ShiftRestraint._call_weights(unweighted, np.ones(3))          # built without weights: the chain reads none
    for bad in (np.ones(2), np.zeros(3), np.array([1.0, -1.0, 1.0])):
        with pytest.raises(ValueError):
            ShiftRestraint._call_weights(weighted, bad)
    assert ShiftRestraint._call_weights(weighted, None) is None
    assert np.array_equal(ShiftRestraint._call_weights(weighted, [2.0, 1.0, 1.0]),
                          np.array([0.5, 0.25, 0.25], np.float32))


def test_restraint_loss_ex_is_bound_and_declared():
    from nmrgnn_amd import _lib
    assert "ng_restraint_loss_ex" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "nmrgnn_hip.h")) as f:
        text = f.read()
    assert "#define NG_RESTRAINT_ENSEMBLE 0" in text and "#define NG_RESTRAINT_INDEPENDENT 1" in text
    decl = re.search(r"int ng_restraint_loss_ex\(([^;]*)\);", text)
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["ng_restraint_loss_ex"][1])
