"""The host restatements of the ensemble-averaged loss (tests/group_loss_ref.py) against themselves: the float64 gradient by
central differences, the float32 mean and spread on singleton groups, and the float32 chain against the float64 one.  No GPU."""
import numpy as np
import pytest

import group_loss_ref as R


make_case, member_weights = R.make_case, R.member_weights

CASE = [(7, 2), (5, 3), (4, 1)]


@pytest.mark.parametrize("s", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_float64_gradient_by_central_differences(s, weighted):
    gp, qp, pred, y, w, _ = make_case(3, CASE)
    c = member_weights(4, qp) if weighted else None
    pred = pred.astype(np.float64)
    loss, dpred, means = R.ensemble_loss_f64(gp, qp, pred, y, w, s=s, c=c, scale=0.25)
    assert np.isfinite(loss) and means.shape == (16,)
    h = 1e-5
    num = np.empty_like(dpred)
    for k in range(len(pred)):
        up, dn = pred.copy(), pred.copy()
        up[k] += h
        dn[k] -= h
        num[k] = 0.25 * (R.ensemble_loss_f64(gp, qp, up, y, w, s=s, c=c)[0] - R.ensemble_loss_f64(gp, qp, dn, y, w, s=s, c=c)[0]) / (2 * h)
    # central differences of a smooth function in float64: truncation h^2 f''' and rounding eps |f| / h, both far below this
    assert np.max(np.abs(num - dpred)) <= 1e-7 * max(1.0, np.max(np.abs(dpred))), np.max(np.abs(num - dpred))


def test_float64_loss_of_singletons_is_the_per_graph_loss():
    gp, qp, pred, y, w, _ = make_case(5, [(6, 1), (9, 1), (3, 1)], zero_weight_group=1)
    loss, dpred, means = R.ensemble_loss_f64(gp, qp, pred, y, w, s=0.5)
    per = [R.name_loss(y[a:b], w[a:b], pred[a:b].astype(np.float64), 0.5) for a, b in zip(gp[:-1], gp[1:])]
    assert loss == pytest.approx(np.mean([p[0] for p in per]), rel=1e-14)
    assert np.allclose(dpred, np.concatenate([p[1] for p in per]) / 3, rtol=1e-14, atol=0)
    assert np.array_equal(means, pred.astype(np.float64))
    assert np.all(dpred[gp[1]:gp[2]] == 0)            # divide_no_nan: a graph without weights pulls nothing


def test_float32_singletons_reproduce_their_input_bits():
    gp, _, pred, y, w, names = make_case(6, [(1, 1), (5, 1), (8, 1)])
    pred[3] = np.float32(-0.0)
    qp = np.arange(len(gp), dtype=np.int32)
    mean, yo, wo, no = R.group_mean_f32(gp, qp, pred, y, w, names=names)
    for got, ref in ((mean, pred), (yo, y), (wo, w)):
        assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    assert np.array_equal(no, names)
    d = np.random.default_rng(1).standard_normal(len(pred)).astype(np.float32)
    assert np.array_equal(R.group_spread_f32(gp, qp, d).view(np.int32), d.view(np.int32))
    assert np.array_equal(R.group_spread_f32(gp, qp, d, scale=0.25), d * np.float32(0.25))


def test_float32_mean_and_spread_order():
    """three members: ((p0 + p1) + p2) / 3 and ((c0 p0) + c1 p1) + c2 p2, every step rounded; the spread hits every row"""
    gp, qp = np.array([0, 2, 4, 6], np.int32), np.array([0, 3], np.int32)
    p = np.array([1.0, 2.0, 1e-8, 3.0, -1.0, 5.0], np.float32)
    y, w = np.array([1, 2, 9, 9, 9, 9], np.float32), np.ones(6, np.float32)
    mean, yo, wo, _ = R.group_mean_f32(gp, qp, p, y, w)
    f = np.float32
    assert mean[0] == f(f(f(f(1.0) + f(1e-8)) + f(-1.0)) / f(3)) and mean[1] == f(f(f(2) + f(3)) + f(5)) / f(3)
    assert list(yo) == [1, 2] and list(wo) == [1, 1]
    c = np.array([0.5, 0.0, 0.5], np.float32)
    mean, *_ = R.group_mean_f32(gp, qp, p, y, w, c=c)
    assert mean[0] == f(f(f(0.5) * f(1.0)) + f(0.0)) + f(f(0.5) * f(-1.0)) and mean[1] == f(3.5)
    d = R.group_spread_f32(gp, qp, np.array([3.0, 6.0], np.float32), c=c, scale=2.0)
    assert list(d) == [3.0, 6.0, 0.0, 0.0, 3.0, 6.0]
    d = R.group_spread_f32(gp, qp, np.array([3.0, 6.0], np.float32))
    assert list(d) == [1.0, 2.0] * 3


def test_unequal_members_are_refused():
    with pytest.raises(AssertionError, match="group 0"):
        R.mean_ptr_of([0, 3, 7], [0, 2])


@pytest.mark.parametrize("s,loss_dtype", [(1.0, np.float32), (0.5, np.float64)])
def test_float32_chain_is_close_to_float64(s, loss_dtype):
    """the rounding of the float32 mean (values near 120, differences near 0.7) is what separates the two: a few 1e-5 of the
    largest gradient entry"""
    gp, qp, pred, y, w, _ = make_case(3, CASE)
    l64, d64, _ = R.ensemble_loss_f64(gp, qp, pred, y, w, s=s)
    l32, d32 = R.ensemble_loss_f32(gp, qp, pred, y, w, s=s, loss_dtype=loss_dtype)
    assert abs(float(l32) - l64) <= 1e-4 * abs(l64)
    assert np.max(np.abs(d32 - d64)) <= 1e-4 * np.max(np.abs(d64))
