"""Host tests of the maximum-entropy reweighting (no GPU): the float64 reference tests/reweight_ref.py checked against
independent statements of the same mathematics, the meaning of its error bound, the command-line helpers of
nmrgnn_amd/reweight.py, and the exported symbols."""
import csv
import ctypes
import os

import numpy as np
import pytest

import reweight_ref as R


# -------------------------------------------------------------------------------------------------------- the reference
def test_gradient_against_central_differences():
    S, y = R.synthetic(40, 6, 1)
    rng = np.random.default_rng(2)
    sigma = rng.uniform(0.3, 1.0, 6)
    w0 = rng.uniform(0.2, 1.0, 40)
    logw0 = np.log(w0 / w0.sum())
    lam = 0.4 * rng.standard_normal(6)
    for lw in (None, logw0):
        _, g = R.gamma_grad(S, y, sigma, 1.7, lam, lw)
        h = 1e-6
        for m in range(6):
            e = np.zeros(6)
            e[m] = h
            fd = (R.gamma_grad(S, y, sigma, 1.7, lam + e, lw)[0] - R.gamma_grad(S, y, sigma, 1.7, lam - e, lw)[0]) / (2 * h)
            assert abs(fd - g[m]) <= 1e-8 * (1 + abs(g[m]))


def test_two_frames_one_observable_against_bisection():
    """T = 2, M = 1: the stationarity condition is one scalar equation, -mean(lam) + theta sigma^2 lam = 0, monotone in lam"""
    S = np.array([[1.0], [3.0]], np.float32)
    y = np.array([2.6], np.float32)
    sigma, theta = 0.5, 0.8
    d = S[:, 0].astype(np.float64) - float(y[0])

    def f(lam):
        w = np.exp(-lam * d - np.max(-lam * d))
        return -float(w @ d / w.sum()) + theta * sigma ** 2 * lam

    lo, hi = -100.0, 100.0
    assert f(lo) < 0 < f(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) < 0 else (lo, mid)
    lam, it, ok = R.newton(S, y, sigma, theta)
    assert ok and it < 50 and abs(lam[0] - 0.5 * (lo + hi)) <= 1e-12


def test_lambda_zero_gives_the_prior():
    S, y = R.synthetic(30, 4, 3)
    r = R.evaluate(S, y, np.zeros(4))
    assert abs(r["logZ"]) <= 1e-15 and np.allclose(r["p"], 1 / 30, rtol=1e-15)
    w0 = np.random.default_rng(1).uniform(0, 1, 30)
    w0[3] = 0
    with np.errstate(divide="ignore"):
        lw = np.log(w0 / w0.sum())
    r = R.evaluate(S, y, np.zeros(4), lw)
    assert abs(r["logZ"]) <= 1e-15 and np.allclose(r["p"], w0 / w0.sum(), rtol=1e-14) and r["p"][3] == 0
    assert R.stats(r["p"], lw)[0] == pytest.approx(1.0, abs=1e-14)
    r = R.evaluate(S, y, np.ones(4), np.full(30, -np.inf))
    assert r["logZ"] == -np.inf and (r["mean"] == 0).all() and (r["p"] == 0).all()


def test_phi_eff_and_the_regularisation_path():
    """phi_eff in (0, 1]; along descending theta chi2_post does not rise and phi_eff does not rise (the path of
    min chi2 / 2 + theta KL)"""
    S, y = R.synthetic(120, 9, 4)
    prev = None
    for theta in (16.0, 8.0, 4.0, 2.0, 1.0, 0.5):
        r = R.solve(S, y, 0.5, theta, lam0=None if prev is None else prev["lam"])
        assert r["converged"] and r["iterations"] < 50
        assert 0 < r["phi_eff"] <= 1 and 0 < r["kish"] <= 1 + 1e-12
        assert r["chi2_post"] < r["chi2_prior"]
        if prev is not None:
            assert r["chi2_post"] <= prev["chi2_post"] + 1e-12 and r["phi_eff"] <= prev["phi_eff"] + 1e-12
        prev = r


def test_end_to_end_cases_converge_quickly():
    """the two sets of tests/test_gpu_reweight.py: the reference Newton must converge in under 50 iterations on them"""
    for T, M, theta, seed in R.END_TO_END:
        S, y = R.synthetic(T, M, seed)
        r = R.solve(S, y, 0.5, theta)
        assert r["converged"] and r["iterations"] < 50 and r["chi2_post"] < r["chi2_prior"]


@pytest.mark.parametrize("case", ["moderate", "wide"])
def test_the_bound_is_meaningful(case):
    """other float64 summation orders stay inside the bound; float32 logits fall outside it on the wide-spread case"""
    T, M = 133, 37
    if case == "wide":
        S, y, lam = R.wide_case(T, M, T - 1, 31)
    else:
        S, y = R.synthetic(T, M, 7)
        lam = 0.3 * np.random.default_rng(8).standard_normal(M) / np.sqrt(M)
    ref = R.evaluate(S, y, lam)
    f = R.bound_factor(T, M, ref["A"])
    for order in ("reversed", "pairwise"):
        logZ, mean = R.evaluate_ordered(S, y, lam, order=order)
        assert abs(logZ - ref["logZ"]) <= f
        assert (np.abs(mean - ref["mean"]) <= f * ref["absmean"]).all()
    if case == "wide":
        assert ref["a"].max() - ref["a"].min() > 1500
        logZ, mean = R.evaluate_ordered(S, y, lam, logit_dtype=np.float32)
        assert abs(logZ - ref["logZ"]) > f or (np.abs(mean - ref["mean"]) > f * ref["absmean"]).any()


def test_weighted_moments_reference():
    rng = np.random.default_rng(5)
    mu = (100 + rng.standard_normal((7, 3))).astype(np.float32)
    mu[:, 1] = mu[0, 1]
    p = rng.uniform(0, 1, 7)
    p /= p.sum()
    r = R.weighted_moments(mu, p)
    m64 = mu.astype(np.float64)
    assert np.allclose(r["mean"], p @ m64, rtol=1e-14)
    assert np.allclose(r["var"], p @ (m64 - (p @ m64)[None]) ** 2, atol=1e-12) and r["var"][1] == 0


# ----------------------------------------------------------------------------------------------------------- the package
def test_module_imports_without_a_gpu_and_symbols_are_exported():
    import nmrgnn_amd.reweight as rw
    from nmrgnn_amd import _lib
    assert hasattr(rw, "ShiftReweighter") and hasattr(rw, "ReweightResult")
    import __graft_entry__ as ge
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ng_reweight_eval", "ng_reweight_weights", "ng_weighted_moments"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.ng_abi_version() == 9
    from nmrgnn_amd.library import reweight_trajectory      # noqa: F401


def test_parse_sigma():
    from nmrgnn_amd.reweight import parse_sigma
    assert parse_sigma("0.4") == 0.4 and parse_sigma(" 1e-1 ") == 0.1
    assert parse_sigma("H=0.3,C=1.1, n=2.5") == {"H": 0.3, "C": 1.1, "N": 2.5}
    for bad in ("", "x", "0", "-1", "nan", "inf", "H=", "H=0", "=0.3", "H=0.3,H=0.4", "H=0.3,C", "H=a"):
        with pytest.raises(ValueError):
            parse_sigma(bad)


def test_error_column_and_atom_sigma(tmp_path):
    from nmrgnn_amd.reweight import atom_sigma, parse_sigma, read_shift_errors
    from nmrgnn_amd.structure import read_shift_table
    t = tmp_path / "shifts.csv"
    t.write_text("resid,name,shift,error\n1,H,8.1,0.2\n\n1,CA,55.0,\n2,N,120.5,abc\n2,H,8.3,-1\n3,CB,30.1,1.5\n")
    table = read_shift_table(str(t))
    err = read_shift_errors(str(t))
    assert len(err) == len(table["shift"]) == 5
    assert err[0] == 0.2 and err[4] == 1.5 and np.isnan(err[1:4]).all()
    t2 = tmp_path / "plain.csv"
    t2.write_text("resid,name,shift\n1,H,8.1\n")
    assert np.isnan(read_shift_errors(str(t2))).all() and len(read_shift_errors(str(t2))) == 1
    elements = ["H", "C", "N", "O", "h"]
    labelled = np.array([True, True, True, False, True])
    s = atom_sigma(elements, labelled, parse_sigma("H=0.3,C=1.1"), errors=np.array([np.nan, 0.7, np.nan, 0.1, np.nan]))
    assert s[0] == 0.3 and s[1] == 0.7 and np.isnan(s[2]) and np.isnan(s[3]) and s[4] == 0.3
    s = atom_sigma(elements, labelled, 0.5)
    assert (s[labelled] == 0.5).all() and np.isnan(s[3])


def test_csv_writers(tmp_path):
    from nmrgnn_amd.reweight import REWEIGHT_COLUMNS, write_reweight_csv, write_weights_csv
    w = np.array([0.1, 1.0 / 3.0, 1.0 - 0.1 - 1.0 / 3.0])
    write_weights_csv(str(tmp_path / "sub" / "o.weights.csv"), w)
    with open(tmp_path / "sub" / "o.weights.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "weight"] and [r[0] for r in rows[1:]] == ["0", "1", "2"]
    assert np.array_equal(np.array([float(r[1]) for r in rows[1:]]), w)      # 17 significant digits: the float64 comes back
    write_reweight_csv(str(tmp_path / "o.csv"), [0, 4], ["ALA", "GLY"], [1, 2], ["H", "CA"], [8.123, 55.0], [0.118, 0.0],
                       [True, False], 12, [8.2, 54.99], [8.05, np.nan], [0.3, np.nan])
    with open(tmp_path / "o.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == REWEIGHT_COLUMNS == ["index", "residues", "resids", "names", "peaks", "peaks_std", "confident", "frames",
                                           "peaks_prior", "target", "sigma"]
    assert rows[1] == ["0", "ALA", "1", "H", "8.12", "0.12", "True", "12", "8.2", "8.05", "0.3"]
    assert rows[2] == ["4", "GLY", "2", "CA", "55.0", "0.0", "False", "12", "54.99", "", ""]


def test_eval_struct_usage_errors_need_no_gpu(tmp_path):
    """the checks that come before any device work"""
    from nmrgnn_amd.main import ReweightUsageError, eval_structure
    t = tmp_path / "s.csv"
    t.write_text("resid,name,shift\n1,H,8.1\n")
    out = str(tmp_path / "o.csv")
    for kw in (dict(reweight=str(t), sigma="0.3"), dict(reweight=str(t), theta=1.0),
               dict(reweight=str(t), theta=1.0, sigma="0.3", average=True),
               dict(reweight=str(t), theta=1.0, sigma="0.3", separate=True),
               dict(reweight=str(t), theta=1.0, sigma="0.3", uncertainty=4),
               dict(reweight=str(t), theta=-1.0, sigma="0.3"), dict(theta=1.0)):
        with pytest.raises(ReweightUsageError):
            eval_structure(("x.pdb",), out, **kw)
