"""Maximum-entropy reweighting end to end on the GPU: ShiftReweighter.fit / scan against the float64 Newton solver of
tests/reweight_ref.py, library.reweight_trajectory on a small model, and eval_structure(reweight=...) / the command line.

Gamma is strictly convex with modulus mu = theta min sigma^2, so a point with |grad|_inf <= g lies within sqrt(M) g / mu of the
minimiser; both solvers stop at g = tol min sigma:

    ||lam - lam*||_2 <= 2 sqrt(M) tol min sigma / (theta min sigma^2),     |log p_t - log p*_t| <= 2 max_t ||d_t||_2 ||dlam||_2
    (log p_t = -lam . d_t - logZ, and logZ is 1-Lipschitz in the logits)"""
import csv
import math
import os

import numpy as np
import pytest
import torch

import reweight_ref as R
from helpers import make_hp, randomize_biases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PDB1 = os.path.join(HERE, "data", "108M.pdb")
PEAK_ATOL = 1e-4          # the constant of tests/test_gpu_parity.py, as tests/test_gpu_receptive.py carries it
SIGMA, TOL = 0.5, 1e-9


# ------------------------------------------------------------------------------------------------- (a) fit against Newton
@pytest.mark.parametrize("T,M,theta,seed", R.END_TO_END)
def test_fit_against_the_reference_newton(gpu_device, T, M, theta, seed):
    from nmrgnn_amd.reweight import ShiftReweighter
    S, y = R.synthetic(T, M, seed)
    ref = R.solve(S, y, SIGMA, theta, tol=1e-12)
    assert ref["converged"] and ref["iterations"] < 50          # the cap that keeps the case honest
    rw = ShiftReweighter(S, y, np.full(M, SIGMA), device=gpu_device)
    res = rw.fit(theta, tol=TOL)
    lam = res.lam.cpu().numpy()
    p = res.weights.cpu().numpy()
    d = S.astype(np.float64) - y.astype(np.float64)[None, :]
    dlam_bound = 2 * math.sqrt(M) * TOL * SIGMA / (theta * SIGMA ** 2)
    dlam = float(np.linalg.norm(lam - ref["lam"]))
    dlogp = float(np.max(np.abs(np.log(p) - np.log(ref["p"]))))
    dlogp_bound = 2 * float(np.max(np.linalg.norm(d, axis=1))) * dlam_bound
    total = math.fsum(p.tolist())
    print(f"fit T={T} M={M} theta={theta}: {res.evaluations} evaluations, ||dlam|| {dlam:.2e} (bound {dlam_bound:.2e}), "
          f"max |dlog p| {dlogp:.2e} (bound {dlogp_bound:.2e}), |sum p - 1| {abs(total - 1):.2e} (bound {T * R.U:.2e}), "
          f"chi2 {res.chi2_prior:.4f} -> {res.chi2_post:.4f}, phi_eff {res.phi_eff:.4f}")
    assert res.converged and res.evaluations <= 2000
    assert res.weights.dtype == torch.float64 and res.weights.is_cuda and tuple(res.weights.shape) == (T,)
    assert dlam <= dlam_bound
    assert dlogp <= dlogp_bound
    assert res.chi2_post < res.chi2_prior
    assert abs(total - 1.0) <= T * R.U
    assert res.theta == theta
    # the reported numbers are those of the weights
    assert res.phi_eff == pytest.approx(ref["phi_eff"], rel=1e-6) and res.kish == pytest.approx(ref["kish"], rel=1e-6)
    assert res.chi2_prior == pytest.approx(ref["chi2_prior"], rel=1e-9) and res.chi2_post == pytest.approx(ref["chi2_post"], rel=1e-5)


def test_fit_returns_the_best_point_when_evaluations_run_out(gpu_device):
    from nmrgnn_amd.reweight import ShiftReweighter
    T, M, theta, seed = R.END_TO_END[1]
    S, y = R.synthetic(T, M, seed)
    rw = ShiftReweighter(torch.from_numpy(S).to(gpu_device), y, SIGMA)
    res = rw.fit(theta, tol=TOL, max_evals=5)
    assert not res.converged and res.evaluations == 5
    assert abs(float(res.weights.sum()) - 1.0) < 1e-12 and res.chi2_post < res.chi2_prior
    prior = np.random.default_rng(0).uniform(0.0, 1.0, T)
    prior[:7] = 0
    res = ShiftReweighter(S, y, SIGMA, prior=prior, device=gpu_device).fit(theta, tol=TOL)
    p = res.weights.cpu().numpy()
    assert res.converged and (p[:7] == 0).all() and (p[7:] > 0).all()
    lw = np.log(np.where(prior > 0, prior, 1.0) / prior.sum())
    lw[:7] = -np.inf
    ref = R.solve(S, y, SIGMA, theta, logw0=lw)
    assert np.max(np.abs(np.log(p[7:]) - np.log(ref["p"][7:]))) <= 2 * np.max(np.linalg.norm(S - y[None], axis=1)) * \
        2 * math.sqrt(M) * TOL * SIGMA / (theta * SIGMA ** 2)


# ---------------------------------------------------------------------------------------------------------------- (b) scan
def test_scan_is_monotone_and_warm_starts_pay(gpu_device):
    from nmrgnn_amd.reweight import ShiftReweighter
    T, M, _, seed = R.END_TO_END[1]
    S, y = R.synthetic(T, M, seed)
    rw = ShiftReweighter(S, y, np.full(M, SIGMA), device=gpu_device)
    thetas = [1, 8, 2, 4]
    results = rw.scan(thetas, tol=TOL)
    assert [r.theta for r in results] == [8.0, 4.0, 2.0, 1.0] and all(r.converged for r in results)
    for a, b in zip(results, results[1:]):
        assert b.chi2_post <= a.chi2_post and b.phi_eff <= a.phi_eff
    cold = [rw.fit(t, tol=TOL) for t in (8, 4, 2, 1)]
    print(f"scan: warm {[r.evaluations for r in results]}, cold {[r.evaluations for r in cold]}")
    assert sum(r.evaluations for r in results) <= sum(r.evaluations for r in cold)
    for w, c in zip(results, cold):
        assert float((w.lam - c.lam).norm()) <= 2 * math.sqrt(M) * TOL * SIGMA / (w.theta * SIGMA ** 2)


# ------------------------------------------------------------------------------------------------- (c) reweight_trajectory
N_ATOMS, N_FRAMES = 60, 8


def _small_structure():
    from nmrgnn_amd.structure import Structure, atoms_onehot, read_pdb
    s = read_pdb(PDB1)
    k = N_ATOMS
    rng = np.random.default_rng(4)
    first = np.asarray(s.frames[0][:k], np.float32)
    frames = [first] + [np.round(first + 0.2 * rng.standard_normal((k, 3)), 3).astype(np.float32) for _ in range(N_FRAMES - 1)]
    small = Structure(s.names[:k], s.resnames[:k], s.resids[:k], s.elements[:k], frames, [None] * N_FRAMES)
    return small, atoms_onehot(small.elements)


def _unit_scale_model(dev, num_elem):
    """a random-weight F = 64 model with the per-element output scaling of tests/test_gpu_receptive.py (std in [0.5, 2])"""
    from nmrgnn_amd.model import GNNModel
    rng = np.random.default_rng(5)
    std, avg = rng.uniform(0.5, 2.0, 10).astype(np.float32), rng.uniform(-1.0, 1.0, 10).astype(np.float32)
    model = GNNModel(make_hp(atom_feature_size=64), {k: ("X", float(avg[k]), float(std[k])) for k in range(10)}, device=dev, seed=3)
    model.build(num_elem)
    randomize_biases(model.engine)
    return model, std


def test_reweight_trajectory(gpu_device):
    from nmrgnn_amd.graph import frames_to_batch
    from nmrgnn_amd.library import reweight_trajectory
    from nmrgnn_amd.reweight import ShiftReweighter
    s, atoms = _small_structure()
    n = s.n_atoms
    model, std = _unit_scale_model(gpu_device, atoms.shape[1])
    frames = np.stack(s.frames)
    own = model(frames_to_batch(atoms, frames, 16, device=gpu_device)).detach().reshape(N_FRAMES, n)
    own_h = own.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(6)
    labelled = np.zeros(n, bool)
    labelled[rng.choice(n, n // 3, replace=False)] = True
    spread = float(own_h.std(axis=0)[labelled].mean())
    assert spread > 0
    targets = np.where(labelled, own_h.mean(axis=0) + 0.5 * spread * rng.standard_normal(n), np.nan)
    sigma, theta = spread, 2.0
    res, shifts = reweight_trajectory(model, atoms, frames, targets, sigma, theta, tol=1e-8)
    assert torch.equal(shifts, own) and res.converged
    idx = np.nonzero(labelled)[0]
    by_hand = ShiftReweighter(own[:, torch.from_numpy(idx).to(gpu_device)].contiguous(), targets[idx], np.full(len(idx), sigma))
    want = by_hand.fit(theta, tol=1e-8)
    assert torch.equal(res.weights, want.weights) and torch.equal(res.lam, want.lam)      # the same path: the same bits
    assert res.evaluations == want.evaluations and res.chi2_post < res.chi2_prior
    # prune=True: the labelled columns only, the same shifts within the pruned-versus-full tolerance of
    # tests/test_gpu_receptive.py (PEAK_ATOL std_e + 2^-23 |shift| per entry), and weights as close as that allows:
    # the two objectives' gradients differ at any lam by at most G = sqrt(M) (eps + (exp(2 eta) - 1) max |d|), eta = ||lam||_1 eps,
    # so their minimisers by G / (theta sigma^2) plus the two stopping tolerances, and log p by 2 (eta + max ||d_t|| ||dlam||)
    # (a worst case: on these 60 atoms four list steps from 20 labelled atoms reach nearly everything, so the pruned run
    # differs from the full one in last bits or not at all, and the printed figures sit far below the bound)
    res_p, shifts_p = reweight_trajectory(model, atoms, frames, targets, sigma, theta, prune=True, tol=1e-8)
    assert tuple(shifts_p.shape) == (N_FRAMES, len(idx)) and res_p.converged
    full = own_h[:, idx]
    eps_tm = PEAK_ATOL * std[np.argmax(atoms[idx], axis=1)].astype(np.float64)[None, :] + 2.0 ** -23 * np.abs(full)
    assert (np.abs(shifts_p.cpu().numpy() - full) <= eps_tm).all()
    M, eps = len(idx), float(eps_tm.max())
    d = full - targets[idx].astype(np.float32).astype(np.float64)[None, :]
    lam1 = max(float(res.lam.abs().sum()), float(res_p.lam.abs().sum()))
    eta = lam1 * eps
    G = math.sqrt(M) * (eps + math.expm1(2 * eta) * float(np.abs(d).max()))
    dlam = (G + 2 * math.sqrt(M) * 1e-8 * sigma) / (theta * sigma ** 2)
    bound = 2 * (eta + (float(np.max(np.linalg.norm(d, axis=1))) + math.sqrt(M) * eps) * dlam)
    got = float(np.max(np.abs(np.log(res_p.weights.cpu().numpy()) - np.log(res.weights.cpu().numpy()))))
    print(f"reweight_trajectory prune: max |dlog p| {got:.2e} (bound {bound:.2e}), ||dlam|| "
          f"{float((res_p.lam - res.lam).norm()):.2e} (bound {dlam:.2e})")
    assert got <= bound and float((res_p.lam - res.lam).norm()) <= dlam
    # refusals
    with pytest.raises(ValueError, match="no atom is labelled"):
        reweight_trajectory(model, atoms, frames, np.full(n, np.nan), sigma, theta)
    bad = np.full(n, sigma)
    bad[idx[0]] = 0.0
    with pytest.raises(ValueError, match="sigma"):
        reweight_trajectory(model, atoms, frames, targets, bad, theta)
    bad[idx[0]] = np.nan
    with pytest.raises(ValueError, match="sigma"):
        reweight_trajectory(model, atoms, frames, targets, bad, theta)


# ------------------------------------------------------------------------------------------------------ (d) eval-struct
def _write_trajectory(path, s):
    lines = []
    for m, frame in enumerate(s.frames):
        lines.append("MODEL     %4d\n" % (m + 1))
        for k in range(s.n_atoms):
            nm = s.names[k] if len(s.names[k]) == 4 else " " + s.names[k]
            lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s\n"
                         % (k + 1, nm, s.resnames[k], s.resids[k], frame[k, 0], frame[k, 1], frame[k, 2], s.elements[k]))
        lines.append("ENDMDL\n")
    path.write_text("".join(lines))


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_eval_struct_reweight(gpu_device, tmp_path):
    from click.testing import CliRunner
    from nmrgnn_amd.main import ReweightUsageError, eval_structure, main
    from nmrgnn_amd.reweight import REWEIGHT_COLUMNS
    s, _ = _small_structure()
    n = s.n_atoms
    traj = tmp_path / "traj.pdb"
    _write_trajectory(traj, s)
    quiet = dict(keep_going=True, echo=lambda *a: None)
    eval_structure((str(traj),), str(tmp_path / "avg.csv"), average=True, **quiet)
    avg = _rows(tmp_path / "avg.csv")
    assert len(avg) == n + 1
    mean = np.array([float(r[4]) for r in avg[1:]])
    rng = np.random.default_rng(8)
    pick = np.sort(rng.choice(n, n // 3, replace=False))
    table = tmp_path / "shifts.csv"
    with open(table, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["resid", "name", "shift", "error"])
        for j, i in enumerate(pick):
            wr.writerow([int(s.resids[i]), s.names[i], f"{mean[i] + 0.3 * rng.standard_normal():.3f}", "0.25" if j == 0 else ""])
    spec = ",".join(f"{e}=0.5" for e in sorted({str(e).upper() for e in s.elements}))
    lines = []
    eval_structure((str(traj),), str(tmp_path / "rw.csv"), reweight=str(table), theta=2.0, sigma=spec, keep_going=True,
                   echo=lines.append)
    rw = _rows(tmp_path / "rw.csv")
    assert rw[0] == REWEIGHT_COLUMNS and len(rw) == n + 1
    assert [r[:4] for r in rw[1:]] == [r[:4] for r in avg[1:]] and all(r[7] == str(N_FRAMES) for r in rw[1:])
    assert [r[8] for r in rw[1:]] == [r[4] for r in avg[1:]]                  # peaks_prior is the --average mean
    labelled = np.zeros(n, bool)
    labelled[pick] = True
    for i, r in enumerate(rw[1:]):
        assert (r[9] != "") == bool(labelled[i]) and (r[10] != "") == bool(labelled[i])
    assert float(rw[1 + pick[0]][10]) == 0.25 and all(float(rw[1 + i][10]) == 0.5 for i in pick[1:])
    assert all(float(r[5]) >= 0 for r in rw[1:]) and any(r[4] != r[8] for r in rw[1:])
    wfile = _rows(tmp_path / "rw.weights.csv")
    assert wfile[0] == ["frame", "weight"] and [r[0] for r in wfile[1:]] == [str(k) for k in range(N_FRAMES)]
    w = np.array([float(r[1]) for r in wfile[1:]])
    assert (w > 0).all() and abs(math.fsum(w.tolist()) - 1.0) <= 1e-12
    summary = [ln for ln in lines if "phi_eff" in ln]
    assert len(summary) == 1 and "theta 2" in summary[0] and "->" in summary[0] and "evaluations" in summary[0] and \
        "converged" in summary[0] and "NOT" not in summary[0]
    # the weighted mean lies between the frames' extremes and moves towards the targets
    chi = [float(x) for x in summary[0].split("chi2 ")[1].split(",")[0].split(" -> ")]
    assert chi[1] < chi[0]
    # the command line writes the same bytes; --atom-names keeps the labelled atoms among the selected
    res = CliRunner().invoke(main, ["eval-struct", "--keep-going", "--reweight", str(table), "--theta", "2", "--sigma", spec,
                                    str(traj), str(tmp_path / "cli.csv")])
    assert res.exit_code == 0, res.output
    assert (tmp_path / "cli.csv").read_bytes() == (tmp_path / "rw.csv").read_bytes()
    assert (tmp_path / "cli.weights.csv").read_bytes() == (tmp_path / "rw.weights.csv").read_bytes()
    names = sorted({s.names[i] for i in pick[:4]})
    eval_structure((str(traj),), str(tmp_path / "sel.csv"), reweight=str(table), theta=2.0, sigma="0.5", atom_names=names, **quiet)
    sel = _rows(tmp_path / "sel.csv")
    assert sel[0] == REWEIGHT_COLUMNS and {r[3] for r in sel[1:]} == set(names)
    assert sum(r[9] != "" for r in sel[1:]) == sum(1 for i in pick if s.names[i] in names)
    assert len(_rows(tmp_path / "sel.weights.csv")) == N_FRAMES + 1
    # usage errors
    out = str(tmp_path / "no.csv")
    with pytest.raises(ReweightUsageError, match="theta"):
        eval_structure((str(traj),), out, reweight=str(table), sigma=spec, **quiet)
    with pytest.raises(ReweightUsageError, match="average"):
        eval_structure((str(traj),), out, reweight=str(table), theta=2.0, sigma=spec, average=True, **quiet)
    plain = tmp_path / "plain.csv"
    plain.write_text("".join(ln.rsplit(",", 1)[0] + "\n" for ln in table.read_text().splitlines()))      # no error column
    with pytest.raises(ReweightUsageError, match="has no sigma"):
        eval_structure((str(traj),), out, reweight=str(plain), theta=2.0, sigma="Xx=0.5", **quiet)
    unlabelled = sorted({s.names[i] for i in range(n)} - {s.names[i] for i in pick})
    if unlabelled:
        with pytest.raises(ReweightUsageError, match="no labelled atom"):
            eval_structure((str(traj),), out, reweight=str(table), theta=2.0, sigma=spec, atom_names=unlabelled[:1], **quiet)
    for args in (["--reweight", str(table), "--sigma", spec], ["--reweight", str(table), "--theta", "2"],
                 ["--reweight", str(table), "--theta", "2", "--sigma", spec, "--average"],
                 ["--reweight", str(table), "--theta", "2", "--sigma", spec, "--uncertainty", "2"],
                 ["--reweight", str(table), "--theta", "2", "--sigma", spec, "--separate"], ["--theta", "2"]):
        res = CliRunner().invoke(main, ["eval-struct"] + args + [str(traj), out])
        assert res.exit_code == 2, (args, res.output)
    assert not os.path.exists(out)
