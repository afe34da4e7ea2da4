"""Bayesian / maximum-entropy reweighting of a trajectory against measured shifts: which weights on the
frames make the ensemble agree with experiment, and how much of the ensemble survives.

With the predicted shifts ``S [T frames, M labelled atoms]``, targets ``y``, errors ``sigma``, prior weights ``w0`` and a
regularisation strength ``theta > 0`` the weights are ``p_t ∝ w0_t exp(-lambda . (S_t - y))`` at the unique minimiser of

    Gamma(lambda) = log sum_t w0_t exp(-lambda . d_t) + theta/2 sum_m sigma_m^2 lambda_m^2,      d_tm = S_tm - y_m
    grad_m        = -sum_t p_t d_tm + theta sigma_m^2 lambda_m

``ShiftReweighter`` holds ``S`` on the device as float32 and minimises ``Gamma`` with L-BFGS; every evaluation is ONE call of
``ng_reweight_eval`` (csrc/reweight.hip: one pass over ``S``, float64 sums, a running maximum, bitwise deterministic), the
weights and their entropy come from ``ng_reweight_weights``.  There is no CPU path.

The helpers at the end (``parse_sigma``, ``read_shift_errors``, ``atom_sigma`` and the two CSV writers) serve ``eval-struct
--reweight`` and need no GPU."""
from __future__ import annotations

import csv
import gzip
import math
import os
from dataclasses import dataclass, field

import numpy as np

MAX_OBSERVABLES = 16384       # ng_reweight_eval: columns of S


@dataclass
class ReweightResult:
    """``weights``: float64 [T] on the device, summing to 1.  ``lam``: float64 [M] on the device.  ``phi_eff`` =
    exp(-sum p log(p / w0)), the effective fraction of frames that survive; ``kish`` = 1 / (T sum p^2); ``chi2_prior`` /
    ``chi2_post``: mean_m ((<S_m> - y_m) / sigma_m)^2 under the prior and under the weights; ``evaluations``: calls of
    (Gamma, grad) the optimiser made; ``converged``: max_m |grad_m| <= tol * min_m sigma_m at ``lam``."""
    weights: object
    lam: object
    theta: float
    phi_eff: float
    kish: float
    chi2_prior: float
    chi2_post: float
    evaluations: int
    converged: bool
    history: object = field(default=None, repr=False, compare=False)      # (theta, L-BFGS pairs): what ``scan`` hands on


class _Stop(Exception):
    """leaves the optimiser from inside an evaluation: converged, or out of evaluations"""


class ShiftReweighter:
    """``shifts`` [T, M] float32 (a device tensor is used as it stands), ``targets`` and ``sigma`` [M] (targets are held as
    float32, like the shifts; sigma > 0), ``prior`` [T] with entries >= 0 and a positive sum (normalised once, on the host;
    None: uniform).  Holds ``S`` on the device and the device's library context.  Only ``ng_reweight_eval`` and
    ``ng_reweight_weights`` read ``S`` during a fit."""

    def __init__(self, shifts, targets, sigma, prior=None, device=None):
        import torch
        from . import _lib
        if isinstance(shifts, torch.Tensor):
            if device is None and shifts.is_cuda:
                device = shifts.device
        else:
            shifts = torch.from_numpy(np.ascontiguousarray(np.asarray(shifts), dtype=np.float32))
        if shifts.dim() != 2 or shifts.shape[0] < 1 or shifts.shape[1] < 1:
            raise ValueError(f"ShiftReweighter: shifts must be [T, M] with T, M >= 1, got {tuple(shifts.shape)}")
        T, M = int(shifts.shape[0]), int(shifts.shape[1])
        if M > MAX_OBSERVABLES:
            raise ValueError(f"ShiftReweighter: {M} observables, at most {MAX_OBSERVABLES}")
        y = np.asarray(_host(targets), np.float64).reshape(-1)
        sg = np.asarray(_host(sigma), np.float64).reshape(-1)
        if sg.size == 1 and M > 1:
            sg = np.full(M, float(sg[0]))
        if y.shape != (M,) or sg.shape != (M,):
            raise ValueError(f"ShiftReweighter: targets and sigma need {M} entries, got {y.shape} and {sg.shape}")
        if not np.isfinite(y).all():
            raise ValueError("ShiftReweighter: targets must be finite")
        if not (np.isfinite(sg).all() and (sg > 0).all()):
            raise ValueError("ShiftReweighter: sigma must be finite and > 0")
        logw0 = None
        if prior is not None:
            w0 = np.asarray(_host(prior), np.float64).reshape(-1)
            if w0.shape != (T,):
                raise ValueError(f"ShiftReweighter: prior needs {T} entries, got {w0.shape}")
            if not np.isfinite(w0).all() or (w0 < 0).any() or not w0.sum() > 0:
                raise ValueError("ShiftReweighter: prior entries must be finite and >= 0 with a positive sum")
            with np.errstate(divide="ignore"):
                logw0 = np.log(w0 / w0.sum())
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise ValueError("ShiftReweighter runs on the GPU: pass a cuda device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.ctx = _lib.get_context(device.index)
        self.T, self.M = T, M
        self.S = shifts.detach().to(device=device, dtype=torch.float32).contiguous()
        self.y = torch.from_numpy(y.astype(np.float32)).to(device)
        self.sigma = torch.from_numpy(sg).to(device)
        self.sigma_min = float(sg.min())
        self._sig2 = self.sigma * self.sigma
        self.logw0 = None if logw0 is None else torch.from_numpy(logw0).to(device)
        self._chi2_prior = None

    # ------------------------------------------------------------------------------------------------------ the kernels
    def _stream(self):
        import torch
        from . import _lib
        return _lib._vp(torch.cuda.current_stream(self.device).cuda_stream)

    def evaluate(self, lam):
        """``{logZ, mean_0 .. mean_{M-1}}`` float64 [1 + M] on the device at ``lam`` (float64 [M] on the device): one
        ``ng_reweight_eval`` call, queued on the current stream"""
        import torch
        from ._lib import ptr
        out = torch.empty(1 + self.M, dtype=torch.float64, device=self.device)
        self.ctx.check(self.ctx.lib.ng_reweight_eval(self.ctx.handle, self._stream(), self.T, self.M, ptr(self.S), ptr(self.y),
                                                     ptr(self.logw0), ptr(lam), ptr(out)), "ng_reweight_eval")
        return out

    def weights(self, lam, logZ):
        """``(p float64 [T], stats float64 [2] = {sum p log(p / w0), sum p^2})`` on the device (``ng_reweight_weights``);
        ``logZ``: a float64 device tensor, as ``evaluate(lam)[0:1]``"""
        import torch
        from ._lib import ptr
        p = torch.empty(self.T, dtype=torch.float64, device=self.device)
        stats = torch.empty(2, dtype=torch.float64, device=self.device)
        self.ctx.check(self.ctx.lib.ng_reweight_weights(self.ctx.handle, self._stream(), self.T, self.M, ptr(self.S),
                                                        ptr(self.y), ptr(self.logw0), ptr(lam), ptr(logZ), ptr(p), ptr(stats)),
                       "ng_reweight_weights")
        return p, stats

    def _chi2(self, out):
        return float(((out[1:] / self.sigma) ** 2).mean().item())

    def chi2_prior(self):
        if self._chi2_prior is None:
            import torch
            self._chi2_prior = self._chi2(self.evaluate(torch.zeros(self.M, dtype=torch.float64, device=self.device)))
        return self._chi2_prior

    # ------------------------------------------------------------------------------------------------------------ the fit
    def fit(self, theta, lam0=None, tol=1e-6, max_evals=2000, history=None):
        """Minimise Gamma at ``theta`` from ``lam0`` (default 0) with L-BFGS on a float64 ``lambda`` (``_lbfgs``: a line
        search on the gradient alone).  Converged: max_m |grad_m| <= tol * min_m sigma_m.  After ``max_evals`` evaluations
        without that, or at the rounding floor of the gradient, the best point found (smallest max |grad|) is returned
        with ``converged=False``; no exception.  ``history``: the ``history`` of a result at another theta on the same data
        (``scan``) — its curvature pairs (s, y) start this fit's L-BFGS memory, each y shifted by the exactly known change
        of the regulariser's Hessian, (theta - theta_old) sigma^2 s."""
        import torch
        theta = float(theta)
        if not (theta > 0 and math.isfinite(theta)):
            raise ValueError(f"fit: theta must be finite and > 0, got {theta}")
        max_evals = max(1, int(max_evals))
        gtol = float(tol) * self.sigma_min
        # the optimiser's M-vectors live on the host: an evaluation costs one small copy each way and the kernel, where
        # the hundred-odd small device launches of an L-BFGS update cost more than the kernel
        if lam0 is None:
            start = torch.zeros(self.M, dtype=torch.float64)
        else:
            start = torch.as_tensor(_host(lam0), dtype=torch.float64).reshape(-1).clone()
            if start.shape[0] != self.M:
                raise ValueError(f"fit: lam0 needs {self.M} entries")
        sig2 = self._sig2.cpu()
        state = {"evals": 0, "best": None, "converged": False}      # best: (max |grad|, lam on the host, out, lam on the device)

        def point(lam_now):
            """(Gamma, grad, max |grad|) at lam_now: one evaluation; keeps the best point and leaves through _Stop"""
            if state["evals"] >= max_evals:
                raise _Stop
            lam_dev = lam_now.to(self.device)
            out = self.evaluate(lam_dev)
            out_h = out.cpu()                          # the host's read of an evaluation: 1 + M doubles
            state["evals"] += 1
            reg = theta * sig2 * lam_now
            gamma = out_h[0] + 0.5 * (reg * lam_now).sum()
            grad = reg - out_h[1:]
            gmax = float(grad.abs().max())
            best = state["best"]
            if best is None or gmax < best[0] or (best[0] != best[0] and gmax == gmax):
                state["best"] = (gmax, lam_now.clone(), out, lam_dev)
            if gmax <= gtol:
                state["converged"] = True
                raise _Stop
            return gamma, grad, gmax

        pairs = []
        if history is not None:
            theta_old, old = history
            for s_, y_, _ in old:
                y_new = y_ + (theta - theta_old) * sig2 * s_
                sy = float(torch.dot(s_, y_new))
                if sy > 0:
                    pairs.append((s_, y_new, 1.0 / sy))
        try:
            self._lbfgs(point, start, pairs)
        except _Stop:
            pass
        if state["best"] is None:      # not reachable: the first evaluation always records a point
            raise RuntimeError("fit: no evaluation was made")
        _, _, out, lam_best = state["best"]
        p, stats = self.weights(lam_best, out[0:1])
        s = stats.cpu().numpy()
        return ReweightResult(weights=p, lam=lam_best, theta=theta, phi_eff=float(math.exp(-s[0])),
                              kish=float(1.0 / (self.T * s[1])) if s[1] > 0 else float("nan"),
                              chi2_prior=self.chi2_prior(), chi2_post=self._chi2(out), evaluations=state["evals"],
                              converged=bool(state["converged"]), history=(theta, pairs))

    @staticmethod
    def _lbfgs(point, x, pairs, history=20, max_ls=20, c2=0.9):
        """L-BFGS whose line search reads the gradient only.  Along a direction d with phi'(t) = grad(x + t d) . d a step is
        kept when |phi'(t)| <= c2 |phi'(0)| (the curvature half of the strong-Wolfe pair); otherwise the zero of phi' is
        sought by the secant rule, outwards while phi' < 0 and inside the bracket once it has changed sign.  Gamma is
        strictly convex, so phi' rises along every line and such a step lowers Gamma; the search never compares values of
        Gamma, whose rounding hides a decrease of |grad|^2 / (2 theta sigma^2) once max |grad| is near 1e-8 (where
        torch.optim.LBFGS with the strong-Wolfe search stops short of tol = 1e-9).  Ends through ``point`` (_Stop: converged or
        out of evaluations), or where not even the plain gradient direction gives such a step: the rounding floor.
        ``pairs``: the memory, a list of (s, y, 1 / s.y), oldest first, changed in place."""
        import torch
        _, g, _ = point(x)
        while True:
            q = g.clone()
            alphas = []
            for s_, y_, rho in reversed(pairs):
                al = rho * float(torch.dot(s_, q))
                alphas.append(al)
                q.add_(y_, alpha=-al)
            if pairs:
                s_, y_, _ = pairs[-1]
                q.mul_(float(torch.dot(s_, y_)) / float(torch.dot(y_, y_)))
            for (s_, y_, rho), al in zip(pairs, reversed(alphas)):
                q.add_(s_, alpha=al - rho * float(torch.dot(y_, q)))
            d = -q
            gd = float(torch.dot(g, d))
            if not gd < 0:
                if not pairs:
                    return
                del pairs[:]
                continue
            t = 1.0 if pairs else min(1.0, 1.0 / float(g.abs().sum()))
            lo, hi, done = (0.0, gd), None, False
            for _ in range(max_ls):
                x_new = x + t * d
                _, g_new, _ = point(x_new)
                gd_new = float(torch.dot(g_new, d))
                if abs(gd_new) <= c2 * abs(gd):
                    done = True
                    break
                if gd_new < 0:
                    lo = (t, gd_new)
                else:
                    hi = (t, gd_new)
                if hi is None:      # still descending: outwards, by the secant through the last two points, 2 to 10 times t
                    sec = t - gd_new * (t - 0.0) / (gd_new - gd) if gd_new != gd else 10.0 * t
                    t = min(10.0 * t, max(2.0 * t, sec))
                else:               # the zero of phi' lies between lo and hi
                    w = hi[0] - lo[0]
                    sec = lo[0] - lo[1] * w / (hi[1] - lo[1])
                    t = min(hi[0] - 0.1 * w, max(lo[0] + 0.1 * w, sec))
            if not done:
                if not pairs:
                    return
                del pairs[:]
                continue
            s_, y_ = x_new - x, g_new - g
            sy = float(torch.dot(s_, y_))
            if sy > 0:
                pairs.append((s_, y_, 1.0 / sy))
                del pairs[:-history]
            x, g = x_new, g_new

    def scan(self, thetas, tol=1e-6, max_evals=2000):
        """``fit`` at every theta in DESCENDING order, each warm-started from the previous ``lambda``: the list of results in
        that order — the curve (chi2_post against phi_eff) from which theta is chosen.  The L-BFGS memory is handed on too."""
        results, lam, history = [], None, None
        for theta in sorted((float(t) for t in thetas), reverse=True):
            r = self.fit(theta, lam0=lam, tol=tol, max_evals=max_evals, history=history)
            results.append(r)
            lam, history = r.lam, r.history
        return results


def _host(x):
    """array-likes and tensors alike as something NumPy takes"""
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def weighted_moments(mu, p):
    """``(mean, var)`` float32 [N] on the device of the shifts ``mu`` [T, N] (float32, device) under the frame weights ``p``
    [T] (float64, device, summing to 1): ``ng_weighted_moments`` — float64 sums over the frames in a fixed order, the
    population variance, 0 for a column of equal values"""
    import torch
    from . import _lib
    from ._lib import ptr
    if not (isinstance(mu, torch.Tensor) and mu.is_cuda and mu.dim() == 2 and mu.shape[0] >= 1):
        raise ValueError("weighted_moments: mu must be a [T, N] device tensor with T >= 1")
    T, N = int(mu.shape[0]), int(mu.shape[1])
    mu = mu.to(torch.float32).contiguous()
    p = torch.as_tensor(p, dtype=torch.float64, device=mu.device).contiguous()
    if tuple(p.shape) != (T,):
        raise ValueError(f"weighted_moments: p needs {T} entries, got {tuple(p.shape)}")
    ctx = _lib.get_context(mu.device.index if mu.device.index is not None else torch.cuda.current_device())
    mean = torch.empty(N, dtype=torch.float32, device=mu.device)
    var = torch.empty(N, dtype=torch.float32, device=mu.device)
    st = _lib._vp(torch.cuda.current_stream(mu.device).cuda_stream)
    ctx.check(ctx.lib.ng_weighted_moments(ctx.handle, st, T, N, ptr(mu), ptr(p), ptr(mean), ptr(var)), "ng_weighted_moments")
    return mean, var


# ---------------------------------------------------------------------------------------- command-line helpers (no GPU)
def parse_sigma(spec):
    """``--sigma SPEC``: one number (ppm, for every labelled atom) gives a float; ``H=0.3,C=1.1,N=2.5`` gives ``{element:
    ppm}``.  ``ValueError`` for anything else, and for a value that is not finite and > 0."""
    text = str(spec).strip()
    if not text:
        raise ValueError("--sigma: empty")

    def number(s, what):
        try:
            v = float(s)
        except ValueError:
            raise ValueError(f"--sigma: {what} {s!r} is no number") from None
        if not (math.isfinite(v) and v > 0):
            raise ValueError(f"--sigma: {what} {s!r} must be finite and > 0")
        return v

    if "=" not in text:
        return number(text, "value")
    out = {}
    for part in text.split(","):
        if not part.strip():
            continue
        if part.count("=") != 1:
            raise ValueError(f"--sigma: {part.strip()!r} is not ELEMENT=VALUE")
        el, val = (s.strip() for s in part.split("="))
        if not el:
            raise ValueError(f"--sigma: {part.strip()!r} names no element")
        if el.upper() in out:
            raise ValueError(f"--sigma: element {el} given twice")
        out[el.upper()] = number(val, f"value of {el}")
    if not out:
        raise ValueError("--sigma: empty")
    return out


def read_shift_errors(path):
    """float64 [m]: the ``error`` column of a shift table, one entry per row that ``structure.read_shift_table`` returns (the
    same rows in the same order: blank lines are skipped), NaN where the column is absent, blank, non-numeric, not finite
    or not > 0"""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt", newline="") as f:
        rd = csv.reader(f)
        try:
            header = [h.strip().lower() for h in next(rd)]
        except StopIteration:
            raise ValueError(f"{path}: empty shift table") from None
        at = header.index("error") if "error" in header else None
        out = []
        for row in rd:
            if not row or all(not c.strip() for c in row):
                continue
            v = float("nan")
            if at is not None and at < len(row):
                try:
                    v = float(row[at])
                except ValueError:
                    v = float("nan")
            out.append(v if (math.isfinite(v) and v > 0) else float("nan"))
    return np.asarray(out, np.float64)


def atom_sigma(elements, labelled, spec, errors=None):
    """float64 [n]: the error of every atom — ``errors[i]`` where it is finite (the table's ``error`` column laid on the
    atoms), else ``spec`` (``parse_sigma``: a float, or a dict by the upper-cased element), NaN where neither gives one and
    on atoms that are not ``labelled``"""
    elements = [str(e).strip().upper() for e in elements]
    labelled = np.asarray(labelled, bool)
    n = len(elements)
    if isinstance(spec, dict):
        out = np.array([spec.get(e, np.nan) for e in elements], np.float64)
    elif spec is None:
        out = np.full(n, np.nan)
    else:
        out = np.full(n, float(spec))
    if errors is not None:
        errors = np.asarray(errors, np.float64)
        out = np.where(np.isfinite(errors), errors, out)
    out[~labelled] = np.nan
    return out


def write_weights_csv(path, weights):
    """``frame, weight`` per frame read, the weight with 17 significant digits (a float64 round trip)"""
    w = np.asarray(_host(weights), np.float64).reshape(-1)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["frame", "weight"])
        for i, v in enumerate(w):
            wr.writerow([i, f"{v:.17g}"])


REWEIGHT_COLUMNS = ["index", "residues", "resids", "names", "peaks", "peaks_std", "confident", "frames", "peaks_prior",
                    "target", "sigma"]


def write_reweight_csv(path, index, residues, resids, names, peaks, peaks_std, confident, frames, peaks_prior, target, sigma):
    """One row per atom, the columns ``REWEIGHT_COLUMNS``: ``peaks`` / ``peaks_std`` the weighted mean and standard
    deviation, ``peaks_prior`` the unweighted mean (all rounded to 0.01 ppm like every peaks column), ``target`` and
    ``sigma`` blank where the atom has no label (NaN)"""
    peaks = np.round(np.asarray(peaks, np.float64), 2)
    peaks_std = np.round(np.asarray(peaks_std, np.float64), 2)
    peaks_prior = np.round(np.asarray(peaks_prior, np.float64), 2)
    target, sigma = np.asarray(target, np.float64), np.asarray(sigma, np.float64)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(REWEIGHT_COLUMNS)
        for j in range(len(peaks)):
            has = bool(np.isfinite(target[j]))
            wr.writerow([int(index[j]), residues[j], int(resids[j]), names[j], peaks[j], peaks_std[j], bool(confident[j]),
                         int(frames), peaks_prior[j], float(target[j]) if has else "",
                         float(sigma[j]) if has and np.isfinite(sigma[j]) else ""])
