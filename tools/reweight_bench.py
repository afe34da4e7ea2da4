"""What one evaluation of the reweighting objective costs: log-partition function and ensemble mean of
S [T frames][M shifts] under the weights exp(-lambda . (S_t - y)).

At T = ``--frames`` (100000) and M = 1024 (backbone and CB shifts of a ~250-residue protein; the one-pass register form) and
M = 4096 (the two-pass form), median (min, max) over ``--reps`` alternating rounds of ``--launches`` back-to-back calls between
device events, 5 warm-up calls each:

  1. ``ng_reweight_eval`` through the C entry point (float32 S, float64 sums, one pass / two passes over S);
  2. the same quantity in torch float64 on a float64 COPY of S (a matrix-vector product, a logsumexp, a second product);
  3. the same in torch float32 on S itself;
  4. host wall time per evaluation inside ``ShiftReweighter.fit`` (the kernel plus the optimiser's vector operations and its
     scalar reads), from a fit that is stopped after ``--evals`` evaluations.

Each time is also given as bytes of S (4 T M, once) over time, against the 6.3 TB/s that MI355X_MICROARCH.md gives as achievable
from HBM.  The three results are also compared with each other: the kernel and the float64 torch path must agree to rounding,
and the float32 path's distance from them is printed, because that distance is one reason the kernel exists.
usage: python tools/reweight_bench.py [--frames T] [--reps N] [--launches L] [--evals E] [out.txt]"""
import ctypes as C
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrgnn_amd import _lib  # noqa: E402
from nmrgnn_amd._lib import ptr  # noqa: E402
from nmrgnn_amd.reweight import ShiftReweighter  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)
HBM = 6.3e12


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fns, launches, reps):
    """median, min, max us per call of every leg, the legs alternating"""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    return [(statistics.median(u), min(u), max(u)) for u in us]


def one_shape(T, M, launches, reps, evals, out):
    g = torch.Generator(device=dev).manual_seed(M)
    offsets = 1.0 + 129.0 * torch.rand(M, device=dev, generator=g)
    S = offsets[None, :] + 1.5 * torch.randn(T, M, device=dev, generator=g)
    y = (S.mean(dim=0) + 0.7 * torch.randn(M, device=dev, generator=g)).float()
    lam = (0.3 / np.sqrt(M)) * torch.randn(M, device=dev, dtype=torch.float64, generator=g)
    ctx = _lib.get_context(dev.index)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    o = torch.empty(1 + M, dtype=torch.float64, device=dev)
    logw = -float(np.log(T))

    def kernel():
        ctx.check(ctx.lib.ng_reweight_eval(ctx.handle, st, T, M, ptr(S), ptr(y), None, ptr(lam), ptr(o)), "ng_reweight_eval")

    S64, y64 = S.double(), y.double()
    lam32 = lam.float()
    res = {}

    def torch64():
        a = logw - (S64 @ lam - torch.dot(y64, lam))
        logZ = torch.logsumexp(a, 0)
        res["t64"] = (logZ, torch.exp(a - logZ) @ S64 - y64)

    def torch32():
        a = logw - (S @ lam32 - torch.dot(y, lam32))
        logZ = torch.logsumexp(a, 0)
        res["t32"] = (logZ, torch.exp(a - logZ) @ S - y)

    t = timed([kernel, torch64, torch32], launches, reps)
    nbytes = 4.0 * T * M
    out(f"T = {T}, M = {M} ({'one-pass register form' if M <= 2048 else 'two-pass form'}), S = {nbytes / 1e6:.0f} MB float32, "
        f"{launches} calls back to back, {reps} alternating rounds; median (min, max) us per evaluation, bytes of S / time, share of "
        f"6.3 TB/s:")
    for name, (med, lo, hi) in zip(("1. ng_reweight_eval", "2. torch float64 on a float64 copy of S", "3. torch float32"), t):
        out(f"    {name}: {med:.1f} ({lo:.1f}, {hi:.1f}) us, {nbytes / med / 1e6:.2f} TB/s, {nbytes / med * 1e6 / HBM * 100:.0f} %")
    out(f"    ng_reweight_eval / torch float64 = {t[0][0] / t[1][0]:.2f}, / torch float32 = {t[0][0] / t[2][0]:.2f} (time ratios; "
        f"the float64 path also holds {2 * nbytes / 1e6:.0f} MB more)")
    kernel()
    torch.cuda.synchronize()
    k0, km = float(o[0]), o[1:]
    z64, m64 = res["t64"]
    z32, m32 = res["t32"]
    out(f"    agreement: |logZ - torch64| = {abs(k0 - float(z64)):.2e}, max |mean - torch64| = {float((km - m64).abs().max()):.2e}; "
        f"torch32: |dlogZ| = {abs(float(z32) - float(z64)):.2e}, max |dmean| = {float((m32.double() - m64).abs().max()):.2e}")
    del S64
    # 4. wall time per evaluation inside fit
    rw = ShiftReweighter(S, y, 0.5, device=dev)
    rw.fit(4.0, tol=1e-12, max_evals=5)
    per = []
    for _ in range(max(reps, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = rw.fit(4.0, tol=1e-12, max_evals=evals)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6 / (r.evaluations + 1))      # + 1: the weights pass reads S once more
    out(f"    4. wall per evaluation inside fit ({r.evaluations} evaluations + the weights pass, host clock to a synchronise): "
        f"{statistics.median(per):.1f} ({min(per):.1f}, {max(per):.1f}) us, {nbytes / statistics.median(per) / 1e6:.2f} TB/s")


def main():
    path = next((a for a in sys.argv[1:] if a.endswith(".txt")), None)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"device: {torch.cuda.get_device_name(dev)}")
    T = arg("--frames", 100000)
    for M in (1024, 4096):
        one_shape(T, M, arg("--launches", 20), arg("--reps", 5), arg("--evals", 40), out)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
