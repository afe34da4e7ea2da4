"""Cost of the shift uncertainties, timed with CUDA events, median of 20 calls, ms per call:
  GNNModel.predict_uncertainty on one 7lgi frame (2,770 atoms), S = 32 replicas in one batch, against S calls of
  model(batch, training=True) — what a user could do before: one draw of noise AND dropout per call, and the dropout part
  still to be estimated from the draws;
  ng_head_fwd_var against ng_head_fwd alone at N = 131,072, Fh = 32 (C = 10), in windows of 200 launches: the variance
  costs the head no second pass over g.
usage: python tools/uncertainty_time.py [out.json]"""
import ctypes as C
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrgnn_amd import _lib  # noqa: E402
from nmrgnn_amd._lib import ptr  # noqa: E402
from nmrgnn_amd.graph import frames_to_batch  # noqa: E402
from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space  # noqa: E402
from nmrgnn_amd.model import GNNModel  # noqa: E402
from nmrgnn_amd.standards import load_standards  # noqa: E402
from nmrgnn_amd.structure import atoms_onehot, read_pdb  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)


def median_ms(fn, reps=20, inner=1):
    """median over ``reps`` timed windows of ``inner`` back-to-back calls each, per call"""
    fn(); fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts))


def ensemble_rows(S=32):
    s = read_pdb(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "data", "7lgi.pdb.gz"))
    atoms = atoms_onehot(s.elements)
    out = {}
    for F in (64, 256):
        model = GNNModel(declare_gnn_space(HyperParameters(atom_feature_size=F)), load_standards(), device=dev, seed=3)
        model.build(atoms.shape[1])
        batch = frames_to_batch(atoms, np.asarray(s.frames[0], np.float32), 16, device=dev)

        def sampled():
            for k in range(S):
                model(batch, training=True, seed=k)
        row = {"predict_uncertainty_ms": median_ms(lambda: model.predict_uncertainty(batch, samples=S, seed=1)),
               f"{S}_training_calls_ms": median_ms(sampled), "atoms": batch.N, "samples": S}
        out[f"F{F}"] = row
        print("7lgi", f"F{F}", {k: round(v, 4) for k, v in row.items()}, flush=True)
    return out


def head_rows(N=131072, Fh=32, Cn=10):
    ctx = _lib.get_context(0)
    lib, h = ctx.lib, ctx.handle
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(5)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    g = up(rng.standard_normal((N, Fh)))
    W, b = up(rng.standard_normal((Fh, Cn)) / np.sqrt(Fh)), up(0.1 * rng.standard_normal(Cn))
    atoms = up(np.eye(Cn)[rng.integers(0, Cn, N)])
    std, avg = up(rng.uniform(0.5, 40.0, Cn)), up(rng.uniform(-3.0, 120.0, Cn))
    pk, var = torch.empty(N, device=dev), torch.empty(N, device=dev)
    # a launch of 8 us is shorter than an event pair resolves: windows of 200 back-to-back launches (g then stays in the
    # caches between launches, for both entry points alike)
    plain = lambda: ctx.check(lib.ng_head_fwd(h, st, N, Fh, Cn, ptr(g), None, ptr(W), ptr(b), ptr(atoms), ptr(std), ptr(avg),
                                              ptr(pk)), "ng_head_fwd")
    withvar = lambda: ctx.check(lib.ng_head_fwd_var(h, st, N, Fh, Cn, ptr(g), 0.8, ptr(W), ptr(b), ptr(atoms), ptr(std), ptr(avg),
                                                    ptr(pk), ptr(var)), "ng_head_fwd_var")
    row = {"ng_head_fwd_ms": median_ms(plain, inner=200), "ng_head_fwd_var_ms": median_ms(withvar, inner=200),
           "ng_head_fwd_again_ms": median_ms(plain, inner=200), "g_megabytes": N * Fh * 4 / 1e6}
    print("head", {k: round(v, 4) for k, v in row.items()}, flush=True)
    return row


def main():
    res = {"ensemble_7lgi": ensemble_rows(), "head_N131072_Fh32": head_rows()}
    if sys.argv[1:]:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
