"""What receptive-field pruning saves a restraint on a solvated system.

A synthetic system: ``--atoms`` (100 000) random points at liquid density (0.1 atoms / A^3) in a cubic periodic box; the
restrained atoms are those inside a centred sphere that holds about 1 %, 5 % and 20 % of them (a solute in solvent); kNN
lists with K = 16; atom_feature_size 64 and 256.  Timed: ``library.shift_restraint`` with and without ``prune``, whole
calls — list building, the pruned call's one host synchronisation, forward, backward, positions kernel — host clock around
a call that ends in a device synchronise, two warm-up calls, then the two variants ALTERNATING in one process, median of
``--reps``.  Also printed: kept atoms M / N, kept live edges / all live edges, and the time of the list building alone
(paid by both variants).  With ``--prof`` one more call of each variant runs with the library's per-launch timers on and
their totals are listed.
usage: python tools/prune_bench.py [--atoms N] [--reps R] [--prof] [out.json]"""
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrgnn_amd.graph import frames_to_batch  # noqa: E402
from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space  # noqa: E402
from nmrgnn_amd.library import shift_restraint  # noqa: E402
from nmrgnn_amd.model import GNNModel  # noqa: E402
from nmrgnn_amd.standards import load_standards  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def launches(model, fn):
    ctx = model.engine.ctx
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    torch.cuda.synchronize()
    rows = sorted(ctx.prof_read().items(), key=lambda kv: -kv[1][0])
    ctx.prof_enable(False)
    return {k: [round(v[0], 4), int(v[1])] for k, v in rows}


def main():
    args = sys.argv[1:]
    n = int(args[args.index("--atoms") + 1]) if "--atoms" in args else 100_000
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 9
    prof = "--prof" in args
    out_path = next((a for a in args if a.endswith(".json")), None)
    rng = np.random.default_rng(7)
    L = float((n / 0.1) ** (1.0 / 3.0))
    pos_h = rng.uniform(0.0, L, (n, 3)).astype(np.float32)
    elem = rng.choice([2, 3, 4, 5], size=n, p=[0.1, 0.05, 0.6, 0.25])
    atoms_h = np.zeros((n, 10), np.float32)
    atoms_h[np.arange(n), elem] = 1.0
    box = (L, L, L, 90.0, 90.0, 90.0)
    pos, atoms = torch.from_numpy(pos_h).to(dev), torch.from_numpy(atoms_h).to(dev)
    y = torch.from_numpy((rng.standard_normal(n) * 3.0).astype(np.float32)).to(dev)
    order = np.argsort(((pos_h - 0.5 * L) ** 2).sum(1))
    res = {"atoms": n, "box_A": L, "K": 16, "reps": reps, "rows": []}
    for F in (64, 256):
        model = GNNModel(declare_gnn_space(HyperParameters(atom_feature_size=F)), load_standards(), device=dev, seed=3)
        model.build(10)
        build_ms = float(np.median([wall_ms(lambda: frames_to_batch(atoms, pos, device=dev, box=box)) for _ in range(5)][2:]))
        for frac in (0.01, 0.05, 0.20):
            w_h = np.zeros(n, np.float32)
            w_h[order[:int(round(frac * n))]] = 1.0
            w = torch.from_numpy(w_h).to(dev)
            batch = frames_to_batch(atoms, pos, device=dev, box=box)
            pr = batch.restrict(w != 0, model.receptive_hops)
            row = {"F": F, "selected": frac, "M_over_N": pr.N / batch.N,
                   "live_edges_kept": int((pr.edges > 0).sum()) / int((batch.edges > 0).sum()), "list_building_ms": build_ms}
            del batch, pr
            calls = {k: (lambda p=p: shift_restraint(model, atoms, pos, y, w, box=box, prune=p)) for k, p in
                     (("whole", False), ("pruned", True))}
            e0, f0 = calls["whole"]()
            e1, f1 = calls["pruned"]()
            row["forces_max_rel_diff"] = float((f0 - f1).abs().max() / f0.abs().max())
            row["energy_rel_diff"] = abs(float(e0) - float(e1)) / abs(float(e0))
            for c in calls.values():
                c()
            ts = {k: [] for k in calls}
            for _ in range(reps):
                for k, c in calls.items():
                    ts[k].append(wall_ms(c))
            for k in calls:
                row[f"{k}_ms"] = float(np.median(ts[k]))
                row[f"{k}_ms_min_max"] = [float(np.min(ts[k])), float(np.max(ts[k]))]
            row["speedup"] = row["whole_ms"] / row["pruned_ms"]
            if prof:
                row["launches_ms_count"] = {k: launches(model, c) for k, c in calls.items()}
            res["rows"].append(row)
            print({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in row.items() if k != "launches_ms_count"}, flush=True)
            if prof:
                for k, v in row["launches_ms_count"].items():
                    print(" ", k, v, flush=True)
        del model
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
