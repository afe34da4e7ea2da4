"""What the ensemble-averaged loss costs a training step.

512 groups of 8 frames x 32 atoms — 4,096 graphs, 131,072 atoms, K = 16, C = 10, atom_feature_size 64, the architecture of
bench.py.  One engine and one Trainer per variant, all from the same weights, on the same batch:
  grouped          Trainer(loss_balance=S).step(groups=)      forward, ng_group_mean, ng_loss_name on the means, ng_group_spread,
                                                              backward, Adam
  plain, unfused   Trainer(loss_balance=S).step()             forward, ng_loss_name on the 4,096 records, backward, Adam: the
                                                              route a step took before groups existed, with the loss outside
                                                              the head launch as in the grouped step
  grouped s=1      Trainer(loss_balance=1).step(groups=)      ng_loss_l2 on the means
  plain s=1        Trainer(loss_balance=1).step()             the fused head + loss + head-backward launch, for scale
with S = 0.999 (``--balance``).  Timing: device events around ``--steps`` (20) steps that end in a synchronise, ``--warmup``
(10) steps of every variant first, then ``--reps`` (7) rounds in which the variants ALTERNATE; median, min and max of the
per-step time of a round.  The spread of a row over the rounds is the noise to read the differences against.  Then the
library's own event pairs around every entry point (``ng_prof_enable``) over ``--steps`` grouped steps give the time of
the launches of ng_group_mean, ng_group_spread and the loss between them.
usage: python tools/ensemble_bench.py [--steps S] [--warmup W] [--reps R] [--groups Q] [--frames R] [--atoms n] [out.txt]"""
import os
import statistics
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrgnn_amd import synth  # noqa: E402
from nmrgnn_amd.engine import Engine  # noqa: E402
from nmrgnn_amd.graph import GraphBatch  # noqa: E402
from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space  # noqa: E402
from nmrgnn_amd.train import Trainer  # noqa: E402

warnings.simplefilter("ignore")
K, NC = 16, 10
ARCH = dict(atom_feature_size=64, edge_feature_size=3, edge_hidden_size=128, mp_layers=4, fc_layers=4, edge_fc_layers=4)


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed_ms(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    path = next((a for a in sys.argv[1:] if a.endswith(".txt")), None)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    Q, R, n = arg("--groups", 512), arg("--frames", 8), arg("--atoms", 32)
    steps, warmup, reps, S = arg("--steps", 20), arg("--warmup", 10), arg("--reps", 7), arg("--balance", 0.999, float)
    dev = torch.device("cuda", 0)
    hp = declare_gnn_space(HyperParameters(**ARCH))
    b = synth.make_batch(Q * R, n, K, NC, 0.05, seed=42)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    y, w = torch.from_numpy(b["y"]).to(dev), torch.from_numpy(b["w"]).to(dev)
    groups = np.arange(0, Q * R + 1, R, dtype=np.int32)
    runs = []
    for name, balance, grouped in (("grouped", S, True), ("plain, unfused", S, False), ("grouped s=1", 1.0, True),
                                   ("plain s=1", 1.0, False)):
        tr = Trainer(Engine(hp, NC, device=dev, seed=1234), lr=1e-4, loss_balance=balance)
        runs.append((name, tr, (lambda tr=tr: tr.step(gb, y, w, groups=groups)) if grouped else (lambda tr=tr: tr.step(gb, y, w)), []))
    for _, _, step, _ in runs:
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    for _ in range(reps):
        for _, _, step, ms in runs:
            ms.append(timed_ms(step, steps))
    out(f"ensemble step time on {torch.cuda.get_device_name(0)}: {Q} groups x {R} frames x {n} atoms = {Q * R} graphs, "
        f"{Q * R * n} atoms; s = {S}; {reps} alternating rounds of {steps} steps, ms per step")
    out(f"  {'variant':<16} {'median':>8} {'min':>8} {'max':>8}")
    for name, _, _, ms in runs:
        out(f"  {name:<16} {statistics.median(ms):>8.3f} {min(ms):>8.3f} {max(ms):>8.3f}")
    med = {name: statistics.median(ms) for name, _, _, ms in runs}
    out(f"  grouped - plain, unfused: {1e3 * (med['grouped'] - med['plain, unfused']):+.1f} us per step")
    # the entry points' own times (event pairs inside the library; they serialise the host against nothing but add a record
    # per call, so the step time above is taken without them)
    _, tr, step, _ = runs[0]
    ctx = tr.engine.ctx
    ctx.prof_reset()
    ctx.prof_enable(True)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    prof = ctx.prof_read()
    ctx.prof_enable(False)
    out(f"  per call over {steps} grouped steps, us: " + ", ".join(
        f"{k} {1e3 * prof[k][0] / max(prof[k][1], 1):.1f}" for k in ("group_mean", "loss_name", "group_spread") if k in prof))
    for _, tr, _, _ in runs:
        tr.close()
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
