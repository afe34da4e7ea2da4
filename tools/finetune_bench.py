"""What a truncated backward and the grouped Adam buy a fine-tuning step.

The bench shape — 512 graphs x 256 atoms, K = 16, C = 10, the architecture of bench.py — at atom_feature_size 64 and 256,
edge MLP per edge as bench.py's `value` (``--edge-table``: the Engine's default, the guarded table).  One engine and one
Trainer per trainable set, all from the same weights:
  full            Trainer(engine)                       the plain step: ng_adam_step, every launch of the backward
  fc+out          trainable = fc, out                   the backward ends behind the FC block
  mpL-1+fc+out    trainable = mp/L-1, fc, out           ... behind the top MP layer
  edge_fc frozen  trainable = everything but edge_fc    the full walk without the edge-MLP backward
Timing: device events around ``--steps`` (20) steps that end in a synchronise, ``--warmup`` (10) steps of every set first,
then ``--reps`` (7) rounds in which the sets ALTERNATE; median, min and max of the per-step time of a round, and the ratio
of the medians to the full step of the same run.  The spread of the full step over the rounds is the noise to read the
other rows against.
usage: python tools/finetune_bench.py [--steps S] [--warmup W] [--reps R] [--graphs G] [--edge-table] [out.txt]"""
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrgnn_amd import synth  # noqa: E402
from nmrgnn_amd.engine import Engine  # noqa: E402
from nmrgnn_amd.graph import GraphBatch  # noqa: E402
from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space  # noqa: E402
from nmrgnn_amd.train import Trainer  # noqa: E402

warnings.simplefilter("ignore")
ATOMS, K, NC = 256, 16, 10
ARCH = dict(edge_feature_size=3, edge_hidden_size=128, mp_layers=4, fc_layers=4, edge_fc_layers=4)


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def sets(L):
    return [("full", None), ("fc+out", ["fc", "out"]), (f"mp{L - 1}+fc+out", [f"mp/{L - 1}", "fc", "out"]),
            ("edge_fc frozen", ["out", "fc", "embed"] + [f"mp/{l}" for l in range(L)])]


def timed_ms(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def leg(F, graphs, steps, warmup, reps, edge_table, out):
    dev = torch.device("cuda", 0)
    hp = declare_gnn_space(HyperParameters(atom_feature_size=F, **ARCH))
    b = synth.make_batch(graphs, ATOMS, K, NC, 0.05, seed=42)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    y, w = torch.from_numpy(b["y"]).to(dev), torch.from_numpy(b["w"]).to(dev)
    runs = []
    for name, trainable in sets(hp.get("mp_layers")):
        eng = Engine(hp, NC, device=dev, seed=1234)
        eng.edge_table = bool(edge_table)
        tr = Trainer(eng, lr=1e-4) if trainable is None else Trainer(eng, lr=1e-4, trainable=trainable)
        runs.append((name, tr, lambda tr=tr: tr.step(gb, y, w), []))
    for _, _, step, _ in runs:
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    for _ in range(reps):
        for _, _, step, ms in runs:
            ms.append(timed_ms(step, steps))
    base = statistics.median(runs[0][3])
    out(f"F = {F}: {graphs} graphs x {ATOMS} atoms, edge MLP {'through the table' if edge_table else 'per edge'}; {reps} alternating "
        f"rounds of {steps} steps, ms per step")
    out(f"  {'trainable':<16} {'parameters':>10} {'median':>8} {'min':>8} {'max':>8} {'/ full':>7}")
    for name, tr, _, ms in runs:
        med = statistics.median(ms)
        out(f"  {name:<16} {tr.trainable_count():>10} {med:>8.3f} {min(ms):>8.3f} {max(ms):>8.3f} {med / base:>7.3f}")
        tr.close()


def main():
    path = next((a for a in sys.argv[1:] if a.endswith(".txt")), None)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"fine-tuning step time on {torch.cuda.get_device_name(0)}")
    for F in (64, 256):
        leg(F, arg("--graphs", 512), arg("--steps", 20), arg("--warmup", 10), arg("--reps", 7), "--edge-table" in sys.argv, out)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
