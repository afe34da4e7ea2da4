"""Time of the input gradients, in ms per call, on one 7lgi frame and on the bench batch:
forward; forward + backward; forward + backward + edge_grad (ng_edge_mlp_dinput); the same plus positions (ng_positions_grad).
The 7lgi frame is a kNN graph built on the GPU from positions (one frame, inference-mode forward with a tape: what
library.shift_restraint runs); the bench batch is bench.py's (512 graphs x 256 atoms, K = 16, training-mode forward).
The bench batch has no positions: its last column is the edge_grad time again plus nothing.  CUDA-event timing, median."""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nmrgnn_amd import synth  # noqa: E402
from nmrgnn_amd.engine import Engine  # noqa: E402
from nmrgnn_amd.graph import GraphBatch, frames_to_batch  # noqa: E402
from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space  # noqa: E402
from nmrgnn_amd.structure import atoms_onehot, read_pdb  # noqa: E402

dev = torch.device("cuda", 0)


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def legs(eng, gb, training, positions):
    dp = torch.ones(gb.N, device=dev)
    eg = torch.empty(gb.edges.shape, device=dev)

    def fwd():
        eng.forward(gb, training=training, keep_tape=True)
        eng.tape = None

    def fwd_bwd(edge_grad=None, pos=False):
        eng.forward(gb, training=training, keep_tape=True)
        eng.backward(dp, edge_grad=edge_grad)
        if pos:
            gb.positions_grad(eg)

    out = {"forward": timed(fwd), "forward+backward": timed(fwd_bwd),
           "forward+backward+edge_grad": timed(lambda: fwd_bwd(eg))}
    if positions:
        out["forward+backward+edge_grad+positions"] = timed(lambda: fwd_bwd(eg, True))
    return {k: round(v, 4) for k, v in out.items()}


def main():
    hp = declare_gnn_space(HyperParameters())
    s = read_pdb(os.path.join(R, "tests", "data", "7lgi.pdb.gz"))
    atoms = atoms_onehot(s.elements)
    eng = Engine(hp, atoms.shape[1], device=dev, seed=1)
    gb = frames_to_batch(atoms, torch.from_numpy(s.frames[0]).to(dev), 16, device=dev)
    print("7lgi frame (%d atoms, %d edges):" % (gb.N, gb.n_edges), legs(eng, gb, False, True))
    b = synth.make_batch(512, 256, 16, 10, 0.05, seed=42)
    eng2 = Engine(declare_gnn_space(HyperParameters(atom_feature_size=64)), 10, device=dev, seed=1234)
    gb2 = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    print("bench batch (%d atoms, %d edges):" % (gb2.N, gb2.n_edges), legs(eng2, gb2, True, False))
    eng2.edge_table = False
    print("bench batch, per-edge path:", legs(eng2, gb2, True, False))


if __name__ == "__main__":
    main()
