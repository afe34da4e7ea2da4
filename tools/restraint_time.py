"""Cost of the replica-averaged shift restraint (library.ShiftRestraint), timed with CUDA events, median of 20 calls, ms per
call:
  eager shift_restraint (one 7lgi frame) against ShiftRestraint replayed and eager, R = 1 and R = 8 7lgi frames, with no box,
  an orthorhombic box and the reduced triclinic box of DESIGN 7.3 (the rhombic dodecahedron), positions and box staged per
  call (the host-to-device copy of the inputs is inside the timed region, as an MD engine would pay it);
  Engine.backward(edge_grad=) with param_grad True against False on the bench batch (512 graphs x 256 atoms, K = 16), per-edge
  and table edge paths (the forward with a tape is untimed);
  the restraint forms, replayed, one 7lgi frame and R = 8, no box: harmonic, flat-bottom, weighted replicas
  (new weights staged every call), independent replicas, time-averaged;
  the Jacobian table of DESIGN 7.11: Engine.backward(edge_grad=, param_grad=False) on the bench batch's table path with
  edge_grad_table off and on.
usage: python tools/restraint_time.py [--forms | --table] [out.json]     (--forms / --table: only those rows)"""
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrgnn_amd import synth  # noqa: E402
from nmrgnn_amd.engine import Engine  # noqa: E402
from nmrgnn_amd.graph import GraphBatch  # noqa: E402
from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space  # noqa: E402
from nmrgnn_amd.library import ShiftRestraint, shift_restraint  # noqa: E402
from nmrgnn_amd.model import GNNModel  # noqa: E402
from nmrgnn_amd.pbc import triclinic_vectors, widths  # noqa: E402
from nmrgnn_amd.standards import load_standards  # noqa: E402
from nmrgnn_amd.structure import atoms_onehot, read_pdb  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)


def median_ms(fn, reps=20):
    fn(); fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def restraint_rows():
    s = read_pdb("tests/data/7lgi.pdb.gz")
    atoms = atoms_onehot(s.elements)
    p = np.asarray(s.frames[0], np.float32)
    n = p.shape[0]
    rng = np.random.default_rng(1)
    y = (rng.standard_normal(n) * 3.0).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    hp = declare_gnn_space(HyperParameters(atom_feature_size=64))
    model = GNNModel(hp, load_standards(), device=dev, seed=3)
    model.build(atoms.shape[1])
    e = p.max(0) - p.min(0) + 13.0
    d = np.array([1.0, 1.0, 1.0, 60.0, 60.0, 90.0])
    d[:3] *= float(e.max()) / widths(triclinic_vectors(d)).min()
    out = {}
    for name, box in [("none", None), ("ortho", np.array([e[0], e[1], e[2], 90.0, 90.0, 90.0])), ("triclinic", d)]:
        row = {"eager_shift_restraint_ms": median_ms(lambda: shift_restraint(model, atoms, p, y, w, box=box))}
        for R in (1, 8):
            frames = np.stack([p + 0.05 * rng.standard_normal(p.shape).astype(np.float32) for _ in range(R)])
            pos = frames[0] if R == 1 else frames
            for replay in (True, False):
                r = ShiftRestraint(model, atoms, y, w, replicas=R, box=box, replay=replay)
                key = f"R{R}_{'replay' if replay else 'eager'}_ms"
                row[key] = median_ms(lambda: r(pos, box=box))
                del r
        out[name] = row
        print(name, {k: round(v, 4) for k, v in row.items()}, flush=True)
    return out


def backward_rows():
    hp = declare_gnn_space(HyperParameters(atom_feature_size=64, edge_feature_size=3, edge_hidden_size=128, mp_layers=4,
                                           fc_layers=4, edge_fc_layers=4))
    eng = Engine(hp, 10, device=dev, seed=1234)
    b = synth.make_batch(512, 256, 16, 10, 0.05, seed=42)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    dpeaks = torch.from_numpy(np.random.default_rng(2).standard_normal(gb.N).astype(np.float32)).to(dev)
    dedges = torch.empty(gb.edges.shape, dtype=torch.float32, device=dev)
    out = {}
    for label, table in (("per_edge", False), ("table", True)):
        eng.edge_table = table
        row = {}
        for pg in (True, False):
            ts = []
            for _ in range(22):
                eng.forward(gb, training=False, keep_tape=True)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.backward(dpeaks, edge_grad=dedges, param_grad=pg)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            row[f"param_grad_{pg}_ms"] = float(np.median(ts[2:]))
        out[label] = row
        print("backward", label, {k: round(v, 4) for k, v in row.items()}, flush=True)
    return out


def forms_rows():
    s = read_pdb("tests/data/7lgi.pdb.gz")
    atoms = atoms_onehot(s.elements)
    p = np.asarray(s.frames[0], np.float32)
    n = p.shape[0]
    rng = np.random.default_rng(3)
    y = (rng.standard_normal(n) * 3.0).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    hp = declare_gnn_space(HyperParameters(atom_feature_size=64))
    model = GNNModel(hp, load_standards(), device=dev, seed=3)
    model.build(atoms.shape[1])
    out = {}
    for R in (1, 8):
        frames = np.stack([p + 0.05 * rng.standard_normal(p.shape).astype(np.float32) for _ in range(R)])
        pos = frames[0] if R == 1 else frames
        forms = [("harmonic", {}), ("flat", dict(tolerance=0.3)), ("averaged", dict(tau=10.0))]
        if R > 1:
            forms[2:2] = [("weighted", dict(replica_weights=np.ones(R))), ("independent", dict(independent=True))]
        row = {}
        for name, kw in forms:
            r = ShiftRestraint(model, atoms, y, w, replicas=R, **kw)
            if name == "weighted":
                cs = [rng.random(R) + 0.1 for _ in range(2)]
                k = [0]

                def call():
                    k[0] ^= 1
                    r(pos, replica_weights=cs[k[0]])
                row[f"{name}_ms"] = median_ms(call)
            else:
                row[f"{name}_ms"] = median_ms(lambda: r(pos))
            del r
        out[f"R{R}"] = row
        print("forms", R, {k: round(v, 4) for k, v in row.items()}, flush=True)
    return out


def table_rows():
    out = {}
    eng = Engine(declare_gnn_space(HyperParameters(atom_feature_size=64)), 10, device=dev, seed=1234)
    b = synth.make_batch(512, 256, 16, 10, 0.05, seed=42)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    dpeaks = torch.from_numpy(np.random.default_rng(2).standard_normal(gb.N).astype(np.float32)).to(dev)
    dedges = torch.empty(gb.edges.shape, dtype=torch.float32, device=dev)
    row = {}
    for on in (False, True):
        eng.edge_grad_table = on
        ts = []
        for _ in range(22):
            eng.forward(gb, training=False, keep_tape=True)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.backward(dpeaks, edge_grad=dedges, param_grad=False)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        row[f"edge_grad_table_{on}_ms"] = float(np.median(ts[2:]))
    row["j_guard"] = list(eng.edge_grad_table_report())
    out["backward_bench_batch_table_path"] = row
    print("table backward", row, flush=True)
    return out


def main():
    flags = ("--forms", "--table")
    args = [a for a in sys.argv[1:] if a not in flags]
    if "--forms" in sys.argv[1:]:
        res = {"restraint_forms_7lgi": forms_rows()}
    elif "--table" in sys.argv[1:]:
        res = {"jacobian_table": table_rows()}
    else:
        res = {"restraint_7lgi": restraint_rows(), "backward_bench_batch": backward_rows(),
               "restraint_forms_7lgi": forms_rows(), "jacobian_table": table_rows()}
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
