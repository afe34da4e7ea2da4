"""Cost of the box gradient (csrc/box_grad.hip: ng_box_grad / ng_box_grad_csr) with no box, an orthorhombic box and a
reduced triclinic box, hipEvent-timed, median of 20 calls, ms per call.
  sizes: one 7lgi frame (2,770 atoms); 100 7lgi frames in one call; 7lgi tiled to a 443 k-atom frame; the 4096-molecule
  ragged batch of DESIGN 7.4 (8-120 atoms each, open boundaries only)
  lists: kNN K = 16 (padded, ng_box_grad) and a 4 A cutoff (CSR, ng_box_grad_csr); dd random, built once, untimed
  and shift_restraint on one 7lgi frame with and without virial=True (open and orthorhombic), ms per call.
usage: python tools/box_grad_time.py [out.json]"""
import ctypes as C
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nmrgnn_amd  # noqa: E402
from nmrgnn_amd import _lib  # noqa: E402
from nmrgnn_amd._lib import ptr  # noqa: E402
from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff, structures_to_batch  # noqa: E402
from nmrgnn_amd.library import shift_restraint  # noqa: E402
from nmrgnn_amd.structure import atoms_onehot, read_pdb  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)
ctx = _lib.get_context(0)
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
s = read_pdb("tests/data/7lgi.pdb.gz")
atoms = atoms_onehot(s.elements)
prot = np.asarray(s.frames[0], np.float32)
ext = prot.max(0) - prot.min(0) + 12.0


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


def boxes(e):
    """(label, dims or None) for no box, an orthorhombic box of extent e, a reduced triclinic box of the same volume"""
    v = np.array([[e[0], 0, 0], [0.25 * e[0], e[1], 0], [-0.2 * e[0], 0.3 * e[1], e[2]]])
    L = np.linalg.norm(v, axis=1)
    ang = lambda x, y: np.degrees(np.arccos(np.dot(x, y) / np.linalg.norm(x) / np.linalg.norm(y)))
    tric = [L[0], L[1], L[2], ang(v[1], v[2]), ang(v[0], v[2]), ang(v[0], v[1])]
    return [("none", None), ("ortho", [e[0], e[1], e[2], 90.0, 90.0, 90.0]), ("triclinic", tric)]


def call(b, dd, strain, dvec):
    """the library call alone on the batch's device arrays"""
    tric = int(b.box_triclinic) if b.box is not None else -1
    if b.is_csr:
        return lambda: ctx.check(ctx.lib.ng_box_grad_csr(ctx.handle, st, b.N, b.edges.numel(), ptr(b.positions), ptr(b.row_ptr),
                                                         ptr(b.nlist), ptr(dd), b.scale, b.G, ptr(b.graph_ptr), ptr(b.box), tric,
                                                         ptr(strain), ptr(dvec)), "box_grad_csr")
    return lambda: ctx.check(ctx.lib.ng_box_grad(ctx.handle, st, b.N, b.K, ptr(b.positions), ptr(b.nlist), ptr(b.edges),
                                                 ptr(dd), b.scale, b.G, ptr(b.graph_ptr), ptr(b.box), tric, ptr(strain),
                                                 ptr(dvec)), "box_grad")


def timed(b, label, name):
    rng = np.random.default_rng(3)
    dd = torch.from_numpy(rng.standard_normal(tuple(b.edges.shape)).astype(np.float32)).to(dev)
    strain = torch.empty(b.G, 9, dtype=torch.float64, device=dev)
    dvec = torch.empty(b.G, 9, dtype=torch.float64, device=dev)
    ms = median_ms(call(b, dd, strain, dvec))
    print(f"{label:>26s} {name:>9s} {'csr' if b.is_csr else 'knn':>4s}: {ms:.4f} ms  ({b.N} rows, {b.edges.numel()} slots)",
          flush=True)
    return ms


def sizes(frames, e, label, cutoff=True):
    at = np.tile(atoms, (frames.shape[1] // atoms.shape[0], 1))
    out = {}
    for name, dims in boxes(e):
        r = {"knn_ms": timed(frames_to_batch(at, frames, 16, device=dev, box=dims), label, name)}
        if cutoff:
            r["cutoff_ms"] = timed(frames_to_batch_cutoff(at, frames, 4.0, device=dev, box=dims), label, name)
        out[name] = r
    return out


rng = np.random.default_rng(7)
res = {}
one = (prot - prot.min(0) + 6.0)[None]
res["7lgi_1frame"] = sizes(one, ext, "7lgi, 1 frame")
hundred = np.stack([one[0] + rng.normal(0, 0.3, prot.shape).astype(np.float32) for _ in range(100)])
res["7lgi_100frames"] = sizes(hundred, ext, "7lgi, 100 frames")
side = 16                                                           # 160 copies: 10 x 16 tiles
tiles = [one[0] + np.array([(c % side) * ext[0], (c // side) * ext[1], 0.0], np.float32) for c in range(160)]
big = np.concatenate(tiles)[None]
res["443k_frame"] = sizes(big, np.array([side * ext[0], 10 * ext[1], ext[2]]), f"{big.shape[1]} atoms, 1 frame", cutoff=False)

# the 4096 molecules of tools/ragged_time.py (a): 8-120 atoms at 0.1 atoms / A^3, H/C/N/O
mrng = np.random.default_rng(1)
m_atoms, m_pos = [], []
for n in mrng.integers(8, 121, 4096):
    m_atoms.append(atoms_onehot(mrng.choice(["H", "C", "N", "O"], n, p=[0.5, 0.3, 0.1, 0.1])))
    m_pos.append(mrng.uniform(0, (n / 0.1) ** (1.0 / 3.0), (n, 3)).astype(np.float32))
res["ragged_4096"] = {"none": {"knn_ms": timed(structures_to_batch(m_atoms, m_pos, device=dev), "4096 molecules", "none"),
                               "cutoff_ms": timed(structures_to_batch(m_atoms, m_pos, cutoff=4.0, device=dev), "4096 molecules",
                                                  "none")}}

# shift_restraint on one frame, with and without the virial
model = nmrgnn_amd.load_model()
model.build(atoms.shape[1])
targets = rng.normal(0, 2.0, prot.shape[0]).astype(np.float32)
res["shift_restraint_ms"] = {}
for name, dims in boxes(ext)[:2]:
    r = {"plain": [], "virial": []}
    for _ in range(3):                     # interleaved passes, median of 50 each: the call is host-bound and noisy
        for vir in (False, True):
            r["virial" if vir else "plain"].append(
                median_ms(lambda: shift_restraint(model, atoms, one[0], targets, box=dims, virial=vir), reps=50))
    res["shift_restraint_ms"][name] = r
    print(f"{'shift_restraint, 1 frame':>26s} {name:>9s}: plain " + " ".join(f"{x:.4f}" for x in r["plain"])
          + " ms, virial=True " + " ".join(f"{x:.4f}" for x in r["virial"]) + " ms", flush=True)

if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1)
