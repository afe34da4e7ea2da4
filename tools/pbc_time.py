"""Cost of periodic boxes (csrc/pbc.cuh): every list builder with no box, an orthorhombic box and a reduced triclinic box,
hipEvent-timed, median of 20 calls, ms per call.
  sizes: one 7lgi frame (2,770 atoms); 100 7lgi frames in one call; 7lgi tiled to a 443 k-atom frame (cell grid)
  builders: ng_knn_graph(_pbc) K = 16; ng_cutoff_count(_pbc) + ng_cutoff_fill_rows(_pbc) at 4 A (scan and nnz read excluded)
  and the eval-struct frame end to end (frames_to_batch + model, 32 frames per batch as eval-struct), ms per frame.
usage: python tools/pbc_time.py [out.json]"""
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
from nmrgnn_amd.graph import frames_to_batch  # noqa: E402
from nmrgnn_amd.pbc import prepare  # noqa: E402
from nmrgnn_amd.structure import atoms_onehot, read_pdb  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)
ctx = _lib.get_context(0)
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
s = read_pdb("tests/data/7lgi.pdb.gz")
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


def builders(frames, e, label, cutoff=True):
    G, n, _ = frames.shape
    tp = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    nl = torch.empty((G * n, 16), dtype=torch.int32, device=dev)
    ed = torch.empty((G * n, 16), device=dev)
    inv = torch.empty((G * n,), device=dev)
    deg = torch.empty((G * n,), dtype=torch.int32, device=dev)
    row_ptr = torch.empty((G * n + 1,), dtype=torch.int32, device=dev)
    out = {}
    for name, dims in boxes(e):
        if dims is None:
            knn = lambda: ctx.check(ctx.lib.ng_knn_graph(ctx.handle, st, G, n, 16, 0.1, ptr(tp), ptr(nl), ptr(ed), ptr(inv)), "knn")
            count = lambda: ctx.check(ctx.lib.ng_cutoff_count(ctx.handle, st, G, n, 4.0, ptr(tp), ptr(deg)), "count")
        else:
            vec, tric, _ = prepare(dims, G)
            bx = torch.from_numpy(vec).to(dev)
            knn = lambda bx=bx, tric=tric: ctx.check(ctx.lib.ng_knn_graph_pbc(ctx.handle, st, G, n, 16, 0.1, ptr(tp), ptr(bx), int(tric),
                                                                               ptr(nl), ptr(ed), ptr(inv)), "knn_pbc")
            count = lambda bx=bx, tric=tric: ctx.check(ctx.lib.ng_cutoff_count_pbc(ctx.handle, st, G, n, 4.0, ptr(tp), ptr(bx), int(tric),
                                                                                   ptr(deg)), "count_pbc")
        r = {"knn_ms": median_ms(knn)}
        if cutoff:
            count()
            ctx.check(ctx.lib.ng_exclusive_scan_i32(ctx.handle, st, G * n, ptr(deg), ptr(row_ptr)), "scan")
            nnz = int(row_ptr[-1])
            col = torch.empty(nnz, dtype=torch.int32, device=dev)
            dist = torch.empty(nnz, device=dev)
            row_of = torch.empty(nnz, dtype=torch.int32, device=dev)
            if dims is None:
                fill = lambda: ctx.check(ctx.lib.ng_cutoff_fill_rows(ctx.handle, st, G, n, 4.0, 0.1, ptr(tp), ptr(row_ptr), ptr(col),
                                                                     ptr(dist), ptr(inv), ptr(row_of)), "fill")
            else:
                fill = lambda bx=bx, tric=tric: ctx.check(ctx.lib.ng_cutoff_fill_rows_pbc(
                    ctx.handle, st, G, n, 4.0, 0.1, ptr(tp), ptr(bx), int(tric), ptr(row_ptr), ptr(col), ptr(dist), ptr(inv),
                    ptr(row_of)), "fill_pbc")
            r["cutoff_count_ms"] = median_ms(count)
            r["cutoff_fill_ms"] = median_ms(fill)
        out[name] = r
        print(f"{label:>22s} {name:>9s}: " + "  ".join(f"{k} {v:.4f}" for k, v in r.items()), flush=True)
    return out


rng = np.random.default_rng(7)
res = {}
one = (prot - prot.min(0) + 6.0)[None]
res["7lgi_1frame"] = builders(one, ext, "7lgi, 1 frame")
hundred = np.stack([one[0] + rng.normal(0, 0.3, prot.shape).astype(np.float32) for _ in range(100)])
res["7lgi_100frames"] = builders(hundred, ext, "7lgi, 100 frames")
side = 16                                                           # 160 copies: 10 x 16 tiles
tiles = [one[0] + np.array([(c % side) * ext[0], (c // side) * ext[1], 0.0], np.float32) for c in range(160)]
big = np.concatenate(tiles)[None]
res["443k_frame"] = builders(big, np.array([side * ext[0], 10 * ext[1], ext[2]]), f"{big.shape[1]} atoms, 1 frame", cutoff=False)

# eval-struct's frame: frames_to_batch + model, 32 frames per batch, 96 frames
atoms = atoms_onehot(s.elements)
model = nmrgnn_amd.load_model()
model.build(atoms.shape[1])
model.freeze()
res["eval_struct_ms_per_frame"] = {}
for name, dims in boxes(ext):
    def frame_loop(dims=dims):
        for b0 in range(0, 96, 32):
            model(frames_to_batch(atoms, hundred[b0:b0 + 32], 16, device=dev, box=dims))
    ms = median_ms(frame_loop, reps=5) / 96
    res["eval_struct_ms_per_frame"][name] = ms
    print(f"{'eval-struct frame':>22s} {name:>9s}: {ms:.4f} ms per frame", flush=True)

if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1)
