"""Neighbour lists of ragged batches (csrc/ragged.hip, graph.structures_to_batch), hipEvent-timed, median of 20 calls after
warm-up, ms per call.
  (a) 4096 seeded synthetic molecules of 8-120 atoms, K = 16:
      ragged kNN build, ragged cutoff build (4 A), a loop of per-structure frames_to_batch + concat_graphs, host knn_graph +
      concat_graphs; the ragged builds both as the library calls alone (kernels; the cutoff's scan and nnz read excluded)
      and as the whole structures_to_batch call
  (b) one 7lgi frame + 108M + 2000 of those molecules in one batch: ragged kNN and cutoff; and the 7lgi frame alone through
      the uniform builder (ng_knn_graph) and the ragged one
  (c) model inference on (a) end to end (structures_to_batch + model, baseline architecture, seeded weights)
--boxes: periodic boxes per structure (structures_to_batch(boxes=), the _ragged_pbc entry points) on (a) and (b): all open
  through the open entry points, all orthorhombic, all triclinic (b_x = a_x / 4, c_x = -a_x / 5, c_y = 0.3 b_y), and one third
  of each kind; kNN kernels, cutoff count and fill, and the whole calls, each also as a ratio to the open figure of the same run.
  The open figures of another build of the library (the parent commit's, to show the open path did not move) come from a run
  of the plain mode with NMRGNN_HIP_LIB set to that build, alternating with this one on the same machine.
Each mode is one process: run it under a time limit of its own (timeout -k 10 300 python tools/ragged_time.py --boxes out.json)
and start nothing more on the GPU after a run that faulted or timed out.
usage: python tools/ragged_time.py [--boxes] [out.json]"""
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrgnn_amd import _lib  # noqa: E402
from nmrgnn_amd._lib import ptr  # noqa: E402
from nmrgnn_amd.graph import concat_graphs, frames_to_batch, structures_to_batch  # noqa: E402
from nmrgnn_amd.structure import atoms_onehot, inv_degree_of, knn_graph, read_pdb  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)
ctx = _lib.get_context(0)
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
K = 16


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


def molecules(G, seed=1, lo=8, hi=120):
    """G molecules of lo..hi atoms at liquid-like density (0.1 atoms / A^3), H/C/N/O"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, G)
    atoms, pos = [], []
    for n in sizes:
        atoms.append(atoms_onehot(rng.choice(["H", "C", "N", "O"], n, p=[0.5, 0.3, 0.1, 0.1])))
        pos.append(rng.uniform(0, (n / 0.1) ** (1.0 / 3.0), (n, 3)).astype(np.float32))
    return atoms, pos


def kernels(pos_dev, gp_host, cutoff):
    """the library calls alone on device inputs: kNN; cutoff count + fill (row_ptr from one untimed count + scan)"""
    N, G = int(gp_host[-1]), len(gp_host) - 1
    max_n = int(np.max(np.diff(gp_host)))
    gp_dev = torch.from_numpy(gp_host).to(dev)
    nl = torch.empty((N, K), dtype=torch.int32, device=dev)
    ed = torch.empty((N, K), device=dev)
    inv = torch.empty(N, device=dev)
    deg = torch.empty(N, dtype=torch.int32, device=dev)
    rp = torch.empty(N + 1, dtype=torch.int32, device=dev)
    knn = lambda: ctx.check(ctx.lib.ng_knn_graph_ragged(ctx.handle, st, G, N, K, 0.1, ptr(pos_dev), ptr(gp_dev),
                                                         C.c_void_p(gp_host.ctypes.data), max_n, ptr(nl), ptr(ed), ptr(inv)),
                            "knn")
    count = lambda: ctx.check(ctx.lib.ng_cutoff_count_ragged(ctx.handle, st, G, N, cutoff, ptr(pos_dev), ptr(gp_dev), max_n,
                                                             ptr(deg)), "count")
    count()
    ctx.check(ctx.lib.ng_exclusive_scan_i32(ctx.handle, st, N, ptr(deg), ptr(rp)), "scan")
    nnz = int(deg.sum(dtype=torch.int64))
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    dist = torch.empty(nnz, device=dev)
    row_of = torch.empty(nnz, dtype=torch.int32, device=dev)
    fill = lambda: ctx.check(ctx.lib.ng_cutoff_fill_rows_ragged(ctx.handle, st, G, N, cutoff, 0.1, ptr(pos_dev), ptr(gp_dev),
                                                                max_n, ptr(rp), ptr(col), ptr(dist), ptr(inv), ptr(row_of)),
                             "fill")
    return {"knn_kernel_ms": median_ms(knn), "cutoff_count_ms": median_ms(count), "cutoff_fill_ms": median_ms(fill),
            "nnz": nnz}


def set_a(out):
    atoms, pos = molecules(4096)
    sizes = np.array([len(p) for p in pos])
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    A = np.concatenate(atoms)
    P = torch.from_numpy(np.concatenate(pos)).to(dev)
    pairs = int((sizes.astype(np.int64) * (sizes - 1)).sum())
    r = {"structures": 4096, "atoms": int(gp[-1]), "pairs": pairs}
    r.update(kernels(P, gp, 4.0))
    r["ragged_knn_call_ms"] = median_ms(lambda: structures_to_batch(A, P, K, sizes=sizes, device=dev))
    r["ragged_cutoff_call_ms"] = median_ms(lambda: structures_to_batch(A, P, cutoff=4.0, sizes=sizes, device=dev))

    def loop():
        tup = []
        for a, p in zip(atoms, pos):
            b = frames_to_batch(a, p, K, device=dev)
            tup.append(tuple(t.cpu() for t in b.as_tuple()))
        return concat_graphs(tup, device=dev)
    r["per_structure_loop_ms"] = median_ms(loop)

    def host():
        tup = []
        for a, p in zip(atoms, pos):
            nl, ed = knn_graph(p, K)
            tup.append((a, nl, ed, inv_degree_of(nl)))
        return concat_graphs(tup, device=dev)
    r["host_knn_concat_ms"] = median_ms(host)
    r["loop_over_ragged_knn_call"] = r["per_structure_loop_ms"] / r["ragged_knn_call_ms"]
    out["a"] = r
    return atoms, pos


def set_b(out, atoms, pos):
    s1 = read_pdb("tests/data/7lgi.pdb.gz")
    s2 = read_pdb("tests/data/108M.pdb")
    at = [atoms_onehot(s1.elements), atoms_onehot(s2.elements)] + atoms[:2000]
    ps = [np.asarray(s1.frames[0], np.float32), np.asarray(s2.frames[0], np.float32)] + pos[:2000]
    sizes = np.array([len(p) for p in ps])
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    P = torch.from_numpy(np.concatenate(ps)).to(dev)
    r = {"structures": len(ps), "atoms": int(gp[-1])}
    r.update(kernels(P, gp, 4.0))
    r["ragged_knn_call_ms"] = median_ms(lambda: structures_to_batch(np.concatenate(at), P, K, sizes=sizes, device=dev))
    # the 7lgi frame alone: uniform (one wave per query) and ragged (one thread per query)
    n = len(ps[0])
    P1 = P[:n].contiguous()
    nl = torch.empty((n, K), dtype=torch.int32, device=dev)
    ed = torch.empty((n, K), device=dev)
    inv = torch.empty(n, device=dev)
    r["lgi_alone_uniform_knn_ms"] = median_ms(lambda: ctx.check(ctx.lib.ng_knn_graph(
        ctx.handle, st, 1, n, K, 0.1, ptr(P1), ptr(nl), ptr(ed), ptr(inv)), "knn"))
    r["lgi_alone_ragged_knn_ms"] = kernels(P1, np.array([0, n], np.int32), 4.0)["knn_kernel_ms"]
    out["b"] = r


def set_c(out, atoms, pos):
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    from nmrgnn_amd.model import GNNModel
    from nmrgnn_amd.standards import load_standards
    model = GNNModel(declare_gnn_space(HyperParameters()), load_standards(), device=dev, seed=1)
    model.build(atoms[0].shape[1])
    model.freeze()
    sizes = np.array([len(p) for p in pos])
    A = np.concatenate(atoms)
    P = torch.from_numpy(np.concatenate(pos)).to(dev)
    b = structures_to_batch(A, P, K, sizes=sizes, device=dev)
    out["c"] = {"model_only_ms": median_ms(lambda: model(b)),
                "build_plus_model_ms": median_ms(lambda: model(structures_to_batch(A, P, K, sizes=sizes, device=dev)))}


def boxes_of(sizes, kinds, min_width=8.5):
    """one box per structure at 0.1 atoms / A^3, grown where needed until its smallest width is min_width (above twice the
    4 A cutoff); kinds -1 open, 0 orthorhombic, 1 triclinic"""
    from nmrgnn_amd.pbc import triclinic_vectors, widths
    out = []
    for n, k in zip(sizes, kinds):
        if k < 0:
            out.append(None)
            continue
        L = (n / 0.1) ** (1.0 / 3.0)
        if k == 0:
            d = np.array([L, L, L, 90.0, 90.0, 90.0])
        else:
            v = np.array([[L, 0, 0], [L / 4, L, 0], [-L / 5, 0.3 * L, L]])
            nv = np.linalg.norm(v, axis=1)
            ang = lambda x, y: np.degrees(np.arccos(np.dot(x, y) / np.linalg.norm(x) / np.linalg.norm(y)))
            d = np.array([nv[0], nv[1], nv[2], ang(v[1], v[2]), ang(v[0], v[2]), ang(v[0], v[1])])
        w = widths(triclinic_vectors(d)).min()
        if w < min_width:
            d[:3] *= 1.01 * min_width / w
        out.append(tuple(float(x) for x in d))
    return out


def kernels_boxed(pos_dev, gp_host, cutoff, boxes):
    """kernels() through the per-structure entry points"""
    from nmrgnn_amd.pbc import prepare_ragged
    N, G = int(gp_host[-1]), len(gp_host) - 1
    max_n = int(np.max(np.diff(gp_host)))
    vec, kind_host, _ = prepare_ragged(boxes, G)
    gp_dev, box, kind = torch.from_numpy(gp_host).to(dev), torch.from_numpy(vec).to(dev), torch.from_numpy(kind_host).to(dev)
    gph, kh = C.c_void_p(gp_host.ctypes.data), C.c_void_p(kind_host.ctypes.data)
    nl = torch.empty((N, K), dtype=torch.int32, device=dev)
    ed = torch.empty((N, K), device=dev)
    inv = torch.empty(N, device=dev)
    deg = torch.empty(N, dtype=torch.int32, device=dev)
    rp = torch.empty(N + 1, dtype=torch.int32, device=dev)
    knn = lambda: ctx.check(ctx.lib.ng_knn_graph_ragged_pbc(ctx.handle, st, G, N, K, 0.1, ptr(pos_dev), ptr(gp_dev), gph, max_n,
                                                             ptr(box), ptr(kind), kh, ptr(nl), ptr(ed), ptr(inv)), "knn")
    count = lambda: ctx.check(ctx.lib.ng_cutoff_count_ragged_pbc(ctx.handle, st, G, N, cutoff, ptr(pos_dev), ptr(gp_dev), max_n,
                                                                 ptr(box), ptr(kind), kh, ptr(deg)), "count")
    count()
    ctx.check(ctx.lib.ng_exclusive_scan_i32(ctx.handle, st, N, ptr(deg), ptr(rp)), "scan")
    nnz = int(deg.sum(dtype=torch.int64))
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    dist = torch.empty(nnz, device=dev)
    row_of = torch.empty(nnz, dtype=torch.int32, device=dev)
    fill = lambda: ctx.check(ctx.lib.ng_cutoff_fill_rows_ragged_pbc(ctx.handle, st, G, N, cutoff, 0.1, ptr(pos_dev), ptr(gp_dev),
                                                                    max_n, ptr(box), ptr(kind), kh, ptr(rp), ptr(col),
                                                                    ptr(dist), ptr(inv), ptr(row_of)), "fill")
    return {"knn_kernel_ms": median_ms(knn), "cutoff_count_ms": median_ms(count), "cutoff_fill_ms": median_ms(fill),
            "nnz": nnz}


def boxed_set(A, P, sizes, with_calls=True):
    """open / orthorhombic / triclinic / one third each on one batch; ratios to the open figures of this run"""
    from nmrgnn_amd.pbc import prepare_ragged
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    G = len(sizes)
    r = {"open": kernels(P, gp, 4.0)}
    if with_calls:
        r["open"]["knn_call_ms"] = median_ms(lambda: structures_to_batch(A, P, K, sizes=sizes, device=dev))
        r["open"]["cutoff_call_ms"] = median_ms(lambda: structures_to_batch(A, P, cutoff=4.0, sizes=sizes, device=dev))
    for name, kinds in (("ortho", np.zeros(G, int)), ("tric", np.ones(G, int)), ("mixed", np.arange(G) % 3 - 1)):
        boxes = boxes_of(sizes, kinds)
        q = kernels_boxed(P, gp, 4.0, boxes)
        if with_calls:
            q["knn_call_ms"] = median_ms(lambda: structures_to_batch(A, P, K, sizes=sizes, device=dev, boxes=boxes))
            q["cutoff_call_ms"] = median_ms(lambda: structures_to_batch(A, P, cutoff=4.0, sizes=sizes, device=dev, boxes=boxes))
            t0 = time.perf_counter()
            prepare_ragged(boxes, G)
            q["host_prepare_ms"] = 1e3 * (time.perf_counter() - t0)     # the host validation inside the whole calls
        for k in [k for k in q if k.endswith("_ms") and k in r["open"]]:
            q[k.replace("_ms", "_over_open")] = q[k] / r["open"][k]
        r[name] = q
    return r


def main_boxes(path):
    out = {}
    atoms, pos = molecules(4096)
    sizes = np.array([len(p) for p in pos])
    out["a"] = boxed_set(np.concatenate(atoms), torch.from_numpy(np.concatenate(pos)).to(dev), sizes)
    print(json.dumps({"a": out["a"]}), flush=True)
    s1 = read_pdb("tests/data/7lgi.pdb.gz")
    s2 = read_pdb("tests/data/108M.pdb")
    at = [atoms_onehot(s1.elements), atoms_onehot(s2.elements)] + atoms[:2000]
    ps = [np.asarray(s1.frames[0], np.float32), np.asarray(s2.frames[0], np.float32)] + pos[:2000]
    out["b"] = boxed_set(np.concatenate(at), torch.from_numpy(np.concatenate(ps)).to(dev), np.array([len(p) for p in ps]))
    print(json.dumps({"b": out["b"]}), flush=True)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


def main():
    args = [a for a in sys.argv[1:] if a != "--boxes"]
    if "--boxes" in sys.argv[1:]:
        return main_boxes(args[0] if args else None)
    out = {}
    atoms, pos = set_a(out)
    print(json.dumps({"a": out["a"]}), flush=True)
    set_b(out, atoms, pos)
    print(json.dumps({"b": out["b"]}), flush=True)
    set_c(out, atoms, pos)
    print(json.dumps({"c": out["c"]}), flush=True)
    if args:
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
