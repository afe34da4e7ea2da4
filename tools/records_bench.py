"""What building a record store on the device costs.

(a) ``ng_store_from_batch`` alone, through the C entry point: a batch of 4096 structures of 256 atoms, K = 16, C = 10
    (synthetic lists: neighbours drawn inside each structure, an eighth of the slots padding), written to store rows 0 ..
    N.  Device events around ``--launches`` launches back to back after 20 warm-up ones, against the bytes the launch must
    move (every batch word read once: atoms, nlist, edges, shift, name id; every store word written once: atoms, nlist,
    edges, inv_degree, y (3 words), w; graph_ptr and the binary search's re-reads not counted) at 6.3 TB/s (the achievable
    HBM rate, MI355X_MICROARCH.md) and at the 8 TB/s peak.  One launch reads 185 MB and writes 197 MB; consecutive launches
    ALTERNATE between two batches and two stores (764 MB in all, three times the 256 MiB Infinity Cache), so that no launch
    finds its inputs on-die from the launch before.
(b) ``ShiftDataset.from_structures`` on ``--molecules`` (4096) synthetic molecules of 8 to 120 atoms held in memory
    (``Structure`` objects and shift tables, a label on about 40 % of the atoms) against the host loop the package offered
    before: ``library.universe2graph`` per molecule plus the same labels, then ``ShiftDataset.from_records`` — both end
    with the store on the device.  Host clock to a device synchronise, one warm-up of each, then the two ALTERNATING,
    ``--reps`` each; median, min and max.  Where from_structures' time goes: the host preparation (label join, one-hot
    rows, name ids) timed on its own, and the device part (``structures_to_batch`` + ``ng_store_from_batch`` on prepared
    arrays) timed on its own.  PDB parsing is host work outside both loops: ``read_pdb`` of the two test fixtures is
    reported separately.
usage: python tools/records_bench.py [--molecules M] [--reps N] [--launches L] [out.txt]"""
import ctypes as C
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nmrgnn_amd import _lib  # noqa: E402
from nmrgnn_amd._lib import ptr  # noqa: E402
from nmrgnn_amd.dataset import ShiftDataset  # noqa: E402
from nmrgnn_amd.graph import structures_to_batch  # noqa: E402
from nmrgnn_amd.library import universe2graph  # noqa: E402
from nmrgnn_amd.structure import Structure, atoms_onehot, join_shifts, name_ids, name_keys, name_table, read_pdb  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)
ATOMS, K, NC = 256, 16, 10


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def synthetic_batch(G, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    N = G * ATOMS
    off = (torch.arange(N, device=dev, dtype=torch.int32) // ATOMS * ATOMS)[:, None]
    nlist = off + torch.randint(0, ATOMS, (N, K), generator=g, device=dev, dtype=torch.int32)
    edges = torch.rand(N, K, generator=g, device=dev) * 0.4 + 0.05
    edges[torch.rand(N, K, generator=g, device=dev) < 0.125] = 0.0
    atoms = torch.zeros(N, NC, device=dev)
    atoms[torch.arange(N, device=dev), torch.randint(0, NC, (N,), generator=g, device=dev)] = 1.0
    shift = torch.randn(N, generator=g, device=dev) * 30 + 100
    shift[torch.rand(N, generator=g, device=dev) < 0.5] = float("nan")
    name_id = torch.randint(0, 500, (N,), generator=g, device=dev, dtype=torch.int32)
    gp = torch.arange(G + 1, device=dev, dtype=torch.int32) * ATOMS
    return gp, atoms, nlist.contiguous(), edges, shift, name_id


def store_alone(G, launches, out):
    ctx = _lib.get_context(dev.index)
    N = G * ATOMS
    f32, i32 = torch.float32, torch.int32
    batches = [synthetic_batch(G, s) for s in (1, 2)]
    stores = [[torch.empty(N, NC, dtype=f32, device=dev), torch.empty(N, K, dtype=i32, device=dev),
               torch.empty(N, K, dtype=f32, device=dev), torch.empty(N, dtype=f32, device=dev),
               torch.empty(N, 3, dtype=f32, device=dev), torch.empty(N, dtype=f32, device=dev)] for _ in (0, 1)]
    counters = torch.zeros(2, dtype=i32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch(i):
        b, s = batches[i & 1], stores[i & 1]
        ctx.check(ctx.lib.ng_store_from_batch(ctx.handle, st, N, K, NC, G, *[ptr(t) for t in b], 0, N, *[ptr(t) for t in s],
                                              ptr(counters)), "ng_store_from_batch")
    for i in range(20):
        launch(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        launch(i)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / launches
    rd, wr = N * (4 * NC + 8 * K + 4 + 4), N * (4 * NC + 8 * K + 4 + 12 + 4)
    nbytes = rd + wr
    roof63, roof8 = nbytes / 6.3e12 * 1e6, nbytes / 8e12 * 1e6
    bad, labelled = counters.cpu().tolist()
    out(f"(a) ng_store_from_batch: G = {G}, N = {N}, K = {K}, C = {NC}: {rd / 1e6:.1f} MB read + {wr / 1e6:.1f} MB written per "
        f"launch, {launches} launches back to back alternating between two batches and two stores ({2 * nbytes / 1e6:.0f} MB "
        f"touched): {us:.2f} us per launch = {nbytes / us / 1e6:.2f} TB/s; HBM roofline {roof63:.2f} us at 6.3 TB/s "
        f"({us / roof63:.2f}x over), {roof8:.2f} us at 8 TB/s ({us / roof8:.2f}x over); counters after {launches + 20} launches: "
        f"{bad} slots outside, {labelled} labelled rows")


def molecules(M, seed=11):
    rng = np.random.default_rng(seed)
    structs, tables = [], []
    for m in range(M):
        n = int(rng.integers(8, 121))
        el = rng.choice(["H", "C", "N", "O"], size=n, p=[0.5, 0.3, 0.1, 0.1])
        names = [f"{e}{i}" for i, e in enumerate(el)]
        pos = rng.uniform(0, 2.2 * n ** (1 / 3) + 2.0, (n, 3))
        structs.append(Structure(names, ["LIG"] * n, [1 + i // 8 for i in range(n)], list(el), [pos]))
        pick = np.nonzero(rng.random(n) < 0.4)[0]
        tables.append({"resid": np.asarray([1 + i // 8 for i in pick], np.int64), "name": np.asarray([names[i] for i in pick], dtype=str),
                       "shift": rng.normal(60, 40, len(pick)).astype(np.float32), "resname": None})
    return structs, tables


def host_loop(structs, tables, table):
    recs = []
    for s, t in zip(structs, tables):
        sh, _ = join_shifts(s, t)
        has = np.isfinite(sh)
        y = np.stack([np.where(has, sh, 0), name_ids(s, table).astype(np.float32), has], axis=1).astype(np.float32)
        recs.append((universe2graph(s), y, has.astype(np.float32)))
    return ShiftDataset.from_records(recs, device=dev)


def host_prep(structs, tables):
    keys = [name_keys(s) for s in structs]
    table = name_table(structs, keys)
    return [(atoms_onehot(s.elements), join_shifts(s, t)[0], name_ids(s, table, k)) for s, t, k in zip(structs, tables, keys)]


def device_part(structs, per):
    ctx = _lib.get_context(dev.index)
    gb = structures_to_batch([p[0] for p in per], [s.frames[0] for s in structs], K, device=dev)
    N = gb.N
    meta = torch.from_numpy(np.concatenate([np.concatenate([p[1] for p in per]).view(np.int32),
                                            np.concatenate([p[2] for p in per])])).to(dev)
    f32, i32 = torch.float32, torch.int32
    s = [torch.empty(N, NC, dtype=f32, device=dev), torch.empty(N, K, dtype=i32, device=dev), torch.empty(N, K, dtype=f32, device=dev),
         torch.empty(N, dtype=f32, device=dev), torch.empty(N, 3, dtype=f32, device=dev), torch.empty(N, dtype=f32, device=dev)]
    counters = torch.zeros(2, dtype=i32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ctx.check(ctx.lib.ng_store_from_batch(ctx.handle, st, N, K, NC, gb.G, ptr(gb.graph_ptr), ptr(gb.atoms), ptr(gb.nlist),
                                          ptr(gb.edges), ptr(meta[:N]), ptr(meta[N:]), 0, N, *[ptr(t) for t in s], ptr(counters)),
              "ng_store_from_batch")
    return counters.cpu()


def med(v):
    return f"{statistics.median(v):.1f} ms (min {min(v):.1f}, max {max(v):.1f})"


def build_store(M, reps, out):
    structs, tables = molecules(M)
    table = name_table(structs)
    n_atoms = sum(s.n_atoms for s in structs)
    new = lambda: ShiftDataset.from_structures(structs, tables, neighbor_number=K, device=dev)  # noqa: E731
    old = lambda: host_loop(structs, tables, table)  # noqa: E731
    a, b = new(), old()
    torch.cuda.synchronize()
    same_labels = torch.equal(a.y, b.y) and torch.equal(a.w, b.w) and torch.equal(a.atoms, b.atoms)
    agree = float((a.nlist == b.nlist).float().mean())
    ta, tb, tp, td = [], [], [], []
    for _ in range(reps):
        ta.append(wall_ms(new)[0])
        tb.append(wall_ms(old)[0])
        ms, per = wall_ms(lambda: host_prep(structs, tables))
        tp.append(ms)
        td.append(wall_ms(lambda: device_part(structs, per))[0])
    fa, fb = statistics.median(ta), statistics.median(tb)
    out(f"(b) {M} molecules of 8-120 atoms ({n_atoms} atoms, {int(a.w.sum().item())} labels), K = {K}, {reps} alternating "
        f"repetitions: from_structures {med(ta)}; host loop universe2graph + from_records {med(tb)}; host loop / "
        f"from_structures = {fb / fa:.2f}")
    out(f"    where from_structures' time goes: host preparation (name table, label join, one-hot rows, name ids) {med(tp)}; "
        f"device part (structures_to_batch + ng_store_from_batch + the counter read, from prepared arrays) {med(td)}")
    out(f"    same labels, weights and atom rows in both stores: {same_labels}; neighbour slots that agree between the GPU "
        f"lists and the host's cKDTree lists: {100 * agree:.3f} %")
    for f in ("108M.pdb", "7lgi.pdb.gz"):
        ms = []
        for _ in range(3):
            t = time.perf_counter()
            s = read_pdb(os.path.join(ROOT, "tests", "data", f))
            ms.append((time.perf_counter() - t) * 1e3)
        out(f"    read_pdb {f} ({s.n_atoms} atoms x {len(s)} frames): {statistics.median(ms):.1f} ms on the host, outside both loops")


def main():
    path = next((a for a in sys.argv[1:] if a.endswith(".txt")), None)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"device: {torch.cuda.get_device_name(dev)}")
    store_alone(4096, arg("--launches", 100), out)
    build_store(arg("--molecules", 4096), arg("--reps", 5), out)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
