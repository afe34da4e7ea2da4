"""What the device-resident record store buys a training loop.

A synthetic store: ``--records`` (4096) records of 256 atoms, K = 16, C = 10 (``--unique`` (512) different graphs, repeated:
generating one costs a 256 x 256 random matrix), atom_feature_size 64.  About 190 bytes per atom, 200 MB in all — below the
256 MiB Infinity Cache, so part of the collate's reads may be served on-die.

(a) ``ng_collate_batch`` alone, through the C entry point on preallocated outputs: 512 random records per launch, device
    events around ``--launches`` launches after 20 warm-up ones, against the bytes it must move (every store row read once,
    every batch row written once; the 2 KB of ids / graph_ptr and the binary search's re-reads not counted) at 6.3 TB/s (the
    achievable HBM rate, MI355X_MICROARCH.md) and at the 8 TB/s peak.  Also the host wall time of ``ShiftDataset.batch``
    (the copy of ids / graph_ptr, the launch, the list builders) ending in a device synchronise.
(b) one epoch (4096 records, store order, no validation) at 512 records per step and at 1 record per step:
    ``GNNModel.fit`` against the only loop the package offered before — host records -> ``graph.concat_graphs`` ->
    ``Trainer.step``.  Host clock around an epoch that ends in a device synchronise, one warm-up epoch of each, then the two
    ALTERNATING, ``--reps`` each; median, min and max.  Both loops end in the same weights (checked bit for bit).
usage: python tools/fit_bench.py [--records R] [--unique U] [--reps N] [--launches L] [out.txt]"""
import ctypes as C
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmrgnn_amd import _lib, synth  # noqa: E402
from nmrgnn_amd._lib import ptr  # noqa: E402
from nmrgnn_amd.dataset import ShiftDataset  # noqa: E402
from nmrgnn_amd.graph import concat_graphs  # noqa: E402
from nmrgnn_amd.hypers import HyperParameters  # noqa: E402
from nmrgnn_amd.model import build_GNNModel  # noqa: E402
from nmrgnn_amd.train import Trainer  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)
ATOMS, K, NC = 256, 16, 10


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def make_records(n_records, n_unique):
    rng = np.random.default_rng(7)
    uniq = []
    for _ in range(n_unique):
        atoms, nl, d = synth.make_graph(ATOMS, K, NC, 0.05, rng)
        y = np.stack([rng.standard_normal(ATOMS), rng.integers(0, 40, size=ATOMS), np.ones(ATOMS)], axis=1).astype(np.float32)
        uniq.append(((atoms, nl.astype(np.int32), d, synth.inv_degree(nl)), y, np.ones(ATOMS, np.float32)))
    return [uniq[i % n_unique] for i in range(n_records)]


def collate_alone(ds, G, launches, out):
    ctx = _lib.get_context(dev.index)
    rng = np.random.default_rng(1)
    ids = rng.integers(0, len(ds), size=G)
    gp = np.concatenate([[0], np.cumsum(ds.record_sizes()[ids])])
    N = int(gp[-1])
    ids_d = torch.from_numpy(ids.astype(np.int32)).to(dev)
    gp_d = torch.from_numpy(gp.astype(np.int32)).to(dev)
    f32, i32 = torch.float32, torch.int32
    o = [torch.empty(N, NC, dtype=f32, device=dev), torch.empty(N, K, dtype=i32, device=dev), torch.empty(N, K, dtype=f32, device=dev),
         torch.empty(N, dtype=f32, device=dev), torch.empty(N, dtype=f32, device=dev), torch.empty(N, dtype=f32, device=dev),
         torch.empty(N, dtype=i32, device=dev)]
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        ctx.check(ctx.lib.ng_collate_batch(ctx.handle, st, ds.R, ds.Ntot, ptr(ds.atoms), ptr(ds.nlist), ptr(ds.edges),
                                           ptr(ds.inv_degree), ptr(ds.y), ptr(ds.w), ptr(ds.rec_ptr), ptr(ids_d), ptr(gp_d), N, K, NC,
                                           G, *[ptr(t) for t in o], None), "ng_collate_batch")
    for _ in range(20):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / launches
    # read: atoms, nlist, edges, inv_degree, y (3 words), w; written: atoms, nlist, edges, inv_degree, y0, w, names
    nbytes = N * (4 * NC + 8 * K + 4 + 12 + 4) + N * (4 * NC + 8 * K + 4 * 4)
    roof63, roof8 = nbytes / 6.3e12 * 1e6, nbytes / 8e12 * 1e6
    out(f"(a) ng_collate_batch: G = {G}, N = {N}, {nbytes / 1e6:.2f} MB moved, {launches} launches back to back: "
        f"{us:.2f} us per launch = {nbytes / us / 1e6:.2f} TB/s; HBM roofline {roof63:.2f} us at 6.3 TB/s ({us / roof63:.2f}x over), "
        f"{roof8:.2f} us at 8 TB/s ({us / roof8:.2f}x over)")
    walls = []
    for _ in range(30):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ds.batch(ids)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t) * 1e3)
    out(f"    ShiftDataset.batch (ids copy + collate + list builders), host wall to a device synchronise: median "
        f"{statistics.median(walls[10:]):.3f} ms over 20 calls")


def model():
    return build_GNNModel(HyperParameters(atom_feature_size=64), device=dev)


def fit_epoch(m, ds, G):
    m.fit(ds, epochs=1, batch_graphs=G, shuffle=False, verbose=0)


def host_epoch(m, tr, recs, G):
    for c in range(0, len(recs), G):
        part = recs[c:c + G]
        gb = concat_graphs([r[0] for r in part], device=dev)
        y = torch.from_numpy(np.concatenate([r[1][:, 0] for r in part])).to(dev)
        w = torch.from_numpy(np.concatenate([r[2] for r in part])).to(dev)
        tr.step(gb, y, w)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def epochs(ds, recs, G, reps, out):
    ma, mb = model(), model()
    mb.build(NC)
    tr = Trainer(mb.engine, lr=mb.optimizer["learning_rate"], loss_balance=1.0)
    fit_epoch(ma, ds, G)
    host_epoch(mb, tr, recs, G)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(wall_ms(lambda: fit_epoch(ma, ds, G)))
        tb.append(wall_ms(lambda: host_epoch(mb, tr, recs, G)))
    tr.close()
    same = torch.equal(ma.engine.params.flat, mb.engine.params.flat)
    steps = -(-len(recs) // G)
    fa, fb = statistics.median(ta), statistics.median(tb)
    out(f"(b) epoch of {len(recs)} records at {G} per step ({steps} steps), {reps} alternating repetitions: "
        f"fit on the device store {fa:.1f} ms (min {min(ta):.1f}, max {max(ta):.1f}) = {fa / steps:.3f} ms per step; "
        f"host records -> concat_graphs -> Trainer.step {fb:.1f} ms (min {min(tb):.1f}, max {max(tb):.1f}) = {fb / steps:.3f} ms per "
        f"step; host loop / fit = {fb / fa:.2f}; same weights afterwards: {same}")


def main():
    path = next((a for a in sys.argv[1:] if a.endswith(".txt")), None)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    n_rec, n_uni, reps = arg("--records", 4096), arg("--unique", 512), arg("--reps", 5)
    t = time.perf_counter()
    recs = make_records(n_rec, min(n_uni, n_rec))
    ds = ShiftDataset.from_records(recs, device=dev)
    out(f"store: {len(ds)} records x {ATOMS} atoms, K = {K}, C = {NC}, {ds.Ntot * (4 * NC + 8 * K + 20) / 1e6:.0f} MB on "
        f"{torch.cuda.get_device_name(dev)}; built in {time.perf_counter() - t:.1f} s; model F = 64")
    collate_alone(ds, min(512, n_rec), arg("--launches", 200), out)
    for G in (512, 1):
        epochs(ds, recs, G, reps, out)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
