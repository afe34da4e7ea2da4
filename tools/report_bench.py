"""What the evaluation report's device pass costs and what it saves.

(a) the ``ng_class_moments`` launch pair through the C entry point at ``--atoms`` (131072) atoms, M = 3 groupings of a table of
    20 residues x 95 atom names (K = 118 rows), with all, 30 % and none of the atoms labelled (none: the walk skips every atom,
    what is left is the tile load, the partial store and the final launch), against
      * the ``ng_name_metrics`` pair at K = 15 on the same arrays (the kernel it generalises), and
      * the time to read the 16 bytes per atom (y, w, name id, prediction) at 6.3 TB/s, the achievable HBM rate
        (MI355X_MICROARCH.md), and
      * the F = 64 inference forward on a batch of the same size (512 graphs x 256 atoms), which the pass follows.
    Device events around ``--launches`` launches, 20 warm-up ones, the legs ALTERNATING over ``--reps`` rounds; medians.
(b) a report over ``--records`` (4096) records of 256 atoms at 512 records per batch: ``GNNModel.evaluate_report`` (with and
    without the rows) against the only way there was before: ``model(batch)`` per batch, predictions to the host, grouped
    there in NumPy per element and atom name as the reference groups them in pandas.  Host clock around a run that ends in a device
    synchronise, one warm-up of each, then alternating; both ways must end in the same table.
usage: python tools/report_bench.py [--atoms N] [--records R] [--unique U] [--reps N] [--launches L] [out.txt]"""
import ctypes as C
import math
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
from nmrgnn_amd.graph import GraphBatch  # noqa: E402
from nmrgnn_amd.hypers import HyperParameters  # noqa: E402
from nmrgnn_amd.model import build_GNNModel  # noqa: E402
from nmrgnn_amd.report import class_maps  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda", 0)
ATOMS, K, NC = 256, 16, 10
CENTRE = {'H': (8.0, 1.0), 'C': (60.0, 10.0), 'N': (120.0, 5.0)}


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def name_table():
    """20 residues x 95 atom names, every residue with a third of the names: {'RES-NAME': id}, id 0 = 'X'"""
    rng = np.random.default_rng(3)
    names = ['H', 'N', 'C', 'CA', 'CB', 'HA'] + [f'{e}{g}{i}' for e in 'HCN' for g in 'BGDEZ' for i in range(1, 7)][:89]
    table = {'X': 0}
    for r in range(20):
        for n in sorted(set(names[:6]) | set(rng.choice(names, 30).tolist())):
            table[f'R{r:02d}-{n}'] = len(table)
    return table


def labels_for(ids, table, rng):
    keys = {v: k for k, v in table.items()}
    mu_sd = np.array([CENTRE[keys[i].split('-')[1][0]] if i else (0.0, 1.0) for i in range(len(table))])
    return (mu_sd[ids, 0] + mu_sd[ids, 1] * rng.standard_normal(len(ids))).astype(np.float32)


def timed(fns, launches, reps):
    """median us per call of every leg, the legs alternating"""
    for fn in fns:
        for _ in range(20):
            fn()
    us = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    return [(statistics.median(u), min(u), max(u)) for u in us]


def launch_pair(N, launches, reps, out):
    ctx = _lib.get_context(dev.index)
    rng = np.random.default_rng(1)
    table = name_table()
    class_of, labels = class_maps(table)
    Kc, n_ids = len(labels.text), class_of.shape[1]
    ids = rng.integers(0, n_ids, N)
    y = labels_for(ids, table, rng)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    y_d, names_d = t(y, torch.float32), t(ids, torch.int32)
    p_d = t(y + 0.5 * rng.standard_normal(N).astype(np.float32), torch.float32)
    w_all = torch.ones(N, device=dev)
    w_30 = t((rng.random(N) < 0.3).astype(np.float32), torch.float32)
    w_none = torch.zeros(N, device=dev)
    table_d = t(class_of, torch.int32)
    mom = torch.zeros(Kc, 7, dtype=torch.float64, device=dev)
    member = t(rng.integers(0, 1 << 15, n_ids).astype(np.int32), torch.int32)
    mom15 = torch.zeros(15, 7, dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def cm(w):
        return lambda: ctx.check(ctx.lib.ng_class_moments(ctx.handle, st, N, ptr(y_d), ptr(w), ptr(names_d), ptr(p_d), n_ids, 3,
                                                          ptr(table_d), Kc, 0, ptr(mom)), "ng_class_moments")

    def nm():
        ctx.check(ctx.lib.ng_name_metrics(ctx.handle, st, N, ptr(y_d), ptr(w_all), ptr(names_d), ptr(p_d), n_ids, ptr(member), 15,
                                          0, ptr(mom15)), "ng_name_metrics")
    m = build_GNNModel(HyperParameters(atom_feature_size=64), device=dev)
    b = synth.make_batch(max(N // ATOMS, 1), ATOMS, K, NC, 0.05, seed=1)
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    m.build(NC)
    m.freeze()
    fwd = lambda: m.engine.forward(gb, training=False)
    res = timed([cm(w_all), cm(w_30), cm(w_none), nm, fwd], launches, reps)
    roof = 16 * N / 6.3e12 * 1e6
    out(f"(a) N = {N} atoms, M = 3, K = {Kc} rows ({n_ids} name ids), {launches} calls back to back, {reps} alternating rounds; "
        f"median (min, max) us per call:")
    for name, (med, lo, hi) in zip(("ng_class_moments, every atom labelled", "ng_class_moments, 30 % labelled",
                                    "ng_class_moments, no atom labelled (no walk)", "ng_name_metrics, K = 15",
                                    f"F = 64 inference forward, {gb.G} x {ATOMS} atoms"), res):
        out(f"    {name}: {med:.2f} ({lo:.2f}, {hi:.2f})")
    out(f"    reading 16 B per atom at 6.3 TB/s: {roof:.2f} us; class moments (all labelled) / name metrics = "
        f"{res[0][0] / res[3][0]:.2f}; class moments (all labelled) / forward = {res[0][0] / res[4][0]:.3f}, "
        f"(30 % labelled) / forward = {res[1][0] / res[4][0]:.3f}")


def make_store(n_records, n_unique, table):
    rng = np.random.default_rng(7)
    uniq = []
    for _ in range(n_unique):
        atoms, nl, d = synth.make_graph(ATOMS, K, NC, 0.05, rng)
        ids = rng.integers(0, len(table), size=ATOMS)
        mask = (rng.random(ATOMS) < 0.4).astype(np.float32)
        y = np.stack([labels_for(ids, table, rng), ids, mask], axis=1).astype(np.float32)
        uniq.append(((atoms, nl.astype(np.int32), d, synth.inv_degree(nl)), y, mask))
    return ShiftDataset.from_records([uniq[i % n_unique] for i in range(n_records)], device=dev)


def host_table(m, ds, table, G):
    """the way there was: per batch the predictions and labels to the host; grouped there per element and atom name"""
    keys = {v: k for k, v in table.items()}
    name_of = np.array([keys[i].split('-')[1] if '-' in keys[i] else '' for i in range(len(table))], dtype=object)
    elem_of = np.array([n[:1] for n in name_of], dtype=object)
    ys, ps, ids = [], [], []
    for batch, y_true in ds.eval_batches(G):
        p = m(batch).cpu().numpy().reshape(-1)
        yt = y_true.cpu().numpy()
        on = (yt[:, 2] > 0) & (yt[:, 1] > 0)
        ys.append(yt[on, 0])
        ps.append(p[on])
        ids.append(yt[on, 1].astype(np.int64))
    y, p, ids = np.concatenate(ys).astype(np.float64), np.concatenate(ps).astype(np.float64), np.concatenate(ids)
    rows = {}
    for stat in ('r', 'rmsd'):
        for col in (elem_of[ids], name_of[ids]):
            for v in np.unique(col):
                sel = col == v
                a, b = y[sel], p[sel]
                rows[f'-{v}-{stat}'] = [int(sel.sum()), float(np.corrcoef(a, b)[0, 1]) if stat == 'r' else float(np.mean((b - a) ** 2))]
    return rows


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, res


def whole_report(n_rec, n_uni, reps, out):
    table = name_table()
    t = time.perf_counter()
    ds = make_store(n_rec, min(n_uni, n_rec), table)
    m = build_GNNModel(HyperParameters(atom_feature_size=64), device=dev)
    m.build(NC)
    G = 512
    out(f"(b) store: {len(ds)} records x {ATOMS} atoms (40 % labelled), built in {time.perf_counter() - t:.1f} s; model F = 64; "
        f"{G} records per batch, {reps} alternating repetitions; host wall to a device synchronise, median (min, max) ms:")
    legs = [("evaluate_report, rows=False", lambda: m.evaluate_report(ds, table, batch_graphs=G, rows=False)),
            ("evaluate_report, rows=True", lambda: m.evaluate_report(ds, table, batch_graphs=G, rows=True)),
            ("model(batch) -> host -> NumPy groups", lambda: host_table(m, ds, table, G))]
    for _, fn in legs:
        fn()
    ms, last = [[] for _ in legs], [None] * len(legs)
    for _ in range(reps):
        for k, (_, fn) in enumerate(legs):
            dt, last[k] = wall_ms(fn)
            ms[k].append(dt)
    for (name, _), v in zip(legs, ms):
        out(f"    {name}: {statistics.median(v):.1f} ({min(v):.1f}, {max(v):.1f})")
    out(f"    host way / evaluate_report(rows=False) = {statistics.median(ms[2]) / statistics.median(ms[0]):.2f}, "
        f"/ evaluate_report(rows=True) = {statistics.median(ms[2]) / statistics.median(ms[1]):.2f}")
    mine, theirs = last[0].table('m')[1], last[2]
    same_keys = list(mine) == list(theirs)
    dn = max(abs(mine[k][0] - theirs[k][0]) for k in mine) if same_keys else math.nan
    dr = max(abs(mine[k][1] - theirs[k][1]) for k in mine if k.endswith('-r')) if same_keys else math.nan
    dm = max(abs(mine[k][1] - theirs[k][1]) / theirs[k][1] for k in mine if k.endswith('-rmsd')) if same_keys else math.nan
    out(f"    the two tables: same keys in the same order: {same_keys} ({len(mine)} rows); max |dN| = {dn}, max |dr| = {dr:.2e}, "
        f"max relative difference of the mean squared error = {dm:.2e}")


def main():
    path = next((a for a in sys.argv[1:] if a.endswith(".txt")), None)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"device: {torch.cuda.get_device_name(dev)}")
    launch_pair(arg("--atoms", 131072), arg("--launches", 200), arg("--reps", 5), out)
    whole_report(arg("--records", 4096), arg("--unique", 512), arg("--reps", 5), out)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
