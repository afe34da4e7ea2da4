"""NumPy statement of ``ShiftDataset.batch(ids)`` / ``ng_collate_batch``: pure copies and integer adds.

``store`` is a dict of host arrays: atoms [Ntot, C] f32, nlist [Ntot, K] i32 (record-local), edges [Ntot, K] f32,
inv_degree [Ntot] f32, y [Ntot, 3] f32, w [Ntot] f32, rec_ptr [R + 1] int64.  ``collate_ref(store, ids)`` returns the batch of
the records ``ids`` in that order: every array row by row, ``nlist`` with the graph's batch offset added to EVERY slot."""
import numpy as np


def make_records(sizes, K=16, C=10, seed=0, onehot=False):
    """synthetic ``(x, y, w)`` records: neighbours drawn from the same record, trailing slots padded (nlist 0, edges 0); a
    record with n <= K is mostly padding.  ``atoms`` rows are arbitrary floats unless ``onehot`` (the store keeps them as
    given)."""
    rng = np.random.default_rng(seed)
    recs = []
    for n in sizes:
        n = int(n)
        live = rng.integers(0, min(K, max(n - 1, 0)) + 1, size=n)         # live slots per atom
        real = np.arange(K)[None, :] < live[:, None]
        nlist = np.where(real, rng.integers(0, n, size=(n, K)), 0).astype(np.int32)
        edges = np.where(real, rng.uniform(0.09, 0.45, size=(n, K)), 0.0).astype(np.float32)
        if onehot:
            atoms = np.zeros((n, C), np.float32)
            atoms[np.arange(n), rng.integers(0, C, size=n)] = 1.0
        else:
            atoms = rng.standard_normal((n, C)).astype(np.float32)
        deg = (nlist > 0).sum(axis=1).astype(np.float32)
        inv = np.where(deg > 0, 1.0 / np.maximum(deg, 1.0), 0.0).astype(np.float32)
        y = np.stack([rng.standard_normal(n), rng.integers(0, 40, size=n) + rng.choice([0.0, 0.25, 0.75], size=n),
                      rng.integers(0, 2, size=n)], axis=1).astype(np.float32)
        w = rng.uniform(0.0, 2.0, size=n).astype(np.float32)
        recs.append(((atoms, nlist, edges, inv), y, w))
    return recs


def store_of(records):
    """the host arrays of a store holding ``records`` back to back"""
    cat = lambda f, dt: np.ascontiguousarray(np.concatenate([f(r) for r in records]), dtype=dt)  # noqa: E731
    return dict(atoms=cat(lambda r: r[0][0], np.float32), nlist=cat(lambda r: r[0][1], np.int32),
                edges=cat(lambda r: r[0][2], np.float32), inv_degree=cat(lambda r: np.reshape(r[0][3], -1), np.float32),
                y=cat(lambda r: r[1], np.float32), w=cat(lambda r: r[2], np.float32),
                rec_ptr=np.concatenate([[0], np.cumsum([r[0][0].shape[0] for r in records])]).astype(np.int64))


def collate_ref(store, ids):
    rp = store["rec_ptr"]
    out = {k: [] for k in ("atoms", "nlist", "edges", "inv_degree", "y_true", "w")}
    gp = [0]
    for i in ids:
        a, b = int(rp[i]), int(rp[i + 1])
        out["atoms"].append(store["atoms"][a:b])
        out["nlist"].append(store["nlist"][a:b] + np.int32(gp[-1]))
        out["edges"].append(store["edges"][a:b])
        out["inv_degree"].append(store["inv_degree"][a:b])
        out["y_true"].append(store["y"][a:b])
        out["w"].append(store["w"][a:b])
        gp.append(gp[-1] + b - a)
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["nlist"] = out["nlist"].astype(np.int32)
    out["y"] = np.ascontiguousarray(out["y_true"][:, 0])
    out["names"] = out["y_true"][:, 1].astype(np.int32)          # truncation
    out["graph_ptr"] = np.asarray(gp, np.int32)
    return out
