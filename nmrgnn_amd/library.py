"""Library surface of the reference (nmrgnn/library.py): ``load_model``, ``universe2graph``,
``check_peaks`` (+ ``save_model``), same names, argument order and return order; ``shift_restraint``, the
chemical-shift restraint energy and forces of a structure; and ``ShiftRestraint``, the replica-averaged restraint of R
structures as one graph-replayed call for an MD engine."""
from __future__ import annotations

import json
import os
import warnings

import numpy as np

from .hypers import HyperParameters, declare_gnn_space
from .standards import load_standards
from .structure import Structure, atoms_onehot, inv_degree_of, knn_graph, read_pdb


def _bundle_prefix(path):
    """SavedModel directory / variables directory / bundle prefix -> bundle prefix, or None."""
    for cand in (os.path.join(path, "variables", "variables"), os.path.join(path, "variables"), path):
        if os.path.isfile(cand + ".index"):
            return cand
    return None


def _load_tf_bundle(prefix, device):
    from .model import GNNModel
    from .tfbundle import load_gnn_bundle
    state, arch, num_elem = load_gnn_bundle(prefix)
    hp = declare_gnn_space(HyperParameters(**arch))
    model = GNNModel(hp, load_standards(), device=device)
    model.set_weights(state)
    model._num_elem_hint = num_elem
    return model


def load_model(model_file=None, device=None):
    """Load a chemical shift prediction model (nmrgnn/library.py:92-103).

    ``model_file`` is either a Keras SavedModel directory as the reference writes it (main.py:87-90:
    the weights are read from ``variables/variables.{index,data-*}`` with the built-in bundle reader,
    nmrgnn_amd/tfbundle.py; the architecture is inferred from the tensor shapes) or a directory
    written by ``GNNModel.save`` (weights.npz + config.json).  With no argument the reference loads
    its bundled pre-trained SavedModel; that bundle ships WITHOUT weight values (the data shard is
    missing upstream), so the baseline ARCHITECTURE and peak standards are restored and
    the weights are taken from $NMRGNN_AMD_BASELINE (a SavedModel directory or a weights.npz) when
    set, else seeded glorot — with a loud warning, because predictions are then meaningless."""
    from .model import GNNModel
    if model_file is None:
        w = os.environ.get("NMRGNN_AMD_BASELINE")
        if w and _bundle_prefix(w):
            return _load_tf_bundle(_bundle_prefix(w), device)
        hp = declare_gnn_space(HyperParameters())
        model = GNNModel(hp, load_standards(), device=device)
        if w:
            model.load_weights(w)
        else:
            warnings.warn("nmrgnn_amd.load_model(): the reference's bundled baseline has no weight "
                          "values (variables.data-00000-of-00001 is missing upstream); using seeded "
                          "random weights. Set NMRGNN_AMD_BASELINE=/path/to/saved_model_dir (or weights.npz).",
                          RuntimeWarning, stacklevel=2)
        return model
    if not os.path.exists(os.path.join(model_file, "config.json")):
        prefix = _bundle_prefix(model_file)
        if prefix is None:
            raise ValueError(f"{model_file}: neither a SavedModel directory (variables/variables.index) "
                             "nor a nmrgnn_amd model directory (config.json)")
        return _load_tf_bundle(prefix, device)
    with open(os.path.join(model_file, "config.json")) as f:
        cfg = json.load(f)
    hp = declare_gnn_space(HyperParameters(**cfg["hypers"]))
    standards = {int(k): tuple(v) for k, v in cfg["peak_standards"].items()}
    model = GNNModel(hp, standards, device=device)
    model.load_weights(model_file)
    if "num_elem" in cfg:
        model.build(int(cfg["num_elem"]))
    return model


def save_model(model, path):
    model.save(path)


def universe2graph(u, neighbor_number=16):
    """Convert a structure into the tuple (atoms, nlist, edges, inv_degree)
    (nmrgnn/library.py:106-117; note the order differs from parse_universe's).

    ``u`` may be an MDAnalysis Universe (``u.atoms.positions`` / ``.elements`` or ``.names``), a
    :class:`nmrgnn_amd.structure.Structure`, or a path to a PDB file.  Angstrom in, nm-scale
    distances out."""
    if isinstance(u, (str, os.PathLike)):
        u = read_pdb(u)
    if isinstance(u, Structure):
        pos, elements = u.positions, u.elements
    else:
        ag = u.atoms
        pos = np.asarray(ag.positions)
        try:
            elements = [str(e).capitalize() for e in ag.elements]
        except Exception:
            elements = ["".join(c for c in n if c.isalpha())[:1].upper() for n in ag.names]
    atoms = atoms_onehot(elements)
    nlist, edges = knn_graph(pos, neighbor_number)
    return atoms, nlist, edges, inv_degree_of(nlist)


def check_peaks(atoms, peaks, cutoff_sigma=4, warn_sigma=2.5):
    """True where a predicted shift is plausible given the training distribution of its element
    (nmrgnn/library.py:30-47; vectorised, ``np.bool`` -> ``bool``).  Raises ``Warning`` when fewer
    than 75 % of the atoms are within ``warn_sigma`` — the reference's behaviour."""
    standards = load_standards()
    atoms = np.asarray(atoms)
    peaks = np.asarray(peaks, dtype=np.float64).reshape(-1)
    C = atoms.shape[1]
    avg = np.array([standards.get(c, ('X', 0.0, 0.0))[1] for c in range(C)])
    std = np.array([standards.get(c, ('X', 0.0, 0.0))[2] for c in range(C)])
    elem = np.argmax(atoms != 0, axis=1)          # int(np.nonzero(atoms[i])[0]) of library.py:38
    s, a = std[elem], avg[elem]
    with np.errstate(divide="ignore", invalid="ignore"):
        z2 = (peaks - a) ** 2 / s ** 2
    confident = ~((s == 0) | (z2 > warn_sigma ** 2))
    if confident.shape[0] and confident.sum() / confident.shape[0] < 0.75:
        raise Warning('Your peaks look awful. Likely solvent or missing hydrogens or bad units. '
                      'Check README for suggestions')
    return confident


def shift_restraint(model, atoms, positions, targets, weights=None, neighbor_number=16, box=None, virial=False, prune=False):
    """Chemical-shift restraint of one structure: ``(energy, forces)`` with

        energy = sum_i w_i (delta_pred_i - delta_exp_i)^2          ppm^2, a 0-d device tensor
        forces = -d energy / d positions                           ppm^2 / Angstrom, [n, 3] on the device

    ``atoms`` [n, C] one-hot, ``positions`` [n, 3] in Angstrom, ``targets`` [n] measured shifts in ppm, ``weights`` [n]
    (default 1; put 0 where no shift was measured).  The graph is the kNN graph of ``frames_to_batch`` with
    ``neighbor_number`` neighbours; the model runs in inference mode.  One forward with a tape, one backward with the
    edge gradient (``Engine.backward(edge_grad=...)``) and one positions kernel (``GraphBatch.positions_grad``), no torch
    autograd; the forces are bitwise those of ``energy.backward()`` through ``model(frames_to_batch(atoms, pos))``.

    The forces are the gradient at FIXED neighbour lists: where an atom's K nearest neighbours change between two
    structures the energy and the forces jump (the model itself is discontinuous there, as the reference is).  The call
    overwrites the engine's parameter gradient buffer (``engine.params.grad``) as a side effect.

    ``box`` ``(a, b, c, alpha, beta, gamma)``: a periodic box under the minimum-image convention, as ``frames_to_batch``
    takes it; the forces are then those of ``model(frames_to_batch(atoms, pos, box=box))``.

    ``virial=True`` returns ``(energy, forces, virial)``: ``virial`` [3, 3] float64 ppm^2 on the device is ``-strain`` of
    ``GraphBatch.box_grad`` for the same edge gradient, the negative derivative of the energy with respect to a homogeneous
    strain of positions and box together, at fixed lists and images (its pressure contribution is trace / (3 V)).  One more
    library call, no torch autograd; energy and forces are bitwise those of ``virial=False``.  Without a box it is the
    same sum over the open-boundary edges.

    ``prune=True``: the forward and the backward run on the receptive field of the atoms with ``weights != 0`` alone
    (``GraphBatch.restrict``, DESIGN.md §7.17: the atoms within ``mp_layers`` list steps of them) and the edge gradient is
    expanded to the whole structure before the positions kernel.  The lists are still built for every atom.  Same
    shapes; energy, forces and virial are those of ``prune=False`` up to float32 summation order, the forces exactly 0.0
    on atoms outside the field.  One host synchronisation (the size of the field); all weights 0 raises ValueError.  The
    call to use when a few percent of the atoms carry a measured shift (a solute in explicit solvent)."""
    import torch
    from .graph import frames_to_batch
    if model.engine is None:
        model.build(int(np.asarray(atoms).shape[-1]) if not isinstance(atoms, torch.Tensor) else int(atoms.shape[-1]))
    eng = model.engine
    pos = positions.detach() if isinstance(positions, torch.Tensor) else positions
    box = box.detach() if isinstance(box, torch.Tensor) else box
    batch = frames_to_batch(atoms, pos, neighbor_number=neighbor_number, device=eng.device, box=box)
    if batch.G != 1:
        raise ValueError("shift_restraint: one structure [n, 3] at a time")
    y = torch.as_tensor(np.asarray(targets, np.float32) if not isinstance(targets, torch.Tensor) else targets,
                        dtype=torch.float32, device=eng.device).reshape(-1)
    w = torch.ones_like(y) if weights is None else torch.as_tensor(
        np.asarray(weights, np.float32) if not isinstance(weights, torch.Tensor) else weights,
        dtype=torch.float32, device=eng.device).reshape(-1)
    if y.shape[0] != batch.N or w.shape[0] != batch.N:
        raise ValueError(f"shift_restraint: targets / weights need {batch.N} entries")
    run = batch
    if prune:
        run = batch.restrict(w != 0, model.receptive_hops)
        keep = run.keep.to(torch.int64)
        y, w = y[keep], w[keep]
    peaks = eng.forward(run, training=False, keep_tape=True)
    diff = peaks - y
    energy = (diff * diff * w).sum()
    dpeaks = w * (2.0 * diff)              # d energy / d peaks, the bits torch autograd gives for the same expression
    dedges = torch.empty(run.edges.shape, dtype=torch.float32, device=eng.device)
    eng.backward(dpeaks, edge_grad=dedges)
    if prune:
        dedges = run.expand_edge_grad(dedges)
    forces = -batch.positions_grad(dedges)[0]
    if virial:
        return energy, forces, -batch.box_grad(dedges, want_dvec=False)[0][0]
    return energy, forces


def _position_sigma(position_sigma, n):
    """host check of a coordinate error (a scalar or [n] Angstrom, finite, >= 0): float32 [n]"""
    try:
        s = _host64(position_sigma)
    except (TypeError, ValueError):
        raise ValueError(f"shift_uncertainty: position_sigma must be a number or an [{n}] array, got {position_sigma!r}")
    if s.ndim == 0:
        s = np.full(n, float(s))
    if s.shape != (n,):
        raise ValueError(f"shift_uncertainty: position_sigma must be a scalar or [{n}], got {s.shape}")
    if not np.isfinite(s).all() or (s < 0).any():
        raise ValueError("shift_uncertainty: position_sigma must be finite and >= 0")
    return s.astype(np.float32)


def shift_uncertainty(model, atoms, positions, samples=32, position_sigma=None, neighbor_number=16, box=None, seed=0,
                      select=None):
    """``(mean, std_model, std_input)`` [n] in ppm, on the device: the predicted shifts of one structure with an error bar
    per atom.  ``std_model`` is the closed-form spread of the model's Dropout, ``std_input`` the sampled spread over
    ``samples`` perturbed inputs (``GNNModel.predict_uncertainty``); the two parts add in variance:

        total_std = sqrt(std_model**2 + std_input**2)
        restraint = ShiftRestraint(model, atoms, targets, tolerance=k * total_std)     # a flat bottom of k error bars

    ``atoms`` [n, C] one-hot, ``positions`` [n, 3] in Angstrom; the graph is the kNN graph of ``frames_to_batch`` with
    ``neighbor_number`` neighbours, in the periodic ``box`` if one is given.

    ``position_sigma=None``: the input part comes from the model's own GaussianNoise on the distances, at fixed neighbour
    lists — ``model.predict_uncertainty(frames_to_batch(atoms, positions), samples, seed)``.

    ``position_sigma``: a scalar or [n] coordinate error in Angstrom, finite and >= 0 (from a crystallographic B-factor:
    sqrt(B / (8 pi^2))).  The input part then comes from coordinate error instead: the S replicas are
    ``positions + sigma_i * xi`` with xi standard normal (``ng_randn(seed, offset 0)`` over [S, n, 3]), their neighbour lists
    are rebuilt per replica, and the model's distance noise is off.  A bad sigma raises ValueError before any device work.

    ``select``: a mask [n] or an index array — error bars for these atoms only.  The batch (or the batch of replicas) is
    restricted to their receptive field before the forward (``GraphBatch.restrict``); the outputs stay [n], NaN outside
    the selection.  The model's distance noise is then drawn over the restricted lists: the same distribution, not the
    same draws, as without ``select``."""
    import torch
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"shift_uncertainty: samples must be >= 1, got {samples}")
    shape = tuple(positions.shape) if hasattr(positions, "shape") else np.shape(positions)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"shift_uncertainty: one structure, positions [n, 3]; got {shape}")
    n = shape[0]
    sigma = None if position_sigma is None else _position_sigma(position_sigma, n)
    from .graph import frames_to_batch
    if model.engine is None:
        model.build(int(atoms.shape[-1]) if isinstance(atoms, torch.Tensor) else int(np.asarray(atoms).shape[-1]))
    eng = model.engine
    pos = positions.detach() if isinstance(positions, torch.Tensor) else torch.from_numpy(np.asarray(positions, np.float32))
    pos = pos.to(device=eng.device, dtype=torch.float32)
    box = box.detach() if isinstance(box, torch.Tensor) else box
    if sigma is None:
        batch = frames_to_batch(atoms, pos, neighbor_number=neighbor_number, device=eng.device, box=box)
        if select is None:
            return model.predict_uncertainty(batch, samples=samples, seed=seed)
        pruned = batch.restrict(select, model.receptive_hops)
        sel = pruned.selected
        return tuple(pruned.expand(t[sel], selected=True) for t in model.predict_uncertainty(pruned, samples=samples, seed=seed))
    xi = eng.randn(samples * n * 3, seed, 0).view(samples, n, 3)
    frames = pos[None] + torch.from_numpy(sigma).to(eng.device)[None, :, None] * xi
    batch = frames_to_batch(atoms, frames, neighbor_number=neighbor_number, device=eng.device, box=box)
    if select is not None:
        # the same atoms in every replica; each replica has a receptive field of its own (its lists were rebuilt)
        from .graph import selection_mask
        one = selection_mask(select, n, eng.device)
        pruned = batch.restrict(one.bool().repeat(samples), model.receptive_hops)
        sel = pruned.selected
        S_ = sel.shape[0] // samples
        mu, var = eng.forward_moments(pruned, seed=seed, noise=False)
        mean, var_in, var_model = eng.ensemble_moments(mu[sel].view(samples, S_).contiguous(), var[sel].view(samples, S_).contiguous())
        at = torch.nonzero(one).reshape(-1)
        out = torch.full((3, n), float("nan"), dtype=torch.float32, device=eng.device)
        out[:, at] = torch.stack([mean, torch.sqrt(var_model), torch.sqrt(var_in)])
        return out[0], out[1], out[2]
    mu, var = eng.forward_moments(batch, seed=seed, noise=False)
    mean, var_in, var_model = eng.ensemble_moments(mu.view(samples, n), var.view(samples, n))
    return mean, torch.sqrt(var_model), torch.sqrt(var_in)


def _is_trajectory(x):
    """a binary trajectory in one of the forms the consumers take: a path, a reader or a stream"""
    from .trajectory import TrajectoryStream, _Trajectory
    return isinstance(x, (str, os.PathLike, _Trajectory, TrajectoryStream))


def _trajectory_stream(x, chunk_frames, device):
    """the stream of a path or reader in chunks of ``chunk_frames`` on ``device``; a stream is taken as it is"""
    from .trajectory import TrajectoryStream
    return x if isinstance(x, TrajectoryStream) else TrajectoryStream(x, chunk_frames=chunk_frames, device=device)


def predict_trajectory(model, atoms, traj_or_stream, neighbor_number=16, pbc=False, select=None, frames_per_batch=32):
    """The predicted shifts of every frame of a binary trajectory, float32 [T, n] on the device.

    ``atoms`` [n, C] one-hot; ``traj_or_stream``: a path, a reader (``trajectory.open_trajectory``) or a
    ``trajectory.TrajectoryStream`` (its frames, stride and chunk size then hold; it must deliver all n atoms).  The frozen
    model runs over the chunks of the stream (``frames_per_batch`` frames each): one ``frames_to_batch`` and one model call per
    chunk, the positions decoded on the device (``ng_frames_decode``).  ``pbc``: minimum-image lists in every frame's box, from
    the file's cell data; a frame without one raises ValueError.  ``select``: a mask [n] or an index array — the model runs on
    the receptive field of these atoms alone (``GNNModel.predict_selected``) and the result is [T, n_sel], the selected atoms
    in ascending index."""
    import torch
    from .graph import frames_to_batch
    atoms_np = atoms.detach().cpu().numpy() if isinstance(atoms, torch.Tensor) else np.asarray(atoms)
    n = int(atoms_np.shape[0])
    mask = None
    if select is not None:
        s = np.asarray(select)
        mask = s.astype(bool) if s.dtype == bool else np.isin(np.arange(n), s.astype(np.int64))
        if mask.shape != (n,) or not mask.any():
            raise ValueError(f"predict_trajectory: select must name atoms in [0, {n})")
    if model.engine is None:
        model.build(int(atoms_np.shape[-1]))
    model.freeze()
    dev = model.engine.device
    stream = _trajectory_stream(traj_or_stream, max(1, int(frames_per_batch)), dev)
    if stream.n_out != n:
        raise ValueError(f"predict_trajectory: atoms has {n} rows but the trajectory delivers {stream.n_out} atoms")
    kept = []
    for ids, pos, dims in stream:
        box = None
        if pbc:
            if dims is None or np.isnan(dims).any():
                k = 0 if dims is None else int(np.argmax(np.isnan(dims).any(axis=1)))
                raise ValueError(f"predict_trajectory: pbc, but frame {int(ids[k])} has no box (no cell data, or zero lengths)")
            box = dims
        batch = frames_to_batch(atoms_np, pos, neighbor_number, device=dev, box=box)
        peaks = model(batch) if mask is None else model.predict_selected(batch, np.tile(mask, len(ids)))
        kept.append(peaks.detach().reshape(len(ids), -1))
    if not kept:
        return torch.empty((0, n if mask is None else int(mask.sum())), dtype=torch.float32, device=dev)
    return torch.cat(kept)


def reweight_trajectory(model, atoms, frames, targets, sigma, theta, prior=None, neighbor_number=16, box=None,
                        frames_per_batch=32, prune=False, **fit_args):
    """Maximum-entropy reweighting of the frames of a trajectory against measured shifts (nmrgnn_amd.reweight):
    ``(result, shifts)`` — a ``ReweightResult`` whose ``weights`` [T] make the ensemble agree with ``targets`` within
    ``sigma`` as far as ``theta`` allows, and the predicted shifts of every frame, float32 on the device.

    ``atoms`` [n, C] one-hot, ``frames`` [T, n, 3] in Angstrom — or a binary trajectory (a path, a reader of
    ``trajectory.open_trajectory`` or a ``trajectory.TrajectoryStream``: the same chunks, decoded on the device) —, ``targets`` [n] in ppm with NaN where an atom has no label,
    ``sigma`` a scalar or [n] (read on the labelled atoms only), ``theta`` > 0, ``prior`` [T] frame weights or None.  The
    frozen model runs over the frames ``frames_per_batch`` at a time, as ``eval-struct`` does (``box``: [6] for every frame or
    [T, 6]); the [T, n] shifts stay on the device, the labelled columns are gathered there, and ``ShiftReweighter.fit(theta,
    **fit_args)`` does the rest.  ``prune=True``: the model runs on the receptive field of the labelled atoms alone
    (``GNNModel.predict_selected``) and ``shifts`` is [T, M], the labelled atoms in ascending index.

    ``ValueError``: no labelled atom, or a labelled atom whose ``sigma`` is not finite and > 0."""
    import torch
    from .graph import frames_to_batch
    from .reweight import ShiftReweighter
    atoms_np = atoms.detach().cpu().numpy() if isinstance(atoms, torch.Tensor) else np.asarray(atoms)
    n = int(atoms_np.shape[0])
    y = _host64(targets).reshape(-1)
    if y.shape != (n,):
        raise ValueError(f"reweight_trajectory: targets need {n} entries, got {y.shape}")
    labelled = np.isfinite(y)
    if not labelled.any():
        raise ValueError("reweight_trajectory: no atom is labelled (targets are NaN everywhere)")
    sg = _host64(sigma)
    sg = np.full(n, float(sg)) if sg.ndim == 0 else sg.reshape(-1)
    if sg.shape != (n,):
        raise ValueError(f"reweight_trajectory: sigma must be a scalar or [{n}], got {sg.shape}")
    bad = labelled & ~(np.isfinite(sg) & (sg > 0))
    if bad.any():
        raise ValueError(f"reweight_trajectory: atom {int(np.nonzero(bad)[0][0])} is labelled but its sigma is not finite and > 0")
    step = max(1, int(frames_per_batch))
    binary = _is_trajectory(frames)
    if not binary:
        shape = tuple(frames.shape)
        if len(shape) != 3 or shape[1] != n or shape[2] != 3 or shape[0] < 1:
            raise ValueError(f"reweight_trajectory: frames must be [T, {n}, 3] with T >= 1, got {shape}")
    if model.engine is None:
        model.build(int(atoms_np.shape[-1]))
    model.freeze()
    dev = model.engine.device
    if binary:                      # a binary trajectory: the same chunks, decoded on the device
        stream = _trajectory_stream(frames, step, dev)
        if stream.n_out != n or len(stream.frame_ids) < 1:
            raise ValueError(f"reweight_trajectory: the trajectory must hold frames of {n} atoms, got {len(stream.frame_ids)} "
                             f"frames of {stream.n_out}")
        chunks = (pos for _, pos, _ in stream)
    else:
        chunks = (frames[b0:b0 + step] for b0 in range(0, shape[0], step))
    per_frame_box = box is not None and len(np.shape(box)) == 2
    kept = []
    b0 = -step
    for chunk in chunks:
        b0 += step
        G = int(chunk.shape[0])
        batch = frames_to_batch(atoms_np, chunk.detach() if isinstance(chunk, torch.Tensor) else chunk, neighbor_number,
                                device=dev, box=box[b0:b0 + step] if per_frame_box else box)
        peaks = model.predict_selected(batch, np.tile(labelled, G)) if prune else model(batch)
        kept.append(peaks.detach().reshape(G, -1))
    shifts = torch.cat(kept)
    idx = torch.from_numpy(np.nonzero(labelled)[0]).to(dev)
    S = shifts if prune else shifts.index_select(1, idx).contiguous()
    rw = ShiftReweighter(S, y[labelled], sg[labelled], prior=prior, device=dev)
    return rw.fit(theta, **fit_args), shifts


def _restraint_positions(positions, R, n):
    """host check of a call's positions: [R, n, 3] (or [n, 3] when R == 1); returns the torch view [R, n, 3] (not yet on the
    device) and whether the caller gave [n, 3]"""
    import torch
    shape = tuple(positions.shape) if hasattr(positions, "shape") else np.shape(positions)
    flat = len(shape) == 2
    if flat and R != 1:
        raise ValueError(f"ShiftRestraint: positions [n, 3] only for one replica; this restraint has {R}: pass [{R}, {n}, 3]")
    if (shape != (n, 3)) if flat else (shape != (R, n, 3)):
        raise ValueError(f"ShiftRestraint: positions must be [{R}, {n}, 3]" + (" (or [n, 3])" if R == 1 else "")
                         + f", got {shape}")
    p = positions.detach() if isinstance(positions, torch.Tensor) else torch.from_numpy(np.asarray(positions, np.float32))
    return p.reshape(R, n, 3), flat


def _restraint_box(box, R, triclinic=None):
    """host check of a box ([6] or [R, 6], pbc.prepare's refusals included): (vectors [R, 9] float32, triclinic flag).
    ``triclinic``: the kind the restraint was built for (the displacement policy of its captured kernels)."""
    from .pbc import prepare
    import torch
    if isinstance(box, torch.Tensor):
        box = box.detach().cpu().numpy()
    vecs, tric, _ = prepare(box, R)
    if triclinic is not None and bool(tric) != bool(triclinic):
        want, got = ("triclinic", "orthorhombic") if triclinic else ("orthorhombic", "triclinic")
        raise ValueError(f"ShiftRestraint: built for a {want} box, called with a {got} one (the kind of box is fixed at "
                         "construction)")
    return vecs, bool(tric)


def _host64(x):
    import torch
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64)


def _restraint_tolerance(tolerance, n):
    """host check of a flat-bottom tolerance (a scalar or [n] ppm, finite, >= 0): float32 [n]"""
    t = _host64(tolerance)
    if t.ndim == 0:
        t = np.full(n, float(t))
    if t.shape != (n,):
        raise ValueError(f"ShiftRestraint: tolerance must be a scalar or [{n}], got {t.shape}")
    if not np.isfinite(t).all() or (t < 0).any():
        raise ValueError("ShiftRestraint: tolerance must be finite and >= 0")
    return t.astype(np.float32)


def _restraint_replica_weights(c, R):
    """host check of replica weights ([R], finite, >= 0, positive sum): normalised in float64, then float32 [R]"""
    c = _host64(c)
    if c.shape != (R,):
        raise ValueError(f"ShiftRestraint: replica_weights must be [{R}], got {c.shape}")
    if not np.isfinite(c).all() or (c < 0).any() or not c.sum() > 0:
        raise ValueError("ShiftRestraint: replica_weights must be finite, >= 0, with a positive sum")
    return (c / c.sum()).astype(np.float32)


def _restraint_lambda(tau):
    """host check of a memory time tau (calls, finite, > 0): lambda = float32(exp(-1 / tau)), below 1 in float32"""
    try:
        t = float(tau)
    except (TypeError, ValueError):
        t = float("nan")
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"ShiftRestraint: tau must be a finite number of calls > 0, got {tau!r}")
    lam = np.float32(np.exp(-1.0 / t))
    if not lam < 1:
        raise ValueError(f"ShiftRestraint: tau = {tau!r} gives lambda = 1 in float32 (a memory that never forgets)")
    return float(lam)


class ShiftRestraint:
    """Replica-averaged chemical-shift restraint of ``replicas`` structures of one topology, for an MD engine that asks for
    forces every step:

        energy = sum_i w_i (mean_r delta_pred[r, i] - delta_exp_i)^2     ppm^2, a 0-d float32 device tensor
        forces = -d energy / d positions                                 ppm^2 / Angstrom, [R, n, 3] ([n, 3] given [n, 3])
        virial = -strain per replica (``virial=True``)                   [R, 3, 3] float64, as shift_restraint defines it

    ``r(positions)`` / ``r(positions, box=...)`` with positions [R, n, 3] in Angstrom (or [n, 3] when R == 1) and, for a
    restraint built with a box, the box of this call ([6] or [R, 6], the same kind — orthorhombic or triclinic — as at
    construction).  Returns ``(energy, forces)`` or ``(energy, forces, virial)``.  Everything is taken at FIXED neighbour
    lists, as shift_restraint: the kNN lists of every call's positions (and box), held fixed for the derivative.

    The chain — kNN lists of the R frames (ng_knn_graph / _pbc), the inference forward with a tape, ng_restraint_loss,
    ``Engine.backward(param_grad=False, edge_grad=...)``, ng_positions_grad (/ _pbc) and, with ``virial``, ng_box_grad — is
    captured ONCE as a HIP graph at construction; a call stages the positions (and box vectors) into static device buffers
    (one ng_replay_stage) and replays it.  The outputs are static buffers: read them before the next call.  With R = 1 the
    forces and the virial are bitwise those of ``shift_restraint`` (the energy is summed in another order: float64 here).
    ``replay=False`` runs the same chain eagerly (the reference of the tests and the debugging path).

    Restraint forms (ng_restraint_loss_ex); with all four at their defaults the chain is the one above:
      ``tolerance``        a scalar or [n] ppm (finite, >= 0): flat bottom, no energy and no force while
                           |value - delta_exp_i| <= tol_i, and (|value - delta_exp_i| - tol_i)^2 outside
      ``replica_weights``  [R] (finite, >= 0, positive sum; normalised in float64, then float32): the weighted mean
                           sum_r c_r delta_pred[r, i] instead of the uniform one.  ``r(positions, replica_weights=...)``
                           replaces them for this call and the next ones (staged with the positions)
      ``independent``      one energy per replica, ``r.energies`` [R] float64 on the device; ``energy`` is their sum and
                           the forces on replica r are -dE_r / dpos_r
      ``tau``              a running average over calls with memory tau (calls): a = lambda a_prev + (1 - lambda) value,
                           lambda = float32(exp(-1 / tau)), restrained in place of the value; the forces are the derivative
                           of this call's energy with the earlier average held fixed, (1 - lambda) times those of the
                           instantaneous restraint after the first call.  ``r.reset()`` forgets the average.
    ``r.energies`` is [1] (the energy in float64) without ``independent``.

    Refused with ValueError before any device work: wrong shapes, a box where none was given at construction or none where
    one was, a box of the other kind or one pbc.prepare refuses, and a call after the model's weights changed (a training
    step, a load): the captured chain would read stale packed weights — build a new restraint.  Also bad tolerances, replica
    weights or tau, ``replica_weights`` with ``independent``, and ``replica_weights`` at a call for a restraint built without
    them or with R = 1.  The call leaves ``engine.params.grad`` alone."""

    def __init__(self, model, atoms, targets, weights=None, replicas=1, neighbor_number=16, box=None, virial=False,
                 replay=True, tolerance=None, replica_weights=None, independent=False, tau=None):
        import torch
        from .geometry import OPEN_BOUNDARY, UNIFORM, Boundary, Layout
        R = int(replicas)
        if R < 1 or R != replicas:
            raise ValueError(f"ShiftRestraint: replicas must be a positive integer, got {replicas!r}")
        if replica_weights is not None and independent:
            raise ValueError("ShiftRestraint: replica_weights average the replicas; independent replicas have none")
        a_shape = tuple(atoms.shape) if hasattr(atoms, "shape") else np.shape(atoms)
        if len(a_shape) != 2 or a_shape[0] < 1:
            raise ValueError(f"ShiftRestraint: atoms must be [n, C] one-hot, got {a_shape}")
        n = int(a_shape[0])
        K = int(neighbor_number)
        if K < 1:
            raise ValueError("ShiftRestraint: neighbor_number must be >= 1")
        host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        y = np.asarray(host(targets), np.float32).reshape(-1)
        w = np.ones(n, np.float32) if weights is None else np.asarray(host(weights), np.float32).reshape(-1)
        if y.shape[0] != n or w.shape[0] != n:
            raise ValueError(f"ShiftRestraint: targets and weights need {n} entries (one per atom)")
        tol = None if tolerance is None else _restraint_tolerance(tolerance, n)
        c = None if replica_weights is None else _restraint_replica_weights(replica_weights, R)
        lam = 0.0 if tau is None else _restraint_lambda(tau)
        self.R, self.n, self.K = R, n, K
        self.virial = bool(virial)
        self.replay = bool(replay)
        self.independent = bool(independent)
        self.tau, self._lam = tau, lam
        # the forms go through ng_restraint_loss_ex; with none of them set the chain keeps ng_restraint_loss, launch for launch
        self._ex = tol is not None or c is not None or self.independent or tau is not None
        vecs, self._tric = (None, None) if box is None else _restraint_box(box, R)
        # ---- device side
        if model.engine is None:
            model.build(int(a_shape[1]))
        eng = self.eng = model.engine
        dev = eng.device
        self._wgen = eng._wgen
        at = (atoms.detach() if isinstance(atoms, torch.Tensor) else torch.from_numpy(np.asarray(atoms, np.float32)))
        at = at.to(device=dev, dtype=torch.float32).contiguous()
        self.s_atoms = at.repeat(R, 1).contiguous() if R > 1 else at
        self.s_y = torch.from_numpy(y).to(dev)
        self.s_w = torch.from_numpy(w).to(dev)
        self.s_pos = torch.zeros(R, n, 3, dtype=torch.float32, device=dev)
        self.s_box = None if vecs is None else torch.from_numpy(vecs).to(dev)
        self._boundary = OPEN_BOUNDARY if vecs is None else Boundary(UNIFORM, self.s_box, bool(self._tric))
        self._layout = Layout.frames(R, n)
        self._nlist = torch.empty(R * n, K, dtype=torch.int32, device=dev)
        self._edges = torch.empty(R * n, K, dtype=torch.float32, device=dev)
        self._inv = torch.empty(R * n, dtype=torch.float32, device=dev)
        G = R if self.independent else 1
        self._e64 = torch.zeros(G, dtype=torch.float64, device=dev)
        self.energies = self._e64
        self.s_tol = None if tol is None else torch.from_numpy(tol).to(dev)
        self.s_c = None if c is None else torch.from_numpy(c).to(dev)
        self._avg = torch.zeros(G * n, dtype=torch.float32, device=dev) if lam > 0 else None
        self._primed = torch.zeros(1, dtype=torch.int32, device=dev) if lam > 0 else None
        self.energy = torch.zeros((), dtype=torch.float32, device=dev)
        self.forces = torch.zeros(R, n, 3, dtype=torch.float32, device=dev)
        self.virial_out = torch.zeros(R, 3, 3, dtype=torch.float64, device=dev) if self.virial else None
        # ADVICE (edge path of warm-up vs capture): the host-guarded edge-function table ("table_host", edge shapes without the
        # fused kernels on >= edge_table_min_edges slots) reads its guard on the host, which a capture cannot, so a captured
        # call would go per edge while its eager warm-up took the table — a chain the warm-up never sized.  Every call of
        # this restraint, eager or replayed, takes the per-edge path there; the device-guarded table is capturable and kept.
        from .engine import edge_path
        live_k = bool(eng.lib.ng_edge_live_supported(eng.H, eng.E, eng.Le, eng.fc_act))
        self._no_table = edge_path(eng.edge_table, eng.use_live_edges, live_k, eng.E, R * n * K, eng.edge_table_min_edges,
                                   False, False) == "table_host"
        self._graph = None
        if self.replay:
            self._capture()

    # ------------------------------------------------------------------ the chain
    def _chain(self):
        """one call on the static buffers: every launch reads s_pos / s_box and writes energy / forces / virial_out"""
        import ctypes as C
        import torch
        from ._lib import ptr
        from .graph import batch_from_positions
        eng = self.eng
        lib, h = eng.lib, eng.ctx.handle
        st = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
        R, n = self.R, self.n
        # the builders' own path on the static buffers, no allocation, copy or host read of its own; the captured chain reads
        # buffers the batch owns
        self._batch = b = batch_from_positions(self.s_atoms, self.s_pos, self._layout, 0.1, self._boundary, self.K,
                                               out=(self._nlist, self._edges, self._inv))
        keep = eng.edge_table
        if self._no_table:
            eng.edge_table = False
        try:
            peaks = eng.forward(b, training=False, keep_tape=True)
        finally:
            eng.edge_table = keep
        dpeaks = torch.empty_like(peaks)
        if self._ex:
            eng._ck(lib.ng_restraint_loss_ex(h, st, R, n, 1 if self.independent else 0, ptr(peaks), ptr(self.s_y), ptr(self.s_w),
                                             ptr(self.s_c), ptr(self.s_tol), self._lam, ptr(self._avg), ptr(self._primed),
                                             ptr(self._e64), ptr(dpeaks)), "ng_restraint_loss_ex")
        else:
            eng._ck(lib.ng_restraint_loss(h, st, R, n, ptr(peaks), ptr(self.s_y), ptr(self.s_w), ptr(self._e64), ptr(dpeaks)),
                    "ng_restraint_loss")
        self.energy.copy_(self._e64.sum() if self.independent else self._e64[0])
        dedges = torch.empty_like(self._edges)
        eng.backward(dpeaks, edge_grad=dedges, param_grad=False)
        torch.neg(b.positions_grad(dedges), out=self.forces)
        if self.virial:
            torch.neg(b.box_grad(dedges, want_dvec=False)[0], out=self.virial_out)

    def _capture(self):
        import torch
        eng = self.eng
        self._stream = torch.cuda.Stream(device=eng.device)
        self._graph = torch.cuda.CUDAGraph()
        cur = torch.cuda.current_stream(eng.device)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            # two eager warm-up calls on the capture stream size every scratch buffer and fill the caches the chain relies on
            # (the batch's device graph_ptr, the context's workspace); they take the same edge path as the capture
            for _ in range(2):
                self._chain()
            torch.cuda.synchronize(eng.device)
            with torch.cuda.graph(self._graph, stream=self._stream):
                self._chain()
        cur.wait_stream(self._stream)
        if self._primed is not None:
            self.reset()            # the warm-up calls ran the running average: the first call starts it afresh

    def reset(self):
        """forget the running average (``tau``): the next call restrains its own shifts and starts the average from them.
        An ordinary write on the current stream, between calls; a no-op without ``tau``."""
        if self._primed is not None:
            self._primed.zero_()

    # ------------------------------------------------------------------ calls
    def _call_weights(self, replica_weights):
        """host check of a call's replica_weights: None (keep the staged ones) or float32 [R]"""
        if replica_weights is None:
            return None
        if self.R == 1:
            raise ValueError("ShiftRestraint: replica_weights at a call need more than one replica")
        if self.s_c is None:
            raise ValueError("ShiftRestraint: built without replica_weights (the chain reads none); pass them at construction")
        return _restraint_replica_weights(replica_weights, self.R)

    def check(self, positions, box=None, replica_weights=None):
        """the host-side refusals of a call (ValueError), without device work; returns (positions [R, n, 3], box vectors or
        None, whether positions were [n, 3])"""
        self._call_weights(replica_weights)
        pos, flat = _restraint_positions(positions, self.R, self.n)
        if (box is None) != (self._tric is None):
            raise ValueError("ShiftRestraint: built without a box, called with one" if box is not None else
                             "ShiftRestraint: built with a box, called without one (pass the box of this call)")
        vecs = None if box is None else _restraint_box(box, self.R, self._tric)[0]
        if self.eng._wgen != self._wgen:
            raise ValueError("ShiftRestraint: the model's weights changed since the restraint was built (a training step or "
                             "a load); build a new ShiftRestraint")
        return pos, vecs, flat

    def __call__(self, positions, box=None, replica_weights=None):
        import torch
        from .replay import _stage
        c = self._call_weights(replica_weights)
        pos, vecs, flat = self.check(positions, box)
        eng = self.eng
        p = pos.to(device=eng.device, dtype=torch.float32).contiguous()
        pairs = [(p, self.s_pos)]
        if vecs is not None:
            pairs.append((torch.from_numpy(vecs).to(eng.device), self.s_box))
        if c is not None:
            pairs.append((torch.from_numpy(c).to(eng.device), self.s_c))
        _stage(eng, 0, 1e-4, 1, pairs)
        if self._graph is not None:
            self._graph.replay()
        else:
            self._chain()
        forces = self.forces[0] if flat else self.forces
        if self.virial:
            return self.energy, forces, self.virial_out
        return self.energy, forces
