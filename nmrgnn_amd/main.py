"""Command line of the hot path's caller: ``eval-struct`` (nmrgnn/main.py:192-278) and ``train`` (nmrgnn/main.py:36-90).

Same arguments, options, CSV columns and per-phase timing line as the reference command.  Frames
of a trajectory are independent graphs, so they are concatenated ``--frames-per-batch`` at a time into
one device batch (one launch sequence per batch instead of one per frame) and their neighbour lists
are built on the GPU (ng_knn_graph); the reference evaluates frame by frame with a CPU neighbour search.  With
``--separate`` every file is a structure of its own, batched as a ragged batch (graph.structures_to_batch).
The first file is a PDB; the files behind it are further PDB pieces, or binary trajectories (``.dcd``, ``.nc``, ``.ncdf``:
nmrgnn_amd.trajectory) — then, as with ``md.Universe(topology, *trajectory)``, the PDB gives the names only and
the frames are those of the trajectory files in order, decoded on the device.

``train RECORDS... NAME [EPOCHS]`` is the reference's training command on ``dataset.ShiftDataset`` files (``.npz``, written by
``ShiftDataset.save``; the package reads no TFRecords): ``GNNModel.fit`` with the reference's callbacks, the model saved to
NAME and the history pickled beside it.  ``make-records OUT.npz --pair STRUCT SHIFTS ...`` writes such a file from structures
and CSV tables of assigned shifts (``ShiftDataset.from_structures``).  ``eval-records RECORDS... --embeddings
FILE`` is the reference's ``eval-tfrecords`` (nmrgnn/main.py:93-189) on such files: the CSV of every labelled atom and the
markdown table of r and squared error per element and atom name (``GNNModel.evaluate_report``).  Out of
scope: ``--tensorboard`` and ``hyper`` (the hyper-parameter search)."""
from __future__ import annotations

import csv
import os
import sys
import time

import click
import numpy as np


@click.group()
def main():
    pass


def _open_structure(struct_files):
    from .structure import Structure, read_pdb
    from .trajectory import TrajectoryUniverse, is_trajectory_file
    if is_trajectory_file(struct_files[0]):
        raise ValueError(f"{struct_files[0]}: the first file is the topology and must be a PDB; trajectory files follow it")
    first = read_pdb(struct_files[0])
    binary = [f for f in struct_files[1:] if is_trajectory_file(f)]
    if binary:
        # md.Universe(topology, *trajectory files): the topology gives the names, the trajectory files every frame
        if len(binary) != len(struct_files) - 1:
            other = [f for f in struct_files[1:] if not is_trajectory_file(f)]
            raise ValueError(f"PDB and binary trajectory files cannot be mixed behind the topology {struct_files[0]}: "
                             f"{other[0]} is no .dcd, .nc or .ncdf file, {binary[0]} is one")
        return TrajectoryUniverse(first, binary, label=struct_files[0])
    frames, dims = list(first.frames), list(first.dimensions)
    for extra in struct_files[1:]:                  # md.Universe(topology, *trajectory pieces)
        s = read_pdb(extra)
        if s.n_atoms != first.n_atoms:
            raise ValueError(f"{extra}: {s.n_atoms} atoms, but {struct_files[0]} has {first.n_atoms}")
        frames.extend(s.frames)
        dims.extend(s.dimensions)
    return Structure(first.names, first.resnames, first.resids, first.elements, frames, dims)


def eval_structure(struct_files, output_csv, model_file=None, neighbor_number=16, stride=1,
                   frames_per_batch=32, keep_going=False, device=None, echo=print, pbc=False, separate=False, boxes=False,
                   uncertainty=0, position_sigma=None, average=False, atom_names=None, reweight=None, theta=None, sigma=None):
    """Predict shifts for every ``stride``-th frame and write the reference's CSV.  Returns the timing
    buckets in seconds.  ``pbc``: neighbour lists under the minimum-image convention in each frame's box (its CRYST1
    record); a frame without one is an error.  ``separate``: every file is a structure of its own (see
    :func:`_eval_separate`); with ``boxes`` every (file, frame) structure uses its own CRYST1 box when it has one and open
    boundaries otherwise.

    ``struct_files``: a PDB, then more PDB pieces of the same atoms or binary trajectory files (DCD, Amber NetCDF-3; not both
    kinds).  With binary files the PDB contributes the atoms only, the frames are the trajectory files' in order, every file
    must have the PDB's atom count, ``pbc`` takes the boxes from the cell records, and ``separate`` is refused.  The frames
    reach the loop below through one frame source either way (``trajectory.frame_source``), ``frames_per_batch`` at a time, so
    a binary trajectory gives the batches, and the CSV, of the same frames as a PDB.

    ``uncertainty`` = S > 0: two more columns behind ``frame``, ``std_model`` and ``std_input`` in ppm, rounded like
    ``peaks``: the error bar of every shift from S replicas of its frame (library.shift_uncertainty, seeded with the frame
    number; total = sqrt(std_model^2 + std_input^2)).  ``position_sigma`` (Angstrom): the input part from a coordinate error
    of that size instead of the model's distance noise.  ``average``: ONE row per atom over the frames read — ``index,
    residues, resids, names, peaks`` (the mean over the frames), ``peaks_std`` (the sample standard deviation over the
    frames, n - 1 in the denominator; 0 for one frame), ``confident`` (of the mean), ``frames`` (how many were read); the
    moments are taken on the device (ng_ensemble_moments).  Without these options the CSV is what it always was.

    ``atom_names``: a sequence of PDB atom names (exact match) — rows for these atoms only, with their original ``index``;
    the model runs on their receptive field alone (GNNModel.predict_selected) and ``check_peaks`` on them.  Names that match
    no atom raise AtomNamesError.

    ``reweight``: a CSV of assigned shifts (``structure.read_shift_table``; an optional ``error`` column in ppm) — maximum-
    entropy reweighting of the frames read against it (nmrgnn_amd.reweight) at the strength ``theta``, with
    the errors ``sigma`` (a number, ``'H=0.3,C=1.1'`` or what ``reweight.parse_sigma`` returns; a finite ``error`` of the
    table wins for its row).  ONE row per atom: ``index, residues, resids, names, peaks`` (the weighted mean), ``peaks_std``
    (the weighted standard deviation; both from ng_weighted_moments), ``confident`` (of the weighted mean), ``frames``,
    ``peaks_prior`` (the unweighted mean, that of ``average``), ``target``, ``sigma`` (blank without a label); the frame
    weights go to ``<output stem>.weights.csv`` (``frame, weight``).  With ``atom_names`` the observables are the labelled
    atoms among the selected ones.  ReweightUsageError: no ``theta``, a labelled atom without a sigma, no labelled atom left,
    or a combination with ``separate``, ``uncertainty`` or ``average``."""
    if reweight is not None:
        if separate or uncertainty or average:
            raise ReweightUsageError('--reweight cannot be combined with --separate, --uncertainty or --average')
        if theta is None:
            raise ReweightUsageError('--reweight needs --theta X (the regularisation strength, > 0)')
        if not (float(theta) > 0 and np.isfinite(float(theta))):
            raise ReweightUsageError(f'--theta must be finite and > 0, got {theta}')
        if sigma is None:
            raise ReweightUsageError('--reweight needs --sigma SPEC: there is no default error')
    elif theta is not None or sigma is not None:
        raise ReweightUsageError('--theta and --sigma go with --reweight TABLE')
    if len(struct_files) == 0:
        raise ValueError('Must pass at least on structure file')
    uncertainty = int(uncertainty or 0)
    if uncertainty < 0:
        raise ValueError('--uncertainty takes a number of replicas >= 1')
    if separate and (uncertainty or average):
        raise ValueError('--separate cannot be combined with --uncertainty or --average: the files are different topologies, '
                         'and both options work on the frames of one')
    if position_sigma is not None and not uncertainty:
        raise ValueError('--position-sigma goes with --uncertainty S')
    if average and uncertainty:
        raise ValueError('--average and --uncertainty cannot be combined: run them one after the other')
    if separate and pbc:
        raise ValueError('--separate and --pbc cannot be combined: --pbc wants a box on every frame of one topology; '
                         'use --separate --boxes for one box, or none, per structure')
    if boxes and not separate:
        raise ValueError('--boxes goes with --separate (one box, or none, per structure); use --pbc for frames of one topology')
    if separate:
        from .trajectory import is_trajectory_file
        if any(is_trajectory_file(f) for f in struct_files):
            raise ValueError('--separate takes PDB files, each a structure of its own; a binary trajectory (.dcd, .nc, .ncdf) '
                             'holds frames of the topology in front of it: run it without --separate')
        return _eval_separate(struct_files, output_csv, model_file, neighbor_number, stride, frames_per_batch, keep_going,
                              device, echo, boxes, atom_names)
    import torch
    from .graph import frames_to_batch
    from .library import check_peaks, load_model, shift_uncertainty
    from .structure import atoms_onehot
    from .trajectory import frame_source

    model = load_model(model_file, device=device)
    u = _open_structure(struct_files)
    source = frame_source(u)        # host frames of a PDB, or binary trajectory files decoded on the device
    frame_ids = list(range(0, len(u), stride))
    if pbc:
        missing = [fr for fr, box in zip(frame_ids, source.boxes(frame_ids)) if box is None]
        if missing:
            raise ValueError(f"--pbc: frame {missing[0]} has no box (no CRYST1 record, or the 1 Angstrom placeholder; in a "
                             "binary trajectory: no cell record, or one with zero lengths)")
    atoms = atoms_onehot(u.elements)
    n = atoms.shape[0]
    select = _name_mask(u.names, atom_names)        # None: every atom
    idx = np.arange(n) if select is None else np.nonzero(select)[0]
    if select is not None:
        if len(idx) == 0:
            raise AtomNamesError(f"--atom-names {','.join(atom_names)}: no atom of {', '.join(struct_files)} has one of these names")
        atoms_all, atoms, n = atoms, atoms[idx], len(idx)      # what follows the model call sees the selected atoms only
    else:
        atoms_all = atoms
    rw_target = rw_sigma = None
    if reweight is not None:
        rw_target, rw_sigma = _reweight_labels(u, reweight, sigma, select)
    model.build(atoms.shape[1])
    model.freeze()          # inference only: the engine keeps its packed weight images across the per-frame calls
    timing = {'Structure': 0.0, 'Model Inference (MI355X)': 0.0, 'Parsing': 0.0}
    rows = []
    kept = []               # --average: the [frames, n] peaks stay on the device
    step = max(1, frames_per_batch)
    chunks = source.chunks([frame_ids[b0:b0 + step] for b0 in range(0, len(frame_ids), step)], device=model.engine.device)
    while True:
        t = time.perf_counter()
        taken = next(chunks, None)          # (frame numbers, positions [G, n, 3] on the host or the device, boxes)
        if taken is None:
            break
        chunk, positions, chunk_boxes = taken
        model.build(atoms.shape[1])
        dev = model.engine.device
        box = np.stack(chunk_boxes) if pbc else None
        batch = frames_to_batch(atoms_all, positions, neighbor_number, device=dev, box=box)
        torch.cuda.synchronize(dev)
        timing['Structure'] += time.perf_counter() - t
        t = time.perf_counter()
        peaks = model(batch) if select is None else model.predict_selected(batch, np.tile(select, len(chunk)))
        if average or reweight is not None:
            kept.append(peaks.reshape(len(chunk), n))
            timing['Model Inference (MI355X)'] += time.perf_counter() - t
            echo('|'.join(f'{k}:{v:5.2f}s' for k, v in timing.items()))
            continue
        peaks = peaks.cpu().numpy()
        peaks = peaks.reshape(len(chunk), n)
        stds = []
        for k, fr in (enumerate(chunk) if uncertainty else ()):
            _, sm, si = shift_uncertainty(model, atoms_all, positions[k], samples=uncertainty, position_sigma=position_sigma,
                                          neighbor_number=neighbor_number, box=chunk_boxes[k] if pbc else None, seed=fr,
                                          select=select)
            if select is not None:
                sm, si = sm[idx], si[idx]
            stds.append((np.round(sm.cpu().numpy().astype(np.float64), 2), np.round(si.cpu().numpy().astype(np.float64), 2)))
        conf = []
        for k in range(len(chunk)):
            try:
                conf.append(check_peaks(atoms, peaks[k]))
            except Warning as w:
                if not keep_going:
                    raise
                echo(f'frame {chunk[k]}: {w}')
                conf.append(np.zeros(n, dtype=bool))
        timing['Model Inference (MI355X)'] += time.perf_counter() - t
        t = time.perf_counter()
        for k, fr in enumerate(chunk):
            pk = np.round(peaks[k].astype(np.float64), 2)
            for j, i in enumerate(idx):
                row = (int(i), u.resnames[i], int(u.resids[i]), u.names[i], pk[j], bool(conf[k][j]), float(fr), fr)
                rows.append(row + (stds[k][0][j], stds[k][1][j]) if uncertainty else row)
        timing['Parsing'] += time.perf_counter() - t
        echo('|'.join(f'{k}:{v:5.2f}s' for k, v in timing.items()))
    header = ['index', 'residues', 'resids', 'names', 'peaks', 'confident', 'time', 'frame']
    if uncertainty:
        header += ['std_model', 'std_input']
    if average:
        t = time.perf_counter()
        mean, var, _ = model.engine.ensemble_moments(torch.cat(kept))
        pk = np.round(mean.cpu().numpy().astype(np.float64), 2)
        sd = np.round(torch.sqrt(var).cpu().numpy().astype(np.float64), 2)
        try:
            conf = check_peaks(atoms, mean.cpu().numpy())
        except Warning as w:
            if not keep_going:
                raise
            echo(f'mean over {len(frame_ids)} frames: {w}')
            conf = np.zeros(n, dtype=bool)
        rows = [(int(i), u.resnames[i], int(u.resids[i]), u.names[i], pk[j], sd[j], bool(conf[j]), len(frame_ids))
                for j, i in enumerate(idx)]
        header = ['index', 'residues', 'resids', 'names', 'peaks', 'peaks_std', 'confident', 'frames']
        timing['Parsing'] += time.perf_counter() - t
    if reweight is not None:
        from .reweight import ShiftReweighter, weighted_moments, write_reweight_csv, write_weights_csv
        t = time.perf_counter()
        shifts = torch.cat(kept)                            # [frames, n] on the device
        cols = np.nonzero(np.isfinite(rw_target[idx]))[0]   # the labelled atoms among the rows
        S = shifts.index_select(1, torch.from_numpy(cols).to(shifts.device)).contiguous()
        res = ShiftReweighter(S, rw_target[idx][cols], rw_sigma[idx][cols]).fit(float(theta))
        mean, var = weighted_moments(shifts, res.weights)
        prior_mean = model.engine.ensemble_moments(shifts)[0]
        timing['Model Inference (MI355X)'] += time.perf_counter() - t
        t = time.perf_counter()
        mean = mean.cpu().numpy()
        try:
            conf = check_peaks(atoms, mean)
        except Warning as w:
            if not keep_going:
                raise
            echo(f'weighted mean over {len(frame_ids)} frames: {w}')
            conf = np.zeros(n, dtype=bool)
        write_reweight_csv(output_csv, idx, [u.resnames[i] for i in idx], [u.resids[i] for i in idx], [u.names[i] for i in idx],
                           mean, torch.sqrt(var).cpu().numpy(), conf, len(frame_ids), prior_mean.cpu().numpy(),
                           rw_target[idx], rw_sigma[idx])
        weights_csv = os.path.splitext(output_csv)[0] + '.weights.csv'
        write_weights_csv(weights_csv, res.weights)
        timing['Parsing'] += time.perf_counter() - t
        echo(f'reweighted {len(frame_ids)} frames on {len(cols)} shifts: theta {float(theta):g}, phi_eff {res.phi_eff:.4f}, '
             f'chi2 {res.chi2_prior:.4f} -> {res.chi2_post:.4f}, {res.evaluations} evaluations, '
             f"{'converged' if res.converged else 'NOT converged'}")
        echo(f'You can now find your result in {output_csv} and the frame weights in {weights_csv}')
        return timing
    os.makedirs(os.path.dirname(os.path.abspath(output_csv)), exist_ok=True)
    with open(output_csv, 'w', newline='') as f:
        wr = csv.writer(f)
        wr.writerow(header)
        wr.writerows(rows)
    echo(f'You can now find your result in {output_csv}')
    return timing


class ReweightUsageError(ValueError):
    """--reweight used wrongly: the command line reports it as a usage error"""


def _reweight_labels(u, table_file, sigma, select):
    """``(target, sigma)`` float64 [n] of ``eval-struct --reweight``: the table's shifts laid on the atoms of ``u`` (NaN: no
    label; with ``select`` the labels outside it are dropped) and the error of every labelled atom — the table's ``error``
    where finite, else ``sigma`` (a number, a SPEC string or a parsed dict).  ReweightUsageError where no labelled atom is
    left or one has no error."""
    from .reweight import atom_sigma, parse_sigma, read_shift_errors
    from .structure import join_shifts, read_shift_table
    table = read_shift_table(table_file)
    target = join_shifts(u, table, label=str(table_file))[0].astype(np.float64)
    errors = read_shift_errors(table_file)
    err_atoms = join_shifts(u, dict(table, shift=errors.astype(np.float32)), strict=False)[0].astype(np.float64)
    if select is not None:
        target[~select] = np.nan
    labelled = np.isfinite(target)
    if not labelled.any():
        raise ReweightUsageError(f'--reweight {table_file}: no labelled atom' + (' among the selected atoms' if select is not None else ''))
    try:
        spec = parse_sigma(sigma) if isinstance(sigma, str) else sigma
    except ValueError as e:
        raise ReweightUsageError(str(e)) from None
    sig = atom_sigma(u.elements, labelled, spec, err_atoms)
    missing = np.nonzero(labelled & ~np.isfinite(sig))[0]
    if len(missing):
        i = int(missing[0])
        raise ReweightUsageError(f'--sigma: the labelled atom {u.resnames[i]} {int(u.resids[i])} {u.names[i]} (element '
                                 f'{u.elements[i]}) has no sigma; give one number, or a value for every labelled element')
    return target, sig


class AtomNamesError(ValueError):
    """--atom-names matched no atom: the command line reports it as a message"""


def _name_mask(names, atom_names):
    """bool [n]: the atoms whose PDB name is one of ``atom_names`` (exact match); None without a name list"""
    if atom_names is None:
        return None
    want = {a.strip() for a in atom_names if a.strip()}
    return np.array([str(nm).strip() in want for nm in names], dtype=bool)


def _eval_separate(struct_files, output_csv, model_file, neighbor_number, stride, frames_per_batch, keep_going, device, echo,
                   boxes=False, atom_names=None):
    """``eval-struct --separate``: every file is a structure of its own, with all of its MODEL frames (every ``stride``-th,
    counted per file).  The structure-frames of all files go ``frames_per_batch`` at a time into one ragged device batch
    (graph.structures_to_batch); the CSV has a leading ``file`` column (the path as given), then the reference's.  ``boxes``:
    minimum-image lists in the CRYST1 box of every structure-frame that has one, open boundaries for the others."""
    import torch
    from .graph import structures_to_batch
    from .library import check_peaks, load_model
    from .structure import atoms_onehot, read_pdb

    model = load_model(model_file, device=device)
    timing = {'Structure': 0.0, 'Model Inference (MI355X)': 0.0, 'Parsing': 0.0}
    t = time.perf_counter()
    structs = [read_pdb(f) for f in struct_files]
    atoms = [atoms_onehot(s.elements) for s in structs]
    items = [(k, fr) for k, s in enumerate(structs) for fr in range(0, len(s), stride)]     # (file, frame)
    masks = [_name_mask(s.names, atom_names) for s in structs]      # None: every atom
    if atom_names is not None:
        if not any(m.any() for m in masks):
            raise AtomNamesError(f"--atom-names {','.join(atom_names)}: no atom of {', '.join(struct_files)} has one of these names")
        items = [(k, fr) for k, fr in items if masks[k].any()]      # a structure without a match gives no rows
    index = [np.arange(s.n_atoms) if m is None else np.nonzero(m)[0] for s, m in zip(structs, masks)]
    timing['Structure'] += time.perf_counter() - t
    model.build(atoms[0].shape[1])
    model.freeze()
    rows = []
    for b0 in range(0, len(items), max(1, frames_per_batch)):
        chunk = items[b0:b0 + max(1, frames_per_batch)]
        t = time.perf_counter()
        dev = model.engine.device
        batch = structures_to_batch([atoms[k] for k, _ in chunk], [structs[k].frames[fr] for k, fr in chunk],
                                    neighbor_number, device=dev,
                                    boxes=[structs[k].dimensions[fr] for k, fr in chunk] if boxes else None)
        torch.cuda.synchronize(dev)
        timing['Structure'] += time.perf_counter() - t
        t = time.perf_counter()
        if atom_names is None:
            peaks = model(batch).cpu().numpy().reshape(-1)
            gp = batch.graph_ptr_host
        else:       # the selected atoms of every structure-frame, on their receptive fields alone
            peaks = model.predict_selected(batch, np.concatenate([masks[k] for k, _ in chunk])).cpu().numpy().reshape(-1)
            gp = np.concatenate([[0], np.cumsum([len(index[k]) for k, _ in chunk])])
        conf = []
        for m, (k, fr) in enumerate(chunk):
            try:
                conf.append(check_peaks(atoms[k][index[k]], peaks[gp[m]:gp[m + 1]]))
            except Warning as w:
                if not keep_going:
                    raise
                echo(f'{struct_files[k]} frame {fr}: {w}')
                conf.append(np.zeros(gp[m + 1] - gp[m], dtype=bool))
        timing['Model Inference (MI355X)'] += time.perf_counter() - t
        t = time.perf_counter()
        for m, (k, fr) in enumerate(chunk):
            s = structs[k]
            pk = np.round(peaks[gp[m]:gp[m + 1]].astype(np.float64), 2)
            for j, i in enumerate(index[k]):
                rows.append((struct_files[k], int(i), s.resnames[i], int(s.resids[i]), s.names[i], pk[j], bool(conf[m][j]),
                             float(fr), fr))
        timing['Parsing'] += time.perf_counter() - t
        echo('|'.join(f'{k}:{v:5.2f}s' for k, v in timing.items()))
    os.makedirs(os.path.dirname(os.path.abspath(output_csv)), exist_ok=True)
    with open(output_csv, 'w', newline='') as f:
        wr = csv.writer(f)
        wr.writerow(['file', 'index', 'residues', 'resids', 'names', 'peaks', 'confident', 'time', 'frame'])
        wr.writerows(rows)
    echo(f'You can now find your result in {output_csv}')
    return timing


@main.command(name='eval-struct')
@click.argument('struct-files', nargs=-1, type=click.Path(exists=True))
@click.argument('output-csv')
@click.option('--model-file', type=click.Path(exists=True), default=None,
              help='Model file. If not provided, baseline will be used.')
@click.option('--neighbor-number', default=16, help='The model specific size of neighbor lists')
@click.option('--stride', default=1, help='Stride for reading trajectory, if multiple frames are present')
@click.option('--frames-per-batch', default=32, help='Frames evaluated per device batch')
@click.option('--keep-going', is_flag=True, help='Report implausible-shift warnings instead of aborting')
@click.option('--pbc', is_flag=True, help='Minimum-image neighbour lists in each frame\'s periodic box (CRYST1)')
@click.option('--separate', is_flag=True,
              help='Treat every struct file as a structure of its own (CSV gains a leading file column)')
@click.option('--boxes', is_flag=True,
              help='With --separate: minimum-image neighbour lists in each structure\'s own box (CRYST1), open boundaries '
                   'for structures without one')
@click.option('--uncertainty', default=0, metavar='S',
              help='Append std_model and std_input (ppm) per atom and frame: the closed-form dropout spread and the spread '
                   'over S noisy replicas of the frame')
@click.option('--position-sigma', default=None, type=float, metavar='X',
              help='With --uncertainty: the input spread from a coordinate error of X Angstrom instead of the model\'s '
                   'distance noise')
@click.option('--average', is_flag=True,
              help='One row per atom: mean and standard deviation of the shifts over the frames read')
@click.option('--atom-names', default=None, metavar='A,B,...',
              help='Only the atoms with one of these PDB names (exact match, comma separated, e.g. H,N,CA,CB,C): the model runs '
                   'on the atoms that can reach them; rows keep their original index')
@click.option('--reweight', default=None, type=click.Path(exists=True), metavar='TABLE',
              help='Maximum-entropy reweighting of the frames against the assigned shifts of TABLE (CSV: resid,name,shift'
                   '[,resname][,error]): one row per atom with the weighted mean and spread, and <output stem>.weights.csv '
                   'with the weight of every frame; needs --theta and --sigma')
@click.option('--theta', default=None, type=float, metavar='X',
              help='With --reweight: the regularisation strength (> 0); large keeps the ensemble, small fits the shifts')
@click.option('--sigma', default=None, metavar='SPEC',
              help='With --reweight: the error of a measured-minus-predicted shift in ppm, one number or per element as '
                   'H=0.3,C=1.1,N=2.5; an error column of TABLE overrides it for its row.  No default: the honest values are '
                   'the per-element RMSDs of an eval-records report of the model')
def eval_struct(struct_files, output_csv, model_file, neighbor_number, stride, frames_per_batch, keep_going, pbc, separate,
                boxes, uncertainty, position_sigma, average, atom_names, reweight, theta, sigma):
    '''Predict NMR chemical shifts with specific file'''
    if separate and (uncertainty or average):
        raise click.UsageError('--separate cannot be combined with --uncertainty or --average: the files are different '
                               'topologies, and both options work on the frames of one')
    if uncertainty < 0:
        raise click.UsageError('--uncertainty takes a number of replicas >= 1')
    if position_sigma is not None and not uncertainty:
        raise click.UsageError('--position-sigma goes with --uncertainty S')
    if average and uncertainty:
        raise click.UsageError('--average and --uncertainty cannot be combined: run them one after the other')
    if separate and pbc:
        raise click.UsageError('--separate and --pbc cannot be combined; use --separate --boxes for one box, or none, per '
                               'structure')
    if boxes and not separate:
        raise click.UsageError('--boxes goes with --separate; use --pbc for frames of one topology')
    if separate and any(f.lower().endswith(('.dcd', '.nc', '.ncdf')) for f in struct_files):
        raise click.UsageError('--separate takes PDB files, each a structure of its own; a binary trajectory (.dcd, .nc, '
                               '.ncdf) holds frames of the topology in front of it: run it without --separate')
    if reweight is not None:
        if separate or uncertainty or average:
            raise click.UsageError('--reweight cannot be combined with --separate, --uncertainty or --average')
        if theta is None:
            raise click.UsageError('--reweight needs --theta X (the regularisation strength, > 0)')
        if sigma is None:
            raise click.UsageError('--reweight needs --sigma SPEC: there is no default error')
    elif theta is not None or sigma is not None:
        raise click.UsageError('--theta and --sigma go with --reweight TABLE')
    names = None
    if atom_names is not None:
        names = [a.strip() for a in atom_names.split(',') if a.strip()]
        if not names:
            raise click.UsageError('--atom-names takes a comma-separated list of PDB atom names')
    try:
        eval_structure(struct_files, output_csv, model_file, neighbor_number, stride, frames_per_batch,
                       keep_going, echo=click.echo, pbc=pbc, separate=separate, boxes=boxes, uncertainty=uncertainty,
                       position_sigma=position_sigma, average=average, atom_names=names, reweight=reweight, theta=theta,
                       sigma=sigma)
    except ReweightUsageError as e:
        raise click.UsageError(str(e))
    except AtomNamesError as e:
        raise click.ClickException(str(e))


def _load_embeddings(path):
    """nmrdata's embeddings dict ({'atom': ..., 'nlist': ..., 'name': {name: id}}) from a JSON or a pickle file"""
    import json
    import pickle
    with open(path, 'rb') as f:
        raw = f.read()
    try:
        emb = json.loads(raw.decode('utf-8'))
    except (UnicodeDecodeError, ValueError):
        emb = pickle.loads(raw)
    if not isinstance(emb, dict) or 'name' not in emb:
        raise ValueError(f"{path}: no embeddings dict with a 'name' table")
    return emb


def _parse_lr_scale(text):
    """'mp/*=0.1,fc=0.5' -> {'mp/*': 0.1, 'fc': 0.5}, in the order given"""
    out = {}
    for item in text.split(','):
        pat, eq, val = item.strip().partition('=')
        try:
            out[pat.strip()] = float(val)
        except ValueError:
            eq = ''
        if not eq or not pat.strip():
            raise ValueError(f"--lr-scale: {item!r} is not PATTERN=SCALE")
    return out


def _finetune_args(freeze, lr_scale, clipnorm):
    """(trainable tensor names or None, lr_scale dict or None) of ``train``'s fine-tuning options, checked against the
    model's parameter tensors: ``freeze`` names what KEEPS its values, so the trainable set is its complement.  ValueError on
    a pattern that selects nothing, a malformed or negative scale, a freeze that leaves nothing, a clipnorm not > 0."""
    from .finetune import resolve, scales
    from .hypers import HyperParameters, declare_gnn_space
    from .params import param_shapes
    names = [n for n, _ in param_shapes(declare_gnn_space(HyperParameters()), 1)]      # what build_GNNModel builds
    trainable = None
    if freeze:
        frozen = set(resolve(freeze, names))
        trainable = [n for n in names if n not in frozen]
        if not trainable:
            raise ValueError(f"--freeze {freeze!r} leaves no tensor to train")
    if isinstance(lr_scale, str):
        lr_scale = _parse_lr_scale(lr_scale)
    if lr_scale:
        scales(names, trainable, lr_scale)
    if clipnorm is not None and not 0.0 < float(clipnorm) < float('inf'):
        raise ValueError(f"--clipnorm must be positive and finite, got {clipnorm}")
    return trainable, (lr_scale or None)


def train_model(records, name, epochs=3, checkpoint_path='/tmp/checkpoint', embeddings=None, validation=0.1, load=False,
                loss_balance=1.0, batch_graphs=1, seed=0, device=None, echo=print, standards='default', freeze=None,
                lr_scale=None, clipnorm=None):
    """The reference's ``train`` (nmrgnn/main.py:36-90) on ``ShiftDataset`` files: build the model, optionally load the
    checkpoint, fit with ReduceLROnPlateau(val_loss, 0.99, patience 4, min_lr 1e-4) and a checkpoint every epoch, save the
    model to ``name`` and pickle the history to the first free ``name-history-<i>.pb``.  Returns ``(model, history)``.
    ``standards``: ``'default'`` (the bundled ``standards.load_standards()``) or ``'data'`` (``standards()`` of the train
    view: the per-element mean and spread of the labels the model is trained on).
    Fine-tuning (with ``load``): ``freeze``: patterns (``GNNModel.trainable_names``) of the tensors that KEEP their values —
    everything else trains; ``lr_scale``: ``'pattern=scale,...'`` or a dict, the first match wins; ``clipnorm``: clip the
    gradient of the trained tensors to this norm.  A pattern that matches nothing raises ValueError before any work."""
    import pickle
    from .callbacks import ModelCheckpoint, ReduceLROnPlateau, history_path
    from .dataset import ShiftDataset
    from .model import build_GNNModel
    if len(records) == 0:
        raise ValueError('Must give input record files')
    if standards not in ('default', 'data'):
        raise ValueError(f"standards is 'default' or 'data', got {standards!r}")
    emb = _load_embeddings(embeddings) if embeddings is not None else None
    trainable, lr_scale = _finetune_args(freeze, lr_scale, clipnorm)
    data = ShiftDataset.load(list(records), device=device)
    train_data, validation_data = data.split(validation)
    if train_data.grouped:
        echo(f"Ensemble-averaged training: {len(train_data.group_ptr) - 1} groups of {len(train_data)} frames; the loss is "
             "taken on the mean prediction of every group")
    model = build_GNNModel(loss_balance=loss_balance, device=device, embeddings=emb,
                           peak_standards=train_data.standards() if standards == 'data' else None)
    if trainable is not None:
        from .params import param_shapes
        sizes = {n: int(np.prod(sh)) for n, sh in param_shapes(model.hypers, train_data.C)}
        echo(f"Training {sum(sizes[n] for n in trainable)} of {sum(sizes.values())} parameters: {', '.join(trainable)}")
    if load:
        model.load_weights(checkpoint_path)
    callbacks = []
    if len(validation_data):              # the plateau rule watches val_loss
        callbacks.append(ReduceLROnPlateau(monitor='val_loss', factor=0.99, patience=4, min_lr=1e-4, verbose=1))
    callbacks.append(ModelCheckpoint(checkpoint_path))
    results = model.fit(train_data, epochs=epochs, callbacks=callbacks, batch_graphs=batch_graphs, seed=seed,
                        validation_data=validation_data if len(validation_data) else None, verbose=0, trainable=trainable,
                        lr_scale=lr_scale, clipnorm=clipnorm)
    for e, i in enumerate(results.epoch):
        echo(f"Epoch {i + 1}: " + " - ".join(f"{k}: {v[e]:.6g}" for k, v in results.history.items()))
    model.save(name)
    pfile = history_path(name)
    with open(pfile, 'wb') as f:
        pickle.dump(results.history, file=f)
    echo(f'Model saved to {name}, history to {pfile}')
    return model, results


@main.command(name='train')
@click.argument('records', nargs=-1, type=click.Path(exists=True))
@click.argument('name')
@click.argument('epochs', default=3)
@click.option('--checkpoint-path', default='/tmp/checkpoint', type=click.Path(), help='where to save model')
@click.option('--embeddings', default=None, type=click.Path(exists=True),
              help='JSON or pickle file with the nmrdata embeddings dict (enables the per-name metrics)')
@click.option('--validation', default=0.1, help='relative size of validation')
@click.option('--load/--noload', default=False, help='Load saved model at checkpoint path?')
@click.option('--loss-balance', default=1.0, help='Balance between L2 (max @ 1.0) and corr loss (max @ 0.0)')
@click.option('--batch-graphs', default=1, help='Records per optimiser step (1: the reference; more changes the optimisation)')
@click.option('--seed', default=0, help='Seed of the per-epoch shuffle')
@click.option('--device', default=None, help='Device, e.g. cuda:0')
@click.option('--standards', default='default', type=click.Choice(['default', 'data']),
              help='Peak standards of the model: the bundled ones, or the per-element mean and spread of the training labels')
@click.option('--freeze', default=None,
              help="Fine-tuning: comma-separated tensors, groups or patterns that keep their values, e.g. "
                   "'embed/*,edge_fc/*,mp/0/*'; everything else trains")
@click.option('--lr-scale', default=None, help="Rate scales 'PATTERN=SCALE,...', e.g. 'mp/*=0.1'; the first match wins")
@click.option('--clipnorm', default=None, type=float, help='Clip the gradient of the trained tensors to this norm')
def train(records, name, epochs, checkpoint_path, embeddings, validation, load, loss_balance, batch_graphs, seed, device,
          standards, freeze, lr_scale, clipnorm):
    '''Train the model on ShiftDataset record files (.npz)'''
    if len(records) == 0:
        raise click.UsageError('Must give input record files')
    try:        # a pattern that selects nothing is a usage error, found before any data is read
        _finetune_args(freeze, lr_scale, clipnorm)
    except ValueError as e:
        raise click.UsageError(str(e))
    train_model(records, name, epochs, checkpoint_path=checkpoint_path, embeddings=embeddings, validation=validation,
                load=load, loss_balance=loss_balance, batch_graphs=batch_graphs, seed=seed, device=device, echo=click.echo,
                standards=standards, freeze=freeze, lr_scale=lr_scale, clipnorm=clipnorm)


def _pair_structure(field):
    """the structure field of ``make-records --pair``: a PDB path, or ``top.pdb,traj.dcd[,more]`` — the atoms of the PDB with
    the frames of the binary trajectory files (``trajectory.load_structure``)"""
    from .trajectory import is_trajectory_file, load_structure
    parts = [p for p in str(field).split(',') if p]
    if not os.path.exists(str(field)) and len(parts) > 1 and all(is_trajectory_file(p) for p in parts[1:]):
        missing = [p for p in parts if not os.path.exists(p)]
        if missing:
            raise ValueError(f"--pair {field}: {missing[0]} does not exist")
        return load_structure(parts[0], *parts[1:])
    return field


def make_records(out, pairs, frames='first', neighbor_number=16, embeddings=None, embeddings_out=None, pbc=False,
                 keep_going=False, device=None, echo=print, ensembles=False):
    """``make-records``: structures with assigned shifts -> one ``ShiftDataset`` file.  ``pairs``: ``(structure file, shift
    table CSV)`` per structure.  ``embeddings``: take the name ids from this file's ``'name'`` table (keys it lacks get id 0);
    otherwise the table is ``structure.name_table`` of the structures, and ``embeddings_out`` writes it as the JSON
    ``{'atom': ..., 'name': ...}`` that ``train --embeddings`` reads.  ``pbc``: minimum-image lists in every frame's CRYST1
    box.  ``keep_going``: drop and count shift-table rows that do not join instead of stopping.  ``ensembles`` (with
    ``frames='all'``): the frames of every structure become one ensemble group, and ``train`` fits their mean.  Returns the
    store."""
    import json
    from .dataset import ShiftDataset
    from .standards import load_embeddings
    if len(pairs) == 0:
        raise ValueError('Must give at least one --pair STRUCT SHIFTS')
    if embeddings is not None and embeddings_out is not None:
        raise ValueError('--embeddings and --embeddings-out cannot be combined')
    names = _load_embeddings(embeddings)['name'] if embeddings is not None else None
    ds = ShiftDataset.from_structures([_pair_structure(p[0]) for p in pairs], [p[1] for p in pairs], neighbor_number=neighbor_number,
                                      frames=frames, names=names, boxes=pbc, strict=not keep_going, device=device,
                                      ensembles=ensembles)
    ds.save(out)
    rep = ds.join_report
    echo(f"{ds.R} records, {ds.Ntot} atoms, {rep['labelled']} labelled rows from {rep['rows']} table rows of "
         f"{rep['structures']} structures written to {out}")
    if ensembles:
        echo(f"{len(ds.group_ptr) - 1} ensemble groups: the frames of a structure are trained on their mean")
    dropped = {k: v for k, v in rep.items() if k not in ('rows', 'labelled', 'structures') and v}
    if dropped:
        echo('table rows dropped: ' + ', '.join(f'{k}: {v}' for k, v in dropped.items()))
    if embeddings_out is not None:
        with open(embeddings_out, 'w') as f:
            json.dump({'atom': load_embeddings()['atom'], 'name': ds.name_table}, f, indent=1)
        echo(f'Embeddings written to {embeddings_out}')
    return ds


@main.command(name='make-records')
@click.argument('out', type=click.Path())
@click.option('--pair', 'pairs', nargs=2, multiple=True, type=click.Path(), metavar='STRUCT SHIFTS',
              help='A structure file (PDB, or top.pdb,traj.dcd[,more.nc]: the frames of binary trajectory files on the atoms of '
                   'the PDB) and the CSV of its assigned shifts (resid,name,shift[,resname]); repeat per structure')
@click.option('--frames', default='first', type=click.Choice(['first', 'all']),
              help='One record per structure, or one per frame (MODEL) with the same labels')
@click.option('--ensembles', is_flag=True,
              help='With --frames all: the frames of a structure are one ensemble group; train then fits their MEAN to the shifts')
@click.option('--neighbor-number', default=16, help='The model specific size of neighbor lists')
@click.option('--embeddings', default=None, type=click.Path(exists=True),
              help='JSON or pickle file with an embeddings dict: name ids come from its name table')
@click.option('--embeddings-out', default=None, type=click.Path(),
              help='Write the name table built from the structures as a JSON embeddings file for train --embeddings')
@click.option('--pbc', is_flag=True, help='Minimum-image neighbour lists in each frame\'s periodic box (CRYST1)')
@click.option('--keep-going', is_flag=True, help='Drop and count shift-table rows that match no atom instead of stopping')
@click.option('--device', default=None, help='Device, e.g. cuda:0')
def make_records_cmd(out, pairs, frames, ensembles, neighbor_number, embeddings, embeddings_out, pbc, keep_going, device):
    '''Build a ShiftDataset record file (.npz) from structures and shift tables'''
    if len(pairs) == 0:
        raise click.UsageError('Must give at least one --pair STRUCT SHIFTS')
    if embeddings is not None and embeddings_out is not None:
        raise click.UsageError('--embeddings and --embeddings-out cannot be combined')
    if ensembles and frames != 'all':
        raise click.UsageError('--ensembles groups the frames of a structure and needs --frames all')
    for struct, table in pairs:
        for p in ([struct] if os.path.exists(struct) else [q for q in struct.split(',') if q]) + [table]:
            if not os.path.exists(p):
                raise click.BadParameter(f"Path '{p}' does not exist.", param_hint="'--pair'")
    try:
        make_records(out, pairs, frames=frames, neighbor_number=neighbor_number, embeddings=embeddings,
                     embeddings_out=embeddings_out, pbc=pbc, keep_going=keep_going, device=device, echo=click.echo,
                     ensembles=ensembles)
    except ValueError as e:
        raise click.ClickException(str(e))


def eval_records(records, model_file=None, embeddings=None, validation=0.0, data_name='', merge=None, batch_graphs=64,
                 device=None, square_root=False, write_csv=True, out_dir=None, echo=print):
    """The reference's ``eval-tfrecords`` (nmrgnn/main.py:93-189) on ``ShiftDataset`` files: per element and per atom name
    the count, the Pearson r and the squared error of the model's shifts on the labelled atoms (``GNNModel.evaluate_report``:
    the sums are taken on the device, one pass per batch).  Writes ``{model_name}.csv`` (``element,y,yhat,class,name``, unless
    ``write_csv`` is off) and ``{model_name}.md`` into ``out_dir`` (default: the working directory), or the table into the
    ``merge`` file with that file's rows appended; ``model_name`` is the base name of ``model_file`` (``baseline`` without one).
    ``embeddings``: the file ``train --embeddings`` reads; its ``'name'`` table says which key a name id of the records stands
    for.  ``validation`` > 0: only the validation share of ``ShiftDataset.split`` is evaluated.  The rows keyed ``-rmsd`` hold
    the MEAN SQUARED ERROR, as the reference's do; ``square_root`` writes the root instead.  Returns the ``EvalReport``."""
    from .dataset import ShiftDataset
    from .library import load_model
    if len(records) == 0:
        raise ValueError('Must give input record files')
    if embeddings is None:
        raise ValueError('eval-records needs --embeddings: the record files carry name ids, the table their keys')
    name_table = _load_embeddings(embeddings)['name']
    model = load_model(model_file, device=device)
    model_name = 'baseline' if model_file is None else os.path.basename(os.path.normpath(model_file))
    data = ShiftDataset.load(list(records), device=device)
    train_data, validation_data = data.split(validation)
    data = validation_data if validation > 0 else train_data
    echo('Computing...')
    report = model.evaluate_report(data, name_table, data_name=data_name, batch_graphs=batch_graphs, rows=write_csv)
    echo(f'done: {len(data)} records, {report.labelled} labelled atoms' + (f', {report.unnamed} of them unnamed' if report.unnamed else ''))
    out_dir = '.' if out_dir is None else out_dir
    if write_csv:
        report.to_csv(os.path.join(out_dir, f'{model_name}.csv'))
    target = os.path.join(out_dir, f'{model_name}.md') if merge is None else merge
    report.to_markdown(target, model_name, merge=merge, square_root=square_root)
    echo(f'You can now find your result in {target}')
    return report


@main.command(name='eval-records')
@click.argument('records', nargs=-1, type=click.Path(exists=True))
@click.option('--model-file', type=click.Path(exists=True), default=None,
              help='Model file. If not provided, baseline will be used.')
@click.option('--validation', default=0.0, help='relative size of validation. If non-zero, only validation will be saved')
@click.option('--data-name', default='', help='Short name for data on table output')
@click.option('--merge', default=None, help='Merge results with another markdown table')
@click.option('--embeddings', required=True, type=click.Path(exists=True),
              help='JSON or pickle file with the embeddings dict whose name table gives the key of every name id')
@click.option('--batch-graphs', default=64, help='Records per device batch')
@click.option('--device', default=None, help='Device, e.g. cuda:0')
@click.option('--sqrt', 'square_root', is_flag=True,
              help='Write the root of the mean squared error in the -rmsd rows; by default they hold the MEAN SQUARED ERROR, '
                   'as the reference writes it under that key')
@click.option('--no-csv', is_flag=True, help='Write the table only, not the CSV of every labelled atom')
def eval_records_cmd(records, model_file, validation, data_name, merge, embeddings, batch_graphs, device, square_root, no_csv):
    '''Evaluate a model on ShiftDataset record files (.npz): r and squared error per element and atom name'''
    if len(records) == 0:
        raise click.UsageError('Must give input record files')
    try:
        eval_records(records, model_file=model_file, embeddings=embeddings, validation=validation, data_name=data_name,
                     merge=merge, batch_graphs=batch_graphs, device=device, square_root=square_root, write_csv=not no_csv,
                     echo=click.echo)
    except ValueError as e:
        raise click.ClickException(str(e))


if __name__ == '__main__':
    main()
