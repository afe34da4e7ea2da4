"""Test-side builders of binary trajectory files, independent of nmrgnn_amd.trajectory: DCD bytes from ``struct`` / NumPy by the
layout of DESIGN.md §7.26, Amber NetCDF through ``scipy.io.netcdf_file``; and a NumPy decode of the byte layout that
``ng_frames_decode`` takes.  Nothing here imports the package."""
import struct

import numpy as np


def cell_record(dims, cosines=False):
    """the 6 float64 of a DCD unit-cell record, ``A, gamma, B, beta, alpha, C``, from (a, b, c, alpha, beta, gamma); the angles
    as degrees, or as the cosines NAMD writes"""
    a, b, c, al, be, ga = [float(x) for x in dims]
    if cosines:
        al, be, ga = [float(np.cos(np.radians(x))) for x in (al, be, ga)]
    return [a, ga, b, be, al, c]


def dcd_bytes(frames, cells=None, big=False, ntitle=2, fourth=False, nset=None, fixed=0, charmm=24, cut=0, wide_markers=False):
    """A CHARMM-form DCD as bytes.  ``frames`` float32 [T, n, 3]; ``cells``: per frame the six float64 of its cell record
    (``cell_record``) or None; ``fourth``: a W record behind Z; ``nset``: the frame count the header announces (default T);
    ``cut``: bytes dropped from the end; ``wide_markers``: 64-bit record markers (a file the reader refuses)."""
    frames = np.asarray(frames, np.float32)
    T, n = frames.shape[:2]
    e = '>' if big else '<'
    mark = (lambda k: struct.pack(e + 'q', k)) if wide_markers else (lambda k: struct.pack(e + 'i', k))

    def record(payload):
        return mark(len(payload)) + payload + mark(len(payload))

    icntrl = [0] * 20
    icntrl[0] = T if nset is None else nset
    icntrl[1], icntrl[2] = 1, 1
    icntrl[8] = fixed
    icntrl[10] = 1 if cells is not None else 0
    icntrl[11] = 1 if fourth else 0
    icntrl[19] = charmm
    out = [record(b'CORD' + struct.pack(e + '20i', *icntrl)),
           record(struct.pack(e + 'i', ntitle) + b''.join((b'title line %d' % k).ljust(80) for k in range(ntitle))),
           record(struct.pack(e + 'i', n))]
    for t in range(T):
        if cells is not None:
            out.append(record(struct.pack(e + '6d', *cells[t])))
        for c in range(3):
            out.append(record(frames[t, :, c].astype(e + 'f4').tobytes()))
        if fourth:
            out.append(record(np.full(n, 7.0, e + 'f4').tobytes()))
    blob = b''.join(out)
    return blob[:len(blob) - cut] if cut else blob


def write_dcd_ref(path, frames, **kw):
    with open(path, 'wb') as f:
        f.write(dcd_bytes(frames, **kw))


def write_netcdf_ref(path, frames, dims=None, version=1, before=(), after=(), scale_factor=None, coordinates='coordinates',
                     spatial=3):
    """An Amber NetCDF trajectory written by scipy.  ``dims`` [T, 6] or None; ``before`` / ``after``: names of extra record
    variables created before and after ``coordinates`` (``time``: float32 per frame; anything else: float32 (frame, atom,
    spatial)); ``scale_factor``: that attribute on the coordinates; ``coordinates``: the name the variable gets."""
    from scipy.io import netcdf_file
    frames = np.asarray(frames, np.float32)
    T, n = frames.shape[:2]
    f = netcdf_file(str(path), 'w', version=version)
    f.Conventions = 'AMBER'
    f.ConventionVersion = '1.0'
    f.createDimension('frame', None)
    f.createDimension('spatial', spatial)
    f.createDimension('atom', n)
    if dims is not None:
        f.createDimension('cell_spatial', 3)
        f.createDimension('cell_angular', 3)

    def extra(name):
        if name == 'time':
            v = f.createVariable('time', 'f', ('frame',))
            v[:T] = np.arange(T, dtype=np.float32)
        else:
            v = f.createVariable(name, 'f', ('frame', 'atom', 'spatial'))
            v[:T] = np.full((T, n, spatial), -3.5, np.float32)

    for name in before:
        extra(name)
    co = f.createVariable(coordinates, 'f', ('frame', 'atom', 'spatial'))
    co.units = 'angstrom'
    if scale_factor is not None:
        co.scale_factor = np.float32(scale_factor)
    if T:
        co[:T] = frames[:, :, :spatial]
    for name in after:
        extra(name)
    if dims is not None:
        cl = f.createVariable('cell_lengths', 'd', ('frame', 'cell_spatial'))
        ca = f.createVariable('cell_angles', 'd', ('frame', 'cell_angular'))
        if T:
            cl[:T] = np.asarray(dims, np.float64)[:, :3]
            ca[:T] = np.asarray(dims, np.float64)[:, 3:]
    f.close()


def decode_ref(raw, G, frame_stride, off, elem_stride, swap, n_src, sel=None):
    """uint32 [G, n_out, 3]: the words of a raw chunk (uint8 array) by the layout of ``ng_frames_decode``, and the count of
    values among them that are not finite"""
    raw = np.asarray(raw, np.uint8)
    atoms = np.arange(n_src) if sel is None else np.asarray(sel, np.int64)
    out = np.empty((G, len(atoms), 3), np.uint32)
    for g in range(G):
        for c in range(3):
            at = g * frame_stride + off[c] + atoms * elem_stride
            quad = raw[at[:, None] + np.arange(4)[None, :]].astype(np.uint32)
            if swap:        # the file's order is the reverse of the host's (little-endian) one
                out[g, :, c] = (quad[:, 0] << 24) | (quad[:, 1] << 16) | (quad[:, 2] << 8) | quad[:, 3]
            else:
                out[g, :, c] = quad[:, 0] | (quad[:, 1] << 8) | (quad[:, 2] << 16) | (quad[:, 3] << 24)
    bad = int(((out & 0x7f800000) == 0x7f800000).sum())
    return out, bad
