"""Binary trajectories: DCD (CHARMM/NAMD form) and Amber NetCDF-3, from the file to ``[frames, atoms, 3]`` positions on the
device.

``open_trajectory(path)`` picks the reader by the file's magic bytes.  A reader knows ``n_atoms``, ``n_frames``, ``has_box``,
reads frames on the host with NumPy (``read``, ``dimensions``) and describes its bytes (``layout``) for the device path:
``TrajectoryStream`` moves raw file bytes through two pinned staging buffers and decodes them with one kernel launch per
chunk (``ng_frames_decode``, csrc/traj.hip: either endianness, planar or interleaved components, atom selection, a count of
non-finite values).  ``write_dcd`` / ``write_netcdf`` write both formats; ``load_structure`` makes a host ``Structure`` of a
topology PDB and trajectory files.  Both formats are uncompressed float32.  XTC and TRR are not read: convert them.
"""
from __future__ import annotations

import os
import queue
import struct
import sys
import threading
import warnings

import numpy as np

_HOST_BIG = sys.byteorder == 'big'
_CHUNK_LIMIT = (1 << 31) - 1            # ng_frames_decode takes fewer than 2^31 bytes per call

TRAJECTORY_SUFFIXES = ('.dcd', '.nc', '.ncdf')


class TrajectoryError(ValueError):
    """a trajectory file that is refused: the message names the file and the reason"""


def is_trajectory_file(path):
    """True for the suffixes that ``eval-struct`` and ``make-records`` take as binary trajectories"""
    return str(path).lower().endswith(TRAJECTORY_SUFFIXES)


def _cell_rows(lengths, angles):
    """[G, 6] (a, b, c, alpha, beta, gamma); a frame whose lengths are all zero has no box: a row of NaN"""
    dims = np.concatenate([lengths, angles], axis=1).astype(np.float64)
    dims[(lengths == 0).all(axis=1)] = np.nan
    return dims


class _Trajectory:
    """What both readers share: frames are ``frame_stride`` bytes apart from the file offset ``first``, and component c of atom
    a of a frame is the 32-bit word at ``off[c] + a * elem_stride`` inside it."""

    path = None
    n_atoms = 0
    n_frames = 0
    has_box = False
    format = ''
    big_endian = False
    _first = 0
    _frame_stride = 0
    _off = (0, 0, 0)
    _elem_stride = 4
    _span = (0, 0)

    def __len__(self):
        return self.n_frames

    def layout(self):
        """The bytes of the file as ``ng_frames_decode`` wants them: ``first`` (file offset of frame 0), ``frame_stride``,
        ``off`` (the byte offsets of x, y, z inside a frame), ``elem_stride`` (bytes between consecutive atoms of one
        component), ``swap`` (1: the file's byte order is not the host's), ``span`` ``(start, bytes)`` — the part of a frame
        that holds its coordinates and cell data, which is all a strided read fetches — and ``n_atoms``, ``n_frames``."""
        return {'first': self._first, 'frame_stride': self._frame_stride, 'off': tuple(self._off),
                'elem_stride': self._elem_stride, 'swap': int(self.big_endian != _HOST_BIG), 'span': tuple(self._span),
                'n_atoms': self.n_atoms, 'n_frames': self.n_frames}

    def frame_ids(self, frame_ids=None):
        """int64 [G] frame numbers, checked against ``n_frames`` (None: every frame)"""
        if frame_ids is None:
            return np.arange(self.n_frames, dtype=np.int64)
        ids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= self.n_frames):
            raise IndexError(f"{self.path}: frame {int(ids.max() if ids.max() >= self.n_frames else ids.min())} is outside "
                             f"[0, {self.n_frames})")
        return ids

    def _body(self):
        """the frames of the file as a read-only [n_frames, frame_stride] byte matrix"""
        if self.n_frames == 0:
            return np.zeros((0, max(self._frame_stride, 1)), np.uint8)
        mm = np.memmap(self.path, dtype=np.uint8, mode='r', offset=self._first, shape=(self.n_frames * self._frame_stride,))
        return mm.reshape(self.n_frames, self._frame_stride)

    def read(self, frame_ids=None):
        """float32 [G, n_atoms, 3] of the frames ``frame_ids`` (None: all), decoded on the host with NumPy.  Words are moved
        as integers, so every bit pattern survives."""
        ids = self.frame_ids(frame_ids)
        out = np.empty((len(ids), self.n_atoms, 3), np.uint32)
        if len(ids):
            body, word = self._body(), '>u4' if self.big_endian else '<u4'
            n, es = self.n_atoms, self._elem_stride
            for c in range(3):
                run = np.ascontiguousarray(body[ids, self._off[c]:self._off[c] + (n - 1) * es + 4])
                if es == 4:
                    out[:, :, c] = run.view(word)
                else:       # one word every es bytes
                    out[:, :, c] = np.lib.stride_tricks.as_strided(run.view(word), (len(ids), n),
                                                                   (run.strides[0], es), writeable=False)
        return out.view(np.float32)

    def dimensions(self, frame_ids=None):
        """float64 [G, 6] ``(a, b, c, alpha, beta, gamma)`` in Angstrom and degrees — the conventions of
        ``Structure.dimensions`` — or None for a file without cell data.  A frame whose cell lengths are all zero has no box:
        its row is NaN."""
        if not self.has_box:
            return None
        ids = self.frame_ids(frame_ids)
        if not len(ids):
            return np.zeros((0, 6))
        start, nbytes = self._span
        return self.decode_cells(np.ascontiguousarray(self._body()[ids, start:start + nbytes]), start)

    def decode_cells(self, rows, shift):
        """[G, 6] boxes from staged bytes: ``rows`` uint8 [G, >= span] whose column 0 is byte ``shift`` of a frame"""
        raise NotImplementedError


# ---------------------------------------------------------------------------------------------------------------- DCD

class DCDTrajectory(_Trajectory):
    """DCD in the CHARMM/NAMD form: Fortran records framed by 32-bit markers; per frame an optional 48-byte unit-cell record
    (6 float64 ``A, gamma, B, beta, alpha, C``), then X, Y, Z records of NATOM float32 and an optional fourth one."""
    format = 'DCD'

    def __init__(self, path):
        self.path = str(path)
        size = os.path.getsize(self.path)
        with open(self.path, 'rb') as f:
            head = f.read(92)
            if len(head) < 92:
                raise TrajectoryError(f"{self.path}: too short for a DCD header")
            if struct.unpack('<q', head[:8])[0] == 84 or struct.unpack('>q', head[:8])[0] == 84:
                raise TrajectoryError(f"{self.path}: DCD with 64-bit record markers is not supported (32-bit markers only)")
            if struct.unpack('<i', head[:4])[0] == 84:
                e = '<'
            elif struct.unpack('>i', head[:4])[0] == 84:
                e = '>'
            else:
                raise TrajectoryError(f"{self.path}: not a DCD file: the first record marker is 84 in neither byte order")
            if head[4:8] != b'CORD' or struct.unpack(e + 'i', head[88:92])[0] != 84:
                raise TrajectoryError(f"{self.path}: not a coordinate DCD: the first record does not hold 'CORD' and 20 integers")
            icntrl = struct.unpack(e + '20i', head[8:88])
            if icntrl[8] != 0:
                raise TrajectoryError(f"{self.path}: DCD with fixed atoms ({icntrl[8]} of them) is not supported")
            m = f.read(4)
            if len(m) < 4:
                raise TrajectoryError(f"{self.path}: truncated DCD title record")
            ltitle = struct.unpack(e + 'i', m)[0]
            title = f.read(ltitle + 4)
            if ltitle < 4 or len(title) < ltitle + 4 or struct.unpack(e + 'i', title[ltitle:])[0] != ltitle:
                raise TrajectoryError(f"{self.path}: malformed DCD title record")
            natom = f.read(12)
            if len(natom) < 12 or struct.unpack(e + 'i', natom[:4])[0] != 4 or struct.unpack(e + 'i', natom[8:])[0] != 4:
                raise TrajectoryError(f"{self.path}: malformed DCD atom-count record")
            n = struct.unpack(e + 'i', natom[4:8])[0]
            if n < 1:
                raise TrajectoryError(f"{self.path}: DCD with {n} atoms")
            self._first = f.tell()
        self.big_endian = e == '>'
        self.n_atoms = n
        self.has_box = icntrl[10] != 0
        self.has_fourth = icntrl[11] != 0
        self.charmm = icntrl[19] != 0
        self.nset = int(icntrl[0])
        rec = 4 * n + 8
        base = 56 if self.has_box else 0
        self._frame_stride = base + (4 if self.has_fourth else 3) * rec
        self._off = (base + 4, base + rec + 4, base + 2 * rec + 4)
        self._elem_stride = 4
        self._span = (0, self._frame_stride)
        self.n_frames, rest = divmod(size - self._first, self._frame_stride)
        if rest:
            warnings.warn(f"{self.path}: the last frame is truncated ({rest} of {self._frame_stride} bytes) and is dropped",
                          RuntimeWarning, stacklevel=3)
        if self.nset != self.n_frames:
            warnings.warn(f"{self.path}: the header announces {self.nset} frames, the file holds {self.n_frames} complete "
                          f"ones; using {self.n_frames}", RuntimeWarning, stacklevel=3)

    def decode_cells(self, rows, shift):
        if not self.has_box:
            return None
        cell = np.ascontiguousarray(rows[:, 4 - shift:52 - shift]).view('>f8' if self.big_endian else '<f8').astype(np.float64)
        lengths = cell[:, [0, 2, 5]]
        ang = cell[:, [4, 3, 1]]        # alpha, beta, gamma of the record's A, gamma, B, beta, alpha, C
        cosines = (np.abs(ang) <= 1.0).all(axis=1)
        with np.errstate(invalid='ignore'):
            ang = np.where(cosines[:, None], 90.0 - np.degrees(np.arcsin(np.clip(ang, -1.0, 1.0))), ang)
        return _cell_rows(lengths, ang)


def _frames_array(frames):
    fr = np.ascontiguousarray(np.asarray(frames, dtype=np.float32))
    if fr.ndim == 2:
        fr = fr[None]
    if fr.ndim != 3 or fr.shape[2] != 3 or fr.shape[1] < 1:
        raise ValueError(f"frames must be [T, n, 3] with n >= 1, got {fr.shape}")
    return fr


def _dimension_rows(dimensions, T):
    if dimensions is None:
        return None
    d = np.asarray(dimensions, dtype=np.float64)
    if d.shape == (6,):
        d = np.tile(d, (T, 1))
    if d.shape != (T, 6):
        raise ValueError(f"dimensions must be [6] or [{T}, 6], got {d.shape}")
    return d


def write_dcd(path, frames, dimensions=None, big_endian=False):
    """Write ``frames`` [T, n, 3] float32 (Angstrom) as a CHARMM-form DCD.  ``dimensions``: [6] or [T, 6] ``(a, b, c, alpha,
    beta, gamma)``, written as the unit-cell record with the angles in degrees; None: no cell records."""
    fr = _frames_array(frames)
    T, n = fr.shape[:2]
    dims = _dimension_rows(dimensions, T)
    e = '>' if big_endian else '<'
    icntrl = [0] * 20
    icntrl[0], icntrl[1], icntrl[2], icntrl[3] = T, 1, 1, T
    icntrl[9] = struct.unpack(e + 'i', struct.pack(e + 'f', 1.0))[0]       # the time step, a float32 in this slot
    icntrl[10] = 1 if dims is not None else 0
    icntrl[19] = 24
    title = b'Written by nmrgnn_amd'.ljust(80)
    fields = ([('cm0', e + 'i4'), ('cell', e + 'f8', (6,)), ('cm1', e + 'i4')] if dims is not None else [])
    for c in 'xyz':
        fields += [(c + '0', e + 'i4'), (c, e + 'u4', (n,)), (c + '1', e + 'i4')]      # float32 moved as bits
    rec = np.dtype(fields)
    with open(path, 'wb') as f:
        f.write(struct.pack(e + 'i4s20ii', 84, b'CORD', *icntrl, 84))
        f.write(struct.pack(e + 'ii80si', 84, 1, title, 84))
        f.write(struct.pack(e + 'iii', 4, n, 4))
        step = max(1, (64 << 20) // rec.itemsize)
        for t0 in range(0, T, step):
            part = fr[t0:t0 + step]
            buf = np.zeros(len(part), rec)
            if dims is not None:
                d = dims[t0:t0 + step]
                buf['cm0'] = buf['cm1'] = 48
                buf['cell'] = d[:, [0, 5, 1, 4, 3, 2]]      # A, gamma, B, beta, alpha, C
            for k, c in enumerate('xyz'):
                buf[c + '0'] = buf[c + '1'] = 4 * n
                buf[c] = part[:, :, k].view(np.uint32)
            f.write(buf.tobytes())


# ------------------------------------------------------------------------------------------------------------- NetCDF

_NC_DIMENSION, _NC_VARIABLE, _NC_ATTRIBUTE = 0x0A, 0x0B, 0x0C
_NC_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4, 6: 8}             # byte, char, short, int, float, double
_NC_CODE = {1: 'i1', 3: '>i2', 4: '>i4', 5: '>f4', 6: '>f8'}
_NC_STREAMING = 0xFFFFFFFF


def _pad4(n):
    return (n + 3) & ~3


class _NCHeader:
    """The header of a classic NetCDF file (CDF-1: 32-bit ``begin`` offsets, CDF-2: 64-bit): ``numrecs``, ``dims`` [(name,
    length)], ``attrs`` {name: value} and ``vars`` {name: dict(dimids, attrs, type, begin, shape, record)}.  ``parse`` raises
    ``struct.error`` when ``buf`` ends inside the header."""

    def __init__(self, buf):
        self.buf, self.pos = buf, 4
        self.wide = buf[3] == 2
        self.numrecs = self.u32()
        self.dims = []
        tag, count = self.u32(), self.u32()
        if tag not in (0, _NC_DIMENSION) or (tag == 0 and count):
            raise ValueError("malformed dimension list")
        for _ in range(count):
            name = self.name()
            self.dims.append((name, self.u32()))
        self.attrs = self.attr_list()
        self.vars = {}
        tag, count = self.u32(), self.u32()
        if tag not in (0, _NC_VARIABLE) or (tag == 0 and count):
            raise ValueError("malformed variable list")
        for _ in range(count):
            name = self.name()
            dimids = [self.u32() for _ in range(self.u32())]
            attrs = self.attr_list()
            typ = self.u32()
            self.u32()      # vsize: not relied on
            begin = struct.unpack_from('>Q' if self.wide else '>I', self.take(8 if self.wide else 4))[0]
            if typ not in _NC_SIZE or any(d >= len(self.dims) for d in dimids):
                raise ValueError(f"malformed variable {name}")
            record = bool(dimids) and self.dims[dimids[0]][1] == 0
            shape = [self.dims[d][1] for d in (dimids[1:] if record else dimids)]
            self.vars[name] = {'dimids': dimids, 'attrs': attrs, 'type': typ, 'begin': begin, 'shape': shape, 'record': record,
                               'bytes': int(np.prod(shape, dtype=np.int64)) * _NC_SIZE[typ]}
        recvars = [v for v in self.vars.values() if v['record']]
        # a record holds every record variable padded to 4 bytes; a single record variable is not padded
        self.recsize = recvars[0]['bytes'] if len(recvars) == 1 else sum(_pad4(v['bytes']) for v in recvars)
        self.rec0 = min((v['begin'] for v in recvars), default=0)

    def take(self, n):
        if self.pos + n > len(self.buf):
            raise struct.error("header continues beyond the buffer")
        b = self.buf[self.pos:self.pos + n]
        self.pos += n
        return b

    def u32(self):
        return struct.unpack('>I', self.take(4))[0]

    def name(self):
        n = self.u32()
        return bytes(self.take(_pad4(n))[:n]).decode('utf-8', 'replace')

    def attr_list(self):
        tag, count = self.u32(), self.u32()
        if tag not in (0, _NC_ATTRIBUTE) or (tag == 0 and count):
            raise ValueError("malformed attribute list")
        out = {}
        for _ in range(count):
            name, typ, n = self.name(), self.u32(), self.u32()
            if typ not in _NC_SIZE:
                raise ValueError(f"attribute {name} has the unknown type {typ}")
            raw = bytes(self.take(_pad4(n * _NC_SIZE[typ]))[:n * _NC_SIZE[typ]])
            out[name] = raw.decode('utf-8', 'replace').rstrip('\x00') if typ == 2 else np.frombuffer(raw, _NC_CODE[typ])
        return out


class NetCDFTrajectory(_Trajectory):
    """Amber NetCDF trajectory (convention "AMBER") in the classic NetCDF-3 format: big-endian, ``coordinates(frame, atom,
    spatial)`` float32 and optionally ``cell_lengths`` / ``cell_angles`` (float64, degrees) among the record variables."""
    format = 'NetCDF'
    big_endian = True

    def __init__(self, path):
        self.path = str(path)
        size = os.path.getsize(self.path)
        want = 1 << 16
        while True:
            with open(self.path, 'rb') as f:
                buf = f.read(want)
            if buf[:4] == b'\x89HDF':
                raise TrajectoryError(f"{self.path}: an HDF5-based NetCDF-4 file; NetCDF-4 trajectories must be converted to "
                                      "NetCDF-3 (classic or 64-bit offset)")
            if buf[:3] != b'CDF' or buf[3:4] not in (b'\x01', b'\x02'):
                raise TrajectoryError(f"{self.path}: not a NetCDF-3 file (magic {buf[:4]!r})")
            try:
                h = _NCHeader(buf)
                break
            except struct.error:
                if want >= size:
                    raise TrajectoryError(f"{self.path}: truncated NetCDF header") from None
                want *= 4
            except ValueError as err:
                raise TrajectoryError(f"{self.path}: {err}") from None
        self.header = h
        co = h.vars.get('coordinates')
        if co is None:
            raise TrajectoryError(f"{self.path}: no 'coordinates' variable: not an Amber NetCDF trajectory")
        if not co['record'] or len(co['shape']) != 2:
            raise TrajectoryError(f"{self.path}: 'coordinates' must have the dimensions (frame, atom, spatial)")
        if co['shape'][1] != 3:
            raise TrajectoryError(f"{self.path}: the spatial dimension of 'coordinates' is {co['shape'][1]}, not 3")
        if co['type'] != 5:
            raise TrajectoryError(f"{self.path}: 'coordinates' must be float32")
        sf = co['attrs'].get('scale_factor')
        if sf is not None and not (np.size(sf) == 1 and float(np.asarray(sf).reshape(-1)[0]) == 1.0):
            raise TrajectoryError(f"{self.path}: 'coordinates' has a scale_factor other than 1 ({np.asarray(sf).tolist()}); "
                                  "it is not applied, so the file is refused")
        self.n_atoms = int(co['shape'][0])
        if self.n_atoms < 1:
            raise TrajectoryError(f"{self.path}: no atoms")
        self._first, self._frame_stride = h.rec0, h.recsize
        c0 = co['begin'] - h.rec0
        self._off, self._elem_stride = (c0, c0 + 4, c0 + 8), 12
        lo, hi = c0, c0 + co['bytes']
        self._cell = None
        cl, ca = h.vars.get('cell_lengths'), h.vars.get('cell_angles')
        if cl is not None and ca is not None:
            for v in (cl, ca):
                if not v['record'] or v['type'] != 6 or v['shape'] != [3]:
                    raise TrajectoryError(f"{self.path}: cell_lengths and cell_angles must be float64 (frame, 3)")
            self._cell = (cl['begin'] - h.rec0, ca['begin'] - h.rec0)
            lo, hi = min(lo, *self._cell), max(hi, self._cell[0] + 24, self._cell[1] + 24)
        self.has_box = self._cell is not None
        self._span = (lo, hi - lo)
        avail = max(0, size - h.rec0) // h.recsize
        self.n_frames = avail if h.numrecs == _NC_STREAMING else h.numrecs
        if self.n_frames > avail:
            warnings.warn(f"{self.path}: the header announces {self.n_frames} frames, the file holds {avail} complete ones; "
                          f"using {avail}", RuntimeWarning, stacklevel=3)
            self.n_frames = avail

    def decode_cells(self, rows, shift):
        if self._cell is None:
            return None
        part = [np.ascontiguousarray(rows[:, o - shift:o - shift + 24]).view('>f8').astype(np.float64) for o in self._cell]
        return _cell_rows(part[0], part[1])


def _nc_name(s):
    b = s.encode()
    return struct.pack('>I', len(b)) + b.ljust(_pad4(len(b)), b'\x00')


def _nc_text_attr(name, text):
    b = text.encode()
    return _nc_name(name) + struct.pack('>II', 2, len(b)) + b.ljust(_pad4(len(b)), b'\x00')


def write_netcdf(path, frames, dimensions=None):
    """Write ``frames`` [T, n, 3] float32 (Angstrom) as an Amber NetCDF-3 trajectory: ``time`` and ``coordinates``, and with
    ``dimensions`` ([6] or [T, 6], degrees) ``cell_lengths`` and ``cell_angles``.  The 64-bit offset form is used when the file
    reaches 2 GiB."""
    fr = _frames_array(frames)
    T, n = fr.shape[:2]
    dims = _dimension_rows(dimensions, T)
    dim_list = [('frame', 0), ('spatial', 3), ('atom', n)]
    if dims is not None:
        dim_list += [('cell_spatial', 3), ('cell_angular', 3), ('label', 5)]
    did = {name: i for i, (name, _) in enumerate(dim_list)}
    # (name, dims, type, bytes per record or in all, attributes, fixed data)
    variables = [('spatial', ['spatial'], 2, 3, b'', b'xyz'),
                 ('time', ['frame'], 5, 4, _nc_text_attr('units', 'picosecond'), None),
                 ('coordinates', ['frame', 'atom', 'spatial'], 5, 12 * n, _nc_text_attr('units', 'angstrom'), None)]
    fields = [('time', '>f4'), ('coordinates', '>u4', (n, 3))]
    if dims is not None:
        variables += [('cell_spatial', ['cell_spatial'], 2, 3, b'', b'abc'),
                      ('cell_angular', ['cell_angular', 'label'], 2, 15, b'', b'alphabeta gamma'),
                      ('cell_lengths', ['frame', 'cell_spatial'], 6, 24, _nc_text_attr('units', 'angstrom'), None),
                      ('cell_angles', ['frame', 'cell_angular'], 6, 24, _nc_text_attr('units', 'degree'), None)]
        fields += [('cell_lengths', '>f8', (3,)), ('cell_angles', '>f8', (3,))]
    rec = np.dtype(fields)
    gatts = b''.join(_nc_text_attr(k, v) for k, v in (('title', 'nmrgnn_amd trajectory'), ('application', 'nmrgnn_amd'),
                                                      ('program', 'nmrgnn_amd'), ('programVersion', '1.0'),
                                                      ('Conventions', 'AMBER'), ('ConventionVersion', '1.0')))

    def header(wide, begins):
        out = [b'CDF\x02' if wide else b'CDF\x01', struct.pack('>I', T),
               struct.pack('>II', _NC_DIMENSION, len(dim_list))]
        out += [_nc_name(name) + struct.pack('>I', length) for name, length in dim_list]
        out += [struct.pack('>II', _NC_ATTRIBUTE, 6), gatts, struct.pack('>II', _NC_VARIABLE, len(variables))]
        for (name, vdims, typ, nbytes, atts, _), begin in zip(variables, begins):
            out.append(_nc_name(name) + struct.pack('>I', len(vdims)) + b''.join(struct.pack('>I', did[d]) for d in vdims))
            out.append(struct.pack('>II', _NC_ATTRIBUTE, 1) + atts if atts else struct.pack('>II', 0, 0))
            out.append(struct.pack('>II', typ, _pad4(nbytes)) + struct.pack('>Q' if wide else '>I', begin))
        return b''.join(out)

    for wide in (False, True):
        pos = len(header(wide, [0] * len(variables)))
        begins = []
        for v in variables:                         # the fixed variables first, then the record variables in their order
            if v[5] is not None:
                begins.append(pos)
                pos += _pad4(v[3])
            else:
                begins.append(None)
        rec0 = pos
        for k, v in enumerate(variables):
            if v[5] is None:
                begins[k] = pos
                pos += v[3]
        if wide or rec0 + T * rec.itemsize < (1 << 31):
            break
    with open(path, 'wb') as f:
        f.write(header(wide, begins))
        for v in variables:
            if v[5] is not None:
                f.write(v[5].ljust(_pad4(v[3]), b'\x00'))
        step = max(1, (64 << 20) // rec.itemsize)
        for t0 in range(0, T, step):
            part = fr[t0:t0 + step]
            buf = np.zeros(len(part), rec)
            buf['time'] = np.arange(t0, t0 + len(part), dtype=np.float32)
            buf['coordinates'] = part.view(np.uint32)
            if dims is not None:
                buf['cell_lengths'] = dims[t0:t0 + step, :3]
                buf['cell_angles'] = dims[t0:t0 + step, 3:]
            f.write(buf.tobytes())


# ------------------------------------------------------------------------------------------------------------ opening

def open_trajectory(path):
    """The reader of ``path``, chosen by the file's magic bytes (not by its suffix): ``DCDTrajectory`` or
    ``NetCDFTrajectory``.  A reader is returned as it is."""
    if isinstance(path, _Trajectory):
        return path
    with open(path, 'rb') as f:
        magic = f.read(8)
    if magic[:3] == b'CDF' or magic[:4] == b'\x89HDF':
        return NetCDFTrajectory(path)
    return DCDTrajectory(path)


def load_structure(topology, *trajectories, stride=1):
    """A ``Structure`` with host frames: the atoms of the PDB ``topology`` and every ``stride``-th frame of the trajectory
    files in order (as ``md.Universe(topology, *trajectories)``: the topology's own coordinates are not a frame).  Without
    trajectory files it is ``read_pdb(topology)`` at that stride."""
    from .structure import Structure, read_pdb
    top = read_pdb(topology)
    if not trajectories:
        keep = range(0, len(top), stride)
        return Structure(top.names, top.resnames, top.resids, top.elements, [top.frames[k] for k in keep],
                         [top.dimensions[k] for k in keep])
    frames, dims = [], []
    for p in trajectories:
        t = open_trajectory(p)
        if t.n_atoms != top.n_atoms:
            raise ValueError(f"{t.path}: {t.n_atoms} atoms, but {topology} has {top.n_atoms}")
        frames.append(t.read())
        d = t.dimensions()
        dims.extend([None] * t.n_frames if d is None else [None if np.isnan(r).any() else r for r in d])
    frames = np.concatenate(frames)[::stride]
    return Structure(top.names, top.resnames, top.resids, top.elements, list(frames), dims[::stride])


# ---------------------------------------------------------------------------------------------------------- streaming

def _select_indices(select, n):
    """int32 [n_sel] atom indices of a mask or an index array, checked once against [0, n); None stays None"""
    if select is None:
        return None
    s = np.asarray(select)
    if s.dtype == bool:
        if s.shape != (n,):
            raise ValueError(f"select: a mask needs {n} entries, got {s.shape}")
        s = np.nonzero(s)[0]
    s = s.astype(np.int64).reshape(-1)
    if len(s) and (s.min() < 0 or s.max() >= n):
        raise IndexError(f"select: atom index outside [0, {n})")
    return s.astype(np.int32)


class TrajectoryStream:
    """Iterate over a trajectory in chunks of ``chunk_frames`` frames: ``(frame_ids int64 [G], positions float32 [G, n_sel, 3]
    on ``device``, dimensions float64 [G, 6] or None)``.

    ``frames``: the frame numbers to visit (None: all), of which every ``stride``-th is taken.  ``select``: a mask or an index
    array of atoms (any order, repeats allowed), validated here once.

    On a GPU the file's bytes go through two pinned staging buffers.  One reader thread does file I/O only (``readinto`` a
    staging buffer; consecutive frames in one read, other frames one span each into consecutive slots) and makes no GPU call.
    The calling thread queues, on the current stream, the copy of the staged bytes, ``ng_frames_decode`` and the read-back of
    its count of non-finite values, waits on an event behind them, decodes the chunk's cell records on the host from the
    staged bytes and only then hands the buffer back to the reader — which therefore fills one buffer while the consumer works
    on the chunk from the other.  A non-finite coordinate (also what a wrong byte order gives) raises ``TrajectoryError``
    naming the first bad frame.  On a CPU device the stream is ``traj.read`` per chunk."""

    def __init__(self, traj, frames=None, stride=1, select=None, chunk_frames=32, device=None, chunks=None):
        import torch
        self.traj = open_trajectory(traj)
        if int(stride) < 1 or int(chunk_frames) < 1:
            raise ValueError("TrajectoryStream: stride and chunk_frames must be >= 1")
        self.select = _select_indices(select, self.traj.n_atoms)
        self.n_out = self.traj.n_atoms if self.select is None else len(self.select)
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        if chunks is not None:          # an explicit partition (eval-struct: batches that span trajectory files)
            self.chunks = [self.traj.frame_ids(c) for c in chunks if len(c)]
        else:
            ids = self.traj.frame_ids(frames)[::int(stride)]
            self.chunks = [ids[i:i + int(chunk_frames)] for i in range(0, len(ids), int(chunk_frames))]
        self.frame_ids = np.concatenate(self.chunks) if self.chunks else np.zeros(0, np.int64)
        lay = self.traj.layout()
        biggest = max((len(c) for c in self.chunks), default=0)
        if biggest * lay['frame_stride'] > _CHUNK_LIMIT:
            raise ValueError(f"TrajectoryStream: {biggest} frames of {lay['frame_stride']} bytes reach 2^31 bytes; use at most "
                             f"{_CHUNK_LIMIT // lay['frame_stride']} frames per chunk")
        self._capacity = max(biggest * lay['frame_stride'], 4)

    def __len__(self):
        return len(self.chunks)

    def __iter__(self):
        if self.device.type != 'cuda':
            return self._iter_host()
        return self._iter_device()

    def _iter_host(self):
        import torch
        for ids in self.chunks:
            pos = self.traj.read(ids)
            if self.select is not None:
                pos = pos[:, self.select]
            yield ids, torch.from_numpy(np.ascontiguousarray(pos)), self.traj.dimensions(ids)

    def _reader(self, views, free, ready, lay):
        """the reader thread: file bytes into the staging buffers, nothing else"""
        try:
            fs, (s0, sb) = lay['frame_stride'], lay['span']
            with open(self.traj.path, 'rb', buffering=0) as f:
                for k, ids in enumerate(self.chunks):
                    b = free.get()
                    if b is None:
                        return
                    G = len(ids)
                    whole = G == 1 or bool((np.diff(ids) == 1).all())
                    if whole:
                        spans = [(lay['first'] + int(ids[0]) * fs, 0, G * fs)]
                    else:
                        spans = [(lay['first'] + int(fr) * fs + s0, j * sb, sb) for j, fr in enumerate(ids)]
                    for src, dst, nbytes in spans:
                        f.seek(src)
                        view = memoryview(views[b])[dst:dst + nbytes]
                        got = 0
                        while got < nbytes:
                            r = f.readinto(view[got:])
                            if not r:
                                raise IOError(f"{self.traj.path}: the file ends inside frame data (it changed while open)")
                            got += r
                    ready.put((b, k, whole))
        except BaseException as err:        # handed to the calling thread, which raises it
            ready.put(err)

    def _iter_device(self):
        import torch
        from . import _lib
        from ._lib import ptr
        dev, lay = self.device, self.traj.layout()
        if not self.chunks:
            return
        ctx = _lib.get_context(dev.index)
        fs, (s0, sb) = lay['frame_stride'], lay['span']
        stage = [torch.empty(self._capacity, dtype=torch.uint8).pin_memory() for _ in range(2)]
        views = [s.numpy() for s in stage]
        raw = torch.empty(self._capacity, dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        bad_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        sel = None if self.select is None else torch.from_numpy(self.select).to(dev)
        done = torch.cuda.Event()
        free, ready = queue.Queue(), queue.Queue()
        free.put(0)
        free.put(1)
        reader = threading.Thread(target=self._reader, args=(views, free, ready, lay), name='trajectory-reader', daemon=True)
        reader.start()
        try:
            for _ in self.chunks:
                item = ready.get()
                if isinstance(item, BaseException):
                    raise item
                b, k, whole = item
                ids = self.chunks[k]
                G = len(ids)
                slot, shift = (fs, 0) if whole else (sb, s0)
                nbytes = G * slot
                out = torch.empty((G, self.n_out, 3), dtype=torch.float32, device=dev)
                with torch.cuda.device(dev):
                    raw[:nbytes].copy_(stage[b][:nbytes], non_blocking=True)
                    bad.zero_()
                    st = _lib._vp(torch.cuda.current_stream(dev).cuda_stream)
                    ctx.check(ctx.lib.ng_frames_decode(ctx.handle, st, ptr(raw), nbytes, G, slot, lay['off'][0] - shift,
                                                       lay['off'][1] - shift, lay['off'][2] - shift, lay['elem_stride'],
                                                       lay['swap'], self.traj.n_atoms, ptr(sel), self.n_out, ptr(out), ptr(bad)),
                              "ng_frames_decode")
                    bad_host.copy_(bad, non_blocking=True)
                    done.record()
                done.synchronize()      # the copy has left the staging buffer, and the count has arrived
                dims = self.traj.decode_cells(views[b][:nbytes].reshape(G, slot), shift) if self.traj.has_box else None
                free.put(b)
                if int(bad_host[0]):
                    per_frame = torch.isfinite(out).reshape(G, -1).all(dim=1).cpu().numpy()
                    first = int(ids[int(np.argmin(per_frame))])
                    raise TrajectoryError(f"{self.traj.path}: frame {first} holds a coordinate that is not finite "
                                          f"({int(bad_host[0])} such values in its chunk); a damaged file or a wrong byte order")
                yield ids, out, dims
        finally:
            free.put(None)
            reader.join()


# ---------------------------------------------------------------------------------------------------- frame sources

class TrajectoryUniverse:
    """The atoms of a topology ``Structure`` with the frames of binary trajectory files in order: what ``_open_structure``
    returns for ``top.pdb traj.dcd ...``.  ``len()`` is the number of frames, ``frames[i]`` reads frame i on the host,
    ``dimensions[i]`` is its box or None."""

    def __init__(self, topology, trajectories, label='topology'):
        self.names, self.resnames, self.resids, self.elements = (topology.names, topology.resnames, topology.resids,
                                                                 topology.elements)
        self.trajectories = [open_trajectory(t) for t in trajectories]
        for t in self.trajectories:
            if t.n_atoms != topology.n_atoms:
                raise ValueError(f"{t.path}: {t.n_atoms} atoms, but {label} has {topology.n_atoms}")
        self.starts = np.concatenate([[0], np.cumsum([t.n_frames for t in self.trajectories])]).astype(np.int64)
        self.frames = _HostFrames(self)
        self._dims = None

    @property
    def n_atoms(self):
        return len(self.names)

    def __len__(self):
        return int(self.starts[-1])

    def locate(self, frame_ids):
        """(file number, frame number inside it) of global frame numbers"""
        ids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        k = np.searchsorted(self.starts, ids, side='right') - 1
        return k, ids - self.starts[k]

    @property
    def dimensions(self):
        if self._dims is None:
            self._dims = []
            for t in self.trajectories:
                d = t.dimensions()
                self._dims.extend([None] * t.n_frames if d is None else [None if np.isnan(r).any() else r for r in d])
        return self._dims


class _HostFrames:
    def __init__(self, u):
        self.u = u

    def __len__(self):
        return len(self.u)

    def __getitem__(self, i):
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        k, local = self.u.locate([i % len(self)])
        return self.u.trajectories[int(k[0])].read(local)[0]


class StructureFrames:
    """Frame source over the host frames of a ``Structure`` (a PDB): ``chunks(partition, device)`` yields ``(frame_ids,
    positions [G, n, 3], boxes)`` with ``boxes`` a list of [6] arrays or None per frame."""

    def __init__(self, u):
        self.u = u

    def boxes(self, frame_ids):
        return [self.u.dimensions[fr] for fr in frame_ids]

    def chunks(self, partition, device=None):
        for ids in partition:
            yield ids, np.stack([self.u.frames[fr] for fr in ids]), self.boxes(ids)


class TrajectoryFrames:
    """Frame source over a ``TrajectoryUniverse``: the same chunks as ``StructureFrames``, their positions decoded on the device
    by one ``TrajectoryStream`` per file.  A chunk that spans two files is the concatenation of its parts."""

    def __init__(self, u):
        self.u = u

    def boxes(self, frame_ids):
        return [self.u.dimensions[fr] for fr in frame_ids]

    def chunks(self, partition, device=None):
        import torch
        partition = [np.asarray(c, dtype=np.int64) for c in partition]
        where = [self.u.locate(c) for c in partition]
        want = iter(range(len(partition)))
        cur, parts = next(want, None), []
        for k, traj in enumerate(self.u.trajectories):
            subs = [local[file == k] for file, local in where]
            for _, pos, dims in TrajectoryStream(traj, chunks=subs, device=device):
                while cur is not None and len(partition[cur]) == 0:
                    cur = next(want, None)
                parts.append((pos, dims))
                if sum(len(p) for p, _ in parts) == len(partition[cur]):
                    ids = partition[cur]
                    pos = parts[0][0] if len(parts) == 1 else torch.cat([p for p, _ in parts])
                    boxes = []
                    for p, d in parts:
                        boxes.extend([None] * len(p) if d is None else [None if np.isnan(r).any() else r for r in d])
                    yield [int(i) for i in ids], pos, boxes
                    cur, parts = next(want, None), []


def frame_source(u):
    """the frame source of what ``_open_structure`` returned"""
    return TrajectoryFrames(u) if isinstance(u, TrajectoryUniverse) else StructureFrames(u)
