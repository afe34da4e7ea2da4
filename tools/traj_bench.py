"""Trajectory input measurements: the ten frames of tests/data/7lgi.pdb.gz tiled to a FRAMES-frame trajectory
with a small jitter, written as a multi-MODEL PDB, a DCD and an Amber NetCDF file into a temporary directory.

  host    read_pdb against traj.read for the same frames: host wall clock, no GPU involved
  decode  ng_frames_decode against the host-to-device copy it follows, per chunk of 32 frames: device events around each,
          the median of REPS repeats after a warm-up
  eval    eval-struct --average from each of the three files: host wall clock around the whole call (it ends in device-to-
          host copies, so in a synchronise) and its three timing buckets; every file is run ROUNDS times, alternating

  python tools/traj_bench.py [--frames 1000] [--parts host,decode,eval] [--rounds 2]

Needs the GPU for decode and eval; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nmrgnn_amd.structure import read_pdb  # noqa: E402
from nmrgnn_amd.trajectory import open_trajectory, write_dcd, write_netcdf  # noqa: E402


def write_pdb(path, s, frames):
    head = []
    for k in range(s.n_atoms):
        nm = s.names[k] if len(s.names[k]) == 4 else " " + s.names[k]
        head.append("ATOM  %5d %-4s %3s A%4d    " % ((k + 1) % 100000, nm, s.resnames[k], s.resids[k]))
    tail = ["  1.00  0.00          %2s\n" % e for e in s.elements]
    with open(path, "w") as f:
        for m, fr in enumerate(frames):
            f.write("MODEL     %4d\n" % ((m + 1) % 10000))
            f.write("".join("%s%8.3f%8.3f%8.3f%s" % (head[k], fr[k, 0], fr[k, 1], fr[k, 2], tail[k]) for k in range(s.n_atoms)))
            f.write("ENDMDL\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--parts", default="host,decode,eval")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    parts = args.parts.split(",")
    warnings.simplefilter("ignore")
    s = read_pdb(os.path.join(ROOT, "tests", "data", "7lgi.pdb.gz"))
    rng = np.random.default_rng(7)
    T, n = args.frames, s.n_atoms
    # three decimals, as the PDB text holds them: the three files carry the same float32 values
    frames = np.stack([np.round(s.frames[i % len(s)].astype(np.float64) + rng.normal(0, 0.05, (n, 3)), 3) for i in range(T)])
    frames32 = frames.astype(np.float32)
    with tempfile.TemporaryDirectory() as d:
        files = {"pdb": os.path.join(d, "traj.pdb"), "dcd": os.path.join(d, "traj.dcd"), "netcdf": os.path.join(d, "traj.nc")}
        top = os.path.join(d, "top.pdb")
        write_pdb(files["pdb"], s, frames)
        write_pdb(top, s, frames[:1])
        write_dcd(files["dcd"], frames32)
        write_netcdf(files["netcdf"], frames32)
        print(json.dumps({"frames": T, "atoms": n, "bytes": {k: os.path.getsize(v) for k, v in files.items()}}))

        if "host" in parts:
            t = time.perf_counter()
            u = read_pdb(files["pdb"])
            host = {"read_pdb_s": time.perf_counter() - t}
            assert len(u) == T
            for k in ("dcd", "netcdf"):
                best = []
                for _ in range(3):
                    t = time.perf_counter()
                    got = open_trajectory(files[k]).read()
                    best.append(time.perf_counter() - t)
                assert np.array_equal(got.view(np.uint32), np.stack(u.frames).view(np.uint32))
                host[f"read_{k}_s"] = min(best)
            host["how"] = "host wall clock; read_pdb once, traj.read the best of 3 (file in the page cache)"
            print(json.dumps({"host": host}))
            del u

        if "decode" in parts:
            import torch
            from nmrgnn_amd import _lib
            dev = torch.device("cuda", 0)
            ctx = _lib.get_context(0)
            out = {}
            for k in ("dcd", "netcdf"):
                traj = open_trajectory(files[k])
                lay, G = traj.layout(), min(32, T)
                nbytes = G * lay["frame_stride"]
                stage = torch.from_numpy(np.fromfile(files[k], np.uint8, nbytes, offset=lay["first"])).pin_memory()
                raw = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                pos = torch.empty((G, n, 3), dtype=torch.float32, device=dev)
                bad = torch.zeros(1, dtype=torch.int32, device=dev)
                st = _lib._vp(torch.cuda.current_stream(dev).cuda_stream)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                copy_ms, kernel_ms = [], []
                for rep in range(args.reps + 5):
                    ev[0].record()
                    raw.copy_(stage, non_blocking=True)
                    ev[1].record()
                    ctx.check(ctx.lib.ng_frames_decode(ctx.handle, st, _lib.ptr(raw), nbytes, G, lay["frame_stride"], *lay["off"],
                                                       lay["elem_stride"], lay["swap"], n, None, n, _lib.ptr(pos), _lib.ptr(bad)),
                              "ng_frames_decode")
                    ev[2].record()
                    torch.cuda.synchronize(dev)
                    if rep >= 5:
                        copy_ms.append(ev[0].elapsed_time(ev[1]))
                        kernel_ms.append(ev[1].elapsed_time(ev[2]))
                assert int(bad.cpu()[0]) == 0
                assert np.array_equal(pos.cpu().numpy().view(np.uint32), frames32[:G].view(np.uint32))
                out[k] = {"chunk_frames": G, "chunk_bytes": nbytes, "copy_ms": statistics.median(copy_ms),
                          "decode_ms": statistics.median(kernel_ms),
                          "decode_GBps_read_plus_written": (nbytes + pos.numel() * 4) / statistics.median(kernel_ms) / 1e6}
            out["how"] = f"device events around the pinned-memory copy and around the launch, median of {args.reps} after 5 warm-up repeats"
            print(json.dumps({"decode": out}))

        if "eval" in parts:
            from nmrgnn_amd.main import eval_structure
            quiet = dict(keep_going=True, echo=lambda *a: None, average=True)
            runs = {"pdb": [files["pdb"]], "dcd": [top, files["dcd"]], "netcdf": [top, files["netcdf"]]}
            eval_structure([top], os.path.join(d, "warm.csv"), **quiet)        # code objects, weight images
            res = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, fl in runs.items():
                    t = time.perf_counter()
                    timing = eval_structure(fl, os.path.join(d, f"{k}.csv"), **quiet)
                    res[k].append({"wall_s": time.perf_counter() - t, **{b: round(v, 4) for b, v in timing.items()}})
            same = len({open(os.path.join(d, f"{k}.csv"), "rb").read() for k in runs}) == 1
            print(json.dumps({"eval_average": res, "same_csv": same,
                              "how": "host wall clock around eval_structure(average=True), 32 frames per batch; the buckets are its own; "
                                     "the PDB wall time includes read_pdb"}))


if __name__ == "__main__":
    main()
