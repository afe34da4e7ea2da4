#!/usr/bin/env python
"""bench.py — atoms/s (fwd+bwd+Adam) of the nmrgnn message-passing hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--scaling weak|strong --total-graphs G]
    python bench.py ... --dump-outputs DIR     also writes the last timed step's loss, updated parameters and
                                               gradients as DIR/<name>.npy (same arguments -> same inputs)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
Without a torchrun environment `--gpus N` (N > 1) re-executes itself under torch.distributed.run on 127.0.0.1 with N
ranks; a world size different from --gpus, or a backend other than nccl (= RCCL), is an error, not a warning.

Workload (BASELINE.json configs[2]/[3]): per GPU 512 synthetic graphs x 256 atoms
(N = 131,072 atom rows), K = 16 neighbours, F = 64, E = 3, H = 128, 4 MP / 4 edge-FC / 4 FC layers,
fp32, noise + dropout on, weighted-MSE NameLoss (s = 1), Adam(lr 1e-4).  One "step" = forward +
loss + backward + gradient all-reduce (N > 1) + Adam over one batch already resident in HBM.
Weak scaling (default): per-GPU work is fixed; ranks hold different graphs (seed 42 + rank).
Strong scaling (--scaling strong --total-graphs 4096, the north star's 8-GPU configuration): the total is fixed and
rank r holds the contiguous shard parallel.shard_range(total, r, world) of the same 4096 graphs.

Prints ONE JSON line on rank 0 with `value` = whole-job atoms/s, plus
  roofline     — dominant kernel: algorithmic flops per launch / its mean launch duration
                 (hipEvent-bracketed inside the C library on the launch stream) vs the fp32 MFMA peak
  roofline_all — the same for every profiled kernel (HBM-bound ones against 8 TB/s)
  cpu_baseline — the reference's op order restated in torch-CPU fp32 (oracle/torch_ref.py; TensorFlow
                 is not installed) timed on this box's host cores on a bounded sample of the workload.
  f256         — the same step at the reference's DEFAULT width (atom_feature_size 256) with its own roofline row
  configs4     — whole-protein inference (7lgi, 100 jittered frames, GPU graph build + model, F = 256)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# the host driver only supports dmabuf IPC: without this RCCL fails with hipIpcGetMemHandle: invalid argument
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch
import torch.distributed as dist

PEAK_MFMA_F32_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_MFMA_F16_TFLOPS = 2516.6   # dense fp16 (= bf16): 256 CU x 4 SIMD x 1024 flop/cycle x 2.4 GHz; tools/ubench/mfma_f16.hip
# kernels that run fp32 arithmetic on the fp16 pipe with two pieces per operand, 3 piece products per multiply (the
# default edge kernels): ALGORITHMIC fp32 flops against fp16 peak / 3.  Round 2 started with three bf16 pieces and 6
# products (peak / 6): the matrix pipe now does half the work for the same algorithmic flops, so `frac` (matrix-pipe
# share of the kernel time) is LOWER for a FASTER kernel: the remainder is VALU issue time (softplus, splits, RBF),
# which adds to matrix time on a gfx950 SIMD.
H2_KERNELS = {"edge_fwd_h2", "edge_bwd_h2"}
# window kernels whose matrix phase runs on the fp16 pipe unless NG_GEMM_MATH=fp32 (mp_win.hip)
H2_WINDOW_KERNELS = {"mp_win_fwd", "mp_win_bwd_edge", "mp_win_bwd_node"}
# the fused FC block at F = 64 (fc_fused.hip: fc_h2_on()) runs on fp16 pieces as well unless NG_GEMM_MATH=fp32 — priced against
# the pipe it uses (round-4 verdict: it was priced at the f32-input peak, 0.45 instead of 0.085)
H2_FC_KERNELS = {"fc_fused_fwd", "fc_fused_bwd"}
PEAK_HBM_GBS = 8000.0          # spec; ~6300 achievable

ARCH = dict(atom_feature_size=64, edge_feature_size=3, edge_hidden_size=128, mp_layers=4,
            fc_layers=4, edge_fc_layers=4)
GRAPHS_PER_GPU, ATOMS_PER_GRAPH, K_NEIGH, NUM_ELEM = 512, 256, 16, 10


def kernel_work(N, K, F, E, H, Le, L, Lf, C, live_edges=None):
    """ALGORITHMIC work per launch of each profiled kernel: (bound, flops, bytes)  (DESIGN.md §4).
    ``live_edges``: slots with edges > 0 — the fused edge kernels walk only those (round 4), so their work is priced per
    LIVE edge; every other kernel sees all N*K slots."""
    ne = N * K if live_edges is None else int(live_edges)
    Fh = F // 2
    KF = E * F
    f4 = 4.0
    w = {
        # fused edge kernels (edge_fused.hip)
        "edge_fused_fwd": ("mfma", 2.0 * ne * ((Le - 1) * H * H + H * E),
                           f4 * ne * (1 + 1 + E + (Le - 1) * H)),
        "edge_fwd_h2": ("mfma", 2.0 * ne * ((Le - 1) * H * H + H * E),
                        f4 * ne * (1 + 1 + E + (Le - 1) * H)),
        "edge_bwd_h2": ("mfma", 2.0 * ne * ((2 * (Le - 1) - 1) * H * H + 2 * H * E),
                        f4 * ne * (1 + 1 + E + (Le - 1) * H)),
        "edge_fused_bwd": ("mfma", 2.0 * ne * ((2 * (Le - 1) - 1) * H * H + 2 * H * E),
                           f4 * ne * (1 + 1 + E + (Le - 1) * H)),
    }
    ne = N * K
    w.update({
        # layered edge path (every slot)
        "rbf": ("hbm", 0.0, f4 * ne * (2 + H)),
        "edge_dense_fwd": ("mfma", 2.0 * ne * H * H, f4 * ne * 2 * H),
        "edge_dense_dx": ("mfma", 2.0 * ne * H * H, f4 * ne * 3 * H),
        "edge_dense_dw": ("mfma", 2.0 * ne * H * H, f4 * ne * 3 * H),
        "edge_out_fwd": ("hbm", 2.0 * ne * H * E, f4 * ne * (H + E + 1)),
        "edge_out_bwd": ("hbm", 4.0 * ne * H * E, f4 * ne * (2 * H + E + 1)),
        "bias_grad": ("hbm", 0.0, f4 * ne * 2 * H),
        # node path
        # (bytes: every tensor the kernel must read or write once; gathered rows counted once)
        "mp_aggregate": ("hbm", 2.0 * N * K * F * E, f4 * N * (F + K + K * E + F * E)),
        "mp_aggregate_csc": ("hbm", 2.0 * N * K * F * E, f4 * N * (F + 2 * K + K * E + F * E)),
        "mp_update_fwd": ("mfma", 2.0 * N * KF * F, f4 * N * (KF + 3 * F + 1)),
        # window-resident fused forward (mp_win.hip): gather + GEMM, the aggregate never leaves the CU
        "mp_win_fwd": ("mfma", 2.0 * N * (K * F * E + KF * F), f4 * N * (3 * F + K + K * E + 1) + f4 * KF * F),
        "mp_win_bwd_edge": ("mfma", 2.0 * N * (KF * F + K * F * E), f4 * N * (4 * F + K + 2 * K * E + 1) + f4 * KF * F),
        "mp_win_bwd_node": ("mfma", 2.0 * N * (K * F * E + 2 * KF * F), f4 * N * (4 * F + 4 * K + 1) + f4 * KF * F),
        "mp_records": ("hbm", 0.0, f4 * N * K * (1 + E + 4)),
        # fused FC block (fc_fused.hip): Lf-1 residual layers F->F and the F->F/2 output layer
        "fc_fused_fwd": ("mfma", 2.0 * N * ((Lf - 1) * F * F + F * Fh), f4 * N * (Lf * F + Fh)),
        "fc_fused_bwd": ("mfma", 4.0 * N * ((Lf - 1) * F * F + F * Fh), f4 * N * ((Lf + 1) * F + 2 * Fh)),
        "mp_fused_fwd": ("hbm", 2.0 * N * (K * F * E + KF * F), f4 * N * (3 * F + K + K * E + 1 + KF)),
        "mp_dw": ("mfma", 2.0 * N * KF * F, f4 * N * (KF + F)),
        "mp_dA": ("mfma", 2.0 * N * KF * F, f4 * N * (3 * F + 1 + KF)),
        "mp_dh": ("mfma", 2.0 * N * KF * F, f4 * N * (KF + 2 * F)),
        "mp_edge_grad": ("hbm", 2.0 * N * K * F * E, f4 * N * (F + K + K * E + F * E)),
        "mp_scatter_pull": ("hbm", 2.0 * N * K * F * E, f4 * N * (2 * F + K + K * E + F * E)),
        "mp_bwd_edge": ("hbm", 2.0 * N * (KF * F + K * F * E), f4 * N * (4 * F + K + K * E + 1)),
        "mp_bwd_node": ("hbm", 2.0 * N * (K * F * E + KF * F), f4 * N * (3 * F + 2 * K + K * E)),
        "dense_fwd": ("mfma", 2.0 * N * F * F, f4 * N * 3 * F),
        "dense_dx": ("mfma", 2.0 * N * F * F, f4 * N * 3 * F),
        "dense_dw": ("mfma", 2.0 * N * F * F, f4 * N * 3 * F),
    })
    # a kernel whose arithmetic intensity is below the ridge (157.3 TF / 6.3 TB/s ~ 25 flop/B) is priced
    # against HBM even when its inner loop is MFMA
    ridge = PEAK_MFMA_F32_TFLOPS * 1e12 / 6.3e12
    for k, (bound, fl, by) in list(w.items()):
        if bound == "mfma" and by > 0 and fl / by < ridge:
            w[k] = ("hbm", fl, by)
    return w


def step_flops_per_atom(K, F, E, H, Le, L, Lf):
    """algorithmic flops per atom of the forward (edge MLP + L MPLayers + FC block + head column), MAC = 2 flop;
    forward + backward = 3 x the forward."""
    fwd = 2.0 * K * ((Le - 1) * H * H + H * E) + L * 2.0 * (K * F * E + F * F * E) + 2.0 * ((Lf - 1) * F * F + F * F / 2) + 2.0 * (F / 2)
    return fwd, 3.0 * fwd


def survey_8d_block(rows, N, K, F, E, H, Le, L, Lf, ms_per_step, n_live):
    """the accounting of SURVEY.md 8(d), beside the per-kernel rows (whose byte counts are the kernels' own operand lists):
      step      whole-step algorithmic flops / measured step time / the fp16-pipe fp32-equivalent peak (2516.6 / 3 TF)
      mp_layer  the MPLayer's 8(d) bytes per atom — forward 4 (2F + K + KE + 1), backward 4 (3F + K + 2KE + 1) — over the time
                of the launches that do that work (backward: edge-side + node-side kernels summed), against 8 TB/s
      tape      what the edge MLP's saved activations move through HBM per step (written by the forward, read by the backward)"""
    t = {r["kernel"]: r for r in rows}
    fwd_fl, all_fl = step_flops_per_atom(K, F, E, H, Le, L, Lf)
    peak = PEAK_MFMA_F16_TFLOPS / 3.0
    out = {"step": {"flops_per_atom": all_fl, "tflop_per_step": all_fl * N / 1e12, "ms_per_step": ms_per_step,
                    "achieved_tflops": all_fl * N / (ms_per_step * 1e-3) / 1e12, "peak_tflops": peak,
                    "frac": all_fl * N / (ms_per_step * 1e-3) / 1e12 / peak}}
    fb, bb = 4.0 * (2 * F + K + K * E + 1), 4.0 * (3 * F + K + 2 * K * E + 1)
    mp = {"fwd_bytes_per_atom": fb, "bwd_bytes_per_atom": bb, "peak_gbs": PEAK_HBM_GBS}
    fwd_k = [k for k in ("mp_win_fwd",) if k in t] or [k for k in ("mp_aggregate", "mp_update_fwd", "mp_fused_fwd") if k in t]
    bwd_k = [k for k in ("mp_win_bwd_edge", "mp_win_bwd_node") if k in t] or \
            [k for k in ("mp_dP", "mp_dA", "mp_edge_grad", "mp_scatter_pull", "mp_dw", "mp_bwd_edge", "mp_bwd_node") if k in t]
    if fwd_k:
        ms = sum(t[k]["ms_per_step"] for k in fwd_k) / L
        mp.update(fwd_kernels=fwd_k, fwd_ms_per_layer=ms, fwd_gbs=fb * N / (ms * 1e-3) / 1e9, fwd_frac=fb * N / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS)
    if bwd_k:
        ms = sum(t[k]["ms_per_step"] for k in bwd_k) / L
        mp.update(bwd_kernels=bwd_k, bwd_ms_per_layer=ms, bwd_gbs=bb * N / (ms * 1e-3) / 1e9, bwd_frac=bb * N / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS)
    out["mp_layer"] = mp
    if n_live is not None:
        out["tape"] = {"bytes_per_step": 2.0 * (Le - 1) * n_live * H * 4.0, "note": "(Le-1) x live edges x H fp32 values, written by "
                       "edge_fwd_h2 and read by edge_bwd_h2: ~97 % of either kernel's HBM bytes"}
    return out


def usable_cores():
    """cores this process may actually run on: affinity mask capped by the cgroup CPU quota"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return n


def cpu_baseline(hp_dict, sample_graphs, seed, budget_s=20.0):
    """reference op order (torch CPU fp32), fwd+bwd+Adam, atoms/s on a bounded sample.
    The intra-op thread count is calibrated (one step each over a few candidates) because the GPU
    box reports far more logical CPUs than a container is allowed to use."""
    from oracle import nmrgnn_oracle as O
    from oracle import torch_ref as R
    from nmrgnn_amd import synth
    cores = usable_cores()
    hp = O.hypers(**hp_dict)
    b = synth.make_batch(sample_graphs, ATOMS_PER_GRAPH, K_NEIGH, NUM_ELEM, 0.05, seed)
    p = R.to_torch_params(O.init_params(hp, NUM_ELEM, dtype=np.float32), dtype=torch.float32,
                          requires_grad=True)
    opt = torch.optim.Adam(list(p.values()), lr=1e-4, eps=1e-7)
    N, K = b["edges"].shape
    gen = torch.Generator().manual_seed(seed)
    gids = torch.as_tensor(np.repeat(np.arange(sample_graphs), ATOMS_PER_GRAPH))
    y, w = torch.as_tensor(b["y"]), torch.as_tensor(b["w"])
    inputs = (b["atoms"], b["nlist"], b["edges"], b["inv_degree"])

    def one(order="ref"):
        xi = torch.randn(N, K, generator=gen)
        mask = (torch.rand(N, hp["atom_feature_size"] // 2, generator=gen) < 0.8).float()
        opt.zero_grad(set_to_none=True)
        pred = R.forward(inputs, p, hp, training=True, noise=xi, dropout_mask=mask, order=order)
        loss = R.batch_loss_s1(y, w, pred, gids, sample_graphs)
        loss.backward()
        opt.step()

    cands = sorted({c for c in (cores, cores // 2, 64, 32, 16, 8) if 1 <= c <= cores}, reverse=True)
    best_thr, best_t = cands[0], float("inf")
    for c in cands:
        torch.set_num_threads(c)
        one()  # warm-up at this setting
        t0 = time.perf_counter()
        one()
        dt = time.perf_counter() - t0
        if dt < best_t:
            best_thr, best_t = c, dt
        if dt > 4 * best_t:
            continue
    torch.set_num_threads(best_thr)
    times = []
    t_all = time.perf_counter()
    while len(times) < 5 or (time.perf_counter() - t_all < budget_s and len(times) < 50):
        t0 = time.perf_counter()
        one()
        times.append(time.perf_counter() - t0)
        if time.perf_counter() - t_all > 3 * budget_s:
            break
    med = float(np.median(times))
    # the same step with the MPLayer contracted in the algorithmic order (aggregate over neighbours, then one GEMM):
    # the reference's own order executes ~6x the flops at F=64, so this is the fairer CPU number
    alt = []
    one("alg")
    for _ in range(3):
        t0 = time.perf_counter()
        one("alg")
        alt.append(time.perf_counter() - t0)
    alt_med = float(np.median(alt))
    return {"value": N / med, "aggregate_then_gemm_value": N / alt_med, "unit": "atoms/s", "cores": best_thr, "cores_available": cores,
            "kind": "port",
            "sample": f"{sample_graphs} graphs x {ATOMS_PER_GRAPH} atoms (one concatenated call), "
                      f"fwd+bwd+Adam, reference op order (lmn,ijl->mnij; mnij,ijn->mi; mi,i->im), "
                      f"torch-CPU fp32 eager, median of {len(times)} runs",
            "ms_per_step": med * 1e3}


def cpu_baseline_protein(budget_s=12.0):
    """configs[4] beside its GPU number: the reference's op order (and the aggregate-then-GEMM order) in torch-CPU fp32,
    forward only, on ONE frame of 7lgi (2770 atoms, kNN-16 lists) at the baseline architecture (F = 256) — the
    configuration the north star states its >= 50x for.  Graph build not included (the reference's is MDAnalysis)."""
    from oracle import nmrgnn_oracle as O
    from oracle import torch_ref as R
    from nmrgnn_amd.structure import atoms_onehot, inv_degree_of, knn_graph, read_pdb
    s = read_pdb(os.path.join(ROOT, "tests", "data", "7lgi.pdb.gz"))
    atoms = atoms_onehot(s.elements)
    nlist, edges = knn_graph(s.frames[0], 16)
    inv = inv_degree_of(nlist)
    hp = O.hypers()
    p = R.to_torch_params(O.init_params(hp, atoms.shape[1], dtype=np.float32), dtype=torch.float32)
    inputs = (atoms, nlist, edges, inv)
    cores = usable_cores()
    best = None
    for thr in sorted({c for c in (cores, 32, 16, 8) if 1 <= c <= cores}, reverse=True):
        torch.set_num_threads(thr)
        with torch.no_grad():
            R.forward(inputs, p, hp, order="ref")
            t0 = time.perf_counter()
            R.forward(inputs, p, hp, order="ref")
            dt = time.perf_counter() - t0
        if best is None or dt < best[1]:
            best = (thr, dt)
    torch.set_num_threads(best[0])
    out = {"cores": best[0], "cores_available": cores, "kind": "port", "unit": "atoms/s",
           "sample": f"one 7lgi frame ({atoms.shape[0]} atoms, K=16), forward only, atom_feature_size 256, torch-CPU fp32 eager"}
    for order, key in (("ref", "value"), ("alg", "aggregate_then_gemm_value")):
        ts, t_all = [], time.perf_counter()
        with torch.no_grad():
            while len(ts) < 3 or (time.perf_counter() - t_all < budget_s / 2 and len(ts) < 30):
                t0 = time.perf_counter()
                R.forward(inputs, p, hp, order=order)
                ts.append(time.perf_counter() - t0)
        out[key] = atoms.shape[0] / float(np.median(ts))
        out[key.replace("value", "ms_per_frame")] = float(np.median(ts)) * 1e3
    return out


# kernels whose generic GEMM runs on the fp16 pipe with two-piece split operands when the shape allows (gemm_h2.hip)
H2_GEMM_TAGS = {"mp_update_fwd", "mp_dw", "mp_dA", "dense_fwd", "dense_dx", "dense_dw", "edge_dense_fwd",
                "edge_dense_dx", "edge_dense_dw"}
# kernel tag -> the source files whose content decides whether a committed PMC number still describes it
KERNEL_SOURCES = {
    "edge_fwd_h2": ["edge_fwd_h2.hip", "h2_common.cuh", "pack_bodies.cuh"],
    "edge_bwd_h2": ["edge_bwd_h2.hip", "edge_bwd_h2.cuh", "h2_common.cuh", "pack_bodies.cuh"],
    "edge_fused_fwd": ["edge_fused.hip"], "edge_fused_bwd": ["edge_fused_bwd.hip"],
    "mp_win_fwd": ["mp_wave.hip", "mp_wave_common.cuh", "mp_win16.hip", "mp_win16_common.cuh", "mp_win.hip", "h2_common.cuh"],
    "mp_win_bwd_edge": ["mp_win16_bwd.hip", "mp_win16_common.cuh", "mp_win_bwd.hip", "h2_common.cuh"],
    "mp_win_bwd_node": ["mp_win_bwd.hip", "mp_win16_common.cuh", "h2_common.cuh"],
    "fc_fused_fwd": ["fc_fused.hip"], "fc_fused_bwd": ["fc_fused.hip"],
    "head_fwd": ["head_ops.hip"], "head_bwd": ["head_ops.hip"], "head_loss": ["head_ops.hip"], "embed_bwd": ["node_ops.hip"], "adam": ["node_ops.hip"],
    "reduce_partials": ["reduce.cuh", "capi.hip"], "mp_records": ["mp_win_bwd.hip"], "repack_all": ["repack.hip", "pack_bodies.cuh"],
}


def source_digest(kernel):
    import hashlib
    h = hashlib.sha256()
    for f in KERNEL_SOURCES.get(kernel, []):
        with open(os.path.join(ROOT, "nmrgnn_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_lookup(kernel):
    """(traffic bytes per launch, matrix-pipe busy share, note) from the rocprofv3 PMC passes committed under
    profiles/ (tools/pmc_traffic.sh, tools/pmc_mfma.sh).  The files carry the digest of the kernel sources they were
    collected on; a number whose kernel has changed since is NOT printed."""
    traffic = busy = coexec = None
    notes = []
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            pmc = json.load(f)
        meta = pmc.get("_meta", {})
        ent = pmc.get(kernel)
        if ent:
            if meta.get("source_digest", {}).get(kernel) == source_digest(kernel):
                # FETCH_SIZE doubled as the MI355X guide prescribes for wide coalesced reads on gfx950
                traffic = 2.0 * ent["FETCH_SIZE_KB"] * 1024 + ent["WRITE_SIZE_KB"] * 1024
                notes.append(f"traffic: profiles/pmc_traffic.json @ {meta.get('commit', '?')}")
            else:
                notes.append("traffic: committed PMC pass predates the current kernel source (stale, not shown)")
    except Exception:
        pass
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_mfma.json")) as f:
            pm = json.load(f)
        meta = pm.get("_meta", {})
        if meta.get("source_digest", {}).get(kernel) == source_digest(kernel):
            for kname, v in pm.items():
                if kname != "_meta" and kernel + "_kernel" in kname and v.get("GRBM_GUI_ACTIVE", 0) > 0:
                    busy = v["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024.0 / (v["GRBM_GUI_ACTIVE"] / 8.0)
                    # share of the matrix pipe's busy cycles during which the SIMD's VALU also executed
                    if v.get("SQ_VALU_MFMA_BUSY_CYCLES", 0) > 0 and "SQ_VALU_MFMA_COEXEC_CYCLES" in v:
                        coexec = v["SQ_VALU_MFMA_COEXEC_CYCLES"] / v["SQ_VALU_MFMA_BUSY_CYCLES"]
                    notes.append(f"mfma_pipe_busy: profiles/pmc_mfma.json @ {meta.get('commit', '?')}")
        elif kernel in meta.get("source_digest", {}):
            notes.append("mfma_pipe_busy: committed PMC pass predates the current kernel source (stale, not shown)")
    except Exception:
        pass
    return traffic, busy, coexec, "; ".join(notes) or None


def roofline_rows(prof, psteps, work, h2_gemm):
    rows = []
    for name, (tot_ms, cnt) in prof.items():
        avg_ms = tot_ms / max(cnt, 1)
        row = {"kernel": name, "launches_per_step": cnt / psteps, "avg_ms": avg_ms, "ms_per_step": tot_ms / psteps}
        if name in work and avg_ms > 0:
            _, fl, by = work[name]
            on_h2 = name in H2_KERNELS or (h2_gemm and name in H2_GEMM_TAGS) or (
                name in (H2_WINDOW_KERNELS | H2_FC_KERNELS) and os.environ.get("NG_GEMM_MATH", "") != "fp32")
            peak_tf = PEAK_MFMA_F16_TFLOPS / 3.0 if on_h2 else PEAK_MFMA_F32_TFLOPS
            # both rooflines, the binding one is reported: floor = max(flops at the matrix peak, bytes at the HBM peak)
            t_mfma = fl / (peak_tf * 1e12) * 1e3 if fl > 0 else 0.0
            t_hbm = by / (PEAK_HBM_GBS * 1e9) * 1e3
            if t_mfma >= t_hbm:
                ach = fl / (avg_ms * 1e-3) / 1e12
                row.update(bound="mfma", achieved=ach, peak=peak_tf, unit="TFLOP/s", frac=ach / peak_tf)
                if on_h2:
                    row["peak_note"] = ("fp32-equivalent: fp16 dense peak 2516.6 / 3 piece products; achieved is "
                                        f"{ach / PEAK_MFMA_F32_TFLOPS:.2f}x the f32-input MFMA peak (157.3)")
            else:
                ach = by / (avg_ms * 1e-3) / 1e9
                row.update(bound="hbm", achieved=ach, peak=PEAK_HBM_GBS, unit="GB/s", frac=ach / PEAK_HBM_GBS)
            row["floor_ms"] = {"mfma": t_mfma, "hbm": t_hbm}
        rows.append(row)
    rows.sort(key=lambda r: -r["ms_per_step"])
    return rows


def profiled_steps(eng, step_fn, psteps):
    eng.ctx.prof_reset()
    eng.ctx.prof_enable(True)
    for _ in range(psteps):
        step_fn()
    torch.cuda.synchronize()
    prof = eng.ctx.prof_read()
    eng.ctx.prof_enable(False)
    eng.ctx.prof_reset()
    return prof


def event_timed(step_fn, n):
    """per-step durations (ms) from hipEvents on the launch stream (the engine launches on torch's current stream)"""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    evs[0].record()
    for i in range(n):
        step_fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]


def collective_library(backend):
    """what torch.distributed is talking through, for the record of a multi-GPU run ("nccl" IS RCCL on ROCm)"""
    if backend != "nccl":
        return backend
    try:
        v = torch.cuda.nccl.version()
        return "rccl " + ".".join(str(x) for x in (v if isinstance(v, tuple) else (v,))) + f" (torch {torch.__version__}, hip {torch.version.hip})"
    except Exception as ex:
        return f"nccl (version unavailable: {ex!r})"


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def relaunch_under_torchrun(n):
    """`python bench.py --gpus N` without a torchrun environment: start the N ranks ourselves"""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=GRAPHS_PER_GPU, help="graphs per GPU (weak scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--total-graphs", type=int, default=4096, help="graphs over all GPUs (strong scaling)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the inference / fp32 / F=256 / configs[4] legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (loss, updated parameters, gradients) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_under_torchrun(args.gpus))

    from nmrgnn_amd import _lib, parallel, synth
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.graph import BatchPrefetcher, GraphBatch
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    from nmrgnn_amd.train import Trainer

    world, rank, local = parallel.init_distributed()
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks", file=sys.stderr)
        sys.exit(2)
    # (a process group can exist in a world of one: NMRGNN_FORCE_COLLECTIVES=1 runs the gradient all-reduces through the real
    # backend on a single-GPU box)
    backend = dist.get_backend() if dist.is_initialized() else None
    if world > 1:
        assert dist.get_world_size() == args.gpus
        if backend != "nccl" and os.environ.get("NMRGNN_DIST_BACKEND") != backend:
            print(f"bench.py: torch.distributed backend is {backend!r}, expected 'nccl' (RCCL)", file=sys.stderr)
            sys.exit(2)
    if backend == "nccl" and torch.cuda.device_count() < world:
        print(f"bench.py: {world} ranks but only {torch.cuda.device_count()} GPUs visible", file=sys.stderr)
        sys.exit(2)
    local = local % torch.cuda.device_count()      # (ranks may share a GPU only in the gloo smoke test)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    hp = declare_gnn_space(HyperParameters(**ARCH))
    eng = Engine(hp, NUM_ELEM, device=dev, seed=1234)          # same weights on every rank
    # `value` and every leg that does not say otherwise: the edge MLP evaluated PER EDGE, as the reference does and as
    # SURVEY 8(d) prices it (a timed region that replaces 2 M MLP evaluations by 4,096 would read as skipped
    # work).  The Engine's default since round 6 — the guarded edge-function table — is measured beside it (`edge_table`).
    eng.edge_table = os.environ.get("NG_BENCH_EDGE_TABLE", "0") == "1"      # (tools/step_trace.sh: the trace of the table-path step)
    if args.scaling == "strong":
        # the SAME total_graphs graphs whatever the world size; this rank's contiguous shard
        lo, hi = parallel.shard_range(args.total_graphs, rank, world)
        full = synth.make_batch(args.total_graphs, ATOMS_PER_GRAPH, K_NEIGH, NUM_ELEM, 0.05, seed=42)
        a, z = lo * ATOMS_PER_GRAPH, hi * ATOMS_PER_GRAPH
        b = dict(atoms=full["atoms"][a:z], nlist=full["nlist"][a:z] - a, edges=full["edges"][a:z],
                 inv_degree=full["inv_degree"][a:z], graph_ptr=full["graph_ptr"][lo:hi + 1] - a, y=full["y"][a:z],
                 w=full["w"][a:z])
        total_graphs = args.total_graphs
        del full
    else:
        b = synth.make_batch(args.graphs, ATOMS_PER_GRAPH, K_NEIGH, NUM_ELEM, 0.05, seed=42 + rank)
        total_graphs = args.graphs * world
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
    torch.cuda.synchronize()
    t_h2d = time.perf_counter() - t0
    # steady state of the per-batch list construction (ng_build_incoming_lists; the first call above also paid the
    # scratch allocation): device tuple in, lists out
    raw = (gb.atoms, gb.nlist, gb.edges, gb.inv_degree)
    ev = event_timed(lambda: GraphBatch(*raw, graph_ptr=b["graph_ptr"], device=dev, validate=False), 5)
    t_csc = float(np.median(ev)) * 1e-3
    y = torch.from_numpy(b["y"]).to(dev)
    w = torch.from_numpy(b["w"]).to(dev)
    tr = Trainer(eng, lr=1e-4)
    tr.measure_comm = world > 1 or (parallel.force_collectives() and dist.is_initialized())

    def step():
        return tr.step(gb, y, w, total_graphs=total_graphs)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        loss = step()
    tr.comm_exposed_ms()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    barrier()
    elapsed_local = time.perf_counter() - t0
    # --dump-outputs: what the LAST timed step handed its caller, copied before any later leg runs another step: the
    # loss Trainer.step returns, the parameters Adam left and the gradient it applied
    dumped = None
    if args.dump_outputs:
        dumped = {"loss": loss.detach().reshape(-1).cpu().numpy()}
        for name, v in eng.params.views.items():
            dumped["param." + name.replace("/", ".")] = v.detach().cpu().numpy()
        for name, v in eng.params.grad_views.items():
            dumped["grad." + name.replace("/", ".")] = v.detach().cpu().numpy()
    elapsed = elapsed_local
    rank_ms = [elapsed_local / args.steps * 1e3]
    if world > 1:
        t = torch.tensor([elapsed_local], dtype=torch.float64, device=dev)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        rank_ms = [float(x.item()) / args.steps * 1e3 for x in allt]
        elapsed = max(float(x.item()) for x in allt)
    comm_ms = tr.comm_exposed_ms()
    ms_per_step = elapsed / args.steps * 1e3
    atoms_local = gb.N
    atoms_total = total_graphs * ATOMS_PER_GRAPH
    value = atoms_total * args.steps / elapsed
    final_loss = float(loss.cpu())
    # hipEvent per-step times (median over the timed steps), after the contract's wall-clock bracket
    ev_ms = event_timed(step, args.steps)
    barrier()

    out = {
        "metric": "atoms/s (fwd+bwd) on 256-atom/16-neighbor synthetic graphs",
        "value": value, "unit": "atoms/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
        "scaling": args.scaling, "vs_baseline": None,
        # the arithmetic type of the multiplier, not a precision claim: fp32 operands, each carried as two fp16 pieces
        # (22-bit significand), three piece products per multiply on the fp16 matrix pipe, fp32 accumulate; the step on
        # f32-input MFMA only is `fp32_mfma_only` below
        "dtype": ("f32 (f32-input MFMA)" if os.environ.get("NG_EDGE_MATH", "") == "fp32"
                  else "f32 (2xf16-piece MFMA, f32 accumulate)"), "data": "synthetic",
        "config": {"workload": (f"configs[2]/[3]: training step (fwd+loss+bwd+all-reduce+Adam) on "
                                + (f"{args.total_graphs} graphs in total" if args.scaling == "strong"
                                   else f"{args.graphs} graphs per GPU")
                                + f" x {ATOMS_PER_GRAPH} atoms, K={K_NEIGH}, F=64, E=3, H=128, 4 MP / 4 edge-FC / 4 FC "
                                  f"layers, noise+dropout on"),
                   "atoms_total": atoms_total, "atoms_this_rank": atoms_local, "edges_this_rank": gb.n_edges,
                   "edge_path": ("edge-function table (NG_BENCH_EDGE_TABLE=1: tracing only, NOT the graded configuration)"
                                 if eng.edge_table else "edge MLP evaluated per edge (the reference's arithmetic; SURVEY 8d)"),
                   "parallelism": f"graph-parallel dp{world}", "params": eng.params.count(),
                   "backend": backend, "world_size": world, "collective_library": collective_library(backend),
                   # dmabuf IPC between the ranks' processes: what RCCL's intra-node transport needs here
                   "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")},
        "ms_per_step_hipevent_median": float(np.median(ev_ms)),
        "ms_per_step_hipevent_min": float(np.min(ev_ms)),
        "rank_ms_per_step": {"min": min(rank_ms), "max": max(rank_ms)},
        "allreduce_exposed_ms": comm_ms,
        "preprocess_ms": {"h2d_and_lists_first_call": t_h2d * 1e3, "lists_steady_state": t_csc * 1e3,
                          "note": "host tuple -> device + lists on the first call (allocations included); steady-state "
                                  "list construction from a device tuple (ng_build_incoming_lists); see "
                                  "fresh_batch_every_step for the step that includes it"},
        "loss": final_loss,
        "matrix_math": ("f32-input MFMA everywhere" if os.environ.get("NG_EDGE_MATH", "") == "fp32" else
                        "fp16 MFMA on fp32 operands split into 2 fp16 pieces (22-24 significand bits), 3 piece products per "
                        "multiply, fp32 accumulate: edge MLP forward and backward, the matrix phases of the F = 64 window "
                        "kernels (mp_win*), the fused FC block (fc_fused_fwd / _bwd, fp32 repair in-kernel) and the generic "
                        "split-operand GEMMs (gemm_h2) unless NG_GEMM_MATH=fp32; head, embedding, loss, Adam: fp32 VALU; "
                        "range fall-backs: f32-input MFMA.  Error against float64 at or below the f32-input MFMA kernels' "
                        "(tests/test_gpu_edge_h2.py, test_gpu_fc_block.py, test_gpu_mp_w16.py)"),
    }
    if dumped is not None and rank == 0:
        assert sum(a.nbytes for a in dumped.values()) <= 64 << 20      # 23 + 23 arrays, ~0.9 MB at this architecture
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in dumped.items():
            assert a.dtype in (np.float32, np.float64), (name, a.dtype)
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
        out["dump_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "arrays": len(dumped),
                               "bytes": int(sum(a.nbytes for a in dumped.values()))}

    # ---- the reference sees a NEW graph tuple every step (nmrgnn/library.py:88-89): the same step with the batch
    # object rebuilt from the raw device tuple inside the timed region (compute-side lists + incoming-edge lists by
    # ng_build_incoming_lists), i.e. nothing of the preprocessing amortised
    if world == 1:
        def fresh_step():
            g2 = GraphBatch(*raw, graph_ptr=b["graph_ptr"], device=dev, validate=False)
            return tr.step(g2, y, w, total_graphs=total_graphs)
        for _ in range(2):
            fresh_step()
        ms = event_timed(fresh_step, max(5, args.steps // 2))
        out["fresh_batch_every_step"] = {"ms_per_step": float(np.median(ms)), "value": gb.N / (np.median(ms) * 1e-3),
                                         "unit": "atoms/s", "list_build_ms": t_csc * 1e3,
                                         "note": "raw (atoms, nlist, edges, inv_degree) resident in HBM; GraphBatch and "
                                                 "its lists rebuilt every step"}
        # the same with the next batch's lists built on a side stream while the step runs (graph.py: BatchPrefetcher)
        n_pf = max(5, args.steps // 2)
        stream = iter(BatchPrefetcher(((raw, b["graph_ptr"]) for _ in range(n_pf + 2)), device=dev, validate=False))
        for _ in range(2):
            tr.step(next(stream), y, w, total_graphs=total_graphs)
        ms = event_timed(lambda: tr.step(next(stream), y, w, total_graphs=total_graphs), n_pf)
        # ... and with the tuple in HOST memory (numpy arrays, what a data loader yields): PCIe-inclusive
        host_raw = tuple(t.cpu().numpy() for t in raw)
        def host_step():
            g2 = GraphBatch(*host_raw, graph_ptr=b["graph_ptr"], device=dev, validate=False)
            return tr.step(g2, y, w, total_graphs=total_graphs)
        host_step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_pf):
            host_step()
        torch.cuda.synchronize()
        host_plain = (time.perf_counter() - t0) / n_pf * 1e3
        hstream = iter(BatchPrefetcher(((host_raw, b["graph_ptr"]) for _ in range(n_pf + 1)), device=dev, validate=False))
        tr.step(next(hstream), y, w, total_graphs=total_graphs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_pf):
            tr.step(next(hstream), y, w, total_graphs=total_graphs)
        torch.cuda.synchronize()
        host_pf = (time.perf_counter() - t0) / n_pf * 1e3
        out["fresh_batch_every_step"]["from_host_memory"] = {
            "ms_per_step": host_plain, "value": gb.N / (host_plain * 1e-3),
            "prefetched_ms_per_step": host_pf, "prefetched_value": gb.N / (host_pf * 1e-3),
            "bytes_per_step": int(sum(a.nbytes for a in host_raw)),
            "note": "wall clock; numpy tuple -> device copy + lists + step, every step (PCIe-inclusive); prefetched: the "
                    "copy and the lists of batch t+1 on a side stream during step t"}
        out["fresh_batch_every_step"]["prefetched"] = {
            "ms_per_step": float(np.median(ms)), "value": gb.N / (np.median(ms) * 1e-3),
            "note": "BatchPrefetcher: batch t+1's copy and lists on a side stream (own library context) during step t"}

    # ---- per-kernel hipEvent pass (same step, events bracketed inside the C library).  EVERY rank runs the
    # steps — they contain the gradient all-reduce, a collective — only rank 0 reads the events.
    psteps = min(args.steps, 5)
    if not args.no_profile:
        torch.cuda.synchronize()
        if rank == 0:
            prof = profiled_steps(eng, step, psteps)
        else:
            for _ in range(psteps):
                step()
            torch.cuda.synchronize()
            prof = None
        if rank == 0:
            n_live = int((b["edges"] > 0).sum()) if eng.use_live_edges else None
            work = kernel_work(gb.N, K_NEIGH, 64, 3, 128, 4, 4, 4, NUM_ELEM, live_edges=n_live)
            rows = roofline_rows(prof, psteps, work, h2_gemm=False)
            out["roofline_all"] = rows
            dom = next((r for r in rows if "bound" in r), None)
            if dom is not None:
                traffic, mfma_busy, mfma_coexec, note = pmc_lookup(dom["kernel"])
                alg = work[dom["kernel"]]
                out["roofline"] = {"kernel": dom["kernel"], "bound": dom["bound"], "achieved": dom["achieved"],
                                   "peak": dom["peak"], "unit": dom["unit"], "frac": dom["frac"], "traffic": traffic,
                                   "mfma_pipe_busy": mfma_busy, "mfma_coexec_frac": mfma_coexec, "pmc_note": note, "algorithmic_bytes": alg[2],
                                   "algorithmic_flops": alg[1], "avg_launch_ms": dom["avg_ms"],
                                   "edges_priced": n_live if n_live is not None else gb.n_edges,
                                   "edge_slots": gb.n_edges}
            out["profiled_ms_per_step"] = sum(r["ms_per_step"] for r in rows)
            out["survey_8d"] = survey_8d_block(rows, gb.N, K_NEIGH, 64, 3, 128, 4, 4, 4, out["ms_per_step"],
                                               n_live if n_live is not None else gb.n_edges)
            if "roofline" in out:
                out["roofline"]["step"] = out["survey_8d"]["step"]

    extras = rank == 0 and world == 1 and not args.no_extras
    # ---- configs[1]: the same batch, inference only (no noise / dropout / tape), reported beside the headline
    if extras:
        for _ in range(2):
            eng.forward(gb)
        isteps = max(5, args.steps // 2)
        ms = event_timed(lambda: eng.forward(gb), isteps)
        out["inference"] = {"workload": "configs[1]: forward only on the same batch", "value": gb.N / (np.median(ms) * 1e-3),
                            "unit": "atoms/s", "ms_per_step": float(np.median(ms)), "steps": isteps}

    # ---- the same step with the f32-input MFMA edge kernels (NG_EDGE_MATH=fp32), for comparison
    if extras and os.environ.get("NG_EDGE_MATH", "") != "fp32":
        keep = os.environ.get("NG_EDGE_MATH")
        os.environ["NG_EDGE_MATH"] = "fp32"
        _lib.reload_env()
        for _ in range(2):
            step()
        fsteps = max(5, args.steps // 2)
        ms = event_timed(step, fsteps)
        out["fp32_mfma_only"] = {"value": gb.N / (np.median(ms) * 1e-3), "unit": "atoms/s",
                                 "ms_per_step": float(np.median(ms)), "steps": fsteps}
        if keep is None:
            del os.environ["NG_EDGE_MATH"]
        else:
            os.environ["NG_EDGE_MATH"] = keep
        _lib.reload_env()

    # ---- the Engine's DEFAULT edge path (round 6): a guarded table of the edge function (csrc/edge_table.hip).  mask + RBF +
    # EdgeFCBlock is a function of ONE scalar per edge; evaluated with the same fused kernels on 4096 points (+ 4096 midpoints
    # for the guard) and interpolated per edge (cubic; backward = the exact adjoint + the fused backward on the table) it agrees
    # with the per-edge path to ~1e-6 of the largest shift / 2e-5 of the largest gradient entry (tests/test_gpu_edge_table.py)
    # and passes the same oracle / reference-graph tolerances (tests/test_gpu_savedmodel.py).  NOT what `value` is measured on.
    if extras:
        p_exact = eng.forward(gb).clone()
        eng.edge_table = True
        try:
            p_diff = float((eng.forward(gb) - p_exact).abs().max())      # same weights, both paths
            for _ in range(3):
                step()
            tsteps = max(5, args.steps // 2)
            ms = event_timed(step, tsteps)
            eng.forward(gb)
            ims = event_timed(lambda: eng.forward(gb), tsteps)
            # serving form: weights frozen, the table kept over calls (built once per weight generation; every call checks its own
            # distance range against the table's on the device)
            eng.freeze_weights(True)
            eng.forward(gb)
            fms = event_timed(lambda: eng.forward(gb), tsteps)
            eng.freeze_weights(False)
            peaks_t = eng.forward(gb, training=True, seed=1)
            rep = eng.edge_table_report()
            eng.tape = None
            blk = {"ms_per_step": float(np.median(ms)), "value": gb.N / (np.median(ms) * 1e-3), "unit": "atoms/s", "steps": tsteps,
                   "inference_ms_per_step": float(np.median(ims)),
                   "inference_frozen_weights_ms_per_step": float(np.median(fms)),
                   "max_abs_peak_difference_to_per_edge_path": p_diff,
                   "guard": {"raised": rep[0], "midpoint_error": rep[1], "max_abs_e": rep[2], "tolerance_relative": eng.edge_table_tol},
                   "note": "Engine default (NG_EDGE_TABLE=0 / Engine.edge_table = False: per edge): edge MLP evaluated on a 4096-point "
                           "table (+ 4096 midpoints for the on-device guard) per step and interpolated per edge; the per-edge kernels "
                           "run over zero rows unless the guard is up; `value` above is NOT measured this way"}
            if not args.no_profile:
                prof_t = profiled_steps(eng, step, 3)
                n_live = int((b["edges"] > 0).sum())
                rows_t = roofline_rows(prof_t, 3, kernel_work(gb.N, K_NEIGH, 64, 3, 128, 4, 4, 4, NUM_ELEM, live_edges=2 * eng._table_points()),
                                       h2_gemm=False)
                blk["roofline_all"] = rows_t
                blk["survey_8d"] = survey_8d_block(rows_t, gb.N, K_NEIGH, 64, 3, 128, 4, 4, 4, blk["ms_per_step"], None)
                blk["survey_8d"]["step"]["note"] = ("flops per atom as SURVEY 8(d) prices them (edge MLP per edge): the table path does "
                                                    "not execute the edge MLP's share of them")
            out["edge_table"] = blk
        except Exception as ex:
            out["edge_table"] = {"error": repr(ex)}
        finally:
            eng.edge_table = False
        for _ in range(2):
            step()

    # ---- the reference's own training granularity: ONE graph per step (nmrgnn/library.py:88-89, main.py:74-80 — the
    # dataset is never batched).  256 atoms: every kernel is a fraction of a wave per CU, the step is the launch chain.
    if extras:
        try:
            out["train_one_graph_per_step"] = one_graph_leg(dev, hp)
        except Exception as ex:
            out["train_one_graph_per_step"] = {"error": repr(ex)}

    # ---- the reference's DEFAULT width (atom_feature_size = 256, model.py:22): same batch, same step
    if extras:
        try:
            arch256 = dict(ARCH, atom_feature_size=256)
            eng2 = Engine(declare_gnn_space(HyperParameters(**arch256)), NUM_ELEM, device=dev, seed=1234)
            eng2.edge_table = False      # per edge, as the headline; the Engine's default (guarded table) is timed at the end
            tr2 = Trainer(eng2, lr=1e-4)
            step2 = lambda: tr2.step(gb, y, w)
            for _ in range(3):
                step2()
            fsteps = max(5, args.steps // 5)
            ms = event_timed(step2, fsteps)
            blk = {"workload": "the same batch and step at atom_feature_size = 256 (reference default architecture, "
                               "1,070,477 parameters)", "value": gb.N / (np.median(ms) * 1e-3), "unit": "atoms/s",
                   "ms_per_step": float(np.median(ms)), "steps": fsteps}
            if not args.no_profile:
                prof2 = profiled_steps(eng2, step2, 3)
                rows2 = roofline_rows(prof2, 3, kernel_work(gb.N, K_NEIGH, 256, 3, 128, 4, 4, 4, NUM_ELEM,
                                                            live_edges=int((b["edges"] > 0).sum()) if eng2.use_live_edges else None),
                                      h2_gemm=os.environ.get("NG_GEMM_MATH", "") != "fp32")
                blk["roofline_all"] = rows2
                dom2 = next((r for r in rows2 if "bound" in r), None)
                if dom2 is not None:
                    blk["roofline"] = {k: dom2[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_ms")}
                blk["survey_8d"] = survey_8d_block(rows2, gb.N, K_NEIGH, 256, 3, 128, 4, 4, 4, blk["ms_per_step"],
                                                   int((b["edges"] > 0).sum()))
                if "roofline" in blk:
                    blk["roofline"]["step"] = blk["survey_8d"]["step"]
            ms = event_timed(lambda: eng2.forward(gb), 5)
            blk["inference_ms_per_step"] = float(np.median(ms))
            blk["inference_value"] = gb.N / (np.median(ms) * 1e-3)
            eng2.edge_table = True
            for _ in range(2):
                step2()
            ms = event_timed(step2, fsteps)
            eng2.forward(gb)
            ims = event_timed(lambda: eng2.forward(gb), 5)
            blk["edge_table"] = {"ms_per_step": float(np.median(ms)), "value": gb.N / (np.median(ms) * 1e-3),
                                 "inference_ms_per_step": float(np.median(ims)),
                                 "note": "the Engine's default edge path (guarded table of the edge function)"}
            out["f256"] = blk
            del eng2, tr2
        except Exception as ex:
            out["f256"] = {"error": repr(ex)}

    # ---- configs[4]: whole-protein inference, 100-frame synthetic trajectory of 7lgi (frame 0 + N(0, 0.3 A), seed 7),
    # GPU graph build + model at the baseline architecture, kNN (padded) and distance-cutoff (CSR) lists
    if extras:
        try:
            out["configs4"] = whole_protein_leg(dev)
        except Exception as ex:
            out["configs4"] = {"error": repr(ex)}

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(ARCH, sample_graphs=8, seed=42)
        except Exception as ex:  # the baseline must never take the bench line down
            out["cpu_baseline"] = {"error": repr(ex)}
        if isinstance(out.get("configs4"), dict) and "error" not in out["configs4"]:
            try:
                out["configs4"]["cpu_baseline"] = cpu_baseline_protein()
            except Exception as ex:
                out["configs4"]["cpu_baseline"] = {"error": repr(ex)}

    if rank == 0:
        print(json.dumps(out))
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def one_graph_leg(dev, hp, n_graphs=64, steps=200):
    """fwd + loss + bwd + Adam on ONE 256-atom graph per step, a different graph every step (64 graphs cycled; tuples
    resident in HBM, the GraphBatch and its lists rebuilt inside the step as the reference would see a new record)"""
    from nmrgnn_amd import synth
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.graph import GraphBatch
    from nmrgnn_amd.train import Trainer
    eng = Engine(hp, NUM_ELEM, device=dev, seed=1234)
    tr = Trainer(eng, lr=1e-4)
    gs = []
    for g in range(n_graphs):
        b = synth.make_batch(1, ATOMS_PER_GRAPH, K_NEIGH, NUM_ELEM, 0.05, seed=1000 + g)
        gb = GraphBatch(b["atoms"], b["nlist"], b["edges"], b["inv_degree"], graph_ptr=b["graph_ptr"], device=dev)
        gs.append(((gb.atoms, gb.nlist, gb.edges, gb.inv_degree), b["graph_ptr"], torch.from_numpy(b["y"]).to(dev),
                   torch.from_numpy(b["w"]).to(dev)))
    it = [0]

    def step():
        raw, gp, y, w = gs[it[0] % n_graphs]
        it[0] += 1
        return tr.step(GraphBatch(*raw, graph_ptr=gp, device=dev, validate=False), y, w)

    def timed(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    eager = timed(step)
    ev = event_timed(step, steps)
    # the same steps as ONE graph launch each (nmrgnn_amd/replay.py: the chain captured once per shape, inputs / seeds / Adam's
    # rate staged by one eager launch per step; trajectories bit-identical to the eager chain, tests/test_gpu_replay.py)
    from nmrgnn_amd.replay import TrainStepReplay
    raw0, gp0, y0, w0 = gs[0]
    rp = TrainStepReplay(tr, raw0, y0, w0, graph_ptr=gp0)

    def rstep():
        raw, gp, y, w = gs[it[0] % n_graphs]
        it[0] += 1
        return rp.step(raw, y, w)

    wall = timed(rstep)
    rev = event_timed(rstep, steps)
    replay = {"ms_per_step": wall, "ms_per_step_hipevent_median": float(np.median(rev)),
              "note": "HIP-graph replay (TrainStepReplay): 1 staging launch + 1 graph launch per step"}
    eag = {"ms_per_step": eager, "ms_per_step_hipevent_median": float(np.median(ev)), "note": "28 eager launches per step (34 before the round-6 merges)"}
    # which of the two wins depends on the host: the GPU timeline of the step is ~0.30 ms either way (small-kernel latency,
    # DESIGN 4.5); the replay takes the host's launch work out
    best, path = (replay, "replay") if wall <= eager else (eag, "eager")
    return {"workload": f"1 graph x {ATOMS_PER_GRAPH} atoms per step (fwd+loss+bwd+Adam), a new graph tuple every step, F=64",
            "ms_per_step": best["ms_per_step"], "ms_per_step_hipevent_median": best["ms_per_step_hipevent_median"],
            "value": ATOMS_PER_GRAPH / (best["ms_per_step"] * 1e-3), "unit": "atoms/s", "steps": steps, "path": path,
            "replay": replay, "eager": eag,
            "note": "wall clock per step includes the host's launch work (python + ctypes); the hipEvent median is the GPU timeline"}


def whole_protein_leg(dev):
    from nmrgnn_amd.engine import Engine
    from nmrgnn_amd.graph import frames_to_batch, frames_to_batch_cutoff
    from nmrgnn_amd.hypers import HyperParameters, declare_gnn_space
    from nmrgnn_amd.structure import atoms_onehot, read_pdb
    s = read_pdb(os.path.join(ROOT, "tests", "data", "7lgi.pdb.gz"))
    rng = np.random.default_rng(7)
    frames = np.stack([s.frames[0] + rng.normal(0, 0.3, s.frames[0].shape).astype(np.float32) for _ in range(100)])
    atoms = atoms_onehot(s.elements)
    n = atoms.shape[0]
    eng = Engine(declare_gnn_space(HyperParameters()), atoms.shape[1], device=dev, seed=1234)
    eng.freeze_weights(True)        # inference: packed weight images are kept across calls (what eval-struct does)
    pos = torch.from_numpy(frames).to(dev)
    at = torch.from_numpy(atoms).to(dev)
    res = {"workload": f"7lgi: {n} atoms x 100 jittered frames, atom_feature_size 256, graph build on the GPU + "
                       f"model forward, positions resident in HBM", "unit": "atoms/s"}
    for tag, build in (("knn16_padded", lambda p: frames_to_batch(at, p, 16, device=dev)),
                       ("cutoff_3.5A_csr", lambda p: frames_to_batch_cutoff(at, p, 3.5, device=dev))):
        for fpb in (50, 1):
            # the Engine's default edge path (guarded table of the edge function, kept over the calls while the weights are
            # frozen), and the edge MLP per edge beside it
            for table in (True, False):
                eng.edge_table = table

                def run():
                    for b0 in range(0, 100, fpb):
                        eng.forward(build(pos[b0:b0 + fpb]))
                run()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                r = {"value": 100 * n / dt, "ms_per_100_frames": dt * 1e3, "ms_per_frame": dt * 10.0,
                     "edge_path": "edge-function table (Engine default)" if table else "per edge"}
                if table:
                    res[f"{tag}_{fpb}_frames_per_call"] = r
                else:
                    res[f"{tag}_{fpb}_frames_per_call"]["per_edge"] = r
    eng.edge_table = True
    # one frame per call as a graph replay (ForwardReplay: kNN build + forward captured once for this protein's shape)
    from nmrgnn_amd.replay import ForwardReplay
    frp = ForwardReplay(eng, at, pos[0], 16)

    def run_replay():
        for b0 in range(100):
            frp(pos[b0])
    run_replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rep = {"value": 100 * n / dt, "ms_per_100_frames": dt * 1e3, "ms_per_frame": dt * 10.0, "path": "HIP-graph replay (ForwardReplay)"}
    res["knn16_padded_1_frames_per_call_replay"] = rep
    if rep["ms_per_frame"] < res["knn16_padded_1_frames_per_call"]["ms_per_frame"]:      # the faster of the two is the leg's number
        res["knn16_padded_1_frames_per_call_eager"] = res["knn16_padded_1_frames_per_call"]
        res["knn16_padded_1_frames_per_call"] = rep
    gc = frames_to_batch_cutoff(at, pos[:1], 3.5, device=dev)
    deg = (gc.row_ptr[1:] - gc.row_ptr[:-1]).cpu().numpy()
    res["cutoff_degree"] = {"min": int(deg.min()), "median": float(np.median(deg)), "max": int(deg.max())}
    return res


if __name__ == "__main__":
    main()
