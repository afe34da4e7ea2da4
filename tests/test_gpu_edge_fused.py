"""The fused edge-MLP kernels at H = 128, Le = 4, softplus, through the C entry points ng_edge_mlp_fwd, ng_edge_mlp_bwd_tape,
ng_edge_mlp_fwd_live / _bwd_live, ng_edge_tape_layout and ng_build_live_edges, element by element against the float64 statement of
tests/edge_mlp_ref.py (checked on the CPU by tests/test_edge_mlp_ref_host.py).

Every output — e, the tape, dW, db — is filled with NaN before the call and allocated with GUARD = 64 extra rows that must still
hold the fill afterwards.  Two families per case:
  exact   edge_mlp_ref.exact_forward_case / exact_backward_case: every output equals the float64 statement BIT FOR BIT (float64
          value rounded to float32; dead rows of e are +0): a dropped or doubled k-step, a misplaced fragment, tape row or partial
          row, a wrong bias or a missing piece product cannot pass.  That the statement is made of float32 numbers any float32
          order reaches, and that no operand leaves two fp16 pieces (so the range guard stays down), is checked on the CPU for
          every case of EXACT_FWD / EXACT_BWD.
  normal  edge_mlp_ref.normal_case: per element |got - ref| <= C_EDGE * mag + 1e-7 * max(mag) (check); for a tensor of at least
          STAT_MIN elements from a split-operand kernel also rms(got - ref) / rms(mag) <= sqrt(r32s * r_drop), both anchors computed
          here from the case's inputs; and max err / max mag <= 8 x that of the same call under NG_EDGE_MATH=fp32 + 1e-6.

Dispatch, from the conditions in the sources (edge_ops.hip, edge_fwd_h2.hip: edge_h2_fwd, edge_fused.hip: edge_fused_fwd_f32,
edge_fused_bwd.hip: edge_fused_bwd, edge_bwd_h2.hip: edge_tape_blocked / edge_bwd_h2_launch), and the case ids that launch each
(test_forward[...] / test_backward[...] unless another test is named; <n> stands for every size of the row):
  forward, NG_EDGE_MATH unset (split operands), persistent min(tiles, num_cu) workgroups of 256-edge tiles
    tape and edge_tape_blocked (E <= 4, NG_EDGE_BWD_MATH unset)  edge_fwd_h2_kernel<2>   h2<2>-<n>-E1|E3|E4
    tape, not blocked (E in 5..8, or NG_EDGE_BWD_MATH=fp32)      edge_fwd_h2_kernel<1>   h2<1>-<n>-E5|E7|E8, h2<1>-<n>-E3-bwdfp32
    no tape                                                      edge_fwd_h2_kernel<0>   h2<0>-<n>-E2|E4|E5|E6|E8
    behind each, run only when the range guard went up           edge_fused_fwd_kernel   test_range_fallback_row_major_tape[E8],
                                                                 (edge_fwd_range_fallback)   [E3-bwdfp32]
  forward, NG_EDGE_MATH=fp32: 2 num_cu workgroups of 64-edge tiles
    edge_fused_fwd_kernel<E, true, 64>    fused-65-E1|E3|E5|E7-tape, fused-n_loop32-E2|E4|E6|E8-tape
    edge_fused_fwd_kernel<E, false, 64>   fused-65-E2|E4|E6|E8-notape, fused-n_loop32-E1|E3|E5|E7-notape
  backward: split = tape_layout == 1 or edge_tape_blocked(E)
    split, blocked tape (layout 1, E <= 4)        edge_bwd_h2_kernel<false>   bh2-<n>-E1..E4-blocked, the scale and reduce rows
    split, row-major tape (layout 0, E <= 4)      edge_bwd_h2_kernel<false>   bh2-33|4097-E3|E4-rowmajor
    not split (E in 5..8, or NG_EDGE_MATH=fp32)   edge_fused_bwd_kernel<E>    bfused-<n>-E5..E8, bfused-<n>-E1..E4-fp32
    behind the split kernel, on a raised guard    edge_fused_bwd_kernel<E>    (edge_bwd_range_fallback; blocked tape only:
                                                  test_gpu_edge_h2.py::test_edge_backward_beyond_the_fp16_range_equals_float64)
    gradient scale: n E <= 32768 and de 16-byte aligned -> in-kernel scan; else hx_absmax_kernel, float4 body when aligned,
    element by element when not                   bh2-8192-E4-blocked | bh2-8193-E4-blocked | test_gradient_scale_unaligned_de
    edge_bwd_reduce_kernel: 8-deep loop above 112 partial rows / waves without a row below 16
                                                  bh2-7300-E3-blocked / bh2-900-E3-blocked
    blocked tape and E > 4                        refused, nothing launched   test_blocked_tape_refused_at_E8
    n_edges = 0                                   two memsets per layer       test_backward_of_no_edges
  live view (perm given)
    edge_fwd_h2_kernel<2|1|0>, edge_fused_fwd_kernel<3, true, 64>   test_live_forward[h2<2>|h2<1>|h2<0>|fused-<p_dead>]
    edge_bwd_h2_kernel<true>, edge_fused_bwd_kernel<6> with perm    test_live_backward[bh2<true>|bfused-<p_dead>]
The names edge_fwd_h2, edge_fused_fwd and edge_fwd_range_fallback are confirmed by test_profile_names_follow_the_switch.

Sizes that make a persistent workgroup take a second tile follow the device: n_loop = 256 num_cu + 4465 (ragged 256-tile and ragged
32-group at the end), n_loop32 = 128 num_cu + 77 (f32-input forward), n_bwd = 64 num_cu + 4465 (64-edge backward tiles)."""
import ctypes as C

import numpy as np
import pytest

import edge_mlp_ref as R
from edge_mlp_ref import C_EDGE, H, STAT_MIN, check, f32, rstat
from test_gpu_edge_h2 import _overflow_case

pytestmark = pytest.mark.gpu

GUARD = 64
HOST_CU = 256                   # compute units the CPU-side checks assume for the sizes that follow the device
BIG = 1024                      # references above this many rows are kept one at a time
FP32 = {"NG_EDGE_MATH": "fp32"}
BWD_FP32 = {"NG_EDGE_BWD_MATH": "fp32"}


def rows_of(n, cu):
    return {"n_loop": 256 * cu + 4465, "n_loop32": 128 * cu + 77, "n_bwd": 64 * cu + 4465}[n] if isinstance(n, str) else n


# ------------------------------------------------------------------------------------------------------------------ case tables
def _fwd_cases():
    t = {}

    def add(kern, n, E, save, env=None, tag=""):
        t[f"{kern}-{n}-E{E}{tag}"] = dict(kern=kern, n=n, E=E, save=save, env=env or {}, layout={"h2<2>": 1, "h2<1>": 0}.get(kern))

    for E in (1, 3, 4):
        for n in (1, 31, 32, 33, 255, 257, "n_loop"):
            add("h2<2>", n, E, True)
    for n in (1, 33, 257, "n_loop"):
        for E in (5, 7, 8):
            add("h2<1>", n, E, True)
        add("h2<1>", n, 3, True, BWD_FP32, "-bwdfp32")
    for E in (2, 4, 5, 6, 8):
        for n in (1, 257, "n_loop"):
            add("h2<0>", n, E, False)
    for E in range(1, 9):
        for i, n in enumerate((65, "n_loop32")):
            save = (E + i) % 2 == 1
            add("fused", n, E, save, FP32, "-tape" if save else "-notape")
    return t


def _bwd_cases():
    t = {}

    def add(kern, n, E, layout, env=None, tag=""):
        t[f"{kern}-{n}-E{E}{tag}"] = dict(kern=kern, n=n, E=E, layout=layout, env=env or {})

    for E in (1, 2, 3, 4):
        for n in (1, 63, 65, "n_bwd"):
            add("bh2", n, E, 1, tag="-blocked")
    for E in (3, 4):
        for n in (33, 4097):
            add("bh2", n, E, 0, tag="-rowmajor")
    for E in range(1, 9):
        for n in (65, "n_bwd"):
            add("bfused", n, E, 0, FP32 if E <= 4 else None, "-fp32" if E <= 4 else "")
    for n in (8192, 8193):              # n E = 32768: the workgroups scan de themselves; 32772: hx_absmax_kernel's float4 body
        add("bh2", n, 4, 1, tag="-blocked")
    for n in (7300, 900):               # 115 partial rows: the reduction's 8-deep loop; 15: waves without a row
        add("bh2", n, 3, 1, tag="-blocked")
    return t


FWD, BWD = _fwd_cases(), _bwd_cases()


def _pairs(table):
    """(case, family), the cases above BIG rows grouped by family and size so that their reference is computed once"""
    def key(p):
        n = rows_of(table[p[0]]["n"], HOST_CU)
        return (n > BIG, p[1] if n > BIG else "", n if n > BIG else 0)
    return sorted([(k, f) for k in table for f in ("exact", "normal")], key=key)


FWD_PAIRS, BWD_PAIRS = _pairs(FWD), _pairs(BWD)
EXACT_FWD = sorted({(sp["n"], sp["E"]) for sp in FWD.values()}, key=str)
UNALIGNED_N = (10922, 10923)                            # n E = 32766 and 32769 at E = 3: either side of the in-kernel scan's limit
EXACT_BWD = sorted({(sp["n"], sp["E"]) for sp in BWD.values()} | {(n, 3) for n in UNALIGNED_N}, key=str)
NORMAL_FWD, NORMAL_BWD = EXACT_FWD, EXACT_BWD          # both families run at every shape
RANGE_ROWS = [(8, {}), (3, BWD_FP32)]                   # the range-fallback row: E and the switches
LIVE_FWD = {"h2<2>": (3, True, {}), "h2<1>": (5, True, {}), "h2<0>": (4, False, {}), "fused": (3, True, FP32)}
LIVE_BWD = {"bh2<true>": (3, {}), "bfused": (6, {})}
LIVE_N = 777
LIVE_P = (0.3, 1.0)


# ------------------------------------------------------------------------------------------------- references (NumPy, cached)
_HID, _BWD = {}, {}


def _args(c):
    return c["d_src"], c["d_eff"], c["centers"], c["gap"], c["Ws"], c["bs"]


def hidden_ref(fam, n, p_dead=0.15):
    """the E-independent part of a forward case: inputs, float64 z and magnitudes and (normal family) the statistics of the float32
    and the dropped-piece evaluation of z and their third layer for the output statistics"""
    key = (fam, n, p_dead)
    if key not in _HID:
        if n > BIG:
            for k in [k for k in _HID if k[1] > BIG]:
                del _HID[k]
        hid = (R.normal_hidden if fam == "normal" else R.exact_hidden)(n, n, p_dead)
        a = (hid["d_src"], hid["d_eff"], hid["centers"], hid["gap"], hid["Wh"], hid["bh"])
        (_, zs), (_, ms) = R.ref_hidden(*a)
        ent = dict(hid=hid, z=zs, mz=ms)
        if fam == "normal":
            z32, zd = R.f32_hidden(*a), R.drop_hidden(*a)
            ent.update(zstat=R.stats_of({"z": z32}, {"z": zd}, {"z": zs}, {"z": ms}), z32=z32[2], zd=zd[2])
        _HID[key] = ent
    return _HID[key]


def fwd_reference(fam, n, E, p_dead=0.15):
    """case, float64 values, magnitudes and (normal family) {tensor: (r32, r32s, r_drop)}"""
    ent = hidden_ref(fam, n, p_dead)
    c = (R.normal_output if fam == "normal" else R.exact_output)(ent["hid"], E, n)
    e, me = R.ref_output(c["d_src"], ent["z"][2], ent["mz"][2], c["Ws"][3], c["bs"][3])
    v, mg, st = {"e": e, "z": ent["z"]}, {"e": me, "z": ent["mz"]}, {}
    if fam == "normal":
        st = dict(ent["zstat"])
        st.update(R.stats_of({"e": R.f32_output(c["d_src"], ent["z32"], c["Ws"][3], c["bs"][3])},
                             {"e": R.drop_output(c["d_src"], ent["zd"], c["Ws"][3], c["bs"][3])}, {"e": e}, {"e": me}))
    return c, v, mg, st


def bwd_reference(fam, n, E, p_dead=0.15):
    """the same for the backward; the normal family's tape is the float64 forward rounded to float32"""
    key = (fam, n, E, p_dead)
    if key not in _BWD:
        _BWD.clear()
        if fam == "normal":
            ent = hidden_ref(fam, n, p_dead)
            c = R.normal_output(ent["hid"], E, n)
            c["zs32"] = [f32(z) for z in ent["z"]]
        else:
            c = R.exact_backward_case(n, E, n, p_dead)
        v, mg = R.ref_backward(c["d_src"], c["d_eff"], c["centers"], c["gap"], c["Ws"], c["zs32"], c["de"])
        _BWD[key] = (c, v, mg, R.backward_stats(c, v, mg) if fam == "normal" and n else {})
    return _BWD[key]


# ---------------------------------------------------------------------------------------------------------------- device side
def num_cu_of(dev):
    import torch
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _ctx():
    from nmrgnn_amd import _lib
    return _lib.get_context(0)


def _st(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _t(dev, a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _nan(dev, *shape):
    import torch
    return torch.full(shape, float("nan"), device=dev)


def _untouched(name, t, first):
    import torch
    assert bool(torch.isnan(t[first:]).all()), f"{name}: a store past the end of the output"


def tape_layout(E, n):
    return int(_ctx().lib.ng_edge_tape_layout(H, E, 4, 1, n))


def build_live(dev, d_src):
    import torch
    from nmrgnn_amd._lib import ptr
    n = len(d_src)
    td = _t(dev, d_src)
    perm = torch.full((n,), -7, dtype=torch.int32, device=dev)
    pos = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_c = torch.full((n,), -7.0, device=dev)
    n_live = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ctx = _ctx()
    ctx.check(ctx.lib.ng_build_live_edges(ctx.handle, _st(dev), n, ptr(td), ptr(perm), ptr(pos), ptr(d_c), ptr(n_live)),
              "ng_build_live_edges")
    idx = np.flatnonzero(np.asarray(d_src, np.float32) > 0)
    assert int(n_live.cpu()) == len(idx) and np.array_equal(perm.cpu().numpy()[:len(idx)], idx)
    return dict(perm=perm, d_c=d_c, n_live=n_live, idx=idx)


def run_fwd(dev, c, save, live=None):
    """ng_edge_mlp_fwd (live: ng_edge_mlp_fwd_live) -> {"e": [n, E], "z": three row-major [rows, 128]} as float32 arrays.  The tape
    rows are the n edges, or with the live view the live slots in ascending order"""
    import torch
    from nmrgnn_amd._lib import ptr, ptr_array
    n, E = c["n"], c["E"]
    tc = _t(dev, c["centers"])
    tW, tb = [_t(dev, w) for w in c["Ws"]], [_t(dev, b) for b in c["bs"]]
    e = _nan(dev, n + GUARD, E)
    z = _nan(dev, 3 * n + GUARD, H) if save else None
    ctx = _ctx()
    layout = tape_layout(E, n)
    if live is None:
        td, te = _t(dev, c["d_src"]), _t(dev, c["d_eff"])
        ctx.check(ctx.lib.ng_edge_mlp_fwd(ctx.handle, _st(dev), n, H, E, 4, 1, ptr(td), ptr(te), ptr(tc), float(c["gap"]),
                                          ptr_array(tW), ptr_array(tb), ptr(e), ptr(z)), "ng_edge_mlp_fwd")
        rows = n
    else:
        rows = len(live["idx"])
        te = torch.full((n,), 3.0, device=dev)
        te[:rows] = _t(dev, c["d_eff"][live["idx"]])
        ctx.check(ctx.lib.ng_edge_mlp_fwd_live(ctx.handle, _st(dev), n, H, E, 4, 1, ptr(live["d_c"]), ptr(te), ptr(live["perm"]),
                                               ptr(live["n_live"]), ptr(tc), float(c["gap"]), ptr_array(tW), ptr_array(tb),
                                               ptr(e), ptr(z)), "ng_edge_mlp_fwd_live")
    torch.cuda.synchronize()
    _untouched("e", e, n)
    out = {"e": e[:n].cpu().numpy()}
    if save:
        _untouched("tape", z, 3 * n)
        zz = z[:3 * n].reshape(3, n * H).cpu().numpy()
        out["z"] = [R.tape_to_rows(zz[l], rows, layout) for l in range(3)]
    return out


def run_bwd(dev, c, layout, live=None, de_shift=0, refused=False):
    """ng_edge_mlp_bwd_tape (live: ng_edge_mlp_bwd_live) with the tape c["zs32"] handed in `layout` -> {"dW": [4], "db": [4]};
    de_shift: de starts that many floats into its allocation; refused: the call must return an error, which is returned with its
    text"""
    import torch
    from nmrgnn_amd._lib import ptr, ptr_array
    n, E = c["n"], c["E"]
    tc = _t(dev, c["centers"])
    tW = [_t(dev, w) for w in c["Ws"]]
    rows_idx = None if live is None else live["idx"]
    tape = np.full((3, max(n, 1) * H), np.nan, np.float32)
    for l in range(3):
        zr = np.asarray(c["zs32"][l], np.float32)
        zr = zr if rows_idx is None else zr[rows_idx]
        tape[l, :zr.shape[0] * H] = R.rows_to_tape(zr, layout)
    tz = _t(dev, tape)
    buf = torch.zeros(n * E + de_shift + 4, device=dev)
    tde = buf[de_shift:de_shift + n * E]
    tde.copy_(_t(dev, c["de"]).reshape(-1))
    assert tde.data_ptr() % 16 == (4 * de_shift) % 16
    dW = [_nan(dev, H + GUARD, k) for k in (H, H, H, E)]
    db = [_nan(dev, k + GUARD) for k in (H, H, H, E)]
    ctx = _ctx()
    if live is None:
        td, te = _t(dev, c["d_src"]), _t(dev, c["d_eff"])
        rc = ctx.lib.ng_edge_mlp_bwd_tape(ctx.handle, _st(dev), n, H, E, 4, 1, ptr(td), ptr(te), ptr(tc), float(c["gap"]),
                                          ptr_array(tW), ptr(tz), ptr(tde), ptr_array(dW), ptr_array(db), layout)
    else:
        te = torch.full((n,), 3.0, device=dev)
        te[:len(rows_idx)] = _t(dev, c["d_eff"][rows_idx])
        rc = ctx.lib.ng_edge_mlp_bwd_live(ctx.handle, _st(dev), n, H, E, 4, 1, ptr(live["d_c"]), ptr(te), ptr(live["perm"]),
                                          ptr(live["n_live"]), ptr(tc), float(c["gap"]), ptr_array(tW), ptr(tz), ptr(tde),
                                          ptr_array(dW), ptr_array(db), layout)
    torch.cuda.synchronize()
    if refused:
        assert all(bool(torch.isnan(t).all()) for t in dW + db), "a refused call wrote an output"
        return rc, (ctx.lib.ng_last_error(ctx.handle) or b"").decode()
    ctx.check(rc, "ng_edge_mlp_bwd")
    for l in range(4):
        _untouched(f"dW{l}", dW[l], H)
        _untouched(f"db{l}", db[l], (H, H, H, E)[l])
    return {"dW": [w[:H].cpu().numpy() for w in dW], "db": [b[:k].cpu().numpy() for b, k in zip(db, (H, H, H, E))]}


# ---------------------------------------------------------------------------------------------------------------- comparisons
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def hold(fam, got, v, mg, failures, sel=None):
    """every tensor of `got` against float64 by the family's criterion (sel: rows of the reference the rows of got stand for; e keeps
    the caller's rows); returns max err / max mag per tensor (normal family)"""
    errs = {}
    M = dict(R.tensors(mg))
    ref = dict(R.tensors(v))
    for name, g in R.tensors(got):
        r, m = ref[name], M[name]
        if sel is not None and name.startswith("z"):
            r, m = r[sel], m[sel]
        if fam == "exact":
            want = r.astype(np.float32)
            if not same_bits(g, want):
                bad = np.ascontiguousarray(g, np.float32).reshape(-1).view(np.int32) != want.reshape(-1).view(np.int32)
                k = int(np.flatnonzero(bad)[0])
                failures.append(f"{name}: {int(bad.sum())} of {bad.size} elements differ from float64; first at flat {k}: "
                                f"got {g.reshape(-1)[k]!r} ref {want.reshape(-1)[k]!r}")
        else:
            try:
                errs[name] = check(name, g, r, m, c_rel=C_EDGE)
            except AssertionError as err:
                failures.append(str(err))
    return errs


def hold_stats(kind, cid, got, v, mg, st, failures, sel=None):
    """the rms statistic of the tensors behind a split-operand product (forward: e and z; backward: dW of the hidden layers — the
    output layer's gradients are plain float32 sums on the vector unit), where they have STAT_MIN elements"""
    M, ref = dict(R.tensors(mg)), dict(R.tensors(v))
    for name, g in R.tensors(got):
        if g.size < STAT_MIN or name in ("dW3", "db3"):
            continue
        r, m = ref[name], M[name]
        if sel is not None and name.startswith("z"):
            r, m = r[sel], m[sel]
        _, r32s, r_drop = st[name]
        rs, thr = rstat(g, r, m), float(np.sqrt(r32s * r_drop))
        print(f"RSTAT {kind} {cid:28s} {name:4s} r {rs:.3e} r32s {r32s:.3e} r_drop {r_drop:.3e} thr {thr:.3e}")
        if not rs <= thr:
            failures.append(f"{name}: r = {rs:.3e} above sqrt(r32s * r_drop) = {thr:.3e} (r32s {r32s:.3e}, r_drop {r_drop:.3e})")


def against_fp32(cid, errs, errs32, failures):
    print("ERR", cid, {k: (f"{errs[k]:.2e}", f"{errs32.get(k, 0):.2e}") for k in errs})
    failures += [f"{k}: error {errs[k]:.3e} above 8 x the f32-input run's {errs32[k]:.3e} + 1e-6"
                 for k in errs if k in errs32 and errs[k] > 8.0 * errs32[k] + 1e-6]


# ---------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("cid,fam", FWD_PAIRS)
def test_forward(gpu_device, monkeypatch, cid, fam):
    """every element of e and of the tape of the case's kernel against the float64 statement"""
    sp = FWD[cid]
    n = rows_of(sp["n"], num_cu_of(gpu_device))
    c, v, mg, st = fwd_reference(fam, n, sp["E"])
    for k, val in sp["env"].items():
        monkeypatch.setenv(k, val)
    split = sp["kern"].startswith("h2")
    if sp["save"] and split:
        assert tape_layout(sp["E"], n) == sp["layout"]                     # the case reaches the schedule it names
    got = run_fwd(gpu_device, c, sp["save"])
    failures = []
    errs = hold(fam, got, v, mg, failures)
    if fam == "exact":
        dead = c["d_src"] <= 0
        if not same_bits(got["e"][dead], np.zeros((int(dead.sum()), sp["E"]), np.float32)):
            failures.append("e: a dead row is not +0")
    elif split:
        hold_stats("fwd", cid, got, v, mg, st, failures)
        if not failures:
            monkeypatch.setenv("NG_EDGE_MATH", "fp32")
            against_fp32(cid, errs, hold(fam, run_fwd(gpu_device, c, sp["save"]), v, mg, failures), failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("E,env", RANGE_ROWS, ids=["E8", "E3-bwdfp32"])
def test_range_fallback_row_major_tape(gpu_device, monkeypatch, E, env):
    """operands beyond the fp16 range where the split-operand forward would have written a ROW-MAJOR tape (edge_fwd_h2_kernel<1>):
    the f32-input kernel behind it answers the call; float64 bound, and the bits of the explicit NG_EDGE_MATH=fp32 run"""
    n = 1000
    d_src, centers, gap, Ws, bs = _overflow_case(n, E)
    c = dict(n=n, E=E, d_src=f32(d_src), d_eff=f32(d_src), centers=f32(centers), gap=float(np.float32(gap)),
             Ws=[f32(w) for w in Ws], bs=[f32(b) for b in bs])
    v, mg = R.ref_forward(*_args(c))
    assert np.abs(v["z"][2]).max() > 65504
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    assert tape_layout(E, n) == 0
    got = run_fwd(gpu_device, c, True)
    failures = []
    hold("normal", got, v, mg, failures)
    monkeypatch.setenv("NG_EDGE_MATH", "fp32")
    got32 = run_fwd(gpu_device, c, True)
    for (name, a), (_, b) in zip(R.tensors(got), R.tensors(got32)):
        if not same_bits(a, b):
            failures.append(f"{name}: not the bits of the NG_EDGE_MATH=fp32 run")
    assert not failures, "\n".join(failures)


def test_profile_names_follow_the_switch(gpu_device, monkeypatch):
    """the profile scopes of the forward: edge_fwd_h2 with edge_fwd_range_fallback behind it by default, edge_fused_fwd alone under
    NG_EDGE_MATH=fp32"""
    c, _, _, _ = fwd_reference("normal", 257, 3)
    ctx = _ctx()
    seen = {}
    for math in ("f16x2", "fp32"):
        monkeypatch.setenv("NG_EDGE_MATH", math)
        ctx.prof_enable(True)
        ctx.prof_reset()
        run_fwd(gpu_device, c, True)
        seen[math] = set(ctx.prof_read())
        ctx.prof_enable(False)
    fwd_names = {"edge_fwd_h2", "edge_fwd_range_fallback", "edge_fused_fwd"}
    assert seen["f16x2"] & fwd_names == {"edge_fwd_h2", "edge_fwd_range_fallback"}, seen
    assert seen["fp32"] & fwd_names == {"edge_fused_fwd"}, seen


@pytest.mark.parametrize("kern", list(LIVE_FWD))
def test_forward_does_not_depend_on_the_position(gpu_device, monkeypatch, kern):
    """300 distinct (d_src, d_eff) pairs recur in the first tiles, in tiles a workgroup takes on its second trip and in the ragged
    tail of n_loop rows: e and the tape rows of equal inputs are equal bit for bit (the distances prefetched a tile ahead, the ring
    state carried over and layer 0's weight slab reloaded leave no trace)"""
    E, save, env = LIVE_FWD[kern]
    cu = num_cu_of(gpu_device)
    n = rows_of("n_loop", cu)
    c = dict(R.normal_case(n, E, 5))
    c["d_src"], c["d_eff"] = c["d_src"].copy(), c["d_eff"].copy()
    P = 300
    src = np.arange(P)
    places = [src, 256 * cu + src, n - P + src]
    assert 256 * cu >= P and n - P >= 256 * cu + P
    c["d_src"][src[::17]] = 0.0                                            # a few dead pairs among them
    c["d_eff"][src[::17]] = 0.0
    for p in places[1:]:
        c["d_src"][p], c["d_eff"][p] = c["d_src"][src], c["d_eff"][src]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    got = run_fwd(gpu_device, c, save)
    assert np.isfinite(got["e"]).all()
    for name, g in R.tensors(got):
        for p in places[1:]:
            assert same_bits(g[p], g[src]), (name, int(p[0]))


# --------------------------------------------------------------------------------------------------------------------- backward
def _bwd_env_ok(sp, n):
    """the switches in force send the call to the kernel the case names"""
    blocked_now = tape_layout(sp["E"], n) == 1
    if sp["kern"] == "bh2":
        assert sp["layout"] == 1 or blocked_now
    else:
        assert sp["layout"] == 0 and not blocked_now


@pytest.mark.parametrize("cid,fam", BWD_PAIRS)
def test_backward(gpu_device, monkeypatch, cid, fam):
    """every element of dW[0..3] and db[0..3] of the case's kernel against the float64 statement"""
    sp = BWD[cid]
    n = rows_of(sp["n"], num_cu_of(gpu_device))
    c, v, mg, st = bwd_reference(fam, n, sp["E"])
    for k, val in sp["env"].items():
        monkeypatch.setenv(k, val)
    _bwd_env_ok(sp, n)
    got = run_bwd(gpu_device, c, sp["layout"])
    failures = []
    errs = hold(fam, got, v, mg, failures)
    if fam == "normal" and sp["kern"] == "bh2":
        hold_stats("bwd", cid, got, v, mg, st, failures)
        if not failures:
            monkeypatch.setenv("NG_EDGE_MATH", "fp32")
            assert tape_layout(sp["E"], n) == 0
            against_fp32(cid, errs, hold(fam, run_bwd(gpu_device, c, 0), v, mg, failures), failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n,E", [(33, 4), (4097, 3)])
def test_backward_with_the_tape_in_both_layouts(gpu_device, n, E):
    """the same call with the same tape, handed once blocked (layout 1) and once row-major (layout 0), gives the same bits"""
    c, _, _, _ = bwd_reference("normal", n, E)
    assert tape_layout(E, n) == 1
    a, b = run_bwd(gpu_device, c, 1), run_bwd(gpu_device, c, 0)
    for (name, x), (_, y) in zip(R.tensors(a), R.tensors(b)):
        assert same_bits(x, y), name


@pytest.mark.parametrize("n", UNALIGNED_N)
@pytest.mark.parametrize("fam", ["exact", "normal"])
def test_gradient_scale_unaligned_de(gpu_device, fam, n):
    """de handed as a view that starts 4 bytes into its allocation: hx_absmax_kernel runs element by element at either size.  The
    maximum is exact and order-free, so the scale and every bit of the result equal the aligned call's"""
    E = 3
    c, v, mg, _ = bwd_reference(fam, n, E)
    assert tape_layout(E, n) == 1
    got = run_bwd(gpu_device, c, 1, de_shift=1)
    failures = []
    hold(fam, got, v, mg, failures)
    aligned = run_bwd(gpu_device, c, 1)
    for (name, x), (_, y) in zip(R.tensors(got), R.tensors(aligned)):
        if not same_bits(x, y):
            failures.append(f"{name}: not the bits of the call with an aligned de")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("E", [3, 8])
def test_backward_of_no_edges(gpu_device, E):
    c, _, _, _ = bwd_reference("normal", 0, E)
    got = run_bwd(gpu_device, c, tape_layout(E, 0))
    for name, g in R.tensors(got):
        assert same_bits(g, np.zeros_like(g)), name


def test_blocked_tape_refused_at_E8(gpu_device):
    """a blocked tape can only be read by the split-operand kernel, which stops at E = 4: NG_ERR_INVALID with the sources' message,
    no backward kernel launched and every output left with its fill"""
    c, _, _, _ = bwd_reference("normal", 64, 8)
    ctx = _ctx()
    ctx.prof_enable(True)
    ctx.prof_reset()
    rc, msg = run_bwd(gpu_device, c, 1, refused=True)
    names = set(ctx.prof_read())
    ctx.prof_enable(False)
    assert rc == -1 and "edge_mlp_bwd: blocked tape for an unsupported shape" in msg, (rc, msg)
    assert not names & {"edge_bwd_h2", "edge_bwd_h2_prep", "edge_fused_bwd", "edge_bwd_range_fallback", "edge_bwd_reduce"}, names


# -------------------------------------------------------------------------------------------------------------------- live view
@pytest.mark.parametrize("p_dead", LIVE_P)
@pytest.mark.parametrize("kern", list(LIVE_FWD))
def test_live_forward(gpu_device, monkeypatch, kern, p_dead):
    """ng_edge_mlp_fwd_live: live rows against float64 through the per-element bound (tape row r = the r-th live slot), dead slots
    exactly 0; with every slot dead e is all zero"""
    E, save, env = LIVE_FWD[kern]
    c, v, mg, _ = fwd_reference("normal", LIVE_N, E, p_dead)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    live = build_live(gpu_device, c["d_src"])
    assert (len(live["idx"]) == 0) == (p_dead == 1.0)
    got = run_fwd(gpu_device, c, save, live)
    failures = []
    hold("normal", got, v, mg, failures, sel=live["idx"])
    dead = c["d_src"] <= 0
    assert same_bits(got["e"][dead], np.zeros((int(dead.sum()), E), np.float32))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("p_dead", LIVE_P)
@pytest.mark.parametrize("kern", list(LIVE_BWD))
def test_live_backward(gpu_device, monkeypatch, kern, p_dead):
    """ng_edge_mlp_bwd_live (edge_bwd_h2_kernel<true> / edge_fused_bwd_kernel with perm): the tape holds the live rows only, de keeps
    the caller's slots; gradients against float64, exactly zero when every slot is dead"""
    E, env = LIVE_BWD[kern]
    c, v, mg, _ = bwd_reference("normal", LIVE_N, E, p_dead)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    layout = tape_layout(E, LIVE_N)
    assert layout == (1 if kern == "bh2<true>" else 0)
    live = build_live(gpu_device, c["d_src"])
    got = run_bwd(gpu_device, c, layout, live)
    failures = []
    hold("normal", got, v, mg, failures)
    if p_dead == 1.0:
        for name, g in R.tensors(got):
            assert same_bits(g, np.zeros_like(g)), name
    assert not failures, "\n".join(failures)
