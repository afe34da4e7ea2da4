"""Every kernel form of csrc/input_grad.hip's position gradient and of csrc/box_grad.hip through the C entry points, against
tests/geom_grad_ref.py (checked on the CPU by test_geom_grad_ref_host.py): the grid family bit for bit (dpos) and within
(terms + C_BOX) 2^-53 mag (S, B), the float family within its per-element bounds.  Every output is filled with NaN before the
call and carries eight guard words; every call runs twice and must give the same bits.

  positions_grad_kernel<DispOpen>, padded / CSR         ng_positions_grad, _csr          N = 1, 2, 255, 256, 257, 700; K = 1, 5, 16
  <DispOrtho>, <DispTric>, padded / CSR                 ng_positions_grad_pbc, _csr_pbc  G = 1, 3, 5 frames of n = 1, 85, 257, a
                                                                                         different box per frame
  <DispTric>, the rolled image search                   same                             a box thin along c (reach 1, 2, 3)
  positions_grad_ragged_kernel, padded / CSR            _ragged_pbc, _csr_ragged_pbc     sizes 1, 2, 17, 0, 255, 256, 300, kinds
                                                                                         mixed, kind_host given and NULL
  box_grad_chunk_kernel<Open | Ortho | Tric | Per>      ng_box_grad, _csr, _ragged,      the frame patterns of
  + box_grad_frame_kernel                               _csr_ragged                      geom_grad_ref.BOX_PATTERNS"""
import ctypes as C
import functools

import numpy as np
import pytest

import geom_grad_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 8
RATIOS = {}
FORMS = ["padded", "csr"]
FAMILIES = ["grid", "float"]


# ---- calls ----------------------------------------------------------------------------------------------------------------

def _env(dev):
    import torch
    from nmrgnn_amd import _lib
    ctx = _lib.get_context(dev.index)
    return ctx, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _in(a, dtype, dev):
    """an input on the device, with guard words behind it so that an empty list still has an address"""
    import torch
    a = np.asarray(a).reshape(-1)
    return torch.from_numpy(np.concatenate([a.astype(dtype), np.zeros(GUARD, dtype)])).to(dev)


def _poison(n, dtype, dev):
    import torch
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev)


def _untouched(t):
    return bool(t.isnan().all())


class Batch:
    """the device copies of one case"""

    def __init__(self, c, dev, shuffled=False):
        self.c, self.dev = c, dev
        self.pos, self.dd = _in(c.pos, F32, dev), _in(c.dd, F32, dev)
        self.gp, self.box, self.kind = _in(c.gp, np.int32, dev), _in(c.box, F32, dev), _in(c.kinds, np.int32, dev)
        self.csc_ptr = _in(c.csc_ptr, np.int32, dev)
        self.csc_edge = _in(c.csc_edge_shuffled if shuffled else c.csc_edge, np.int32, dev)
        if c.form == "padded":
            self.nlist, self.edges = _in(c.nlist, np.int32, dev), _in(c.edges, F32, dev)
        else:
            self.row_ptr, self.col, self.row_of = (_in(x, np.int32, dev) for x in (c.row_ptr, c.col, c.row_of))


def call_positions(b, entry, dpos, kind_host=True, **over):
    """one call; entry: 'open', 'pbc' (n = the first frame's size, the flag of the first frame's kind) or 'ragged'.  `over`
    replaces arguments by name (the refusal tests); returns the status"""
    from nmrgnn_amd._lib import ptr
    c = b.c
    ctx, st = _env(b.dev)
    a = dict(ctx=ctx.handle, N=c.N, K=c.K, nnz=c.n_entries, scale=float(c.scale), n=c.sizes[0] if c.sizes else 1,
             tric=int(c.kinds[0]) if c.G else 0, G=c.G, pos=ptr(b.pos), dd=ptr(b.dd), csc_ptr=ptr(b.csc_ptr),
             csc_edge=ptr(b.csc_edge), box=ptr(b.box), gp=ptr(b.gp), kind=ptr(b.kind), dpos=ptr(dpos),
             kh=C.c_void_p(c.kinds.ctypes.data) if kind_host is True else kind_host)
    if c.form == "padded":
        a.update(nlist=ptr(b.nlist), edges=ptr(b.edges))
    else:
        a.update(row_ptr=ptr(b.row_ptr), col=ptr(b.col), row_of=ptr(b.row_of))
    a.update(over)
    L = ctx.lib
    if c.form == "padded":
        head = (a["ctx"], st, a["N"], a["K"], a["pos"], a["nlist"], a["edges"], a["dd"], a["scale"], a["csc_ptr"], a["csc_edge"])
        name = {"open": "ng_positions_grad", "pbc": "ng_positions_grad_pbc", "ragged": "ng_positions_grad_ragged_pbc"}[entry]
    else:
        head = (a["ctx"], st, a["N"], a["nnz"], a["pos"], a["row_ptr"], a["col"], a["row_of"], a["dd"], a["scale"], a["csc_ptr"],
                a["csc_edge"])
        name = {"open": "ng_positions_grad_csr", "pbc": "ng_positions_grad_csr_pbc",
                "ragged": "ng_positions_grad_csr_ragged_pbc"}[entry]
    tail = {"open": (), "pbc": (a["n"], a["box"], a["tric"]), "ragged": (a["G"], a["gp"], a["box"], a["kind"], a["kh"])}[entry]
    return getattr(L, name)(*head, *tail, a["dpos"])


def call_box(b, policy, strain, dvec, kind_host=True, **over):
    """policy: 'open', 'ortho', 'tric' (ng_box_grad(_csr), one flag for the batch) or 'per' (the ragged entry points)"""
    from nmrgnn_amd._lib import ptr
    c = b.c
    ctx, st = _env(b.dev)
    a = dict(ctx=ctx.handle, N=c.N, K=c.K, nnz=c.n_entries, scale=float(c.scale), G=c.G, pos=ptr(b.pos), dd=ptr(b.dd),
             box=ptr(b.box), gp=ptr(b.gp), kind=ptr(b.kind), strain=ptr(strain), dvec=ptr(dvec), tric=R.KIND_OF.get(policy, 0),
             kh=C.c_void_p(c.kinds.ctypes.data) if kind_host is True else kind_host)
    if c.form == "padded":
        a.update(nlist=ptr(b.nlist), edges=ptr(b.edges))
    else:
        a.update(row_ptr=ptr(b.row_ptr), col=ptr(b.col))
    a.update(over)
    L = ctx.lib
    if c.form == "padded":
        head = (a["ctx"], st, a["N"], a["K"], a["pos"], a["nlist"], a["edges"], a["dd"], a["scale"], a["G"], a["gp"], a["box"])
        name = "ng_box_grad_ragged" if policy == "per" else "ng_box_grad"
    else:
        head = (a["ctx"], st, a["N"], a["nnz"], a["pos"], a["row_ptr"], a["col"], a["dd"], a["scale"], a["G"], a["gp"], a["box"])
        name = "ng_box_grad_csr_ragged" if policy == "per" else "ng_box_grad_csr"
    mid = (a["kind"], a["kh"]) if policy == "per" else (a["tric"],)
    return getattr(L, name)(*head, *mid, a["strain"], a["dvec"])


def run_positions(dev, c, entry, shuffled=False, kind_host=True):
    """dpos [N, 3] float32 of two identical calls (same bits), guards checked"""
    import torch
    b = Batch(c, dev, shuffled)
    runs = []
    for _ in range(2):
        out = _poison(3 * c.N, torch.float32, dev)
        assert call_positions(b, entry, out, kind_host) == 0
        torch.cuda.synchronize(dev)
        assert _untouched(out[3 * c.N:])
        runs.append(out[:3 * c.N].cpu().numpy().reshape(c.N, 3))
    np.testing.assert_array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32), err_msg="run to run")
    return runs[0]


def run_box(dev, c, policy, want_dvec=True, kind_host=True):
    import torch
    b = Batch(c, dev)
    runs = []
    for _ in range(2):
        S, B = _poison(9 * c.G, torch.float64, dev), _poison(9 * c.G, torch.float64, dev)
        assert call_box(b, policy, S, B if want_dvec else None, kind_host) == 0
        torch.cuda.synchronize(dev)
        assert _untouched(S[9 * c.G:]) and _untouched(B[9 * c.G:] if want_dvec else B)
        runs.append((S[:9 * c.G].cpu().numpy().reshape(c.G, 3, 3), B[:9 * c.G].cpu().numpy().reshape(c.G, 3, 3)))
    for x, y in zip(*runs):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64), err_msg="run to run")
    return runs[0] if want_dvec else (runs[0][0], None)


# ---- checks ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(family, form, sizes, kinds, seed, K=5, boxes=None, coincident=False):
    c = R.make_case(family, form, list(sizes), list(kinds), seed, K, boxes=list(boxes) if boxes else None, coincident=coincident)
    return c, R.references(c)


def _note(kernel, r):
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)
    print(f"{kernel}: largest |got - ref| / bound so far {RATIOS[kernel]:.3f}")


def check_positions(c, rp, got, kernel):
    assert got.shape == (c.N, 3) and np.isfinite(got).all(), "a poisoned or non-finite row"
    if c.exact:
        np.testing.assert_array_equal(got.view(np.uint32), (rp.dpos + 0.0).astype(F32).view(np.uint32), err_msg="dpos bits")
    r = R.ratios(c, got, None, None, rp, None)[0] if c.N else 0.0
    _note(kernel, r)
    assert r <= 1.0, r
    p = c.plants
    for name in ("hub", "orphan", "alldead"):
        if name in p:
            i = p[name]
            assert (np.abs(got[i].astype(np.float64) - rp.dpos[i]) <= rp.bound[i]).all(), (name, i, got[i], rp.dpos[i])
    if "hub" in p:
        assert rp.terms[p["hub"]] >= 0.8 * (max(c.sizes) - 2)
        assert rp.terms[p["alldead"]] == ((c.dst == p["alldead"]) & (c.g != 0)).sum()      # incoming terms alone


def check_box(c, rb, S, B, kernel):
    assert np.isfinite(S).all() and (B is None or np.isfinite(B).all()), "a poisoned or non-finite frame"
    rs, rbb = R.ratios(c, None, S, B, None, rb)[1:] if c.G else (0.0, 0.0)
    _note(kernel, max(rs, rbb))
    assert rs <= 1.0 and rbb <= 1.0, (rs, rbb)
    for g in range(c.G):
        np.testing.assert_array_equal(S[g], S[g].T)
        if B is not None and (c.kinds[g] < 0 or c.sizes[g] == 0):
            assert (B[g] == 0).all()
        if c.sizes[g] == 0:
            assert (S[g] == 0).all()


def positions_all_orders(dev, c, rp, entry, kernel, kind_host=True):
    got = run_positions(dev, c, entry, kind_host=kind_host)
    check_positions(c, rp, got, kernel)
    sh = run_positions(dev, c, entry, shuffled=True, kind_host=kind_host)
    check_positions(c, rp, sh, kernel + " (shuffled incoming lists)")
    if c.exact:
        np.testing.assert_array_equal(got.view(np.uint32), sh.view(np.uint32))
    return got


# ---- the position gradient ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,K", R.OPEN_SHAPES)
def test_positions_open(gpu_device, N, K, family, form):
    c, (rp, _) = case(family, form, (N,), (-1,), 1, K)
    positions_all_orders(gpu_device, c, rp, "open", f"positions_grad_kernel<DispOpen> {form}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", [0, 1], ids=["ortho", "tric"])
@pytest.mark.parametrize("G,n", R.UNIFORM_SHAPES)
def test_positions_uniform_boxes(gpu_device, G, n, kind, family, form):
    c, (rp, _) = case(family, form, (n,) * G, (kind,) * G, 2)
    if G > 1:
        assert len({tuple(b) for b in c.box.tolist()}) == G            # a different box per frame
    positions_all_orders(gpu_device, c, rp, "pbc", f"positions_grad_kernel<{'DispTric' if kind else 'DispOrtho'}> {form}")


@pytest.mark.parametrize("form", FORMS)
def test_positions_thin_box_rolled_search(gpu_device, form):
    c, (rp, _) = case("grid", form, (300,), (1,), 5, 5, (R.THIN_BOX,))
    assert max(R.kernel_reach(c.box[0].astype(np.float64).reshape(3, 3))) >= 2
    _, n, _, _, _ = c.disp(c.pos, c.src, c.dst)
    u0 = (c.pos[c.dst].astype(np.float64) - c.pos[c.src]).copy()
    h = c.box[0].astype(np.float64).reshape(3, 3)
    ns = np.zeros_like(u0)
    for r in (2, 1, 0):
        ns[:, r] = -np.rint(u0[:, r] / h[r, r])
        u0 += ns[:, r][:, None] * h[r]
    assert (np.abs(n - ns)[:, 2] >= 2).any(), "no pair whose image lies two steps along c from the wrapped vector"
    positions_all_orders(gpu_device, c, rp, "pbc", f"positions_grad_kernel<DispTric> rolled search {form}")


@pytest.mark.parametrize("kind_host", [True, None], ids=["kind_host", "NULL"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", FAMILIES)
def test_positions_ragged(gpu_device, family, form, kind_host):
    c, (rp, _) = case(family, form, tuple(R.RAGGED_SIZES), tuple(R.RAGGED_KINDS), 3)
    assert {-1, 0, 1} == set(c.kinds.tolist()) and 0 in c.sizes
    positions_all_orders(gpu_device, c, rp, "ragged", f"positions_grad_ragged_kernel {form}", kind_host)


POLICIES = ["open", "ortho", "tric", "per"]


def _pair_case(policy):
    """two atoms, one entry 0 -> 1 (CSR), float positions"""
    kind = R.KIND_OF.get(policy, 1)
    pos = np.array([[0.3, 1.7, 16.1], [19.2, 0.4, 0.9]], F32)
    box = (R.FLOAT_TRIC if kind == 1 else np.diag(R.FLOAT_ORTHO)).astype(F32).reshape(1, 9)
    gp = np.array([0, 2], np.int32)
    csc_ptr, csc_edge, _ = R.GL.incoming_lists(np.array([1]), None, 2, 0)
    return R.SimpleNamespace(
        family="float", form="csr", exact=False, scale=R.FLOAT_SCALE, N=2, G=1, K=0, gp=gp, sizes=[2], kinds=np.array([kind], np.int32),
        box=box, pos=pos, plants={}, disp=R.make_disp(gp, [kind], box, False), src=np.array([0]), dst=np.array([1]),
        g=np.array([0.7], F32), dd=np.array([0.7], F32), row_ptr=np.array([0, 1, 1], np.int32), col=np.array([1], np.int32),
        row_of=np.array([0], np.int32), n_entries=1, csc_ptr=csc_ptr.astype(np.int32), csc_edge=csc_edge.astype(np.int32),
        csc_edge_shuffled=csc_edge.astype(np.int32))


@pytest.mark.parametrize("policy", POLICIES)
def test_one_edge_is_antisymmetric(gpu_device, policy):
    """what one atom gains the other loses, bit for bit, in each of the four kernels"""
    c = _pair_case(policy)
    entry = {"open": "open", "per": "ragged"}.get(policy, "pbc")
    got = run_positions(gpu_device, c, entry)
    assert (got[0] != 0).all()
    np.testing.assert_array_equal(got[0].view(np.uint32), (-got[1]).view(np.uint32))
    rp = R.ref_positions_grad(c.pos, c.src, c.dst, c.g, c.scale, c.disp)
    check_positions(c, rp, got, f"one edge {policy}")


# ---- the box gradient -----------------------------------------------------------------------------------------------------

EXPECTED_PATHS = {
    "small40": [("partial", 1)] + ["inside"] * 38 + [("partial", 1)],
    "f256": [("partial", 1)],
    "f257": [("partial", 2)],
    "f700": [("partial", 3)],
    "boundary": [("partial", 1)] * 3,                   # the second frame ends on the chunk boundary
    "empties": ["empty", ("partial", 1), "empty", "empty", ("partial", 2), "inside", "empty", ("partial", 1), "empty"],
    "one100": [("partial", 1)],
}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("pattern", list(R.BOX_PATTERNS))
def test_box_grad_frame_patterns(gpu_device, pattern, policy, family):
    sizes = R.BOX_PATTERNS[pattern]
    kernel = f"box_grad_chunk_kernel<{ {'open': 'DispOpen', 'ortho': 'DispOrtho', 'tric': 'DispTric', 'per': 'DispPer'}[policy]}>"
    for form in FORMS:
        c, (_, rb) = case(family, form, tuple(sizes), tuple(R.pattern_kinds(policy, len(sizes))), 4)
        assert R.frame_paths(c.gp, c.N) == EXPECTED_PATHS[pattern]
        if pattern == "boundary":
            assert c.gp[2] % R.BG_ROWS == 0
        S, B = run_box(gpu_device, c, policy)
        check_box(c, rb, S, B, f"{kernel} {form}")
        if any(k >= 0 and s >= 30 for k, s in zip(c.kinds, sizes)):
            assert np.abs(rb.B).max() > 0
        if pattern in ("one100", "small40"):                  # dvec = NULL: the same strain, nothing else written
            S2, _ = run_box(gpu_device, c, policy, want_dvec=False)
            np.testing.assert_array_equal(S.view(np.uint64), S2.view(np.uint64))
        if pattern == "empties" and policy == "per":          # the ragged entry points without the host copy of the kinds
            S3, B3 = run_box(gpu_device, c, policy, kind_host=None)
            np.testing.assert_array_equal(S.view(np.uint64), S3.view(np.uint64))
            np.testing.assert_array_equal(B.view(np.uint64), B3.view(np.uint64))


# ---- entries of length zero -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("policy", POLICIES)
def test_zero_length_entries_contribute_nothing(gpu_device, policy, family):
    """a CSR pair of coincident atoms (in a box: one lattice translation apart on the grid) listed both ways with dd != 0: the
    gradient of |r| at 0 is taken as 0, so dpos, S and B are finite and equal the reference, which leaves the pair out"""
    sizes = (40, 300, 17)
    c, (rp, rb) = case(family, "csr", sizes, tuple(R.pattern_kinds(policy, 3)) if policy == "per" else (R.KIND_OF[policy],) * 3, 6,
                       coincident=True)
    a, b = c.plants["coincident"]
    sel = (c.src == a) & (c.dst == b)
    assert sel.sum() == 1 and c.g[sel][0] != 0
    u = c.disp(c.pos, c.src[sel], c.dst[sel])[0]
    assert (u == 0).all()
    entry = {"open": "open", "per": "ragged"}.get(policy)
    if entry:
        check_positions(c, rp, run_positions(gpu_device, c, entry), f"zero length, positions {policy}")
    else:                                                    # the uniform entry points take frames of one size
        cu, (rpu, _) = case(family, "csr", (85, 85, 85), (R.KIND_OF[policy],) * 3, 6, coincident=True)
        check_positions(cu, rpu, run_positions(gpu_device, cu, "pbc"), f"zero length, positions {policy}")
    S, B = run_box(gpu_device, c, policy)
    check_box(c, rb, S, B, f"zero length, box {policy}")


@pytest.mark.parametrize("boxed", [False, True], ids=["open", "box"])
def test_cutoff_batch_with_coincident_atoms(gpu_device, boxed):
    """the way a caller meets such entries: the cutoff builder lists two atoms on one point (edges = 0 both ways), and
    GraphBatch.positions_grad / box_grad get dedges of the caller's own.  Finite, and the bits of the same call with those
    entries' dedges set to zero"""
    import torch
    from nmrgnn_amd.graph import frames_to_batch_cutoff
    rng = np.random.default_rng(12)
    n = 120
    frames = (rng.random((2, n, 3)) * 10.0).astype(F32)
    frames[0, 7] = frames[0, 3]
    frames[1, 100] = frames[1, 20]
    atoms = np.eye(4, dtype=F32)[np.arange(n) % 4]
    batch = frames_to_batch_cutoff(atoms, frames, cutoff=3.0, box=np.array([10.0, 10.0, 10.0, 90, 90, 90]) if boxed else None)
    assert batch.is_csr
    zero = batch.edges == 0
    assert int(zero.sum()) == 4
    dd = torch.from_numpy(rng.standard_normal(batch.edges.numel()).astype(F32)).to(gpu_device).reshape(batch.edges.shape)
    assert bool((dd[zero] != 0).all())
    dd0 = torch.where(zero, torch.zeros_like(dd), dd)
    dpos, (S, B) = batch.positions_grad(dd), batch.box_grad(dd)
    assert bool(dpos.isfinite().all()) and bool(S.isfinite().all()) and bool(B.isfinite().all())
    assert torch.equal(dpos, batch.positions_grad(dd0))
    S0, B0 = batch.box_grad(dd0)
    assert torch.equal(S, S0) and torch.equal(B, B0)
    assert float(dpos.abs().max()) > 0 and float(S.abs().max()) > 0 and (not boxed or float(B.abs().max()) > 0)


def _zeroed_atom(c):
    """a copy of case c in which every entry from or to one atom carries dd = 0 (half of them -0.0) and that atom sits at
    infinity; the reference is taken on the finite positions, where those entries are skipped all the same"""
    import copy
    out_deg, in_deg = np.bincount(c.src, minlength=c.N), np.bincount(c.dst, minlength=c.N)
    z = int(np.nonzero((out_deg >= 2) & (in_deg >= 2) & (np.arange(c.N) != c.plants["hub"]))[0][0])
    touch = np.nonzero((c.src == z) | (c.dst == z))[0]
    d = copy.copy(c)
    d.g = c.g.copy()
    d.g[touch] = np.where(np.arange(len(touch)) % 2 == 0, F32(0.0), F32(-0.0))
    if c.form == "padded":
        flat = np.nonzero((c.edges > 0).reshape(-1))[0]
        dd = c.dd.reshape(-1).copy()
        dd[flat] = d.g
        d.dd = dd.reshape(c.dd.shape)
    else:
        d.dd = d.g.copy()
    refs = R.references(d)
    d.pos = c.pos.copy()
    d.pos[z] = F32(np.inf)
    return d, z, refs


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("policy", POLICIES)
def test_zero_weight_entries_are_skipped_whatever_their_geometry(gpu_device, policy, family, form):
    """dd == 0 means skipped on BOTH ends of an entry, not multiplied by: an atom at infinity whose entries all carry dd = 0
    gets a zero row and leaves its neighbours, and its frame's S and B, what they are without it"""
    kinds = tuple(R.pattern_kinds(policy, 3)) if policy == "per" else (R.KIND_OF[policy],) * 3
    c, _ = case(family, form, (85, 85, 85), kinds, 10)
    d, z, (rp, rb) = _zeroed_atom(c)
    got = run_positions(gpu_device, d, {"open": "open", "per": "ragged"}.get(policy, "pbc"))
    assert (got[z] == 0).all() and rp.terms[z] == 0
    check_positions(d, rp, got, f"zero weight, positions {policy}")
    S, B = run_box(gpu_device, d, policy)
    check_box(d, rb, S, B, f"zero weight, box {policy}")


# ---- refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_alone(gpu_device):
    import torch
    dev = gpu_device
    cases = {f: case("float", f, (17, 17), (1, 1), 8)[0] for f in FORMS}
    batches = {f: Batch(c, dev) for f, c in cases.items()}
    dpos = _poison(3 * 34, torch.float32, dev)
    S, B = _poison(18, torch.float64, dev), _poison(18, torch.float64, dev)
    bad_kind = np.array([1, 2], np.int32)
    kh_bad = C.c_void_p(bad_kind.ctypes.data)
    P, X = batches["padded"], batches["csr"]
    pos_calls = [
        (P, "open", dict(K=0)), (P, "pbc", dict(K=0)), (P, "ragged", dict(K=0)),
        (P, "open", dict(N=1 << 27, K=16)), (P, "pbc", dict(N=1 << 27, K=16, n=1)), (P, "ragged", dict(N=1 << 27, K=16)),
        (X, "open", dict(nnz=-1)), (X, "pbc", dict(nnz=-1)), (X, "ragged", dict(nnz=-1)),
        (X, "open", dict(nnz=1 << 31)),
        (P, "pbc", dict(tric=2)), (X, "pbc", dict(tric=2)), (P, "pbc", dict(tric=-1)),
        (P, "pbc", dict(n=5)), (X, "pbc", dict(n=5)), (P, "pbc", dict(n=0)),
        (P, "pbc", dict(box=None)), (X, "pbc", dict(box=None)), (P, "ragged", dict(box=None)), (X, "ragged", dict(box=None)),
        (P, "open", dict(edges=None)), (P, "pbc", dict(edges=None)), (P, "ragged", dict(edges=None)),
        (X, "open", dict(row_ptr=None)), (X, "pbc", dict(row_ptr=None)), (X, "ragged", dict(row_ptr=None)),
        (X, "open", dict(row_of=None)), (X, "pbc", dict(row_of=None)), (X, "ragged", dict(row_of=None)),
        (P, "ragged", dict(G=0)), (X, "ragged", dict(G=0)),
        (P, "ragged", dict(kh=kh_bad)), (X, "ragged", dict(kh=kh_bad)),
        (P, "ragged", dict(gp=None)), (P, "ragged", dict(kind=None)), (P, "open", dict(dpos=None)),
    ]
    for b, entry in ((P, "open"), (P, "pbc"), (P, "ragged"), (X, "open"), (X, "pbc"), (X, "ragged")):
        pos_calls.append((b, entry, dict(ctx=None)))
    for b, entry, over in pos_calls:
        rest = {k: v for k, v in over.items() if k != "dpos"}
        assert call_positions(b, entry, None if "dpos" in over else dpos, **rest) != 0, (b.c.form, entry, over)
    box_calls = [
        (P, "tric", dict(K=0)), (P, "per", dict(K=0)), (P, "tric", dict(N=1 << 27, K=16)), (P, "per", dict(N=1 << 27, K=16)),
        (X, "tric", dict(nnz=-1)), (X, "per", dict(nnz=-1)),
        (P, "tric", dict(tric=2)), (X, "tric", dict(tric=2)), (P, "tric", dict(tric=-2)),
        (P, "tric", dict(box=None)), (X, "ortho", dict(box=None)), (P, "per", dict(box=None)), (X, "per", dict(box=None)),
        (P, "tric", dict(edges=None)), (P, "per", dict(edges=None)), (X, "tric", dict(row_ptr=None)), (X, "per", dict(row_ptr=None)),
        (P, "tric", dict(G=0)), (X, "tric", dict(G=0)), (P, "per", dict(G=0)), (X, "per", dict(G=0)), (P, "tric", dict(G=-1)),
        (P, "per", dict(kh=kh_bad)), (X, "per", dict(kh=kh_bad)), (P, "per", dict(kind=None)),
        (P, "tric", dict(gp=None)), (P, "tric", dict(strain=None)),
        (P, "tric", dict(ctx=None)), (X, "tric", dict(ctx=None)), (P, "per", dict(ctx=None)), (X, "per", dict(ctx=None)),
    ]
    for b, policy, over in box_calls:
        rest = {k: v for k, v in over.items() if k != "strain"}
        assert call_box(b, policy, None if "strain" in over else S, B, **rest) != 0, (b.c.form, policy, over)
    torch.cuda.synchronize(dev)
    assert _untouched(dpos) and _untouched(S) and _untouched(B)
    # N = 0: fine, and nothing is written (the position gradient; the box gradient of G frames without atoms is G zeros)
    for b, entry in ((P, "open"), (P, "pbc"), (P, "ragged"), (X, "open"), (X, "pbc"), (X, "ragged")):
        assert call_positions(b, entry, dpos, N=0, nnz=0) == 0, (b.c.form, entry)
        assert call_positions(b, entry, dpos, N=0, nnz=0, G=0) == 0
    for b, policy in ((P, "tric"), (P, "per"), (X, "tric"), (X, "per")):
        assert call_box(b, policy, S, B, N=0, nnz=0, G=0) == 0
    torch.cuda.synchronize(dev)
    assert _untouched(dpos) and _untouched(S) and _untouched(B)
    # the valid call still works after all of that
    for f, b in batches.items():
        rp, _ = case("float", f, (17, 17), (1, 1), 8)[1]
        check_positions(b.c, rp, run_positions(dev, b.c, "pbc"), "after the refusals")
