"""Every kernel and branch of csrc/graph_ops.hip through its C entry points (ng_build_incoming_lists, ng_build_live_edges,
ng_build_graph_lists, ng_graph_lists_one_launch) and its Python callers (GraphBatch), against the integer statement of
tests/graph_lists_ref.py (checked on the CPU by test_graph_lists_ref_host.py).  Everything here is integers or copied floats: every
comparison is exact, d_c as uint32.

Every output is filled with -7 (-7.0) before the call and carries eight guard words behind its extent; nothing behind what the
header promises may change: csc_edge[total:], d_c[n_live:], the guards.  The builders with atomics (the unordered fill of the
incoming lists) run twice and must give the same bits.

Dispatch, from the conditions in the source (N targets, n entries or slots; TILE = 1024, caps 2048 targets / 16384 slots):
  ng_build_incoming_lists   N == 0 -> csc_ptr[0] = 0 and return
                            1 <= N <= 2048, 0 < n <= 16384, K > 0 -> gl_lists_small_kernel (gl_lists_small_body)
                            else (N or n over a cap, n == 0, or the CSR form K == 0) -> gl_count_kernel (n > 0), gl_scan_local_kernel
                            [ceil(N / 1024) blocks], gl_scan_sums_kernel [one trip per 256 block totals, carry between trips],
                            gl_scan_apply_kernel, gl_fill_kernel (n > 0), gl_sort_kernel [16 targets per block; a segment of
                            <= 64 entries: 16-lane rank loop; 65..4096: bitonic sort in LDS; > 4096: chunked rank sort]
  ng_build_live_edges       n == 0 -> *n_live = 0;  n <= 16384 -> gl_live_small_kernel (gl_live_small_body)
                            else gl_live_count_kernel, gl_live_scan_kernel [one trip per 256 tiles of 1024 slots, carry between
                            trips], gl_live_fill_kernel
  ng_build_graph_lists      gl_small_shape(N, K, N K) [the one-launch condition above] -> gl_both_small_kernel (both bodies)
                            else ng_build_incoming_lists, then ng_build_live_edges
gl_scan_small_kernel and gl_scan_offsets_kernel belong to ng_exclusive_scan_i32 (test_gpu_nlist_exact.py)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import graph_lists_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 8
CAP_TARGETS, CAP_SLOTS = 2048, 16384          # GL_SMALL_TARGETS, GL_SMALL_SLOTS
POISON_BITS = int(np.array(-7.0, F32).view(np.uint32))
eq = np.testing.assert_array_equal


def one_launch(N, K):
    """gl_small_shape(N, K, N * K) of the source"""
    return N >= 1 and N <= CAP_TARGETS and N * K <= CAP_SLOTS and N * K > 0 and K > 0


# ---- calls ----------------------------------------------------------------------------------------------------------------

def _env(dev):
    import torch
    from nmrgnn_amd import _lib
    ctx = _lib.get_context(dev.index)
    return ctx, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _poison(n, dtype, dev):
    import torch
    return torch.full((n + GUARD,), -7, dtype=dtype, device=dev)


def _dev(a, dtype, dev):
    import torch
    if a is None or np.asarray(a).size == 0:
        return None
    return torch.from_numpy(np.array(np.asarray(a).reshape(-1), dtype=dtype)).to(dev)       # a copy: the cases are read-only


def _host(outs):
    """numpy copies, floats as their bits"""
    res = {}
    for k, v in outs.items():
        a = v.cpu().numpy()
        res[k] = a.view(np.uint32) if a.dtype == np.float32 else a
    return res


def _outputs(dev, N, n, names):
    import torch
    size = {"csc_ptr": N + 1, "n_live": 1}
    return {k: _poison(size.get(k, n), torch.float32 if k == "d_c" else torch.int32, dev) for k in names}


def _twice(call, dev, N, n, names):
    import torch
    runs = []
    for _ in range(2):
        o = _outputs(dev, N, n, names)
        call(o)
        torch.cuda.synchronize(dev)
        runs.append(_host(o))
    for k in names:
        eq(runs[0][k], runs[1][k], err_msg=f"{k}: run to run")
    return runs[0]


def run_incoming(dev, N, K, nlist, edges, with_c=True):
    from nmrgnn_amd._lib import ptr
    ctx, st = _env(dev)
    n = 0 if nlist is None else int(np.asarray(nlist).size)
    tn, te = _dev(nlist, np.int32, dev), _dev(edges, np.float32, dev)
    names = ["csc_ptr", "csc_edge"] + (["nlist_c"] if K > 0 and with_c else [])

    def call(o):
        ctx.check(ctx.lib.ng_build_incoming_lists(ctx.handle, st, N, K, n, ptr(tn), ptr(te), ptr(o.get("nlist_c")),
                                                  ptr(o["csc_ptr"]), ptr(o["csc_edge"])), "ng_build_incoming_lists")
    return _twice(call, dev, N, n, names)


LIVE = ["perm", "pos", "d_c", "n_live"]


def run_live(dev, edges):
    from nmrgnn_amd._lib import ptr
    ctx, st = _env(dev)
    n = int(np.asarray(edges).size)
    te = _dev(edges, np.float32, dev)

    def call(o):
        ctx.check(ctx.lib.ng_build_live_edges(ctx.handle, st, n, ptr(te), ptr(o["perm"]), ptr(o["pos"]), ptr(o["d_c"]),
                                              ptr(o["n_live"])), "ng_build_live_edges")
    return _twice(call, dev, 0, n, LIVE)


def run_both(dev, N, K, nlist, edges, with_c=True):
    from nmrgnn_amd._lib import ptr
    ctx, st = _env(dev)
    n = N * K
    tn, te = _dev(nlist, np.int32, dev), _dev(edges, np.float32, dev)
    names = ["csc_ptr", "csc_edge"] + (["nlist_c"] if with_c else []) + LIVE

    def call(o):
        ctx.check(ctx.lib.ng_build_graph_lists(ctx.handle, st, N, K, ptr(tn), ptr(te), ptr(o.get("nlist_c")), ptr(o["csc_ptr"]),
                                               ptr(o["csc_edge"]), ptr(o["perm"]), ptr(o["pos"]), ptr(o["d_c"]), ptr(o["n_live"])),
                  "ng_build_graph_lists")
    return _twice(call, dev, N, n, names)


# ---- checks ---------------------------------------------------------------------------------------------------------------

def check_incoming(out, nlist, edges, N, K):
    n = 0 if nlist is None else int(np.asarray(nlist).size)
    ptr, eid, nc = R.incoming_lists(np.zeros(0, np.int32) if nlist is None else nlist, edges, N, K)
    total = int(ptr[-1])
    eq(out["csc_ptr"][:N + 1], ptr)
    eq(out["csc_ptr"][N + 1:], -7)
    assert out["csc_ptr"].shape[0] == N + 1 + GUARD and out["csc_edge"].shape[0] == n + GUARD
    eq(out["csc_edge"][:total], eid)
    eq(out["csc_edge"][total:], -7)               # the dropped entries' share of the buffer and the guard
    if "nlist_c" in out:
        eq(out["nlist_c"][:n], nc)
        eq(out["nlist_c"][n:], -7)
    return ptr


def check_live(out, edges):
    e = np.asarray(edges, F32).reshape(-1)
    n = e.shape[0]
    perm, pos, d_c, n_live = R.live_partition(e)
    eq(out["n_live"], [n_live] + [-7] * GUARD)
    eq(out["perm"][:n], perm)
    eq(out["perm"][n:], -7)
    eq(out["pos"][:n], pos)
    eq(out["pos"][n:], -7)
    assert out["d_c"].dtype == np.uint32 and out["d_c"].shape[0] == n + GUARD
    eq(out["d_c"][:n_live], d_c.view(np.uint32))
    eq(out["d_c"][n_live:], POISON_BITS)         # behind n_live nothing is written, the guard included
    return n_live


# ---- padded cases -----------------------------------------------------------------------------------------------------------

SEG_LENGTHS = (0, 1, 15, 16, 17, 32, 33, 64)          # around the 16 lanes of the rank loop, up to GL_SORT_GROUP_MAX

# name: (N, K, one launch?)  — the third entry is what the dispatch conditions above give; test_one_launch_query holds the
# library's own answer to the same table
PADDED = {
    # gl_lists_small_kernel / gl_both_small_kernel at their smallest: one thread with work, per = 1
    "one_slot": (1, 1, True),
    # total 0: csc_ptr all zero, csc_edge untouched, every nlist_c entry the atom itself, perm = identity (all dead)
    "all_dead_5x2": (5, 2, True),
    # n = 16384 = the slot cap exactly (<=): one launch, 64 KB of dynamic LDS, per = 16 slots per thread in gl_live_small_body
    "cap_1024x16": (1024, 16, True),
    # N = 2048 = the target cap exactly and n = 16384: one launch, the scan's thread 1023 owns targets 2046 and 2047
    "cap_2048x8": (2048, 8, True),
    # n = 16400 > 16384, N under its cap: multi-launch with 2 scan tiles (the second holds one target), gl_live_* multi-launch
    "over_1025x16": (1025, 16, False),
    # N = 2049 > 2048 (n = 16392 over as well): gl_scan_local_kernel with 3 tiles, the last holding one target
    "over_2049x8": (2049, 8, False),
    # 3000 live entries at atom 5 and 17 at the last atom, under both caps: gl_lists_small_body ranks a 3000-entry segment in
    # 16-lane groups (no long-segment branch there), and the last target's segment ends at the total
    "hub_2000x8": (2000, 8, True),
    # segment lengths around the 16 lanes of the rank loop (padding lanes, one and several trips), one launch
    "seg_700x16": (700, 16, True),
    # the same lengths over the target cap: the same loop in gl_sort_kernel (len <= 64: the group branch)
    "seg_2100x8": (2100, 8, False),
}
SEG_TARGETS = {"seg_700x16": (3, 10, 17, 64, 65, 333, 698, 699), "seg_2100x8": (3, 10, 17, 64, 65, 333, 2098, 2099)}


@functools.lru_cache(maxsize=None)
def padded_case(name):
    N, K, _ = PADDED[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    want = {}
    if name == "one_slot":
        nlist, edges = np.zeros((1, 1), np.int32), np.full((1, 1), 0.5, F32)
    elif name == "all_dead_5x2":
        nlist, edges = rng.integers(0, N, (N, K)).astype(np.int32), R.dead_edges(rng, N * K).reshape(N, K)
    else:
        nlist, edges = R.special_batch(rng, N, K)
    if name == "hub_2000x8":
        want = {5: 3000, N - 1: 17}
    elif name in SEG_TARGETS:
        want = dict(zip(SEG_TARGETS[name], SEG_LENGTHS))
    if want:
        R.plant_segments(rng, nlist, edges, N, want, spare=100)
    nlist.setflags(write=False)
    edges.setflags(write=False)
    return N, K, nlist, edges, want


@pytest.mark.parametrize("with_edges", [True, False], ids=["edges", "edges_null"])
@pytest.mark.parametrize("name", list(PADDED))
def test_incoming_lists_padded(gpu_device, name, with_edges):
    N, K, nlist, edges, want = padded_case(name)
    assert one_launch(N, K) == PADDED[name][2]
    e = edges if with_edges else None           # NULL: every entry with a target in [0, N) is live
    out = run_incoming(gpu_device, N, K, nlist, e)
    ptr = check_incoming(out, nlist, e, N, K)
    if with_edges:
        assert {t: int(ptr[t + 1] - ptr[t]) for t in want} == want
        if name == "all_dead_5x2":
            assert ptr[-1] == 0
    # without nlist_c (what GraphBatch.csc() asks for when the lists are built late): the same lists
    if name in ("cap_2048x8", "over_2049x8"):
        out2 = run_incoming(gpu_device, N, K, nlist, e, with_c=False)
        eq(out2["csc_ptr"], out["csc_ptr"])
        eq(out2["csc_edge"], out["csc_edge"])


GRAPH_LISTS = [k for k in PADDED if k != "seg_2100x8"]       # every case at or under the caps, and the two just over them


@pytest.mark.parametrize("name", GRAPH_LISTS)
def test_graph_lists_equal_the_reference_and_the_two_builders(gpu_device, name):
    """gl_both_small_kernel where one_launch(N, K), else the fallback to the two builders, which no Python caller takes
    (GraphBatch asks ng_graph_lists_one_launch first): all seven outputs, and bit for bit what the two separate calls write"""
    N, K, nlist, edges, _ = padded_case(name)
    out = run_both(gpu_device, N, K, nlist, edges)
    check_incoming(out, nlist, edges, N, K)
    check_live(out, edges)
    sep = run_incoming(gpu_device, N, K, nlist, edges)
    sep.update(run_live(gpu_device, edges))
    assert sorted(sep) == sorted(out) and len(out) == 7
    for k in out:
        eq(out[k], sep[k], err_msg=k)
    if name in ("seg_700x16", "over_1025x16"):      # nlist_c is optional in both branches
        out2 = run_both(gpu_device, N, K, nlist, edges, with_c=False)
        for k in out2:
            eq(out2[k], out[k], err_msg=k)


def test_one_launch_query(gpu_device):
    ctx, _ = _env(gpu_device)
    for name, (N, K, one) in PADDED.items():
        assert ctx.lib.ng_graph_lists_one_launch(N, K) == int(one), name
    for N, K in [(0, 4), (-1, 4), (5, 0), (5, -1), (1, 16384), (1, 16385), (2048, 1), (2049, 1), (2048, 9), (16384, 1),
                 (1 << 20, 16), (1 << 31, 1 << 30)]:
        assert ctx.lib.ng_graph_lists_one_launch(N, K) == int(one_launch(N, K)), (N, K)


# ---- CSR cases (K == 0: always the multi-launch form, edges NULL, no nlist_c) -------------------------------------------------

@functools.lru_cache(maxsize=None)
def csr_case(name):
    rng = np.random.default_rng(len(name))
    if name == "three_long":
        # targets 32..47 are one block of gl_sort_kernel (16 targets per block): 65 -> bitonic with m = 128, 4097 -> chunked rank
        # sort (two chunks, the second of one entry), 700 -> bitonic with m = 1024, and 64 on target 47 stays on the group branch:
        # s_nlong = 3, every barrier of the long loop beside a finished group
        N, n = 600, 8000
        want = {32: 65, 33: 4097, 34: 700, 47: 64}
    elif name == "scan_carry":
        # 258 scan tiles: gl_scan_sums_kernel takes a second trip (tiles 256, 257) with the carry of the first, and
        # gl_scan_apply_kernel reads block_sum[i / 1024] for i / 1024 >= 256
        N = 262144 + 1025
        n = int(rng.integers(0, 3, N).sum())              # degrees in {0, 1, 2}
        want = {1023: 3, 1024: 5, 262143: 7, 262144: 2, 262145: 4, N - 1: 6}
    col = rng.integers(0, N, n).astype(np.int32)
    R.plant_segments(rng, col, None, N, want, spare=2000 if N > 2000 else 100)
    col.setflags(write=False)
    return N, col, want


@pytest.mark.parametrize("name", ["three_long", "scan_carry"])
def test_incoming_lists_csr(gpu_device, name):
    N, col, want = csr_case(name)
    out = run_incoming(gpu_device, N, 0, col, None)
    ptr = check_incoming(out, col, None, N, 0)
    assert {t: int(ptr[t + 1] - ptr[t]) for t in want} == want
    assert ptr[-1] == col.shape[0]
    if name == "scan_carry":
        assert -(-N // 1024) == 258 and ptr[262144] > 0


def test_incoming_lists_without_entries_or_atoms(gpu_device):
    # N = 700, n = 0: no count and no fill launch; scan, apply and sort over 700 empty segments -> csc_ptr all zero
    out = run_incoming(gpu_device, 700, 0, None, None)
    check_incoming(out, None, None, 700, 0)
    eq(out["csc_ptr"][:701], 0)
    # N = 0: the early return writes csc_ptr[0] = 0 and nothing else
    out = run_incoming(gpu_device, 0, 0, None, None)
    eq(out["csc_ptr"], [0] + [-7] * GUARD)
    eq(out["csc_edge"], -7)


# ---- live partition -------------------------------------------------------------------------------------------------------------

# 16384: the last one-launch size (per = 16); 16385: the first multi-launch size, 17 tiles, the last with one slot;
# 17407 / 17408 / 17409: a tile edge above the cap (k 1024 - 1, k 1024, k 1024 + 1 with k = 17);
# 262143 / 262144: 256 block totals, one trip of gl_live_scan_kernel; 262145 / 263169: 257 / 258 totals, the carry
LIVE_SIZES = (16384, 16385, 17407, 17408, 17409, 262143, 262144, 262145, 263169)
LIVE_CASES = [(n, "mixed") for n in LIVE_SIZES] + [(n, kind) for n in (16385, 262145)
                                                   for kind in ("all_dead", "all_live", "last_only", "first_only")]


@pytest.mark.parametrize("n,kind", LIVE_CASES)
def test_live_partition(gpu_device, n, kind):
    rng = np.random.default_rng(n)
    if kind == "mixed":
        e = R.special_edges(rng, n, p_dead=0.3)
    elif kind == "all_live":
        e = R.live_edges(rng, n)
    else:
        e = R.dead_edges(rng, n)                       # n_live = 0 (or 1): perm's dead tail starts at its front
        if kind == "last_only":
            e[-1] = F32(0.5)
        elif kind == "first_only":
            e[0] = F32(0.5)
    n_live = check_live(run_live(gpu_device, e), e)
    assert n_live == {"all_dead": 0, "all_live": n, "last_only": 1, "first_only": 1}.get(kind, n_live)
    assert -(-n // 1024) == {16385: 17, 262144: 256, 262145: 257}.get(n, -(-n // 1024))


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(gpu_device):
    """non-zero return, the context's message names the refusal (a different refusal is provoked before each, so that the message
    is this call's), and no output changes"""
    import torch
    from nmrgnn_amd._lib import ptr
    dev = gpu_device
    ctx, st = _env(dev)
    lib, h = ctx.lib, ctx.handle
    N, K = 10, 4
    n = N * K
    nlist, edges = R.special_batch(np.random.default_rng(0), N, K)
    tn, te = _dev(nlist, np.int32, dev), _dev(edges, np.float32, dev)

    def inc(o, **kw):
        a = dict(ctx=h, N=N, K=K, n=n, nlist=ptr(tn), nlist_c=ptr(o["nlist_c"]), csc_ptr=ptr(o["csc_ptr"]), csc_edge=ptr(o["csc_edge"]))
        a.update(kw)
        return lib.ng_build_incoming_lists(a["ctx"], st, a["N"], a["K"], a["n"], a["nlist"], ptr(te), a["nlist_c"], a["csc_ptr"],
                                           a["csc_edge"])

    def both(o, **kw):
        a = dict(ctx=h, K=K, **{k: ptr(o[k]) for k in ("nlist_c", "csc_ptr", "csc_edge", "perm", "pos", "d_c", "n_live")})
        a.update(kw)
        return lib.ng_build_graph_lists(a["ctx"], st, N, a["K"], ptr(tn), ptr(te), a["nlist_c"], a["csc_ptr"], a["csc_edge"],
                                        a["perm"], a["pos"], a["d_c"], a["n_live"])

    def live(o, **kw):
        a = dict(ctx=h, edges=ptr(te), n_live=ptr(o["n_live"]))
        a.update(kw)
        return lib.ng_build_live_edges(a["ctx"], st, n, a["edges"], ptr(o["perm"]), ptr(o["pos"]), ptr(o["d_c"]), a["n_live"])

    cases = [(inc, dict(ctx=None), None),                                   # no context to carry a message: return code only
             (inc, dict(nlist=None), "incoming lists: nlist required"),
             (inc, dict(K=0), "incoming lists: nlist_c needs the padded form"),
             (inc, dict(n=n - 1), "incoming lists: padded form has N*K entries"),
             (inc, dict(N=-1, K=0, n=0, nlist_c=None), "incoming lists: sizes out of range"),
             (inc, dict(csc_ptr=None), "incoming lists: csc_ptr / csc_edge required"),
             (inc, dict(csc_edge=None), "incoming lists: csc_ptr / csc_edge required"),
             (both, dict(ctx=None), None),
             (both, dict(K=0), "graph lists: padded form"),
             (live, dict(ctx=None), None),
             (live, dict(n_live=None), "live edges: arguments"),
             (live, dict(edges=None), "live edges: arguments")]
    cases += [(both, {k: None}, "graph lists: arguments") for k in ("csc_ptr", "csc_edge", "perm", "pos", "d_c", "n_live")]
    for fn, kw, message in cases:
        o = _outputs(dev, N, n, ["nlist_c", "csc_ptr", "csc_edge"] + LIVE)
        assert lib.ng_exclusive_scan_i32(h, st, -1, None, None) != 0
        assert b"exclusive scan" in lib.ng_last_error(h)
        assert fn(o, **kw) != 0, (fn.__name__, kw)
        if message is not None:
            assert message in lib.ng_last_error(h).decode(), (fn.__name__, kw)
        torch.cuda.synchronize(dev)
        for k, v in _host(o).items():
            eq(v, POISON_BITS if k == "d_c" else -7, err_msg=f"{fn.__name__} {kw}: {k}")
    # and the same arguments without the fault are taken (the refusals above are not an accident of the set-up)
    o = _outputs(dev, N, n, ["nlist_c", "csc_ptr", "csc_edge"] + LIVE)
    assert inc(o) == 0 and live(o) == 0 and both(o) == 0
    torch.cuda.synchronize(dev)


# ---- Python callers -------------------------------------------------------------------------------------------------------------

def _np64(t):
    return t.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("N,K", [(700, 16), (2100, 8)], ids=["one_launch", "multi_launch"])
def test_graphbatch_without_validation(gpu_device, N, K):
    """validate=False leaves the builders' own guard as the only one: out-of-range targets and every special distance through
    GraphBatch (ng_build_graph_lists at (700, 16); ng_build_incoming_lists and, on demand, ng_build_live_edges at (2100, 8)),
    and through to_csr() (the CSR form with edges NULL and out-of-range targets in gl_count_kernel / gl_fill_kernel)"""
    from nmrgnn_amd.graph import GraphBatch
    nlist, edges = R.special_batch(np.random.default_rng(N), N, K)
    gb = GraphBatch(np.zeros((N, 10), F32), nlist, edges, np.ones(N, F32), device=gpu_device, validate=False)
    assert (gb._live is not None) == one_launch(N, K)
    ptr, eid, nc = R.incoming_lists(nlist, edges, N, K)
    eq(_np64(gb.nlist_c).reshape(-1), nc)
    cp, ce = gb.csc()
    eq(_np64(cp), ptr)
    eq(_np64(ce)[:ptr[-1]], eid)
    perm, pos, d_c, n_live = gb.live_edges(force=True)
    rp, rq, rd, rn = R.live_partition(edges)
    assert int(n_live.cpu()) == rn
    eq(_np64(perm), rp)
    eq(_np64(pos), rq)
    eq(d_c.cpu().numpy().view(np.uint32)[:rn], rd.view(np.uint32))
    # to_csr keeps exactly the slots with edges > 0, in slot order
    with np.errstate(invalid="ignore"):
        keep = edges > 0
    csr = gb.to_csr()
    eq(_np64(csr.nlist), nlist[keep])
    eq(csr.edges.cpu().numpy().view(np.uint32), edges[keep].view(np.uint32))
    eq(_np64(csr.row_ptr), np.concatenate([[0], np.cumsum(keep.sum(1))]))
    ptr2, eid2, _ = R.incoming_lists(nlist[keep], None, N, 0)
    cp2, ce2 = csr.csc()
    eq(_np64(cp2), ptr2)
    eq(_np64(ce2)[:ptr2[-1]], eid2)


def test_device_lists_equal_the_host_builder(gpu_device):
    """valid targets only (GraphBatch._build_lists_host counts with bincount): padded under and over the caps, and CSR"""
    from nmrgnn_amd.graph import GraphBatch
    rng = np.random.default_rng(9)
    for N, K in [(300, 16), (2500, 8)]:
        nlist = rng.integers(0, N, (N, K)).astype(np.int32)
        edges = R.special_edges(rng, N * K).reshape(N, K)
        a = np.zeros((N, 10), F32)
        dv, hs = (GraphBatch(a, nlist, edges, np.ones(N, F32), device=d) for d in (gpu_device, "cpu"))
        eq(dv.nlist_c.cpu().numpy(), hs.nlist_c.numpy())
        total = int(hs.csc()[0][-1])
        eq(dv.csc()[0].cpu().numpy(), hs.csc()[0].numpy())
        eq(dv.csc()[1].cpu().numpy()[:total], hs.csc()[1].numpy())
    N, nnz = 900, 7000
    row_ptr = np.zeros(N + 1, np.int32)
    row_ptr[1:] = np.cumsum(rng.multinomial(nnz, np.ones(N) / N))
    col = rng.integers(0, N, nnz).astype(np.int32)
    dist = rng.uniform(0.1, 0.4, nnz).astype(F32)
    dv, hs = (GraphBatch.from_csr(np.zeros((N, 10), F32), row_ptr, col, dist, inv_degree=np.ones(N, F32), device=d)
              for d in (gpu_device, "cpu"))
    eq(dv.csc()[0].cpu().numpy(), hs.csc()[0].numpy())
    eq(dv.csc()[1].cpu().numpy()[:nnz], hs.csc()[1].numpy())
