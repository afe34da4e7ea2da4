"""Reference and case builders for the geometry gradients (csrc/input_grad.hip: positions_grad_kernel<DispOpen | DispOrtho |
DispTric>, positions_grad_ragged_kernel; csrc/box_grad.hip: box_grad_chunk_kernel, box_grad_frame_kernel).  NumPy only.

What is stated (include/nmrgnn_hip.h).  For every live entry e = (i -> j) with dd_e != 0 and a displacement u_e = D(r_i, r_j)
of non-zero length:
    dpos[i] -= t_e,  dpos[j] += t_e,        t_e = dd_e * scale * u_e / |u_e|
    S_g += u_e (x) t_e,  B_g += n_e (x) t_e    (g the frame of i; n_e the integer image triple, u_e = r_j - r_i + n_e h_g)
An entry of length zero contributes nothing (the gradient of |r| at 0 is taken as 0); a padded slot is live when edges > 0.

The displacement D is stated once, in `min_image`: the sequential wrap along c, b, a of csrc/pbc.cuh, then the shortest of
the images within `reach` of the wrapped vector, in float64 on the float32 inputs.  Pairs on which that is not well defined
(two shortest images, a wrapped component at half a box width; for random floats two images within 1e-4 in length) are ties:
the case builders leave them out of the lists and report their share.

Two data families:
  grid   positions and lattice vectors are multiples of 1/8 (tests/nlist_ref.py), box diagonals from {8, 16, 32}, dd = +-2^k
         len32 (len32 the correctly rounded float32 length) and scale a power of two.  Every displacement and squared length
         is a float32 number, g * scale / len is exactly +-2^k scale, every product and partial sum is exact: the float32
         dpos equals the reference bit for bit in any summation order (`check_grid_exact` asserts the conditions).  The box
         gradient divides by a float64 square root, so its terms are rounded: bound (terms + C_BOX) 2^-53 mag per element.
  float  random float32 positions, a share of them several boxes out, dd standard normal.

The counted constants (unit roundoffs; 2^-24 for float32, 2^-53 for float64):
  C_PG = 5    dpos bound (terms + C_PG) 2^-24 mag: pg_term rounds the three squares and their two sums (<= 3 roundings of
              the squared length, half of that after the root: 1.5), the root (1), g * scale (1), the quotient (1), f * v
              (1): 5.5; a row of T terms is summed with T - 1 roundings of partial sums no larger than mag; the float64
              reference is below 1e-8 of one float32 rounding.  5.5 + T - 1 <= T + 5.
  C_DISP = 7  roundings on the way to one component of a float32 displacement: c - q (1), three wrap steps (x: 3, y: 2,
              z: 1), three fused steps of the image search.  Each is at most 2^-24 of the largest intermediate value of that
              component, A_a = |d_a| + sum_r (|wrap_r| + |image_r|) |h[r][a]|: an ABSOLUTE error, because an atom several boxes
              out has |d| far above |u|.  It therefore enters per entry, not through mag: a term g scale u_a / |u| moves by at
              most |g scale| (|du_a| + |du|_1) / |u| <= 2 |g scale| C_DISP 2^-24 A / |u|, A = sum_a A_a.  Grid family: zero.
  C_BOX = 8   S, B bound (terms + C_BOX) 2^-53 mag: the squared length (<= 3 roundings, 1.5 after the root), the root (1), the
              quotient (1), w * u_b (1), u_a * (w u_b) or n_a * (w u_b) (1): 5.5, the reference's own rounding to float64 (1,
              it is summed in extended precision), T - 1 for the sums of the row pass, the segmented scan, the chunk
              partials and the butterfly in whatever order: 7.5 + T - 1 <= T + 7, and one spare for second-order terms.
              Float family: plus the displacement error, 2^-24 |g scale| C_DISP 3 A per entry for S (u enters twice and
              through the length) and 2^-24 |n_a| |g scale| C_DISP 2 A / |u| for B."""
import itertools
from types import SimpleNamespace

import numpy as np

import graph_lists_ref as GL
import nlist_ref as NL

F32 = np.float32
U24, U53 = 2.0 ** -24, 2.0 ** -53
C_PG, C_DISP, C_BOX = 5, 7, 8
BG_ROWS = 256
GRID_SCALE, FLOAT_SCALE = 0.125, 0.1
GRID_K = (-2, -1, 0, 1, 2)                 # dd = +-2^k len32
FLOAT_TIE = 1e-4
DEAD_EDGES = (F32(0.0), F32(-0.0), F32(np.nan), F32(-0.3))
DEAD_DD = (F32(np.nan), F32(3.0))
MIN_PLANT = 8                              # frames of at least this many atoms carry the planted rows


# ---- the displacement ---------------------------------------------------------------------------------------------------

def kernel_reach(h):
    """(ni, nj, nk): the reach of DispTric's image search along a, b, c by the rule of csrc/pbc.cuh, in float64"""
    ax, bx, by, cx, cy, cz = h[0, 0], h[1, 0], h[1, 1], h[2, 0], h[2, 1], h[2, 2]
    r = 0.5 * np.sqrt(ax * ax + by * by + cz * cz) * 1.0001
    nk = int(r / cz + 0.5)
    nj = int(r / by + 0.5 + nk * abs(cy) / by)
    ni = max(int(np.ceil((nj * abs(bx) + nk * abs(cx)) / ax)), 1)
    return ni, nj, nk


def min_image(d, h, exact):
    """d [E, 3] float64 = r_j - r_i, h [3, 3] float64 (rows a, b, c, lower triangular) ->
    u [E, 3], n [E, 3] (u = d + n h), tie [E] bool, A [E] (the sum over components of the largest intermediate magnitude).
    Wrap along c, b, a; then the shortest image within max(2, the kernel's reach) of the wrapped vector."""
    E = d.shape[0]
    w = d.copy()
    ns = np.zeros((E, 3))
    for r in (2, 1, 0):
        s = np.rint(w[:, r] / h[r, r])
        w -= s[:, None] * h[r]
        ns[:, r] = -s
    half = (np.abs(w) * 2.0 == np.diag(h)[None, :]).any(1)
    reach = [max(2, x) for x in kernel_reach(h)]
    best = np.full(E, np.inf)
    second = np.full(E, np.inf)
    img = np.zeros((E, 3))
    for k, j, i in itertools.product(*(range(-x, x + 1) for x in reach[::-1])):
        t = np.array([i, j, k], np.float64)
        c = w + t @ h
        c2 = (c * c).sum(1)
        take = c2 < best
        second = np.where(take, best, np.minimum(second, c2))
        best = np.where(take, c2, best)
        img[take] = t
    u = w + img @ h
    if exact:
        tie = (second == best) | half
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            tie = np.sqrt(second) < np.sqrt(best) * (1.0 + FLOAT_TIE)
    A = (np.abs(d) + (np.abs(ns) + np.abs(img)) @ np.abs(h)).sum(1)
    return u, ns + img, tie, A


def make_disp(gp, kinds, box, exact):
    """disp(pos, src, dst) -> (u, n, tie, A, frame) over edges (src -> dst): every edge by the kind and box of src's frame
    (kinds [G]: -1 open, 0 orthorhombic, 1 reduced triclinic; box [G, 9] float32).  An orthorhombic frame reads the diagonal
    alone, as DispOrtho does."""
    gp = np.asarray(gp, np.int64)
    kinds = np.asarray(kinds)
    H = np.asarray(box, F32).astype(np.float64).reshape(-1, 3, 3)

    def disp(pos, src, dst):
        p = np.asarray(pos, F32).astype(np.float64)
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        frame = np.searchsorted(gp, src, side="right") - 1
        d = p[dst] - p[src]
        u, n, tie, A = d.copy(), np.zeros_like(d), np.zeros(len(d), bool), np.abs(d).sum(1)
        for g in np.unique(frame):
            if kinds[g] < 0:
                continue
            m = frame == g
            h = H[g] if kinds[g] == 1 else np.diag(np.diag(H[g]))
            u[m], n[m], tie[m], A[m] = min_image(d[m], h, exact)
        return u, n, tie, A, frame
    return disp


# ---- the reference ------------------------------------------------------------------------------------------------------

def _terms(pos, src, dst, dd, scale, disp, len32=False):
    """len32: the length as the correctly rounded float32 root of the (exact) squared length, which is what pg_term divides by
    in the grid family; the float64 root otherwise"""
    u, n, _, A, frame = disp(pos, src, dst)
    g = np.asarray(dd, F32).astype(np.float64)
    ln = np.sqrt((u * u).sum(1).astype(F32)).astype(np.float64) if len32 else np.sqrt((u * u).sum(1))
    keep = (g != 0) & (ln > 0)
    return u[keep], n[keep], A[keep], frame[keep], g[keep] * float(F32(scale)), ln[keep], keep


def ref_positions_grad(pos, src, dst, dd, scale, disp, exact=False):
    """the float64 dpos [N, 3] over the edges (src -> dst) with weights dd; beside it mag [N, 3] (the same sums over absolute
    values), terms [N] (the term count of every row: out-going and incoming) and bound [N, 3]"""
    N = np.asarray(pos).shape[0]
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    u, _, A, _, gs, ln, keep = _terms(pos, src, dst, dd, scale, disp, len32=exact)
    s, t = src[keep], dst[keep]
    w = (gs / ln)[:, None] * -u                        # f * (r_i - r_j)
    dpos, mag, dw = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N)
    terms = np.zeros(N, np.int64)
    np.add.at(dpos, s, w)
    np.subtract.at(dpos, t, w)
    for idx in (s, t):
        np.add.at(mag, idx, np.abs(w))
        np.add.at(terms, idx, 1)
        np.add.at(dw, idx, np.abs(gs) * 2.0 * C_DISP * A / ln)
    bound = U24 * ((terms + C_PG)[:, None] * mag + (0.0 if exact else dw[:, None]))
    return SimpleNamespace(dpos=dpos, mag=mag, terms=terms, bound=bound)


def ref_box_grad(pos, src, dst, dd, scale, disp, G, exact=False):
    """per frame S [G, 3, 3], B [G, 3, 3] (summed in extended precision, rounded once), magS / magB, terms [G], boundS / boundB"""
    LD = np.longdouble
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    u, n, A, frame, gs, ln, _ = _terms(pos, src, dst, dd, scale, disp)
    ul = u.astype(LD)
    p = (gs.astype(LD) / np.sqrt((ul * ul).sum(1)))[:, None] * ul
    S, B = np.zeros((G, 3, 3), LD), np.zeros((G, 3, 3), LD)
    magS, magB, dS, dB = (np.zeros((G, 3, 3)) for _ in range(4))
    terms = np.zeros(G, np.int64)
    tS, tB = ul[:, :, None] * p[:, None, :], n.astype(LD)[:, :, None] * p[:, None, :]
    np.add.at(S, frame, tS)
    np.add.at(B, frame, tB)
    np.add.at(magS, frame, np.abs(tS).astype(np.float64))
    np.add.at(magB, frame, np.abs(tB).astype(np.float64))
    np.add.at(terms, frame, 1)
    if not exact:
        e = np.abs(gs) * C_DISP * A
        np.add.at(dS, frame, np.broadcast_to((3.0 * e)[:, None, None], tS.shape))
        np.add.at(dB, frame, np.broadcast_to((np.abs(n) * (2.0 * e / ln)[:, None])[:, :, None], tB.shape))
    k = (terms + C_BOX)[:, None, None] * U53
    return SimpleNamespace(S=S.astype(np.float64), B=B.astype(np.float64), magS=magS, magB=magB, terms=terms,
                           boundS=k * magS + U24 * dS, boundB=k * magB + U24 * dB)


def frame_paths(gp, N):
    """what box_grad.hip does with every frame, from graph_ptr alone: 'empty' (zeros from the frame pass), 'inside' (strictly
    inside one 256-row chunk: written by the chunk pass), or ('partial', number of chunks) (summed by the frame pass)"""
    out = []
    for lo, hi in zip(gp[:-1], gp[1:]):
        lo, hi = int(lo), int(hi)
        if hi <= lo:
            out.append("empty")
            continue
        cf, cl = lo // BG_ROWS, (hi - 1) // BG_ROWS
        end = min(N, (cl + 1) * BG_ROWS)
        out.append("inside" if cf == cl and lo > cf * BG_ROWS and hi < end else ("partial", cl - cf + 1))
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------

GRID_BOXES = [((16, 16, 16), (40, -24, 56)), ((32, 16, 16), (-56, 104, 16)), ((16, 32, 8), (24, 8, -96)),
              ((8, 8, 16), (-32, 16, 24)), ((32, 32, 32), (120, -96, 72))]        # diag (A), (b_x, c_x, c_y) in eighths
THIN_BOX = ((32, 32, 8), (0, 24, 120))    # 2 c - b = (6, -2, 16) is shorter than c = (3, 15, 8): the search needs k = 2
FLOAT_TRIC = np.array([[20.0, 0, 0], [6.5, 18.0, 0], [-7.2, 5.1, 16.0]])
FLOAT_ORTHO = np.array([17.3, 21.1, 19.7])


def _frame_positions(family, n, kind, seed, f, boxes):
    """(pos [n, 3] float32, box [9] float32, q8 or None, box8 or None)"""
    rng = np.random.default_rng([seed, f, n, kind + 1])
    if family == "grid":
        if kind < 0:
            q8 = NL.family("spread", max(n, 1), seed + f)[:n]
            NL.check_exact_domain(q8)
            return NL.positions_f32(q8), np.zeros(9, F32), q8, None
        diag, off = boxes[f % len(boxes)] if boxes else GRID_BOXES[(f + seed) % len(GRID_BOXES)]
        q8, box8 = NL.periodic_family(max(n, 1), seed + f, diag, off if kind == 1 else (0, 0, 0))
        q8 = q8[:n]
        NL.check_exact_domain(q8, box8)
        return NL.positions_f32(q8), NL.box_f32(box8), q8, box8
    side = (max(n, 2) / 0.1) ** (1 / 3)
    if kind < 0:
        return (rng.random((n, 3)) * side).astype(F32), np.zeros(9, F32), None, None
    s = (0.9, 1.0, 1.15, 1.3, 0.8)[f % 5]
    v = (FLOAT_TRIC if kind == 1 else np.diag(FLOAT_ORTHO)) * s
    v = v.astype(F32).astype(np.float64)
    fr = rng.random((n, 3))
    shift = rng.integers(-3, 4, (n, 3)) * (rng.random((n, 1)) < 0.3)
    return ((fr + shift) @ v).astype(F32), v.astype(F32).reshape(9), None, None


def make_case(family, form, sizes, kinds, seed, K=5, boxes=None, coincident=False, p_live=0.8):
    """One batch of len(sizes) frames (kinds per frame) in the padded (K slots per atom) or CSR form, with its incoming lists
    in two orders, the plants and the live edge list the reference takes.  See the module docstring."""
    assert family in ("grid", "float") and form in ("padded", "csr")
    exact = family == "grid"
    scale = GRID_SCALE if exact else FLOAT_SCALE
    rng = np.random.default_rng([seed, len(sizes), K, int(exact), int(form == "csr")])
    sizes = [int(s) for s in sizes]
    G, N = len(sizes), int(sum(sizes))
    gp = np.zeros(G + 1, np.int64)
    gp[1:] = np.cumsum(sizes)
    parts = [_frame_positions(family, n, int(k), seed, f, boxes) for f, (n, k) in enumerate(zip(sizes, kinds))]
    pos = np.concatenate([p[0] for p in parts]).astype(F32).reshape(N, 3)
    box = np.stack([p[1] for p in parts]).astype(F32).reshape(G, 9)
    # targets: random within the frame, never the row itself where the frame has another atom
    T = np.zeros((N, K), np.int64)
    for f, n in enumerate(sizes):
        if n:
            i = np.arange(n)[:, None]
            T[gp[f]:gp[f + 1]] = gp[f] + (i + 1 + rng.integers(0, max(n - 1, 1), (n, K))) % n      # n == 1: itself
    live = rng.random((N, K)) < p_live
    plants = {}
    big = int(np.argmax(sizes)) if G else 0
    if G and sizes[big] >= MIN_PLANT:
        b0, n = int(gp[big]), sizes[big]
        hub, orphan, alldead, dup, ca, cb = (b0 + x for x in rng.choice(n, 6, replace=False))
        rows = np.arange(b0, b0 + n)
        T[rows[rows != hub], 0] = hub
        live[rows[rows != hub], 0] = True
        if K >= 3:
            T[dup, 1] = T[dup, K - 1] = [x for x in rows if x not in (dup, orphan, hub)][0]
            live[dup, 1] = live[dup, K - 1] = True
            plants["dup"] = int(dup)
        if K >= 2:
            if coincident:
                h = box[big].astype(np.float64).reshape(3, 3)
                pos[cb] = pos[ca] + ((h[0] - h[2]).astype(F32) if exact and kinds[big] >= 0 else 0)
                T[ca, 1], T[cb, 1] = cb, ca
                live[ca, 1] = live[cb, 1] = True
                plants["coincident"] = (int(ca), int(cb))
        back = T == orphan
        T[back] = np.where(np.arange(N)[:, None] == hub, dup, hub)[np.nonzero(back)[0], 0]
        live[alldead] = False
        plants.update(hub=int(hub), orphan=int(orphan), alldead=int(alldead))
    disp = make_disp(gp, kinds, box, exact)
    row = np.repeat(np.arange(N), K).reshape(N, K)
    u, _, tie, _, _ = disp(pos, row.reshape(-1), T.reshape(-1))
    ln = np.sqrt((u * u).sum(1)).reshape(N, K)
    zero = ln == 0
    tie = tie.reshape(N, K) & ~zero
    n_pairs = int(live.sum())
    tie_share = float((live & tie).sum()) / max(n_pairs, 1)
    live &= ~tie
    if form == "padded" or not coincident:
        live &= ~zero                                  # a padded slot of length zero is dead (edges = 0)
    else:
        pair = np.zeros((N, K), bool)
        pair[list(plants["coincident"]), 1] = True
        live &= ~zero | pair                           # CSR: only the planted pair stays
    # weights
    if exact:
        len32 = np.sqrt(((u * u).sum(1)).astype(F32)).reshape(N, K)      # the squared length is a float32 number
        dd = (len32 * (2.0 ** rng.choice(GRID_K, (N, K))).astype(F32) * rng.choice([-1, 1], (N, K)).astype(F32)).astype(F32)
        dd[zero] = F32(2.0)
    else:
        dd = rng.standard_normal((N, K)).astype(F32)
        dd[dd == 0] = F32(1.0)
    cand = np.argwhere(live & ~zero & (np.arange(K)[None, :] > 0))
    if len(cand) >= 2:
        (r0, k0), (r1, k1) = cand[rng.choice(len(cand), 2, replace=False)]
        dd[r0, k0], dd[r1, k1] = F32(0.0), F32(-0.0)
        plants["zero_dd"] = 2
    c = SimpleNamespace(family=family, form=form, exact=exact, scale=scale, N=N, G=G, K=K, gp=gp.astype(np.int32),
                        sizes=sizes, kinds=np.asarray(kinds, np.int32).reshape(G), box=box, pos=pos, plants=plants,
                        tie_share=tie_share, n_pairs=n_pairs, disp=disp)
    lf = live.reshape(-1)
    c.src, c.dst, c.g = row.reshape(-1)[lf], T.reshape(-1)[lf], dd.reshape(-1)[lf]
    if form == "padded":
        dead = np.nonzero(~lf)[0]
        edges = (ln * scale).astype(F32).reshape(-1)
        edges[dead] = np.array(DEAD_EDGES, F32)[np.arange(len(dead)) % 4]
        ddf = dd.reshape(-1).copy()
        ddf[dead] = np.array(DEAD_DD, F32)[np.arange(len(dead)) % 2]
        nl = np.where(live, T, row)
        c.nlist, c.edges, c.dd = nl.astype(np.int32), edges.reshape(N, K), ddf.reshape(N, K)
        c.n_entries = N * K
        ptr, eid, _ = GL.incoming_lists(c.nlist.reshape(-1), c.edges.reshape(-1), N, K)
    else:
        deg = live.sum(1)
        c.row_ptr = NL.scan(deg)
        c.col = c.dst.astype(np.int32)
        c.row_of = c.src.astype(np.int32)
        c.dd = c.g.copy()
        c.n_entries = int(deg.sum())
        ptr, eid, _ = GL.incoming_lists(c.col, None, N, 0)
    c.csc_ptr, c.csc_edge = ptr.astype(np.int32), eid.astype(np.int32)
    sh = c.csc_edge.copy()
    for a, b in zip(ptr[:-1], ptr[1:]):
        sh[a:b] = rng.permutation(sh[a:b])
    c.csc_edge_shuffled = sh
    return c


def check_grid_exact(c, ref):
    """the grid family's exactness conditions on a built case: inputs on the 1/8 grid with power-of-two diagonals
    (nlist_ref.check_exact_domain, called per frame by the builder), every displacement a multiple of 1/8 with a squared length
    below 2^24 / 64, g * scale / len32 a signed power of two, and every row's sum of magnitudes below 2^24 quanta"""
    assert c.exact and float(F32(c.scale)) == 2.0 ** round(np.log2(c.scale))
    u, _, tie, _, _ = c.disp(c.pos, c.src, c.dst)
    assert not tie.any()
    assert (u * 8.0 == np.rint(u * 8.0)).all()
    d2 = (u * u).sum(1) * 64.0
    assert (d2 < NL.EXACT).all()
    ln32 = np.sqrt((d2 / 64.0).astype(F32))
    nz = (c.g != 0) & (d2 > 0)
    q = (c.g[nz].astype(np.float64) / ln32[nz].astype(np.float64))
    assert (np.abs(q) == 2.0 ** np.rint(np.log2(np.abs(q)))).all()
    quantum = 2.0 ** min(GRID_K) * c.scale / 8.0
    assert (ref.mag / quantum < NL.EXACT).all()
    assert (ref.dpos.astype(F32).astype(np.float64) == ref.dpos).all()
    return True


# ---- a float32 emulation of the kernels' expressions -----------------------------------------------------------------------

def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _dist2(x, y, z):
    return _fma(z, z, _fma(y, y, x * x))


def _emulate_disp(q, p, kind, b):
    """float32 DispOpen / DispOrtho / DispTric of csrc/pbc.cuh on rows q, p [E, 3] float32 -> u [E, 3] float32"""
    d = (p - q).astype(F32)
    if kind < 0:
        return d
    one = F32(1.0)
    x, y, z = d[:, 0].copy(), d[:, 1].copy(), d[:, 2].copy()
    if kind == 0:
        for v, L in ((x, b[0]), (y, b[4]), (z, b[8])):
            v[:] = _fma(-L, np.rint(v * (one / L)), v)
        return np.stack([x, y, z], 1)
    ax, bx, by, cx, cy, cz = b[0], b[3], b[4], b[6], b[7], b[8]
    s = np.rint(z * (one / cz))
    x, y, z = _fma(-s, cx, x), _fma(-s, cy, y), _fma(-s, cz, z)
    s = np.rint(y * (one / by))
    x, y = _fma(-s, bx, x), _fma(-s, by, y)
    s = np.rint(x * (one / ax))
    x = _fma(-s, ax, x)
    v = ax * by * cz
    bcx, bcy, bcz = by * cz, -bx * cz, bx * cy - by * cx
    wa = v / np.sqrt(bcx * bcx + bcy * bcy + bcz * bcz)
    wb = by * cz / np.sqrt(cy * cy + cz * cz)
    w = min(wa, wb, cz)
    h2 = F32(0.25) * w * w
    ni, nj, nk = kernel_reach(b.astype(np.float64).reshape(3, 3))
    best = _dist2(x, y, z)
    far = best >= h2
    o = (x.copy(), y.copy(), z.copy())
    for k, j, i in itertools.product(range(-nk, nk + 1), range(-nj, nj + 1), range(-ni, ni + 1)):
        ex = _fma(F32(k), cx, _fma(F32(j), bx, _fma(F32(i), ax, o[0])))
        ey = _fma(F32(k), cy, _fma(F32(j), by, o[1]))
        ez = _fma(F32(k), cz, o[2])
        e2 = _dist2(ex, ey, ez)
        take = far & (e2 < best)
        best = np.where(take, e2, best)
        x, y, z = np.where(take, ex, x), np.where(take, ey, y), np.where(take, ez, z)
    return np.stack([x, y, z], 1).astype(F32)


def emulate(c, drop_incoming=False, flip_incoming=False, next_box=False):
    """dpos [N, 3] float32, S, B [G, 3, 3] float64 as the kernels' expressions give them on case c, in NumPy; the three
    switches are the deliberately wrong results of the host test"""
    box = np.roll(c.box, -1, axis=0) if next_box else c.box
    kinds = np.roll(c.kinds, -1) if next_box else c.kinds
    frame = np.searchsorted(c.gp.astype(np.int64), c.src, side="right") - 1
    u = np.zeros((len(c.src), 3), F32)
    for g in np.unique(frame):
        m = frame == g
        u[m] = _emulate_disp(c.pos[c.src[m]], c.pos[c.dst[m]], int(kinds[g]), box[g])
    v = -u
    ln = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(ln > 0, c.g * F32(c.scale) / ln, F32(0.0)).astype(F32)
    f[c.g == 0] = 0
    w = (f[:, None] * v).astype(F32)
    dpos = np.zeros((c.N, 3), F32)
    np.add.at(dpos, c.src, w)
    inc = np.ones(len(c.src), bool)
    if drop_incoming:
        inc[np.nonzero((c.g != 0) & (ln > 0))[0][-1]] = False
    if flip_incoming:
        np.add.at(dpos, c.dst[inc], w[inc])
    else:
        np.subtract.at(dpos, c.dst[inc], w[inc])
    x = u.astype(np.float64)
    l64 = np.sqrt((x * x).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        w64 = np.where((l64 > 0) & (c.g != 0), c.g.astype(np.float64) * float(F32(c.scale)) / l64, 0.0)
    p = w64[:, None] * x
    n = np.zeros_like(x)
    H = box.astype(np.float64).reshape(-1, 3, 3)
    delta = x - (c.pos[c.dst].astype(np.float64) - c.pos[c.src].astype(np.float64))
    for g in np.unique(frame):
        if kinds[g] < 0:
            continue
        m = frame == g
        h = H[g] if kinds[g] == 1 else np.diag(np.diag(H[g]))
        dl = delta[m].copy()
        for r in (2, 1, 0):
            n[m, r] = np.rint(dl[:, r] / h[r, r])
            dl -= n[m, r][:, None] * h[r]
    S, B = np.zeros((c.G, 3, 3)), np.zeros((c.G, 3, 3))
    np.add.at(S, frame, x[:, :, None] * p[:, None, :])
    np.add.at(B, frame, n[:, :, None] * p[:, None, :])
    return dpos, S, B


def references(c):
    rp = ref_positions_grad(c.pos, c.src, c.dst, c.g, c.scale, c.disp, c.exact)
    rb = ref_box_grad(c.pos, c.src, c.dst, c.g, c.scale, c.disp, c.G, c.exact)
    return rp, rb


def ratios(c, dpos, S, B, rp, rb):
    """largest |got - ref| / bound of dpos, S, B (0 / 0 counts as 0; anything over a zero bound as inf)"""
    out = []
    for got, r, names in ((dpos, rp, ("dpos", "bound")), (S, rb, ("S", "boundS")), (B, rb, ("B", "boundB"))):
        if got is None:
            out.append(0.0)
            continue
        ref, bound = getattr(r, names[0]), getattr(r, names[1])
        err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
        err = np.where(np.isfinite(err), err, np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        out.append(float(r.max(initial=0.0)))
    return out


# ---- the cases of the two test files --------------------------------------------------------------------------------------

OPEN_SHAPES = [(1, 1), (2, 1), (255, 5), (256, 16), (257, 5), (700, 16)]                     # (N, K)
UNIFORM_SHAPES = [(1, 1), (1, 85), (3, 85), (5, 257), (3, 1)]                                # (G, n)
RAGGED_SIZES = [1, 2, 17, 0, 255, 256, 300]
RAGGED_KINDS = [0, -1, 1, 1, 0, -1, 1]
BOX_PATTERNS = {
    "small40": [1 + (7 * i) % 12 for i in range(40)],       # 256 rows: the first and the last frame in partials, 38 inside
    "f256": [256],
    "f257": [257],
    "f700": [700],
    "boundary": [100, 156, 50],
    "empties": [0, 30, 0, 0, 300, 40, 0, 10, 0],
    "one100": [100],
}
KIND_OF = {"open": -1, "ortho": 0, "tric": 1}


def pattern_kinds(policy, G):
    """the kinds of a box-gradient case: one for the whole batch, or mixed per frame ('per')"""
    return [(1, 0, -1)[g % 3] for g in range(G)] if policy == "per" else [KIND_OF[policy]] * G
