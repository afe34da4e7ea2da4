"""Plain NumPy statements of the small node-side kernels of csrc/node_ops.hip: the counter RNG (csrc/rng.cuh: Philox4x32-10, u01,
Box-Muller, the keep-mask), the Adam update and the AMP attention aggregation with its backward.  No GPU is needed to import or
run this; tests/test_node_small_ref_host.py checks it on the CPU and tests/test_gpu_node_small.py holds the kernels to it.

Integers are uint64 arrays holding 32-bit words (a product of two words fits), floats are float64 unless a function says
float32.  Every float64 reference also returns the same expression on absolute values ("mag"), the scale its bound is stated on."""
import numpy as np

U24 = 2.0 ** -24                                  # one float32 rounding, relative
MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
TWO_PI32 = np.float32(6.28318530717958648)
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))        # the largest radius: u = 2^-24, sqrt(-2 ln 2^-24)
# ng_randn's bound, |z - z_ref| <= C_RANDN 2^-24 max(r_ref, 2^-24): C_HOST is the largest such ratio of randn_f32 (NumPy's
# float32 log, sqrt, cos, sin) over 2^20 draws of seed 20231, measured 3.160 (test_node_small_ref_host.py measures it again);
# the device's logf / sinf / cosf are allowed about two ulp where the host gives under one and fused multiply-adds move a
# rounding, hence the factor 4 (floor 8)
C_HOST = 3.16
C_RANDN = max(8.0, 4.0 * C_HOST)


def f32(a):
    """round to float32, keep as float64"""
    return np.asarray(a, np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------- counter RNG
def _words(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(ctr128, key64):
    """Philox4x32-10 (Salmon et al. 2011): ctr128 = four 32-bit words (word 0 first), key64 = two.  Python ints or uint64
    arrays of one shape; returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (_words(c) for c in ctr128)
    k0, k1 = (_words(k) for k in key64)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> _S32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + _W0) & MASK32, (k1 + _W1) & MASK32
    return c0, c1, c2, c3


def draw_words(seed, offset, n):
    """the n 32-bit words the kernels draw: counter (lo32(offset + q), hi32(offset + q), 0, 0), key (lo32(seed), hi32(seed)),
    element 4 q + k takes word k"""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    n4 = (int(n) + 3) // 4
    ctr = np.uint64(offset) + np.arange(n4, dtype=np.uint64)          # wraps at 2^64 like the kernel's sum
    zero = np.zeros(n4, np.uint64)
    w = philox4x32_10((ctr & MASK32, ctr >> _S32, zero, zero), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:n]


def u01(x):
    """((x >> 8) + 1) 2^-24 in (0, 1]: 24 bits, exact in float32"""
    return ((_words(x) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * U24


def dropout_ref(seed, offset, keep, n):
    """the keep-mask in float32, comparable bit for bit: 1 / keep where u01 <= keep, else 0"""
    keep = np.float32(keep)
    u = u01(draw_words(seed, offset, n)).astype(np.float32)
    return np.where(u <= keep, np.float32(1) / keep, np.float32(0)).astype(np.float32)


def _pairs(seed, offset, n):
    """(u, t) per element as float32: the radius uniform and the angle float32(2 pi) * uniform of the element's pair;
    first[k]: the element takes the cosine"""
    n4 = (int(n) + 3) // 4
    u = u01(draw_words(seed, offset, 4 * n4)).astype(np.float32).reshape(n4, 2, 2)
    ur = np.repeat(u[:, :, 0], 2, axis=1).reshape(-1)
    t = np.repeat(TWO_PI32 * u[:, :, 1], 2, axis=1).reshape(-1)       # float32 product, rounded once
    first = np.tile(np.array([True, False]), 2 * n4)
    return ur, t, first


def randn_ref(seed, offset, n):
    """Box-Muller in float64 from the float32 uniforms and angles the kernel forms: z = (r0 cos t0, r0 sin t0, r1 cos t1,
    r1 sin t1), r = sqrt(-2 ln u), words (0, 1) for pair 0 and (2, 3) for pair 1.  Returns (z, r), one entry per element."""
    ur, t, first = _pairs(seed, offset, n)
    r = np.sqrt(-2.0 * np.log(ur.astype(np.float64)))
    t = t.astype(np.float64)
    z = r * np.where(first, np.cos(t), np.sin(t))
    return z[:n], r[:n]


def randn_f32(seed, offset, n):
    """the same draw with NumPy's float32 log, sqrt, cos and sin: what a float32 evaluation gives on the host (it sets the
    scale of the GPU bound, nothing is compared with it)"""
    ur, t, first = _pairs(seed, offset, n)
    r = np.sqrt(np.float32(-2) * np.log(ur))
    z = r * np.where(first, np.cos(t), np.sin(t))
    assert z.dtype == np.float32
    return z[:n]


def randn_ratio(z, z_ref, r_ref):
    """|z - z_ref| in units of 2^-24 max(r_ref, 2^-24), per element"""
    return np.abs(np.asarray(z, np.float64) - z_ref) / (U24 * np.maximum(r_ref, U24))


# ------------------------------------------------------------------------------------------------- Adam
def adam_constants(lr, b1, b2, step):
    """(lr_t, 1 - b1, 1 - b2) as the entry point and the kernel form them from float32 arguments"""
    lr, b1, b2 = (float(np.float32(x)) for x in (lr, b1, b2))
    lr_t = float(np.float32(lr * np.sqrt(1.0 - b2 ** float(step)) / (1.0 - b1 ** float(step))))
    return lr_t, float(np.float32(1) - np.float32(b1)), float(np.float32(1) - np.float32(b2))


def adam_ref(p, g, m, v, lr, b1, b2, eps, step, gscale):
    """Keras Adam in float64 on float32 inputs, with the float32 constants of adam_constants.  Returns (p, m, v) and the
    magnitudes dict(m1, m2: the two terms of m on absolute values; v1, v2: those of v; upd: lr_t (m1 + m2) / (sqrt(v) + eps))."""
    p, g, m, v = (np.asarray(x, np.float32).astype(np.float64) for x in (p, g, m, v))
    lr_t, omb1, omb2 = adam_constants(lr, b1, b2, step)
    b1, b2, eps, gscale = (float(np.float32(x)) for x in (b1, b2, eps, gscale))
    gi = g * gscale
    m1, m2 = b1 * m, omb1 * gi
    v1, v2 = b2 * v, omb2 * gi * gi
    mi, vi = m1 + m2, v1 + v2
    den = np.sqrt(vi) + eps
    with np.errstate(invalid="ignore", divide="ignore"):
        pn = p - lr_t * mi / den
        upd = lr_t * (np.abs(m1) + np.abs(m2)) / den
    return pn, mi, vi, dict(m1=np.abs(m1), m2=np.abs(m2), v1=np.abs(v1), v2=np.abs(v2), upd=upd)


# ------------------------------------------------------------------------------------------------- AMP attention
def incoming_lists(nlist, N):
    """(in_ptr [N + 1], in_slot [N K]) int32: the flat slots i K + j sorted by their target, stably"""
    tgt = np.asarray(nlist).reshape(-1).astype(np.int64)
    in_slot = np.argsort(tgt, kind="stable").astype(np.int32)
    in_ptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=N))]).astype(np.int32)
    return in_ptr, in_slot


def _amp_fwd(h, nlist, e, inv, wq, wk):
    h, e, inv, wq, wk = (np.asarray(x, np.float64) for x in (h, e, inv, wq, wk))
    nl = np.asarray(nlist).astype(np.int64)
    q = h @ wq                                             # [N, E]
    u = q @ wk.T                                           # u[n] = sum_k wk[n, k] q[k]
    s = inv[:, None] * np.einsum("ijn,in->ij", e, u)
    mq = np.abs(h) @ np.abs(wq)
    mu = mq @ np.abs(wk).T
    L = (np.abs(inv)[:, None] * np.einsum("ijn,in->ij", np.abs(e), mu)).max(axis=1)       # [N]
    b = np.exp(s - s.max(axis=1, keepdims=True))
    b /= b.sum(axis=1, keepdims=True)
    return h, nl, e, inv, wq, wk, q, u, mq, mu, L, b


def amp_ref(h, nlist, e, inv, wq, wk):
    """q_i = h_i wq, u = wk q, s_j = inv_i <e_ij, u>, b = softmax_j(s), agg_i = sum_j b_j h[nl_ij].  Returns (agg, b) and
    dict(agg: sum_j b_j |h[nl_ij]|, L: per row, the largest logit on absolute values)."""
    h, nl, e, inv, wq, wk, q, u, mq, mu, L, b = _amp_fwd(h, nlist, e, inv, wq, wk)
    agg = np.einsum("ij,ijl->il", b, h[nl])
    return agg, b, dict(agg=np.einsum("ij,ijl->il", b, np.abs(h)[nl]), L=L)


def amp_bwd_ref(h, nlist, e, inv, wq, wk, dagg):
    """the formulas above amp_attend_bwd_atom_kernel in float64:
        db_j = <dA, h[nl_ij]>, ds_j = b_j (db_j - sum_k b_k db_k), de_ij = inv_i ds_j u, du = inv_i sum_j ds_j e_ij,
        dq = wk^T du, dwk = sum_i du q^T, dwq = sum_i h_i dq^T, dh_t = sum_{(i,j): nl_ij = t} b_ij dA_i + dq_t wq^T.
    Returns dict(dh, de, dwq, dwk), the same on absolute values, and L (per row)."""
    h, nl, e, inv, wq, wk, q, u, mq, mu, L, b = _amp_fwd(h, nlist, e, inv, wq, wk)
    dA = np.asarray(dagg, np.float64)
    N, F = h.shape

    def chain(h_, e_, inv_, wq_, wk_, dA_, q_, u_, minus):
        db = np.einsum("il,ijl->ij", dA_, h_[nl])
        ds = b * (db + minus * np.sum(b * db, axis=1, keepdims=True))
        de = inv_[:, None, None] * ds[:, :, None] * u_[:, None, :]
        du = inv_[:, None] * np.einsum("ij,ijn->in", ds, e_)
        dq = du @ wk_                                      # dq[k] = sum_n wk[n, k] du[n]
        dwk = du.T @ q_
        dwq = h_.T @ dq
        dh = np.zeros((N, F))
        np.add.at(dh, nl.reshape(-1), (b[:, :, None] * dA_[:, None, :]).reshape(-1, F))
        dh += dq @ wq_.T
        return dict(dh=dh, de=de, dwq=dwq, dwk=dwk)

    ref = chain(h, e, inv, wq, wk, dA, q, u, -1.0)
    mag = chain(np.abs(h), np.abs(e), np.abs(inv), np.abs(wq), np.abs(wk), np.abs(dA), mq, mu, 1.0)
    return ref, mag, L


def row_logit_scale(nlist, L):
    """the L each output's bound takes: agg and de rows their own, a dh row the largest over itself and the rows that name it,
    the weight gradients the largest of all"""
    nl = np.asarray(nlist).astype(np.int64)
    Ldh = L.copy()
    np.maximum.at(Ldh, nl.reshape(-1), np.repeat(L, nl.shape[1]))
    return dict(agg=L[:, None], de=L[:, None, None], dh=Ldh[:, None], dwq=L.max(initial=0.0), dwk=L.max(initial=0.0))


# graph patterns of the attention tests
def amp_nlist(rng, N, K, pattern):
    if pattern == "hub":                                   # every slot names atom 0: all other incoming lists are empty
        return np.zeros((N, K), np.int32)
    if pattern == "self":
        return np.repeat(np.arange(N, dtype=np.int32)[:, None], K, axis=1)
    nl = rng.integers(0, N, (N, K)).astype(np.int32)
    if pattern == "dup":                                   # one row with the same target in all K slots
        nl[N // 2, :] = nl[N // 2, 0]
    return nl


def amp_exact_data(rng, N, K, F, E, nlist, setting):
    """small integers, inv in {1/2, 1}; "wq0": wq = 0 with integer wk, "wk0": wk = 0 with integer wq.  All logits are exactly
    0 in both, so b = 1 / K (K a power of two) and every output is a multiple of min(inv) / K^2."""
    lim = 1 if F * E > 2048 or N > 500 else 2
    d = dict(h=rng.integers(-lim, lim + 1, (N, F)).astype(np.float64), nlist=nlist,
             e=rng.integers(-lim, lim + 1, (N, K, E)).astype(np.float64), inv=rng.choice([0.5, 1.0], N),
             wq=rng.integers(-lim, lim + 1, (F, E)).astype(np.float64), wk=rng.integers(-lim, lim + 1, (E, E)).astype(np.float64),
             dagg=rng.integers(-lim, lim + 1, (N, F)).astype(np.float64))
    d["wq" if setting == "wq0" else "wk"][...] = 0.0
    return d


def amp_exact_in_range(d, K):
    """for every sum the kernels form on exact-family data, the sum of the absolute values of its terms in units of the
    terms' grid (1 for q, u, db; 1 / K for the softmax-weighted sums; min(inv) / K^2 = 1 / (2 K^2) for everything behind ds).
    Each stage takes the exact values of the stage before, so with all of these below 2^24 every partial sum in any order
    is exact in float32, stage by stage."""
    h, nl, e, inv, wq, wk, q, u, mq, mu, L, b = _amp_fwd(d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"])
    assert not L.any() and (b == 1.0 / K).all(), "exact family: a logit is not zero"
    dA, a = d["dagg"], np.abs
    u2 = 0.5 / K ** 2
    db = np.einsum("il,ijl->ij", dA, h[nl])
    t = db.mean(axis=1, keepdims=True)
    ds = (db - t) / K
    du = inv[:, None] * np.einsum("ij,ijn->in", ds, e)
    dq = du @ wk
    scat = np.zeros_like(h)
    np.add.at(scat, nl.reshape(-1), np.repeat(a(dA), K, axis=0) / K)
    return {"q": mq.max(), "u": (a(q) @ a(wk).T).max(), "db": np.einsum("il,ijl->ij", a(dA), a(h)[nl]).max(),
            "agg": a(h)[nl].sum(axis=1).max(), "t": a(db).sum(axis=1).max(), "ds": ((a(db) + a(t)) * K).max(),
            "du": np.einsum("ij,ijn->in", a(ds), a(e)).max() * K ** 2, "dq": (a(du) @ a(wk)).max() / u2,
            "dwq": (a(h).T @ a(dq)).max() / u2, "dwk": (a(du).T @ a(q)).max() / u2,
            "dh": (a(dq) @ a(wq).T + scat).max() / u2}


def amp_widen(d, span):
    """scale wq and wk by one factor so that the largest |logit| becomes about `span` (the softmax saturates)"""
    h, nl, e, inv, wq, wk, q, u, mq, mu, L, b = _amp_fwd(d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"])
    top = np.abs(inv[:, None] * np.einsum("ijn,in->ij", e, u)).max()
    k = np.sqrt(span / top)
    return dict(d, wq=f32(k * d["wq"]), wk=f32(k * d["wk"]))


# (N, K, E, F, pattern): every value of N in {1, 3, 4, 5, 257, 769}, K in {1, 2, 7, 16, 63, 64} (and 4 for the exact family),
# E in {1, 3, 8, 63, 64}, F in {1, 16, 63, 64, 65, 100, 256}; E > K, E < K, every graph pattern
AMP_CASES = [(1, 1, 64, 1, "self"), (5, 64, 64, 65, "random"), (3, 2, 1, 16, "random"), (4, 7, 3, 63, "random"),
             (5, 16, 8, 64, "dup"), (257, 16, 8, 64, "random"), (769, 16, 3, 100, "random"), (257, 63, 63, 16, "hub"),
             (4, 64, 8, 256, "random"), (5, 1, 64, 100, "random"), (769, 2, 8, 16, "hub"), (257, 7, 1, 65, "self"),
             (3, 63, 64, 1, "random"), (5, 64, 1, 63, "hub"), (4, 16, 63, 256, "self"), (257, 2, 64, 64, "dup"),
             (1, 16, 8, 64, "self"), (769, 64, 3, 16, "dup"), (5, 4, 8, 64, "random"), (257, 4, 3, 65, "hub"),
             (3, 1, 1, 1, "random")]
AMP_EXACT_CASES = [c for c in AMP_CASES if c[1] in (1, 2, 4, 16, 64)]
AMP_WIDE_CASES = [(4, 7, 3, 63, "random"), (5, 16, 8, 64, "dup"), (257, 16, 8, 64, "random"), (5, 64, 64, 65, "random")]


def amp_id(c):
    return "N%d-K%d-E%d-F%d-%s" % c


def amp_rng(c, tag):
    return np.random.default_rng([*c[:4], ["random", "hub", "self", "dup"].index(c[4]), tag])


def amp_normal_data(rng, N, K, F, E, nlist, scale=1.0, zero_inv_row=True):
    """random normal float32 data, inv = 1 / degree; scale multiplies wq and wk (row logits then span about scale^2 * 3)"""
    d = dict(h=f32(rng.standard_normal((N, F))), nlist=nlist, e=f32(rng.standard_normal((N, K, E))),
             inv=f32(1.0 / rng.integers(1, K + 1, N)), wq=f32(scale * rng.standard_normal((F, E)) / np.sqrt(F)),
             wk=f32(scale * rng.standard_normal((E, E)) / np.sqrt(E)), dagg=f32(rng.standard_normal((N, F))))
    if zero_inv_row:
        d["inv"][N // 3] = 0.0                             # uniform weights in that row
    return d
