"""tests/geom_grad_ref.py on the CPU: the reference against plain loops over edges and against the float64 formulation of
test_gpu_ragged_pbc.py, the grid family's exactness conditions, the caps on the share of image ties, a float32 emulation of
the kernels' expressions inside the bounds (and equal to the grid reference bit for bit), and three wrong results that both
families must reject."""
import math

import numpy as np
import pytest

import geom_grad_ref as R

F32 = np.float32
SMALL = [("padded", [12, 9, 0, 14], [0, 1, -1, 1], 4), ("csr", [40], [1], 5), ("csr", [10, 11, 12], [-1, 0, 1], 3),
         ("padded", [1, 2, 20], [1, 0, 0], 2)]


def _all_cases():
    """(name, builder) of every case of the GPU file: the tie caps and the exactness conditions hold on each"""
    out = []
    for fam in ("grid", "float"):
        for form in ("padded", "csr"):
            for N, K in R.OPEN_SHAPES:
                out.append((f"open-{fam}-{form}-{N}-{K}", lambda fam=fam, form=form, N=N, K=K: R.make_case(fam, form, [N], [-1], 1, K)))
            for kind in (0, 1):
                for G, n in R.UNIFORM_SHAPES:
                    out.append((f"uni-{fam}-{form}-{kind}-{G}x{n}",
                                lambda fam=fam, form=form, kind=kind, G=G, n=n: R.make_case(fam, form, [n] * G, [kind] * G, 2, 5)))
            if fam == "grid":
                out.append((f"thin-{fam}-{form}", lambda fam=fam, form=form: R.make_case("grid", form, [300], [1], 5, 5, boxes=[R.THIN_BOX])))
            out.append((f"ragged-{fam}-{form}", lambda fam=fam, form=form: R.make_case(fam, form, R.RAGGED_SIZES, R.RAGGED_KINDS, 3, 5)))
            for name, sizes in R.BOX_PATTERNS.items():
                for policy in ("open", "ortho", "tric", "per"):
                    out.append((f"box-{fam}-{form}-{name}-{policy}",
                                lambda fam=fam, form=form, sizes=sizes, policy=policy: R.make_case(
                                    fam, form, sizes, R.pattern_kinds(policy, len(sizes)), 4, 5)))
            for policy in ("open", "ortho", "tric", "per"):    # test_zero_weight_entries_are_skipped_whatever_their_geometry
                kinds = R.pattern_kinds(policy, 3) if policy == "per" else [R.KIND_OF[policy]] * 3
                out.append((f"zero-weight-{fam}-{form}-{policy}", lambda fam=fam, form=form, kinds=kinds: R.make_case(
                    fam, form, [85, 85, 85], kinds, 10, 5)))
            out.append((f"refusals-{fam}-{form}", lambda fam=fam, form=form: R.make_case(fam, form, [17, 17], [1, 1], 8, 5)))
        for policy in ("open", "ortho", "tric", "per"):        # the coincident pairs of test_zero_length_entries_contribute_nothing
            for sizes in ([40, 300, 17], [85, 85, 85]):
                kinds = R.pattern_kinds(policy, 3) if sizes[0] == 40 else [R.KIND_OF.get(policy, 1)] * 3
                out.append((f"zero-{fam}-{policy}-{sizes[0]}", lambda fam=fam, sizes=sizes, kinds=kinds: R.make_case(
                    fam, "csr", sizes, kinds, 6, 5, coincident=True)))
    return out


def _loop_reference(c):
    """plain Python over the edges: math.fsum of every row's and frame's terms"""
    u, n, _, _, frame = c.disp(c.pos, c.src, c.dst)
    rows = [[[] for _ in range(3)] for _ in range(c.N)]
    S = [[[[] for _ in range(3)] for _ in range(3)] for _ in range(c.G)]
    B = [[[[] for _ in range(3)] for _ in range(3)] for _ in range(c.G)]
    count = [0] * c.N
    for e in range(len(c.src)):
        g = float(c.g[e])
        ln = math.sqrt(sum(float(x) ** 2 for x in u[e]))
        if g == 0.0 or ln == 0.0:
            continue
        ln_p = float(np.sqrt(F32(ln * ln))) if c.exact else ln
        i, j = int(c.src[e]), int(c.dst[e])
        count[i] += 1
        count[j] += 1
        for a in range(3):
            t = g * float(F32(c.scale)) * float(u[e, a])
            rows[i][a].append(-t / ln_p)
            rows[j][a].append(t / ln_p)
            for b in range(3):
                S[frame[e]][a][b].append(float(u[e, a]) * g * float(F32(c.scale)) * float(u[e, b]) / ln)
                B[frame[e]][a][b].append(float(n[e, a]) * g * float(F32(c.scale)) * float(u[e, b]) / ln)
    f = lambda tree: np.array([[[math.fsum(x) for x in r] for r in m] for m in tree]).reshape(-1, 3, 3)
    dpos = np.array([[math.fsum(x) for x in r] for r in rows]).reshape(-1, 3)
    return dpos, f(S), f(B), np.array(count, np.int64)


@pytest.mark.parametrize("family", ["grid", "float"])
@pytest.mark.parametrize("form,sizes,kinds,K", SMALL)
def test_reference_against_plain_loops(family, form, sizes, kinds, K):
    c = R.make_case(family, form, sizes, kinds, 7, K, coincident=form == "csr")
    assert c.N <= 40
    rp, rb = R.references(c)
    dpos, S, B, count = _loop_reference(c)
    np.testing.assert_array_equal(rp.terms, count)
    tol = lambda m: 1e-14 * m + 1e-300
    assert (np.abs(rp.dpos - dpos) <= tol(rp.mag)).all()
    assert (np.abs(rb.S - S) <= tol(rb.magS)).all() and (np.abs(rb.B - B) <= tol(rb.magB)).all()
    assert np.isfinite(rp.dpos).all() and np.isfinite(rb.S).all() and np.isfinite(rb.B).all()
    if (np.asarray(kinds) >= 0).any():
        assert np.abs(rb.B).max() > 0
    for g, k in enumerate(kinds):
        if k < 0:
            assert (rb.B[g] == 0).all()
        np.testing.assert_allclose(rb.S[g], rb.S[g].T, rtol=0, atol=1e-12 * max(rb.magS[g].max(), 1e-300))


@pytest.mark.parametrize("kind", [-1, 0, 1])
def test_reference_against_the_fractional_formulation(kind):
    """one structure of the float family (no coincident pair, ties left out): the two statements of the minimum image agree to
    float64 rounding"""
    from test_gpu_ragged_pbc import _positions_grad64      # a plain NumPy function of that file; importing it starts no GPU work
    c = R.make_case("float", "csr", [300], [kind], 9, 5)
    rp, _ = R.references(c)
    vecs = None if kind < 0 else c.box[0].reshape(3, 3)
    if kind == 0:
        vecs = np.diag(np.diag(vecs))
    keep = c.g != 0
    other = _positions_grad64(c.pos, c.src[keep], c.dst[keep], c.g[keep], float(F32(c.scale)), vecs)
    assert (np.abs(other - rp.dpos) <= 1e-12 * rp.mag + 1e-300).all()


CASES = _all_cases()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_case_conditions_ties_and_emulation(name):
    """every case of the GPU file: tie share under its cap (10 % grid, 1 % float), the planted rows present, the grid family's
    exactness conditions, and the float32 emulation inside the bounds (bit for bit on the grid)"""
    c = dict(CASES)[name]()
    assert c.tie_share <= (0.10 if c.exact else 0.01), c.tie_share
    if max(c.sizes) >= R.MIN_PLANT:
        assert {"hub", "orphan", "alldead", "zero_dd"} <= set(c.plants)
        assert not (c.dst == c.plants["orphan"]).any() and not (c.src == c.plants["alldead"]).any()
        b = int(np.argmax(c.sizes))
        assert (c.dst == c.plants["hub"]).sum() >= 0.8 * (c.sizes[b] - 2)
        if c.form == "padded":
            dead = ~(c.edges > 0)
            assert np.isnan(c.dd[dead]).any() and (c.dd[dead] == 3.0).any()
            assert (c.nlist[dead] == np.nonzero(dead)[0]).all()
    rp, rb = R.references(c)
    dpos, S, B = R.emulate(c)
    if c.exact:
        R.check_grid_exact(c, rp)
        np.testing.assert_array_equal(dpos.astype(np.float64), rp.dpos)
    r = R.ratios(c, dpos, S, B, rp, rb)
    print(f"{name}: ties {c.tie_share:.4f} of {c.n_pairs}, largest |emulation - ref| / bound: dpos {r[0]:.3f} S {r[1]:.3f} B {r[2]:.3f}")
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("wrong", ["drop_incoming", "flip_incoming", "next_box"])
@pytest.mark.parametrize("family", ["grid", "float"])
def test_wrong_results_are_rejected(family, wrong):
    """a dropped incoming term, the sign of the incoming sum, frame g + 1's box used for frame g"""
    c = R.make_case(family, "csr", [85, 85, 85], [1, 1, 1], 2, 5)
    rp, rb = R.references(c)
    dpos, S, B = R.emulate(c, **{wrong: True})
    r = R.ratios(c, dpos, S, B, rp, rb)
    if c.exact:
        assert not np.array_equal(dpos.astype(np.float64), rp.dpos)
    assert r[0] > 1.0, r
    if wrong == "next_box":
        assert r[1] > 1.0 and r[2] > 1.0, r


def test_frame_paths():
    paths = R.frame_paths(np.cumsum([0] + R.BOX_PATTERNS["small40"]), 256)
    assert paths[0] == ("partial", 1) and paths[-1] == ("partial", 1) and paths[1:-1] == ["inside"] * 38
    assert R.frame_paths([0, 256], 256) == [("partial", 1)] and R.frame_paths([0, 257], 257) == [("partial", 2)]
    assert R.frame_paths([0, 700], 700) == [("partial", 3)]
    assert R.frame_paths([0, 100, 256, 306], 306) == [("partial", 1), ("partial", 1), ("partial", 1)]
    gp = np.cumsum([0] + R.BOX_PATTERNS["empties"])
    assert R.frame_paths(gp, 380) == ["empty", ("partial", 1), "empty", "empty", ("partial", 2), "inside", "empty", ("partial", 1),
                                      "empty"]
    assert R.frame_paths([0, 100], 100) == [("partial", 1)]
