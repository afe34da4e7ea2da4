"""tests/node_small_ref.py checked on the CPU: the statements that test_gpu_node_small.py holds the counter RNG, the Adam
update and the AMP attention kernels of csrc/node_ops.hip to.

Philox4x32-10 against the published known-answer vectors; the counter convention, u01 and the keep-mask; the moments of 2^20
reference normals from one fixed seed (5 sigma); the ratio c_host of a float32 host evaluation to the float64 reference, which
sets the GPU bound; adam_ref against the oracle's Adam; amp_ref / amp_bwd_ref against the oracle's AMPLayer with wv = I and
against central differences; the exact-family data of every GPU case inside the exact range."""
import numpy as np
import pytest

import node_small_ref as R
from oracle import nmrgnn_oracle as O

SEED, N_STAT = 20231, 1 << 20


# ------------------------------------------------------------------------------------------------- counter RNG
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,out", KAT, ids=["zero", "ones", "pi"])
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(w) for w in R.philox4x32_10(ctr, key)) == out
    got = R.philox4x32_10([np.full(3, c, np.uint64) for c in ctr], [np.full(3, k, np.uint64) for k in key])
    assert all((g == o).all() for g, o in zip(got, out))


def test_draw_words_convention():
    """element 4 q + k is word k of counter (lo, hi, 0, 0) = offset + q under key (lo, hi) = seed; the high counter word and
    the high key word are used; the low counter word carries into the high one"""
    seed, off = 0x9E3779B97F4A7C15, (1 << 32) - 3
    w = R.draw_words(seed, off, 24)
    assert w.shape == (24,) and w.dtype == np.uint64 and (w <= 0xFFFFFFFF).all()
    for q in (0, 2, 3, 5):                                       # q = 3 is the first counter past 2^32
        c = off + q
        one = R.philox4x32_10((c & 0xFFFFFFFF, c >> 32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
        assert [int(x) for x in one] == [int(x) for x in w[4 * q:4 * q + 4]]
    assert not np.array_equal(R.draw_words(seed, 7, 8), R.draw_words(seed, 7 + (1 << 32), 8))
    assert not np.array_equal(R.draw_words(77, 7, 8), R.draw_words(77 + (1 << 32), 7, 8))
    assert np.array_equal(R.draw_words(seed, 7, 8)[4:], R.draw_words(seed, 8, 4))
    assert np.array_equal(R.draw_words(seed, 7, 5), R.draw_words(seed, 7, 8)[:5])
    assert R.draw_words(seed, 7, 0).size == 0


def test_u01_edges():
    u = R.u01([0, 255, 256, 0xFFFFFFFF])
    assert u.tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    all24 = R.u01(np.arange(0, 1 << 32, 1 << 8, dtype=np.uint64)[:: 4099])
    assert np.array_equal(all24.astype(np.float32).astype(np.float64), all24) and all24.min() > 0 and all24.max() <= 1


@pytest.fixture(scope="module")
def normals():
    z, r = R.randn_ref(SEED, 0, N_STAT)
    return z, r


def test_normal_moments(normals):
    z, r = normals
    assert np.isfinite(z).all() and np.abs(z).max() <= R.Z_MAX and r.max() <= R.Z_MAX
    cols = z.reshape(-1, 4)
    nk = cols.shape[0]
    for k in range(4):
        assert abs(cols[:, k].mean()) <= 5 / np.sqrt(nk), k
        assert abs(cols[:, k].var() - 1.0) <= 5 * np.sqrt(2.0 / nk), k
        nxt = cols[:, (k + 1) % 4] if k < 3 else np.roll(cols[:, 0], -1)
        assert abs(np.mean(cols[:, k] * nxt)) <= 5 / np.sqrt(nk), k


def test_normal_tail_and_offsets():
    """an element's value depends on its counter and word only: a draw at offset + 1 is the draw at offset, four on"""
    z, r = R.randn_ref(SEED, 5, 13)
    z1, r1 = R.randn_ref(SEED, 6, 9)
    assert np.array_equal(z[4:], z1) and np.array_equal(r[4:], r1)
    assert np.array_equal(r[0:12:2], r[1:12:2])                                    # a pair shares its radius


def test_float32_host_ratio(normals):
    """c_host: the float32 host evaluation against the float64 reference in units of 2^-24 max(r, 2^-24).  The GPU bound is
    c = max(8, 4 c_host); the measured value is quoted in test_gpu_node_small.py and DESIGN.md 7.10."""
    z, r = normals
    ratio = R.randn_ratio(R.randn_f32(SEED, 0, N_STAT), z, r)
    c_host = float(ratio.max())
    print(f"c_host = {c_host:.3f}")
    assert 0.5 * R.C_HOST <= c_host <= R.C_HOST, c_host
    assert R.C_RANDN == max(8.0, 4.0 * R.C_HOST)


@pytest.mark.parametrize("keep", [0.5, 0.8, 1.0])
def test_keep_share(keep):
    m = R.dropout_ref(SEED, 1 << 40, keep, N_STAT)
    assert m.dtype == np.float32
    inv = np.float32(1) / np.float32(keep)
    assert np.isin(m, [np.float32(0), inv]).all()
    share = float((m != 0).mean())
    assert abs(share - keep) <= 5 * np.sqrt(keep * (1 - keep) / N_STAT)
    if keep == 1.0:
        assert (m == 1).all()


def test_keep_boundary_is_inclusive():
    w = R.draw_words(SEED, 3, 64)
    keep = np.float32(R.u01(w[17]))
    m = R.dropout_ref(SEED, 3, keep, 64)
    assert m[17] != 0 and np.array_equal(m != 0, R.u01(w) <= float(keep))


# ------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
@pytest.mark.parametrize("b1,b2", [(0.9, 0.999), (0.5, 0.75), (0.0, 0.999)])
def test_adam_ref_equals_oracle(b1, b2, step):
    rng = np.random.default_rng(step)
    n = 500
    p, g = R.f32(rng.standard_normal(n)), R.f32(rng.standard_normal(n))
    m, v = R.f32(0.1 * rng.standard_normal(n)), R.f32((0.1 * rng.standard_normal(n)) ** 2)
    for gscale in (1.0, 3.7):
        pn, mn, vn, mag = R.adam_ref(p, g, m, v, 1e-3, b1, b2, 1e-7, step, gscale)
        f = lambda x: float(np.float32(x))                       # the entry point takes float32 arguments
        po, mo, vo = O.adam_step(p, g * f(gscale), m, v, step, lr=f(1e-3), b1=f(b1), b2=f(b2), eps=f(1e-7))
        for name, a, b in (("p", pn, po), ("m", mn, mo), ("v", vn, vo)):
            assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), name
        assert (mag["m1"] + mag["m2"] >= np.abs(mn) * (1 - 1e-12)).all() and (mag["upd"] >= np.abs(pn - p) * (1 - 1e-9)).all()
    lr_t, omb1, omb2 = R.adam_constants(2.0 ** -6, 0.5, 0.75, 1)
    assert (lr_t, omb1, omb2) == (2.0 ** -6, 0.5, 0.25)
    assert R.adam_constants(1e-3, 0.9, 0.999, 10 ** 6)[0] == float(np.float32(1e-3))


def test_adam_ref_zero_element():
    pn, mn, vn, mag = R.adam_ref([1.5], [0.0], [0.0], [0.0], 1e-3, 0.9, 0.999, 1e-7, 3, 1.0)
    assert pn[0] == 1.5 and mn[0] == 0 and vn[0] == 0 and mag["upd"][0] == 0


# ------------------------------------------------------------------------------------------------- AMP attention
@pytest.mark.parametrize("c", [(7, 3, 4, 6, "random"), (9, 5, 2, 8, "hub"), (6, 1, 3, 5, "random"), (8, 4, 5, 3, "dup"),
                               (5, 6, 2, 4, "self")], ids=R.amp_id)
def test_amp_ref_equals_oracle(c):
    N, K, E, F, pattern = c
    rng = R.amp_rng(c, 0)
    d = R.amp_normal_data(rng, N, K, F, E, R.amp_nlist(rng, N, K, pattern), scale=2.0)
    args = (d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"])
    agg, b, fm = R.amp_ref(*args)
    ref = O.amp_layer_forward(*args, np.eye(F), None)
    assert np.abs(agg - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.allclose(b.sum(1), 1.0, rtol=0, atol=1e-14) and np.allclose(b[N // 3], 1.0 / K)       # inv = 0: uniform
    assert (fm["agg"] >= np.abs(agg) * (1 - 1e-12)).all()
    got, mag, L = R.amp_bwd_ref(*args, d["dagg"])
    ob = O.amp_layer_backward(*args, np.eye(F), None, d["dagg"])
    for k, name in (("dh", "nodes"), ("de", "edges"), ("dwq", "wq"), ("dwk", "wk")):
        assert np.abs(got[k] - ob[name]).max() <= 1e-12 * max(1.0, np.abs(ob[name]).max()), k
        assert (mag[k] >= np.abs(got[k]) * (1 - 1e-12)).all(), k
    s = d["inv"][:, None] * np.einsum("ijn,in->ij", d["e"], (d["h"] @ d["wq"]) @ d["wk"].T)
    assert (L >= np.abs(s).max(1) * (1 - 1e-12)).all()
    ls = R.row_logit_scale(d["nlist"], L)
    assert (ls["dh"][:, 0] >= L).all() and ls["dwq"] == L.max()


def test_amp_de_equals_central_differences():
    c = (5, 3, 4, 6, "random")
    N, K, E, F, pattern = c
    rng = R.amp_rng(c, 1)
    d = R.amp_normal_data(rng, N, K, F, E, R.amp_nlist(rng, N, K, pattern), scale=1.5, zero_inv_row=False)
    got, _, _ = R.amp_bwd_ref(d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"], d["dagg"])

    def loss(e_):
        return float(np.sum(d["dagg"] * R.amp_ref(d["h"], d["nlist"], e_, d["inv"], d["wq"], d["wk"])[0]))

    eps, num = 1e-6, np.zeros((N, K, E))
    for idx in np.ndindex(N, K, E):
        ep, em = d["e"].copy(), d["e"].copy()
        ep[idx] += eps
        em[idx] -= eps
        num[idx] = (loss(ep) - loss(em)) / (2 * eps)
    assert np.abs(num - got["de"]).max() <= 1e-8 * max(1.0, np.abs(got["de"]).max())


def test_amp_incoming_lists():
    nl = np.array([[2, 0], [2, 2], [0, 1]], np.int32)
    in_ptr, in_slot = R.incoming_lists(nl, 3)
    assert in_ptr.tolist() == [0, 2, 3, 6] and in_slot.tolist() == [1, 4, 5, 0, 2, 3]
    in_ptr, _ = R.incoming_lists(R.amp_nlist(None, 4, 3, "hub"), 4)
    assert in_ptr.tolist() == [0, 12, 12, 12, 12]


@pytest.mark.parametrize("setting", ["wq0", "wk0"])
@pytest.mark.parametrize("c", R.AMP_EXACT_CASES, ids=R.amp_id)
def test_amp_exact_family_in_range(c, setting):
    """the data test_gpu_node_small.py uses: all logits 0, every output below 2^24 units of its grid, and float64 itself
    exact in float32"""
    N, K, E, F, pattern = c
    rng = R.amp_rng(c, 2 + (setting == "wk0"))
    d = R.amp_exact_data(rng, N, K, F, E, R.amp_nlist(rng, N, K, pattern), setting)
    for name, units in R.amp_exact_in_range(d, K).items():
        assert units < 2.0 ** 24, (name, units)
    agg, b, _ = R.amp_ref(d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"])
    ref, _, _ = R.amp_bwd_ref(d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"], d["dagg"])
    assert (b == 1.0 / K).all() and not ref["de"].any()
    assert not ref["dwk" if setting == "wq0" else "dwq"].any()
    for k, v in dict(ref, agg=agg).items():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), k
    if K > 1 and N > 1 and pattern in ("random", "dup"):      # hub and self-loop rows: equal db in every slot, ds = 0
        assert ref["dwq" if setting == "wq0" else "dwk"].any() and ref["dh"].any() and agg.any()


@pytest.mark.parametrize("span", [80.0, 1e4])
def test_amp_wide_data_saturates(span):
    c = R.AMP_WIDE_CASES[2]
    N, K, E, F, pattern = c
    rng = R.amp_rng(c, 4)
    d = R.amp_widen(R.amp_normal_data(rng, N, K, F, E, R.amp_nlist(rng, N, K, pattern)), span)
    agg, b, fm = R.amp_ref(d["h"], d["nlist"], d["e"], d["inv"], d["wq"], d["wk"])
    assert np.isfinite(agg).all() and 0.5 * span <= fm["L"].max() and (b.max(axis=1) > 0.99).any()
    if span > 1e3:
        assert (b == 0).any() and (b.max(axis=1) > 0.999).mean() > 0.8
